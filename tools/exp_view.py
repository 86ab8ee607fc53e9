"""Device-resident step outputs measured -> profiles/view_timing.jsonl.

    python tools/exp_view.py timing [--runs 7] [--periods 200] [--timeout 300]

Float32 contexts, DqlConfig defaults, at 4 096, 131 072 and 1 048 576 envs; each shape in a child process of its own.  Three loops alternate in one process,
all on the same fixed random actions:
  step_dev            dql_step_dev alone (actions in device memory)
  step_dev+view_dev   dql_step_dev + dql_view_dev with every output, float32, into device buffers
  step+step_outputs   dql_step with host actions + dql_step_outputs (the host path: pinned gather, wait, host loop over n_envs)
One warm-up, then the median of `runs` runs of `periods` periods with smallest and largest: device time between two HIP events on the context's stream around
work that ends in a synchronise, and the wall clock beside it.  k_env_view's own time comes from an event pair around single launches (median of 50; an event
pair around one small kernel includes the events' own cost).  The tool is torch-free: device memory comes from the HIP runtime the library runs on.

A child that fails or runs out of time ends the tool."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SHAPES = (4096, 131072, 1048576)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timing_child(a):
    from dql_multirotor_landing_amd import _lib
    from dql_multirotor_landing_amd.config import DqlConfig, F32
    from dql_multirotor_landing_amd.engine import Engine
    n, P = a.envs, a.periods
    eng = Engine(DqlConfig(dtype=F32), n, seed=7)
    hip = C.CDLL(str(_lib.LIB_PATH))
    stream = C.c_void_p(eng.stream_handle())

    def ok(rc):
        assert rc == 0, f"HIP error {rc}"

    def alloc(nbytes):
        p = C.c_void_p()
        ok(hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)))
        return p.value

    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(e0))); ok(hip.hipEventCreate(C.byref(e1)))

    def timed(work):
        """(device ms between the two events, wall ms) of `work`, which the second event's synchronise ends"""
        eng.sync()
        t0 = time.perf_counter()
        ok(hip.hipEventRecord(e0, stream))
        work()
        ok(hip.hipEventRecord(e1, stream))
        ok(hip.hipEventSynchronize(e1))
        wall = (time.perf_counter() - t0) * 1e3
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        return ms.value, wall

    act = np.random.default_rng(0).integers(0, 3, n).astype(np.uint8)
    d_act = alloc(n)
    ok(hip.hipMemcpy(C.c_void_p(d_act), act.ctypes.data_as(C.c_void_p), C.c_size_t(n), 1))
    sizes = {"obs": 32 * n, "reward": 4 * n, "cumulative_reward": 4 * n, "idx_x": 4 * n, "idx_y": 4 * n, "step_count": 4 * n, "done": n, "was_reset": n, "code": n, "bad_actions": 8}
    view = {k: alloc(b) for k, b in sizes.items()}

    def loop_step_dev():
        for _ in range(P):
            eng.step_dev(d_act)

    def loop_view():
        for _ in range(P):
            eng.step_dev(d_act)
            eng.view_dev(real_dtype=F32, **view)

    def loop_host():
        for _ in range(P):
            eng.step_raw(act)
            eng.step_outputs_view()

    loops = {"step_dev": loop_step_dev, "step_dev+view_dev": loop_view, "step+step_outputs": loop_host}
    dev_ms = {k: [] for k in loops}; wall_ms = {k: [] for k in loops}
    for run in range(a.runs + 1):  # run 0 warms up
        for name, fn in loops.items():
            ms, wall = timed(fn)
            if run:
                dev_ms[name].append(ms / P * 1e3); wall_ms[name].append(wall / P * 1e3)
    single = [timed(lambda: eng.view_dev(real_dtype=F32, **view))[0] * 1e3 for _ in range(51)][1:]
    read_b = 80 * n  # the int4 word and four quads per env at most (the compiler loads the components it needs)
    write_b = sum(sizes.values())
    base = {"what": "view_timing", "envs": n, "dtype": "float32", "real_dtype": "float32", "periods": P, "unit": "us per period", "instance": eng.step_instance()}
    for name in loops:
        print(json.dumps(dict(base, loop=name, device_us=spread(dev_ms[name]), wall_us=spread(wall_ms[name]))), flush=True)
    m = {k: statistics.median(v) for k, v in dev_ms.items()}
    w = {k: statistics.median(v) for k, v in wall_ms.items()}
    kv = statistics.median(single)
    print(json.dumps(dict(base, what="view_summary", k_env_view_event_pair_us=spread(single), view_bytes_read_at_most=read_b, view_bytes_written=write_b,
                          view_added_device_us=m["step_dev+view_dev"] - m["step_dev"], view_added_over_step=(m["step_dev+view_dev"] - m["step_dev"]) / m["step_dev"],
                          host_path_over_device_path_wall=w["step+step_outputs"] / w["step_dev+view_dev"],
                          view_gb_per_s_from_event_pair=(read_b + write_b) / (kv * 1e-6) / 1e9)), flush=True)
    eng.sync()
    for p in [d_act, *view.values()]:
        hip.hipFree(C.c_void_p(p))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--periods", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--envs", type=int, default=4096, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return timing_child(a)
    import __graft_entry__ as g
    g.build_hip()
    me = [sys.executable, str(Path(__file__).resolve()), "timing", "--child", "--runs", str(a.runs), "--periods", str(a.periods)]
    out = Path(a.out or ROOT / "profiles" / "view_timing.jsonl")
    lines = []
    for n in SHAPES:
        r = subprocess.run(me + ["--envs", str(n)], capture_output=True, text=True, timeout=a.timeout)  # a time-out or a failure ends the tool: nothing more is started on the GPU
        if r.returncode != 0:
            sys.exit(f"envs {n} failed with status {r.returncode}:\n{r.stderr[-4000:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln); print(ln, flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
