"""The split transition-model operator measured -> profiles/split_model_timing.jsonl and profiles/split_model_table.jsonl.

    python tools/exp_split_model.py timing [--runs 7] [--timeout 300]
    python tools/exp_split_model.py table  [--envs 262144] [--episodes 8] [--seeds 2] [--timeout 900]

`timing`: k_model_split (feature pitch_sp, cut 0: both halves in use) against k_model on identical arguments — the same flights — for 1 table set x 4 096 and
1 x 65 536 envs, float32, level 4, simulation flavour, eps 0.1, one episode per env.  The two kernels alternate in one process: one warm-up, then the median of
7 runs with min and max; kernel time (HIP events around the launch) beside the wall clock of the call, which includes the copy of the pair tables (10.7 MB and
21.4 MB per set).  The halves summed must equal the model.

`table`: the table the operator exists for, on the reference's stage-4 tables (tests/golden/assets): scripts/simulation.py's `evaluate_split` for every feature
at eps 0.1 and eps 1.0 at section 19's sample size (262 144 envs x 8 episodes), `--seeds` seeds summed (with two, the odd seed's coin is also held against the
even seed's), one line per feature and eps.

Every GPU step runs in a child process of its own under `--timeout` seconds; a child that fails or runs out of time ends the tool."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
LEVEL, SEED, MAX_STEPS, EPS = 4, 123, 600, 0.1
SHAPES = ((1, 4096), (1, 65536))
ASSETS = ROOT / "tests" / "golden" / "assets"


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timing_child(a):
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import F32, Q_PAPER
    qa, qb = (np.load(ASSETS / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
    n = a.envs
    cfg = evaluation._flavour_config("simulation", LEVEL, F32, {"quirks": Q_PAPER})
    calls = {"k_model": lambda t: ops.transition_model(cfg, qa, qb, n, SEED, EPS, episodes=1, max_steps=MAX_STEPS, timing=t),
             "k_model_split": lambda t: ops.split_model(cfg, qa, qb, n, SEED, EPS, "pitch_sp", 0.0, episodes=1, max_steps=MAX_STEPS, timing=t)}
    wall = {k: [] for k in calls}; kern = {k: [] for k in calls}; res = {}
    for run in range(a.runs + 1):  # run 0 warms both kernels up
        for name, fn in calls.items():
            t = {}
            t0 = time.perf_counter()
            res[name] = fn(t)
            w = (time.perf_counter() - t0) * 1e3
            if run:
                wall[name].append(w); kern[name].append(t["kernel_ms"])
    m, s = res["k_model"], res["k_model_split"]
    for f in ("pairs", "reward_fx", "terminal"):
        assert np.array_equal(s[f].astype(np.int64).sum(axis=1), m[f].astype(np.int64)), f
    assert np.array_equal(s["by_code"], m["by_code"]) and (s["visits"][:, 0].sum() > 0) and (s["visits"][:, 1].sum() > 0)
    for name in calls:
        print(json.dumps({"what": "model_split_vs_model", "kernel": name, "flavour": "simulation", "table_sets": 1, "envs_per_table": n, "episodes_per_env": 1, "level": LEVEL, "seed": SEED,
                          "eps": EPS, "dtype": "float32", "max_steps": MAX_STEPS, "kernel_ms": spread(kern[name]), "wall_ms": spread(wall[name])}), flush=True)
    km, ks = statistics.median(kern["k_model"]), statistics.median(kern["k_model_split"])
    print(json.dumps({"what": "model_split_over_model", "envs_per_table": n, "kernel_ratio": ks / km, "kernel_ms_difference": ks - km,
                      "k_model_min_max_spread_ms": max(kern["k_model"]) - min(kern["k_model"]), "wall_ratio": statistics.median(wall["k_model_split"]) / statistics.median(wall["k_model"]),
                      "decisions": int(m["visits"].sum()), "half1_share": float(s["visits"][:, 1].sum() / s["visits"].sum())}), flush=True)


def table_child(a):
    import simulation
    from dql_multirotor_landing_amd import ops
    from dql_multirotor_landing_amd.config import Q_PAPER
    names = [f for f in ops.SPLIT_FEATURES if f != "coin"]
    t0 = time.perf_counter()
    m, table = simulation.evaluate_split(str(ASSETS), names, a.envs, LEVEL, flavour="simulation", episodes=a.episodes, eps=a.eps, n_seeds=a.seeds, quirks=Q_PAPER)
    base = {"what": "aliasing_table", "flavour": "simulation", "level": LEVEL, "envs": a.envs, "episodes_per_env": a.episodes, "seeds": m["seeds"].tolist(), "eps": a.eps,
            "max_steps": MAX_STEPS, "dtype": "float32", "tables": "tests/golden/assets", "min_visits": 30, "decisions": int(m["pairs_coin"].sum() + m["terminal_coin"].sum())}
    for name, row in table.items():
        print(json.dumps(dict(base, feature=name, **row)), flush=True)
    print(json.dumps(dict(base, what="aliasing_table_wall", seconds=time.perf_counter() - t0, launches=(2 * len(names) + 1) * a.seeds)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "table"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--envs", type=int, default=262144)
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=None, help="seconds a child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--eps", type=float, default=EPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return timing_child(a) if a.what == "timing" else table_child(a)
    import __graft_entry__ as g
    g.build_hip()
    timeout = a.timeout or (300 if a.what == "timing" else 900)
    me = [sys.executable, str(Path(__file__).resolve()), a.what, "--child"]
    if a.what == "timing":
        jobs = [me + ["--envs", str(n), "--runs", str(a.runs)] for _, n in SHAPES]
    else:
        jobs = [me + ["--envs", str(a.envs), "--episodes", str(a.episodes), "--seeds", str(a.seeds), "--eps", str(eps)] for eps in (0.1, 1.0)]
    out = Path(a.out or ROOT / "profiles" / ("split_model_timing.jsonl" if a.what == "timing" else "split_model_table.jsonl"))
    lines = []
    for cmd in jobs:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)  # a time-out or a failure ends the tool: nothing more is started on the GPU
        if r.returncode != 0:
            sys.exit(f"{' '.join(cmd[2:])} failed with status {r.returncode}:\n{r.stderr[-4000:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln); print(ln, flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
