"""The scenario-grid scorer measured -> profiles/score_grid_timing.jsonl and profiles/score_grid_findings.jsonl.

    python tools/exp_score_grid.py timing   [--runs 7] [--timeout 300]
    python tools/exp_score_grid.py findings [--envs 4096] [--timeout 300]

`timing`: one `ops.score_grid` call over S scenarios against S `ops.score` calls on identical arguments (the parent's code, which the grid does not touch), float32,
the published tables (tests/golden/assets), level 4, simulation flavour, one episode per env, 4 096 envs per set: S in {1, 8, 32} platform speeds x {1, 16} table
sets.  The two alternate in one child process per shape: one warm-up, then the median of 7 runs with the smallest and largest, kernel time (HIP events around the
launch; for the S calls their sum) beside the wall clock of the calls.  `by_code` and `steps_sum` of the two must be equal in every run.

`findings`: the published tables on a grid of 20 scenarios per flavour — platform speed mp_t_x in {0.4, 0.8, 1.2, 1.6, 2.0} x observation noise {none, as launched}
x trajectory {rectilinear, eight} — 4 096 envs x 1 episode, one launch per flavour.  Recorded per scenario: its label, `by_code`, the rate of the flavour's good
outcome (touchdown / goal hold), `touch_hist` and `evaluation.robustness_table`'s columns; per flavour the worst scenario.

Every GPU step runs in a child process of its own under `--timeout` seconds; a child that fails or runs out of time ends the tool."""
import argparse
import dataclasses
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
LEVEL, SEED, MAX_STEPS, ENVS = 4, 123, 600, 4096
SHAPES = tuple((S, K) for K in (1, 16) for S in (1, 8, 32))
FLAVOURS = ("simulation", "training")
SPEEDS = (0.4, 0.8, 1.2, 1.6, 2.0)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def reference_tables():
    assets = ROOT / "tests" / "golden" / "assets"
    return tuple(np.load(assets / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))


def timing_child(a):
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import F32, Q_PAPER, scenario_grid
    qa, qb = reference_tables()
    sets3 = [(qa, qb), (np.zeros_like(qa), np.zeros_like(qb)), (qa, -qb)]
    S, K, n = a.scenarios, a.sets, a.envs
    QA = np.stack([sets3[k % 3][0] for k in range(K)]); QB = np.stack([sets3[k % 3][1] for k in range(K)])
    base = evaluation._flavour_config("simulation", LEVEL, F32, {"quirks": Q_PAPER})
    cfgs, labels = scenario_grid(base, mp_t_x=[1.6] if S == 1 else [float(x) for x in np.linspace(0.4, 2.0, S)])

    def grid(t):
        r = ops.score_grid(cfgs, QA, QB, n, SEED, episodes=1, max_steps=MAX_STEPS, touch=False, timing=t)
        return r["by_code"], r["steps_sum"]

    def calls(t):
        t["kernel_ms"], bc, ss = 0.0, [], []
        for c in cfgs:
            ti = {}
            r = ops.score(c, QA, QB, n, SEED, episodes=1, max_steps=MAX_STEPS, timing=ti)
            t["kernel_ms"] += ti["kernel_ms"]; t["instance"] = ti["instance"]
            bc.append(r["by_code"]); ss.append(r["steps_sum"])
        return np.stack(bc), np.stack(ss)

    fns = {"score_grid_one_call": grid, "score_S_calls": calls}
    wall = {k: [] for k in fns}; kern = {k: [] for k in fns}; inst = {}
    for run in range(a.runs + 1):  # run 0 warms both kernels up
        res = {}
        for name, fn in fns.items():
            t = {}
            t0 = time.perf_counter()
            res[name] = fn(t)
            w = (time.perf_counter() - t0) * 1e3
            inst[name] = t["instance"]
            if run:
                wall[name].append(w); kern[name].append(t["kernel_ms"])
        assert np.array_equal(res["score_grid_one_call"][0], res["score_S_calls"][0]) and np.array_equal(res["score_grid_one_call"][1], res["score_S_calls"][1]), f"run {run}"
    shape = {"scenarios": S, "table_sets": K, "envs_per_table": n, "episodes_per_env": 1, "level": LEVEL, "seed": SEED, "dtype": "float32", "max_steps": MAX_STEPS,
             "waves_per_launch": {"score_grid_one_call": S * K * n // 64, "score_S_calls": K * n // 64}}
    for name in fns:
        print(json.dumps(dict(shape, what="grid_vs_score_calls", method=name, instance=inst[name], kernel_ms=spread(kern[name]), wall_ms=spread(wall[name]))), flush=True)
    kg, ks = statistics.median(kern["score_grid_one_call"]), statistics.median(kern["score_S_calls"])
    print(json.dumps(dict(shape, what="grid_over_score_calls", kernel_ratio=kg / ks, kernel_ms_difference=kg - ks, score_calls_min_max_spread_ms=max(kern["score_S_calls"]) - min(kern["score_S_calls"]),
                          wall_ratio=statistics.median(wall["score_grid_one_call"]) / statistics.median(wall["score_S_calls"]), by_code_equal_in_every_run=True)), flush=True)


def findings_child(a):
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import AS_LAUNCHED, F32, Q_PAPER, TRAJ_EIGHT, TRAJ_RPM
    qa, qb = reference_tables()
    base = evaluation._flavour_config(a.flavour, LEVEL, F32, {"quirks": Q_PAPER})
    good = "TERMINAL_CONTACT" if a.flavour == "simulation" else "TERMINAL_SUCCESS"
    noises = (("none", dict(noise_pos_sd=0.0, noise_vel_sd=0.0)), ("as_launched", {k: AS_LAUNCHED[k] for k in ("noise_pos_sd", "noise_vel_sd")}))
    cfgs, labels = [], []
    for speed in SPEEDS:
        for noise, nkw in noises:
            for traj, tname in ((TRAJ_RPM, "rectilinear"), (TRAJ_EIGHT, "eight")):
                cfgs.append(dataclasses.replace(base, mp_t_x=speed, trajectory=traj, **nkw)); labels.append({"mp_t_x": speed, "noise": noise, "trajectory": tname})
    t = {}
    r = ops.score_grid(cfgs, qa, qb, a.envs, SEED, episodes=1, max_steps=MAX_STEPS, timing=t)
    tab = evaluation.robustness_table(r, labels, column=good)
    head = {"flavour": a.flavour, "level": LEVEL, "envs": a.envs, "episodes_per_env": 1, "seed": SEED, "max_steps": MAX_STEPS, "dtype": "float32", "tables": "tests/golden/assets"}
    num = lambda x: None if x is None or np.isnan(x) else float(x)
    for s, lab in enumerate(labels):
        print(json.dumps(dict(head, what="grid_scenario", scenario=s, label=lab, by_code=dict(zip(r["columns"], r["by_code"][s, 0].tolist())), rate_of=good, rate=float(tab["rate"][s, 0]),
                              mean_steps=num(tab["mean_steps"][s, 0]), unfinished=float(tab["unfinished"][s, 0]), touch_hist=r["touch_hist"][s, 0].tolist(),
                              touch_centre=num(tab["touch_centre"][s, 0]), touch_outside=num(tab["touch_outside"][s, 0]))), flush=True)
    print(json.dumps(dict(head, what="grid_summary", scenarios=len(cfgs), kernel_ms=t["kernel_ms"], instance=t["instance"], rate_of=good, worst_scenario=int(tab["worst_scenario"][0]),
                          worst_label=tab["worst_label"][0], worst_rate=float(tab["worst_rate"][0]), best_rate=float(tab["rate"][:, 0].max()),
                          note="the trajectory axis moves the platform on the figure eight of fixed radius 3 m and speed 0.8 m/s: mp_t_x does not act on it")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "findings"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--envs", type=int, default=ENVS)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--flavour", default="simulation", help=argparse.SUPPRESS)
    ap.add_argument("--scenarios", type=int, default=8, help=argparse.SUPPRESS)
    ap.add_argument("--sets", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return timing_child(a) if a.what == "timing" else findings_child(a)
    import __graft_entry__ as g
    g.build_hip()
    me = [sys.executable, str(Path(__file__).resolve()), a.what, "--child", "--envs", str(a.envs)]
    if a.what == "timing":
        jobs = [me + ["--scenarios", str(S), "--sets", str(K), "--runs", str(a.runs)] for S, K in SHAPES]
    else:
        jobs = [me + ["--flavour", fl] for fl in FLAVOURS]
    out = Path(a.out or ROOT / "profiles" / ("score_grid_timing.jsonl" if a.what == "timing" else "score_grid_findings.jsonl"))
    lines = []
    for cmd in jobs:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)  # a time-out or a failure ends the tool: nothing more is started on the GPU
        if r.returncode != 0:
            sys.exit(f"{' '.join(cmd[2:])} failed with status {r.returncode}:\n{r.stderr[-4000:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln); print(ln, flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
