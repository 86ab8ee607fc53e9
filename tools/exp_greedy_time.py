#!/usr/bin/env python3
"""Device time of one call of each greedy-flight operator, one library against another (DESIGN.md sections 15 and 28).

    python tools/exp_greedy_time.py one                       # this process, the library _lib loads (DQL_LIB_PATH): one JSON line, ms per call
    python tools/exp_greedy_time.py one --small               # the wall time of a small call instead, us per call
    python tools/exp_greedy_time.py ab --parent PARENT.so [--raw OUT.jsonl]           # parent and branch alternating, P1 B1 P2 B2 P3 B3, one process each
    python tools/exp_greedy_time.py ab --parent PARENT.so --small [--raw OUT.jsonl]   # the same for the small call

What is timed: `kernel_ms` (HIP events around the launch; the returns: `fly_ms` and `sweep_ms`) of ops.score, ops.score_map, ops.transition_model,
ops.returns_map and ops.score_grid in the shape of the committed timing profiles (profiles/model_timing.jsonl, returns_timing.jsonl, score_grid_timing.jsonl):
16 table sets x 4 096 envs (the grid: 8 scenarios x 1 set x 4 096), 1 episode, max_steps 600, the simulation flavour at level 4, the reference tables those
tools use, eps 0, gamma 0.99, float32 and float64.  --small: the wall time of a call of 1 set x 64 envs (the grid: 2 scenarios), max_steps 8.  Median of 31
calls after 5 warm-up calls.

`ab` starts one child process per run, one at a time, each under --timeout seconds, and stops at the first child that does not exit 0.  Bound of a row:
|branch median - parent mean| <= the parent's max - min, or 2 % of its mean if that is larger."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
LEVEL, SEED, GAMMA, WARMUP, CALLS = 4, 123, 0.99, 5, 31
SHAPE = dict(sets=16, envs=4096, scenarios=8, max_steps=600)
SMALL = dict(sets=1, envs=64, scenarios=2, max_steps=8)


def tables(K):
    assets = ROOT / "tests" / "golden" / "assets"
    qa, qb = (np.load(assets / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
    sets3 = [(qa, qb), (np.zeros_like(qa), np.zeros_like(qb)), (qa, -qb)]
    return np.stack([sets3[k % 3][0] for k in range(K)]), np.stack([sets3[k % 3][1] for k in range(K)])


def one(small):
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import F32, F64, Q_PAPER, scenario_grid
    sh = SMALL if small else SHAPE
    K, n, S, steps = sh["sets"], sh["envs"], sh["scenarios"], sh["max_steps"]
    QA, QB = tables(K)
    out = {}
    for dtype, name in ((F32, "float32"), (F64, "float64")):
        cfg = evaluation._flavour_config("simulation", LEVEL, dtype, {"quirks": Q_PAPER})
        cfgs, _ = scenario_grid(cfg, mp_t_x=[float(x) for x in np.linspace(0.4, 2.0, S)])
        kw = dict(episodes=1, max_steps=steps)
        calls = {"k_score": lambda t: ops.score(cfg, QA, QB, n, SEED, timing=t, **kw),
                 "k_score_map": lambda t: ops.score_map(cfg, QA, QB, n, SEED, timing=t, **kw),
                 "k_model": lambda t: ops.transition_model(cfg, QA, QB, n, SEED, 0.0, timing=t, **kw),
                 "k_returns": lambda t: ops.returns_map(cfg, QA, QB, n, SEED, 0.0, GAMMA, timing=t, **kw),
                 "k_score_grid": lambda t: ops.score_grid(cfgs, QA[:1], QB[:1], n, SEED, touch=True, timing=t, **kw)}
        for op, fn in calls.items():
            wall, dev, dev2 = [], [], []
            for _ in range(WARMUP + CALLS):
                t = {}
                t0 = time.perf_counter()
                fn(t)
                wall.append(time.perf_counter() - t0)
                dev.append(t["fly_ms"] if op == "k_returns" else t["kernel_ms"])
                dev2.append(t.get("sweep_ms", 0.0))
            if small:
                out[f"{op} {name}"] = round(statistics.median(wall[WARMUP:]) * 1e6, 1)
            elif op == "k_returns":
                out[f"k_returns_fly {name}"] = round(statistics.median(dev[WARMUP:]), 4)
                out[f"k_returns_sweep {name}"] = round(statistics.median(dev2[WARMUP:]), 4)
            else:
                out[f"{op} {name}"] = round(statistics.median(dev[WARMUP:]), 4)
    return out


def ab(parent, small, raw, timeout):
    runs = {"P": [], "B": []}
    for i in range(3):
        for who, lib in (("P", parent), ("B", None)):
            env = dict(os.environ)
            if lib:
                env["DQL_LIB_PATH"] = str(Path(lib).resolve())
            else:
                env.pop("DQL_LIB_PATH", None)
            cmd = [sys.executable, __file__, "one"] + (["--small"] if small else [])
            try:
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
            except subprocess.TimeoutExpired:
                sys.exit(f"{who}{i + 1} ran out of its {timeout} s: nothing more is started")
            if r.returncode != 0:
                sys.exit(f"{who}{i + 1} failed with status {r.returncode}: nothing more is started\n{r.stderr[-4000:]}")
            runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
            if raw:
                with open(raw, "a") as f:
                    f.write(json.dumps({"what": "small_call_wall_us" if small else "device_ms", "who": who, "run": i + 1, "values": runs[who][-1]}) + "\n")
    print("| operator | parent P1, P2, P3 | branch B1, B2, B3 | parent median | branch median | spread | branch median − parent mean | within |\n|---|---|---|---|---|---|---|---|")
    for row in runs["P"][0]:
        p, b = [r[row] for r in runs["P"]], [r[row] for r in runs["B"]]
        mean = statistics.mean(p)
        spread, diff = max(max(p) - min(p), 0.02 * mean), statistics.median(b) - mean
        print(f"| `{row}` | {', '.join(map(str, p))} | {', '.join(map(str, b))} | {statistics.median(p)} | {statistics.median(b)} | {spread:.4g} | {diff:+.4g} | "
              f"{'yes' if abs(diff) <= spread else 'NO'} |", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("one", "ab"))
    ap.add_argument("--parent", help="the parent's libdql_hip.so (ab)")
    ap.add_argument("--small", action="store_true", help="the wall time of a small call instead of the device time of the profiles' shape")
    ap.add_argument("--raw", help="append each process's JSON line to this file (ab)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child process may take (ab)")
    a = ap.parse_args()
    if a.what == "one":
        print(json.dumps(one(a.small)), flush=True)
    else:
        if not a.parent:
            ap.error("ab needs --parent")
        ab(a.parent, a.small, a.raw, a.timeout)


if __name__ == "__main__":
    main()
