"""What the map costs on top of scoring -> profiles/score_map_timing.jsonl.

k_score against k_score_map on 4 096 table sets x 256 envs each, float32, both flavours, the published tables repeated (with the all-zero set and the set with
Q_table_b negated, so that not every wave flies the same policy), one episode per env, `log` off.  The two kernels alternate in one process: one warm-up, then
the median of 7 runs with min and max.  Kernel time (HIP events around the launch) is recorded beside the wall clock of the call, which for the map includes
the copy of the 93 MB map to the host.  The outputs the two calls share must be equal.

python tools/exp_score_map.py [--out profiles/score_map_timing.jsonl] [--runs 7] [--table-sets 4096]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
N_ENVS, LEVEL, SEED = 256, 4, 123


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "score_map_timing.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--table-sets", type=int, default=4096)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import F32, Q_PAPER
    assets = ROOT / "tests" / "golden" / "assets"
    qa, qb = (np.load(assets / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
    sets3 = [(qa, qb), (np.zeros_like(qa), np.zeros_like(qb)), (qa, -qb)]
    K = a.table_sets
    QA = np.stack([sets3[k % 3][0] for k in range(K)]); QB = np.stack([sets3[k % 3][1] for k in range(K)])
    lines = []
    for flavour in ("simulation", "training"):
        cfg = evaluation._flavour_config(flavour, LEVEL, F32, {"quirks": Q_PAPER})
        calls = {"k_score": ops.score, "k_score_map": ops.score_map}
        wall = {k: [] for k in calls}; kern = {k: [] for k in calls}; res = {}
        for run in range(a.runs + 1):  # run 0 warms both kernels up
            for name, fn in calls.items():
                t = {}
                t0 = time.perf_counter()
                res[name] = fn(cfg, QA, QB, N_ENVS, SEED, episodes=1, max_steps=600, timing=t)
                w = (time.perf_counter() - t0) * 1e3
                if run:
                    wall[name].append(w); kern[name].append(t["kernel_ms"])
        assert np.array_equal(res["k_score"]["by_code"], res["k_score_map"]["by_code"]) and np.array_equal(res["k_score"]["steps_sum"], res["k_score_map"]["steps_sum"])
        visits = res["k_score_map"]["visits"]
        for name in calls:
            lines.append({"what": "score_vs_score_map", "kernel": name, "flavour": flavour, "table_sets": K, "envs_per_table": N_ENVS, "episodes_per_env": 1, "level": LEVEL,
                          "seed": SEED, "dtype": "float32", "log": False, "kernel_ms": spread(kern[name]), "wall_ms": spread(wall[name]),
                          "wall_minus_kernel_ms": statistics.median(wall[name]) - statistics.median(kern[name]),
                          "touchdown_rate_first3": ops.rates_from_counts(res[name]["by_code"][:3], "TERMINAL_CONTACT").tolist()})
        ks, km = statistics.median(kern["k_score"]), statistics.median(kern["k_score_map"])
        lines.append({"what": "score_map_over_score", "flavour": flavour, "kernel_ratio": km / ks, "kernel_ms_difference": km - ks,
                      "k_score_min_max_spread_ms": max(kern["k_score"]) - min(kern["k_score"]), "wall_ratio": statistics.median(wall["k_score_map"]) / statistics.median(wall["k_score"]),
                      "map_bytes": int(visits.nbytes), "decisions_first3": visits[:3].sum(axis=1).tolist(), "cells_visited_first3": (visits[:3] > 0).sum(axis=1).tolist(),
                      "added_work": "one LDS atomic per lane and period, at most 45 global atomic instructions per wave at the end"})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln), flush=True)


if __name__ == "__main__":
    main()
