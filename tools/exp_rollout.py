"""What a greedy evaluation costs by the stepwise loop and by the roll-out operator -> profiles/rollout_timing.jsonl.

  landing_score   wall clock of `evaluation.landing_score` (both flavours, 4 096 envs, the reference's stage-4 tables) by method "stepwise" and by
                  method "rollout", alternating in the same process, and the device time of the kernels of each: the stepwise loop's from its per-launch
                  event pairs (the loop is restated here with the kernel timer armed; launches counted), the roll-out's from the event pair around its
                  kernel.
  landing_scores  the same for K = 1, 4, 16 table sets in two launches (the K sets: the reference's tables, zeros, Q_table_b negated, repeated).

Every figure: one warm-up, then the median of 7 runs with min and max.  Wall clocks end in a device synchronise (both paths copy their results back).

python tools/exp_rollout.py [--out profiles/rollout_timing.jsonl] [--runs 7]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
N_ENVS, LEVEL, SEED, MAX_STEPS = 4096, 4, 123, 600


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def stepwise_kernel_time(tables, flavour, quirks):
    """evaluation.first_episode_outcomes' loop with the kernel timer armed: (histogram, total kernel ms, launches, instance)"""
    from dql_multirotor_landing_amd import evaluation
    from dql_multirotor_landing_amd.engine import Engine
    cfg = evaluation._flavour_config(flavour, LEVEL, None, dict(quirks=quirks))
    eng = Engine(cfg, N_ENVS, seed=SEED)
    try:
        eng.set_tables(*tables)
        eng.kernel_timer(True)
        first = np.full(N_ENVS, -1, np.int64)
        eng.eval_steps(1)
        for _ in range(MAX_STEPS):
            eng.eval_steps(1)
            d, c = eng.dones()
            new = (d != 0) & (first < 0)
            first[new] = c[new]
            if (first >= 0).all():
                break
        avg, launches = eng.kernel_time_ms()
        return evaluation._histogram(first), avg * launches, launches, eng.step_instance()
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rollout_timing.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    from dql_multirotor_landing_amd import evaluation
    from dql_multirotor_landing_amd.config import Q_PAPER
    assets = ROOT / "tests" / "golden" / "assets"
    qa, qb = (np.load(assets / f).ravel() for f in ("Q_table_a.npy", "Q_table_b.npy"))
    tables = (qa, qb, np.zeros_like(qa))
    sets3 = [(qa, qb), (np.zeros_like(qa), np.zeros_like(qb)), (qa, -qb)]
    lines = []

    # ---- landing_score by both methods, alternating ----
    wall = {"stepwise": [], "rollout": []}
    kern = {"stepwise": [], "rollout": []}
    info = {}
    score = {}
    for run in range(a.runs + 1):  # run 0 warms both paths up
        for method in ("stepwise", "rollout"):
            t0 = time.perf_counter()
            s = evaluation.landing_score(tables, N_ENVS, LEVEL, seed=SEED, method=method)
            w = (time.perf_counter() - t0) * 1e3
            if method == "stepwise":
                k, launches, inst = 0.0, 0, []
                for flavour in ("simulation", "training"):
                    _, ms, n, name = stepwise_kernel_time(tables, flavour, Q_PAPER)
                    k += ms; launches += n; inst.append(name)
                info[method] = {"launches": launches, "instance": inst}
            else:
                t = {}
                evaluation.landing_scores([tables], N_ENVS, LEVEL, seed=SEED, timing=t)
                k = t["kernel_ms"]
                info[method] = {"launches": 2, "instance": t["instance"]}
            score[method] = s
            if run:
                wall[method].append(w); kern[method].append(k)
    assert score["stepwise"] == score["rollout"], score
    for method in ("stepwise", "rollout"):
        lines.append({"what": "landing_score", "method": method, "envs": N_ENVS, "level": LEVEL, "seed": SEED, "score": score[method], "wall_ms": spread(wall[method]),
                      "kernel_ms": spread(kern[method]), **info[method]})
    lines.append({"what": "landing_score_ratio", "stepwise_over_rollout_wall": statistics.median(wall["stepwise"]) / statistics.median(wall["rollout"]),
                  "stepwise_over_rollout_kernel": statistics.median(kern["stepwise"]) / statistics.median(kern["rollout"])})

    # ---- landing_scores of K table sets ----
    for K in (1, 4, 16):
        sets = [sets3[k % 3] for k in range(K)]
        w, k = [], []
        for run in range(a.runs + 1):
            t = {}
            t0 = time.perf_counter()
            sc = evaluation.landing_scores(sets, N_ENVS, LEVEL, seed=SEED, timing=t)
            if run:
                w.append((time.perf_counter() - t0) * 1e3); k.append(t["kernel_ms"])
        assert sc[0] == score["rollout"]
        lines.append({"what": "landing_scores", "method": "rollout", "table_sets": K, "envs": N_ENVS, "wall_ms": spread(w), "kernel_ms": spread(k), "launches": 2,
                      "instance": t["instance"], "wall_ms_per_table_set": statistics.median(w) / K, "scores": sc[:3]})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
