"""What scoring thousands of table sets costs -> profiles/score_timing.jsonl.

  ensemble_vs_rollout  both landing rates of 4 096 learners' tables on 256 envs each, float32: `SequentialEnsemble.landing_rates` (two launches of k_score on
                       the resident tables) against the only way without it — fetch the tables, then 256 calls of `evaluation.landing_scores` with 16 table
                       sets each (512 launches of k_rollout) —, alternating in the same process.  The rates must be equal.
  lane_reuse           the same number of episodes per table set flown two ways: 64 E envs with one episode each against 64 envs with E episodes each,
                       E = 4 and 16, 4 096 table sets, simulation flavour, float32, alternating.  max_steps is 600 per episode asked for (at most 4 096);
                       the unfinished episodes of each way are reported beside its time.

Every figure: one warm-up, then the median of 7 runs with min and max.  Wall clocks include the copies of the results to the host.

python tools/exp_score.py [--out profiles/score_timing.jsonl] [--runs 7] [--learners 4096]"""
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "score_timing.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--learners", type=int, default=4096)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import F32, Q_PAPER, Q_REFERENCE, simulation_config, training_config
    from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
    assets = ROOT / "tests" / "golden" / "assets"
    qa, qb = (np.load(assets / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
    sets3 = [(qa, qb), (np.zeros_like(qa), np.zeros_like(qb)), (qa, -qb)]
    L = a.learners
    QA = np.stack([sets3[k % 3][0] for k in range(L)]); QB = np.stack([sets3[k % 3][1] for k in range(L)])
    lines = []

    # ---- (a) an ensemble's tables: scored where they live, against fetch + landing_scores 16 at a time ----
    ens = SequentialEnsemble(training_config(0, dtype=F32, quirks=Q_REFERENCE), L, seed=42)
    try:
        ens.set_tables(QA, QB)
        wall = {"ensemble_score": [], "landing_scores_x16": []}
        kern = {"ensemble_score": [], "landing_scores_x16": []}
        rates = {}
        for run in range(a.runs + 1):  # run 0 warms both paths up
            t = {}
            t0 = time.perf_counter()
            r = ens.landing_rates(n_envs=N_ENVS, episodes=1, level=LEVEL, seed=SEED, timing=t)
            w = (time.perf_counter() - t0) * 1e3
            rates["ensemble_score"] = (r["touchdown_rate"], r["goal_hold_rate"])
            if run:
                wall["ensemble_score"].append(w); kern["ensemble_score"].append(t["kernel_ms"])
            t0 = time.perf_counter()
            fa, fb, _ = ens.get_tables()
            k_ms, out = 0.0, []
            for lo in range(0, L, ops.ROLLOUT_MAX_TABLES):
                t = {}
                out += evaluation.landing_scores([(fa[k], fb[k]) for k in range(lo, min(lo + ops.ROLLOUT_MAX_TABLES, L))], N_ENVS, LEVEL, seed=SEED, timing=t)
                k_ms += t["kernel_ms"]
            w = (time.perf_counter() - t0) * 1e3
            rates["landing_scores_x16"] = (np.array([s["touchdown_rate"] for s in out]), np.array([s["goal_hold_rate"] for s in out]))
            if run:
                wall["landing_scores_x16"].append(w); kern["landing_scores_x16"].append(k_ms)
        for f in (0, 1):
            assert np.array_equal(rates["ensemble_score"][f], rates["landing_scores_x16"][f])
        calls = -(-L // ops.ROLLOUT_MAX_TABLES)
        for method, launches in (("ensemble_score", 2), ("landing_scores_x16", 2 * calls)):
            lines.append({"what": "ensemble_vs_rollout", "method": method, "table_sets": L, "envs_per_table": N_ENVS, "episodes_per_env": 1, "level": LEVEL, "seed": SEED,
                          "launches": launches, "wall_ms": spread(wall[method]), "kernel_ms": spread(kern[method]),
                          "touchdown_rate_first3": rates[method][0][:3].tolist(), "goal_hold_rate_first3": rates[method][1][:3].tolist()})
        lines.append({"what": "ensemble_vs_rollout_ratio", "rollout_over_score_wall": statistics.median(wall["landing_scores_x16"]) / statistics.median(wall["ensemble_score"]),
                      "rollout_over_score_kernel": statistics.median(kern["landing_scores_x16"]) / statistics.median(kern["ensemble_score"])})
    finally:
        ens.close()

    # ---- (b) lane re-use: 64 E envs x 1 episode against 64 envs x E episodes ----
    cfg = simulation_config(working_curriculum_step=LEVEL, dtype=F32, quirks=Q_PAPER)
    for E in (4, 16):
        ways = {"fresh_lanes": dict(envs=64 * E, episodes=1, max_steps=600), "lane_reuse": dict(envs=64, episodes=E, max_steps=min(600 * E, ops.SCORE_MAX_STEPS))}
        wall = {k: [] for k in ways}; kern = {k: [] for k in ways}; res = {}
        for run in range(a.runs + 1):
            for way, kw in ways.items():
                t = {}
                t0 = time.perf_counter()
                res[way] = ops.score(cfg, QA, QB, kw["envs"], SEED, episodes=kw["episodes"], max_steps=kw["max_steps"], timing=t)
                w = (time.perf_counter() - t0) * 1e3
                if run:
                    wall[way].append(w); kern[way].append(t["kernel_ms"])
        for way, kw in ways.items():
            bc = res[way]["by_code"]
            lines.append({"what": "lane_reuse", "way": way, "E": E, "table_sets": L, **kw, "episodes_per_table_set": 64 * E, "wall_ms": spread(wall[way]),
                          "kernel_ms": spread(kern[way]), "unfinished_episodes": int(bc[:, -1].sum()), "finished_episodes": int(bc[:, :-1].sum()),
                          "mean_episode_length": float(res[way]["steps_sum"].sum() / max(int(bc[:, :-1].sum()), 1)),
                          "touchdown_rate_first3": ops.rates_from_counts(bc[:3], "TERMINAL_CONTACT").tolist()})
        lines.append({"what": "lane_reuse_ratio", "E": E, "fresh_over_reuse_kernel": statistics.median(kern["fresh_lanes"]) / statistics.median(kern["lane_reuse"]),
                      "fresh_over_reuse_wall": statistics.median(wall["fresh_lanes"]) / statistics.median(wall["lane_reuse"])})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln), flush=True)


if __name__ == "__main__":
    main()
