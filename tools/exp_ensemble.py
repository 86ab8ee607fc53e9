#!/usr/bin/env python3
"""Sequential ensembles on the GPU: timing, and G14's second cut at 4 096 seeds.

    python tools/exp_ensemble.py timing [--out profiles/ensemble_timing.jsonl]
    python tools/exp_ensemble.py g14 [--learners 4096] [--episodes 19000] [--out profiles/ensemble_g14_level0.json]

timing: us per period and env-steps/s of `SequentialEnsemble.run` at L = 64, 4 096 and 65 536, float32 and float64 (level 0, eps = 1, no freeze; median of 7
runs of 512 periods after a warm-up run).
g14: the reference's own algorithm at level 0 with the as-launched parameters and quirks 0x7f, one env per learner, until every learner has promoted or spent
its episode budget: the distribution of the first-promotion episode and the goal share per 1 000 episodes, next to the Gazebo run's 18 282."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dql_multirotor_landing_amd.config import CHECK_NAMES, F32, F64, as_launched_config, training_config  # noqa: E402
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble, train_level  # noqa: E402

GOAL = CHECK_NAMES.index("TERMINAL_SUCCESS")


def timing(out):
    rows = []
    for dtype, name in ((F32, "float32"), (F64, "float64")):
        for L in (64, 4096, 65536):
            ens = SequentialEnsemble(training_config(0, dtype=dtype), L, seed=1, eps=[1.0], max_episodes=1 << 30, window=100, min_successes=101)
            try:
                P = 512
                ens.run(P)
                ts = []
                for _ in range(7):
                    t0 = time.perf_counter(); ens.run(P); ts.append(time.perf_counter() - t0)
                t = statistics.median(ts)
                dec = int(ens.counters()["decisions"].sum())
                rows.append({"what": "SequentialEnsemble.run", "dtype": name, "learners": L, "periods_per_run": P, "us_per_period": round(t / P * 1e6, 2),
                             "env_steps_per_s": round(L * P / t), "method": "median of 7 runs after a warm-up run, wall clock around the call",
                             "decisions_so_far": dec, "index_faults": ens.index_faults()})
                print(json.dumps(rows[-1]), flush=True)
            finally:
                ens.close()
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text("".join(json.dumps(r) + "\n" for r in rows))


def g14(out, learners, episodes, seed):
    cfg = as_launched_config(dtype=F32, quirks=0x7F)
    ens = SequentialEnsemble(cfg, learners, seed=seed, log_capacity=episodes, max_episodes=episodes)
    try:
        t0 = time.perf_counter()
        flown = train_level(ens, on_chunk=lambda e, f: print(f"{f} periods, {e.n_live()} learners live, {time.perf_counter() - t0:.1f} s", flush=True))
        wall = time.perf_counter() - t0
        c = ens.counters()
        code, length, n = ens.episode_log()
        promo = c["promotion_episode"]
        hit = promo[promo >= 0]
        blocks = episodes // 1000
        share = []
        for b in range(blocks):
            alive = n >= (b + 1) * 1000
            share.append(None if not alive.any() else round(float((code[alive, b * 1000:(b + 1) * 1000] == GOAL).mean()), 4))
        res = {"what": "SequentialEnsemble, as_launched_config, quirks 0x7f, level 0, float32", "learners": learners, "seed": seed, "episode_budget": episodes,
               "periods": flown, "wall_s": round(wall, 1), "promoted": int(hit.size), "exhausted": int((promo < 0).sum()),
               "first_promotion_episode_quantiles": None if not hit.size else {q: int(np.quantile(hit, float(q))) for q in ("0.05", "0.25", "0.5", "0.75", "0.95")},
               "first_promotion_episode_min_max": None if not hit.size else [int(hit.min()), int(hit.max())],
               "goal_share_per_1000_episodes_over_learners_still_training": share, "gazebo_run_first_promotion_episode": 18282,
               "index_faults": ens.index_faults()}
        print(json.dumps(res), flush=True)
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(res) + "\n")
    finally:
        ens.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("timing", "g14"))
    ap.add_argument("--out")
    ap.add_argument("--learners", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=19000)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args()
    if a.what == "timing":
        timing(a.out or str(ROOT / "profiles" / "ensemble_timing.jsonl"))
    else:
        g14(a.out or str(ROOT / "profiles" / "ensemble_g14_level0.json"), a.learners, a.episodes, a.seed)
