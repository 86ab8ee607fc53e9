#!/usr/bin/env python3
"""The whole curriculum of an ensemble by `ensemble.curriculum` (every level waits for its slowest learner) against `ensemble.curriculum_per_learner` (every
learner walks the levels by itself), on the GPU.

    python tools/exp_ensemble_advance.py [--learners 4096] [--episodes 10000] [--window 100] [--success-rate 0.96] [--repeats 3] [--max-periods N]
                                         [--out profiles/ensemble_advance_timing.jsonl]

float32, `as_launched_config`, quirks 0x7f.  The paths — `curriculum`, `curriculum_per_learner` with E = 4096 and with E = 256 — alternate in one process,
`--repeats` times; per path the median wall clock is reported, with the periods launched summed over the launches, waves x periods launched, the
learner-periods actually flown and the distribution of the learners over the levels at the end.  Every period a live learner flies is a decision or the
reset period that opens an episode; a learner freezes at an episode's end, and the reset that `set_level` or an advance marks is the one that opens its next
episode, so the count is decisions + episodes + 1 per learner, less 1 for a learner that stands frozen (its next reset was not flown).  The yardstick of
tests/advance_checks.py, counting live learners period by period, gives the same figure.  If the per-learner path promotes nobody beyond level 0, a second
set of lines is measured with `--second-window` / `--second-success-rate` (default: 10 episodes, 0.5), a setting chosen beforehand, not tuned.  `--max-periods` caps a path (per level for `curriculum`, divided by the levels); a capped
run says so.  One JSON line per path is appended to `--out`."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dql_multirotor_landing_amd.config import F32, as_launched_config  # noqa: E402
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble, curriculum, curriculum_per_learner  # noqa: E402


def one(path, a):
    ens = SequentialEnsemble(as_launched_config(dtype=F32, quirks=0x7F), a.learners, seed=a.seed, max_episodes=a.episodes)
    try:
        t0 = time.perf_counter()
        if path == "curriculum":
            curriculum(ens, max_episodes=a.episodes, window=a.window, success_rate=a.success_rate,
                       max_periods_per_level=None if a.max_periods is None else a.max_periods // 5)
            level = np.full(a.learners, 4)
            finished = ens.n_live() == 0
            beyond = None
        else:
            h = curriculum_per_learner(ens, advance_every=int(path.split("=")[1]), max_episodes=a.episodes, window=a.window, success_rate=a.success_rate,
                                       max_periods=a.max_periods)
            level = h["level"]
            finished = ens.n_unfinished() == 0
            beyond = int((h["promoted_at"][1:] >= 0).any(axis=0).sum())
        wall = time.perf_counter() - t0
        c = ens.counters()
        n, p, wp = ens.launches()
        return {"wall_s": wall, "launches": n, "periods_launched": p, "wave_periods_launched": wp,
                "learner_periods_flown": int(c["decisions"].sum() + c["episodes"].sum() + a.learners - c["frozen"].astype(bool).sum()), "period_index": ens.period_index(),
                "learners_per_level_at_the_end": np.bincount(level, minlength=5).tolist(), "promoted_at_current_level": int((c["promotion_episode"] >= 0).sum()),
                "promoted_beyond_level_0": beyond, "finished": bool(finished), "index_faults": ens.index_faults()}
    finally:
        ens.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--learners", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=10000)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--success-rate", type=float, default=0.96)
    ap.add_argument("--second-window", type=int, default=10)
    ap.add_argument("--second-success-rate", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-periods", type=int, default=None)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ensemble_advance_timing.jsonl"))
    a = ap.parse_args()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    beyond = measure(a)
    if beyond == 0:
        print("nobody stands above level 1 by promotion: the two paths fly the same budgets; measuring the second setting", flush=True)
        a.window, a.success_rate = a.second_window, a.second_success_rate
        measure(a)


def measure(a):
    """one line per path appended to a.out; -> the learners of the per-learner path that promoted at a level above 0 or reached one by promotion"""
    paths = ("curriculum", "per_learner E=4096", "per_learner E=256")
    runs = {p: [] for p in paths}
    for _ in range(a.repeats):
        for p in paths:
            runs[p].append(one(p, a))
            print(json.dumps({"path": p, **runs[p][-1]}), flush=True)
    with open(a.out, "a") as f:
        for p in paths:
            r = runs[p]
            mid = sorted(r, key=lambda x: x["wall_s"])[len(r) // 2]
            row = {"what": "whole curriculum, float32, as_launched_config, quirks 0x7f", "path": p, "learners": a.learners, "episode_budget_per_level": a.episodes,
                   "window": a.window, "success_rate": a.success_rate, "max_periods": a.max_periods, "repeats": a.repeats,
                   "wall_s_median": round(statistics.median(x["wall_s"] for x in r), 3), "wall_s_all": [round(x["wall_s"], 3) for x in r],
                   "method": "paths alternating in one process, wall clock around the call, the other figures from the median run", **{k: v for k, v in mid.items() if k != "wall_s"}}
            f.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)
    return runs["per_learner E=256"][-1]["promoted_beyond_level_0"]


if __name__ == "__main__":
    main()
