#!/usr/bin/env python3
"""Host time of one dql_ensemble_run call for each of the six learner kernels, one library against another.

    python tools/exp_ensemble_host_time.py one                       # this process, the library _lib loads (DQL_LIB_PATH): one JSON line, us per call
    python tools/exp_ensemble_host_time.py ab --parent PARENT.so     # parent and branch alternating, P1 B1 P2 B2 P3 B3, one process each; the table's rows

What is timed: the wall time of one call on 64 learners (the team mode: 16 x 4 envs), float32, tables of zeros, greedy; 16 periods in plain, team and n-step
mode, 8 periods starting on an advance point (advance_every 8) in the three worklist modes; schedules under which nobody freezes (window 128, 128 successes), so
every call launches.  Median of 31 calls after 5 warm-up calls.  Bound of a row: |branch median - parent mean| <= the parent's max - min, or 2 % of its mean if
that is larger."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
MODES = ("k_learn", "k_learn_team", "k_learn_nstep", "k_learn_levels", "k_learn_recipes", "k_learn_recipes_nstep")
RULE = dict(window=128, min_successes=128, max_episodes=1 << 20)
WARMUP, CALLS = 5, 31


def ensemble(mode):
    from dql_multirotor_landing_amd.config import F32, training_config
    from dql_multirotor_landing_amd.ensemble import LevelSchedule, Recipe, SequentialEnsemble
    team = mode == "k_learn_team"
    ens = SequentialEnsemble(training_config(0, quirks=0x40, dtype=F32), 16 if team else 64, seed=11, eps=[0.0], envs_per_learner=4 if team else 1,
                             nstep=4 if mode == "k_learn_nstep" else 0, **RULE)
    if mode in MODES[3:]:
        for k in range(5):
            ens.set_level_schedules(k, [0.0], **RULE)
        ens.set_curriculum(4, 8)
    if mode in MODES[4:]:
        n = (0, 4) if mode == "k_learn_recipes_nstep" else (0, 0)
        ens.set_recipes([Recipe(quirks=0x40, nstep=n[r], levels=tuple(LevelSchedule(eps=[0.0], **RULE) for _ in range(5))) for r in range(2)], [l % 2 for l in range(64)])
    return ens


def one():
    out = {}
    for mode in MODES:
        ens = ensemble(mode)
        try:
            periods, t = (8 if mode in MODES[3:] else 16), []
            for _ in range(WARMUP + CALLS):
                t0 = time.perf_counter()
                ens.run(periods)
                t.append(time.perf_counter() - t0)
            launches = ens.launches()
            assert launches[0] == WARMUP + CALLS and ens.n_live() == ens.n and ens.index_faults() == 0, (mode, launches)
            out[mode] = round(statistics.median(t[WARMUP:]) * 1e6, 1)
        finally:
            ens.close()
    return out


def ab(parent):
    runs = {"P": [], "B": []}
    for _ in range(3):
        for who, lib in (("P", parent), ("B", None)):
            env = dict(os.environ)
            if lib:
                env["DQL_LIB_PATH"] = str(Path(lib).resolve())
            else:
                env.pop("DQL_LIB_PATH", None)
            r = subprocess.run([sys.executable, __file__, "one"], env=env, capture_output=True, text=True, check=True)
            runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    for mode in MODES:
        p, b = [r[mode] for r in runs["P"]], [r[mode] for r in runs["B"]]
        mean = statistics.mean(p)
        spread, diff = max(max(p) - min(p), 0.02 * mean), statistics.median(b) - mean
        print(f"| `{mode}` | {', '.join(map(str, p))} | {', '.join(map(str, b))} | {statistics.median(p)} | {statistics.median(b)} | {spread:.1f} | {diff:+.1f} | "
              f"{'yes' if abs(diff) <= spread else 'NO'} |", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("one", "ab"))
    ap.add_argument("--parent", help="the parent's libdql_hip.so (ab)")
    a = ap.parse_args()
    if a.what == "one":
        print(json.dumps(one()), flush=True)
    else:
        ab(a.parent)


if __name__ == "__main__":
    main()
