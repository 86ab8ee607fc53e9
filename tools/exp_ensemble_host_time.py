#!/usr/bin/env python3
"""Host time of one dql_ensemble_run call for each of the seven learner kernels, one library against another (DESIGN.md sections 15 and 26).

    python tools/exp_ensemble_host_time.py one                       # this process, the library _lib loads (DQL_LIB_PATH): one JSON line, us per call
    python tools/exp_ensemble_host_time.py ab --parent PARENT.so     # parent and branch alternating, P1 B1 P2 B2 P3 B3, one process each; the table's rows
    python tools/exp_ensemble_host_time.py ab --parent PARENT.so --learners 16384 --raw OUT.jsonl   # a larger ensemble, device time too, the raw lines kept

What is timed: the wall time of one call on 64 learners (the team modes: 16 x 4 envs), float32, tables of zeros, greedy; 16 periods in plain, team and n-step
mode (n = 4), 8 periods starting on an advance point (advance_every 8) in the three worklist modes; schedules under which nobody freezes (window 128, 128
successes), so every call launches.  Median of 31 calls after 5 warm-up calls.  Bound of a row: |branch median - parent mean| <= the parent's max - min, or 2 %
of its mean if that is larger.

--learners N makes the ensemble N learners (the team modes: N / 4 teams x 4 envs) and adds, per mode, the device time of the call (dql_diag_ensemble_last: HIP
events around the call's launches), its median over the same 31 calls, as a second row `mode (device)` under the same bound."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
MODES = ("k_learn", "k_learn_team", "k_learn_team_nstep", "k_learn_nstep", "k_learn_levels", "k_learn_recipes", "k_learn_recipes_nstep")
TEAM, WORKLIST, RECIPES = MODES[1:3], MODES[4:], MODES[5:]
RULE = dict(window=128, min_successes=128, max_episodes=1 << 20)
WARMUP, CALLS, LEARNERS = 5, 31, 64


def ensemble(mode, learners):
    from dql_multirotor_landing_amd.config import F32, training_config
    from dql_multirotor_landing_amd.ensemble import LevelSchedule, Recipe, SequentialEnsemble
    team = mode in TEAM
    ens = SequentialEnsemble(training_config(0, quirks=0x40, dtype=F32), learners // 4 if team else learners, seed=11, eps=[0.0], envs_per_learner=4 if team else 1,
                             nstep=4 if mode == "k_learn_nstep" else 0, team_nstep=4 if mode == "k_learn_team_nstep" else 0, **RULE)
    if mode in WORKLIST:
        for k in range(5):
            ens.set_level_schedules(k, [0.0], **RULE)
        ens.set_curriculum(4, 8)
    if mode in RECIPES:
        n = (0, 4) if mode == "k_learn_recipes_nstep" else (0, 0)
        ens.set_recipes([Recipe(quirks=0x40, nstep=n[r], levels=tuple(LevelSchedule(eps=[0.0], **RULE) for _ in range(5))) for r in range(2)], [l % 2 for l in range(learners)])
    return ens


def one(learners, device):
    from dql_multirotor_landing_amd import _lib
    out = {}
    for mode in MODES:
        ens = ensemble(mode, learners)
        try:
            periods, t, d = (8 if mode in WORKLIST else 16), [], []
            for _ in range(WARMUP + CALLS):
                t0 = time.perf_counter()
                ens.run(periods)
                t.append(time.perf_counter() - t0)
                if device:
                    ms = C.c_double(0.0)
                    _lib.check(ens.lib.dql_diag_ensemble_last(ens._h, C.byref(ms)))
                    d.append(ms.value)
            launches = ens.launches()
            assert launches[0] == WARMUP + CALLS and ens.n_live() == ens.n and ens.index_faults() == 0, (mode, launches)
            out[mode] = round(statistics.median(t[WARMUP:]) * 1e6, 1)
            if device:
                out[mode + " (device)"] = round(statistics.median(d[WARMUP:]) * 1e3, 1)
        finally:
            ens.close()
    return out


def ab(parent, learners, device, raw):
    runs = {"P": [], "B": []}
    for i in range(3):
        for who, lib in (("P", parent), ("B", None)):
            env = dict(os.environ)
            if lib:
                env["DQL_LIB_PATH"] = str(Path(lib).resolve())
            else:
                env.pop("DQL_LIB_PATH", None)
            cmd = [sys.executable, __file__, "one"] + (["--learners", str(learners)] if device else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True)
            runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
            if raw:
                with open(raw, "a") as f:
                    f.write(json.dumps({"learners": learners, "who": who, "run": i + 1, "us": runs[who][-1]}) + "\n")
    for mode in runs["P"][0]:
        p, b = [r[mode] for r in runs["P"]], [r[mode] for r in runs["B"]]
        mean = statistics.mean(p)
        spread, diff = max(max(p) - min(p), 0.02 * mean), statistics.median(b) - mean
        print(f"| `{mode}` | {', '.join(map(str, p))} | {', '.join(map(str, b))} | {statistics.median(p)} | {statistics.median(b)} | {spread:.1f} | {diff:+.1f} | "
              f"{'yes' if abs(diff) <= spread else 'NO'} |", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("one", "ab"))
    ap.add_argument("--parent", help="the parent's libdql_hip.so (ab)")
    ap.add_argument("--learners", type=int, help="the ensemble's size, a multiple of 4 (default 64); given, the device time of each call is reported too")
    ap.add_argument("--raw", help="append each process's JSON line to this file (ab)")
    a = ap.parse_args()
    device, learners = a.learners is not None, a.learners or LEARNERS
    if learners < 4 or learners % 4:
        ap.error("--learners must be a positive multiple of 4 (the team modes fly teams of 4 envs)")
    if a.what == "one":
        print(json.dumps(one(learners, device)), flush=True)
    else:
        ab(a.parent, learners, device, a.raw)


if __name__ == "__main__":
    main()
