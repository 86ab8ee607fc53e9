#!/usr/bin/env python3
"""Team curriculum mode on the GPU: what letting every team walk the levels by itself does to the wall clock of a whole curriculum.

    python tools/exp_team_levels.py [--teams 1024] [--envs 64] [--team-nstep 8] [--episodes 50000] [--seed 42] [--advance-every 4096 512] [--reps 3]
                                    [--score 1024] [--out profiles/team_levels_timing.jsonl]

The workload is README's team n-step line: `--teams` teams of `--envs` envs, the paper preset (evaluation.Q_PAPER, the paper's transfer order,
as_launched_config, float32), `--team-nstep`, `--episodes` episodes per level.  It is flown by the level-by-level driver (scripts/ensemble_training.py's
curriculum_paper: every team waits at every level for the slowest) and by `ensemble.curriculum_per_team` at each `--advance-every`.  The yardstick for the time
is the barrier driver in the same session on the same machine: the variants alternate, `--reps` times, one process per run (a fresh ensemble, a fresh HIP
context), after one small warm-up run per process that loads the code objects.  One line per run: the wall clock of the curriculum (a host clock around calls
that end in a device synchronise; the scoring is outside it), the launches, periods and waves x periods of dql_diag_ensemble_launches, and the median
touchdown rate of `landing_rates` on `--score` envs per team.  A whole curriculum ends with its last team, which may be one that never promotes at the last
level and flies its whole budget there, so a line also says when the teams were done: the barrier driver's wall clock at the end of every level
(`level_done_wall_s`; nobody is done before the last level begins), the per-team driver's after every 8 192 periods with the teams still unfinished (`progress`) and,
from it, the wall clock by which half, 90 %, 99 % and all of the teams had finished (`wall_s_until_finished`).  The two drivers do not produce the same tables — their advance points differ — so the quality
figure is reported as found, not compared bit for bit.  A failure or a time-out ends the tool."""
import argparse
import importlib.util
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PROGRESS_EVERY = 8192  # periods between two looks at the per-team driver's unfinished teams: a multiple of every --advance-every, so no launch is cut by it


def child(a):
    from dql_multirotor_landing_amd import evaluation
    from dql_multirotor_landing_amd.config import F32, as_launched_config
    from dql_multirotor_landing_amd.ensemble import ORDER_PAPER, SequentialEnsemble, curriculum_per_team
    spec = importlib.util.spec_from_file_location("ensemble_training_script", ROOT / "scripts" / "ensemble_training.py")
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    cfg = lambda: as_launched_config(dtype=F32, quirks=evaluation.Q_PAPER)

    def fly(ens, episodes, max_periods=None):
        t0, marks = time.perf_counter(), []
        if a.driver == "barrier":
            script.curriculum_paper(ens, 5, episodes, on_level=lambda e, h: marks.append(time.perf_counter() - t0))
            return {"level_done_wall_s": marks}
        curriculum_per_team(ens, last_level=4, advance_every=a.every, transfer_order=ORDER_PAPER, max_episodes=episodes, max_periods=max_periods, chunk_periods=PROGRESS_EVERY,
                            on_chunk=lambda e, flown: marks.append((flown, time.perf_counter() - t0, e.n_unfinished())))
        until = {str(share): next((w for _, w, u in marks if ens.n - u >= share * ens.n), None) for share in (0.5, 0.9, 0.99, 1.0)}
        return {"progress": marks, "wall_s_until_finished": until}

    warm = SequentialEnsemble(cfg(), 8, seed=1, max_episodes=4, envs_per_learner=a.envs, team_nstep=a.team_nstep)
    try:
        fly(warm, 4, 4096)
        warm.landing_rates(n_envs=64, episodes=1, level=4, seed=1)
    finally:
        warm.close()
    ens = SequentialEnsemble(cfg(), a.teams, seed=a.seed, max_episodes=a.episodes, envs_per_learner=a.envs, team_nstep=a.team_nstep)
    try:
        t0 = time.perf_counter()
        when = fly(ens, a.episodes)
        wall = time.perf_counter() - t0
        launches, periods, wave_periods = ens.launches()
        line = {"what": "team_levels_timing", "driver": a.driver, "advance_every": a.every if a.driver == "per_team" else None, "rep": a.rep, "teams": a.teams, "envs_per_team": a.envs,
                "team_nstep": a.team_nstep, "episodes_per_level": a.episodes, "seed": a.seed, "wall_s": wall, "launches": launches, "periods": periods, "wave_periods": wave_periods,
                "period_index": ens.period_index(), "unfinished": ens.n_unfinished(), "index_faults": ens.index_faults(),
                "teams_per_level": np.bincount(ens.levels()["level"], minlength=5).tolist(), **when}
        if a.score:
            td = ens.landing_rates(n_envs=a.score, episodes=evaluation.DEFAULT_SCORE_EPISODES, level=4, seed=123)["touchdown_rate"]
            line.update({"score_envs": a.score, "touchdown_median": float(np.median(td)), "touchdown_mean": float(td.mean()), "share_at_or_above_bar": float((td >= evaluation.LANDING_BAR).mean())})
        print("LINE " + json.dumps(line), flush=True)
    finally:
        ens.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--teams", type=int, default=1024)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--team-nstep", type=int, default=8)
    ap.add_argument("--episodes", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--advance-every", type=int, nargs="+", default=[4096, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--score", type=int, default=1024)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per run")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "team_levels_timing.jsonl"))
    ap.add_argument("--driver", default=None, help=argparse.SUPPRESS)  # the child's: barrier | per_team
    ap.add_argument("--every", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--rep", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if any(e < 1 or PROGRESS_EVERY % e for e in a.advance_every):
        ap.error(f"--advance-every must divide {PROGRESS_EVERY}")
    if a.driver:
        return child(a)
    variants = [("barrier", 0)] + [("per_team", e) for e in a.advance_every]
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as f:
        for rep in range(a.reps):
            for driver, every in variants:  # alternating: the yardstick and the variants share whatever else the machine is doing
                cmd = [sys.executable, __file__, "--driver", driver, "--every", str(every), "--rep", str(rep), "--teams", str(a.teams), "--envs", str(a.envs), "--team-nstep", str(a.team_nstep),
                       "--episodes", str(a.episodes), "--seed", str(a.seed), "--score", str(a.score)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                lines = [l[5:] for l in r.stdout.splitlines() if l.startswith("LINE ")]
                if r.returncode != 0 or len(lines) != 1:
                    sys.exit(f"{driver} (advance_every {every}, rep {rep}) failed with status {r.returncode}:\n{r.stderr[-3000:]}")
                f.write(lines[0] + "\n"); f.flush()
                print(lines[0], flush=True)


if __name__ == "__main__":
    main()
