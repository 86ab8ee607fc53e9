#!/usr/bin/env python3
"""Team learners with n-step Double-Q targets on the GPU: what a period costs beside k_learn_team, and what the reference's full episode
budget gives with n-step targets.

    python tools/exp_team_nstep.py timing [--learners 1024] [--sizes 1,16,64] [--nsteps 1,4,16] [--periods 512] [--repeats 7] [--timeout 300]
                                          [--out profiles/team_nstep_timing.jsonl]
    python tools/exp_team_nstep.py findings [--learners 1024] [--envs-per-learner 64] [--episodes 50000] [--score 1024] [--nsteps 0,4,8,16] [--seeds 42,43]
                                            [--timeout 300] [--out profiles/team_nstep_findings.jsonl]

timing: tools/exp_teams.py's protocol — float32, `training_config(0)` with the reference's quirks, tables of zeros, exploration rate 1 and no promotion, so
every team stays live.  Per team size E one process holds a team ensemble with team_nstep = 0 (k_learn_team) and one per n of `--nsteps`
(k_learn_team_nstep), all of `--learners` learners; after a warm-up run each, the ways alternate `--repeats` times with runs of `--periods` periods.  Per
way: the median and the smallest and largest of `dql_diag_ensemble_last` (HIP events around the run call's launch), microseconds per period, and the ratio to
k_learn_team of the same process.

findings: section 17(b)'s run — `--learners` learners x `--envs-per-learner` envs, float32, `as_launched_config`, the paper preset (evaluation.Q_PAPER, on
entering level k + 1 `Q[k+1] = Q[k] ratio(k + 1)`, nothing after the last level), `--episodes` episodes per level, the barrier driver — at every team_nstep
of `--nsteps` and every seed of `--seeds`, then `landing_rates` on `--score` envs per learner.  Every (n, seed) is a child process of its own under
`--timeout` seconds; lines are appended to `--out` as they arrive.  A child that fails or runs out of time ends the tool: nothing more is started."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dql_multirotor_landing_amd import _lib  # noqa: E402
from dql_multirotor_landing_amd import evaluation  # noqa: E402
from dql_multirotor_landing_amd.config import F32, as_launched_config, training_config  # noqa: E402
from dql_multirotor_landing_amd.ensemble import (REFERENCE_RATIOS, SequentialEnsemble, exploration_rates, min_successes_for, train_level)  # noqa: E402


def last_ms(ens):
    v = C.c_double()
    _lib.check(ens.lib.dql_diag_ensemble_last(ens._h, C.byref(v)))
    return float(v.value)


def measure(a, E):
    cfg = training_config(0, quirks=0x7F, dtype=F32)
    kw = dict(seed=a.seed, eps=[1.0], window=100, min_successes=97, max_episodes=1 << 30, envs_per_learner=E, teams=True)
    ways = {0: SequentialEnsemble(cfg, a.learners, **kw)}
    try:
        for n in a.nstep_list:
            ways[n] = SequentialEnsemble(cfg, a.learners, team_nstep=n, **kw)
        ms = {n: [] for n in ways}
        for e in ways.values():
            e.run(a.periods)  # warm-up (period 0, the reset period, included)
        before = {n: (int(e.counters()["episodes"].sum()), int(e.counters()["decisions"].sum())) for n, e in ways.items()}
        for _ in range(a.repeats):
            for n, e in ways.items():
                e.run(a.periods)
                ms[n].append(last_ms(e))
        base = statistics.median(ms[0])
        out = []
        for n, e in ways.items():
            assert e.index_faults() == 0 and e.n_live() == a.learners
            c = e.counters()
            episodes, decisions = int(c["episodes"].sum()) - before[n][0], int(c["decisions"].sum()) - before[n][1]
            med = statistics.median(ms[n])
            out.append({"what": "team_nstep_timing", "kernel": "k_learn_team_nstep" if n else "k_learn_team", "team_nstep": n, "dtype": "float32", "learners": a.learners,
                        "envs_per_learner": E, "periods_per_run": a.periods, "runs": a.repeats, "run_ms_median": med, "run_ms_min": min(ms[n]), "run_ms_max": max(ms[n]),
                        "us_per_period": 1000.0 * med / a.periods, "ratio_to_k_learn_team": med / base,
                        "decisions_per_period_and_learner": decisions / (a.repeats * a.periods) / a.learners,
                        "episodes_per_period_and_learner": episodes / (a.repeats * a.periods) / a.learners,
                        "episodes_per_second_and_learner": episodes / (sum(ms[n]) * 1e-3) / a.learners})
        return out
    finally:
        for e in ways.values():
            e.close()


def rate_summary(x):
    q = np.quantile(np.asarray(x, dtype=np.float64), (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0))
    return {"mean": float(np.mean(x)), **{k: float(v) for k, v in zip(("min", "q05", "q25", "q50", "q75", "q95", "max"), q)}}


def findings(a, n, seed):
    ens = SequentialEnsemble(as_launched_config(dtype=F32, quirks=evaluation.Q_PAPER), a.learners, seed=seed, max_episodes=a.episodes, envs_per_learner=a.envs_per_learner,
                             team_nstep=n)
    try:
        t0 = time.perf_counter()
        levels = []
        for k in range(5):
            if k:
                ens.set_level(k)
            ens.set_schedules(eps=exploration_rates(k), window=100, min_successes=min_successes_for(100), max_episodes=a.episodes)
            flown = train_level(ens)
            c = ens.counters()
            p = c["promotion_episode"]
            levels.append({"level": k, "periods": flown, "promoted": int((p >= 0).sum()), "median_promotion_episode": None if not (p >= 0).any() else int(np.median(p[p >= 0])),
                           "episodes_total": int(c["episodes"].sum()), "open_windows_at_the_end": int((ens.team_pending_lengths() > 0).sum())})
            if k < 4:
                ens.transfer(k + 1, REFERENCE_RATIOS[k + 1])
        train_s = time.perf_counter() - t0
        assert ens.index_faults() == 0
        t = {}
        r = ens.landing_rates(timing=t, n_envs=a.score, episodes=1, level=4, seed=123)
        td, gh = r["touchdown_rate"], r["goal_hold_rate"]
        return {"what": "team_nstep_findings", "team_nstep": n, "seed": seed, "preset": "paper", "quirks": evaluation.Q_PAPER, "learners": a.learners,
                "envs_per_learner": a.envs_per_learner, "dtype": "float32", "launched": True, "episode_budget_per_level": a.episodes, "mode": "barrier", "levels": levels,
                "train_wall_s": train_s, "score_envs_per_learner": a.score, "score_kernel_ms": t["kernel_ms"], "bar": evaluation.LANDING_BAR,
                "learners_at_or_above_bar": int((td >= evaluation.LANDING_BAR).sum()), "share_at_or_above_bar": float((td >= evaluation.LANDING_BAR).mean()),
                "touchdown_rate": rate_summary(td), "goal_hold_rate": rate_summary(gh)}
    finally:
        ens.close()


def child(a, extra):
    """one measurement in a process of its own under the time limit -> its JSON lines, or None (then nothing more is started on the GPU)"""
    cmd = [sys.executable, str(Path(__file__).resolve()), *extra, "--learners", str(a.learners), "--periods", str(a.periods), "--repeats", str(a.repeats), "--nsteps", a.nsteps,
           "--envs-per-learner", str(a.envs_per_learner), "--episodes", str(a.episodes), "--score", str(a.score), "--seed", str(a.seed)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write(f"{' '.join(extra)}: no result within {a.timeout} s\n")
        return None
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        return None
    return [l for l in r.stdout.splitlines() if l.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["timing", "one", "findings", "one-findings"])
    ap.add_argument("--learners", type=int, default=1024)
    ap.add_argument("--sizes", default="1,16,64")
    ap.add_argument("--nsteps", default=None, help="timing: 1,4,16; findings: 0,4,8,16")
    ap.add_argument("--periods", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--seeds", default="42,43")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--size", type=int, default=0, help="(mode one) the team size this process measures")
    ap.add_argument("--nstep", type=int, default=0, help="(mode one-findings) the team_nstep this process flies")
    ap.add_argument("--envs-per-learner", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=50000)
    ap.add_argument("--score", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.nsteps is None:
        a.nsteps = "0,4,8,16" if "findings" in a.mode else "1,4,16"
    a.nstep_list = [int(s) for s in a.nsteps.split(",")]
    if a.mode == "one":
        for line in measure(a, a.size):
            print(json.dumps(line), flush=True)
        return 0
    if a.mode == "one-findings":
        print(json.dumps(findings(a, a.nstep, a.seed)), flush=True)
        return 0
    out = Path(a.out or ROOT / "profiles" / ("team_nstep_findings.jsonl" if a.mode == "findings" else "team_nstep_timing.jsonl"))
    jobs = ([["one", "--size", s] for s in a.sizes.split(",")] if a.mode == "timing" else
            [["one-findings", "--nstep", str(n), "--seed", s] for s in a.seeds.split(",") for n in a.nstep_list])
    for extra in jobs:
        if a.mode == "findings":
            a.seed = int(extra[-1]); extra = extra[:-2]
        lines = child(a, extra)
        if lines is None:
            return 1
        with open(out, "a") as f:
            for l in lines:
                print(l, flush=True)
                f.write(l + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
