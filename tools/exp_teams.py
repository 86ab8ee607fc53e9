#!/usr/bin/env python3
"""Learners with teams of envs on the GPU: what a period costs with E envs per learner against the one-env learner kernel.

    python tools/exp_teams.py timing [--learners 1024] [--sizes 1,4,16,64] [--periods 512] [--repeats 7] [--timeout 300]
                                     [--out profiles/ensemble_teams_timing.jsonl]
    python tools/exp_teams.py landing [--learners 1024] [--envs-per-learner 64] [--episodes 50000] [--score 1024] [--timeout 600]
                                      [--out profiles/ensemble_teams_landing.json]

timing: float32, `training_config(0)` with the reference's quirks, tables of zeros, exploration rate 1 and no promotion, so every learner stays live.  Per team
size E one team ensemble of `--learners` learners (k_learn_team, `--learners` * E envs) and one plain ensemble of `--learners` learners (k_learn) live in one
process; after a warm-up run each, the two ways alternate `--repeats` times with runs of `--periods` periods.  Per way the median of
`dql_diag_ensemble_last` (HIP events around the run call's launch) is written as microseconds per period, with the finished episodes per second and learner
over the timed runs.  E = 64 minus E = 1 is what the serial section (team_apply for 64 records) and the two barriers cost per period.  Each team size is
measured by a child process of its own under `--timeout` seconds; a child that fails or runs out of time ends the tool.

landing: section 13(c)'s question with the reference's full episode budget, in the barrier mode (level by level, everyone waits for the slowest), float32,
`as_launched_config`, for two presets, one child process each under `--timeout`: "reference" (quirks 0x7f, after level k `Q[k] = Q[k-1] ratio(k)` with the
k = 0 wrap: `ensemble.curriculum`) and "paper" (`evaluation.Q_PAPER`, on entering level k + 1 `Q[k+1] = Q[k] ratio(k + 1)`, nothing after the last level).  Then
every learner's tables are flown greedily where they live (`landing_rates`, `--score` envs per learner and flavour) and the quantiles of both rates, the
promotions per level and the wall clock are written, with the published tables' figures from the same call."""
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
    kw = dict(seed=a.seed, eps=[1.0], window=100, min_successes=97, max_episodes=1 << 30)
    ways = {"k_learn": SequentialEnsemble(cfg, a.learners, **kw), "k_learn_team": SequentialEnsemble(cfg, a.learners, envs_per_learner=E, teams=True, **kw)}
    try:
        ms = {w: [] for w in ways}
        for e in ways.values():
            e.run(a.periods)  # warm-up (period 0, the reset period, included)
        before = {w: int(e.counters()["episodes"].sum()) for w, e in ways.items()}
        for _ in range(a.repeats):
            for w, e in ways.items():
                e.run(a.periods)
                ms[w].append(last_ms(e))
        out = []
        for w, e in ways.items():
            assert e.index_faults() == 0 and e.n_live() == a.learners
            episodes = int(e.counters()["episodes"].sum()) - before[w]
            med = statistics.median(ms[w])
            out.append({"what": "ensemble_teams_timing", "kernel": w, "dtype": "float32", "learners": a.learners, "envs_per_learner": E if w == "k_learn_team" else 1,
                        "periods_per_run": a.periods, "runs": a.repeats, "run_ms_median": med, "run_ms_min": min(ms[w]), "run_ms_max": max(ms[w]),
                        "us_per_period": 1000.0 * med / a.periods, "episodes_per_second_and_learner": episodes / (sum(ms[w]) * 1e-3) / a.learners,
                        "measured_with_team_size": E})
        return out
    finally:
        for e in ways.values():
            e.close()


def rate_summary(x):
    q = np.quantile(np.asarray(x, dtype=np.float64), (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0))
    return {"mean": float(np.mean(x)), **{k: float(v) for k, v in zip(("min", "q05", "q25", "q50", "q75", "q95", "max"), q)}}


def landing(a, preset):
    quirks = 0x7F if preset == "reference" else evaluation.Q_PAPER
    ens = SequentialEnsemble(as_launched_config(dtype=F32, quirks=quirks), a.learners, seed=a.seed, max_episodes=a.episodes, envs_per_learner=a.envs_per_learner)
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
                           "episodes_total": int(c["episodes"].sum())})
            if preset == "reference":
                ens.transfer(k, REFERENCE_RATIOS[k])
            elif k < 4:
                ens.transfer(k + 1, REFERENCE_RATIOS[k + 1])
        train_s = time.perf_counter() - t0
        assert ens.index_faults() == 0
        kw = dict(n_envs=a.score, episodes=1, level=4, seed=123)
        t = {}
        r = ens.landing_rates(timing=t, **kw)
        td, gh = r["touchdown_rate"], r["goal_hold_rate"]
        ref = ROOT / "tests" / "golden" / "assets"
        qa, qb = (np.load(ref / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
        rr = evaluation.landing_rates(qa, qb, **kw)
        return {"what": "ensemble_teams_landing", "preset": preset, "quirks": quirks, "learners": a.learners, "envs_per_learner": a.envs_per_learner, "dtype": "float32",
                "launched": True, "episode_budget_per_level": a.episodes, "mode": "barrier", "levels": levels, "train_wall_s": train_s, "score_envs_per_learner": a.score,
                "score_kernel_ms": t["kernel_ms"], "bar": evaluation.LANDING_BAR, "learners_at_or_above_bar": int((td >= evaluation.LANDING_BAR).sum()),
                "touchdown_rate": rate_summary(td), "goal_hold_rate": rate_summary(gh),
                "reference_tables": {"touchdown_rate": float(rr["touchdown_rate"][0]), "goal_hold_rate": float(rr["goal_hold_rate"][0])}}
    finally:
        ens.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["timing", "one", "landing", "one-landing"])
    ap.add_argument("--learners", type=int, default=1024)
    ap.add_argument("--sizes", default="1,4,16,64")
    ap.add_argument("--periods", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a team size's child process may take")
    ap.add_argument("--size", type=int, default=0, help="(mode one) the team size this process measures")
    ap.add_argument("--envs-per-learner", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=50000)
    ap.add_argument("--score", type=int, default=1024)
    ap.add_argument("--preset", default="reference", help="(mode one-landing) the preset this process flies")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = str(ROOT / "profiles" / ("ensemble_teams_landing.json" if "landing" in a.mode else "ensemble_teams_timing.jsonl"))
    if a.mode == "one-landing":
        print(json.dumps(landing(a, a.preset)), flush=True)
        return 0
    if a.mode == "landing":
        results = []
        for preset in ("reference", "paper"):
            cmd = [sys.executable, str(Path(__file__).resolve()), "one-landing", "--preset", preset, "--learners", str(a.learners), "--envs-per-learner", str(a.envs_per_learner),
                   "--episodes", str(a.episodes), "--score", str(a.score), "--seed", str(a.seed)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)  # a time-out or a failure ends the tool: nothing more is started on the GPU
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                return r.returncode
            results.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
            print(json.dumps(results[-1]), flush=True)
            Path(a.out).write_text(json.dumps(results, indent=1) + "\n")
        return 0
    if a.mode == "one":
        for line in measure(a, a.size):
            print(json.dumps(line), flush=True)
        return 0
    lines = []
    for E in (int(s) for s in a.sizes.split(",")):
        cmd = [sys.executable, str(Path(__file__).resolve()), "one", "--size", str(E), "--learners", str(a.learners), "--periods", str(a.periods), "--repeats", str(a.repeats),
               "--seed", str(a.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)  # a time-out or a failure ends the tool: nothing more is started on the GPU
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            return r.returncode
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                lines.append(l)
                print(l, flush=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
