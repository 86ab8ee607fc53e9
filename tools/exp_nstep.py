#!/usr/bin/env python3
"""Sequential learners with n-step targets on the GPU: what the new kernel costs, and whether its learners land better.

    python tools/exp_nstep.py timing [--out profiles/nstep_timing.jsonl]
    python tools/exp_nstep.py findings [--learners 1024] [--episodes 50000] [--seeds 42 43] [--out profiles/nstep_findings.jsonl]
    python tools/exp_nstep.py recipes-timing [--out profiles/nstep_recipes_timing.jsonl]
    python tools/exp_nstep.py recipes [--learners 1024] [--episodes 50000] [--seeds 42 43] [--out profiles/nstep_recipes_findings.jsonl]

timing: tools/exp_ensemble.py timing's protocol (level 0, eps = 1, no freeze, 512 periods a run, one warm-up run, then 7 timed runs) for four variants that
alternate in one process per shape: k_learn (n = 0) and k_learn_nstep at n = 1, 4 and 16; 64, 4 096 and 65 536 learners, float32 and float64.  The yardstick
is k_learn in the same session.  Per variant: the median, smallest and largest of the HIP-event time of the call and of its wall clock.
findings: per n in 1, 2, 4, 8, 16 and per seed, `--learners` learners of the paper preset (quirks 0x40, as_launched_config, float32) through the level-by-level
curriculum of scripts/ensemble_training.py --preset paper with `--episodes` episodes per level; then `landing_rates` on 1 024 envs for every learner and
`returns_map` (eps 0.1, gamma 0.99) with `value_calibration` for the first 16.  One process per (n, seed), `--parallel` of them at a time; a failure or a time-out ends the tool.
recipes-timing: timing's protocol on a single-recipe ensemble in curriculum mode (advance_every 4 096, last_level 0, so nobody advances and
the 8 x 512 periods of a variant are cut nowhere): k_learn_recipes (the recipe's n = 0) and k_learn_recipes_nstep at n = 1, 4 and 16; the yardstick is
k_learn_recipes in the same session and process.
recipes (section 23): findings' question in ONE ensemble per seed: recipes n = 1, 2, 4, 8, 16 of the paper preset dealt round-robin over 5 x `--learners` learners,
every learner walking the levels by itself (`ensemble.curriculum_recipes`, advance_every 4 096); then `landing_rates` on 1 024 envs for every learner, reported per
recipe.  One process per seed, `--parallel` of them at a time."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [(dtype, L) for dtype in ("float32", "float64") for L in (64, 4096, 65536)]
VARIANTS = (0, 1, 4, 16)
PERIODS, RUNS = 512, 7
FINDINGS_N = (1, 2, 4, 8, 16)
SCORE_ENVS, RETURNS_LEARNERS, RETURNS_ENVS, RETURNS_EPISODES, EPS, GAMMA, MAX_STEPS, LANDING_BAR = 1024, 16, 4096, 4, 0.1, 0.99, 600, 0.875


def spread(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x)}


def timing_child(a):
    import ctypes as C
    from dql_multirotor_landing_amd import _lib
    from dql_multirotor_landing_amd.config import F32, F64, training_config
    from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
    dtype = F64 if a.dtype == "float64" else F32
    ens = {n: SequentialEnsemble(training_config(0, dtype=dtype), a.learners, seed=1, eps=[1.0], max_episodes=1 << 30, window=100, min_successes=101, nstep=n) for n in VARIANTS}
    try:
        def run(e):
            ms = C.c_double()
            t0 = time.perf_counter(); e.run(PERIODS); w = time.perf_counter() - t0
            _lib.check(e.lib.dql_diag_ensemble_last(e._h, C.byref(ms)))
            return ms.value, w * 1e3
        for e in ens.values():
            run(e)
        kern, wall = {n: [] for n in VARIANTS}, {n: [] for n in VARIANTS}
        for _ in range(RUNS):
            for n, e in ens.items():  # the variants alternate: a drift of the machine reaches all of them
                k, w = run(e)
                kern[n].append(k); wall[n].append(w)
        base = statistics.median(kern[0])
        for n, e in ens.items():
            k = spread(kern[n])
            print(json.dumps({"what": "SequentialEnsemble.run", "kernel": "k_learn" if n == 0 else "k_learn_nstep", "nstep": n, "dtype": a.dtype, "learners": a.learners,
                              "periods_per_run": PERIODS, "runs": RUNS, "event_ms": k, "wall_ms": spread(wall[n]), "us_per_period": round(k["median"] / PERIODS * 1e3, 3),
                              "over_k_learn_same_session": round(k["median"] / base, 4), "k_learn_spread_max_over_min": round(max(kern[0]) / min(kern[0]), 4),
                              "decisions_so_far": int(e.counters()["decisions"].sum()), "open_windows": int((e.pending_lengths() > 0).sum()), "index_faults": e.index_faults(),
                              "method": "one warm-up run, then 7 runs of 512 periods, the four variants alternating in one process"}), flush=True)
    finally:
        for e in ens.values():
            e.close()


def recipes_timing_child(a):
    import ctypes as C
    from dql_multirotor_landing_amd import _lib
    from dql_multirotor_landing_amd.config import F32, F64, training_config
    from dql_multirotor_landing_amd.ensemble import MAX_ADVANCE_EVERY, LevelSchedule, Recipe, SequentialEnsemble
    dtype = F64 if a.dtype == "float64" else F32
    cfg = training_config(0, dtype=dtype)
    levels = tuple(LevelSchedule(eps=(1.0,), window=100, min_successes=101, max_episodes=1 << 30) for _ in range(5))
    ens = {}
    for n in VARIANTS:
        e = SequentialEnsemble(cfg, a.learners, seed=1)
        e.set_curriculum(4, MAX_ADVANCE_EVERY)
        e.set_recipes([Recipe(quirks=cfg.quirks, last_level=0, levels=levels, nstep=n)], np.zeros(a.learners, np.int32))
        ens[n] = e
    try:
        def run(e):
            ms = C.c_double()
            t0 = time.perf_counter(); e.run(PERIODS); w = time.perf_counter() - t0
            _lib.check(e.lib.dql_diag_ensemble_last(e._h, C.byref(ms)))
            return ms.value, w * 1e3
        for e in ens.values():
            run(e)
        kern, wall = {n: [] for n in VARIANTS}, {n: [] for n in VARIANTS}
        for _ in range(RUNS):
            for n, e in ens.items():  # the variants alternate: a drift of the machine reaches all of them
                k, w = run(e)
                kern[n].append(k); wall[n].append(w)
        base = statistics.median(kern[0])
        for n, e in ens.items():
            k = spread(kern[n])
            print(json.dumps({"what": "SequentialEnsemble.run, one recipe", "kernel": "k_learn_recipes" if n == 0 else "k_learn_recipes_nstep", "nstep": n, "dtype": a.dtype,
                              "learners": a.learners, "periods_per_run": PERIODS, "runs": RUNS, "event_ms": k, "wall_ms": spread(wall[n]),
                              "us_per_period": round(k["median"] / PERIODS * 1e3, 3), "over_k_learn_recipes_same_session": round(k["median"] / base, 4),
                              "k_learn_recipes_spread_max_over_min": round(max(kern[0]) / min(kern[0]), 4), "decisions_so_far": int(e.counters()["decisions"].sum()),
                              "open_windows": int((e.pending_lengths() > 0).sum()), "index_faults": e.index_faults(),
                              "method": "one warm-up run, then 7 runs of 512 periods, the four variants alternating in one process"}), flush=True)
    finally:
        for e in ens.values():
            e.close()


def recipes_child(a):
    from dql_multirotor_landing_amd.config import F32, Q_PAPER, as_launched_config
    from dql_multirotor_landing_amd.ensemble import ORDER_PAPER, LevelSchedule, Recipe, SequentialEnsemble, curriculum_recipes
    R = len(FINDINGS_N)
    n_learners = R * a.learners
    recipes = [Recipe(quirks=Q_PAPER, transfer_order=ORDER_PAPER, levels=tuple(LevelSchedule(max_episodes=a.episodes) for _ in range(5)), nstep=n) for n in FINDINGS_N]
    of = (np.arange(n_learners) % R).astype(np.int32)
    ens = SequentialEnsemble(as_launched_config(dtype=F32, quirks=Q_PAPER), n_learners, seed=a.seed, max_episodes=a.episodes)
    try:
        t0 = time.perf_counter()

        def progress(e, flown):
            print(f"seed {a.seed}: {flown} periods, {e.n_unfinished()} unfinished, {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
        h = curriculum_recipes(ens, recipes, of, max_periods=a.max_periods, on_chunk=progress)
        train_s = time.perf_counter() - t0
        summary = ens.recipe_summary()
        rates = ens.landing_rates(n_envs=SCORE_ENVS)
        q = lambda x: {k: float(v) for k, v in zip(("min", "q05", "q25", "q50", "q75", "q95", "max"), np.quantile(x, (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)))}
        for r, n in enumerate(FINDINGS_N):
            td, gh = rates["touchdown_rate"][of == r], rates["goal_hold_rate"][of == r]
            print(json.dumps({"what": "nstep_recipes_landing", "nstep": n, "recipe": r, "seed": a.seed, "learners": int((of == r).sum()), "learners_in_the_ensemble": n_learners,
                              "episodes_per_level": a.episodes, "preset": "paper (quirks 0x40, the paper's order), as_launched_config, float32", "advance_every": 4096,
                              "periods": int(h["periods"]), "unfinished_in_the_ensemble": ens.n_unfinished(), "train_s_of_the_ensemble": round(train_s, 1), **summary[r],
                              "score_envs": SCORE_ENVS, "touchdown_rate": q(td), "goal_hold_rate": q(gh), "share_at_or_above_0.875": float((td >= LANDING_BAR).mean()),
                              "learners_at_or_above_0.875": int((td >= LANDING_BAR).sum()), "index_faults": ens.index_faults()}), flush=True)
    finally:
        ens.close()


def curriculum_paper(ens, levels, max_episodes):
    """scripts/ensemble_training.py's level-by-level driver for --preset paper: Q[k+1] = Q[k] ratios[k+1] on entering level k + 1"""
    from dql_multirotor_landing_amd.ensemble import REFERENCE_RATIOS, exploration_rates, min_successes_for, train_level
    history = []
    for k in range(levels):
        if k:
            ens.set_level(k)
        ens.set_schedules(eps=exploration_rates(k), window=100, min_successes=min_successes_for(100), max_episodes=max_episodes)
        flown = train_level(ens)
        p = ens.counters()["promotion_episode"]
        history.append({"level": k, "periods": int(flown), "promoted": int((p >= 0).sum())})
        if k < 4:
            ens.transfer(k + 1, REFERENCE_RATIOS[k + 1])
    return history


def findings_child(a):
    from dql_multirotor_landing_amd import evaluation
    from dql_multirotor_landing_amd.config import F32, Q_PAPER, as_launched_config
    from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
    ens = SequentialEnsemble(as_launched_config(dtype=F32, quirks=Q_PAPER), a.learners, seed=a.seed, max_episodes=a.episodes, nstep=a.nstep)
    try:
        t0 = time.perf_counter()
        history = curriculum_paper(ens, 5, a.episodes)
        train_s = time.perf_counter() - t0
        rates = ens.landing_rates(n_envs=SCORE_ENVS)
        td, gh = rates["touchdown_rate"], rates["goal_hold_rate"]
        q = lambda x: {k: float(v) for k, v in zip(("min", "q05", "q25", "q50", "q75", "q95", "max"), np.quantile(x, (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)))}
        row = {"what": "nstep_landing", "nstep": a.nstep, "seed": a.seed, "learners": a.learners, "episodes_per_level": a.episodes, "preset": "paper (quirks 0x40), as_launched_config, float32",
               "levels": history, "train_s": round(train_s, 1), "score_envs": SCORE_ENVS, "touchdown_rate": q(td), "goal_hold_rate": q(gh),
               "share_at_or_above_0.875": float((td >= LANDING_BAR).mean()), "learners_at_or_above_0.875": int((td >= LANDING_BAR).sum()), "index_faults": ens.index_faults()}
        print(json.dumps(row), flush=True)
        k = min(RETURNS_LEARNERS, a.learners)
        qa, qb, _ = ens.get_tables(0, k)
        for flavour in ("training", "simulation"):
            cfg = evaluation._flavour_config(flavour, 4, F32, {"quirks": Q_PAPER})
            r = ens.returns_map(cfg, RETURNS_ENVS, seed=123, eps=EPS, gamma=GAMMA, episodes=RETURNS_EPISODES, max_steps=MAX_STEPS, count=k)
            cal = [evaluation.value_calibration(qa[i], qb[i], r["visits"][i], r["return_fx"][i])["summary"]["mean"] for i in range(k)]
            by_level = lambda key: [None if all(np.isnan(c[key][lv]) for c in cal) else float(np.nanmean([c[key][lv] for c in cal])) for lv in range(5)]
            print(json.dumps({"what": "nstep_value_calibration", "nstep": a.nstep, "seed": a.seed, "flavour": flavour, "learners": k, "envs": RETURNS_ENVS, "episodes_per_env": RETURNS_EPISODES,
                              "eps": EPS, "gamma": GAMMA, "min_visits": 30, "tables": "(Q_table_a + Q_table_b) / 2", "mean_over_learners_of": "visit-weighted figures per learner",
                              "mean_bias": float(np.nanmean([c["mean_bias"] for c in cal])), "rms_bias": float(np.nanmean([c["rms_bias"] for c in cal])),
                              "mean_bias_by_level": by_level("mean_bias_by_level"), "rms_bias_by_level": by_level("rms_bias_by_level")}), flush=True)
    finally:
        ens.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "findings", "recipes-timing", "recipes"])
    ap.add_argument("--max-periods", type=int, default=None, help="recipes: stop after this many periods whoever is unfinished")
    ap.add_argument("--out", default=None)
    ap.add_argument("--learners", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=50000, help="findings: episode budget per level and learner (scripts/ensemble_training.py's default)")
    ap.add_argument("--seeds", type=int, nargs="+", default=[42, 43])
    ap.add_argument("--parallel", type=int, default=1, help="findings: children that fly at the same time (at most 16)")
    ap.add_argument("--timeout", type=int, default=None, help="seconds a child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dtype", default="float32", help=argparse.SUPPRESS)
    ap.add_argument("--nstep", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--seed", type=int, default=42, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return {"timing": timing_child, "findings": findings_child, "recipes-timing": recipes_timing_child, "recipes": recipes_child}[a.what](a)
    import __graft_entry__ as g
    g.build_hip()
    me = [sys.executable, str(Path(__file__).resolve()), a.what, "--child"]
    if a.what in ("timing", "recipes-timing"):
        jobs = [me + ["--dtype", dtype, "--learners", str(L)] for dtype, L in SHAPES]
    elif a.what == "recipes":
        jobs = [me + ["--seed", str(s), "--learners", str(a.learners), "--episodes", str(a.episodes)] + (["--max-periods", str(a.max_periods)] if a.max_periods else []) for s in a.seeds]
    else:
        jobs = [me + ["--nstep", str(n), "--seed", str(s), "--learners", str(a.learners), "--episodes", str(a.episodes)] for s in a.seeds for n in FINDINGS_N]
    timeout = a.timeout or (300 if a.what.endswith("timing") else 3000)
    names = {"timing": "nstep_timing.jsonl", "findings": "nstep_findings.jsonl", "recipes-timing": "nstep_recipes_timing.jsonl", "recipes": "nstep_recipes_findings.jsonl"}
    out = Path(a.out or ROOT / "profiles" / names[a.what])
    out.parent.mkdir(parents=True, exist_ok=True)
    lines = []
    k = max(1, a.parallel if a.what in ("findings", "recipes") else 1)
    for first in range(0, len(jobs), k):
        # findings: 1 024 learners are 16 waves, so `--parallel` children share the device (at most 16 processes may hold it); a time-out or a failure ends
        # the tool once the children already started are over: nothing more is started on the GPU
        procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None if a.what == "recipes" else subprocess.PIPE, text=True) for cmd in jobs[first:first + k]]
        deadline, failed = time.monotonic() + timeout, []
        for cmd, p in zip(jobs[first:first + k], procs):
            try:
                so, se = p.communicate(timeout=max(1.0, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                p.kill()
                so, se = p.communicate()
                failed.append(f"{' '.join(cmd[2:])} timed out after {timeout} s")
                continue
            if p.returncode != 0:
                failed.append(f"{' '.join(cmd[2:])} failed with status {p.returncode}:\n{(se or '')[-4000:]}")
                continue
            rows = [ln for ln in so.splitlines() if ln.startswith("{")]
            print("\n".join(rows), flush=True)
            lines += rows
        out.write_text("".join(ln + "\n" for ln in lines))  # kept as it grows: a later child's failure does not lose the earlier rows
        if failed:
            sys.exit("\n".join(failed))


if __name__ == "__main__":
    main()
