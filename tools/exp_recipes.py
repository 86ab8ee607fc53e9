#!/usr/bin/env python3
"""Per-learner recipes on the GPU: what one ensemble of R recipes costs against R ensembles flown one after another, and what four
recipes make of the as-launched curriculum.

    python tools/exp_recipes.py timing  [--recipes 4] [--learners-per-recipe 1024] [--periods 8192] [--advance-every 256] [--repeats 3]
                                        [--out profiles/ensemble_recipes_timing.jsonl]
    python tools/exp_recipes.py landing [--learners-per-recipe 1024] [--episodes 10000] [--advance-every 256] [--score 1024] [--max-periods N]
                                        [--out profiles/ensemble_recipes_landing.json]

timing: float32, `as_launched_config`, tables of zeros, R reference-order recipes that differ in quirks and ratios (so that the sequential way can fly each of
them through the calls that exist without recipes: one `SequentialEnsemble` of 1 024 learners per recipe with the recipe's quirks in its config,
`set_level_schedules` and `set_curriculum`, on k_learn_levels).  Both ways fly `--periods` periods and alternate in one process, `--repeats` times; per way the
median wall clock around the run calls and the median of the summed `dql_diag_ensemble_last` times (HIP events around each run call's launches) are written,
with the launches and waves x periods launched.

landing: scripts/ensemble_training.py --launched --recipes on four recipes dealt round-robin — the reference's; 0x7f with the paper's transfer order; Q_PAPER with
the paper's order; Q_PAPER with the paper's order and eps = 0.1 for a level's first 64 episodes above level 0 — then its --score report with the per-recipe
landing quantiles and the published tables' figures from the same call, written to --out.  The script runs as a child process."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dql_multirotor_landing_amd import _lib  # noqa: E402
from dql_multirotor_landing_amd.config import F32, as_launched_config  # noqa: E402
from dql_multirotor_landing_amd.ensemble import (LevelSchedule, REFERENCE_RATIOS, Recipe, SequentialEnsemble, exploration_rates, min_successes_for)  # noqa: E402

TIMING_QUIRKS = (0x7F, 0x40, 0x60, 0x7F)
TIMING_RATIOS = (REFERENCE_RATIOS, REFERENCE_RATIOS, REFERENCE_RATIOS, (0.75, 0.5, 1.25, 0.625, 0.875))
LANDING_RECIPES = ["reference",
                   {"name": "0x7f, paper order", "preset": "reference", "transfer_order": 1},
                   "paper",
                   {"name": "paper, eps 0.1 for 64 episodes above level 0", "preset": "paper", "levels": {str(k): {"eps": [0.1] * 64 + [0.0]} for k in (1, 2, 3, 4)}}]


def last_ms(ens):
    v = C.c_double()
    _lib.check(ens.lib.dql_diag_ensemble_last(ens._h, C.byref(v)))
    return float(v.value)


def timing_recipe(r, episodes):
    return Recipe(quirks=TIMING_QUIRKS[r % 4], ratios=TIMING_RATIOS[r % 4], levels=tuple(LevelSchedule(max_episodes=episodes) for _ in range(5)))


def fly(ens, periods, chunk):
    """-> (wall seconds around the run calls, summed device ms of the calls)"""
    wall, ms, flown = 0.0, 0.0, 0
    while flown < periods:
        k = min(chunk, periods - flown)
        t0 = time.perf_counter()
        ens.run(k)
        wall += time.perf_counter() - t0
        ms += last_ms(ens)
        flown += k
    return wall, ms


def one_timing(way, a):
    R, n, eps_budget = a.recipes, a.learners_per_recipe, 10000
    wall = ms = 0.0
    n_l = n_p = n_wp = decisions = 0
    if way == "one ensemble of R recipes":
        ens = SequentialEnsemble(as_launched_config(dtype=F32, quirks=0x7F), R * n, seed=a.seed)
        try:
            ens.set_curriculum(4, a.advance_every)
            ens.set_recipes([timing_recipe(r, eps_budget) for r in range(R)], np.arange(R * n) % R)
            wall, ms = fly(ens, a.periods, a.chunk)
            n_l, n_p, n_wp = ens.launches()
            decisions = int(ens.counters()["decisions"].sum())
            assert ens.index_faults() == 0
        finally:
            ens.close()
    else:
        for r in range(R):
            rec = timing_recipe(r, eps_budget)
            ens = SequentialEnsemble(as_launched_config(dtype=F32, quirks=rec.quirks), n, seed=a.seed)
            try:
                for k in range(5):
                    ens.set_level_schedules(k, exploration_rates(k), 100, min_successes_for(100), eps_budget)
                ens.set_curriculum(4, a.advance_every, rec.ratios)
                w, m = fly(ens, a.periods, a.chunk)
                wall += w; ms += m
                l, p, wp = ens.launches()
                n_l += l; n_p += p; n_wp += wp
                decisions += int(ens.counters()["decisions"].sum())
                assert ens.index_faults() == 0
            finally:
                ens.close()
    return {"wall_s": wall, "device_ms": ms, "launches": n_l, "periods_launched": n_p, "wave_periods_launched": n_wp, "decisions": decisions}


def timing(a):
    ways = ("one ensemble of R recipes", "R ensembles one after another")
    runs = {w: [] for w in ways}
    for _ in range(a.repeats):
        for w in ways:
            runs[w].append(one_timing(w, a))
            print(json.dumps({"way": w, **runs[w][-1]}), flush=True)
    med = {w: statistics.median(x["wall_s"] for x in runs[w]) for w in ways}
    with open(a.out, "a") as f:
        for w in ways:
            r = runs[w]
            mid = sorted(r, key=lambda x: x["wall_s"])[len(r) // 2]
            row = {"what": "R recipes x learners_per_recipe learners, float32, as_launched_config, tables of zeros, reference-order recipes", "way": w, "recipes": a.recipes,
                   "learners_per_recipe": a.learners_per_recipe, "periods": a.periods, "advance_every": a.advance_every, "run_call_periods": a.chunk, "repeats": a.repeats,
                   "wall_s_median": round(med[w], 4), "wall_s_all": [round(x["wall_s"], 4) for x in r],
                   "device_ms_median": round(statistics.median(x["device_ms"] for x in r), 2), "device_ms_all": [round(x["device_ms"], 2) for x in r],
                   "wall_ratio_sequential_over_recipes": round(med[ways[1]] / med[ways[0]], 3),
                   "method": "ways alternating in one process; wall clock around the dql_ensemble_run calls only; device ms = HIP events around each call's launches, summed",
                   **{k: v for k, v in mid.items() if k not in ("wall_s", "device_ms")}}
            f.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)


def landing(a):
    with tempfile.TemporaryDirectory() as tmp:
        rf, sj, out = Path(tmp) / "recipes.json", Path(tmp) / "score.json", Path(tmp) / "run.npz"
        rf.write_text(json.dumps(LANDING_RECIPES))
        cmd = [sys.executable, str(ROOT / "scripts" / "ensemble_training.py"), "--learners", str(4 * a.learners_per_recipe), "--launched", "--recipes", str(rf), "--episodes", str(a.episodes),
               "--advance-every", str(a.advance_every), "--score", str(a.score), "--score-json", str(sj), "--out", str(out)]
        if a.max_periods:
            cmd += ["--max-periods", str(a.max_periods)]
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True)
        wall = time.perf_counter() - t0
        rep = json.loads(sj.read_text())
    rep.update({"what": "ensemble_recipes_landing", "command": "scripts/ensemble_training.py " + " ".join(Path(c).name if "/" in c else c for c in cmd[2:]), "recipes_file": LANDING_RECIPES,
                "advance_every": a.advance_every, "max_periods": a.max_periods, "wall_s": round(wall, 1)})
    Path(a.out).write_text(json.dumps(rep, indent=1) + "\n")
    for r in rep["recipes"]:
        print(json.dumps({k: r[k] for k in ("name", "members", "learners_per_level", "promoted_per_level", "finished", "learners_at_or_above_bar")} | {"touchdown": r["touchdown_rate"], "goal_hold": r["goal_hold_rate"]}), flush=True)
    print("reference tables:", rep["reference_tables"], "wall", rep["wall_s"], "s", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("timing", "landing"))
    ap.add_argument("--recipes", type=int, default=4)
    ap.add_argument("--learners-per-recipe", type=int, default=1024)
    ap.add_argument("--periods", type=int, default=8192)
    ap.add_argument("--chunk", type=int, default=4096, help="periods per dql_ensemble_run call")
    ap.add_argument("--advance-every", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=10000)
    ap.add_argument("--score", type=int, default=1024)
    ap.add_argument("--max-periods", type=int, default=None)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or str(ROOT / "profiles" / ("ensemble_recipes_timing.jsonl" if a.what == "timing" else "ensemble_recipes_landing.json"))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    (timing if a.what == "timing" else landing)(a)


if __name__ == "__main__":
    main()
