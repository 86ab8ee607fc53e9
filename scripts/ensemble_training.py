#!/usr/bin/env python3
"""The reference's curriculum training (`Trainer.curriculum_training`: one env, one agent, update after every step) for many independent seeds at once,
one learner per GPU lane (dql_multirotor_landing_amd/ensemble.py).

    python scripts/ensemble_training.py --learners 4096 --seed 42 [--launched] [--levels 5] [--episodes 50000] [--score ENVS] --out run.npz
                                        [--per-learner [--advance-every E] [--drop-exhausted] [--max-periods N]] [--recipes FILE.json]
                                        [--envs-per-learner E [--team-nstep N] [--per-team [--advance-every E] [--drop-exhausted] [--max-periods N]]]
                                        [--score-map] [--preset reference|paper]
                                        [--score-grid FIELD=v1,v2,... [--score-grid ...]]
                                        [--refine FEATURE --refine-cut FILE.npy|FLOAT]

--launched: the parameters the reference's manager node ran with under roslaunch (config.as_launched_config) instead of the launch file's.
--score ENVS: after the curriculum, fly every learner's tables greedily where they live (SequentialEnsemble.landing_rates: ENVS envs per learner and flavour,
two launches), store `touchdown_rate` and `goal_hold_rate` in the .npz and print the share of learners at or above the acceptance bar of attempts.py (0.875
touchdowns), with the figures of the reference's published tables from the same call of `evaluation.landing_rates` (same envs, seed and episodes) beside it.
--score-map (with --score): the scoring launches also count where every learner's greedy policy flies (SequentialEnsemble.flight_maps).
The report gains, per flavour, the quantiles over learners of `evaluation.map_report`'s columns — baseline: the reference's tables from --reference-tables flown
by the same call, `trained_count`: the ensemble's own state_action_counter — per recipe too with --recipes, and the .npz gains `greedy_visits_simulation` and
`greedy_visits_training` (uint32 [learners, 2835]).
--preset paper (level-by-level driver only; default reference): train under evaluation.Q_PAPER with the paper's transfer order — on leaving level k, level k + 1
takes level k's tables times the reference's ratio of k + 1, nothing after the last level — the "paper" preset of DESIGN.md section 17(b).
--per-learner: every learner walks the levels by itself (ensemble.curriculum_per_learner) instead of waiting at each level for the slowest
learner of the ensemble; a learner advances at the next period index that is a multiple of E (--advance-every, default 4096); --drop-exhausted: a learner whose
episode budget ran out stays where it is instead of advancing as the reference's loop does.
--recipes FILE.json: several recipes in ONE ensemble (ensemble.curriculum_recipes; implies --per-learner).  The file is a list; an entry is
a preset name — "reference" (quirks 0x7f, the reference's transfer order) or "paper" (evaluation.Q_PAPER, the paper's order) — or an object with any of "preset"
(default "reference"), "name", "quirks", "transfer_order", "ratios", "last_level", "advance_exhausted", "alpha_table", "alpha_min", "nstep" (0..16: the recipe's
n-step target; default 0, the one-step update) and "levels": {"K": {"eps": [...],
"window", "min_successes", "max_episodes"}} for the levels that differ from the preset's.  Learners are dealt round-robin: recipe r gets the learners with
l % R == r.  With --score the landing-rate quantiles are reported per recipe.
--score-grid FIELD=v1,v2,... (repeatable, with --score): after the curriculum, every learner's tables are also scored where they live over the Cartesian product
of the given DqlConfig fields around the simulation flavour's config, all scenarios in one launch per slice of learners (SequentialEnsemble.score_grid, DESIGN.md
section 20).  The report gains `grid`: per scenario its label and the quantiles over learners of the touchdown rate, and the share of learners whose worst
scenario it is; the .npz gains `grid_touchdown_rate` [scenarios, learners] and `grid_touch_hist` [scenarios, learners, 8].
--envs-per-learner E: every learner owns a team of E envs (1, 2, 4, ..., 64) and applies the reference's update to their transitions in env order (DESIGN.md
section 17), so it collects E episodes in the time of one; --learners times E is at most 2^20.  Teams fly the level-by-level driver or, with --per-team, walk
the levels by themselves; they have no per-learner curriculum and no recipes: the flag is refused together with --per-learner and --recipes.
--per-team (with --envs-per-learner; E = 1 flies teams of one): every team walks the levels by itself (ensemble.curriculum_per_team) instead
of waiting at each level for the slowest team of the ensemble; a team advances at the next period index that is a multiple of E (--advance-every), all of its
envs re-entering through reset, and each launch carries the live teams only.  Works with --advance-every, --drop-exhausted, --max-periods, --team-nstep and
--preset paper (the config's quirk word becomes evaluation.Q_PAPER and the transfer order the paper's); refused together with --per-learner, --recipes and
--nstep.  The .npz records each team's level, the episodes it spent at each level and the period index at which it entered it.
--team-nstep N (with --envs-per-learner above 1): the team learners update with the uncorrected N-step Double-Q return, 1..16, one pending window per env, the
E transitions of a period still taken in env order (SequentialEnsemble.set_team_nstep); 0, the default, is the one-step team update.
Refused together with --nstep, --per-learner and --recipes; works with --per-team; N is recorded in the .npz as `team_nstep`.
--refine FEATURE --refine-cut FILE.npy|FLOAT (level-by-level driver only, with --preset reference or paper): every learner learns on the state split by one bit of
hidden state, half = FEATURE >= cut[state] (SequentialEnsemble.set_refinement).  FEATURE is a name of ops.SPLIT_FEATURES ("pitch_sp", "coin",
...); the cut is one number for every state or a float64 [945] array (scripts/simulation.py --cut-out writes one).  Refused together with --per-learner, --per-team,
--recipes, --nstep, --team-nstep, --envs-per-learner above 1, --score-map and --score-grid.  --score ENVS then flies the refined tables (score_refined), and the .npz
holds the refined tables [learners, 2, 2835], `refine_feature` and `refine_cut` instead of the plain tables.
Writes every learner's tables and, per level, its first-promotion episode (-1: the episode budget ran out first); with --per-learner also each learner's level,
the episodes it spent at each level and the period index at which it entered it."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dql_multirotor_landing_amd.config import F32, F64, Q_REFERENCE, as_launched_config, training_config  # noqa: E402
from dql_multirotor_landing_amd import evaluation  # noqa: E402
from dql_multirotor_landing_amd.ensemble import (LevelSchedule, NSTEP_MAX, ORDER_PAPER, ORDER_REFERENCE, REFERENCE_RATIOS, Recipe, SequentialEnsemble, TEAM_SIZES, curriculum,  # noqa: E402
                                                 curriculum_per_learner, curriculum_per_team, curriculum_recipes, exploration_rates, min_successes_for, train_level)

RECIPE_KEYS = {"preset", "name", "quirks", "transfer_order", "ratios", "last_level", "advance_exhausted", "alpha_table", "alpha_min", "levels", "nstep"}
LEVEL_KEYS = {"eps", "window", "min_successes", "max_episodes"}


def preset_recipe(name, episodes, last_level=4, advance_exhausted=True):
    """"reference": 0x7f with the reference's order; "paper": evaluation.Q_PAPER with the paper's; both with the reference's schedules and `episodes` per level"""
    if name not in ("reference", "paper"):
        raise ValueError(f"unknown preset {name!r}: reference or paper")
    levels = tuple(LevelSchedule(max_episodes=int(episodes)) for _ in range(5))
    if name == "reference":
        return Recipe(quirks=Q_REFERENCE, transfer_order=ORDER_REFERENCE, last_level=last_level, advance_exhausted=advance_exhausted, levels=levels)
    return Recipe(quirks=evaluation.Q_PAPER, transfer_order=ORDER_PAPER, last_level=last_level, advance_exhausted=advance_exhausted, levels=levels)


def load_recipes(path, episodes, last_level=4, advance_exhausted=True):
    """-> (names, recipes) of a --recipes file"""
    entries = json.loads(Path(path).read_text())
    if not isinstance(entries, list) or not 1 <= len(entries) <= 64:
        raise ValueError("a recipes file is a list of 1..64 recipes")
    names, recipes = [], []
    for i, e in enumerate(entries):
        if isinstance(e, str):
            e = {"preset": e, "name": e}
        if not isinstance(e, dict) or set(e) - RECIPE_KEYS:
            raise ValueError(f"recipe {i}: a preset name or an object with keys among {sorted(RECIPE_KEYS)}")
        r = preset_recipe(e.get("preset", "reference"), episodes, last_level, advance_exhausted)
        for k in ("quirks", "transfer_order", "ratios", "last_level", "advance_exhausted", "alpha_table", "alpha_min", "nstep"):
            if k in e:
                setattr(r, k, e[k])
        levels = list(r.levels)
        for k, lv in e.get("levels", {}).items():
            if not 0 <= int(k) < 5 or set(lv) - LEVEL_KEYS:
                raise ValueError(f"recipe {i}: levels are 0..4 with keys among {sorted(LEVEL_KEYS)}")
            levels[int(k)] = LevelSchedule(**{**vars(levels[int(k)]), **lv})
        r.levels = tuple(levels)
        names.append(e.get("name", f"recipe {i}"))
        recipes.append(r)
    return names, recipes


def deal(n, n_recipes):
    """round-robin: recipe r gets the learners with l % R == r"""
    return (np.arange(int(n)) % int(n_recipes)).astype(np.int32)


def curriculum_paper(ens, levels, max_episodes, on_level=None):
    """`ensemble.curriculum` with the paper's transfer order (tools/exp_teams.py's "paper" preset): -> per level, the counters at its end"""
    history = []
    for k in range(int(levels)):
        if k:
            ens.set_level(k)
        ens.set_schedules(eps=exploration_rates(k), window=100, min_successes=min_successes_for(100), max_episodes=max_episodes)
        flown = train_level(ens)
        c = ens.counters()
        history.append({"level": k, "periods": flown, "promotion_episode": c["promotion_episode"].copy(), "level_episodes": c["level_episodes"].copy()})
        if on_level is not None:
            on_level(ens, history[-1])
        if k < 4:
            ens.transfer(k + 1, REFERENCE_RATIOS[k + 1])
    return history


def rate_summary(x):
    x = np.asarray(x, dtype=np.float64)
    q = np.quantile(x, (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0))
    return {"mean": float(x.mean()), **{k: float(v) for k, v in zip(("min", "q05", "q25", "q50", "q75", "q95", "max"), q)}}


MAP_COLUMNS = ("decisions", "states_visited", "cells_visited", "occupancy_overlap", "disagreement_on_baseline", "disagreement_on_own", "untrained_share")
FLAVOURS = ("simulation", "training")


def flight_maps_sliced(ens, timing, **kw):
    """`ens.flight_maps` of all learners, at most ops.SCORE_MAP_MAX_TABLES per call: the slices' arrays joined, the kernel times summed"""
    from dql_multirotor_landing_amd.ops import SCORE_MAP_MAX_TABLES
    parts, ms, inst = [], 0.0, None
    for first in range(0, ens.n, SCORE_MAP_MAX_TABLES):
        t = {}
        parts.append(ens.flight_maps(first=first, count=min(SCORE_MAP_MAX_TABLES, ens.n - first), timing=t, **kw))
        ms, inst = ms + t["kernel_ms"], t["instance"]
    timing.update({"kernel_ms": ms, "instance": inst})
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("touchdown_rate", "goal_hold_rate", "simulation_by_code", "training_by_code", "simulation_visits", "training_visits")}
    out["columns"] = parts[0]["columns"]
    return out


def map_summary(rep, pick=None):
    """quantiles over (the picked) learners of every map_report column; a learner without a decision has NaN shares and is left out of them"""
    out = {}
    for col in MAP_COLUMNS:
        x = np.asarray(rep[col], dtype=np.float64)
        x = x if pick is None else x[pick]
        x = x[np.isfinite(x)]
        out[col] = None if x.size == 0 else rate_summary(x)
    return out


def maps_report(r, ens, a, kw):
    """-> ({flavour: map_report of every learner}, {flavour: map_report of the reference's tables against themselves}): baseline the reference's tables flown by
    the same call, trained_count the ensemble's own state_action_counter"""
    ref = Path(a.reference_tables)
    qa, qb = (np.load(ref / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
    base = evaluation.flight_maps(qa, qb, device=a.device, **kw)
    base_greedy = evaluation.greedy_actions(qa, qb)[0]
    tqa, tqb, count = ens.get_tables()
    greedy = evaluation.greedy_actions(tqa, tqb)
    mine = {f: evaluation.map_report(r[f"{f}_visits"], greedy, base[f"{f}_visits"][0], base_greedy, trained_count=count) for f in FLAVOURS}
    theirs = {f: evaluation.map_report(base[f"{f}_visits"], base_greedy[None], base[f"{f}_visits"][0], base_greedy) for f in FLAVOURS}
    return mine, theirs


def score_report(ens, a):
    """both landing rates of every learner (resident tables, two launches) and of the reference's tables, as one JSON-able dict + the two arrays + with
    --score-map the maps ({"report": {flavour: map_report}, "visits": {flavour: [learners, 2835]}}), else None"""
    level = a.levels - 1
    kw = dict(n_envs=a.score, episodes=a.score_episodes, level=level, seed=a.score_seed)
    t = {}
    r = flight_maps_sliced(ens, t, **kw) if a.score_map else ens.refined_landing_rates(timing=t, **kw) if a.refine is not None else ens.landing_rates(timing=t, **kw)
    td, gh = r["touchdown_rate"], r["goal_hold_rate"]
    rep = {"what": "ensemble_landing_rates", "learners": int(td.size), "envs_per_learner": a.score, "episodes_per_env": a.score_episodes, "level": level,
           "levels_trained": a.levels, "episode_budget_per_level": a.episodes, "launched": bool(a.launched), "seed": a.score_seed, "bar": evaluation.LANDING_BAR, "learners_at_or_above_bar": int((td >= evaluation.LANDING_BAR).sum()),
           "share_at_or_above_bar": float((td >= evaluation.LANDING_BAR).mean()), "touchdown_rate": rate_summary(td), "goal_hold_rate": rate_summary(gh),
           "unfinished_episodes": {"simulation": int(r["simulation_by_code"][:, -1].sum()), "training": int(r["training_by_code"][:, -1].sum())},
           "kernel_ms": t["kernel_ms"], "instance": t["instance"], "reference_tables": None}
    if a.refine is not None:
        rep["refine"] = {"feature": a.refine, "cut": a.refine_cut}
    ref = Path(a.reference_tables)
    if (ref / "Q_table_a.npy").exists() and (ref / "Q_table_b.npy").exists():
        qa, qb = (np.load(ref / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
        rr = evaluation.landing_rates(qa, qb, device=a.device, **kw)
        rep["reference_tables"] = {"touchdown_rate": float(rr["touchdown_rate"][0]), "goal_hold_rate": float(rr["goal_hold_rate"][0])}
    maps = None
    if a.score_map:
        mine, theirs = maps_report(r, ens, a, kw)
        rep["maps"] = {f: map_summary(mine[f]) for f in FLAVOURS}
        rep["reference_tables"]["maps"] = {f: {c: float(v[0]) for c, v in theirs[f].items()} for f in FLAVOURS}
        maps = {"report": mine, "visits": {f: r[f"{f}_visits"] for f in FLAVOURS}}
    return rep, td, gh, maps


def per_recipe_report(names, recipe_of, td, gh, summary):
    """the landing-rate quantiles and `SequentialEnsemble.recipe_summary` of every recipe's learners"""
    return [{"recipe": r, "name": name, **summary[r], "learners_at_or_above_bar": int((td[recipe_of == r] >= evaluation.LANDING_BAR).sum()),
             "touchdown_rate": rate_summary(td[recipe_of == r]), "goal_hold_rate": rate_summary(gh[recipe_of == r])} for r, name in enumerate(names)]


def grid_report(ens, a, quirks):
    """--score-grid: ({"labels", "touchdown_rate": [quantiles per scenario], "worst_share"}, rate [S, learners], touch_hist [S, learners, 8])"""
    from dql_multirotor_landing_amd.config import parse_grid_axes, scenario_grid, simulation_config
    from dql_multirotor_landing_amd.ops import SCORE_MAX_LANES
    base = simulation_config(working_curriculum_step=a.levels - 1, quirks=quirks, dtype=ens.cfg.dtype)
    cfgs, labels = scenario_grid(base, **parse_grid_axes(a.score_grid))
    per_call = max(1, SCORE_MAX_LANES // (len(cfgs) * a.score))  # learners per launch: scenarios x learners x envs <= 2^30
    parts = [ens.score_grid(cfgs, a.score, a.score_seed, episodes=a.score_episodes, first=first, count=min(per_call, ens.n - first)) for first in range(0, ens.n, per_call)]
    r = {f: np.concatenate([p[f] for p in parts], axis=1) for f in ("by_code", "steps_sum", "touch_hist")}
    t = evaluation.robustness_table(r, labels)
    q = lambda x: {f"q{int(100 * p):02d}": float(np.quantile(x, p)) for p in (0.05, 0.25, 0.5, 0.75, 0.95)}
    rep = {"labels": labels, "touchdown_rate": [q(t["rate"][s]) for s in range(len(cfgs))],
           "worst_share": (np.bincount(t["worst_scenario"], minlength=len(cfgs)) / ens.n).tolist()}
    return rep, t["rate"], r["touch_hist"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--learners", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--launched", action="store_true")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=50000, help="episode budget per level and learner")
    ap.add_argument("--f64", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--score", type=int, default=0, metavar="ENVS", help="fly every learner on ENVS envs per flavour after the curriculum (a multiple of 64; 0: do not)")
    ap.add_argument("--score-episodes", type=int, default=evaluation.DEFAULT_SCORE_EPISODES, help="episodes per env of the scoring run")
    ap.add_argument("--score-seed", type=int, default=123)
    ap.add_argument("--reference-tables", default=str(ROOT / "tests" / "golden" / "assets"), help="directory with the reference's Q_table_a.npy / Q_table_b.npy")
    ap.add_argument("--score-json", default=None, help="also write the scoring report to this file")
    ap.add_argument("--per-learner", action="store_true", help="every learner advances through the levels by itself")
    ap.add_argument("--advance-every", type=int, default=4096, metavar="E", help="with --per-learner: learners advance at the period indices that are multiples of E (1..4096)")
    ap.add_argument("--drop-exhausted", action="store_true", help="with --per-learner: a learner out of episodes stays frozen instead of advancing")
    ap.add_argument("--max-periods", type=int, default=None, help="with --per-learner or --recipes: stop after this many periods whoever is unfinished")
    ap.add_argument("--recipes", default=None, metavar="FILE.json", help="fly several recipes in one ensemble, dealt round-robin (implies --per-learner)")
    ap.add_argument("--envs-per-learner", type=int, default=1, metavar="E", help="envs per learner: 1, 2, 4, 8, 16, 32 or 64 (not with --per-learner / --recipes)")
    ap.add_argument("--score-map", action="store_true", help="with --score: also count where every learner's greedy policy flies, and report it against the reference's tables")
    ap.add_argument("--score-grid", action="append", default=[], metavar="FIELD=v1,v2,...", help="with --score: also score every learner over this grid of scenarios in one launch (repeatable)")
    ap.add_argument("--preset", default="reference", choices=["reference", "paper"], help="quirks and transfer order of the level-by-level driver (not with --per-learner / --recipes)")
    ap.add_argument("--nstep", type=int, default=0, metavar="N", help="n-step Double-Q targets, 1..16 (0: the reference's one-step update; not with --per-learner / --recipes / --envs-per-learner above 1; with --recipes give each recipe its own \"nstep\" in the file)")
    ap.add_argument("--team-nstep", type=int, default=0, metavar="N", help="with --envs-per-learner above 1: n-step Double-Q targets for the team learners, 1..16, one pending window per env (0: the one-step team update; not with --nstep / --per-learner / --recipes)")
    ap.add_argument("--per-team", action="store_true", help="every team advances through the levels by itself (with --envs-per-learner; takes --advance-every, --drop-exhausted, --max-periods, --team-nstep and --preset paper; not with --per-learner / --recipes / --nstep)")
    ap.add_argument("--refine", default=None, metavar="FEATURE", help="learn on the state split by FEATURE >= cut[state] (a name of ops.SPLIT_FEATURES; needs --refine-cut; level-by-level driver with one env per learner only)")
    ap.add_argument("--refine-cut", default=None, metavar="FILE.npy|FLOAT", help="with --refine: the cut, one number for every state or a float64 [945] array")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    refine_cut = None
    if (a.refine is None) != (a.refine_cut is None):
        ap.error("--refine FEATURE and --refine-cut FILE.npy|FLOAT go together")
    if a.refine is not None:
        for flag, on in (("--per-learner", a.per_learner), ("--per-team", a.per_team), ("--recipes", a.recipes), ("--nstep", a.nstep), ("--team-nstep", a.team_nstep),
                         ("--envs-per-learner above 1", a.envs_per_learner > 1), ("--score-map", a.score_map), ("--score-grid", a.score_grid)):
            if on:
                ap.error(f"--refine cannot be combined with {flag}: refined learners fly the level-by-level (barrier) driver with one env per learner and the one-step update, and are scored with score_refined")
        from dql_multirotor_landing_amd import ops
        try:
            ops.split_feature_code(a.refine)
            try:
                refine_cut = float(a.refine_cut)
            except ValueError:
                refine_cut = np.load(a.refine_cut)
            refine_cut = ops.split_cut_array(refine_cut)
        except (ValueError, OSError) as e:
            ap.error(f"--refine / --refine-cut: {e}")
    if a.per_team and a.per_learner:
        ap.error("--per-team cannot be combined with --per-learner: --per-learner is the plain ensemble's driver (one env per learner), --per-team the team ensemble's")
    if a.per_team and a.recipes:
        ap.error("--per-team cannot be combined with --recipes: teams have no recipes; --preset paper gives the team driver the paper's quirk word and transfer order")
    if a.per_team and a.nstep:
        ap.error("--per-team cannot be combined with --nstep: --nstep is the plain ensemble's switch; the team learners take --team-nstep")
    if a.preset != "reference" and (a.per_learner or a.recipes):
        ap.error("--preset belongs to the level-by-level driver: with --recipes name the preset in the recipes file")
    if a.score_map and not a.score:
        ap.error("--score-map needs --score ENVS: the maps are counted by the scoring launches")
    if a.score_grid and not a.score:
        ap.error("--score-grid needs --score ENVS: the grid flies ENVS envs per learner and scenario")
    if a.score_map and not all((Path(a.reference_tables) / f).exists() for f in ("Q_table_a.npy", "Q_table_b.npy")):
        ap.error("--score-map needs the baseline's tables: --reference-tables has no Q_table_a.npy / Q_table_b.npy")
    if a.envs_per_learner not in TEAM_SIZES:
        ap.error(f"--envs-per-learner must be one of {', '.join(map(str, TEAM_SIZES))}")
    if a.envs_per_learner > 1 and (a.per_learner or a.recipes):
        ap.error("--envs-per-learner above 1 cannot be combined with --per-learner or --recipes: teams fly the level-by-level (barrier) driver only")
    if not 0 <= a.nstep <= NSTEP_MAX:
        ap.error(f"--nstep must be in 0..{NSTEP_MAX}")
    if a.team_nstep and a.nstep:
        ap.error("--team-nstep cannot be combined with --nstep: --nstep is the plain ensemble's switch (one env per learner), --team-nstep the team ensemble's")
    if a.nstep and (a.per_learner or a.recipes or a.envs_per_learner > 1):
        ap.error("--nstep cannot be combined with --per-learner, --recipes or --envs-per-learner above 1: n-step targets fly the level-by-level (barrier) driver with one env per learner only")
    if not 0 <= a.team_nstep <= NSTEP_MAX:
        ap.error(f"--team-nstep must be in 0..{NSTEP_MAX}")
    if a.team_nstep and a.per_learner:
        ap.error("--team-nstep cannot be combined with --per-learner: teams fly the level-by-level (barrier) driver only")
    if a.team_nstep and a.recipes:
        ap.error("--team-nstep cannot be combined with --recipes: teams fly the level-by-level (barrier) driver only; give each recipe its own \"nstep\" in the file instead")
    if a.team_nstep and a.envs_per_learner < 2 and not a.per_team:
        ap.error("--team-nstep needs a team ensemble: give --envs-per-learner above 1 (with one env per learner use --nstep)")
    dtype = F64 if a.f64 else F32
    quirks = evaluation.Q_PAPER if a.preset == "paper" else Q_REFERENCE
    cfg = as_launched_config(dtype=dtype, quirks=quirks) if a.launched else training_config(0, dtype=dtype, quirks=quirks)
    ens = SequentialEnsemble(cfg, a.learners, seed=a.seed, device=a.device, max_episodes=a.episodes, envs_per_learner=a.envs_per_learner, nstep=a.nstep,
                             team_nstep=a.team_nstep, teams=True if a.per_team else None)
    try:
        if a.refine is not None:
            ens.set_refinement(a.refine, refine_cut)
        def report(e, h):
            p = h["promotion_episode"]
            print(json.dumps({"level": h["level"], "periods": h["periods"], "promoted": int((p >= 0).sum()), "of": int(p.size),
                              "median_promotion_episode": None if not (p >= 0).any() else int(np.median(p[p >= 0]))}), flush=True)
        extra = {}
        names = recipe_of = None

        def progress(e, flown):
            lv = e.levels()["level"]
            print(json.dumps({"periods": flown, "unfinished": e.n_unfinished(), "learners_per_level": np.bincount(lv, minlength=5).tolist()}), flush=True)
        if a.recipes:
            names, recipes = load_recipes(a.recipes, a.episodes, a.levels - 1, not a.drop_exhausted)
            recipe_of = deal(a.learners, len(recipes))
            h = curriculum_recipes(ens, recipes, recipe_of, advance_every=a.advance_every, max_periods=a.max_periods, on_chunk=progress)
            hist = [{"promotion_episode": h["promoted_at"][k], "periods": h["periods"]} for k in range(a.levels)]
            recipe_nstep = [int(r.nstep) for r in ens.recipes()[0]]  # as the library holds them
            extra = {"level": h["level"], "episodes_at": h["episodes_at"], "entered_period": h["entered_period"], "recipe_of": recipe_of,
                     "recipe_nstep": np.asarray(recipe_nstep, np.int32)}
        elif a.per_team:
            h = curriculum_per_team(ens, last_level=a.levels - 1, advance_every=a.advance_every, advance_exhausted=not a.drop_exhausted,
                                    transfer_order=ORDER_PAPER if a.preset == "paper" else ORDER_REFERENCE, max_episodes=a.episodes, max_periods=a.max_periods, on_chunk=progress)
            hist = [{"promotion_episode": h["promoted_at"][k], "periods": h["periods"]} for k in range(a.levels)]
            extra = {"level": h["level"], "episodes_at": h["episodes_at"], "entered_period": h["entered_period"], "per_team": np.int32(1)}
        elif a.per_learner:
            h = curriculum_per_learner(ens, last_level=a.levels - 1, advance_every=a.advance_every, advance_exhausted=not a.drop_exhausted, max_episodes=a.episodes,
                                       max_periods=a.max_periods, on_chunk=progress)
            hist = [{"promotion_episode": h["promoted_at"][k], "periods": h["periods"]} for k in range(a.levels)]
            extra = {"level": h["level"], "episodes_at": h["episodes_at"], "entered_period": h["entered_period"]}
        else:
            hist = (curriculum_paper(ens, a.levels, a.episodes, on_level=report) if a.preset == "paper" else
                    curriculum(ens, levels=a.levels, max_episodes=a.episodes, on_level=report))
        if a.score:
            rep, td, gh, maps = score_report(ens, a)
            extra.update({"touchdown_rate": td, "goal_hold_rate": gh})
            if names is not None:
                rep["recipes"] = per_recipe_report(names, recipe_of, td, gh, ens.recipe_summary())
                for entry, n in zip(rep["recipes"], recipe_nstep):
                    entry["nstep"] = n
                rep.update({"periods": int(h["periods"]), "unfinished": ens.n_unfinished()})
                if maps is not None:
                    for r, entry in enumerate(rep["recipes"]):
                        entry["maps"] = {f: map_summary(maps["report"][f], recipe_of == r) for f in FLAVOURS}
            if maps is not None:
                extra.update({f"greedy_visits_{f}": maps["visits"][f].astype(np.uint32) for f in FLAVOURS})
            if a.score_grid:
                rep["grid"], grid_rate, grid_touch = grid_report(ens, a, evaluation.Q_PAPER)
                extra.update({"grid_touchdown_rate": grid_rate, "grid_touch_hist": grid_touch})
            print(json.dumps(rep), flush=True)
            ref = rep["reference_tables"]
            print(f"{rep['learners_at_or_above_bar']} of {rep['learners']} learners ({100.0 * rep['share_at_or_above_bar']:.1f} %) reach a touchdown rate of "
                  f"{evaluation.LANDING_BAR}; median touchdown {rep['touchdown_rate']['q50']:.4f}, goal hold {rep['goal_hold_rate']['q50']:.4f}; the reference's tables: "
                  + ("not found" if ref is None else f"touchdown {ref['touchdown_rate']:.4f}, goal hold {ref['goal_hold_rate']:.4f}"), flush=True)
            if a.score_json:
                Path(a.score_json).write_text(json.dumps(rep) + "\n")
        if a.refine is not None:
            extra.update({"refine_feature": np.str_(ens.refinement()[0]), "refine_cut": ens.refinement()[1]})
        qa, qb, cnt = ens.get_refined_tables() if a.refine is not None else ens.get_tables()
        np.savez_compressed(a.out, Q_table_a=qa, Q_table_b=qb, state_action_counter=cnt, nstep=np.int32(a.nstep), team_nstep=np.int32(a.team_nstep), **extra,
                            promotion_episode=np.stack([h["promotion_episode"] for h in hist]), periods=np.array([h["periods"] for h in hist]))
    finally:
        ens.close()


if __name__ == "__main__":
    main()
