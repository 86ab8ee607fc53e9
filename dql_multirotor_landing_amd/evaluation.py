"""Greedy evaluation of a set of tables on the engine: the counterpart of the reference's `scripts/simulation.py` loop (load tables, fly landing
episodes, count how they end — SURVEY.md section 8 f2) for a whole batch of envs at once.

`first_episode_outcomes` is the harness (`scripts/simulation.py` and bench.py report with it); `landing_score` is the two figures the repo quotes for a
set of tables: the touchdown rate in `SimulationLandingEnv`'s world (pkg/landing_simulation_env.py:285-428: descent at -0.4 m/s from z = 4 m, an episode
ends on the platform, outside the fly zone or on the ground) and the goal-hold rate in `TrainingLandingEnv`'s (:167-283, the world the promotion rule judges)."""
from __future__ import annotations

import numpy as np

from . import ops
from .config import CHECK_NAMES, F32, Q_PAPER, simulation_config, training_config
from .engine import Engine

METHODS = ("stepwise", "rollout")


def _flavour_config(flavour: str, level: int, dtype, cfg_kw):
    dtype = F32 if dtype is None else dtype
    if flavour == "simulation":
        return simulation_config(working_curriculum_step=level, dtype=dtype, **cfg_kw)
    if flavour == "training":
        return training_config(level, dtype=dtype, **cfg_kw)
    raise ValueError("flavour must be 'simulation' or 'training'")


def _histogram(code):
    hist = {CHECK_NAMES[k]: int((code == k).sum()) for k in range(len(CHECK_NAMES))}
    hist["unfinished"] = int((code < 0).sum())
    return hist


def first_episode_outcomes(tables, n_envs: int = 4096, level: int = 4, max_steps: int = 600, seed: int = 123, dtype=None, flavour: str = "simulation",
                           device=0, method: str = "stepwise", **cfg_kw):
    """Greedy roll-outs of `tables` = (Q_table_a, Q_table_b, state_action_counter), flat and padded as `DoubleQLearningAgent._padded()` returns them;
    the terminal histogram of the FIRST episode of every env (+ "unfinished").  `method`: "stepwise" (one launch and one read-back per agent period, the
    yardstick) or "rollout" (one launch for all episodes, `rollout_outcomes`): the same histogram."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}")
    if method == "rollout":
        return rollout_outcomes(tables, n_envs, level, max_steps, seed, dtype, flavour, device, **cfg_kw)
    cfg = _flavour_config(flavour, level, dtype, cfg_kw)
    eng = Engine(cfg, n_envs, seed=seed, device=device)
    try:
        eng.set_tables(*tables)
        first_code = np.full(n_envs, -1, dtype=np.int64)
        eng.eval_steps(1)  # reset period
        for _ in range(max_steps):
            eng.eval_steps(1)
            d, c = eng.dones()
            new = (d != 0) & (first_code < 0)
            first_code[new] = c[new]
            if (first_code >= 0).all():
                break
    finally:
        eng.close()
    return _histogram(first_code)


def landing_score(tables, n_envs: int = 4096, level: int = 4, seed: int = 123, dtype=None, device=0, quirks: int = Q_PAPER, method: str = "stepwise"):
    """{"touchdown_rate", "goal_hold_rate"} of `n_envs` greedy first episodes each (the figures of bench.py's `stage4_greedy_4096_episodes`)"""
    h = first_episode_outcomes(tables, n_envs, level, seed=seed, dtype=dtype, flavour="simulation", device=device, method=method, quirks=quirks)
    g = first_episode_outcomes(tables, n_envs, level, seed=seed, dtype=dtype, flavour="training", device=device, method=method, quirks=quirks)
    return {"touchdown_rate": h["TERMINAL_CONTACT"] / n_envs, "goal_hold_rate": g["TERMINAL_SUCCESS"] / n_envs}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the roll-out operator (ops.rollout, include/dql.h dql_rollout): all first episodes in ONE launch, for several table sets, with a record per episode
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def rollout_records(list_of_tables, n_envs: int = 4096, level: int = 4, max_steps: int = 600, seed: int = 123, dtype=None, flavour: str = "simulation",
                    device=0, trace_envs: int = 0, timing: dict = None, **cfg_kw):
    """`ops.rollout` on the config of `flavour` / `level`: the per-episode records of every table set, arrays [n_tables, n_envs]"""
    cfg = _flavour_config(flavour, level, dtype, cfg_kw)
    return ops.rollout(cfg, list_of_tables, n_envs, seed, max_steps=max_steps, trace_envs=trace_envs, device=device, timing=timing)


def rollout_outcomes(tables, n_envs: int = 4096, level: int = 4, max_steps: int = 600, seed: int = 123, dtype=None, flavour: str = "simulation",
                     device=0, **cfg_kw):
    """`first_episode_outcomes`' histogram (same keys, "unfinished" included) from one launch of the roll-out operator"""
    rec = rollout_records([tables], n_envs, level, max_steps, seed, dtype, flavour, device, **cfg_kw)
    return _histogram(rec["code"][0])


def landing_scores(list_of_tables, n_envs: int = 4096, level: int = 4, seed: int = 123, dtype=None, device=0, quirks: int = Q_PAPER, timing: dict = None):
    """`landing_score` of up to 16 table sets in two launches, one per flavour: a list of {"touchdown_rate", "goal_hold_rate"}.  Every set is scored on
    the same episodes (paired).  `timing`: a dict that receives the two launches' `kernel_ms` (summed) and `instance` names."""
    list_of_tables = list(list_of_tables)
    ts, tt = {}, {}
    sim = rollout_records(list_of_tables, n_envs, level, seed=seed, dtype=dtype, flavour="simulation", device=device, timing=ts, quirks=quirks)
    trn = rollout_records(list_of_tables, n_envs, level, seed=seed, dtype=dtype, flavour="training", device=device, timing=tt, quirks=quirks)
    if timing is not None:
        timing["kernel_ms"] = ts["kernel_ms"] + tt["kernel_ms"]
        timing["instance"] = [ts["instance"], tt["instance"]]
    contact, success = CHECK_NAMES.index("TERMINAL_CONTACT"), CHECK_NAMES.index("TERMINAL_SUCCESS")
    return [{"touchdown_rate": int((sim["code"][k] == contact).sum()) / n_envs, "goal_hold_rate": int((trn["code"][k] == success).sum()) / n_envs}
            for k in range(len(list_of_tables))]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the scoring operator (ops.score, include/dql.h dql_score): any number of table sets, several episodes per env, counts only
# ---------------------------------------------------------------------------------------------------------------------------------------------------
LANDING_BAR = 0.875  # attempts.py's acceptance bar on the touchdown rate
# episodes per env of the scripts: lane re-use against fresh lanes is measured in profiles/score_timing.jsonl
DEFAULT_SCORE_EPISODES = 1


def landing_rates_with(score_fn, n_envs: int = 4096, episodes: int = 1, level: int = 4, seed: int = 123, dtype=None, quirks: int = Q_PAPER, max_steps: int = 600,
                       timing: dict = None):
    """the two launches of `landing_rates`, one per flavour, through `score_fn(cfg, n_envs, seed, episodes, max_steps, timing)` -> a score result"""
    ts, tt = {}, {}
    sim = score_fn(_flavour_config("simulation", level, dtype, {"quirks": quirks}), n_envs, seed, episodes, max_steps, ts)
    trn = score_fn(_flavour_config("training", level, dtype, {"quirks": quirks}), n_envs, seed, episodes, max_steps, tt)
    if timing is not None:
        timing["kernel_ms"] = ts["kernel_ms"] + tt["kernel_ms"]
        timing["instance"] = [ts["instance"], tt["instance"]]
    return {"touchdown_rate": ops.rates_from_counts(sim["by_code"], "TERMINAL_CONTACT"), "goal_hold_rate": ops.rates_from_counts(trn["by_code"], "TERMINAL_SUCCESS"),
            "simulation_by_code": sim["by_code"], "training_by_code": trn["by_code"], "columns": sim["columns"]}


def landing_rates(qa, qb, n_envs: int = 4096, episodes: int = 1, level: int = 4, seed: int = 123, dtype=None, device=0, quirks: int = Q_PAPER, max_steps: int = 600,
                  timing: dict = None):
    """`landing_scores`' two figures for K table sets (`qa`, `qb`: [K, 2835]), K up to 2^20, in two launches, one per flavour: a dict with `touchdown_rate` [K]
    and `goal_hold_rate` [K] — the share of the n_envs * episodes episodes per set that ended in TERMINAL_CONTACT in the simulation flavour and in
    TERMINAL_SUCCESS in the training flavour — and the two count tables.  With episodes = 1 these are `landing_scores`' numbers."""
    return landing_rates_with(lambda cfg, n, sd, ep, ms, t: ops.score(cfg, qa, qb, n, sd, episodes=ep, max_steps=ms, device=device, timing=t),
                              n_envs, episodes, level, seed, dtype, quirks, max_steps, timing)


QUANTILES = (0.05, 0.5, 0.95)


def _quantiles(x):
    x = np.asarray(x, dtype=np.float64)
    return None if x.size == 0 else {f"q{int(round(100 * q)):02d}": float(v) for q, v in zip(QUANTILES, np.quantile(x, QUANTILES))}


def episode_report(records):
    """What the first episodes looked like at their end, per table set (pure numpy; `records`: what `ops.rollout` / `rollout_records` return, arrays
    [n_tables, n_envs] or [n_envs]).  A list of dicts: `histogram` (terminal codes + "unfinished"), `steps` and `return` (cumulative reward, both axes) with
    their 5 / 50 / 95 % quantiles over the finished episodes, and `touchdown`: over the TERMINAL_CONTACT episodes, the quantiles of `offset` = hypot(px -
    mp_x, py - mp_y), of `rel_speed` = hypot(vx - mp_u, vy - mp_v) and of `sink_rate` = -vz, with their count `n` — None when no episode touched down."""
    code = np.atleast_2d(np.asarray(records["code"]))
    get = lambda f: np.atleast_2d(np.asarray(records[f], dtype=np.float64))
    contact = CHECK_NAMES.index("TERMINAL_CONTACT")
    out = []
    for k in range(code.shape[0]):
        fin, td = code[k] >= 0, code[k] == contact
        rep = {"histogram": _histogram(code[k]), "steps": _quantiles(get("steps")[k][fin]), "return": _quantiles((get("cum_x")[k] + get("cum_y")[k])[fin]), "touchdown": None}
        if td.any():
            rep["touchdown"] = {"n": int(td.sum()),
                                "offset": _quantiles(np.hypot(get("px")[k] - get("mp_x")[k], get("py")[k] - get("mp_y")[k])[td]),
                                "rel_speed": _quantiles(np.hypot(get("vx")[k] - get("mp_u")[k], get("vy")[k] - get("mp_v")[k])[td]),
                                "sink_rate": _quantiles(-get("vz")[k][td])}
        out.append(rep)
    return out
