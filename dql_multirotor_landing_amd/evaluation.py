"""Greedy evaluation of a set of tables on the engine: the counterpart of the reference's `scripts/simulation.py` loop (load tables, fly landing
episodes, count how they end — SURVEY.md section 8 f2) for a whole batch of envs at once.

`first_episode_outcomes` is the harness (`scripts/simulation.py` and bench.py report with it); `landing_score` is the two figures the repo quotes for a
set of tables: the touchdown rate in `SimulationLandingEnv`'s world (pkg/landing_simulation_env.py:285-428: descent at -0.4 m/s from z = 4 m, an episode
ends on the platform, outside the fly zone or on the ground) and the goal-hold rate in `TrainingLandingEnv`'s (:167-283, the world the promotion rule judges)."""
from __future__ import annotations

import numpy as np

from . import ops
from .config import CHECK_NAMES, F32, N_CELLS, Q_PAPER, TARGET_FRAC_BITS, simulation_config, training_config
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


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the mapping scorer (ops.score_map, include/dql.h dql_score_map): where the greedy policies fly, and what can be read from the maps (pure numpy below)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
N_STATES = N_CELLS // 3


def flight_maps_with(score_map_fn, n_envs: int = 4096, episodes: int = 1, level: int = 4, seed: int = 123, dtype=None, quirks: int = Q_PAPER, max_steps: int = 600,
                     timing: dict = None):
    """`landing_rates_with` through `score_map_fn(cfg, n_envs, seed, episodes, max_steps, timing)` -> a score-map result: its dict plus `simulation_visits` and
    `training_visits` int64 [K, 2835], and `simulation_log` / `training_log` = (ep_code, ep_last_cell) of the flavour, or None where the function kept no log"""
    kept = []

    def fn(cfg, n, sd, ep, ms, t):
        kept.append(score_map_fn(cfg, n, sd, ep, ms, t))
        return kept[-1]

    out = landing_rates_with(fn, n_envs, episodes, level, seed, dtype, quirks, max_steps, timing)
    for flavour, r in zip(("simulation", "training"), kept):
        out[f"{flavour}_visits"] = r["visits"]
        out[f"{flavour}_log"] = None if r["ep_last_cell"] is None else (r["ep_code"], r["ep_last_cell"])
    return out


def flight_maps(qa, qb, n_envs: int = 4096, episodes: int = 1, level: int = 4, seed: int = 123, dtype=None, device=0, quirks: int = Q_PAPER, max_steps: int = 600,
                log: bool = False, timing: dict = None):
    """`landing_rates` of K table sets (K up to ops.SCORE_MAP_MAX_TABLES) with both flavours' maps, in two launches (see `flight_maps_with`)"""
    return flight_maps_with(lambda cfg, n, sd, ep, ms, t: ops.score_map(cfg, qa, qb, n, sd, episodes=ep, max_steps=ms, log=log, device=device, timing=t),
                            n_envs, episodes, level, seed, dtype, quirks, max_steps, timing)


def greedy_actions(qa, qb):
    """the greedy action of every state of K table sets (`qa`, `qb`: [K, 2835] or [2835]): int64 [K, 945].  `agent_predict`'s rule: the means of the two tables,
    the first maximum wins (a later action needs a strictly greater mean)."""
    qa, qb = np.atleast_2d(np.asarray(qa, dtype=np.float64)), np.atleast_2d(np.asarray(qb, dtype=np.float64))
    if qa.ndim != 2 or qa.shape[1] != N_CELLS or qb.shape != qa.shape:
        raise ValueError("qa and qb must be [K, 2835] arrays of the same K")
    m = ((qa + qb) / 2).reshape(len(qa), N_STATES, 3)
    k = np.zeros(m.shape[:2], np.int64)
    v = m[..., 0]
    b = m[..., 1] > v
    k[b] = 1
    v = np.where(b, m[..., 1], v)
    k[m[..., 2] > v] = 2
    return k


def _state_shares(visits):
    """(decisions [K], p [K, 945]): every state's share of its set's visits, the three actions summed; NaN rows where a set has no decision"""
    per_state = np.asarray(visits, dtype=np.float64).reshape(-1, N_STATES, 3).sum(axis=2)
    total = per_state.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return total, per_state / total[:, None]


def map_report(visits, greedy, base_visits, base_greedy, trained_count=None):
    """What K maps say against a baseline's (pure numpy).  `visits` [K, 2835] and `greedy` [K, 945] (`greedy_actions`) of the table sets, `base_visits` [2835] and
    `base_greedy` [945] of the baseline.  Returns a dict of [K] arrays:
      decisions, states_visited, cells_visited   totals of the map
      occupancy_overlap          1 - 1/2 sum_s |p_k(s) - p_base(s)|, p = the state's share of the set's visits (actions summed)
      disagreement_on_baseline   sum_s p_base(s) [greedy_k(s) != greedy_base(s)]: the share of the baseline's flight spent where set k would act otherwise
      disagreement_on_own        the same sum weighted with p_k
      untrained_share            only with `trained_count` [K, 2835]: the share of the set's decisions made at cells whose count is 0
    A set (or a baseline) without a decision has NaN shares."""
    visits = np.atleast_2d(np.asarray(visits, dtype=np.int64))
    greedy = np.atleast_2d(np.asarray(greedy))
    base_visits = np.asarray(base_visits, dtype=np.int64).reshape(-1)
    base_greedy = np.asarray(base_greedy).reshape(-1)
    K = len(visits)
    if visits.shape[1] != N_CELLS or greedy.shape != (K, N_STATES) or base_visits.shape != (N_CELLS,) or base_greedy.shape != (N_STATES,):
        raise ValueError("visits [K, 2835], greedy [K, 945], base_visits [2835], base_greedy [945]")
    decisions, p = _state_shares(visits)
    base_total, pb = _state_shares(base_visits[None])
    differs = greedy != base_greedy[None]
    nan_if_empty = lambda x, empty: np.where(empty, np.nan, x)
    no_k, no_b = decisions == 0, bool(base_total[0] == 0)
    with np.errstate(invalid="ignore"):
        out = {"decisions": visits.sum(axis=1), "states_visited": (visits.reshape(K, N_STATES, 3).sum(axis=2) > 0).sum(axis=1), "cells_visited": (visits > 0).sum(axis=1),
               "occupancy_overlap": nan_if_empty(1.0 - 0.5 * np.abs(np.nan_to_num(p) - np.nan_to_num(pb)).sum(axis=1), no_k | no_b),
               "disagreement_on_baseline": nan_if_empty((np.nan_to_num(pb) * differs).sum(axis=1), no_b),
               "disagreement_on_own": nan_if_empty((np.nan_to_num(p) * differs).sum(axis=1), no_k)}
    if trained_count is not None:
        trained_count = np.atleast_2d(np.asarray(trained_count))
        if trained_count.shape != (K, N_CELLS):
            raise ValueError("trained_count must be [K, 2835]")
        with np.errstate(invalid="ignore", divide="ignore"):
            out["untrained_share"] = nan_if_empty((visits * (trained_count == 0)).sum(axis=1) / decisions, no_k)
    return out


def failure_origins(ep_code, ep_last_cell, codes, n_tables: int):
    """int64 [n_tables, 2835]: the histogram of the last x cells (`ep_last_cell[0]`) of the finished episodes whose terminal code is among `codes` (numbers or
    CHECK_NAMES).  `ep_code` [episodes, n_tables * envs], `ep_last_cell` [2, episodes, n_tables * envs] as `ops.score_map(log=True)` returns them."""
    ep_code, cells = np.asarray(ep_code), np.asarray(ep_last_cell)
    if ep_code.ndim != 2 or cells.shape != (2,) + ep_code.shape or n_tables < 1 or ep_code.shape[1] % n_tables:
        raise ValueError("ep_code [episodes, n_tables * envs] and ep_last_cell [2, episodes, n_tables * envs]")
    codes = [CHECK_NAMES.index(c) if isinstance(c, str) else int(c) for c in codes]
    n = ep_code.shape[1] // n_tables
    x = cells[0].astype(np.int64)
    pick = np.isin(ep_code, codes) & (x != ops.NO_CELL)
    if (x[pick] >= N_CELLS).any():
        raise ValueError("a last cell lies outside the table")
    out = np.zeros((n_tables, N_CELLS), np.int64)
    _, col = np.nonzero(pick)
    np.add.at(out, (col // n, x[pick]), 1)
    return out


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


# the empirical transition model (ops.transition_model, include/dql.h dql_model): what can be read from its tables (pure numpy below)
def _model_arrays(pairs, terminal):
    pairs, terminal = np.asarray(pairs), np.asarray(terminal)
    if pairs.shape != (N_CELLS, N_STATES) or terminal.ndim != 2 or terminal.shape[0] != N_CELLS:
        raise ValueError("pairs [2835, 945] and terminal [2835, codes] of ONE table set")
    return pairs.astype(np.float64), terminal.astype(np.float64)


def solve_model(pairs, reward_fx, terminal, gamma: float, min_visits: int = 1, tol: float = 1e-9, max_iter: int = 100000):
    """Value iteration on the empirical model of one table set: `pairs` [2835, 945], `reward_fx` [2835], `terminal` [2835, codes] as `ops.transition_model`
    returns them.  A cell is SOLVED if it was visited at least `min_visits` (>= 1) times; for those
        Q(c) = mean reward(c) + gamma * sum_s' P(s' | c) * max over the solved actions a' of Q(s', a'),
    P(s' | c) = pairs[c, s'] / visits[c]: a transition that ended the episode bootstraps nothing (the paper's mask: bootstrap unless done), and a state none
    of whose actions is solved has value 0.  Iterated from 0 until no Q moves by more than `tol`, `max_iter` sweeps at most.  Unsolved cells get min(solved Q) - 1,
    so that a greedy flight never prefers them.  Returns (Q float64 [2835], solved bool [2835])."""
    p, t = _model_arrays(pairs, terminal)
    reward_fx = np.asarray(reward_fx, dtype=np.float64).reshape(-1)
    if reward_fx.shape != (N_CELLS,) or min_visits < 1 or not 0.0 <= gamma <= 1.0:
        raise ValueError("reward_fx [2835], min_visits >= 1, gamma in [0, 1]")
    visits = p.sum(axis=1) + t.sum(axis=1)
    solved = visits >= min_visits
    safe = np.where(solved, visits, 1.0)
    r = np.where(solved, reward_fx / float(1 << TARGET_FRAC_BITS) / safe, 0.0)
    P = np.where(solved[:, None], p / safe[:, None], 0.0)
    by_state = solved.reshape(N_STATES, 3)
    q = np.zeros(N_CELLS)
    for _ in range(int(max_iter)):
        v = np.where(by_state, q.reshape(N_STATES, 3), -np.inf).max(axis=1)
        v = np.where(by_state.any(axis=1), v, 0.0)
        new = np.where(solved, r + gamma * (P @ v), 0.0)
        moved = float(np.abs(new - q).max())
        q = new
        if moved <= tol:
            break
    floor = (q[solved].min() if solved.any() else 0.0) - 1.0
    return np.where(solved, q, floor), solved


def model_divergence(pairs_a, terminal_a, pairs_b, terminal_b, min_visits: int = 1):
    """float64 [2835]: per cell the total-variation distance 1/2 sum |P_a - P_b| between the next-outcome distributions of two models of one table shape, the
    945 next states and the terminal codes taken as one alphabet.  NaN where either side has fewer than `min_visits` (>= 1) visits.  0: the two behaviour
    policies saw the same thing happen after that (state, action); 1: disjoint outcomes."""
    pa, ta = _model_arrays(pairs_a, terminal_a)
    pb, tb = _model_arrays(pairs_b, terminal_b)
    if ta.shape != tb.shape or min_visits < 1:
        raise ValueError("both terminal tables [2835, codes] with the same codes, min_visits >= 1")
    a, b = np.concatenate([pa, ta], axis=1), np.concatenate([pb, tb], axis=1)
    va, vb = a.sum(axis=1), b.sum(axis=1)
    ok = (va >= min_visits) & (vb >= min_visits)
    tv = 0.5 * np.abs(a / np.where(ok, va, 1.0)[:, None] - b / np.where(ok, vb, 1.0)[:, None]).sum(axis=1)
    return np.where(ok, tv, np.nan)


# the transition model split by a hidden variable (ops.split_model, include/dql.h dql_model_split): pure numpy readers of its result
SPLIT_FRAC_BITS = 20  # include/dql.h DQL_SPLIT_FRAC_BITS


def _state_visits(result):
    pairs, terminal = np.asarray(result["pairs"]), np.asarray(result["terminal"])
    if pairs.ndim != 4 or pairs.shape[1:] != (2, N_CELLS, N_STATES) or terminal.ndim != 4 or terminal.shape[:3] != pairs.shape[:3]:
        raise ValueError("a split-model result: pairs [K, 2, 2835, 945] and terminal [K, 2, 2835, codes]")
    visits = pairs.sum(axis=-1, dtype=np.int64) + terminal.sum(axis=-1, dtype=np.int64)  # [K, 2, 2835]
    return visits, visits.sum(axis=1).reshape(len(visits), N_STATES, 3).sum(axis=-1)


def feature_means(result):
    """float64 [K, 945]: per state the mean of the split feature over the counted decisions taken in it, feat_sum_fx / 2^20 / visits of the state.  An unvisited
    state gets +inf, which is a valid cut (nothing is in its half 1)."""
    _, sv = _state_visits(result)
    fs = np.asarray(result["feat_sum_fx"])
    if fs.shape != sv.shape:
        raise ValueError("feat_sum_fx [K, 945]")
    return np.where(sv > 0, fs.astype(np.float64) / float(1 << SPLIT_FRAC_BITS) / np.where(sv > 0, sv, 1), np.inf)


STATES_PER_LEVEL = N_STATES // 5  # a state's curriculum level is idx_x // 189


def refinement_cut(results_by_level):
    """float64 [945]: the cut of `SequentialEnsemble.set_refinement` from one `ops.split_model` pass per curriculum level (cut = +inf, any eps), merged.  Level k's
    block of states [189 k, 189 (k + 1)) takes the per-state means of the split feature from level k's pass, pooled over its table sets:
    sum feat_sum_fx / 2^20 / sum visits.  A state that is unvisited at its own level stays at +inf (nothing is in its half 1).  `results_by_level`: {level: result}
    or a sequence indexed by level; a level without a pass keeps +inf throughout."""
    items = results_by_level.items() if hasattr(results_by_level, "items") else enumerate(results_by_level)
    cut = np.full(N_STATES, np.inf)
    for k, result in items:
        k = int(k)
        if not 0 <= k < N_STATES // STATES_PER_LEVEL:
            raise ValueError(f"a curriculum level is in 0..4, not {k}")
        if result is None:
            continue
        _, sv = _state_visits(result)
        fs = np.asarray(result["feat_sum_fx"])
        if fs.shape != sv.shape:
            raise ValueError("feat_sum_fx [K, 945]")
        fs, sv = fs.sum(axis=0, dtype=np.int64), sv.sum(axis=0, dtype=np.int64)
        blk = slice(k * STATES_PER_LEVEL, (k + 1) * STATES_PER_LEVEL)
        cut[blk] = np.where(sv[blk] > 0, fs[blk].astype(np.float64) / float(1 << SPLIT_FRAC_BITS) / np.where(sv[blk] > 0, sv[blk], 1), np.inf)
    return cut


def split_divergence(result, min_visits: int = 30):
    """float64 [K, 2835]: per cell the total-variation distance between the next-outcome distributions of the two halves (`model_divergence` of half 0 against
    half 1: next states and terminal codes as one alphabet).  NaN where either half has fewer than `min_visits` (>= 1) visits."""
    _state_visits(result)
    pairs, terminal = np.asarray(result["pairs"]), np.asarray(result["terminal"])
    return np.stack([model_divergence(pairs[k, 0], terminal[k, 0], pairs[k, 1], terminal[k, 1], min_visits) for k in range(len(pairs))])


def _weighted_quantile(x, w, q):
    """the smallest x at which the cumulative weight reaches q of the total (x, w 1-d, w > 0)"""
    order = np.argsort(x, kind="stable")
    x, cw = x[order], np.cumsum(w[order])
    return float(x[min(int(np.searchsorted(cw, q * cw[-1], side="left")), len(x) - 1)])


def aliasing_table(by_feature, coin, min_visits: int = 30):
    """One row per feature: is it hidden state of the discretised MDP?  `by_feature`: name -> the `ops.split_model` result taken at that feature's mean cut;
    `coin`: the coin's result over the same flights (cut 0.5).  All table sets of a result are read together.  A cell is COMPARED for a feature if both halves
    have `min_visits` under the feature AND under the coin, so that both distances are taken over the same cells.  Per feature a dict:
      cells             cells compared
      median            the visit-weighted median distance between the feature's halves over them (the smallest distance at which the cumulative visits reach half)
      coin_median       the coin's, weighted the same way over the same cells
      coin_p95          the coin's 95th percentile over the same cells (unweighted, numpy's linear interpolation)
      above_coin_p95    the share of the compared cells whose distance lies above coin_p95
      half1_share       the share of all counted decisions that fell in half 1
    NaN where no cell is compared.  A variable is hidden state if its halves lie further apart than the coin's do."""
    d_coin = split_divergence(coin, min_visits).ravel()
    out = {}
    for name, r in by_feature.items():
        visits, _ = _state_visits(r)
        d = split_divergence(r, min_visits).ravel()
        if d.shape != d_coin.shape:
            raise ValueError(f"{name}: as many table sets as the coin's result")
        both = ~np.isnan(d) & ~np.isnan(d_coin)
        w = visits.sum(axis=1).ravel()[both].astype(np.float64)
        row = {"cells": int(both.sum()), "half1_share": float(visits[:, 1].sum() / max(int(visits.sum()), 1))}
        if row["cells"]:
            p95 = float(np.percentile(d_coin[both], 95))
            row.update(median=_weighted_quantile(d[both], w, 0.5), coin_median=_weighted_quantile(d_coin[both], w, 0.5), coin_p95=p95,
                       above_coin_p95=float((d[both] > p95).mean()))
        else:
            row.update(median=float("nan"), coin_median=float("nan"), coin_p95=float("nan"), above_coin_p95=float("nan"))
        out[name] = row
    return out


def format_aliasing_table(table):
    """the rows of `aliasing_table` as text, one line per feature"""
    lines = [f"{'feature':<12} {'cells':>6} {'median':>8} {'coin med':>9} {'coin p95':>9} {'> p95':>7} {'half 1':>7}"]
    for name, r in table.items():
        lines.append(f"{name:<12} {r['cells']:>6d} {r['median']:>8.4f} {r['coin_median']:>9.4f} {r['coin_p95']:>9.4f} {r['above_coin_p95']:>7.3f} {r['half1_share']:>7.3f}")
    return "\n".join(lines)


def value_calibration(qa, qb, visits, return_fx, greedy=None, min_visits: int = 30):
    """The tables' values held against the realised returns of `ops.returns_map` (one table set), pure numpy.  `qa`, `qb`: float64 [2835]; `visits`, `return_fx`:
    int64 [2835]; `greedy`: the tables' greedy action per state, [945] (ops' predict), or None.  Returns a dict.  Per cell, float64 [2835]:
      mean_return                  return_fx / visits / 2^26, NaN below `min_visits` (>= 1) visits
      bias_a, bias_b, bias_mean    Q - mean_return for `qa`, `qb` and (qa + qb) / 2: positive = the table overestimates
    and under `summary`, for each of "a", "b" and "mean", over the cells that have `min_visits`, weighted by their visits:
      mean_bias, rms_bias                    floats (NaN if no cell qualifies)
      mean_bias_by_level, rms_bias_by_level  float64 [5], by curriculum level cell // 567 (NaN for a level without such a cell)
      overestimated_share                    the visit share of the cells whose bias is positive
    plus `cells` (how many qualify) and `visits` (their visits).  With `greedy`: `agreement_states`, the states in which the greedy action and at least one
    other action have `min_visits`, and `agreement_share`, the share of those in which the arg-max of the mean returns over the actions that qualify is the
    greedy action (NaN if no state qualifies)."""
    qa, qb = (np.asarray(t, dtype=np.float64).ravel() for t in (qa, qb))
    visits, return_fx = (np.asarray(t, dtype=np.int64).ravel() for t in (visits, return_fx))
    if not (qa.shape == qb.shape == visits.shape == return_fx.shape == (N_CELLS,)) or min_visits < 1 or (visits < 0).any():
        raise ValueError("qa, qb, visits and return_fx must be [2835] (one table set), visits >= 0, min_visits >= 1")
    ok = visits >= min_visits
    mean_return = np.where(ok, return_fx / np.where(ok, visits, 1) / float(1 << TARGET_FRAC_BITS), np.nan)
    out = {"mean_return": mean_return, "bias_a": qa - mean_return, "bias_b": qb - mean_return, "bias_mean": 0.5 * (qa + qb) - mean_return}
    level = np.arange(N_CELLS) // 567
    w = np.where(ok, visits, 0).astype(np.float64)

    def weighted(bias, sel):
        tot = w[sel].sum()
        if tot <= 0.0:
            return float("nan"), float("nan")
        b = np.where(ok, bias, 0.0)[sel]
        return float((w[sel] * b).sum() / tot), float(np.sqrt((w[sel] * b * b).sum() / tot))

    summary = {"cells": int(ok.sum()), "visits": int(visits[ok].sum())}
    everything = np.ones(N_CELLS, bool)
    for name in ("a", "b", "mean"):
        bias = out[f"bias_{name}"]
        mean_bias, rms_bias = weighted(bias, everything)
        per_level = [weighted(bias, level == k) for k in range(N_CELLS // 567)]
        over = float(w[ok & (np.where(ok, bias, 0.0) > 0.0)].sum() / w.sum()) if w.sum() > 0.0 else float("nan")
        summary[name] = {"mean_bias": mean_bias, "rms_bias": rms_bias, "mean_bias_by_level": np.array([p[0] for p in per_level]),
                         "rms_bias_by_level": np.array([p[1] for p in per_level]), "overestimated_share": over}
    if greedy is not None:
        greedy = np.asarray(greedy, dtype=np.int64).ravel()
        if greedy.shape != (N_CELLS // 3,) or (greedy < 0).any() or (greedy > 2).any():
            raise ValueError("greedy must be [945] actions in 0..2")
        ok3, m3 = ok.reshape(-1, 3), np.where(ok, mean_return, -np.inf).reshape(-1, 3)
        states = np.arange(N_CELLS // 3)
        compared = ok3[states, greedy] & (ok3.sum(axis=1) >= 2)
        summary["agreement_states"] = int(compared.sum())
        summary["agreement_share"] = float((m3.argmax(axis=1) == greedy)[compared].mean()) if compared.any() else float("nan")
    out["summary"] = summary
    return out


def robustness_table(result, labels, column: str = "TERMINAL_CONTACT"):
    """What an `ops.score_grid` result says per (scenario, table set), pure numpy.  `result`: a dict with `by_code` [S, K, len(ops.SCORE_COLUMNS)], `steps_sum`
    [S, K] and, optionally, `touch_hist` [S, K, 8]; `labels`: one label per scenario (`config.scenario_grid`'s dicts).  Returns a dict of float64 [S, K] arrays:
      rate        the share of all episodes asked for that ended with `column`
      mean_steps  the mean length of the finished episodes (NaN where none finished)
      unfinished  the share of episodes that did not finish
      touch_centre / touch_outside  the share of touchdowns in bins 0 - 1 (within a quarter of the platform's width of its centre) and in bins >= 4 (beyond the
                  half extent); NaN where nothing touched down, None without `touch_hist`
    and per table set `worst_scenario` int64 [K] (the first scenario with the smallest rate), `worst_rate` [K] and `worst_label` (a list of K labels)."""
    by_code = np.asarray(result["by_code"], dtype=np.int64); steps_sum = np.asarray(result["steps_sum"], dtype=np.int64)
    if by_code.ndim != 3 or by_code.shape[2] != len(ops.SCORE_COLUMNS) or steps_sum.shape != by_code.shape[:2]:
        raise ValueError(f"by_code must be [S, K, {len(ops.SCORE_COLUMNS)}] and steps_sum [S, K]")
    S, K = steps_sum.shape
    if len(labels) != S:
        raise ValueError(f"{len(labels)} labels for {S} scenarios")
    total = by_code.sum(axis=2)
    if (total <= 0).any():
        raise ValueError("a row of by_code counts no episode")
    unfinished = by_code[:, :, -1]
    finished = total - unfinished
    rate = by_code[:, :, ops.SCORE_COLUMNS.index(column)] / total
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"rate": rate, "mean_steps": np.where(finished > 0, steps_sum / np.where(finished > 0, finished, 1), np.nan), "unfinished": unfinished / total,
               "touch_centre": None, "touch_outside": None}
        if result.get("touch_hist") is not None:
            touch = np.asarray(result["touch_hist"], dtype=np.int64)
            if touch.shape != (S, K, ops.GRID_TOUCH_BINS):
                raise ValueError(f"touch_hist must be [S, K, {ops.GRID_TOUCH_BINS}]")
            n = touch.sum(axis=2)
            den = np.where(n > 0, n, 1)
            out["touch_centre"] = np.where(n > 0, touch[:, :, :2].sum(axis=2) / den, np.nan)
            out["touch_outside"] = np.where(n > 0, touch[:, :, 4:].sum(axis=2) / den, np.nan)
    worst = rate.argmin(axis=0)
    out.update(worst_scenario=worst.astype(np.int64), worst_rate=rate[worst, np.arange(K)], worst_label=[labels[int(s)] for s in worst], column=column)
    return out
