"""Shared by the transition-model tests (CPU emulation and GPU): the stepwise yardstick of `dql_model` / `dql_ensemble_model` (include/dql.h) and the cases.

`stepwise_model` is the equality contract spelled out with the unchanged oracle: ONE `Oracle(cfg, n, seed)` stepped with EXTERNAL actions, the action words
of all envs from `oracle.philox_n([(j_lo, j_hi, i, STREAM_ACTION)], (seed_lo, seed_hi))`, the explored action `(w[1] * 3) >> 32` where `(w[0] >> 8) <
eps_thr(eps)`, the greedy one from `oracle.agent_predict` on the set's tables elsewhere (tests/ensemble_checks.py `Reference.run`, vectorised).  An env counts in
a period as in `map_checks.stepwise_map`: fewer than `episodes` episodes finished before it, FL_WAS_RESET clear after it.  It knows nothing of the kernel.  It
also counts the events a kernel can get wrong (`events`), so that every case can assert, before anything else is looked at, that what it is there for occurred."""
import numpy as np

from dql_multirotor_landing_amd.config import CHECK_NAMES, F32, F64, N_CELLS, Q_PAPER, Q_REFERENCE, TARGET_FRAC_BITS, simulation_config, training_config
from oracle import oracle as orc
from oracle.oracle import Oracle

import ensemble_checks as ec
import rollout_checks as rc

N_STATES = N_CELLS // 3          # 945
N_CODES = len(CHECK_NAMES)
N_COLS = N_CODES + 1             # by_code: the terminal codes, then "unfinished"
CELLS_PER_LEVEL, STATES_PER_LEVEL = 567, 189
FL_DONE, FL_WAS_RESET = 1, 8     # dql_device.hpp
STREAM_ACTION = 0
NON_TERMINAL_SUCCESS = CHECK_NAMES.index("NON_TERMINAL_SUCCESS")
SEED = 11
FIELDS = ("pairs", "reward_fx", "terminal", "by_code", "steps_sum", "visits")


def _stage4():
    return rc.stage4_tables()


def _zeros():
    return np.zeros(N_CELLS), np.zeros(N_CELLS)


def _threshold_eps():
    """case E's eps: k / 2^24 with k the draw (w[0] >> 8) of an env in period 1 — the first decision of every env, which no eps can have changed — whose
    explored action is not its greedy one.  eps_thr(eps) is then exactly k: that env's draw EQUALS the threshold, the rule `<` flies it greedily, and a rule
    `<=` would explore.  Among the envs that qualify, the one with the smallest draw."""
    c = CASES["E"]
    cfg, (qa, qb), n = c["cfg"](), c["tables"](), c["n"]
    o = Oracle(cfg, n, seed=SEED)
    o.step(np.full(n, 2, np.uint8))  # period 0: every env goes through reset
    _, ints = o.get_fields()
    s = ints[o.field_names(True).index("idx_x")]
    ctr = np.zeros((n, 4), np.uint32); ctr[:, 0] = 1; ctr[:, 2] = np.arange(n); ctr[:, 3] = STREAM_ACTION
    w = orc.philox_n(ctr, (SEED & 0xffffffff, (SEED >> 32) & 0xffffffff))
    differs = ((w[:, 1].astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int64) != orc.agent_predict(qa, qb, s).astype(np.int64)
    k = int((w[:, 0] >> 8)[differs].min())
    assert 0 < k < 1 << 24 and ec.eps_thr(k / 16777216.0) == k
    return k / 16777216.0


# id -> config, tables, eps (or a function that gives it), envs, max_steps, episodes
CASES = {
    "A": dict(cfg=lambda: simulation_config(working_curriculum_step=4, dtype=F32, quirks=Q_PAPER), tables=_stage4, eps=0.1, n=128, max_steps=320, episodes=2),
    "B": dict(cfg=lambda: training_config(4, dtype=F32, quirks=Q_PAPER), tables=_stage4, eps=0.1, n=128, max_steps=300, episodes=2),
    "B64": dict(cfg=lambda: training_config(4, dtype=F64, quirks=Q_PAPER), tables=_stage4, eps=0.1, n=64, max_steps=300, episodes=2),
    "C": dict(cfg=lambda: training_config(0, dtype=F32, quirks=Q_REFERENCE), tables=_zeros, eps=1.0, n=192, max_steps=120, episodes=3),
    "D": dict(cfg=lambda: training_config(2, dtype=F32, quirks=Q_PAPER), tables=_stage4, eps=0.0, n=64, max_steps=300, episodes=1),
    # beyond the issue's four: a draw that equals the threshold (1 in 2^24 by chance; here by the choice of eps), which is what tells `<` from `<=`
    "E": dict(cfg=lambda: simulation_config(working_curriculum_step=4, dtype=F32, quirks=Q_PAPER), tables=_stage4, eps=_threshold_eps, n=64, max_steps=60, episodes=1),
}
_EPS = {}


def case_args(case_id):
    """(cfg, (qa, qb), eps, n, max_steps, episodes) of a case"""
    c = CASES[case_id]
    if case_id not in _EPS:
        _EPS[case_id] = c["eps"]() if callable(c["eps"]) else c["eps"]
    return c["cfg"](), c["tables"](), _EPS[case_id], c["n"], c["max_steps"], c["episodes"]


def stepwise_model(cfg, tables, n, seed, eps, max_steps, episodes):
    """{"pairs" uint32 [N_CELLS][N_STATES], "reward_fx" int64 [N_CELLS], "terminal" int64 [N_CELLS][N_CODES], "by_code" int64 [N_COLS], "steps_sum" int,
    "visits" int64 [N_CELLS], "events"} of one table set flown by `n` envs for periods 0 .. max_steps, `episodes` episodes per env at most"""
    qa, qb = (np.ascontiguousarray(t, np.float64).ravel() for t in tables)
    o = Oracle(cfg, n, seed=seed)
    rn, inn = o.field_names(False), o.field_names(True)
    i_rew = rn.index("reward")
    i_idx, i_fl, i_code, i_sc = (inn.index(f) for f in ("idx_x", "flags", "code", "step_count"))
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    thr = ec.eps_thr(eps)
    pairs = np.zeros((N_CELLS, N_STATES), np.uint32); reward_fx = np.zeros(N_CELLS, np.int64); terminal = np.zeros((N_CELLS, N_CODES), np.int64)
    by_code = np.zeros(N_COLS, np.int64)
    steps_sum = 0
    finished = np.zeros(n, np.int64); stopped_at = np.full(n, -1, np.int64)
    ev = {"decisions": 0, "explored": 0, "greedy": 0, "reset_periods": 0, "same_pair_wave_periods": 0, "cross_level": 0, "beyond_level0": 0, "rewarded_success_periods": 0,
          "nonzero_terminal_rewards": 0, "periods": 0, "ends_outside_a_decision": 0, "draws_at_the_threshold_that_matter": 0}
    ctr = np.zeros((n, 4), np.uint32); ctr[:, 2] = np.arange(n); ctr[:, 3] = STREAM_ACTION
    for j in range(max_steps + 1):
        _, ints = o.get_fields()
        s = ints[i_idx].astype(np.int64); was_done = (ints[i_fl] & FL_DONE) != 0
        ctr[:, 0] = j & 0xffffffff; ctr[:, 1] = (j >> 32) & 0xffffffff
        w = orc.philox_n(ctr, (k0, k1))
        explore = (w[:, 0] >> 8) < thr
        greedy = orc.agent_predict(qa, qb, np.where(was_done, 0, s)).astype(np.int64)
        explored_action = ((w[:, 1].astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int64)
        act = np.where(explore, explored_action, greedy)
        at_threshold = ((w[:, 0] >> 8) == thr) & (explored_action != greedy)
        act[was_done] = 2  # a reset period takes no action
        o.step(act.astype(np.uint8))
        reals, ints = o.get_fields()
        flags = ints[i_fl]
        was_reset, done = (flags & FL_WAS_RESET) != 0, (flags & FL_DONE) != 0
        assert np.array_equal(was_reset, was_done), "a reset period is the period after a done one"
        live = finished < episodes                       # before this period
        counts = live & ~was_reset
        ev["periods"] = j + 1; ev["reset_periods"] += int((live & was_reset).sum())
        cell, ns, code = s * 3 + act, ints[i_idx].astype(np.int64), ints[i_code].astype(np.int64)
        fx = np.rint(reals[i_rew] * float(1 << TARGET_FRAC_BITS)).astype(np.int64)
        assert (act[counts] < 3).all() and (s[counts] >= 0).all() and (s[counts] < N_STATES).all() and (ns[counts] >= 0).all() and (ns[counts] < N_STATES).all()
        end, go = counts & done, counts & ~done
        assert (code[end] >= 0).all() and (code[end] < N_CODES).all()
        np.add.at(pairs, (cell[go], ns[go]), 1)
        np.add.at(terminal, (cell[end], code[end]), 1)
        np.add.at(reward_fx, cell[counts], fx[counts])
        np.add.at(by_code, code[end], 1)
        steps_sum += int((ints[i_sc][end] & 0xffff).sum())
        ev["decisions"] += int(counts.sum()); ev["explored"] += int((counts & explore).sum()); ev["greedy"] += int((counts & ~explore).sum())
        ev["draws_at_the_threshold_that_matter"] += int((counts & at_threshold).sum())
        ev["cross_level"] += int((s[go] // STATES_PER_LEVEL != ns[go] // STATES_PER_LEVEL).sum())
        ev["beyond_level0"] += int((cell[counts] >= CELLS_PER_LEVEL).sum()) + int((ns[go] >= STATES_PER_LEVEL).sum())
        ev["rewarded_success_periods"] += int((counts & ((code == rc.SUCCESS) | (code == NON_TERMINAL_SUCCESS)) & (fx != 0)).sum())
        ev["nonzero_terminal_rewards"] += int((fx[end] != 0).sum())
        ev["ends_outside_a_decision"] += int((done & live & ~counts).sum())
        for v in range(0, n, 64):                        # a wave: 64 consecutive envs of the set
            m = go[v:v + 64]
            key = cell[v:v + 64][m] * N_STATES + ns[v:v + 64][m]
            if key.size != np.unique(key).size:
                ev["same_pair_wave_periods"] += 1
        finished[end] += 1
        stopped_at[end & (finished >= episodes)] = j
        if (finished >= episodes).all():
            break
    by_code[N_CODES] = n * episodes - int(finished.sum())
    ev["cut_off_envs"] = int((finished < episodes).sum())
    ev["distinct_pairs"] = int((pairs != 0).sum()); ev["largest_pair"] = int(pairs.max())
    ev["distinct_stop_periods"] = len(set(stopped_at[stopped_at >= 0].tolist())); ev["last_stop_period"] = int(stopped_at.max())
    ev["early_lanes"] = int(((stopped_at >= 0) & (stopped_at < ev["periods"] - 1)).sum())
    ev["terminals"] = {CHECK_NAMES[k]: int(terminal[:, k].sum()) for k in range(N_CODES) if terminal[:, k].any()}
    return {"pairs": pairs, "reward_fx": reward_fx, "terminal": terminal, "by_code": by_code, "steps_sum": steps_sum,
            "visits": pairs.sum(axis=1, dtype=np.int64) + terminal.sum(axis=1), "events": ev}


_YARDSTICKS = {}


def yardstick(case_id):
    """the case's stepwise model, computed once and left unchanged; asserts ON IT that the events the case is there for occurred (occurrence, not counts)"""
    if case_id not in _YARDSTICKS:
        cfg, tables, eps, n, max_steps, episodes = case_args(case_id)
        w = stepwise_model(cfg, tables, n, SEED, eps, max_steps, episodes)
        ev, t = w["events"], w["events"]["terminals"]
        print("model case", case_id, ev, "by_code", w["by_code"].tolist(), "steps_sum", w["steps_sum"])
        assert ev["decisions"] > 0 and ev["ends_outside_a_decision"] == 0 and int(w["visits"].sum()) == ev["decisions"]
        assert int(w["terminal"].sum()) == int(w["by_code"][:N_CODES].sum()) > 0
        if case_id == "A":
            assert ev["explored"] > 0 and ev["greedy"] > 0 and ev["same_pair_wave_periods"] > 0 and ev["cross_level"] > 0 and ev["largest_pair"] > 1
            assert t.get("TERMINAL_CONTACT", 0) > 0 and t.get("TERMINAL_FLYZONE_X", 0) > 0 and t.get("TERMINAL_MINIMUM_ALTITUDE", 0) > 0, t
            assert ev["cut_off_envs"] > 0 and w["by_code"][N_CODES] > 0 and ev["reset_periods"] > n
        elif case_id in ("B", "B64"):
            assert t.get("TERMINAL_SUCCESS", 0) > 0 and t.get("TERMINAL_FLYZONE_X", 0) > 0, t
            assert ev["rewarded_success_periods"] > 0 and ev["nonzero_terminal_rewards"] > 0, ev
        elif case_id == "C":
            assert ev["explored"] == ev["decisions"] and ev["greedy"] == 0 and ev["beyond_level0"] == 0 and n == 192, ev
            assert int(w["terminal"].sum()) > 0 and ev["reset_periods"] > n
        elif case_id == "D":
            assert ev["explored"] == 0 and ev["cut_off_envs"] == 0 and ev["reset_periods"] == n, ev
            assert ev["distinct_stop_periods"] >= 8 and ev["early_lanes"] >= n // 2 and ev["last_stop_period"] < max_steps, ev
        elif case_id == "E":
            assert ev["draws_at_the_threshold_that_matter"] > 0 and ev["explored"] > 0 and ev["greedy"] > 0, ev
        _YARDSTICKS[case_id] = w
    return _YARDSTICKS[case_id]


def assert_model_set_equal(got, k, want, what):
    """table set `k` of a model result against the yardstick of that set: every output =="""
    for f in FIELDS:
        g, w = np.asarray(got[f][k]), np.asarray(want[f])
        assert g.shape == w.shape, f"{what}: {f} has shape {g.shape}, want {w.shape}"
        if f == "pairs":
            assert g.dtype == np.uint32, f"{what}: pairs is {g.dtype}"
        bad = np.argwhere(g.astype(np.int64) != w.astype(np.int64))
        assert not len(bad), (f"{what}: {f} differs in {len(bad)} of {w.size} entries (first at {tuple(int(v) for v in bad[0])}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}; "
                              f"sums {int(g.astype(np.int64).sum())} vs {int(w.astype(np.int64).sum())})")
