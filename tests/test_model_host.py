"""The host side of the transition model that needs no GPU: the argument checks `ops.transition_model` makes before it touches the library, the buffers and
bindings, `solve_model` against closed forms on hand-built models, and `model_divergence` on identical, disjoint and under-visited inputs."""
import re
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import CHECK_NAMES, F32, N_CELLS, Q_PAPER, TARGET_FRAC_BITS, simulation_config

import model_checks as mc
import rollout_checks as rc

ROOT = Path(__file__).resolve().parent.parent
N_STATES, N_CODES = N_CELLS // 3, len(CHECK_NAMES)
ONE = 1 << TARGET_FRAC_BITS
SUCCESS = CHECK_NAMES.index("TERMINAL_SUCCESS")


class Model:
    """a hand-built model: go(s, a, s2, reward, times) and end(s, a, code, reward, times) add transitions"""

    def __init__(self):
        self.pairs = np.zeros((N_CELLS, N_STATES), np.uint32); self.reward_fx = np.zeros(N_CELLS, np.int64); self.terminal = np.zeros((N_CELLS, N_CODES), np.int64)

    def go(self, s, a, s2, reward, times=1):
        self.pairs[s * 3 + a, s2] += times; self.reward_fx[s * 3 + a] += int(round(reward * ONE)) * times
        return self

    def end(self, s, a, code, reward, times=1):
        self.terminal[s * 3 + a, code] += times; self.reward_fx[s * 3 + a] += int(round(reward * ONE)) * times
        return self

    def solve(self, gamma, **kw):
        return evaluation.solve_model(self.pairs, self.reward_fx, self.terminal, gamma, **kw)


def test_solve_model_on_a_two_state_chain():
    """0 -> 1 with reward 1, 1 -> 0 with reward 2, gamma 1/2: Q0 = 1 + Q1 / 2, Q1 = 2 + Q0 / 2, so Q0 = 8/3 and Q1 = 10/3"""
    q, solved = Model().go(0, 0, 1, 1.0, 10).go(1, 0, 0, 2.0, 7).solve(0.5)
    assert q.shape == (N_CELLS,) and solved.dtype == bool and np.flatnonzero(solved).tolist() == [0, 3]
    assert q[0] == pytest.approx(8 / 3, abs=1e-8) and q[3] == pytest.approx(10 / 3, abs=1e-8)
    assert (q[~solved] == q[solved].min() - 1.0).all(), "unsolved cells lie below every solved one"
    q0, _ = Model().go(0, 0, 1, 1.0, 10).go(1, 0, 0, 2.0, 7).solve(0.0)
    assert q0[0] == 1.0 and q0[3] == 2.0  # gamma 0: the mean rewards


def test_solve_model_does_not_bootstrap_from_a_terminal_transition():
    """state 2, action 1: three of four visits end the episode, one returns to state 2; mean reward 5, gamma 1/2: Q = 5 + Q / 8, so Q = 40/7"""
    q, solved = Model().end(2, 1, SUCCESS, 6.0, 3).go(2, 1, 2, 2.0, 1).solve(0.5)
    assert np.flatnonzero(solved).tolist() == [7] and q[7] == pytest.approx(40 / 7, abs=1e-8)
    qt, _ = Model().end(2, 1, SUCCESS, 6.0, 3).solve(0.5)
    assert qt[7] == 6.0  # always terminal: the mean reward, whatever gamma


def test_solve_model_takes_the_maximum_over_solved_actions_only():
    """rewards are negative, so the floor min - 1 lies below everything: a state's value must not fall to it through an unvisited action, and a state none of
    whose actions was visited is worth 0, not the floor"""
    m = Model().go(6, 0, 6, -1.0, 4)       # Q(6, 0) = -1 / (1 - 1/2) = -2: the smallest solved value, the floor is -3
    m.go(5, 2, 6, 0.0, 2)                  # Q(5, 2) = gamma * V(6) = -1: V(6) is Q(6, 0), the actions 1 and 2 of state 6 are unsolved
    m.go(7, 0, 8, -1.0, 1)                 # state 8 was never visited: V(8) = 0, Q(7, 0) = -1
    m.go(9, 0, 5, 0.0, 1).go(9, 1, 7, -0.25, 1)  # Q(9, 0) = -1/2, Q(9, 1) = -3/4; state 9's greedy action is 0
    q, solved = m.solve(0.5)
    assert q[6 * 3] == pytest.approx(-2.0, abs=1e-8) and q[5 * 3 + 2] == pytest.approx(-1.0, abs=1e-8) and q[7 * 3] == pytest.approx(-1.0, abs=1e-8)
    assert q[9 * 3] == pytest.approx(-0.5, abs=1e-8) and q[9 * 3 + 1] == pytest.approx(-0.75, abs=1e-8)
    assert solved.sum() == 5 and (q[~solved] == pytest.approx(-3.0, abs=1e-8)) and q[6 * 3 + 1] < q[6 * 3]
    assert evaluation.greedy_actions(q, q)[0][[5, 6, 9]].tolist() == [2, 0, 0], "a greedy flight on the solution never prefers an unsolved cell"


def test_solve_model_min_visits_cuts_thin_cells_out():
    """state 1's only action was seen twice: with min_visits 3 it is unsolved, state 1 is worth 0, and Q(0, 0) falls to its mean reward"""
    m = Model().go(0, 0, 1, 1.0, 10).go(1, 0, 1, 3.0, 2)
    q, solved = m.solve(0.5)
    assert solved[3] and q[3] == pytest.approx(6.0, abs=1e-8) and q[0] == pytest.approx(4.0, abs=1e-8)
    q, solved = m.solve(0.5, min_visits=3)
    assert not solved[3] and solved[0] and q[0] == 1.0 and q[3] == 0.0
    q, solved = m.solve(0.5, min_visits=11)
    assert not solved.any() and (q == -1.0).all()
    q1, _ = m.solve(0.5, max_iter=1)
    assert q1[0] == 1.0 and q1[3] == 3.0, "one sweep from zero gives the mean rewards"
    for bad in (dict(min_visits=0), dict(gamma=1.5)):
        kw = dict(gamma=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            evaluation.solve_model(m.pairs, m.reward_fx, m.terminal, **kw)
    with pytest.raises(ValueError):
        evaluation.solve_model(m.pairs[None], m.reward_fx, m.terminal, 0.5)


def test_solve_model_on_the_oracle_s_model_of_a_case():
    """on case D's yardstick: every visited cell is solved, the fixed point holds, and the mean rewards come back with gamma 0"""
    w = mc.yardstick("D")
    q, solved = evaluation.solve_model(w["pairs"], w["reward_fx"], w["terminal"], 0.9)
    assert np.array_equal(solved, w["visits"] > 0) and solved.sum() > 100 and np.isfinite(q).all()
    v = np.where(solved.reshape(N_STATES, 3), q.reshape(N_STATES, 3), -np.inf).max(axis=1)
    v[~solved.reshape(N_STATES, 3).any(axis=1)] = 0.0
    vis = w["visits"][solved].astype(np.float64)
    rhs = w["reward_fx"][solved] / ONE / vis + 0.9 * (w["pairs"][solved].astype(np.float64) @ v) / vis
    assert np.abs(q[solved] - rhs).max() < 1e-7
    q0, _ = evaluation.solve_model(w["pairs"], w["reward_fx"], w["terminal"], 0.0)
    assert np.array_equal(q0[solved], w["reward_fx"][solved] / ONE / vis)


def test_model_divergence_on_identical_disjoint_and_under_visited_models():
    a = Model().go(0, 0, 1, 0.0, 3).go(0, 0, 2, 0.0, 1).end(4, 1, SUCCESS, 0.0, 2).go(4, 1, 5, 0.0, 2).go(6, 2, 6, 0.0, 5).go(8, 0, 1, 0.0, 2)
    b = Model().go(0, 0, 1, 0.0, 6).go(0, 0, 2, 0.0, 2).end(4, 1, SUCCESS, 0.0, 4).go(6, 2, 7, 0.0, 1).go(8, 0, 1, 0.0, 9)
    same = evaluation.model_divergence(a.pairs, a.terminal, a.pairs, a.terminal)
    visited = a.pairs.sum(axis=1) + a.terminal.sum(axis=1) > 0
    assert same.shape == (N_CELLS,) and (same[visited] == 0.0).all() and np.isnan(same[~visited]).all() and visited.sum() == 4
    d = evaluation.model_divergence(a.pairs, a.terminal, b.pairs, b.terminal)
    assert d[0] == 0.0, "the same distribution from twice the visits"
    assert d[4 * 3 + 1] == pytest.approx(0.5), "the terminal codes are part of the alphabet: (1/2 success, 1/2 state 5) against (all success)"
    assert d[6 * 3 + 2] == 1.0, "disjoint outcomes"
    assert d[8 * 3] == 0.0 and np.isnan(d[1])
    d3 = evaluation.model_divergence(a.pairs, a.terminal, b.pairs, b.terminal, min_visits=3)
    assert np.isnan(d3[8 * 3]) and np.isnan(d3[6 * 3 + 2]) and d3[0] == 0.0 and d3[4 * 3 + 1] == pytest.approx(0.5), "NaN where EITHER side is under-visited"
    assert np.array_equal(np.isnan(evaluation.model_divergence(b.pairs, b.terminal, a.pairs, a.terminal, 3)), np.isnan(d3)), "symmetric"
    with pytest.raises(ValueError):
        evaluation.model_divergence(a.pairs, a.terminal, b.pairs, b.terminal, min_visits=0)
    with pytest.raises(ValueError):
        evaluation.model_divergence(a.pairs, a.terminal, b.pairs, b.terminal[:, :-1])


def test_buffers_have_the_shapes_and_types_of_the_abi():
    pairs, reward_fx, terminal, by_code, steps_sum = ops.model_buffers(3)
    assert (pairs.shape, pairs.dtype) == ((3, N_CELLS, N_STATES), np.uint32) and (reward_fx.shape, reward_fx.dtype) == ((3, N_CELLS), np.int64)
    assert (terminal.shape, terminal.dtype) == ((3, N_CELLS, N_CODES), np.int64) and by_code.shape == (3, N_CODES + 1) and steps_sum.shape == (3,)
    assert ops.MODEL_MAX_TABLES == 16 and ops.N_STATES == mc.N_STATES == 945
    hdr = (ROOT / "include" / "dql.h").read_text()
    assert re.search(r"#define DQL_MODEL_MAX_TABLES 16\b", hdr) and re.search(r"#define DQL_ABI_VERSION 6\b", hdr)


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded for a call that must be refused on the host")

    monkeypatch.setattr(_lib, "load", no_library)
    cfg = rc.case_config("simulation-f32")
    qa, qb = rc.stage4_tables()
    good = dict(envs_per_table=64, seed=1, eps=0.1, episodes=1, max_steps=600)
    bad = {
        "envs 0": dict(envs_per_table=0), "envs 100": dict(envs_per_table=100), "envs -64": dict(envs_per_table=-64),
        "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65), "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097),
        "2^32 pair counts": dict(envs_per_table=1 << 20, max_steps=4095), "eps -0.1": dict(eps=-0.1), "eps 1.01": dict(eps=1.01), "eps nan": dict(eps=float("nan")),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            ops.transition_model(cfg, qa, qb, **dict(good, **kw))
            pytest.fail(what)
    with pytest.raises(ValueError, match="x MDP"):
        ops.transition_model(simulation_config(working_curriculum_step=4, two_axis=1, quirks=Q_PAPER, dtype=F32), qa, qb, **good)
    for tables in ((qa[:-1], qb[:-1]), (np.stack([qa, qa]), qb), (np.zeros((0, 2835)), np.zeros((0, 2835))), (np.tile(qa, (17, 1)), np.tile(qb, (17, 1)))):
        with pytest.raises(ValueError):
            ops.transition_model(cfg, *tables, **good)
    ops.model_check_args(cfg, 16, (1 << 20) - 64, 64, 4095, 1.0)  # just below 2^32 pair counts, the most sets, both ends of eps
    ops.model_check_args(cfg, 1, 64, 1, 1, 0.0)
    with pytest.raises(AssertionError):                            # and a well-formed call does reach the library
        ops.transition_model(cfg, qa, qb, **good)


def test_the_new_symbols_are_declared_and_bound():
    hdr = (ROOT / "include" / "dql.h").read_text()
    diag = (ROOT / "include" / "dql_diag.h").read_text()
    n_args = lambda text, name: re.search(r"\bint %s\(([^;]*)\);" % name, text).group(1).count(",") + 1
    assert n_args(hdr, "dql_model") == len(_lib.SYMBOLS["dql_model"][1]) == 15
    assert n_args(hdr, "dql_ensemble_model") == len(_lib.SYMBOLS["dql_ensemble_model"][1]) == 14
    assert n_args(diag, "dql_diag_model_last") == len(_lib.SYMBOLS["dql_diag_model_last"][1]) == 2
    import __graft_entry__ as g
    g.build_hip()
    lib = _lib.load()
    for name in ("dql_model", "dql_ensemble_model", "dql_diag_model_last"):
        assert getattr(lib, name) is not None
    # the script's flags
    sim = (ROOT / "scripts" / "simulation.py").read_text()
    assert '"--model-out"' in sim and '"--model-eps"' in sim and "ops.transition_model" in sim
