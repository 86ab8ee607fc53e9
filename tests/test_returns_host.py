"""The host side of the realised returns that needs no GPU: the argument checks `ops.returns_map` makes before it touches the library (the overflow guard
among them), the buffers and bindings, and `evaluation.value_calibration` against closed forms on hand-made inputs."""
import re
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import CHECK_NAMES, DqlConfig, F32, N_CELLS, Q_PAPER, TARGET_FRAC_BITS, simulation_config

import rollout_checks as rc

ROOT = Path(__file__).resolve().parent.parent
ONE = 1 << TARGET_FRAC_BITS


def tables(**cells):
    """(qa, qb, visits, return_fx) of zeros, with cells {c: (qa, qb, visits, mean return)} set; the mean returns are multiples of 2^-26"""
    qa, qb = np.zeros(N_CELLS), np.zeros(N_CELLS)
    visits, return_fx = np.zeros(N_CELLS, np.int64), np.zeros(N_CELLS, np.int64)
    for c, (a, b, v, m) in cells.items():
        c = int(c[1:])
        qa[c], qb[c], visits[c], return_fx[c] = a, b, v, int(round(m * ONE)) * v
    return qa, qb, visits, return_fx


def test_value_calibration_on_a_hand_made_two_cell_example():
    """cell 0: Q_a = 5, Q_b = 3, 100 visits with mean return 2 (both overestimate: + 3, + 1); cell 4: Q_a = -1, Q_b = 1, 300 visits with mean return 1 (bias - 2, 0)"""
    r = evaluation.value_calibration(*tables(c0=(5.0, 3.0, 100, 2.0), c4=(-1.0, 1.0, 300, 1.0)))
    assert r["mean_return"].shape == (N_CELLS,) and r["mean_return"][0] == 2.0 and r["mean_return"][4] == 1.0 and np.isnan(r["mean_return"][1])
    assert (r["bias_a"][[0, 4]].tolist(), r["bias_b"][[0, 4]].tolist(), r["bias_mean"][[0, 4]].tolist()) == ([3.0, -2.0], [1.0, 0.0], [2.0, -1.0])
    assert np.isnan(r["bias_a"][1]) and np.isnan(r["bias_mean"][2834])
    s = r["summary"]
    assert s["cells"] == 2 and s["visits"] == 400
    assert s["a"]["mean_bias"] == pytest.approx((100 * 3 - 300 * 2) / 400) and s["a"]["rms_bias"] == pytest.approx(np.sqrt((100 * 9 + 300 * 4) / 400))
    assert s["b"]["mean_bias"] == pytest.approx(0.25) and s["b"]["rms_bias"] == pytest.approx(0.5)
    assert s["mean"]["mean_bias"] == pytest.approx((100 * 2 - 300) / 400)
    assert s["a"]["overestimated_share"] == 0.25 and s["b"]["overestimated_share"] == 0.25, "a bias of exactly 0 does not overestimate"
    assert "agreement_share" not in s


def test_value_calibration_min_visits_cut():
    args = tables(c0=(5.0, 5.0, 29, 2.0), c4=(0.0, 0.0, 30, 1.0), c7=(9.0, 9.0, 1, 0.0))
    r = evaluation.value_calibration(*args)  # the default floor is 30
    assert np.isnan(r["mean_return"][0]) and np.isnan(r["mean_return"][7]) and r["mean_return"][4] == 1.0
    assert r["summary"]["cells"] == 1 and r["summary"]["visits"] == 30 and r["summary"]["a"]["mean_bias"] == -1.0
    r1 = evaluation.value_calibration(*args, min_visits=1)
    assert r1["summary"]["cells"] == 3 and r1["summary"]["visits"] == 60 and r1["mean_return"][7] == 0.0
    assert r1["summary"]["a"]["mean_bias"] == pytest.approx((29 * 3 - 30 + 9) / 60)
    none = evaluation.value_calibration(*args, min_visits=31)
    assert none["summary"]["cells"] == 0 and np.isnan(none["summary"]["a"]["mean_bias"]) and np.isnan(none["summary"]["a"]["overestimated_share"])
    with pytest.raises(ValueError):
        evaluation.value_calibration(*args, min_visits=0)
    with pytest.raises(ValueError):
        evaluation.value_calibration(args[0][:-1], *args[1:])


def test_value_calibration_splits_the_levels_at_cell_567():
    """cell 566 is the last of level 0, cell 567 the first of level 1, cell 2834 the last of level 4"""
    r = evaluation.value_calibration(*tables(c566=(1.0, 1.0, 50, 0.0), c567=(-3.0, -3.0, 50, 0.0), c2834=(2.0, 2.0, 100, 0.0)))
    a = r["summary"]["a"]
    assert a["mean_bias_by_level"].shape == (5,) and a["mean_bias_by_level"][[0, 1, 4]].tolist() == [1.0, -3.0, 2.0] and np.isnan(a["mean_bias_by_level"][[2, 3]]).all()
    assert a["rms_bias_by_level"][[0, 1, 4]].tolist() == [1.0, 3.0, 2.0] and np.isnan(a["rms_bias_by_level"][[2, 3]]).all()
    assert a["mean_bias"] == pytest.approx((50 - 150 + 200) / 200) and a["overestimated_share"] == 0.75


def test_value_calibration_agreement_leaves_out_a_state_with_one_visited_action():
    """state 0: greedy action 0 has the best mean return of two visited actions (agrees); state 1: greedy action 2, but action 0's return is better (disagrees);
    state 2: only its greedy action was visited often enough (left out); state 3: two actions visited but NOT the greedy one (left out)"""
    args = tables(c0=(0, 0, 40, 5.0), c1=(0, 0, 40, 4.0), c3=(0, 0, 40, 2.0), c5=(0, 0, 40, 1.0), c6=(0, 0, 40, 3.0), c7=(0, 0, 10, 9.0), c10=(0, 0, 40, 1.0), c11=(0, 0, 40, 2.0))
    greedy = np.zeros(N_CELLS // 3, np.int64)
    greedy[1] = 2
    s = evaluation.value_calibration(*args, greedy=greedy)["summary"]
    assert s["agreement_states"] == 2 and s["agreement_share"] == 0.5
    s1 = evaluation.value_calibration(*args, greedy=greedy, min_visits=10)["summary"]   # state 2's second action now counts, and beats the greedy one
    assert s1["agreement_states"] == 3 and s1["agreement_share"] == pytest.approx(1 / 3)
    empty = evaluation.value_calibration(*tables(c0=(0, 0, 40, 5.0)), greedy=greedy)["summary"]
    assert empty["agreement_states"] == 0 and np.isnan(empty["agreement_share"])
    with pytest.raises(ValueError):
        evaluation.value_calibration(*args, greedy=greedy[:-1])


def test_buffers_have_the_shapes_and_types_of_the_abi():
    visits, return_fx, cut, by_code, steps_sum = ops.returns_buffers(3)
    assert (visits.shape, visits.dtype) == ((3, N_CELLS), np.int64) and (return_fx.shape, return_fx.dtype) == ((3, N_CELLS), np.int64)
    assert (cut.shape, cut.dtype) == ((3,), np.int64) and by_code.shape == (3, len(CHECK_NAMES) + 1) and steps_sum.shape == (3,)
    hdr = (ROOT / "include" / "dql.h").read_text()
    assert re.search(r"#define DQL_SCORE_MAP_MAX_TABLES \(1 << 14\)", hdr) and ops.SCORE_MAP_MAX_TABLES == 1 << 14 and re.search(r"#define DQL_ABI_VERSION 6\b", hdr)


def test_the_overflow_guard_is_the_issue_s_arithmetic():
    """R = 26.0 by default; at gamma 0.99 and max_steps 600 B = 2 603 reward units and 52.8 M decisions per set fit: 65 536 envs pass, 131 072 do not"""
    cfg = DqlConfig(dtype=F32)
    assert 26.0 <= cfg.max_abs_reward() < 26.01 and cfg.max_abs_td_target() == cfg.max_abs_reward() / (1.0 - cfg.gamma) * (1.0 + 2.0 ** -10)
    bound = ops.returns_bound_fx(cfg, 0.99, 600)
    assert round(bound / ONE) == 2603 and ((1 << 63) - 1) // (bound + 1) // 100_000 == 528
    ops.returns_check_args(cfg, 1, 65536, 1, 600, 0.1, 0.99)
    with pytest.raises(ValueError, match="overflow"):
        ops.returns_check_args(cfg, 1, 131072, 1, 600, 0.1, 0.99)
    # gamma 1: the horizon is max_steps + 1 periods
    assert ops.returns_bound_fx(cfg, 1.0, 600) == ops.returns_bound_fx(cfg, 0.9999, 600) > 6 * bound
    ops.returns_check_args(cfg, 1, 8192, 1, 600, 0.1, 1.0)
    with pytest.raises(ValueError, match="overflow"):
        ops.returns_check_args(cfg, 1, 16384, 1, 600, 0.1, 1.0)


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded for a call that must be refused on the host")

    monkeypatch.setattr(_lib, "load", no_library)
    cfg = rc.case_config("simulation-f32")
    qa, qb = rc.stage4_tables()
    good = dict(envs_per_table=64, seed=1, eps=0.1, gamma=0.99, episodes=1, max_steps=600)
    bad = {
        "envs 0": dict(envs_per_table=0), "envs 100": dict(envs_per_table=100), "envs -64": dict(envs_per_table=-64),
        "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65), "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097),
        "a log beyond 2^29 words": dict(envs_per_table=1 << 20, max_steps=512), "the int64 guard": dict(envs_per_table=131072),
        "eps -0.1": dict(eps=-0.1), "eps 1.01": dict(eps=1.01), "eps nan": dict(eps=float("nan")),
        "gamma -0.1": dict(gamma=-0.1), "gamma 1.01": dict(gamma=1.01), "gamma nan": dict(gamma=float("nan")),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            ops.returns_map(cfg, qa, qb, **dict(good, **kw))
            pytest.fail(what)
    with pytest.raises(ValueError, match="x MDP"):
        ops.returns_map(simulation_config(working_curriculum_step=4, two_axis=1, quirks=Q_PAPER, dtype=F32), qa, qb, **good)
    many = (1 << 14) + 1
    for t in ((qa[:-1], qb[:-1]), (np.stack([qa, qa]), qb), (np.zeros((0, 2835)), np.zeros((0, 2835))), (np.zeros((many, 2835)), np.zeros((many, 2835)))):
        with pytest.raises(ValueError):
            ops.returns_map(cfg, *t, **dict(good, max_steps=1))
    ops.returns_check_args(cfg, 1 << 14, 64, 64, 511, 1.0, 1.0)   # exactly 2^29 log words, the most sets, both upper ends
    ops.returns_check_args(cfg, 1, 64, 1, 1, 0.0, 0.0)
    with pytest.raises(ValueError, match="2\\^29"):
        ops.returns_check_args(cfg, 1 << 14, 64, 64, 512, 1.0, 1.0)
    with pytest.raises(AssertionError):                            # and a well-formed call does reach the library
        ops.returns_map(cfg, qa, qb, **good)


def test_the_new_symbols_are_declared_and_bound():
    hdr = (ROOT / "include" / "dql.h").read_text()
    diag = (ROOT / "include" / "dql_diag.h").read_text()
    n_args = lambda text, name: re.search(r"\bint %s\(([^;]*)\);" % name, text).group(1).count(",") + 1
    assert n_args(hdr, "dql_returns") == len(_lib.SYMBOLS["dql_returns"][1]) == 16
    assert n_args(hdr, "dql_ensemble_returns") == len(_lib.SYMBOLS["dql_ensemble_returns"][1]) == 15
    assert n_args(diag, "dql_diag_returns_last") == len(_lib.SYMBOLS["dql_diag_returns_last"][1]) == 3
    import __graft_entry__ as g
    g.build_hip()
    lib = _lib.load()
    for name in ("dql_returns", "dql_ensemble_returns", "dql_diag_returns_last"):
        assert getattr(lib, name) is not None
    hip = (ROOT / "dql_multirotor_landing_amd" / "csrc" / "dql_hip.hip").read_text()
    assert '#include "dql_returns.hpp"' in hip and '#include "dql_returns.inc"' in hip
    # the script's flags
    sim = (ROOT / "scripts" / "simulation.py").read_text()
    assert '"--returns-out"' in sim and '"--returns-eps"' in sim and '"--returns-gamma"' in sim and "ops.returns_map" in sim
