"""The host side of the split transition model that needs no GPU: the argument checks `ops.split_model` makes before it touches the library, the feature names
against the header, the buffers and bindings, and the pure-numpy readers `feature_means`, `split_divergence` and `aliasing_table` against closed forms."""
import re
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import CHECK_NAMES, F32, N_CELLS, Q_PAPER, simulation_config

import rollout_checks as rc

ROOT = Path(__file__).resolve().parent.parent
N_STATES, N_CODES = N_CELLS // 3, len(CHECK_NAMES)
SUCCESS = CHECK_NAMES.index("TERMINAL_SUCCESS")
HDR = (ROOT / "include" / "dql.h").read_text()


class Split:
    """a hand-built split-model result of one table set: go(half, s, a, s2, times), end(half, s, a, code, times), value(s, total) add to it"""

    def __init__(self):
        self.r = {"pairs": np.zeros((1, 2, N_CELLS, N_STATES), np.uint32), "terminal": np.zeros((1, 2, N_CELLS, N_CODES), np.int64),
                  "reward_fx": np.zeros((1, 2, N_CELLS), np.int64), "feat_sum_fx": np.zeros((1, N_STATES), np.int64)}

    def go(self, half, s, a, s2, times=1):
        self.r["pairs"][0, half, s * 3 + a, s2] += times
        return self

    def end(self, half, s, a, code, times=1):
        self.r["terminal"][0, half, s * 3 + a, code] += times
        return self

    def value(self, s, total):
        self.r["feat_sum_fx"][0, s] += int(round(total * (1 << 20)))
        return self


def test_feature_names_and_limits_are_the_header_s():
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bDQL_SPLIT_([A-Z_]+) = (\d+)", HDR)}
    assert codes == {name: code for code, name in enumerate(ops.SPLIT_FEATURES)} and len(codes) == 11
    assert re.search(r"#define DQL_SPLIT_N_FEATURES 11\b", HDR) and re.search(r"#define DQL_SPLIT_FRAC_BITS 20\b", HDR)
    assert re.search(r"#define DQL_MODEL_SPLIT_MAX_TABLES 8\b", HDR) and re.search(r"#define DQL_ABI_VERSION 6\b", HDR)
    assert ops.MODEL_SPLIT_MAX_TABLES == 8 and ops.SPLIT_FRAC_BITS == evaluation.SPLIT_FRAC_BITS == 20
    for code, name in enumerate(ops.SPLIT_FEATURES):
        assert ops.split_feature_code(name) == ops.split_feature_code(name.upper()) == ops.split_feature_code("DQL_SPLIT_" + name.upper()) == code
        assert ops.split_feature_code(code) == ops.split_feature_code(np.int32(code)) == code
    for bad in ("pitch", "", -1, 11, 1.0, None, True):
        with pytest.raises(ValueError):
            ops.split_feature_code(bad)


def test_buffers_and_bindings_have_the_shapes_and_types_of_the_abi():
    pairs, reward_fx, terminal, feat, by_code, steps_sum = ops.split_model_buffers(3)
    assert (pairs.shape, pairs.dtype) == ((3, 2, N_CELLS, N_STATES), np.uint32) and (reward_fx.shape, reward_fx.dtype) == ((3, 2, N_CELLS), np.int64)
    assert (terminal.shape, terminal.dtype) == ((3, 2, N_CELLS, N_CODES), np.int64) and (feat.shape, feat.dtype) == ((3, N_STATES), np.int64)
    assert by_code.shape == (3, N_CODES + 1) and steps_sum.shape == (3,)
    for name, n_args in (("dql_model_split", 18), ("dql_ensemble_model_split", 17), ("dql_diag_model_split_last", 2)):
        assert len(_lib.SYMBOLS[name][1]) == n_args, name
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR + (ROOT / "include" / "dql_diag.h").read_text(), re.S)
        assert decl and len(decl.group(1).split(",")) == n_args, name
    c = ops.split_cut_array(0.5)
    assert c.shape == (N_STATES,) and c.dtype == np.float64 and (c == 0.5).all()
    both = np.full(N_STATES, np.inf); both[::2] = -np.inf
    assert np.array_equal(ops.split_cut_array(both), both), "+-inf are valid cuts"


def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded for a call that must be refused on the host")

    monkeypatch.setattr(_lib, "load", no_library)
    cfg = rc.case_config("simulation-f32")
    qa, qb = rc.stage4_tables()
    good = dict(envs_per_table=64, seed=1, eps=0.1, feature="pitch_sp", cut=0.0, episodes=1, max_steps=600)
    nan_cut = np.zeros(N_STATES); nan_cut[17] = np.nan
    bad = {
        "envs 0": dict(envs_per_table=0), "envs 100": dict(envs_per_table=100), "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65),
        "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097), "2^30 feature terms": dict(envs_per_table=1 << 18, max_steps=4095),
        "eps -0.1": dict(eps=-0.1), "eps nan": dict(eps=float("nan")), "feature 11": dict(feature=11), "feature -1": dict(feature=-1), "feature name": dict(feature="pitch"),
        "feature 2.0": dict(feature=2.0), "cut nan": dict(cut=float("nan")), "a nan in cut": dict(cut=nan_cut), "cut [944]": dict(cut=np.zeros(N_STATES - 1)),
        "cut [1, 945]": dict(cut=np.zeros((1, N_STATES))), "cut [2835]": dict(cut=np.zeros(N_CELLS)),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            ops.split_model(cfg, qa, qb, **dict(good, **kw))
            pytest.fail(what)
    with pytest.raises(ValueError, match="x MDP"):
        ops.split_model(simulation_config(working_curriculum_step=4, two_axis=1, quirks=Q_PAPER, dtype=F32), qa, qb, **good)
    for tables in ((qa[:-1], qb[:-1]), (np.zeros((0, 2835)), np.zeros((0, 2835))), (np.tile(qa, (9, 1)), np.tile(qb, (9, 1)))):
        with pytest.raises(ValueError):
            ops.split_model(cfg, *tables, **good)
    ops.split_model_check_args(cfg, 8, (1 << 18) - 64, 64, 4095, 1.0)  # just below 2^30 feature terms, the most sets
    with pytest.raises(AssertionError):                               # and a well-formed call does reach the library
        ops.split_model(cfg, qa, qb, **good)
    with pytest.raises(AssertionError):
        ops.split_model(cfg, qa, qb, **dict(good, cut=np.full(N_STATES, np.inf), feature=10))


def test_feature_means_divide_the_sums_by_the_state_s_visits():
    m = Split().go(0, 4, 0, 5, 3).go(1, 4, 2, 5, 1).end(1, 4, 1, SUCCESS, 4).value(4, 8 * 0.375).go(0, 7, 1, 7, 2).value(7, -2 * 1.5)
    means = evaluation.feature_means(m.r)
    assert means.shape == (1, N_STATES) and means[0, 4] == 0.375 and means[0, 7] == -1.5
    unvisited = np.ones(N_STATES, bool); unvisited[[4, 7]] = False
    assert (means[0, unvisited] == np.inf).all(), "an unvisited state gets +inf, a valid cut"
    ops.split_cut_array(means[0])
    with pytest.raises(ValueError):
        evaluation.feature_means({"pairs": m.r["pairs"][0], "terminal": m.r["terminal"][0], "feat_sum_fx": m.r["feat_sum_fx"]})


def test_split_divergence_on_identical_disjoint_and_under_visited_halves():
    m = Split()
    m.go(0, 0, 0, 1, 30).go(0, 0, 0, 2, 10).go(1, 0, 0, 1, 60).go(1, 0, 0, 2, 20)       # identical halves, one from twice the visits
    m.go(0, 6, 2, 6, 30).go(1, 6, 2, 7, 30)                                              # disjoint
    m.end(0, 4, 1, SUCCESS, 15).go(0, 4, 1, 5, 15).end(1, 4, 1, SUCCESS, 40)             # the terminal codes are part of the alphabet
    m.go(0, 8, 0, 1, 100).go(1, 8, 0, 2, 29)                                             # half 1 under min_visits
    d = evaluation.split_divergence(m.r)
    assert d.shape == (1, N_CELLS) and d[0, 0] == 0.0 and d[0, 6 * 3 + 2] == 1.0 and d[0, 4 * 3 + 1] == pytest.approx(0.5)
    assert np.isnan(d[0, 8 * 3]) and np.isnan(d[0, 1]) and np.isnan(d[0]).sum() == N_CELLS - 3
    assert evaluation.split_divergence(m.r, min_visits=29)[0, 8 * 3] == 1.0
    with pytest.raises(ValueError):
        evaluation.split_divergence(m.r, min_visits=0)


def two_cell_example():
    """cells c0 = (0, 0), c1 = (1, 0), c2 = (2, 0) — c2's half 1 is under-visited under the feature and so is not compared, although the coin splits it wide"""
    f = Split()
    f.go(0, 0, 0, 1, 30).go(1, 0, 0, 2, 30)                                    # c0: disjoint, distance 1, 60 visits
    f.go(0, 1, 0, 3, 40).go(1, 1, 0, 3, 20).end(1, 1, 0, SUCCESS, 20)          # c1: (1, 0) against (1/2, 1/2): distance 1/2, 80 visits
    f.go(0, 2, 0, 4, 30).go(0, 2, 0, 5, 20).go(1, 2, 0, 5, 10)                 # c2: 50 and 10 visits
    c = Split()
    c.go(0, 0, 0, 1, 15).go(0, 0, 0, 2, 15).go(1, 0, 0, 1, 15).go(1, 0, 0, 2, 15)                              # c0: distance 0
    c.go(0, 1, 0, 3, 32).end(0, 1, 0, SUCCESS, 8).go(1, 1, 0, 3, 28).end(1, 1, 0, SUCCESS, 12)                 # c1: (0.8, 0.2) against (0.7, 0.3): 0.1
    c.go(0, 2, 0, 4, 30).go(1, 2, 0, 5, 30)                                                                    # c2: distance 1, 30 visits in each half
    return f, c


def test_aliasing_table_on_a_two_cell_example_computed_by_hand():
    f, c = two_cell_example()
    t = evaluation.aliasing_table({"hidden": f.r, "the coin itself": c.r}, c.r)
    row = t["hidden"]
    assert row["cells"] == 2, "c2 is under-visited under the feature: not compared"
    # distances (1/2 with 80 visits, 1 with 60): the cumulative visits reach 70 of 140 at 1/2
    assert row["median"] == pytest.approx(0.5)
    # the coin over the same cells: (0 with 60 visits, 0.1 with 80): reaches 70 at 0.1; 95th percentile of (0, 0.1) = 0.095
    assert row["coin_median"] == pytest.approx(0.1) and row["coin_p95"] == pytest.approx(0.095)
    assert row["above_coin_p95"] == 1.0 and row["half1_share"] == pytest.approx(80 / 200)
    # the coin against itself has all three cells: its percentile is then taken over (0, 0.1, 1), and c2's distance 1 moves it
    own = t["the coin itself"]
    assert own["cells"] == 3 and own["coin_p95"] == pytest.approx(np.percentile([0.0, 0.1, 1.0], 95)) and own["coin_p95"] > 0.9
    assert own["median"] == own["coin_median"] == pytest.approx(0.1) and own["above_coin_p95"] == pytest.approx(1 / 3) and own["half1_share"] == pytest.approx(0.5)
    # nothing compared: NaN, not an error
    none = evaluation.aliasing_table({"hidden": f.r}, c.r, min_visits=1000)["hidden"]
    assert none["cells"] == 0 and np.isnan(none["median"]) and np.isnan(none["coin_p95"]) and none["half1_share"] == pytest.approx(0.4)
    assert "hidden" in evaluation.format_aliasing_table(t)
