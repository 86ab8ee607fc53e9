"""The host side of the refined state that needs no GPU: the argument checks `ops.score_refined` and `SequentialEnsemble.set_refinement` / `set_refined_tables` /
`score_refined` make before they touch the library, the ctypes bindings against the header, `evaluation.refinement_cut` against a closed form, and the refusals
of the two scripts' flags."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import CHECK_NAMES, F32, N_CELLS, Q_PAPER, simulation_config, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

ROOT = Path(__file__).resolve().parent.parent
N_STATES, N_CODES = N_CELLS // 3, len(CHECK_NAMES)
HDR = (ROOT / "include" / "dql.h").read_text()
DIAG = (ROOT / "include" / "dql_diag.h").read_text()


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) by a call that must be refused on the host")


def no_library():
    raise AssertionError("the library was loaded for a call that must be refused on the host")


def host_only_ensemble(n=6, **attrs):
    """a SequentialEnsemble's host side without a device behind it: any library call fails the test"""
    e = object.__new__(SequentialEnsemble)
    e.__dict__.update(dict(lib=NoLibrary(), _h=None, n=n, teams=False, envs_per_learner=1, n_envs=n, _nstep=0, _advance_every=0, _team_nstep=0, _team_every=0,
                           cfg=training_config(0, dtype=F32)), **attrs)
    return e


def test_bindings_have_the_arguments_of_the_header_and_the_limits_agree():
    for name, n_args in (("dql_ensemble_set_refinement", 3), ("dql_ensemble_get_refinement", 3), ("dql_ensemble_get_refined_tables", 6), ("dql_ensemble_set_refined_tables", 6),
                         ("dql_score_refined", 15), ("dql_ensemble_score_refined", 12), ("dql_diag_score_refined_last", 2)):
        assert len(_lib.SYMBOLS[name][1]) == n_args, name
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR + DIAG, re.S)
        assert decl and len(decl.group(1).split(",")) == n_args, name
    # dql_score_refined is dql_score's binding with (feature, cut) in front of the tables; the ensemble twin is dql_ensemble_score's
    s, r = _lib.SYMBOLS["dql_score"][1], _lib.SYMBOLS["dql_score_refined"][1]
    assert r[:7] == s[:7] and r[9:] == s[7:] and _lib.SYMBOLS["dql_ensemble_score_refined"][1] == _lib.SYMBOLS["dql_ensemble_score"][1]
    assert _lib.SYMBOLS["dql_ensemble_get_refined_tables"][1] == _lib.SYMBOLS["dql_ensemble_get_tables"][1]
    assert re.search(r"#define DQL_SCORE_REFINED_MAX_TABLES 4096\b", HDR) and ops.SCORE_REFINED_MAX_TABLES == 4096
    assert re.search(r"#define DQL_ABI_VERSION 6\b", HDR) and _lib.ABI_VERSION == 6


def test_score_refined_refuses_bad_arguments_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", no_library)
    cfg = simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32)
    qa = qb = np.zeros((2, 2, N_CELLS))
    good = dict(feature="pitch_sp", cut=0.0, envs_per_table=64, seed=1, episodes=1, max_steps=600)
    nan_cut = np.zeros(N_STATES); nan_cut[17] = np.nan
    bad = {
        "envs 0": dict(envs_per_table=0), "envs 100": dict(envs_per_table=100), "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65),
        "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097), "feature 11": dict(feature=11), "feature -1": dict(feature=-1),
        "feature name": dict(feature="pitch"), "feature 2.0": dict(feature=2.0), "cut nan": dict(cut=float("nan")), "a nan in cut": dict(cut=nan_cut),
        "cut [944]": dict(cut=np.zeros(N_STATES - 1)), "cut [2835]": dict(cut=np.zeros(N_CELLS)),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            ops.score_refined(cfg, qa, qb, **dict(good, **kw))
            pytest.fail(what)
    for two in (simulation_config(working_curriculum_step=4, two_axis=1, dtype=F32), simulation_config(working_curriculum_step=4, trajectory=1, dtype=F32)):
        with pytest.raises(ValueError, match="x MDP"):
            ops.score_refined(two, qa, qb, **good)
    for tables in ((np.zeros((3, N_CELLS)), np.zeros((3, N_CELLS))), (np.zeros(N_CELLS), np.zeros(N_CELLS)), (np.zeros((1, 3, N_CELLS)), np.zeros((1, 3, N_CELLS))), (np.zeros((0, 2, N_CELLS)), np.zeros((0, 2, N_CELLS))),
                   (np.zeros((2, 2, N_CELLS)), np.zeros((1, 2, N_CELLS))), (np.zeros((4097, 2, 1)), np.zeros((4097, 2, 1)))):
        with pytest.raises(ValueError):
            ops.score_refined(cfg, *tables, **good)
    ops.score_refined_check_args(cfg, 4096, 64, 64, 4096)
    with pytest.raises(ValueError):
        ops.score_refined_check_args(cfg, 4097, 64, 1, 600)
    a, b = ops.refined_table_pair(np.zeros((2, N_CELLS)), np.ones((2, N_CELLS)))
    assert a.shape == b.shape == (1, 2, N_CELLS), "one refined set may be given as [2, 2835]"
    with pytest.raises(AssertionError):  # and a well-formed call does reach the library
        ops.score_refined(cfg, qa, qb, **dict(good, cut=np.full(N_STATES, -np.inf), feature=0))


def test_the_ensemble_refuses_bad_arguments_before_the_library_is_touched():
    e = host_only_ensemble()
    nan_cut = np.zeros(N_STATES); nan_cut[944] = np.nan
    for feature, cut in (("pitch", 0.0), (11, 0.0), (-1, 0.0), (1.0, 0.0), (None, 0.0), ("pitch_sp", float("nan")), ("pitch_sp", nan_cut), ("pitch_sp", np.zeros(944)),
                         ("pitch_sp", np.zeros((945, 1))), ("pitch_sp", np.zeros(N_CELLS))):
        with pytest.raises(ValueError):
            e.set_refinement(feature, cut)
    for attrs in (dict(teams=True), dict(envs_per_learner=2), dict(_nstep=2), dict(_advance_every=64), dict(_team_every=64), dict(_team_nstep=2), dict(_recipes=[object()])):
        with pytest.raises(ValueError):
            host_only_ensemble(**attrs).set_refinement("pitch_sp", 0.0)
    with pytest.raises(AssertionError):  # a well-formed call does reach the library
        e.set_refinement("pitch_sp", np.full(N_STATES, np.inf))
    ok = np.zeros((6, 2, N_CELLS))
    for kw in (dict(), dict(qa=np.zeros((6, N_CELLS))), dict(qa=np.zeros((6, 3, N_CELLS))), dict(qa=ok, qb=np.zeros((5, 2, N_CELLS))), dict(qa=ok, first=1),
               dict(qa=ok[:2], first=5), dict(qa=ok[:1], first=-1), dict(qa=np.zeros((6, 2 * N_CELLS)))):
        with pytest.raises(ValueError):
            e.set_refined_tables(**kw)
    for first, count in ((-1, 2), (5, 2), (0, 7), (6, 1), (0, 0)):
        with pytest.raises(ValueError):
            e.get_refined_tables(first, count)
        with pytest.raises(ValueError):
            e.score_refined(e.cfg, first=first, count=count)
    for kw in (dict(envs_per_learner=63), dict(episodes=0), dict(episodes=65), dict(max_steps=0), dict(max_steps=4097)):
        with pytest.raises(ValueError):
            e.score_refined(e.cfg, **kw)
    with pytest.raises(ValueError, match="x MDP"):
        e.score_refined(simulation_config(working_curriculum_step=4, two_axis=1, dtype=F32))


def split_result(sums, visits, k_sets=1):
    """a split-model result whose feat_sum_fx and state visits are the given [K][945] arrays (the visits as decisions of action 0 that end the episode)"""
    r = {"pairs": np.zeros((k_sets, 2, N_CELLS, N_STATES), np.uint32), "terminal": np.zeros((k_sets, 2, N_CELLS, N_CODES), np.int64),
         "feat_sum_fx": np.asarray(sums, np.int64).reshape(k_sets, N_STATES)}
    r["terminal"][:, 0, 0::3, 0] = np.asarray(visits, np.int64).reshape(k_sets, N_STATES)
    return r


def test_refinement_cut_merges_each_level_s_own_block_and_leaves_unvisited_states_at_infinity():
    rng = np.random.default_rng(1)
    visits = rng.integers(0, 4, size=(5, N_STATES))      # zeros are common: unvisited states
    sums = rng.integers(-(1 << 24), 1 << 24, size=(5, N_STATES)) * (visits > 0)
    cut = evaluation.refinement_cut([split_result(sums[k], visits[k]) for k in range(5)])
    lvl = np.arange(N_STATES) // 189
    own_v, own_s = visits[lvl, np.arange(N_STATES)], sums[lvl, np.arange(N_STATES)]
    want = np.where(own_v > 0, own_s / float(1 << 20) / np.maximum(own_v, 1), np.inf)
    assert cut.shape == (N_STATES,) and cut.dtype == np.float64 and np.array_equal(cut, want)
    assert (own_v == 0).any() and np.isinf(cut[own_v == 0]).all() and np.isfinite(cut[own_v > 0]).all()
    # a state visited at ANOTHER level only stays at +inf: level 0's pass counts in state 200 (level 1), level 1's pass does not
    v = np.zeros((2, N_STATES), np.int64); s = np.zeros((2, N_STATES), np.int64)
    v[0, 200], s[0, 200] = 3, 3 << 20
    v[1, 201], s[1, 201] = 2, 5 << 20
    c = evaluation.refinement_cut({0: split_result(s[0], v[0]), 1: split_result(s[1], v[1])})
    assert np.isinf(c[200]) and c[201] == 2.5 and np.isinf(np.delete(c, 201)).all()
    # table sets are pooled: sum of sums over sum of visits; one level alone; what it gives is a valid cut
    pooled = evaluation.refinement_cut({4: split_result([np.eye(1, N_STATES, 800)[0] * (3 << 20), np.eye(1, N_STATES, 800)[0] * (1 << 20)],
                                                        [np.eye(1, N_STATES, 800)[0] * 1, np.eye(1, N_STATES, 800)[0] * 3], k_sets=2)})
    assert pooled[800] == 1.0 and np.isinf(np.delete(pooled, 800)).all()
    ops.split_cut_array(cut)
    with pytest.raises(ValueError):
        evaluation.refinement_cut({5: split_result(s[0], v[0])})
    with pytest.raises(ValueError):
        evaluation.refinement_cut([{"pairs": np.zeros((2, N_CELLS, N_STATES)), "terminal": np.zeros((2, N_CELLS, N_CODES)), "feat_sum_fx": np.zeros((1, N_STATES))}])


def run_script(name, *args):
    return subprocess.run([sys.executable, str(ROOT / "scripts" / name), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args,word", [
    (["--refine", "pitch_sp"], "go together"), (["--refine-cut", "0.5"], "go together"),
    (["--refine", "pitch_sp", "--refine-cut", "0.0", "--per-learner"], "--per-learner"), (["--refine", "pitch_sp", "--refine-cut", "0.0", "--recipes", "r.json"], "--recipes"),
    (["--refine", "pitch_sp", "--refine-cut", "0.0", "--nstep", "4"], "--nstep"), (["--refine", "pitch_sp", "--refine-cut", "0.0", "--envs-per-learner", "8"], "--envs-per-learner"),
    (["--refine", "pitch", "--refine-cut", "0.0"], "no split feature"), (["--refine", "coin", "--refine-cut", "nan"], "NaN"),
    (["--refine", "coin", "--refine-cut", "no_such_file.npy"], "--refine-cut"),
])
def test_the_training_script_refuses_the_flag_combinations_before_anything_is_built(args, word):
    r = run_script("ensemble_training.py", "--out", "unused.npz", *args)
    assert r.returncode == 2 and word in r.stderr, r.stderr[-600:]


def test_the_simulation_script_wants_cut_out_and_cut_by_together():
    for args in (["--cut-out", "unused.npy"], ["--cut-by", "pitch_sp"]):
        r = run_script("simulation.py", *args)
        assert r.returncode == 2 and "belong together" in r.stderr, r.stderr[-600:]
