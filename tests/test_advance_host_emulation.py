"""Per-learner curriculum levels on the CPU: csrc/dql_advance.hpp's worklist and advance step, with csrc/dql_learner.hpp's
learner_periods, held `==` to the yardstick of tests/advance_checks.py (CPU only, no GPU).

tests/host_emu/advance_emu.cpp compiles the real headers as host C++ and does what dql_ensemble_run does in curriculum mode: advance at the multiples of E,
worklist, wave by wave.  It is a stand-alone program run as its own process, built twice: plain, and with ASan + UBSan (any report fails); the builds, the
child process and the reader of the result (the learners, the level arrays, the period index) are tests/host_emu_harness.py's; the job's layout is this module's.  The cases are those
of tests/test_gpu_ensemble_advance.py; the sanitized build flies the first 24 learners for 384 periods, and the 24 learners of the cases from trained tables
(`advance_checks.TRAINED_CASE`, `TRAINED_CASE_PAPER`, `TRAINED_FROM_3`) whole."""
import struct

import numpy as np
import pytest

from dql_multirotor_landing_amd import ensemble
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import advance_checks as ac
import host_emu_harness as heh

CASE = ac.CASE
CELLS_PER_LEVEL = N_CELLS // 5
SHORT = 384

emu = heh.emu_fixture("advance_emu")


def run_emu(exe, tmp, runs, n=None, dtype=F32, sanitized=False, **over):
    c = dict(CASE, **over)
    n = c["n"] if n is None else n
    cfg = ac.case_config(c, dtype)
    tables = ac.case_tables(c, n)
    cb = bytes(cfg.to_c())
    alpha = cfg.alpha_table()
    sch = ac.case_schedules(c)
    r8 = list(runs) + [0] * (8 - len(runs))
    hdr = [len(cb), cfg.dtype, n, len(runs), *r8, len(alpha), c["E"], c["last_level"], int(c.get("advance_exhausted", True)), c["log_capacity"]]
    for s in sch:
        hdr += [len(s["eps"]), s["window"], s["min_successes"], s["max_episodes"]]
    hdr += [int(tables is not None)]
    hdr += [0] * (40 - len(hdr))
    job = (struct.pack("<40i", *hdr) + struct.pack("<q", c["seed"]) + cb + np.asarray(ac.case_ratios(c), np.float64).tobytes() + alpha.tobytes()
           + b"".join(np.asarray(s["eps"], np.float64).tobytes() for s in sch)
           + b"".join(np.ascontiguousarray(t, np.float64).tobytes() for t in (tables or ())))
    return heh.learner_result(heh.run(exe, job, tmp, "advance", sanitized), n, c["log_capacity"], cfg, tail=("levels",), periods=sum(runs))


@pytest.fixture(scope="module")
def yard():
    y = ac.case_yardstick()
    ac.assert_case_conditions(y)
    return y, y.result()


@pytest.fixture(scope="module")
def main(emu, tmp_path_factory):
    return run_emu(emu["plain"], tmp_path_factory.mktemp("advance_main"), (CASE["periods"],))


def test_python_argument_checks_come_before_the_library_is_touched():
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the library was touched: {name}")

    ens = object.__new__(SequentialEnsemble)
    ens.n, ens.lib, ens._h = 8, Untouchable(), None
    for bad in (dict(advance_every=-1), dict(advance_every=4097), dict(last_level=5), dict(last_level=-1), dict(ratios=[1.0] * 4), dict(ratios=[1.0, np.nan, 1.0, 1.0, 1.0]),
                dict(ratios=[1.0, 1.0, np.inf, 1.0, 1.0])):
        with pytest.raises(ValueError):
            ens.set_curriculum(**{"last_level": 4, "advance_every": 64, **bad})
    for bad in (dict(level=-1), dict(level=5), dict(window=0), dict(window=129), dict(min_successes=0), dict(max_episodes=0), dict(eps=[])):
        with pytest.raises(ValueError):
            ens.set_level_schedules(**{"level": 1, "eps": [0.0], "window": 4, "min_successes": 3, "max_episodes": 6, **bad})
    ens._h = None  # (nothing to close)


def test_whole_run_equals_the_yardstick_f32(yard, main):
    ac.assert_equal(main, yard[1], "run(1024), float32")


def test_whole_run_equals_the_yardstick_f64(emu, tmp_path):
    y = ac.case_yardstick(dtype=F64, n=ac.SMALL, periods=SHORT)
    want = y.result()
    assert len(set(want["level"].tolist())) >= 3 and y.advanced_exhausted >= 1
    ac.assert_equal(run_emu(emu["plain"], tmp_path, (SHORT,), n=ac.SMALL, dtype=F64), want, "run(384), float64")


@pytest.mark.parametrize("runs", [(7, 1017), (7, 100, 917), (64, 1, 63, 896)], ids=lambda r: "+".join(map(str, r)))
def test_splits_equal_one_run(emu, main, runs, tmp_path):
    assert sum(runs) == CASE["periods"]
    ac.assert_equal(run_emu(emu["plain"], tmp_path, runs), main, f"runs {runs} against run(1024)")


def test_first_24_learners_do_not_depend_on_the_other_56(emu, main, tmp_path):
    first = list(range(ac.SMALL))
    ac.assert_equal(main, run_emu(emu["plain"], tmp_path, (CASE["periods"],), n=ac.SMALL), "L = 80 against L = 24", learners=(first, first))


def test_exhausted_learners_stay_where_they_froze_when_they_do_not_advance(emu, tmp_path):
    y = ac.case_yardstick(advance_exhausted=False)
    want = y.result()
    assert y.advanced_exhausted == 0 and y.advanced_promoted >= 1 and y.n_unfinished() == 0 and (want["level"] == 1).any()
    got = run_emu(emu["plain"], tmp_path, (CASE["periods"],), advance_exhausted=False)
    ac.assert_equal(got, want, "advance_exhausted = 0")
    again = run_emu(emu["plain"], tmp_path, (CASE["periods"], 3, 200), advance_exhausted=False)
    ac.assert_equal(again, got, "run(3); run(200) with everyone finished")


def test_last_level_2_is_never_exceeded(emu, main, tmp_path):
    got = run_emu(emu["plain"], tmp_path, (CASE["periods"],), last_level=2)
    assert got["level"].max() == 2 and (got["frozen"].astype(bool) & (got["level"] == 2)).any() and (got["entered_period"][3:] == -1).all()
    for t in ("qa", "qb", "count"):
        assert not got[t][:, 3 * CELLS_PER_LEVEL:].any(), f"{t}: cells of levels 3 and 4 were written"
    # a learner's way up to level 2 does not depend on where the curriculum ends
    assert np.array_equal(got["entered_period"][:3], main["entered_period"][:3]) and (got["entered_period"][2] >= 0).any()
    assert np.array_equal(got["promoted_at"][:2], main["promoted_at"][:2]) and np.array_equal(got["episodes_at"][:2], main["episodes_at"][:2])


def test_ring_is_cleared_on_advance(emu, tmp_path):
    """`advance_checks.RING_CASE`: one success promotes above level 0, and learners arrive there with level-0 successes in their ring"""
    y = ac.case_yardstick(**ac.RING_CASE)
    want = y.result()
    ac.assert_ring_case_conditions(y, want)
    ac.assert_equal(run_emu(emu["plain"], tmp_path, (7, ac.RING_CASE["periods"] - 7), **ac.RING_CASE), want, "the ring case")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_clean_under_asan_and_ubsan(emu, yard, dtype, tmp_path):
    """the first 24 learners, 7 + 377 periods, through the sanitized build; float32 against the first 24 of the yardstick's 80 (a learner does not depend on the others)"""
    first = list(range(ac.SMALL))
    got = run_emu(emu["san"], tmp_path, (7, SHORT - 7), n=ac.SMALL, dtype=dtype, sanitized=True)
    if dtype == F32:
        y = ac.case_yardstick(n=ac.SMALL, periods=SHORT)
    else:
        y = ac.case_yardstick(dtype=F64, n=ac.SMALL, periods=SHORT)
    assert y.advanced_exhausted >= 1 and len(set(y.level.tolist())) >= 3
    ac.assert_equal(got, y.result(), f"sanitized, dtype {dtype}", learners=(first, first))


# ---- from trained tables: promotions through the ring above level 0, transfers of non-zero blocks of both tables, the k = 0 wrap with a ratio that shows ----
TRAINED = {"0x7f": ac.TRAINED_CASE, "0x40": ac.TRAINED_CASE_PAPER, "from-3": ac.TRAINED_FROM_3}


@pytest.fixture(scope="module")
def trained_yard():
    """per (case, dtype, overrides): the yardstick of the case's first 24 learners (3 - 5 s each on the CPU), its conditions asserted, and its result"""
    cache = {}

    def get(name, dtype=F32, **over):
        key = (name, dtype, tuple(sorted(over.items())))
        if key not in cache:
            c = dict(TRAINED[name], n=ac.SMALL, **over)
            y = ac.case_yardstick(dtype=dtype, **c)
            if not over:
                ac.assert_trained_case_conditions(y, c)
            cache[key] = (y, y.result(), c)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(TRAINED))
def test_trained_whole_run_equals_the_yardstick(emu, trained_yard, name, dtype, tmp_path):
    y, want, c = trained_yard(name, dtype)
    ac.assert_equal(run_emu(emu["plain"], tmp_path, (c["periods"],), dtype=dtype, **c), want, f"trained case {name}, dtype {dtype}")


@pytest.mark.parametrize("runs", [(7, 1017), (33, 31, 960)], ids=lambda r: "+".join(map(str, r)))
@pytest.mark.parametrize("name", ["0x7f", "0x40"])
def test_trained_splits_equal_the_yardstick(emu, trained_yard, name, runs, tmp_path):
    """cuts off the multiples of E = 32, one period after one, and on one"""
    y, want, c = trained_yard(name)
    assert sum(runs) == c["periods"] and any(r % c["E"] for r in runs)
    ac.assert_equal(run_emu(emu["plain"], tmp_path, runs, **c), want, f"trained case {name}, runs {runs}")


@pytest.mark.parametrize("name", ["0x7f", "0x40"])
def test_trained_last_level_2_is_never_exceeded(emu, trained_yard, name, tmp_path):
    y, want, c = trained_yard(name, last_level=2)
    done = want["frozen"].astype(bool) & (want["level"] == 2)
    assert want["level"].max() == 2 and (done & (want["promotion_episode"] >= 0)).any(), "on the yardstick nobody finishes at level 2 by promotion"
    assert (want["entered_period"][3:] == -1).all() and y.promoted_from[1] >= 1
    got = run_emu(emu["plain"], tmp_path, (c["periods"],), **c)
    ac.assert_equal(got, want, f"trained case {name}, last_level = 2")
    tables = ac.case_tables(c, c["n"])
    for t, w in zip(("qa", "qb", "count"), tables):
        assert np.array_equal(got[t][:, 3 * CELLS_PER_LEVEL:], w[:, 3 * CELLS_PER_LEVEL:]), f"{t}: cells of levels 3 and 4 were written"


def test_trained_exhausted_learners_do_not_advance(emu, trained_yard, tmp_path):
    """advance_exhausted = 0 on the 0x7f case: learners that promoted above level 0 go on, the ones out of episodes stay where they froze"""
    y, want, c = trained_yard("0x7f", advance_exhausted=False)
    exhausted = want["frozen"].astype(bool) & (want["promotion_episode"] < 0)
    assert y.advanced_exhausted == 0 and (y.promoted_from[1:] > 0).sum() >= 2 and (exhausted & (want["level"] >= 1) & (want["level"] < 4)).any()
    ac.assert_equal(run_emu(emu["plain"], tmp_path, (c["periods"],), **c), want, "trained case 0x7f, advance_exhausted = 0")


@pytest.mark.parametrize("name,dtype", [("0x7f", F32), ("0x40", F64), ("from-3", F32)], ids=["0x7f-f32", "0x40-f64", "from-3-f32"])
def test_trained_clean_under_asan_and_ubsan(emu, trained_yard, name, dtype, tmp_path):
    """the whole case of 24 learners through the sanitized build, in two runs"""
    y, want, c = trained_yard(name, dtype)
    ac.assert_equal(run_emu(emu["san"], tmp_path, (7, c["periods"] - 7), dtype=dtype, sanitized=True, **c), want, f"sanitized trained case {name}, dtype {dtype}")
