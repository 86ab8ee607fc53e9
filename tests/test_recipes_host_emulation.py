"""Per-learner recipes on the CPU: csrc/dql_recipes.hpp's worklist by (recipe, level) and the advance step under a learner's own rule,
with csrc/dql_learner.hpp's learner_periods, held `==` to the yardsticks of tests/recipe_checks.py (CPU only, no GPU).

tests/host_emu/recipes_emu.cpp compiles the real headers as host C++ and does what dql_ensemble_run does with recipes installed.  It is a stand-alone program
run as its own process, built twice: plain, and with ASan + UBSan (any report fails); the builds, the child process and the reader of the learners' result are
tests/host_emu_harness.py's.  The case is that of tests/test_gpu_ensemble_recipes.py with 28 learners (20 / 4 / 4 members)."""
import numpy as np
import pytest

from dql_multirotor_landing_amd.config import F32, F64
from dql_multirotor_landing_amd.ensemble import Recipe, SequentialEnsemble, LevelSchedule

import advance_checks as ac
import host_emu_harness as heh
import recipe_checks as rc
import test_advance_host_emulation as adv_emu

CASE = rc.CASE
N = rc.N_SMALL
WAVE, LEVELS = 64, 5

emu = heh.emu_fixture("recipes_emu")
advance_emu = heh.emu_fixture("advance_emu")


def run_emu(exe, tmp, runs, n=N, dtype=F32, sanitized=False, recipes=None, recipe_of=None, tables=True):
    cfg = rc.case_config(dtype)
    recipes = rc.case_recipes(dtype) if recipes is None else recipes
    of = rc.case_recipe_of(n) if recipe_of is None else np.asarray(recipe_of, np.int32)
    job = heh.recipes_job(cfg, n, CASE["seed"], runs, CASE["E"], CASE["log_capacity"], recipes, of, rc.ec.trained_tables(n) if tables else None)
    return heh.learner_result(heh.run(exe, job, tmp, "recipes", sanitized), n, CASE["log_capacity"], cfg, tail=("levels",), periods=sum(runs))


def run_worklist(exe, tmp, frozen, level, recipe_of, n_recipes, cap, sanitized=False):
    n = len(frozen)
    job = heh.recipes_header(rc.case_config(), n, CASE["seed"], (), CASE["E"], CASE["log_capacity"], n_recipes, 0, mode=1, cap=cap) + b"".join(np.ascontiguousarray(a, np.int32).tobytes() for a in (recipe_of, frozen, level))
    r = heh.Reader(heh.run(exe, job, tmp, "worklist", sanitized))
    n_waves, faults, capacity = (int(v) for v in r.take(np.int64, (3,)))
    out = r.take(np.int32, (cap,)), r.take(np.int32, (cap // WAVE,)), r.take(np.int32, (cap // WAVE,))
    r.done()
    return n_waves, faults, capacity, out


@pytest.fixture(scope="module")
def yards():
    """per dtype: the three yardsticks over the 28 learners (about 6 s together on the CPU), their conditions asserted"""
    cache = {}

    def get(dtype=F32):
        if dtype not in cache:
            cache[dtype] = rc.case_yardsticks(N, dtype)
            rc.assert_case_conditions(cache[dtype])
        return cache[dtype]
    return get


@pytest.fixture(scope="module")
def main(emu, tmp_path_factory):
    return run_emu(emu["plain"], tmp_path_factory.mktemp("recipes_main"), (CASE["periods"],))


def test_python_argument_checks_come_before_the_library_is_touched():
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the library was touched: {name}")

    ens = object.__new__(SequentialEnsemble)
    ens.n, ens.lib, ens._h, ens.cfg = 8, Untouchable(), None, rc.case_config()
    ok, of = Recipe(), np.zeros(8, np.int32)
    lv = lambda **kw: tuple(LevelSchedule(**kw) for _ in range(LEVELS))
    bad_recipes = [Recipe(transfer_order=2), Recipe(transfer_order=-1), Recipe(last_level=5), Recipe(last_level=-1), Recipe(ratios=[1.0] * 4), Recipe(ratios=[1.0, np.nan, 1.0, 1.0, 1.0]),
                   Recipe(ratios=[1.0, 1.0, np.inf, 1.0, 1.0]), Recipe(alpha_table=[]), Recipe(alpha_table=[1.5]), Recipe(alpha_min=-0.1), Recipe(quirks=-1), Recipe(levels=lv()[:4]),
                   Recipe(levels=lv(window=0)), Recipe(levels=lv(window=129)), Recipe(levels=lv(min_successes=0)), Recipe(levels=lv(max_episodes=0)), Recipe(levels=lv(eps=[])),
                   Recipe(levels=lv(eps=[1.5]))]
    for bad in bad_recipes:
        with pytest.raises(ValueError):
            ens.set_recipes([ok, bad], of)
    for bad_of in (np.zeros(7, np.int32), np.full(8, 2, np.int32), np.full(8, -1, np.int32)):
        with pytest.raises(ValueError):
            ens.set_recipes([ok, ok], bad_of)
    with pytest.raises(ValueError):
        ens.set_recipes([ok] * 65, of)
    ens._h = None  # (nothing to close)


def test_whole_run_equals_the_yardsticks_f32(yards, main):
    rc.assert_equal_by_recipe(main, yards(), "run(1024), float32")


def test_whole_run_equals_the_yardsticks_f64(emu, yards, tmp_path):
    rc.assert_equal_by_recipe(run_emu(emu["plain"], tmp_path, (CASE["periods"],), dtype=F64), yards(F64), "run(1024), float64")


@pytest.mark.parametrize("runs", [(7, 1017), (33, 31, 960)], ids=lambda r: "+".join(map(str, r)))
def test_splits_equal_one_run(emu, main, runs, tmp_path):
    """cuts off the multiples of E = 32, one period after one, and on one"""
    assert sum(runs) == CASE["periods"] and any(r % CASE["E"] for r in runs)
    ac.assert_equal(run_emu(emu["plain"], tmp_path, runs), main, f"runs {runs} against run(1024)")


def test_a_single_reference_order_recipe_equals_the_curriculum_emulation(emu, advance_emu, tmp_path):
    """recipe 0 for everybody is `advance_checks.TRAINED_CASE`: recipes_emu against advance_emu's result, every learner"""
    c = dict(ac.TRAINED_CASE, n=N)
    want = adv_emu.run_emu(advance_emu["plain"], tmp_path, (c["periods"],), **c)
    got = run_emu(emu["plain"], tmp_path, (c["periods"],), recipes=rc.case_recipes()[:1], recipe_of=np.zeros(N, np.int32))
    assert (want["level"] > 0).any() and want["decisions"].min() >= 1
    ac.assert_equal(got, want, "one order-0 recipe against curriculum mode without recipes")


def test_relabelled_recipes_change_nothing_per_learner(emu, main, tmp_path):
    recipes, of = rc.case_recipes(), rc.case_recipe_of(N)
    got = run_emu(emu["plain"], tmp_path, (CASE["periods"],), recipes=recipes[::-1], recipe_of=2 - of)
    ac.assert_equal(got, main, "recipes 0 and 2 swapped")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_clean_under_asan_and_ubsan(emu, yards, dtype, tmp_path):
    """the whole case of 28 learners through the sanitized build, in two runs"""
    rc.assert_equal_by_recipe(run_emu(emu["san"], tmp_path, (7, CASE["periods"] - 7), dtype=dtype, sanitized=True), yards(dtype), f"sanitized, dtype {dtype}")


# ---- build_worklist_recipes ----
def check_worklist(frozen, level, recipe_of, n_recipes, n_waves, worklist, wave_recipe, wave_level):
    """one (recipe, level) per wave, segments in (recipe, level) order with learners ascending, padding -1 at a segment's end only, every live learner once"""
    live = [l for l in range(len(frozen)) if not frozen[l] and 0 <= recipe_of[l] < n_recipes and 0 <= level[l] < LEVELS]
    want = sorted(live, key=lambda l: (recipe_of[l], level[l], l))
    flown = [int(l) for l in worklist[:n_waves * WAVE] if l >= 0]
    assert flown == want
    keys = [(int(wave_recipe[w]), int(wave_level[w])) for w in range(n_waves)]
    assert keys == sorted(keys)
    for w in range(n_waves):
        lanes = worklist[w * WAVE:(w + 1) * WAVE]
        members = lanes[lanes >= 0]
        assert len(members) >= 1 and (lanes[:len(members)] >= 0).all(), "padding inside a wave, or an empty wave"
        assert all((recipe_of[l], level[l]) == keys[w] for l in members)
        assert len(members) == WAVE or w == n_waves - 1 or keys[w + 1] != keys[w], "a padded wave inside a segment"
    assert set(np.unique(worklist[:n_waves * WAVE])) <= set(live) | {-1}
    assert (worklist[n_waves * WAVE:] == -2).all() and (wave_recipe[n_waves:] == -2).all() and (wave_level[n_waves:] == -2).all(), "written beyond the waves it returned"


@pytest.mark.parametrize("kind", ["plain", "san"])
def test_worklist_properties(emu, kind, tmp_path):
    rng = np.random.default_rng(3)
    san = kind == "san"
    for n, R in ((112, 3), (1, 1), (64, 1), (65, 2), (700, 64), (333, 7)):
        cap = (n // WAVE + LEVELS * R) * WAVE
        frozen = (rng.random(n) < 0.3).astype(np.int32)
        level, of = rng.integers(0, LEVELS, n).astype(np.int32), rng.integers(0, R, n).astype(np.int32)
        n_waves, faults, capacity, (wl, wr, wv) = run_worklist(emu[kind], tmp_path, frozen, level, of, R, cap, san)
        assert faults == 0 and capacity == cap
        check_worklist(frozen, level, of, R, n_waves, wl, wr, wv)
    # the worst case the capacity is for: every (recipe, level) holds k 64 + 1 learners
    R = 3
    of, level = np.repeat(np.arange(R), LEVELS * 65).astype(np.int32), np.tile(np.repeat(np.arange(LEVELS), 65), R).astype(np.int32)
    n = of.size
    cap = (n // WAVE + LEVELS * R) * WAVE
    n_waves, faults, capacity, (wl, wr, wv) = run_worklist(emu[kind], tmp_path, np.zeros(n, np.int32), level, of, R, cap, san)
    assert faults == 0 and n_waves == 2 * LEVELS * R and n_waves * WAVE <= cap
    check_worklist(np.zeros(n, np.int32), level, of, R, n_waves, wl, wr, wv)
    # out-of-range recipes and levels of LIVE learners are counted and left out; frozen ones are not looked at
    n, R = 100, 4
    frozen, level, of = np.zeros(n, np.int32), rng.integers(0, LEVELS, n).astype(np.int32), rng.integers(0, R, n).astype(np.int32)
    of[[3, 50]] = (R, -1); level[[7, 51, 52]] = (LEVELS, -1, 99); frozen[60] = 1; of[60] = 77
    cap = (n // WAVE + LEVELS * R) * WAVE
    n_waves, faults, _, (wl, wr, wv) = run_worklist(emu[kind], tmp_path, frozen, level, of, R, cap, san)
    assert faults == 5
    check_worklist(frozen, level, of, R, n_waves, wl, wr, wv)
    # a capacity too small: whole waves only, the learners without room counted, nothing written beyond it
    n_waves, faults, _, (wl, wr, wv) = run_worklist(emu[kind], tmp_path, np.zeros(130, np.int32), np.zeros(130, np.int32), np.zeros(130, np.int32), 1, 2 * WAVE + 5, san)
    assert n_waves == 2 and faults == 2 and wl[:128].tolist() == list(range(128)) and (wl[128:] == -2).all()
    # a number of recipes out of range: counted, nothing built
    for bad in (0, 65):
        n_waves, faults, _, (wl, wr, wv) = run_worklist(emu[kind], tmp_path, np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32), bad, 6 * WAVE, san)
        assert n_waves == 0 and faults == 1 and (wl == -2).all()
