"""CPU leg of tests/episode_dtype_checks.py: the float32 ORACLE — the restatement the float32 kernels are held to bit for bit — flown greedily on the
reference's stage-4 tables from reset to every env's terminal, against the float64 oracle flying the same 4 096 envs, for every flavour and two seeds.
The same body through the HIP engine, and one-launch roll-outs of 65 536 pairs: tests/test_gpu_episode_dtypes.py (-m gpu).
22 pairs of flights on 8 oracle threads."""
import copy
import functools

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import F32, F64

import episode_dtype_checks as ec
import rollout_checks as rc
from oracle.oracle import Oracle


def _make(cfg, n, seed):
    return Oracle(cfg, n, seed=seed, n_threads=8)


@pytest.fixture(scope="module")
def tables():
    return rc.stage4_tables()


@functools.lru_cache(maxsize=None)
def _sim_pair():
    """the plain simulation pair, kept for the self-test"""
    return ec.paired_flights(_make, ec.FLAVOURS["sim"][0], rc.stage4_tables(), ec.N_ENVS, ec.SEEDS[0], ec.MAX_STEPS)


def _pair(flavour, seed):
    """flown once per case and left unchanged"""
    if (flavour, seed) == ("sim", ec.SEEDS[0]):
        return _sim_pair()
    return ec.paired_flights(_make, ec.FLAVOURS[flavour][0], rc.stage4_tables(), ec.N_ENVS, seed, ec.MAX_STEPS)


@pytest.mark.parametrize("seed", ec.SEEDS)
@pytest.mark.parametrize("flavour", list(ec.FLAVOURS))
def test_f32_episodes_against_their_f64_twins(flavour, seed):
    """<= 5 % of the envs differ in a decision and <= 0.5 % of the period slots; every env whose decisions all agree ends with the same code after the same
    number of steps, its record fields within BOUNDS of the float64 terminal and the mean difference of its return within CONCORDANT_MEAN_BOUNDS; the flights
    that part show no bias at z = 4 (McNemar on the landing outcome, paired means of steps and cumulative reward)"""
    pair = _pair(flavour, seed)
    m, bal = ec.check(pair, flavour)
    print(flavour, seed, {k: v for k, v in m.items() if k not in ("concordant", "strict_exceptions", "max_abs_per_field")}, bal)


def test_the_bounds_are_four_times_the_recorded_maxima():
    """episode_dtype_checks.BOUNDS is what profiles/f32_episodes_vs_f64.jsonl gives, the file has one line per flavour and seed, and its lines are inside the
    conditions the checks assert"""
    bounds, rows = ec.bounds_from_profile()
    assert bounds == ec.BOUNDS
    assert ec.concordant_mean_bounds_from_profile() == ec.CONCORDANT_MEAN_BOUNDS
    assert sorted((r["flavour"], r["seed"]) for r in rows) == sorted((f, s) for f in ec.FLAVOURS for s in ec.SEEDS)
    for r in rows:
        assert r["n"] == ec.N_ENVS and r["max_steps"] == ec.MAX_STEPS and r["f32_side"] == "oracle"
        assert r["envs_with_a_differing_decision"] <= ec.MAX_DISCORDANT_ENVS * r["n"] and r["differing_period_slots"] <= ec.MAX_DIFFERING_SLOTS * r["f64_periods_flown"]
        assert r["concordant_envs_with_another_code_or_step_count"] == 0
        assert r["mcnemar_z"] <= ec.Z and all(z <= ec.Z for z in r["paired_mean_z"].values())


def test_every_check_turns_red_on_a_flight_that_is_wrong_in_its_way():
    """the plain simulation pair with one thing changed in the float32 flight at a time: each assertion of check() fires on its own kind of error"""
    pair = _sim_pair()
    m = ec.compare(pair)
    conc, disc = np.flatnonzero(m["concordant"]), np.flatnonzero(~m["concordant"])
    contact64 = pair[F64]["code"] == rc.CONTACT

    def changed(**edits):
        p = {F32: copy.deepcopy(pair[F32]), F64: pair[F64]}
        for f, (envs, value) in edits.items():
            if f == "decisions":
                p[F32][f][1, envs] ^= 1
            else:
                p[F32][f][envs] = value if not callable(value) else value(p[F32][f][envs])
        return p

    ec.check(changed(), "sim")
    with pytest.raises(AssertionError, match="agree in every decision and differ at the terminal"):
        ec.check(changed(steps=(conc[:1], lambda v: v + 1)), "sim")
    with pytest.raises(AssertionError, match="agree in every decision and differ at the terminal"):
        ec.check(changed(code=(conc[:1], rc.FLY_X)), "sim")
    with pytest.raises(AssertionError, match="position differs"):
        ec.check(changed(px=(conc[7:8], lambda v: v + 2 * ec.BOUNDS["position"])), "sim")
    with pytest.raises(AssertionError, match="cum differs"):
        ec.check(changed(cum_x=(conc[7:8], lambda v: v - 2 * ec.BOUNDS["cum"])), "sim")
    with pytest.raises(AssertionError, match="decision-concordant envs' mean difference of cum_x"):    # every concordant return 1e-2 higher: 1 / 60 of BOUNDS
        ec.check(changed(cum_x=(conc, lambda v: v + 1e-2)), "sim")
    with pytest.raises(AssertionError, match="envs differ in a decision"):
        ec.check(changed(decisions=(conc[:220], None)), "sim")
    with pytest.raises(AssertionError, match="differing period slots"):
        p = changed()
        p[F32]["decisions"][1:60, conc[:100]] ^= 1     # every env flies more than 60 periods
        ec.check(p, "sim")
    lost = conc[contact64[conc]][:40]                      # 1 % of the pairs lose their touchdown in float32: they part, and not in balance
    with pytest.raises(AssertionError, match="landing outcome in float32 only 0 times, in float64 only 45 times"):
        ec.check(changed(decisions=(lost, None), code=(lost, rc.MIN_ALT)), "sim")
    with pytest.raises(AssertionError, match="mean paired difference of steps"):
        ec.check(changed(steps=(disc, lambda v: v + 2)), "sim")
    with pytest.raises(AssertionError, match="mean paired difference of cum_x"):
        ec.check(changed(cum_x=(disc, lambda v: v - 5.0)), "sim")   # (their own sd is 5)


def test_the_decision_matrix_leaves_the_present_callers_result_alone(tables):
    """stepwise_first_episodes(decisions=True) returns what it returns without, plus the matrix: a word per period flown, the terminal's included, -1 after"""
    cfg = ec.FLAVOURS["sim"][0](F32)
    plain = rc.stepwise_first_episodes(_make(cfg, 256, 5), tables, 300)
    with_words = rc.stepwise_first_episodes(_make(cfg, 256, 5), tables, 300, decisions=True)
    assert set(with_words) == set(plain) | {"decisions"} and plain["trace"] is None
    rc.assert_rows_equal(with_words, plain, "with and without the decision matrix")
    w = with_words["decisions"]
    assert w.shape == (301, 256) and w.dtype == np.int32
    flown = (w >= 0).sum(axis=0)
    done = plain["code"] >= 0
    assert done.sum() >= 200 and np.array_equal(flown[done], plain["steps"][done] + 1) and (flown[~done] == 301).all()
    assert all((w[:k, i] >= 0).all() and (w[k:, i] == -1).all() for i, k in enumerate(flown))
    assert np.array_equal(rc.pack_decision(np.array([944]), np.array([-1]), np.array([2])), [(944 << 12) | (0x3FF << 2) | 2])
