"""The table fold and the int64 accumulators on the CPU (no GPU).

* The oracle's `_contract` (the mean-target fold) against an exact reference that shares none of its steps: a plain
  product of one factor per visit in high-precision fixed point, no batching, no powers by squaring (tests/fold_reference.py, which
  also derives the rounding bound asserted here).  The same inputs go through the HIP kernel in tests/test_gpu_instances_fullsize.py.
* The accumulators' headroom: the largest |TD target| derived from the reward constants and gamma, and every configuration the library
  accepts keeps a cell's sum of targets inside int64; the ones that could not are refused on the host."""
from fractions import Fraction

import numpy as np
import pytest

import fold_reference as fr
from dql_multirotor_landing_amd.config import DqlConfig, F32, N_CELLS, TARGET_FRAC_BITS

SCHEDULES = [(0, 1), (1, 1), (1, 4), (1, 16), (1, 1000)]  # (fold_per_step, launches the accumulators cover)


def _oracle_fold(cfg, qa, qb, cnt, acc, n_launch):
    from oracle.oracle import Oracle
    o = Oracle(cfg, 1)
    qa, qb, cnt, acc = qa.copy(), qb.copy(), cnt.copy(), acc.copy()
    o._contract(qa, qb, cnt, acc, n_launch)
    assert not acc.any(), "the fold clears the accumulators it folded"
    return qa, qb, cnt


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("per_step,n_launch", SCHEDULES)
def test_oracle_fold_within_exact_bound(per_step, n_launch, with_b):
    """m = 1, runs that end at / one past the table end, counts past it, 10^3 .. 10^9 visits, per_step with m below and above n_launch,
    negative / zero / large targets, Tsum near +-2^62; with_b: table b's visits take the learning rates after table a's."""
    cfg = DqlConfig(dtype=F32, fold_per_step=per_step)
    tab = cfg.alpha_table()
    cases = fr.fold_cases(len(tab))
    qa, qb, cnt, acc = fr.fold_inputs(cases, with_b)
    oa, ob, oc = _oracle_fold(cfg, qa, qb, cnt, acc, n_launch)
    fr.check_against_exact(cases, qa, qb, cnt, acc, oa, ob, oc, per_step, n_launch, tab, cfg.alpha_min, f"oracle per_step={per_step} n_launch={n_launch}")
    untouched = np.arange(len(cases), N_CELLS)
    assert np.array_equal(oa[untouched], qa[untouched]) and np.array_equal(oc[untouched], cnt[untouched])


def test_fold_of_one_visit_is_the_reference_update():
    """m = 1: the fold is the reference's Q += alpha(c) (t - Q) (pkg/double_q_learning.py:131-146); both forms within their rounding
    bounds of the exact value (the reference form: fl(Q + fl(alpha fl(t - Q))), u |E| + 3 u |alpha (t - Q)|)."""
    cfg = DqlConfig(dtype=F32)
    tab = cfg.alpha_table()
    cases = [c for c in fr.fold_cases(len(tab)) if c[4] == 1]
    qa, qb, cnt, acc = fr.fold_inputs(cases)
    oa, _, _ = _oracle_fold(cfg, qa, qb, cnt, acc, 1)
    for i, (name, q, c, ts, m) in enumerate(cases):
        a = tab[c] if c < len(tab) else cfg.alpha_min
        t = ts / float(1 << TARGET_FRAC_BITS)
        ref = q + a * (t - q)
        E, B = fr.exact_fold(q, c, ts, 1, 0, 1, tab, cfg.alpha_min)
        assert E == Fraction(q) + Fraction(a) * (Fraction(ts, 1 << TARGET_FRAC_BITS) - Fraction(q))
        b_ref = fr.U * abs(E) + 3 * fr.U * abs(Fraction(a) * (Fraction(t) - Fraction(q)))
        assert abs(Fraction(ref) - E) <= b_ref, name
        assert abs(Fraction(float(oa[i])) - Fraction(ref)) <= B + b_ref, f"{name}: fold {oa[i]!r} vs reference update {ref!r}"


# ---- int64 headroom of the accumulators ----

def _reward_bound(cfg):
    """|reward| per axis and step from pkg/mdp.py:441-541, level by level (see DqlConfig.max_abs_td_target for the terms)"""
    dt = 1.0 / cfg.f_ag
    out = []
    for k in range(5):
        rp = abs(cfg.w_p) * cfg.lim_v[k] * dt
        rv = abs(cfg.w_v) * cfg.lim_a[k] * dt
        rd = abs(cfg.w_dur) * cfg.lim_v[k] * dt
        r_max = rp + rv + abs(cfg.w_theta) * cfg.delta_theta / cfg.theta_max * cfg.lim_v[k] + rd
        r_theta = abs(cfg.w_theta) * abs(cfg.w_theta) / cfg.theta_max * cfg.lim_v[k]  # |pitch set point| <= theta_max (action clamp)
        out.append(rp + rv + r_theta + rd + max(abs(cfg.w_succ), abs(cfg.w_fail)) * r_max)
    return max(out)


def test_largest_td_target_from_the_reward_constants():
    """R bounds every reward (checked on an oracle run in both axis modes and on the reference's stage-4 tables), Q* = R / (1 - gamma)
    bounds every cell that starts inside it and so every TD target; the library's bound is at least this."""
    from pathlib import Path
    from oracle.oracle import Oracle
    for two_axis in (0, 1):
        cfg = DqlConfig(dtype=F32, two_axis=two_axis, t_max=4.0)
        R = _reward_bound(cfg)
        q_star = R / (1.0 - cfg.gamma)
        assert cfg.max_abs_td_target() >= q_star
        o = Oracle(cfg, 512, seed=5, n_threads=4)
        names = o.field_names()
        worst = 0.0
        for _ in range(60):
            o.train_steps(4, 1.0)
            r, _ = o.get_fields()
            worst = max(worst, float(np.abs(r[names.index("reward")]).max()))
        assert 0.0 < worst <= (2 if two_axis else 1) * R, (worst, R)
        assert np.abs(o.qa).max() <= q_star
    g = Path(__file__).parent / "golden" / "assets"
    for f in ("Q_table_a.npy", "Q_table_b.npy"):
        assert np.abs(np.load(g / f)).max() <= DqlConfig().max_abs_td_target()


def _sum_fits(cfg, visits):
    """the worst sum of `visits` targets of the derived bound (each rounded to fixed point) stays below 2^63"""
    q_star = Fraction(_reward_bound(cfg)) / (1 - Fraction(cfg.gamma))
    per_target = -(-q_star.numerator * (1 << TARGET_FRAC_BITS) // q_star.denominator) + 1
    return visits * per_target < (1 << 63)


class _StubEngine:
    """what the window schedule and the launch option read of an Engine, without a device"""
    def __init__(self, cfg, n):
        self.cfg, self.n = cfg, n
    def set_windowed(self, on):
        pass


def _engine_check(stub, P):
    """Engine.set_option("periods_per_launch", P) up to the library call: raises ValueError when the host refuses P"""
    from dql_multirotor_landing_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.cfg, e.n, e.lib, e._h = stub.cfg, stub.n, None, None
    with pytest.raises(AttributeError):  # passed the check, reached the (absent) library
        e.set_option("periods_per_launch", P)


@pytest.mark.parametrize("two_axis", [0, 1])
def test_every_accepted_configuration_fits_int64(two_axis):
    """envs per context up to dql_create's 2^31, periods_per_launch 1 .. 32, sync_period up to 2^31 - 1, ranks 1 .. 8: whatever the host
    accepts keeps a cell's launch accumulator (envs x P x axes targets) and window (ranks x envs x sync_period x axes) below 2^63."""
    from dql_multirotor_landing_amd import dist
    cfg = DqlConfig(dtype=F32, two_axis=two_axis)
    axes = 2 if two_axis else 1
    refused = accepted = 0
    for n in (1, 4096, 131072, 1 << 20, 1 << 22, 26 * 10 ** 6, 1 << 31):
        for P in (1, 2, 16, 32):
            try:
                _engine_check(_StubEngine(cfg, n), P)
                ok = True
            except ValueError as e:
                assert "accum_visit_limit" in str(e) and str(cfg.accum_visit_limit()) in str(e)
                ok = False
            assert ok == _sum_fits(cfg, n * P * axes), (n, P)
            refused += not ok; accepted += ok
        for k in (1, 2, 16, 1024, 1 << 20, (1 << 31) - 1):
            for world in (1, 2, 8):
                class Red:
                    pass
                red = Red(); red.world = world
                try:
                    dist.ShardedRunner(_StubEngine(cfg, n), red, sync_period=k)
                    ok = True
                except ValueError as e:
                    assert "accum_visit_limit" in str(e)
                    ok = False
                assert ok == _sum_fits(cfg, world * n * k * axes), (n, k, world)
                refused += not ok; accepted += ok
    assert refused and accepted


def test_unbounded_sync_period_is_refused():
    """the schedule the r5 curriculum flies is accepted; a sync period whose window could wrap a cell's int64 sum is refused by name"""
    from dql_multirotor_landing_amd import dist
    from dql_multirotor_landing_amd.dist import LocalWindowReducer
    cfg = DqlConfig(dtype=F32)
    dist.ShardedRunner(_StubEngine(cfg, 32768), LocalWindowReducer(None), sync_period=16)
    with pytest.raises(ValueError, match="accum_visit_limit"):
        dist.ShardedRunner(_StubEngine(cfg, 32768), LocalWindowReducer(None), sync_period=1 << 20)
    with pytest.raises(ValueError, match="sync_period"):
        dist.window_headroom(_StubEngine(DqlConfig(dtype=F32, two_axis=1), 1 << 20), 2 ** 31 - 1, 8)
