"""The elementary functions and random draws at the top of csrc/dql_device.hpp — det_sincos, det_atan2, det_log, box_muller (u24 / u24p / sqrt_) and
philox4x32 — on inputs of the test's choosing, for two backends: the CPU oracle's restatement (tests/test_det_math.py) and the HIP library through
dql_diag_det_math_run / dql_diag_box_muller_run / dql_diag_philox_run (tests/test_gpu_det_math.py, -m gpu).

On the HIP backend every call first asserts device == oracle BIT FOR BIT on all of its inputs (HipBackend below), then the check holds the device's own output
to an independent reference, so that no assertion rests on the oracle alone: numpy float64 for float32 results, np.longdouble (x87, eps 1.1e-19) for float64
results, a numpy Philox written from the Random123 definition.  Every bound is a priori: the function's stated accuracy (what tests/test_oracle_golden.py's
test_det_math_accuracy asserted before it moved here, bounds unchanged) or a rounding analysis written next to the constant.  Each check returns the maxima
it measured; tools/det_math_exhaustive.py writes them to profiles/det_math_exhaustive.jsonl.

Inputs move in chunks of 2^21 elements (<= 100 MB per call).
"""
from __future__ import annotations

import numpy as np
import pytest

F32, F64 = 0, 1
DTYPES = (F32, F64)
DTYPE_NAME = {F32: "float32", F64: "float64"}
CHUNK = 1 << 21
N24 = 1 << 24
TWO_PI = 6.28318530717958623200e+00  # the literal box_muller multiplies u24 by, rounded to the dtype

# ---- the bounds (index: dtype) ----
SINCOS_ATOL = (2e-7, 3e-16)   # test_det_math_accuracy's, against the function of the same-dtype argument
ATAN2_ATOL = (5e-7, 5e-16)    # test_det_math_accuracy's
LOG_RTOL = (2e-7, 4e-16)      # test_det_math_accuracy's rtol, with atol 0 on the function's own domain (0, 1]
# radius sqrt(-2 log u): half the log's relative bound (the root halves a relative error) + one rounding of the product -2 * log (exact: a power of two, kept
# as a term all the same) + one of the correctly rounded root, eps = 2^-24 / 2^-53 each: 1e-7 + 2 * 6e-8 = 2.2e-7 -> 2.5e-7; 2e-16 + 2 * 1.11e-16 = 4.2e-16 -> 4.5e-16
RADIUS_RTOL = (2.5e-7, 4.5e-16)
RADIUS_MAX = 5.7682           # sqrt(-2 log 2^-24) = 5.768108
# n0 = r cos, n1 = r sin against the IDEAL angle 2 pi k / 2^24, in units of r: the function's 2e-7 / 3e-16, half an ulp of an angle below 2 pi (2.4e-7 / 4.4e-16),
# the rounding of the literal 2 pi (1.8e-7 / 2.5e-16), and the rounding of the product r * cos (what is left: 3e-8 / 1.1e-16): 6.5e-7, 1.15e-15
ANGLE_ATOL = (6.5e-7, 1.15e-15)
# |n0^2 + n1^2 - r^2| / r^2 = |c^2 + s^2 - 1| <= 2 (|c| + |s|) d <= 2 sqrt(2) d, d = function error + product rounding: 2.83 * 2.6e-7 = 7.4e-7 -> 1e-6;
# 2.83 * 4.1e-16 = 1.16e-15 -> 1.5e-15
NORM_TOL = (1e-6, 1.5e-15)
# mean of cos / sin over a regular grid of the whole circle (ideal: 0).  The systematic term is the literal 2 pi's relative rounding error e (float32 +2.8e-8,
# float64 -3.9e-17): cos(t (1 + e)) = cos t - e t sin t, and the mean of -t sin t over [0, 2 pi) is +1, so mean cos shifts by e; the roundings are zero-mean
# and average out over 2^20 .. 2^24 points.  1e-7 (3.6 e) and, with the same factor, 1.5e-16
MEAN_TRIG_TOL = (1e-7, 1.5e-16)
# mean radius^2 against mean(-2 log u) on the same words: <= 2 RADIUS_RTOL mean(r^2), mean(r^2) = 2: 1e-6, 1.8e-15 -> 2e-15
MEAN_R2_TOL = (1e-6, 2e-15)


def hp_type(dtype):
    """the reference precision for results of `dtype`; float64 results need an extended long double"""
    if dtype == F32:
        return np.float64
    if not np.finfo(np.longdouble).eps < 2e-19:
        pytest.skip("np.longdouble is no wider than float64 here: no independent reference for the float64 functions")
    return np.longdouble


def to_dtype(x, dtype):
    """the values the function sees: float64 inputs rounded to `dtype`, held as float64"""
    x = np.asarray(x, dtype=np.float64)
    return x.astype(np.float32).astype(np.float64) if dtype == F32 else x


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want, what, *inputs):
    bad = np.flatnonzero(bits(got) != bits(want))
    if bad.size:
        i = bad[:5]
        raise AssertionError(f"{what}: {bad.size} of {len(got)} differ bit for bit; first at {i.tolist()}: inputs {[np.asarray(a)[i].tolist() for a in inputs]}, "
                             f"got {np.asarray(got)[i].tolist()}, want {np.asarray(want)[i].tolist()}")


# ---- backends ----
class OracleBackend:
    """oracle/oracle.py's det_math / box_muller / philox_n"""
    name = "oracle"

    def __init__(self):
        from oracle import oracle as orc
        self.o = orc
        self.philox_forms = {"oracle": lambda ctr, k0, k1: orc.philox_n(ctr, (k0, k1))}

    def det_math(self, x, y, dtype):
        return self.o.det_math(x, y, dtype=dtype)

    def box_muller(self, ra, rb, dtype):
        return self.o.box_muller(ra, rb, dtype=dtype)


class HipBackend:
    """the library's diagnostic operators (dql_multirotor_landing_amd/ops.py); every call is held to the oracle bit for bit before its result is used"""
    name = "hip"

    def __init__(self):
        from dql_multirotor_landing_amd import ops
        from oracle import oracle as orc
        self.ops, self.o = ops, orc
        self.philox_forms = {"oracle": lambda ctr, k0, k1: orc.philox_n(ctr, (k0, k1)),
                             "device, inline key schedule": lambda ctr, k0, k1: ops.philox_run(ctr, k0, k1, round_keys=0),
                             "device, round keys in registers": lambda ctr, k0, k1: ops.philox_run(ctr, k0, k1, round_keys=1)}

    def det_math(self, x, y, dtype):
        out = self.ops.det_math_run(x, y, dtype)
        for name, d, o in zip(("sin", "cos", "atan2", "log"), out, self.o.det_math(x, y, dtype=dtype)):
            assert_same_bits(d, o, f"{name} in {DTYPE_NAME[dtype]}, device vs oracle", x, y)
        return out

    def box_muller(self, ra, rb, dtype):
        out = self.ops.box_muller_run(ra, rb, dtype)
        for name, d, o in zip(("n0", "n1"), out, self.o.box_muller(ra, rb, dtype=dtype)):
            assert_same_bits(d, o, f"box_muller {name} in {DTYPE_NAME[dtype]}, device vs oracle", ra, rb)
        return out


def _chunks(n):
    return [(a, min(a + CHUNK, n)) for a in range(0, n, CHUNK)]


def _hold(figs, name, value, bound):
    """record a measured maximum and assert it against its bound (printed first, so a failing run still shows the figure)"""
    figs[name] = float(value)
    figs[name + "_bound"] = bound
    print(f"  {name} = {float(value):.4g} (bound {bound:g})")
    assert value <= bound, f"{name} = {float(value):.6g} exceeds {bound:g}"


def grid_words(dtype, rng, edges=()):
    """the 24-bit values k a check runs: all 2^24 in float32 (in chunks), 2^20 sampled ones plus the edges in float64"""
    if dtype == F32:
        return [np.arange(a, b, dtype=np.int64) for a, b in _chunks(N24)]
    k = np.unique(np.concatenate([rng.integers(0, N24, (1 << 20) - len(edges)), np.asarray(edges, dtype=np.int64)]))
    return [k]


def angle_of_words(k, dtype):
    """box_muller's angle of the word k << 8, in the dtype's arithmetic: T(2 pi) * ((T)k * 2^-24)"""
    if dtype == F32:
        return (np.float32(TWO_PI) * (k.astype(np.float32) * np.float32(2.0 ** -24))).astype(np.float64)
    return np.float64(TWO_PI) * (k.astype(np.float64) * 2.0 ** -24)


# ---- sin / cos ----
def check_sincos(be, dtype):
    hp, atol, rng = hp_type(dtype), SINCOS_ATOL[dtype], np.random.default_rng(11)
    figs = {}

    def err(x):
        s, c, _, _ = be.det_math(x, np.ones_like(x), dtype)
        xh = x.astype(hp)
        return float(np.max(np.abs(s.astype(hp) - np.sin(xh)))), float(np.max(np.abs(c.astype(hp) - np.cos(xh))))

    es = ec = 0.0
    for k in grid_words(dtype, rng, edges=(0, 1, N24 - 1)):
        a, b = err(angle_of_words(k, dtype))
        es, ec = max(es, a), max(ec, b)
    _hold(figs, "sin_grid_2pi_u24", es, atol); _hold(figs, "cos_grid_2pi_u24", ec, atol)
    special = np.array([0.0, 1e-9, np.pi / 2, np.pi, 2 * np.pi])
    es, ec = err(to_dtype(np.concatenate([np.linspace(-0.6, 0.6, 4097), special, -special]), dtype))
    _hold(figs, "sin_setpoint_range", es, atol); _hold(figs, "cos_setpoint_range", ec, atol)
    es, ec = err(to_dtype(rng.uniform(-50, 50, 8192), dtype))  # the platform's phase step: the one argument not bounded by 2 pi
    _hold(figs, "sin_abs_le_50", es, atol); _hold(figs, "cos_abs_le_50", ec, atol)
    return figs


# ---- log ----
def check_log(be, dtype):
    """on u24p's own values k 2^-24, k = 1 .. 2^24: relative error with atol 0, never positive, never non-finite, 0 only at u = 1"""
    hp, rng = hp_type(dtype), np.random.default_rng(12)
    figs, worst = {}, 0.0
    for k in grid_words(dtype, rng, edges=(0, 1, 2, N24 - 2, N24 - 1)):
        u = (k + 1).astype(np.float64) * 2.0 ** -24  # exact in either dtype
        lg = be.det_math(u, np.ones_like(u), dtype)[3]
        assert np.all(np.isfinite(lg)), f"non-finite log at u = {u[~np.isfinite(lg)][:5]}"
        assert not np.any(lg > 0), f"positive log at u = {u[lg > 0][:5]}"
        assert np.array_equal(lg == 0, u == 1.0), f"log is 0 at u = {u[(lg == 0) != (u == 1.0)][:5]}"
        ref = np.log(u.astype(hp))
        m = ref != 0
        worst = max(worst, float(np.max(np.abs(lg[m].astype(hp) - ref[m]) / np.abs(ref[m]))))
    _hold(figs, "log_u24p_rel", worst, LOG_RTOL[dtype])
    return figs


# ---- atan2 ----
def check_atan2_pairs(be, dtype):
    hp, rng = hp_type(dtype), np.random.default_rng(13)
    y, x = to_dtype(rng.standard_normal(1 << 20), dtype), to_dtype(rng.standard_normal(1 << 20), dtype)
    a = be.det_math(x, y, dtype)[2]
    figs = {}
    _hold(figs, "atan2_normal_pairs", np.max(np.abs(a.astype(hp) - np.arctan2(y.astype(hp), x.astype(hp)))), ATAN2_ATOL[dtype])
    return figs


WAVE_FAILING = (0, 1, 2, 32, 63, 64)
ATAN_BOUNDS = (0.4375, 0.6875, 1.1875, 2.4375)  # det_atan's range bounds; the first is the float32 fast path's too


def atan2_wave_kinds(dtype):
    """name -> [(y, x)]: the lanes that fail the float32 fast-path predicate `x > 0 && |y / x| < 0.4375` (the 1e-30 and y = -0 kinds pass it: they sit in
    the same slots so that the degenerate quotients meet both paths as well)"""
    t = np.float32 if dtype == F32 else np.float64
    kinds = {"x<0": [(0.3, -1.0), (-0.3, -1.0), (2.0, -0.5), (-1e-3, -3.0), (0.0, -1.0), (-0.0, -2.0)],
             "x=+0": [(1.0, 0.0), (-2.5, 0.0), (0.0, 0.0), (-0.0, 0.0)],
             "x=-0": [(1.0, -0.0), (-2.5, -0.0), (0.0, -0.0), (-0.0, -0.0)]}
    for b in ATAN_BOUNDS:  # x a power of two: the quotient is y / x exactly
        vs = [float(np.nextafter(t(b), t(0))), b, float(np.nextafter(t(b), t(4)))]
        kinds[f"|y/x|={b}"] = [(sg * v * x, x) for x in (1.0, 4.0) for v in vs for sg in (1.0, -1.0)]
    # just above the fast path's bound, where a wave that took the straight-line polynomial would leave det_atan's first reduced range unreduced
    q = np.random.default_rng(18).uniform(0.4375, 0.5, 64)
    kinds["0.4375<=|y/x|<0.5"] = [(float(sg * v * x), x) for v, sg, x in zip(q, np.tile((1.0, -1.0), 32), np.tile((1.0, 1.0, 2.0, 0.5), 16))]
    # (x stays inside det_sincos's domain: the operator evaluates sin and cos of it too, and device == oracle is asserted on every output)
    kinds["|y/x|=1e-30"] = [(1e-30, 1.0), (-1e-30, 1.0), (3e-29, 30.0)]
    kinds["|y/x|=1e30"] = [(1e30, 1.0), (-1e30, 1.0), (1.0, 1e-30)]
    kinds["y=-0,x>0"] = [(-0.0, 1.0), (-0.0, 3.5)]
    return kinds


def check_atan2_waves(be, dtype):
    """Constructed waves of 64 (dql_diag_det_math_run: elements 64 w .. 64 w + 63 share wave w): for every kind of lane that fails the float32 fast-path
    predicate and k in WAVE_FAILING, k such lanes first and 64 - k passing lanes after them, and again with the failing lanes last.  Asserted: x == 0 gives
    exactly +0 for y = +-0 and +-pi/2 otherwise — the function deliberately does NOT return pi for (+0, -0) as atan2 does —; a zero y gives +0 in front of the
    axis and +pi behind it (the sign of a zero y is not read); every other lane is within ATAN2_ATOL of numpy; and a lane's result does not depend on the wave
    it sits in (the fast path is "bit-identical by construction")."""
    hp, rng = hp_type(dtype), np.random.default_rng(14)
    t = np.float32 if dtype == F32 else np.float64
    # the passing lanes: the same 64 (y, x) in every wave, lane l always the pair l
    px = to_dtype(rng.uniform(0.5, 4.0, 64), dtype)
    py = to_dtype(rng.uniform(-0.43, 0.43, 64) * px, dtype)
    py[:3] = (0.0, 1e-20, -1e-20)
    assert np.all(px > 0) and np.all(np.abs(py.astype(t) / px.astype(t)) < t(0.4375))
    ys, xs, passing = [], [], []
    for variants in atan2_wave_kinds(dtype).values():
        for k in WAVE_FAILING:
            for failing_last in (False, True):
                fail = np.arange(64) >= 64 - k if failing_last else np.arange(64) < k
                fy = np.array([variants[j % len(variants)][0] for j in range(64)]); fx = np.array([variants[j % len(variants)][1] for j in range(64)])
                ys.append(np.where(fail, fy, py)); xs.append(np.where(fail, fx, px)); passing.append(~fail)
    y, x, passing = to_dtype(np.concatenate(ys), dtype), to_dtype(np.concatenate(xs), dtype), np.concatenate(passing)
    a = be.det_math(x, y, dtype)[2]
    pi, pio2 = float(t(3.14159265358979311600e+00)), float(t(1.57079632679489655800e+00))
    zx, zy = x == 0, y == 0
    want = np.where(zy, 0.0, np.where(y > 0, pio2, -pio2))
    assert_same_bits(a[zx], want[zx], "x == 0: (0, +-pi/2) exactly, +0 for y = +-0", x[zx], y[zx])
    m = zy & ~zx
    assert_same_bits(a[m], np.where(x[m] > 0, 0.0, pi), "y == +-0: +0 in front of the axis, +pi behind it", x[m], y[m])
    m = ~zx
    figs = {}
    ref = np.arctan2(np.where(zy, 0.0, y)[m].astype(hp), x[m].astype(hp))  # (a zero y read as +0, as the function does)
    _hold(figs, "atan2_constructed_waves", np.max(np.abs(a[m].astype(hp) - ref)), ATAN2_ATOL[dtype])
    # one result per input pair, whichever wave and lane it ran in
    _, inv = np.unique(np.stack([bits(y), bits(x)], axis=1), axis=0, return_inverse=True)
    inv = inv.ravel()
    lo = np.full(inv.max() + 1, np.iinfo(np.uint64).max, dtype=np.uint64); hi = np.zeros(inv.max() + 1, dtype=np.uint64)
    np.minimum.at(lo, inv, bits(a)); np.maximum.at(hi, inv, bits(a))
    bad = np.flatnonzero((lo != hi)[inv])
    assert bad.size == 0, f"{bad.size} lanes depend on their wave; first (y, x) = {(y[bad[0]], x[bad[0]])}, wave {bad[0] // 64}, lane {bad[0] % 64}"
    figs["waves"] = len(a) // 64
    figs["passing_lanes"] = int(passing.sum())
    return figs


# ---- Box-Muller ----
def _low_bits(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint32)  # the low 8 bits of a word are not used: any value


def check_box_muller_radius(be, dtype):
    """every radius word with the angle word 0 (n0 = radius, n1 = 0 exactly): float32 all 2^24, float64 2^20 sampled"""
    hp, rng = hp_type(dtype), np.random.default_rng(15)
    figs, worst, biggest, smallest, sum_r2, sum_ref, count = {}, 0.0, 0.0, np.inf, hp(0), hp(0), 0
    for k in grid_words(dtype, rng, edges=(0, 1, 2, N24 - 2, N24 - 1)):
        ra = (k.astype(np.uint32) << np.uint32(8)) | _low_bits(rng, len(k))
        n0, n1 = be.box_muller(ra, _low_bits(rng, len(k)), dtype)
        assert np.all(np.isfinite(n0)), f"non-finite radius for ra >> 8 = {k[~np.isfinite(n0)][:5]}"
        assert np.all(n1 == 0), f"n1 != 0 at the angle 0 for ra >> 8 = {k[n1 != 0][:5]}"  # (-0 at u = 1: the radius is sqrt(-2 * 0) = -0)
        assert np.array_equal(n0 == 0, k == N24 - 1), f"radius 0 for ra >> 8 = {k[(n0 == 0) != (k == N24 - 1)][:5]}"
        m2l = -2 * np.log((k + 1).astype(hp) * hp(2.0 ** -24))
        ref = np.sqrt(m2l)
        m = ref != 0
        worst = max(worst, float(np.max(np.abs(n0[m].astype(hp) - ref[m]) / ref[m])))
        biggest, smallest = max(biggest, float(n0.max())), min(smallest, float(n0[n0 > 0].min()))
        sum_r2 += np.sum(n0.astype(hp) ** 2); sum_ref += np.sum(m2l); count += len(k)
    _hold(figs, "radius_rel", worst, RADIUS_RTOL[dtype])
    figs["radius_max"], figs["radius_min_positive"] = biggest, smallest
    assert biggest < RADIUS_MAX, biggest
    assert smallest ** 2 >= SQRT_IEEE_MIN, smallest  # the root's argument stays inside sqrt_(float)'s domain (check_sqrt_ieee)
    figs["mean_radius2"], figs["mean_minus_2_log_u"] = float(sum_r2 / count), float(sum_ref / count)
    _hold(figs, "mean_radius2_vs_ideal", abs(sum_r2 - sum_ref) / count, MEAN_R2_TOL[dtype])
    return figs


def unit_radius_word():
    """the radius word whose u is the grid's nearest to e^(-1/2): radius about 1"""
    return np.uint32((int(round(np.exp(-0.5) * N24)) - 1) << 8)


def check_box_muller_angle(be, dtype):
    """every angle word under a radius of about 1: float32 all 2^24, float64 the regular sub-grid 16 j + 5 (a regular grid of the whole circle has the ideal
    means 0).  n0, n1 against r cos / r sin of the IDEAL angle 2 pi k / 2^24, n0^2 + n1^2 against r^2, the means of cos and sin."""
    hp = hp_type(dtype)
    ra1 = unit_radius_word()
    r = hp(be.box_muller(np.array([ra1]), np.zeros(1, np.uint32), dtype)[0][0])
    assert abs(float(r) - 1.0) < 1e-6, r
    two_pi = 8 * np.arctan(hp(1))
    words = [np.arange(a, b, dtype=np.int64) for a, b in _chunks(N24)] if dtype == F32 else [np.arange(5, N24, 16, dtype=np.int64)]
    figs, e_cos, e_sin, e_norm, s0, s1, count = {}, 0.0, 0.0, 0.0, hp(0), hp(0), 0
    for k in words:
        rb = k.astype(np.uint32) << np.uint32(8)
        n0, n1 = be.box_muller(np.full(len(k), ra1, np.uint32), rb, dtype)
        n0, n1 = n0.astype(hp), n1.astype(hp)
        th = two_pi * k.astype(hp) / N24
        e_cos = max(e_cos, float(np.max(np.abs(n0 - r * np.cos(th))) / r)); e_sin = max(e_sin, float(np.max(np.abs(n1 - r * np.sin(th))) / r))
        e_norm = max(e_norm, float(np.max(np.abs(n0 * n0 + n1 * n1 - r * r)) / (r * r)))
        s0 += np.sum(n0); s1 += np.sum(n1); count += len(k)
    _hold(figs, "n0_vs_ideal_angle", e_cos, ANGLE_ATOL[dtype]); _hold(figs, "n1_vs_ideal_angle", e_sin, ANGLE_ATOL[dtype])
    _hold(figs, "norm_n0_n1_vs_radius", e_norm, NORM_TOL[dtype])
    _hold(figs, "mean_cos", abs(s0 / count / r), MEAN_TRIG_TOL[dtype]); _hold(figs, "mean_sin", abs(s1 / count / r), MEAN_TRIG_TOL[dtype])
    return figs


def check_box_muller_pairs(be, dtype):
    """2^16 random word pairs: n0 and n1 are the dtype's products of the two factors — the radius (the pair's ra with the angle 0) and the cosine / sine of the
    pair's angle (det_sincos of T(2 pi) * u24(rb)) —, bit for bit"""
    rng = np.random.default_rng(16)
    ra = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint32); rb = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint32)
    n0, n1 = be.box_muller(ra, rb, dtype)
    rad = be.box_muller(ra, np.zeros_like(rb), dtype)[0]
    ang = angle_of_words((rb >> np.uint32(8)).astype(np.int64), dtype)
    s, c, _, _ = be.det_math(ang, np.ones_like(ang), dtype)
    t = np.float32 if dtype == F32 else np.float64
    assert_same_bits(n0, (rad.astype(t) * c.astype(t)).astype(np.float64), "n0 = radius * cos", ra, rb)
    assert_same_bits(n1, (rad.astype(t) * s.astype(t)).astype(np.float64), "n1 = radius * sin", ra, rb)
    assert np.all(np.isfinite(n0)) and np.all(np.isfinite(n1))
    return {"pairs": len(ra), "abs_max": float(max(np.abs(n0).max(), np.abs(n1).max()))}


# ---- sqrt_(float), the radius's square root (device only: the oracle's sqrtf is the definition) ----
SQRT_IEEE_MIN = 2.0 ** -102  # the floor of sqrt_(float)'s documented domain (csrc/dql_device.hpp), sqrt_pos's too
FLT_MAX = 3.4028234663852886e38


def check_sqrt_ieee(be):
    """dql_diag_selftest_sqrt_ieee: sqrt_(float) against (float)sqrt((double)x) on every float32 of its domain — 0 and [2^-102, FLT_MAX], 1.93e9 inputs.
    FINDING of the first exhaustive run over all positive normal inputs: 3 954 656 misround, every one below 2^-104 (biased exponents 1 .. 22, largest
    0x0b6e9372), where the residuals of the neighbour test go subnormal.  The comment that claimed correct rounding on every normal input now states the domain;
    the one float32 call site, Box-Muller's radius, takes 0 or [1.19e-7, 33.3] (check_box_muller_radius asserts it on all 2^24 words).  The count below the
    domain is recorded, not asserted."""
    figs = {"misrounded_at_0": be.ops.selftest_sqrt_ieee(0.0, 0.0), "misrounded_2^-102_to_FLT_MAX": be.ops.selftest_sqrt_ieee(SQRT_IEEE_MIN, FLT_MAX),
            "misrounded_normal_below_2^-102": be.ops.selftest_sqrt_ieee(2.0 ** -126, float(np.nextafter(np.float32(SQRT_IEEE_MIN), np.float32(0))))}
    print(" ", figs)
    assert figs["misrounded_at_0"] == 0 and figs["misrounded_2^-102_to_FLT_MAX"] == 0, figs
    return figs


# ---- Philox4x32-10 ----
def philox_numpy(ctr, key):
    """Philox4x32-10 from the Random123 definition (Salmon et al. 2011): ten rounds of two 32 x 32 -> 64 products, the key bumped by the Weyl constants between
    rounds.  ctr uint32 [n][4], key uint32 [n][2] -> uint32 [n][4]"""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = key[:, 0].astype(np.uint64), key[:, 1].astype(np.uint64)
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & m32, (p0 >> s32) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=1).astype(np.uint32)


# Random123's known-answer vectors (kat_vectors: philox4x32 10): counter, key, result
PHILOX_KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
PHILOX_STREAMS = (0, 1, 16, 17, 18, 19, 20, 0xffffffff)  # STREAM_ACTION (+ 1 for the y axis), STREAM_NOISE0 + manager tick 0 .. 4, STREAM_INIT


def philox_structured_counters():
    """(step_lo, step_hi, env_id, stream) as the kernels form them: step_hi != 0 (a step index of 2^32 or more), step_lo at its last value and the successor
    that carries into step_hi, the last env id, every stream constant"""
    steps = ((0, 0), (0xffffffff, 0), (0, 1), (5, 1), (0xfffffffe, 0xffffffff), (0xffffffff, 0xffffffff))
    envs = (0, 1, 12345, 0xffffffff)
    return np.array([(lo, hi, e, s) for lo, hi in steps for e in envs for s in PHILOX_STREAMS], dtype=np.uint32)


def check_philox(be):
    """every form the backend has (the oracle; on the device the inline key schedule and the round keys in registers) == the numpy implementation, word for word"""
    rng = np.random.default_rng(17)
    n = 0
    for name, form in be.philox_forms.items():
        def same(ctr, k0, k1, what):
            ctr = np.ascontiguousarray(ctr, dtype=np.uint32)
            want = philox_numpy(ctr, np.broadcast_to(np.array([k0, k1], dtype=np.uint32), (len(ctr), 2)))
            got = form(ctr, k0, k1)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"philox, {name}, {what}: {bad.size} of {len(ctr)} counters differ; first {ctr[bad[0]].tolist()} key {(hex(k0), hex(k1))}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}"
            return len(ctr)
        for ctr, key, res in PHILOX_KAT:
            np.testing.assert_array_equal(form(np.array([ctr], dtype=np.uint32), *key)[0], res, err_msg=f"{name}: Random123 vector")
            np.testing.assert_array_equal(philox_numpy(np.array([ctr], dtype=np.uint32), np.array([key], dtype=np.uint32))[0], res, err_msg="numpy reference: Random123 vector")
        keys = rng.integers(0, 1 << 32, (64, 2), dtype=np.uint32)   # 2^16 random (counter, key) pairs: 64 keys (a key is a launch constant) x 1 024 counters
        for k0, k1 in keys.tolist():
            n += same(rng.integers(0, 1 << 32, (1024, 4), dtype=np.uint32), k0, k1, "random pairs")
        for k0, k1 in ((0, 0), (42, 0), (0xdeadbeef, 0x12345678), (0xffffffff, 0xffffffff)):
            n += same(philox_structured_counters(), k0, k1, "structured counters")
    return {"forms": list(be.philox_forms), "counters_checked": n}


# ---- what tests/test_oracle_golden.py::test_det_math_accuracy asserted, unchanged ----
def check_legacy_points(be):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-7, 7, 4000), [0.0, 1e-9, np.pi / 2, np.pi, 2 * np.pi - 1e-12]])
    y = rng.uniform(-3, 3, len(x))
    s, c, a, lg = be.det_math(x, y, F64)
    np.testing.assert_allclose(s, np.sin(x), rtol=0, atol=3e-16)
    np.testing.assert_allclose(c, np.cos(x), rtol=0, atol=3e-16)
    np.testing.assert_allclose(a, np.arctan2(y, x), rtol=0, atol=5e-16)
    m = np.abs(x) > 1e-30
    np.testing.assert_allclose(lg[m], np.log(np.abs(x[m])), rtol=4e-16, atol=5e-16)
    s, c, a, lg = be.det_math(x, y, F32)
    x32 = x.astype(np.float32).astype(np.float64); y32 = y.astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(s, np.sin(x32), rtol=0, atol=2e-7)
    np.testing.assert_allclose(c, np.cos(x32), rtol=0, atol=2e-7)
    np.testing.assert_allclose(a, np.arctan2(y32, x32), rtol=0, atol=5e-7)
    m = np.abs(x32) > 1e-30
    np.testing.assert_allclose(lg[m], np.log(np.abs(x32[m])), rtol=2e-7, atol=1e-6)


# name -> (check, per dtype?): what the two test files parametrise over and tools/det_math_exhaustive.py records
CHECKS = {"sincos": check_sincos, "log": check_log, "atan2_pairs": check_atan2_pairs, "atan2_waves": check_atan2_waves,
          "box_muller_radius": check_box_muller_radius, "box_muller_angle": check_box_muller_angle, "box_muller_pairs": check_box_muller_pairs}
