"""The tick's control-side functions against the golden vectors the reference's OWN Python produced (G8 filters / PID, G9 attitude law,
G11 platform, G12 manager tick), for any backend that exposes the replay operators — the CPU oracle (tests/test_oracle_golden.py,
tests/test_f32_fixtures.py) and the HIP library through its C ABI (tests/test_gpu_operators.py) — and in BOTH dtypes:

* float64 spells the reference's expressions out operation by operation: bit-exact (or the fixture's own stand-in tolerance).
* float32 — the arithmetic every throughput figure runs on — takes the same formulas in shorter forms (transposed Butterworth, fused
  multiply-adds, x-axis attitude closed form, v_rsq + residual-correction root behind one med3 clamp, platform sine / cosine carried by rotation,
  Kalman fixed-point shortcut, lazy noise).  Each check below states the bound it asserts and where the bound comes from; eps = 2^-24
  (float32 half ulp relative).  The bounds are a priori (rounding analysis), the measured maxima are quoted next to them.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from dql_multirotor_landing_amd.config import DqlConfig, F32, F64, Q_REFERENCE, TRAJ_EIGHT

GOLDEN = Path(__file__).resolve().parent / "golden"
EPS = 2.0 ** -24


class OracleBackend:
    """oracle/oracle.py's replay operators behind the interface the checks use"""
    name = "oracle"

    def __init__(self):
        from oracle import oracle as orc
        self.o = orc

    def butterworth_run(self, cfg, x):
        return self.o.butterworth_run(x, c=cfg.bw_c, dtype=cfg.dtype)

    def kalman_run(self, cfg, vel, flags):
        return self.o.kalman_run(vel, flags, cfg.kalman_q, cfg.noise_vel_sd, dtype=cfg.dtype)

    def pid_run(self, cfg, params, state):
        return self.o.pid_run(params, state, bw_c=cfg.bw_c, dtype=cfg.dtype)

    def attitude_run(self, cfg, q, w, cmd, xonly=0):
        return self.o.attitude_rotors(cfg, q, w, cmd, xonly=xonly)

    def platform_run(self, cfg, n, carry=0):
        return self.o.platform_run(cfg, n, dtype=cfg.dtype, carry=carry)

    def manager_run(self, cfg, series, contact, seed=0):
        return self.o.manager_run(cfg, series, contact, seed=seed)

    def discretise(self, cfg, p, v, a, ang):
        return self.o.discretise(cfg, p, v, a, ang)

    def mdp_transition(self, cfg, action, obs, ms, prev_idx, simulation=False):
        # SimulationMdp.check is TrainingMdp.check without the goal branch: the library's DQL_MDP_SIMULATION stage feeds prev = -1 (csrc/dql_ops.inc), so does this
        prev = np.full(len(action), -1, dtype=np.int32) if simulation else prev_idx
        return self.o.mdp_transition(cfg, action, obs, ms, prev)


class HipBackend:
    """the product's stateless operators (dql_*_run through ctypes: dql_multirotor_landing_amd/ops.py)"""
    name = "hip"

    def __init__(self):
        from dql_multirotor_landing_amd import ops
        self.o = ops

    def butterworth_run(self, cfg, x):
        return self.o.butterworth_run(cfg, x)

    def kalman_run(self, cfg, vel, flags):
        return self.o.kalman_run(cfg, vel, flags)

    def pid_run(self, cfg, params, state):
        return self.o.pid_run(cfg, params, state)

    def attitude_run(self, cfg, q, w, cmd, xonly=0):
        return self.o.attitude_run(cfg, q, w, cmd, xonly=xonly)

    def platform_run(self, cfg, n, carry=0):
        return self.o.platform_run(cfg, n, carry=carry)

    def manager_run(self, cfg, series, contact, seed=0):
        return self.o.manager_run(cfg, np.asarray(series)[None], np.asarray(contact)[None], seed=seed)[0]

    def discretise(self, cfg, p, v, a, ang):
        return self.o.discretise(cfg, p, v, a, ang)

    def mdp_transition(self, cfg, action, obs, ms, prev_idx, simulation=False):
        return self.o.mdp_transition(cfg, action, obs, ms, prev_idx, stages=self.o.MDP_ALL | (self.o.MDP_SIMULATION if simulation else 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# G8: pkg/filters.py:98-109 (Butterworth), :19-80 (Kalman), pkg/pid.py:62-104 (PID.output)
# ---------------------------------------------------------------------------------------------------------------------------------
def check_g8_butterworth(be, dtype):
    g = np.load(GOLDEN / "g8_filters.npz")
    y = be.butterworth_run(DqlConfig(dtype=dtype), g["bw_in"])
    if dtype == F64:
        np.testing.assert_array_equal(y, g["bw_out"])
        return 0.0
    # float32, transposed direct form: per output 4 roundings of values <= 2 |x|max; the filter is a unit-DC-gain low-pass (poles inside
    # 0.42) so the rounding noise is not amplified: |err| <= 16 eps |x|max = 2.5e-6 for |x| <= 2.64.  Measured: 2.0e-7.
    bound = 16 * EPS * np.abs(g["bw_in"]).max()
    err = np.abs(y - g["bw_out"]).max()
    assert err <= bound, (err, bound)
    return err


def check_g8_kalman(be, dtype):
    g = np.load(GOLDEN / "g8_filters.npz")
    worst = 0.0
    for tag, sd in (("r0", 0.0), ("r01", 0.1)):
        vel = g[f"kf_vel_{tag}"]
        flags = np.array([(i % 17 == 0) for i in range(len(vel))], dtype=np.uint8)
        acc = be.kalman_run(DqlConfig(dtype=dtype, noise_vel_sd=sd, kalman_q=1e-4), vel, flags)
        ref = g[f"kf_acc_{tag}"]
        if dtype == F64:
            np.testing.assert_array_equal(acc, ref)
            continue
        # float32: z = dv / dt.  dv: two roundings of |v| <= 0.55 -> 2 eps 0.55 / 0.01 = 6.6e-6 absolute; dt = difference of two float32
        # time stamps <= 1.2 s -> 2 eps 1.2 / 0.01 = 1.4e-5 RELATIVE (the reference subtracts time stamps too, in float64); the filter
        # (gain <= 1) does not amplify.  Measured: 1.2e-4 at |acc| = 15.
        bound = 1e-5 + 2e-5 * np.abs(ref)
        assert (np.abs(acc - ref) <= bound).all(), (tag, np.abs(acc - ref).max())
        worst = max(worst, np.abs(acc - ref).max())
    return worst


def check_g8_pid(be, dtype):
    g = np.load(GOLDEN / "g8_filters.npz")
    worst = 0.0
    for tag in ("vz", "yaw"):  # the third fixture has Kd != 0: the reference launches both controllers with Kd = 0 and the kernel has no D term
        params, state = g[f"pid_{tag}_params"], g[f"pid_{tag}_state"]
        eff, integ = be.pid_run(DqlConfig(dtype=dtype), params, state)
        if dtype == F64:
            np.testing.assert_array_equal(integ, g[f"pid_{tag}_integral"])
            np.testing.assert_array_equal(eff, g[f"pid_{tag}_effort"])
            continue
        # float32: the integral is a running sum of e dt: one rounding (eps |I|, |I| <= windup) per tick, 400 ticks, and dt itself is a
        # difference of float32 time stamps (relative 2 eps 0.8 / 0.002 = 5e-5 of each increment |e| dt <= 0.01): <= 400 (eps 1 + 5e-7) = 2.3e-4
        # worst case; measured 2.0e-7.  Effort = Kp fe + Ki I: Kp (Butterworth bound) + Ki (integral bound) + 2 roundings.
        kp, ki, wind = params[0], params[1], params[5]
        scale_e = np.abs(params[6] - state).max()
        b_int = 400 * (EPS * min(wind, 400 * 0.002 * scale_e) + 5e-5 * 0.002 * scale_e)
        b_eff = kp * 16 * EPS * scale_e + ki * b_int + 4 * EPS * max(abs(params[3]), abs(params[4]))
        e_int = np.abs(integ - g[f"pid_{tag}_integral"]).max(); e_eff = np.abs(eff - g[f"pid_{tag}_effort"]).max()
        assert e_int <= b_int and e_eff <= b_eff, (tag, e_int, b_int, e_eff, b_eff)
        ref_eff = g[f"pid_{tag}_effort"]
        for lim in (params[3], params[4]):  # a saturated output is the limit itself — its float32 cast — bit for bit (med3 clamp)
            sat = ref_eff == lim
            assert (eff[sat] == float(np.float32(lim))).mean() > 0.98 if sat.any() else True
        worst = max(worst, e_int, e_eff)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# G9: pkg/attitude_controller.py:107-156 -> commanded rotor speeds
# ---------------------------------------------------------------------------------------------------------------------------------
def _g9():
    g = np.load(GOLDEN / "g9_attitude.npz")
    x, y, z, w = g["quat_xyzw"].T
    tilt = np.degrees(np.arccos(np.sqrt(np.clip((1 - 2 * (y * y + z * z)) ** 2 + (2 * (x * y + w * z)) ** 2, 0, 1))))
    return g, tilt


def _alloc_scale(cfg, thrust, moment):
    """size of the terms the inverse allocation adds up to a rotor's w^2 = ia T -+ ib M_xy +- ic M_z (attitude_controller.py:94-105, 148-156)"""
    ia, ib, ic = 1 / (4 * cfg.k_f), 1 / (2 * cfg.arm_length * cfg.k_f), 1 / (4 * cfg.k_f * cfg.k_m)
    return ia * np.abs(thrust) + ib * np.maximum(np.abs(moment[:, 0]), np.abs(moment[:, 1])) + ic * np.abs(moment[:, 2])


def check_g9_rotor_speeds(be, dtype):
    """The reference's rotor speeds sqrt(max(w^2, 0)) for 200 (attitude, body rate, command) samples, incl. the clamp at 0 (112 entries) —
    for float32 through the whole short form: quat_to_R by doubled components, Newton yaw frame, yaw-free attitude error, gains with the
    halving folded in, fused inverse allocation, med3 clamp, v_rsq + residual-correction square root."""
    g, tilt = _g9()
    cfg = DqlConfig(dtype=dtype)
    rot = be.attitude_run(cfg, g["quat_xyzw"], g["omega"], g["cmd"])
    ref = g["rotor"]
    if dtype == F64:
        np.testing.assert_allclose(rot, ref, rtol=1e-10, atol=1e-7)
        return 0.0
    # float32: compared as w^2 (what the law computes; the root of a small w^2 magnifies any error by 1 / (2 w)).  Every w^2 is a sum of
    # three terms of size S (_alloc_scale) carrying ~20 roundings each through R, E, e_R, M: <= 1e-6 S up to 55 deg of tilt (measured
    # 4.0e-7 S); beyond, the yaw frame's 1 / sqrt by three Newton steps from a second-order start is the larger term: 5e-5 S (measured
    # 1.5e-5 S at the fixture's 60 deg samples; the reference's envs fly within +-22 deg, mdp.py theta_max)
    S = _alloc_scale(cfg, g["cmd"][:, 3], g["moment"])
    err = np.abs(rot ** 2 - ref ** 2).max(axis=1) / S
    assert (tilt <= 55).sum() >= 190 and (tilt > 55).sum() >= 3
    assert err[tilt <= 55].max() <= 1e-6, err[tilt <= 55].max()
    assert err[tilt > 55].max() <= 5e-5, err[tilt > 55].max()
    # the clamp at zero: the reference commands exactly 0, the float32 form 1e-15 rad/s (sqrt of the med3 floor 1e-30: sqrt_pos's domain)
    z = ref == 0.0
    assert z.sum() > 100 and (rot[z] <= 1.0000001e-15).mean() > 0.97  # (a w^2 within rounding of 0 may land on the other side)
    assert rot.max() <= cfg.rotor_max
    return err.max()


def check_g9_xonly_form(be):
    """The x-axis kernels' closed form (roll command exactly 0) against the generic float32 form and against the reference-pinned float64
    law on the fixture's attitudes with the roll command zeroed: same law, 10 instructions shorter."""
    g, tilt = _g9()
    cmd = g["cmd"].copy(); cmd[:, 0] = 0.0
    c32, c64 = DqlConfig(dtype=F32), DqlConfig(dtype=F64)
    rx = be.attitude_run(c32, g["quat_xyzw"], g["omega"], cmd, xonly=1)
    rg = be.attitude_run(c32, g["quat_xyzw"], g["omega"], cmd, xonly=0)
    r64 = be.attitude_run(c64, g["quat_xyzw"], g["omega"], cmd)
    # scale from the float64 law's own moments: recover them from w^2 by the allocation matrix A (fixture "A") where no rotor is clamped
    w2 = r64 ** 2
    tm = w2 @ g["A"].T  # rows: roll, pitch, yaw moment, thrust (attitude_controller.py:94-105)
    S = _alloc_scale(c64, cmd[:, 3], np.abs(tm[:, :3])) + 1.0
    ok = tilt <= 55
    assert (np.abs(rx ** 2 - w2).max(axis=1) / S)[ok].max() <= 2e-6
    assert (np.abs(rx ** 2 - rg ** 2).max(axis=1) / S)[ok].max() <= 2e-6  # B01 = B10 = 0 and B11 = 1 exactly: only signed zeros and fusion differ


# ---------------------------------------------------------------------------------------------------------------------------------
# G11: pkg/moving_platform.py:87-127
# ---------------------------------------------------------------------------------------------------------------------------------
G11_CASES = (("rpm_launch", {}), ("rpm_default", dict(mp_t_x=1.0)), ("eight", dict(trajectory=TRAJ_EIGHT)))


def check_g11_platform(be, dtype, carry=0):
    g = np.load(GOLDEN / "g11_platform.npz")
    worst = 0.0
    for name, kw in G11_CASES:
        cfg = DqlConfig(dtype=dtype, **kw)
        out = be.platform_run(cfg, 3000, carry=carry)
        ref = g[name][:, 1:]
        if dtype == F64:
            np.testing.assert_allclose(out, ref, rtol=0, atol=2e-11)
            continue
        # float32: the phase is the state, advanced by fma(omega, dt, phase) and wrapped at 2 pi: one rounding of <= 2^-22 (half an ulp in
        # [4, 8)) per tick, and for a CONSTANT increment the roundings inside one binade share a sign, so the bound is linear in the tick
        # index: |d phase_i| <= (i + 1) 2^-22 + 2 eps 2 pi (wraps).  x = r sin: |dx| <= r |d phase| + 4 eps r (polynomial sine, product);
        # u = r omega cos likewise.  The carried variant (sine / cosine re-seeded every `carry` ticks and rotated in between) adds <= 4 eps
        # per rotation, at most `carry` - 1 of them in a row.  Measured after 30 s: 3.4e-4 m of a bound of 1.4e-3 (eight: 2.1e-3).
        r = 3.0 if kw.get("trajectory") == TRAJ_EIGHT else cfg.mp_r_x
        om = 0.8 / 3.0 if kw.get("trajectory") == TRAJ_EIGHT else cfg.mp_t_x / cfg.mp_r_x
        i = np.arange(3000) + 1.0
        dph = i * 2.0 ** -22 + 4 * EPS * np.pi + (4 * EPS * max(carry - 1, 0))
        bx = r * dph + 8 * EPS * r
        bound = np.stack([bx, 2 * bx, om * bx, 2 * om * bx], axis=1)  # eight: y = r sin cos, v = r omega cos 2 phase: twice the sensitivity
        err = np.abs(out - ref)
        assert (err <= bound).all(), (name, carry, (err / bound).max())
        if kw.get("trajectory") != TRAJ_EIGHT:
            assert (out[:, 1] == 0).all() and (out[:, 3] == 0).all()
        worst = max(worst, err.max())
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# G12: scripts/manager_node.py:192-214, 292-310 + pkg/observation_utils.py:77-158
# ---------------------------------------------------------------------------------------------------------------------------------
def g12_cfg(noise_sd, dtype, quirks=Q_REFERENCE):
    return DqlConfig(dtype=dtype, two_axis=1, noise_pos_sd=float(noise_sd[0]), noise_vel_sd=float(noise_sd[1]), quirks=quirks)


def check_g12_manager_f32(be):
    """The float32 manager tick against ManagerNode.publish_obs over the fixture's three 300-tick series (noise 0, yaw != 0, noise > 0 with
    the Kalman gain at R = sd_v^2).  Columns: obs p_x p_y v_x v_y a_x a_y, v_z plant state, yaw plant state, platform set-point x y u v."""
    z = np.load(GOLDEN / "g12_manager.npz")
    worst = {}
    for tag in ("a_noise0", "c_yaw", "b_noise"):
        got = be.manager_run(g12_cfg(z[f"{tag}_noise_sd"], F32), z[f"{tag}_in"], z[f"{tag}_contact"], seed=5)
        ref = z[f"{tag}_out"]
        inp = z[f"{tag}_in"]
        i = np.arange(len(ref), dtype=np.float64)
        if tag != "b_noise":  # with noise the published p / v carry this build's Philox draws instead of numpy's: compared in distribution (test_g12_noise_*)
            # p / v: differences and a 2x2 rotation of float32 casts of |p| <= 4.5 m, |v| <= 2 m/s: 6 roundings -> 6 eps 4.5 = 1.6e-6
            assert np.abs(got[:, :4] - ref[:, :4]).max() <= 1.6e-6, np.abs(got[:, :4] - ref[:, :4]).max()
        # acceleration under B19 (frozen reference sample): (v_i - v_0) / (0.01 i); v_i and v_0 are each a 2x2 rotation of a difference of
        # two float32 casts, 4 roundings of |v| <= 2 m/s -> 8 eps each, 16 eps / (0.01 i) together, and the float32 product i * 0.01 as the
        # divisor: 2 eps relative; the Kalman gain (<= 1) does not amplify.  Tick 0 publishes 0 exactly.
        assert (got[0, 4:6] == 0).all()
        b_in = 16 * EPS / (0.01 * np.maximum(i, 1.0)) + 4 * EPS * np.abs(ref[:, 4:6]).max(axis=1) + 1e-6
        # ... per tick INPUT of the filter; with R > 0 the estimate remembers earlier inputs: e_i <= (1 - K_i) e_(i-1) + K_i b_i with the
        # filter's own (data-independent) gains K_i (pkg/filters.py:19-36: P += Q; K = P / (P + R); P *= 1 - K)
        P, Q, Rm = 1.0, 1e-4, float(z[f"{tag}_noise_sd"][1]) ** 2
        b_acc = np.zeros(len(ref))
        for k in range(1, len(ref)):
            P += Q; K = 1.0 if Rm == 0.0 else P / (P + Rm); P *= 1 - K
            b_acc[k] = (1 - K) * b_acc[k - 1] + K * b_in[k]
        b_acc += 1e-6
        e_acc = np.abs(got[:, 4:6] - ref[:, 4:6]).max(axis=1)
        assert (e_acc <= b_acc).all(), (tag, (e_acc / b_acc).max())
        # PID plant states: v_z is a cast (eps |v_z|); yaw = atan2 of the yaw-only frame: fdlibm's float kernel, < 1e-6 rad
        assert np.abs(got[:, 6] - ref[:, 6]).max() <= 2 * EPS * np.abs(inp[:, 5]).max() + 1e-9
        assert np.abs(got[:, 7] - ref[:, 7]).max() <= 1e-6
        # the platform set-point published by the tick: G11's linear bound over 300 ticks
        bsp = 2.0 * ((i + 1) * 2.0 ** -22 + 4 * EPS * np.pi) + 16 * EPS
        assert (np.abs(got[:, 8] - ref[:, 8]) <= bsp).all() and (np.abs(got[:, 10] - ref[:, 10]) <= bsp).all()
        worst[tag] = (float(e_acc.max()), float(np.abs(got[:, 8] - ref[:, 8]).max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# G1 / G2 / G2s: pkg/mdp.py:149-170, 257-569 (TrainingMdp), :572-886 (SimulationMdp) — discretise, check, reward, continuous_action
# ---------------------------------------------------------------------------------------------------------------------------------
# float32 forms (csrc/dql_device.hpp): x / x_max is fl(fl(x) * fl(1 / x_max)) (norm_by), a goal edge is fl(lim[k] * fl(lim[k+1] / lim[k])) or
# fl(lim[k] * fl(beta)) from float32 casts of the limits, delta_theta / theta_max is a host quotient (dtheta_ratio).  A bin comparison v < edge can
# therefore fall the other way when v is within rounding of the edge.  How far, relative, in units of eps = 2^-24:
#   the input side:  cast of the input (1) + rounding of the reciprocal (1) + rounding of the product (1)                     = 3
#   the edge side:   the cast limits (lim[k] cancels in lim[k] * (lim[k+1] / lim[k]): 1) + the quotient (1) + the product (1)  = 3
#                    (lim * beta: two casts and a product, also 3; the angle grid: cast angle, cast grid points, two differences: < 3)
# 6 eps to first order; EDGE_ULPS = 8 leaves 2 eps for the second-order terms and for the float64 side's own roundings (2^-53: nothing).
EDGE_ULPS = 8
EDGE_REL = EDGE_ULPS * EPS


def unpack_state(idx):
    idx = np.asarray(idx)
    return np.stack([idx // 189, (idx // 63) % 3, (idx // 21) % 3, (idx // 7) % 3, idx % 7], axis=-1)


def pack_state(s):
    s = np.asarray(s).astype(np.int64)
    return ((((s[..., 0] * 3 + s[..., 1]) * 3 + s[..., 2]) * 3 + s[..., 3]) * 7 + s[..., 4]).astype(np.int32)


_ORACLE = []


def _oracle():
    """the float64 oracle: pinned bit for bit to G1 / G2 by tests/test_oracle_golden.py, so what it says about a perturbed input is what the reference says"""
    if not _ORACLE:
        _ORACLE.append(OracleBackend())
    return _ORACLE[0]


def edge_neighbours(cfg64, p, v, a, ang):
    """float64 packed indices [8][n] of every input with ONE of its four arguments scaled by 1 +- EDGE_REL"""
    args = [np.asarray(x, dtype=np.float64) for x in (p, v, a, ang)]
    out = []
    for j in range(4):
        for s in (1.0 - EDGE_REL, 1.0 + EDGE_REL):
            q = list(args); q[j] = args[j] * s
            out.append(_oracle().discretise(cfg64, *q))
    return np.stack(out)


def _index_rules(idx32, golden_idx, nb, what):
    """the three index assertions shared by G1 / G2 / G2s; returns the edge-near mask"""
    near = (nb != golden_idx[None, :]).any(axis=0)
    bad = ~near & (idx32 != golden_idx)
    assert not bad.any(), f"{what}: {bad.sum()} inputs that are NOT within {EDGE_ULPS} eps of a bin edge differ from the golden state, first {np.flatnonzero(bad)[:5]}"
    ok = (idx32 == golden_idx) | (idx32[None, :] == nb).any(axis=0)
    assert ok.all(), f"{what}: {(~ok).sum()} edge-near inputs have neither the golden state nor a perturbed neighbour's, first {np.flatnonzero(~ok)[:5]}"
    assert not ((idx32 < 0) & (golden_idx >= 0)).any(), f"{what}: float32 refuses an input float64 classifies"
    return near


def check_g1_discretise(be, dtype, level):
    """TrainingMdp.discrete_state over the whole G1 fixture (1 500 random inputs, 500 near the origin, then the edge cases placed on / within 1e-12
    of every bin edge).  float64: bit for bit.  float32: exact wherever the input is not edge-near; an edge-near input (its float64 class changes
    when one argument is scaled by 1 +- 8 eps, derivation above) may take a neighbour's class.  Returns (differing, edge-near) counts.
    Measured on the float32 oracle, levels 0-4: 7-43 inputs differ, all of them edge-near; edge-near 1.5 % (level 0) to 6.6 % (level 4)."""
    g = np.load(GOLDEN / "g1_discretise.npz")
    x = g[f"in_{level}"]
    golden = pack_state(g[f"state_{level}"])
    idx = be.discretise(DqlConfig(working_curriculum_step=level, dtype=dtype), x[:, 0], x[:, 1], x[:, 2], x[:, 3])
    if dtype == F64:
        assert (idx >= 0).all()
        np.testing.assert_array_equal(unpack_state(idx), g[f"state_{level}"])
        return 0, 0
    nb = edge_neighbours(DqlConfig(working_curriculum_step=level, dtype=F64), x[:, 0], x[:, 1], x[:, 2], x[:, 3])
    near = _index_rules(idx, golden, nb, f"G1 level {level}")
    assert not near[:1500].any(), f"{near[:1500].sum()} of the 1 500 random inputs are edge-near: the allowance would hide a wrong form"
    assert near.mean() <= 0.07, near.mean()
    return int((idx != golden).sum()), int(near.sum())


def _g2_replay(level):
    """G2's trace replayed through the float64 oracle as tests/test_oracle_golden.py::test_g2_traces_bit_exact does (and asserted the same), keeping per
    STEP row what a teacher-forced call needs: action, observation [7], MDP state before the step [8], previous index; and the golden row."""
    t = np.load(GOLDEN / "g2_traces.npz")[f"trace_{level}"]
    cfg = DqlConfig(working_curriculum_step=level, dtype=F64)
    orc = _oracle()
    ms = np.zeros((8, 1)); ms[7] = 8
    prev = np.array([-1], dtype=np.int32)
    acts, obss, mss, prevs, rows, after = [], [], [], [], [], []
    for row in t:
        obs = row[2:9].reshape(7, 1).copy()
        if int(row[0]) == 0:
            ms[0] = 0.0; ms[4] = 0.0; ms[5] = 0; ms[6] = 0; ms[7] = 8   # TrainingMdp.reset: everything but the shaping memory (B9)
            prev = orc.discretise(cfg, obs[0], obs[2], obs[3], obs[4]).astype(np.int32)
            np.testing.assert_array_equal(unpack_state(prev)[0], row[9:14].astype(int))
            continue
        acts.append(int(row[1])); obss.append(obs[:, 0]); mss.append(ms[:, 0].copy()); prevs.append(int(prev[0])); rows.append(row)
        ms, idx, rew, done = orc.mdp_transition(cfg, [int(row[1])], obs, ms, prev)
        assert (pack_state(row[9:14])) == idx[0] and int(ms[7, 0]) == int(row[14]) and rew[0] == row[15] and int(done[0]) == int(row[16])
        assert ms[0, 0] == row[17] and ms[4, 0] == row[18] and int(ms[5, 0]) == int(row[19]) and int(ms[6, 0]) == int(row[20])
        after.append(ms[:, 0].copy())
        prev = idx.astype(np.int32)
    return (np.array(acts, dtype=np.uint8), np.array(obss).T.copy(), np.array(mss).T.copy(), np.array(prevs, dtype=np.int32), np.array(rows),
            np.array(after).T.copy())


_G2_CACHE = {}


def g2_replay(level):
    if level not in _G2_CACHE:
        _G2_CACHE[level] = _g2_replay(level)
    return _G2_CACHE[level]


def _limit_near(obs, cfg):
    """a continuous input of check() within EDGE_REL of the limit it is compared with: |rel_p_x|, |rel_p_y| against p_max, z against minimum_altitude and p_max"""
    px, py, z = np.abs(obs[0]), np.abs(obs[1]), obs[5]
    nr = lambda x, lim: np.abs(x - lim) <= EDGE_REL * lim
    return nr(px, cfg.p_max) | nr(py, cfg.p_max) | nr(z, cfg.minimum_altitude) | nr(z, cfg.p_max)


def check_g2_traces(be, dtype, level):
    """check / reward / continuous_action through G2's scripted episodes (quirks B7-B11, B18), every step row TEACHER-FORCED: the float64 replay supplies the
    MDP state before the step, the previous index, the action and the observation, and ALL step rows go through one batched mdp_transition call of the backend.
    No difference is carried into a later row.

    float64: every output equals the golden row bit for bit (what test_g2_traces_bit_exact asserts of the sequential replay).
    float32, per row:
      index        as G1, edge-nearness from the row's observation
      code, done, step and goal counters   == golden where the index is and no input of check() is within 8 eps of its limit (time-out 458.4 and f_ag 22.92
                   are not integers: the integer counters cannot be near them)
      set-point    continuous_action: fl(fl(sp) +- fl(delta_theta)) clipped at fl(theta_max): |err| <= 2 eps theta_max
      reward       mdp_reward's float32 sequence, eps = 2^-24, relative roundings counted per term (rows with equal index and code):
          shp_p = w_p |ncp|: ncp carries 3 eps (cast, reciprocal, product), w_p = -100 is exact, the product 1:           4 eps |shp_p|
          r_p = clip(shp_p - prev_p, +-r_p_max): prev_p is the cast of the float64 memory (1 eps |prev_p|), the difference 1 eps (|r_p| <= |shp_p| + |prev_p|);
                the clip is 1-Lipschitz; its bound r_p_max = |w_p| lim_v delta_t <= 4.37 carries 4 eps:                   5 eps (|shp_p| + |prev_p|) + 18 eps
          r_v likewise with w_v = -10, r_v_max <= 0.44:                                                                     5 eps (|shp_v| + |prev_v|) + 2 eps
          r_theta = fl(fl(w_theta (|shp_a| - |prev_a|)) inv_theta_max) lim_v: shp_a = w_theta npitch, npitch = sp inv_theta_max within 4 eps absolute (set-point
                2 eps theta_max, reciprocal, product), shp_a within 1.55 * 6 eps, prev_a a cast (1.55 eps), the difference 1.55 eps: 1.55 * 8 eps; times w_theta
                (+2): 1.55^2 * 10; times 1 / theta_max = 2.68 (+2): 1.55^2 * 2.68 * 12; times lim_v <= 1 (+2): 1.55^2 * 2.68 * 14                        =  91 eps
          r_dur = w_dur lim_v delta_t <= 0.27, 5 roundings:                                                                                                  2 eps
          r_term = w r_max, r_max = r_p_max + r_v_max + r_theta_max + r_dur_max <= 5.6 with <= 6 eps, times 2.6 (+2): 2.6 * 5.6 * 8                      = 117 eps
          the four additions of terms that sum to <= 4.4 + 0.5 + 2 * 1.55^2 * 2.68 + 0.3 + 14.6 < 33 in magnitude: 4 * 33                                = 132 eps
        |reward error| <= eps (5 (|shp_p| + |prev_p| + |shp_v| + |prev_v|) + 362)  — <= 8.8e-5 at |shp_p| = |prev_p| = 100; measured 1.3e-5 (float32 oracle, level 4)
      shaping memory after the step (every row: it depends on neither index nor code): shp_p, shp_v within 4 eps relative, shp_a within 1.55 * 6 eps — the
                   terms above.  This is where a normalising reciprocal that is off by more than its rounding shows: in the index it only moves the bin
                   edges by a few eps, inside what G1 must allow, here it is a factor of every row's value (measured: <= 2.7 eps relative, shp_a 2.3 eps)
      cumulative   cast of the float64 sum + one addition: reward bound + 2 eps |cum|; measured 4.7e-4 at |cum| ~ 4 000 (half an ulp of the sum)
    and, because G2's own thresholds are not integers, the same rows once more with f_ag = 20 (time-out at exactly 400 steps, success at exactly 20 goal steps)
    against the float64 oracle: code, done and counters equal under the same exclusions — `>=` against `>` shows only there.
    Returns (excluded rows, edge-near rows, max reward error, max cumulative error)."""
    act, obs, ms0, prev, rows, ms_after = g2_replay(level)
    n = len(act)
    assert n > 1000
    cfg = DqlConfig(working_curriculum_step=level, dtype=dtype)
    ms, idx, rew, done = be.mdp_transition(cfg, act, obs, ms0, prev)
    golden = pack_state(rows[:, 9:14])
    if dtype == F64:
        np.testing.assert_array_equal(idx, golden)
        np.testing.assert_array_equal(ms[7].astype(int), rows[:, 14].astype(int), err_msg="check code")
        np.testing.assert_array_equal(rew, rows[:, 15], err_msg="reward")
        np.testing.assert_array_equal(done, rows[:, 16].astype(np.uint8))
        np.testing.assert_array_equal(ms[0], rows[:, 17], err_msg="pitch set-point (B11 float accumulator)")
        np.testing.assert_array_equal(ms[4], rows[:, 18], err_msg="cumulative reward")
        np.testing.assert_array_equal(ms[5].astype(int), rows[:, 19].astype(int)); np.testing.assert_array_equal(ms[6].astype(int), rows[:, 20].astype(int))
        np.testing.assert_array_equal(ms[1:4], ms_after[1:4], err_msg="shaping memory")
        return 0, 0, 0.0, 0.0
    cfg64 = DqlConfig(working_curriculum_step=level, dtype=F64)
    nb = edge_neighbours(cfg64, obs[0], obs[2], obs[3], obs[4])
    near = _index_rules(idx, golden, nb, f"G2 level {level}")
    same_idx = idx == golden
    lim_near = _limit_near(obs, cfg)
    held = same_idx & ~lim_near
    excluded = int((~held).sum())
    msg = f"level {level}: {excluded} of {n} rows excluded ({int((~same_idx).sum())} by index, {int(lim_near.sum())} by a limit), {int(near.sum())} edge-near"
    assert near.mean() <= 0.07 and excluded <= 0.07 * n, msg
    for j, col, name in ((7, 14, "check code"), (5, 19, "step counter"), (6, 20, "goal counter")):
        bad = held & (ms[j].astype(int) != rows[:, col].astype(int))
        assert not bad.any(), f"{name}: rows {np.flatnonzero(bad)[:5]}; {msg}"
    assert not (held & (done != rows[:, 16].astype(np.uint8))).any(), f"done; {msg}"
    e_sp = np.abs(ms[0] - rows[:, 17]).max()
    assert e_sp <= 2 * EPS * cfg.theta_max, (e_sp, msg)
    for j, name in ((1, "shp_p"), (2, "shp_v")):
        rel = np.abs(ms[j] - ms_after[j]) / np.maximum(np.abs(ms_after[j]), 1e-30)
        assert rel.max() <= 4 * EPS, f"{name} after the step: {rel.max() / EPS:.3g} eps relative, row {rel.argmax()}"
    e_a = np.abs(ms[3] - ms_after[3]).max()
    assert e_a <= abs(cfg.w_theta) * 6 * EPS, f"shp_a after the step: {e_a / EPS:.3g} eps"
    ok = held & (ms[7].astype(int) == rows[:, 14].astype(int))
    b_rew = EPS * (5 * (np.abs(ms_after[1]) + np.abs(ms0[1]) + np.abs(ms_after[2]) + np.abs(ms0[2])) + 362)
    e_rew = np.abs(rew - rows[:, 15]); e_cum = np.abs(ms[4] - rows[:, 18])
    b_cum = b_rew + 2 * EPS * np.abs(rows[:, 18])
    assert (e_rew <= b_rew)[ok].all(), f"reward: worst {(e_rew / b_rew)[ok].max():.3g} of the bound; {msg}"
    assert (e_cum <= b_cum)[ok].all(), f"cumulative reward: worst {(e_cum / b_cum)[ok].max():.3g} of the bound; {msg}"
    # integer thresholds: f_ag = 20 -> time-out at 400 steps (B18's episode runs to 459), success at the 20th goal step (the goal sitters run to 23)
    kw = dict(working_curriculum_step=level, f_ag=20.0)
    ms_i, idx_i, _, done_i = be.mdp_transition(DqlConfig(dtype=dtype, **kw), act, obs, ms0, prev)
    ms_r, idx_r, _, done_r = _oracle().mdp_transition(DqlConfig(dtype=F64, **kw), act, obs, ms0, prev)
    held_i = (idx_i == idx_r) & ~lim_near
    on_timeout = held_i & (ms0[5] == 399); on_success = held_i & (ms_r[6] == 20) & (ms0[6] == 19)
    assert on_timeout.any() and (ms_r[7][on_timeout] == 6).any(), "no row sits on the time-out threshold"
    assert on_success.any() and (ms_r[7][on_success] == 1).any(), "no row sits on the success threshold"
    for j in (5, 6, 7):
        bad = held_i & (ms_i[j].astype(int) != ms_r[j].astype(int))
        assert not bad.any(), f"integer thresholds (f_ag = 20), state row {j}: rows {np.flatnonzero(bad)[:5]}"
    assert not (held_i & (done_i != done_r)).any()
    return excluded, int(near.sum()), float(e_rew[ok].max()), float(e_cum[ok].max())


def check_g2s_simulation(be, dtype):
    """SimulationMdp (level 4, no goal branch: the library's DQL_MDP_SIMULATION stage) over G2s, teacher-forced like G2.  The fixture's rows carry the set-point
    and the check code after every step; the step counter before a row is the number of step rows since the episode's reset row; the goal counter is never
    read without the goal branch and the rows carry no reward (SimulationMdp.reward is 0.0), so the shaping memory is not needed either.  x state from
    (rel_p_x, rel_v_x, rel_a_x, pitch) through mdp_transition, y state from (rel_p_y, rel_v_y, rel_a_y, roll) through discretise.
    float64: bit for bit.  float32: the index rules of G1, code / done where the index is equal and no limit is near, set-point within 2 eps theta_max."""
    t = np.load(GOLDEN / "g2s_simulation.npz")["trace"]
    step = t[:, 0] == 1
    prev_row = np.flatnonzero(step) - 1
    count = np.zeros(len(t))
    for i in range(len(t)):
        count[i] = 0 if t[i, 0] == 0 else count[i - 1] + 1
    rows = t[step]
    n = len(rows)
    ms0 = np.zeros((8, n))
    ms0[0] = t[prev_row, 25]; ms0[5] = count[prev_row]
    ms0[7] = np.where(t[prev_row, 23] < 0, 8, t[prev_row, 23])
    obs = np.stack([rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 7], rows[:, 9], rows[:, 11], rows[:, 12]])
    act = rows[:, 1].astype(np.uint8)
    kw = dict(working_curriculum_step=4)
    cfg = DqlConfig(dtype=dtype, **kw)
    ms, idx, _, done = be.mdp_transition(cfg, act, obs, ms0, np.full(n, -1, dtype=np.int32), simulation=True)
    idy = be.discretise(cfg, t[:, 4], t[:, 6], t[:, 8], t[:, 10])
    gx, gy = pack_state(rows[:, 13:18]), pack_state(t[:, 18:23])
    if dtype == F64:
        np.testing.assert_array_equal(idx, gx); np.testing.assert_array_equal(idy, gy)
        np.testing.assert_array_equal(ms[7].astype(int), rows[:, 23].astype(int)); np.testing.assert_array_equal(done, rows[:, 24].astype(np.uint8))
        np.testing.assert_array_equal(ms[0], rows[:, 25]); np.testing.assert_array_equal(ms[5], count[step])
        return 0
    cfg64 = DqlConfig(dtype=F64, **kw)
    near = _index_rules(idx, gx, edge_neighbours(cfg64, obs[0], obs[2], obs[3], obs[4]), "G2s x")
    near_y = _index_rules(idy, gy, edge_neighbours(cfg64, t[:, 4], t[:, 6], t[:, 8], t[:, 10]), "G2s y")
    held = (idx == gx) & ~_limit_near(obs, cfg)
    assert near.mean() <= 0.07 and near_y.mean() <= 0.07 and (~held).sum() <= 0.07 * n, (near.sum(), near_y.sum(), (~held).sum(), n)
    assert not (held & (ms[7].astype(int) != rows[:, 23].astype(int))).any() and not (held & (done != rows[:, 24].astype(np.uint8))).any()
    assert not (held & (ms[5] != count[step])).any()
    assert np.abs(ms[0] - rows[:, 25]).max() <= 2 * EPS * cfg.theta_max
    assert (rows[:, 23] < 7).sum() >= 4, "the trace ends several episodes"
    return int((~held).sum())
