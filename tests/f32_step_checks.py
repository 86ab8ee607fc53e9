"""The fused float32 step against the float64 oracle at the flavours the curriculum and landing figures fly, and the reference's recorded env-class
flights (G13) re-flown in float32 — one body for two float32 sides: the CPU oracle's float32 build (tests/test_f32_step.py) and the HIP engine
(tests/test_gpu_f32_step.py, -m gpu).  The float64 side is always the oracle, which G1-G13 pin to the reference bit for bit.

tests/test_gpu_parity.py::test_f32_kernel_vs_f64_oracle compares the dtypes at level 0 under a random policy, 50 periods after reset, far above the
platform.  Here: levels 2 and 4 (nested limits, bins down to 1 / 6 of level 0's), the paper-mode observation pipeline (no B19: the acceleration is a
per-tick finite difference), a greedy policy on the reference's stage-4 tables, the simulation flavour down to touchdown, TERMINAL_SUCCESS and the
fly-zone terminations.  Under a state-dependent policy a differing index becomes a differing action, so the integer fields are compared after EVERY period
and an env leaves the comparison at its first difference.

Measured maxima per field group and flavour: profiles/f32_step_vs_f64_flavours.jsonl (tools/exp_f32_vs_f64.py flavours)."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from dql_multirotor_landing_amd.config import DqlConfig, F32, F64, Q_PAPER, Q_REFERENCE, simulation_config
from dql_multirotor_landing_amd.state_layout import to_f32_filter_state

GOLDEN = Path(__file__).resolve().parent / "golden"
EPS = 2.0 ** -24
N_ENVS = 2048      # 32 waves: the smallest n at which the 0.5 % cap still means ten envs and every class of episode end occurs
PERIODS = 16
_CONFIGS4 = dict(per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1)
# name -> (config keywords, policy, hand-over period); policy None = greedy (eval_steps), else the epsilon of train_steps
FLAVOURS = {
    "sim_paper": (lambda d: simulation_config(quirks=Q_PAPER, dtype=d), None, 192),
    "sim_paper_two_axis": (lambda d: simulation_config(quirks=Q_PAPER, two_axis=1, dtype=d), None, 192),
    "sim_paper_configs4": (lambda d: simulation_config(quirks=Q_PAPER, dtype=d, **_CONFIGS4), None, 192),
    "train_l4_paper": (lambda d: DqlConfig(working_curriculum_step=4, quirks=Q_PAPER, dtype=d), 0.1, 60),
    "train_l2_reference": (lambda d: DqlConfig(working_curriculum_step=2, quirks=Q_REFERENCE, dtype=d), 0.1, 60),
}
# tests/test_gpu_parity.py's lists and bounds (relative to max(|x|, 1) for _DYN / _OBS, absolute for _REW), after 1 and after 16 periods
_DYN = ["px", "py", "pz", "vx", "vy", "vz", "qw", "qx", "qy", "qz", "wx", "wy", "wz", "om0", "om1", "om2", "om3", "vz_i", "yw_i", "vz_state", "yw_state",
        "mp_phase", "mp_x", "mp_u", "mp_y", "mp_v", "pitch_sp", "roll_sp"]
_OBS = ["obs_p_x", "obs_v_x", "obs_a_x", "obs_p_y", "obs_v_y", "obs_a_y", "kal_x_x", "kal_y_x", "kal_x_P", "kal_y_P"]
_REW = ["reward", "cum_x", "cum_y", "shp_x_p", "shp_x_v", "shp_x_a", "shp_y_p", "shp_y_v", "shp_y_a"]
_ACC = {"obs_a_x": ("vx", "mp_u"), "kal_x_x": ("vx", "mp_u"), "obs_a_y": ("vy", "mp_v"), "kal_y_x": ("vy", "mp_v")}
TOL = {1: (1e-5, 2.5e-4), PERIODS: (1e-4, 5e-3)}
_INT = ("step_count", "code", "flags", "cur_check", "action", "idx_x", "idx_y")
GROUPS = {
    "pose": ["px", "py", "pz", "qw", "qx", "qy", "qz"], "vel": ["vx", "vy", "vz", "wx", "wy", "wz"], "rotor": ["om0", "om1", "om2", "om3"],
    "pid": ["vz_i", "yw_i", "vz_state", "yw_state"], "platform": ["mp_phase", "mp_x", "mp_u", "mp_y", "mp_v"],
    "obs_pv": ["obs_p_x", "obs_v_x", "obs_p_y", "obs_v_y"], "obs_a": ["obs_a_x", "obs_a_y", "kal_x_x", "kal_y_x"], "kal_P": ["kal_x_P", "kal_y_P"],
    "reward": ["reward"], "cum": ["cum_x", "cum_y"], "shaping": ["shp_x_p", "shp_x_v", "shp_x_a", "shp_y_p", "shp_y_v", "shp_y_a"], "sp": ["pitch_sp", "roll_sp"],
}


def stage4_tables():
    a = GOLDEN / "assets"
    return np.load(a / "Q_table_a.npy").ravel(), np.load(a / "Q_table_b.npy").ravel(), np.load(a / "state_action_count.npy").ravel()


def acc_is_difference_quotient(cfg) -> bool:
    """B19 off and Kalman R = 0: the acceleration observation is (v_i - v_(i-1)) / 0.01 passed through with gain 1"""
    from dql_multirotor_landing_amd.config import Q_FROZEN_ACC_REFERENCE
    return not (cfg.quirks & Q_FROZEN_ACC_REFERENCE) and cfg.noise_vel_sd == 0.0


def acc_bound(cfg, r64, names, tol_dyn, key):
    """Bound on |a32 - a64| for the acceleration pair where it is a difference quotient (DESIGN.md section 2 has the same derivation).
    a = (rv_i - rv_(i-1)) / T_m, T_m = manager_div dt = 0.01 s, rv = cy (u - v) + sy (...) the relative velocity in the yaw frame.  The float32 - float64
    difference of rv is a slowly drifting part, which cancels in rv_i - rv_(i-1) up to the dynamics' own difference (<= tol_dyn max(|a|, 1), as for every
    other field), plus what is rounded afresh between the two samples: the drone velocity's rounding in each of the manager_div physics ticks
    (manager_div eps |v|), the platform velocity evaluated anew at either tick (2 * 2 eps |u|), and the four roundings that form rv (difference, 2 eps
    of the yaw frame, product, fma) at either sample (8 eps |u - v|): <= (manager_div + 8) eps (|v| + |u|), divided by T_m — 1.3e3 eps = 7.7e-5 per m/s."""
    v, u = (np.abs(r64[names.index(k)]) for k in _ACC[key])
    a = np.abs(r64[names.index(key)])
    return (cfg.manager_div + 8) * EPS * (v + u) / (cfg.manager_div * cfg.dt) + tol_dyn * np.maximum(a, 1.0)


def fly(make32, flavour, n=N_ENVS, seed=9):
    """Hand a float64 flight over to the float32 side `make32(cfg, n, seed)` at the flavour's period and fly PERIODS more on both, one per call.
    Returns a dict: names / inames, cfg, `alive` [PERIODS][n] (no integer field has differed so far), the fields of both sides after period 1 and
    after the last, `ended` [n_codes] counts of the float64 side's episode ends inside the window by check code, `ended_envs` [n] bool per code 0,
    and the float32 side itself (`side`, still open) with the state both float32 backends were handed (`handed`)."""
    from oracle.oracle import Oracle
    make_cfg, eps, handover = FLAVOURS[flavour]
    qa, qb, cnt = stage4_tables()
    o64 = Oracle(make_cfg(F64), n, seed=seed, n_threads=8)
    s32 = make32(make_cfg(F32), n, seed)
    for s in (o64, s32):
        s.set_option("periods_per_launch", 1)
        s.set_tables(qa, qb, cnt)
    advance = (lambda s, k: s.eval_steps(k)) if eps is None else (lambda s, k: s.train_steps(k, eps))
    advance(o64, handover); advance(s32, handover)       # the float32 side flies too: same period index and table schedule; its state is overwritten
    reals, ints = o64.get_fields()
    names, inames = o64.field_names(), o64.field_names(True)
    assert names == s32.field_names() and inames == s32.field_names(True)
    tq = o64.qa.copy(), o64.qb.copy(), o64.count.copy()
    o64.set_tables(*tq); s32.set_tables(*tq)              # master == acting on both sides from here
    handed = (to_f32_filter_state(reals, names), ints.copy(), tq)
    s32.set_fields(handed[0], handed[1])
    alive = np.ones(n, dtype=bool)
    out = {"names": names, "inames": inames, "cfg": make_cfg(F64), "alive": [], "snap": {}, "side": s32, "handed": handed, "eps": eps,
           "ended": np.zeros(9, dtype=np.int64), "contact_envs": np.zeros(n, dtype=bool)}
    for k in range(1, PERIODS + 1):
        advance(o64, 1); advance(s32, 1)
        r64, i64 = o64.get_fields(); r32, i32 = s32.get_fields()
        for f in _INT:
            j = inames.index(f)
            alive &= i32[j] == i64[j]
        out["alive"].append(alive.copy())
        done = (i64[inames.index("flags")] & 1) != 0
        code = i64[inames.index("code")]
        out["ended"] += np.bincount(code[done], minlength=9)[:9]
        out["contact_envs"] |= done & (code == 0)
        if k in TOL:
            out["snap"][k] = (r32, i32, r64, i64)
    return out


def measured(res):
    """max |f32 - f64| per field group among the envs still compared, absolute and relative to max(|x|, 1), after period 1 and after the last"""
    names = res["names"]
    rows = {}
    for k, (r32, _, r64, _) in res["snap"].items():
        alive = res["alive"][k - 1]
        row = {}
        for g, fields in GROUPS.items():
            d = np.array([np.abs(r32[names.index(f)] - r64[names.index(f)])[alive].max() for f in fields])
            rel = np.array([(np.abs(r32[names.index(f)] - r64[names.index(f)]) / np.maximum(np.abs(r64[names.index(f)]), 1.0))[alive].max() for f in fields])
            row[g] = [float(d.max()), float(rel.max())]
        rows[k] = row
    return rows


def check_flavour(res, flavour):
    """assertions 1-3 of the module's contract on what fly() returned"""
    names, cfg = res["names"], res["cfg"]
    n = len(res["alive"][0])
    left = n - int(res["alive"][-1].sum())
    first = [n - int(a.sum()) for a in res["alive"]]
    assert left <= 0.005 * n, f"{flavour}: {left} of {n} envs left the comparison (per period, cumulative: {first})"
    own_acc = acc_is_difference_quotient(cfg)
    for k, (r32, _, r64, _) in res["snap"].items():
        alive = res["alive"][k - 1]
        tol_dyn, tol_rew = TOL[k]
        for f in _DYN + _OBS:
            j = names.index(f)
            d = np.abs(r32[j] - r64[j])
            if own_acc and f in _ACC:
                worst = (d / acc_bound(cfg, r64, names, tol_dyn, f))[alive].max()
                assert worst <= 1.0, f"{flavour}, {k} periods, {f}: {worst:.3g} of its difference-quotient bound"
            else:
                err = (d / np.maximum(np.abs(r64[j]), 1.0))[alive].max()
                assert err < tol_dyn, f"{flavour}, {k} periods, {f}: {err:.3g}"
        for f in _REW:
            j = names.index(f)
            err = np.abs(r32[j] - r64[j])[alive].max()
            assert err < tol_rew, f"{flavour}, {k} periods, {f}: {err:.3g}"
    ended = res["ended"]
    if res["eps"] is None:   # the simulation flavours: the window contains the touchdowns
        assert res["contact_envs"].sum() >= n // 2, f"{flavour}: only {int(res['contact_envs'].sum())} envs touched down inside the window: move the hand-over"
    else:                    # training: TERMINAL_SUCCESS and a fly-zone end (codes 2, 3, 4) occur
        assert ended[1] >= 1 and ended[2:5].sum() >= 1, f"{flavour}: episode ends by code {ended.tolist()}: move the hand-over"
    return left


def check_same_dtype_parity(res, flavour):
    """Assertion 4 (HIP leg): the float32 oracle, handed the same state at the same period and given the same calls, ends with every real and integer field
    — and, where the flavour learns, the tables — equal to the float32 engine's, bit for bit: same-dtype parity from a state set mid-flight, through
    touchdown, under a greedy policy on trained tables."""
    from oracle.oracle import Oracle
    make_cfg, eps, handover = FLAVOURS[flavour]
    eng = res["side"]
    n = len(res["alive"][0])
    twin = Oracle(make_cfg(F32), n, seed=9, n_threads=8)
    twin.set_option("periods_per_launch", 1)
    twin.set_tables(*stage4_tables())
    advance = (lambda s, k: s.eval_steps(k)) if eps is None else (lambda s, k: s.train_steps(k, eps))
    advance(twin, handover)
    reals, ints, tq = res["handed"]
    twin.set_tables(*tq)
    twin.set_fields(reals, ints)
    for _ in range(PERIODS):
        advance(twin, 1)
    er, ei = eng.get_fields(); tr, ti = twin.get_fields()
    for j, f in enumerate(res["inames"]):
        np.testing.assert_array_equal(ei[j], ti[j], err_msg=f"{flavour}: integer field {f}, HIP float32 != oracle float32")
    for j, f in enumerate(res["names"]):
        np.testing.assert_array_equal(er[j], tr[j], err_msg=f"{flavour}: field {f}, HIP float32 != oracle float32")
    if eps is not None:
        qa, qb, cnt = eng.get_tables()
        np.testing.assert_array_equal(np.ravel(qa), twin.qa); np.testing.assert_array_equal(np.ravel(qb), twin.qb); np.testing.assert_array_equal(np.ravel(cnt), twin.count)


# ---------------------------------------------------------------------------------------------------------------------------------
# G13: the reference's env classes' recorded flights, re-flown in float32 under the fixture's scripted actions
# ---------------------------------------------------------------------------------------------------------------------------------
G13_CASES = {"train0": dict(working_curriculum_step=0, t_max=4.0), "train2": dict(working_curriculum_step=2, t_max=4.0),
             "sim4": dict(working_curriculum_step=4, t_max=6.0, vz_setpoint=-0.4, init_uniform=2, goal_logic=0, z_init=4.0)}
G13_SEED = {"train0": 1300, "train2": 1302, "sim4": 1304}
G13_SIGNALS = ("obs_p_x", "obs_p_y", "obs_v_x", "obs_v_y", "obs_a_x", "obs_a_y", "qw", "qx", "qy", "qz", "pz")
# max |float32 - float64 recording| per signal column over the three flights, measured on the CPU float32 oracle (profiles/f32_step_vs_f64_flavours.jsonl,
# rows "g13"), times 4 and rounded up to one significant digit.  The factor leaves room for another correct float32 form; the actions are scripted, so the
# closed loop is stable and the error does not compound, while a wrong form moves these numbers by orders of magnitude.  CPU-measured; the float32 engine is
# bit-identical to the float32 oracle (tests/test_gpu_parity.py), so they hold for it unchanged.
G13_BOUNDS = {"obs_p_x": 2e-3, "obs_p_y": 7e-6, "obs_v_x": 9e-4, "obs_v_y": 3e-6, "obs_a_x": 7e-5, "obs_a_y": 0.0, "qw": 8e-7, "qx": 2e-7, "qy": 5e-6, "qz": 8e-8, "pz": 4e-5}
# (measured: 2.9e-4 m, 1.6e-6 m, 2.2e-4 m/s, 6.9e-7 m/s, 1.7e-5 m/s^2, 0 — the y observation of an x-axis flight is never computed —, 1.8e-7, 4.1e-8, 1.0e-6, 2.0e-8, 7.8e-6 m)


def g13_fly(make, tag, z):
    """the flight `tag` of the fixture in float32 on `make(cfg, 1, seed)`: per period the signal columns + contact flag, and was_reset, done, idx_x, code, reward, set-point"""
    o = make(DqlConfig(dtype=F32, **G13_CASES[tag]), 1, G13_SEED[tag])
    names, inames = o.field_names(), o.field_names(True)
    sig, res = [], []
    for a in z[f"{tag}_actions"]:
        o.step(np.array([a], dtype=np.uint8))
        reals, ints = o.get_fields()
        g = lambda k: float(reals[names.index(k)][0]); gi = lambda k: int(ints[inames.index(k)][0])
        sig.append([g(k) for k in G13_SIGNALS] + [float(bool(gi("flags") & 16))])
        res.append([float(bool(gi("flags") & 8)), float(bool(gi("flags") & 1)), gi("idx_x"), gi("code"), g("reward"), g("pitch_sp")])
    return np.array(sig), np.array(res)


def g13_signal_errors(tag, z, sig):
    rec = np.column_stack([z[f"{tag}_rec_obs"], z[f"{tag}_rec_quat"], z[f"{tag}_rec_z"]])
    return np.abs(sig[:, :len(G13_SIGNALS)] - rec).max(axis=0)


def check_g13_flight(tag, z, sig, res, bounds=None):
    """One recorded flight re-flown in float32 against the fixture, every period:
      * discrete state, reset flag, done and CheckResult == what the reference's env classes returned (`*_rows`); contact flag == the recording's
      * every signal column within G13_BOUNDS of the float64 recording
      * reward within what the period's own signal differences explain, plus rounding: reward() is the clipped (1-Lipschitz) difference of the shaping values
        of this step and of the previous STEP (reset() does not touch the shaping memory, B9), so a difference d_p, d_v, d_sp of the observed position,
        velocity and set-point moves it by at most |w_p| / p_max (d_p + d_p') + |w_v| / v_max (d_v + d_v') + w_theta^2 / theta_max^2 (d_sp + d_sp') (primed:
        previous step), and the float32 evaluation itself adds at most fixture_checks.check_g2_traces's bound at |shaping| <= |w|: eps (5 * 220 + 362) = 8.8e-5."""
    bounds = G13_BOUNDS if bounds is None else bounds
    cfg = DqlConfig(dtype=F64, **G13_CASES[tag])
    rows, want = z[f"{tag}_rows"], z[f"{tag}_sim"]
    assert len(rows) == len(res)
    pack = lambda t: ((((t[:, 0] * 3 + t[:, 1]) * 3 + t[:, 2]) * 3 + t[:, 3]) * 7 + t[:, 4]).astype(np.int64)
    np.testing.assert_array_equal(res[:, 2].astype(np.int64), pack(rows[:, 2:7]), err_msg=f"{tag}: discrete state")
    np.testing.assert_array_equal(res[:, 0] != 0, rows[:, 0] == 0, err_msg=f"{tag}: reset periods")
    step = rows[:, 0] == 1
    np.testing.assert_array_equal(res[step, 1] != 0, rows[step, 13] != 0, err_msg=f"{tag}: done")
    np.testing.assert_array_equal(res[:, 3], want[:, 3], err_msg=f"{tag}: check code of the float64 flight")
    if tag != "sim4":   # (SimulationLandingEnv returns neither: tests/test_oracle_golden.py)
        np.testing.assert_array_equal(res[step, 3].astype(int), rows[step, 14].astype(int), err_msg=f"{tag}: CheckResult")
    np.testing.assert_array_equal(sig[:, -1], z[f"{tag}_rec_contact"].astype(float), err_msg=f"{tag}: contact flag")
    assert rows[:, 13].sum() >= 3
    err = g13_signal_errors(tag, z, sig)
    for k, e in zip(G13_SIGNALS, err):
        assert e <= bounds[k], f"{tag}: {k} differs from the float64 recording by {e:.3g} > {bounds[k]:.3g}"
    rec = z[f"{tag}_rec_obs"]
    d_p, d_v = np.abs(sig[:, 0] - rec[:, 0]), np.abs(sig[:, 2] - rec[:, 2])
    d_sp = np.abs(res[:, 5] - want[:, 5])
    assert d_sp.max() <= 2 * EPS * cfg.theta_max
    sens = lambda i: abs(cfg.w_p) / cfg.p_max * d_p[i] + abs(cfg.w_v) / cfg.v_max * d_v[i] + cfg.w_theta ** 2 / cfg.theta_max ** 2 * d_sp[i]
    last, worst = None, 0.0
    for i in range(len(rows)):
        if not step[i]:
            continue
        explained = sens(i) + (sens(last) if last is not None else 0.0) + EPS * (5 * 220 + 362)
        ref = rows[i, 12] if tag != "sim4" else want[i, 4]
        e = abs(res[i, 4] - ref)
        assert e <= explained, f"{tag}, period {i}: reward differs by {e:.3g}, the signals explain {explained:.3g}"
        worst = max(worst, e)
        last = i
    return err, worst
