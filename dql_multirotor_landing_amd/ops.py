"""Stateless batch operators of the C ABI (computed on the device): the arithmetic behind the drop-in
`TrainingMdp` / `DoubleQLearningAgent` methods."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .config import CHECK_NAMES, DqlConfig, N_CELLS, Q_REFERENCE, TARGET_FRAC_BITS


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def discretise(cfg: DqlConfig, rel_p, rel_v, rel_a, angle, device: int = 0) -> np.ndarray:
    """TrainingMdp.discrete_state (pkg/mdp.py:257-333) for n observations -> packed indices (-1 where the reference raises)."""
    p, v, a, t = map(_f64, (rel_p, rel_v, rel_a, angle))
    if not (p.shape == v.shape == a.shape == t.shape and p.ndim == 1):
        raise ValueError("inputs must be 1-D arrays of equal length")
    out = np.zeros(len(p), dtype=np.int32)
    c = cfg.to_c()
    _lib.check(_lib.load().dql_discretise(C.byref(c), device, _p(p), _p(v), _p(a), _p(t), len(p), _p(out)))
    return out


MDP_ACTION, MDP_DISCRETISE, MDP_CHECK, MDP_REWARD, MDP_SIMULATION, MDP_ALL = 1, 2, 4, 8, 16, 15


def mdp_transition(cfg: DqlConfig, action, obs, mdp_state, prev_idx, idx=None, stages: int = MDP_ALL, device: int = 0):
    """Selected TrainingMdp / SimulationMdp methods (see DQL_MDP_* in include/dql.h) for n independent MDPs.
    Returns (mdp_state, idx, reward, done); arrays not touched by the selected stages come back unchanged / zero."""
    n = len(action)
    action = np.ascontiguousarray(action, dtype=np.uint8)
    obs = _f64(obs); ms = _f64(mdp_state).copy(); prev_idx = np.ascontiguousarray(prev_idx, dtype=np.int32)
    if obs.shape != (7, n) or ms.shape != (8, n) or prev_idx.shape != (n,):
        raise ValueError("obs must be [7][n], mdp_state [8][n], prev_idx [n]")
    idx = np.full(n, -1, dtype=np.int32) if idx is None else np.ascontiguousarray(idx, dtype=np.int32).copy()
    rew = np.zeros(n); done = np.zeros(n, dtype=np.uint8)
    c = cfg.to_c()
    _lib.check(_lib.load().dql_mdp_transition(C.byref(c), device, n, stages, _p(action), _p(obs), _p(ms), _p(prev_idx), _p(idx), _p(rew), _p(done)))
    return ms, idx, rew, done


def manager_run(cfg: DqlConfig, series, contact, seed: int = 0, device: int = 0) -> np.ndarray:
    """The 100 Hz manager tick (ManagerNode.publish_obs + ObservationUtils) over scripted series: `series` [n_series][n_ticks][14]
    (drone p, v, quaternion wxyz, platform x y u v), `contact` [n_series][n_ticks] -> [n_series][n_ticks][12] (include/dql.h)."""
    a = _f64(series); c = np.ascontiguousarray(contact, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 14 or c.shape != a.shape[:2]:
        raise ValueError("series must be [n_series][n_ticks][14], contact [n_series][n_ticks]")
    out = np.zeros(a.shape[:2] + (12,))
    cc = cfg.to_c()
    _lib.check(_lib.load().dql_manager_run(C.byref(cc), device, a.shape[0], a.shape[1], _p(a), _p(c), int(seed), _p(out)))
    return out


def plant_run(cfg: DqlConfig, init, rotor_cmd, device: int = 0) -> np.ndarray:
    """The plant of the fused step (rotor forces + rigid body + rotor filter + platform extrapolation / contact latch: what stands in
    for gazebo_motor_model.cpp + ODE) open loop: `init` [n_series][21] (p, v, quaternion wxyz, body rates, rotor speeds, platform
    x y u v), `rotor_cmd` [n_series][n_ticks][4] -> [n_series][n_ticks][20] state after every 500 Hz tick (include/dql.h)."""
    a = _f64(init); b = _f64(rotor_cmd)
    if a.ndim != 2 or a.shape[1] != 21 or b.ndim != 3 or b.shape[2] != 4 or b.shape[0] != a.shape[0]:
        raise ValueError("init must be [n_series][21], rotor_cmd [n_series][n_ticks][4]")
    out = np.zeros(b.shape[:2] + (20,))
    cc = cfg.to_c()
    _lib.check(_lib.load().dql_plant_run(C.byref(cc), device, b.shape[0], b.shape[1], _p(a), _p(b), _p(out)))
    return out


def butterworth_run(cfg: DqlConfig, x, device: int = 0) -> np.ndarray:
    """ButterworthFilter.update (pkg/filters.py:98-109) over a series from zero histories, in cfg.dtype arithmetic."""
    x = _f64(x)
    if x.ndim != 1:
        raise ValueError("x must be 1-D")
    y = np.zeros_like(x)
    c = cfg.to_c()
    _lib.check(_lib.load().dql_butterworth_run(C.byref(c), device, _p(x), len(x), _p(y)))
    return y


def kalman_run(cfg: DqlConfig, vel, dt_le0, device: int = 0) -> np.ndarray:
    """KalmanFilter3D.filter (pkg/filters.py:53-80) over vel [n][3] sampled at 100 Hz -> acceleration estimates [n - 1][3]
    (Q = cfg.kalman_q, R = cfg.noise_vel_sd ** 2; dt_le0[i] forces the reference's dt <= 0 branch)."""
    vel = _f64(vel); flags = np.ascontiguousarray(dt_le0, dtype=np.uint8)
    if vel.ndim != 2 or vel.shape[1] != 3 or flags.shape != (len(vel),):
        raise ValueError("vel must be [n][3], dt_le0 [n]")
    acc = np.zeros((max(len(vel) - 1, 0), 3))
    c = cfg.to_c()
    _lib.check(_lib.load().dql_kalman_run(C.byref(c), device, _p(vel), _p(flags), len(vel), _p(acc)))
    return acc


def pid_run(cfg: DqlConfig, params, state, device: int = 0):
    """PID.output (pkg/pid.py:62-104) over 500 Hz ticks; params = Kp Ki Kd lower upper windup setpoint (Kd = 0) -> (effort, integral)."""
    params = _f64(params); state = _f64(state)
    if params.shape != (7,) or state.ndim != 1:
        raise ValueError("params must have 7 entries, state must be 1-D")
    eff = np.zeros(len(state)); integ = np.zeros(len(state))
    c = cfg.to_c()
    _lib.check(_lib.load().dql_pid_run(C.byref(c), device, _p(params), _p(state), len(state), _p(eff), _p(integ)))
    return eff, integ


def attitude_run(cfg: DqlConfig, quat_xyzw, omega, cmd, xonly: int = 0, device: int = 0) -> np.ndarray:
    """AttitudeController.compute_rotor_velocities (pkg/attitude_controller.py:107-156): quaternions (x, y, z, w), body rates,
    cmd = roll, pitch, yaw rate, thrust -> commanded rotor speeds [n][4]."""
    q, w, u = map(_f64, (quat_xyzw, omega, cmd))
    n = len(q)
    if q.shape != (n, 4) or w.shape != (n, 3) or u.shape != (n, 4):
        raise ValueError("quat_xyzw must be [n][4], omega [n][3], cmd [n][4]")
    rot = np.zeros((n, 4))
    c = cfg.to_c()
    _lib.check(_lib.load().dql_attitude_run(C.byref(c), device, _p(q), _p(w), _p(u), n, int(xonly), _p(rot)))
    return rot


def platform_run(cfg: DqlConfig, n: int, carry: int = 0, device: int = 0) -> np.ndarray:
    """MovingPlatform.compute_trajectory (pkg/moving_platform.py:87-127) from phase 0 -> [n][4] = x, y, u, v per 100 Hz tick."""
    out = np.zeros((int(n), 4))
    c = cfg.to_c()
    _lib.check(_lib.load().dql_platform_run(C.byref(c), device, int(n), int(carry), _p(out)))
    return out


def selftest_sqrt(lo: float = 1e-30, hi: float = 3.4028234663852886e38, device: int = 0) -> int:
    """number of float32 inputs in [lo, hi] for which the float32 tick's square root is not the correctly rounded one (must be 0)"""
    lo_b = int(np.float32(lo).view(np.uint32)); hi_b = int(np.float32(hi).view(np.uint32))
    n = C.c_int64(-1)
    _lib.check(_lib.load().dql_diag_selftest_sqrt(device, lo_b, hi_b, C.byref(n)))
    return n.value


def selftest_sqrt_ieee(lo: float = 2.0 ** -102, hi: float = 3.4028234663852886e38, device: int = 0) -> int:
    """the same count for sqrt_(float), the square root of Box-Muller's radius: 0 at x = 0 and on its domain [2^-102, FLT_MAX]"""
    lo_b = int(np.float32(lo).view(np.uint32)); hi_b = int(np.float32(hi).view(np.uint32))
    n = C.c_int64(-1)
    _lib.check(_lib.load().dql_diag_selftest_sqrt_ieee(device, lo_b, hi_b, C.byref(n)))
    return n.value


DIAG_MAX_N = 1 << 24  # include/dql_diag.h DQL_DIAG_MAX_N


def det_math_run(x, y, dtype: int, device: int = 0):
    """The device's det_sincos / det_atan2 / det_log on chosen inputs in float32 (dtype 0) or float64 (1) arithmetic -> (sin x, cos x, atan2(y, x),
    log |x| or log 1 where |x| <= 1e-30) as float64.  Element i runs on thread i: elements 64 w .. 64 w + 63 share a wave (include/dql_diag.h)."""
    x, y = _f64(x), _f64(y)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D arrays of equal length")
    s = np.zeros_like(x); c = np.zeros_like(x); a = np.zeros_like(x); lg = np.zeros_like(x)
    _lib.check(_lib.load().dql_diag_det_math_run(device, int(dtype), _p(x), _p(y), len(x), _p(s), _p(c), _p(a), _p(lg)))
    return s, c, a, lg


def box_muller_run(ra, rb, dtype: int, device: int = 0):
    """The device's box_muller on raw 32-bit words -> the two normal deviates (n0, n1) as float64."""
    ra = np.ascontiguousarray(ra, dtype=np.uint32); rb = np.ascontiguousarray(rb, dtype=np.uint32)
    if ra.ndim != 1 or ra.shape != rb.shape:
        raise ValueError("ra and rb must be 1-D arrays of equal length")
    n0 = np.zeros(len(ra)); n1 = np.zeros(len(ra))
    _lib.check(_lib.load().dql_diag_box_muller_run(device, int(dtype), _p(ra), _p(rb), len(ra), _p(n0), _p(n1)))
    return n0, n1


def philox_run(counters, k0: int, k1: int, round_keys: int = 0, device: int = 0) -> np.ndarray:
    """The device's philox4x32 of counters [n][4] under the key (k0, k1) -> uint32 [n][4]; round_keys = 1: the form with the 20 round keys in registers."""
    ctr = np.ascontiguousarray(counters, dtype=np.uint32)
    if ctr.ndim != 2 or ctr.shape[1] != 4:
        raise ValueError("counters must be [n][4]")
    out = np.zeros_like(ctr)
    _lib.check(_lib.load().dql_diag_philox_run(device, _p(ctr), int(k0), int(k1), int(round_keys), len(ctr), _p(out)))
    return out


def place(cfg: DqlConfig, x0, mp, device: int = 0) -> np.ndarray:
    """Drone start coordinate for (random offset, platform coordinate) pairs: the reset placement selected by cfg.init_uniform."""
    x0, mp = _f64(x0), _f64(mp)
    if x0.shape != mp.shape or x0.ndim != 1:
        raise ValueError("x0 and mp must be 1-D arrays of equal length")
    out = np.zeros(len(x0))
    cc = cfg.to_c()
    _lib.check(_lib.load().dql_place(C.byref(cc), device, _p(x0), _p(mp), len(x0), _p(out)))
    return out


def agent_transfer(qa, qb, k: int, ratio: float, device: int = 0):
    """In-place DoubleQLearningAgent.transfer_learning on contiguous float64 tables of 2835 cells."""
    for t in (qa, qb):
        if t.dtype != np.float64 or not t.flags.c_contiguous or t.size != 2835:
            raise ValueError("tables must be contiguous float64 arrays of 2835 cells")
    _lib.check(_lib.load().dql_agent_transfer(device, _p(qa), _p(qb), int(k), float(ratio)))


def agent_predict(qa, qb, idx, device: int = 0) -> np.ndarray:
    qa, qb = _f64(qa).ravel(), _f64(qb).ravel()
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    out = np.zeros(len(idx), dtype=np.uint8)
    _lib.check(_lib.load().dql_agent_predict(device, _p(qa), _p(qb), _p(idx), len(idx), _p(out)))
    return out


def agent_update(qa, qb, count, sa, ns, alpha, gamma, reward, quirks: int = Q_REFERENCE, device: int = 0, coin=None, done=None):
    """In-place ordered replay of DoubleQLearningAgent.update; qa/qb/count must be contiguous float64 of 2835 cells.
    `quirks`: Q_REFERENCE reproduces the reference (table a only, bootstrap on a position-bin change); with
    Q_UPDATE_TABLE_A_ONLY cleared it is Double Q-learning and needs `coin` (0 = update table a, 1 = table b) per transition,
    with Q_BOOTSTRAP_ON_POS_CHANGE cleared it needs the `done` flags (include/dql.h)."""
    for t in (qa, qb, count):
        if t.dtype != np.float64 or not t.flags.c_contiguous or t.size != 2835:
            raise ValueError("tables must be contiguous float64 arrays of 2835 cells")
    sa = np.ascontiguousarray(sa, dtype=np.int32); ns = np.ascontiguousarray(ns, dtype=np.int32)
    alpha = _f64(alpha); reward = _f64(reward)
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
    coin, done = u8(coin), u8(done)
    for a in (coin, done):
        if a is not None and a.shape != sa.shape:
            raise ValueError("coin / done must have one entry per transition")
    _lib.check(_lib.load().dql_agent_update(device, _p(qa), _p(qb), _p(count), _p(sa), _p(ns), _p(alpha), float(gamma), _p(reward), len(sa), quirks,
                                            None if coin is None else _p(coin), None if done is None else _p(done)))


ROLLOUT_MAX_STEPS, ROLLOUT_MAX_TABLES = 4096, 16  # include/dql.h DQL_ROLLOUT_MAX_STEPS / DQL_ROLLOUT_MAX_TABLES
# include/dql.h dql_rollout_field_name (csrc/dql_rollout.hpp): a record's fields, and what a trace row adds
ROLLOUT_RECORD_FIELDS = ("cum_x", "cum_y", "reward", "px", "py", "pz", "vx", "vy", "vz", "mp_x", "mp_u", "mp_y", "mp_v", "qw", "qx", "qy", "qz", "pitch_sp", "roll_sp")
ROLLOUT_TRACE_FIELDS = ROLLOUT_RECORD_FIELDS + ("action", "idx_x", "idx_y")


def _table_sets(tables):
    """`tables`: one (qa, qb[, count]) set or a list of them -> ([K][2835] qa, [K][2835] qb), checked"""
    if len(tables) in (2, 3) and all(np.ndim(t) >= 1 and np.size(t) == 2835 for t in tables[:2]) and (len(tables) == 2 or np.size(tables[2]) == 2835):
        tables = [tables]
    tables = list(tables)
    if not 1 <= len(tables) <= ROLLOUT_MAX_TABLES:
        raise ValueError(f"between 1 and {ROLLOUT_MAX_TABLES} table sets per roll-out, not {len(tables)}")
    qa, qb = [], []
    for k, t in enumerate(tables):
        if len(t) < 2 or np.size(t[0]) != 2835 or np.size(t[1]) != 2835:
            raise ValueError(f"table set {k} must be (Q_table_a, Q_table_b[, counter]) of 2835 cells each")
        qa.append(_f64(t[0]).ravel()); qb.append(_f64(t[1]).ravel())
    return np.ascontiguousarray(np.stack(qa)), np.ascontiguousarray(np.stack(qb))


def _table_pair(qa, qb):
    """`qa`, `qb` as float64 [K, 2835] arrays of the same K (one set: [2835]), checked: what every greedy-flight operator but the roll-outs takes"""
    qa, qb = np.atleast_2d(_f64(qa)), np.atleast_2d(_f64(qb))
    if qa.ndim != 2 or qa.shape[1] != N_CELLS or qb.shape != qa.shape:
        raise ValueError("qa and qb must be [K, 2835] arrays of the same K")
    return qa, qb


def _last_call(lib, op: str, kernel: str, timing, times=("kernel_ms",)):
    """`timing`, if given, receives the kernel time(s) and the `instance` of this thread's latest completed call of the operator (include/dql_diag.h dql_diag_<op>_last)"""
    if timing is None:
        return
    ms, inst = [C.c_double() for _ in times], (C.c_int32 * 3)()
    _lib.check(getattr(lib, f"dql_diag_{op}_last")(*[C.byref(m) for m in ms], inst))
    timing.update({k: m.value for k, m in zip(times, ms)})
    timing["instance"] = f"{kernel}<{'float' if inst[0] == 4 else 'double'}, {inst[1]}, {inst[2]}>"


def rollout(cfg: DqlConfig, tables, envs_per_table: int, seed: int, max_steps: int = 600, trace_envs: int = 0, device: int = 0, timing: dict = None):
    """Every env's FIRST greedy episode from reset to termination in one launch, for up to 16 table sets at once (include/dql.h dql_rollout).

    `tables`: one (qa, qb) pair or a list of them (a third element, the counter, is ignored).  Every set flies the same `envs_per_table` episodes (env i
    has the RNG key and start of env i of `Engine(cfg, envs_per_table, seed)`).  Returns a dict of arrays [n_tables, envs_per_table]: `code` (the terminal
    CheckResult code, -1 while still flying after `max_steps`), `steps` and one entry per ROLLOUT_RECORD_FIELDS, all taken from the env's state at the end of
    the period its episode ended in; `trace` [max_steps + 1, len(ROLLOUT_TRACE_FIELDS), trace_envs] of table set 0's first envs (NaN after an env's end) or
    None, and `trace_fields`.  `timing`: a dict that receives `kernel_ms` and `instance` of this call."""
    qa, qb = _table_sets(tables)
    K, n, max_steps, trace_envs = len(qa), int(envs_per_table), int(max_steps), int(trace_envs)
    if n < 64 or n % 64:
        raise ValueError(f"envs_per_table must be a positive multiple of 64, not {n}")
    if not 1 <= max_steps <= ROLLOUT_MAX_STEPS:
        raise ValueError(f"max_steps must be in 1..{ROLLOUT_MAX_STEPS}, not {max_steps}")
    if not 0 <= trace_envs <= 64:
        raise ValueError(f"trace_envs must be in 0..64, not {trace_envs}")
    lib = _lib.load()
    nr, nt = C.c_int32(), C.c_int32()
    _lib.check(lib.dql_rollout_n_fields(C.byref(nr), C.byref(nt)))
    names = tuple(lib.dql_rollout_field_name(i, 1).decode() for i in range(nt.value))
    if names != ROLLOUT_TRACE_FIELDS or nr.value != len(ROLLOUT_RECORD_FIELDS):
        raise RuntimeError("libdql_hip.so's roll-out fields are not the ones this module names")
    code = np.zeros((K, n), np.int32); steps = np.zeros((K, n), np.int32); rec = np.zeros((nr.value, K, n))
    trace = np.zeros((max_steps + 1, nt.value, trace_envs)) if trace_envs else None
    c = cfg.to_c()
    _lib.check(lib.dql_rollout(C.byref(c), device, K, n, int(seed), max_steps, _p(qa), _p(qb), _p(code), _p(steps), _p(rec), trace_envs, None if trace is None else _p(trace)))
    _last_call(lib, "rollout", "k_rollout", timing)
    out = {"code": code, "steps": steps, "trace": trace, "trace_fields": ROLLOUT_TRACE_FIELDS}
    out.update({f: rec[k] for k, f in enumerate(ROLLOUT_RECORD_FIELDS)})
    return out


SCORE_MAX_TABLES, SCORE_MAX_EPISODES, SCORE_MAX_STEPS = 1 << 20, 64, 4096  # include/dql.h DQL_SCORE_MAX_*
SCORE_MAX_LANES = 1 << 30
SCORE_COLUMNS = tuple(CHECK_NAMES) + ("unfinished",)  # the columns of `by_code`


def score_check_args(n_tables: int, envs_per_table: int, episodes: int, max_steps: int):
    """the argument checks of dql_score / dql_ensemble_score, made before the library is touched"""
    if not 1 <= n_tables <= SCORE_MAX_TABLES:
        raise ValueError(f"between 1 and {SCORE_MAX_TABLES} table sets per call, not {n_tables}")
    if envs_per_table < 64 or envs_per_table % 64:
        raise ValueError(f"envs_per_table must be a positive multiple of 64, not {envs_per_table}")
    if n_tables * envs_per_table > SCORE_MAX_LANES:
        raise ValueError(f"table sets x envs must be at most 2^30, not {n_tables * envs_per_table}")
    if not 1 <= episodes <= SCORE_MAX_EPISODES:
        raise ValueError(f"episodes must be in 1..{SCORE_MAX_EPISODES}, not {episodes}")
    if not 1 <= max_steps <= SCORE_MAX_STEPS:
        raise ValueError(f"max_steps must be in 1..{SCORE_MAX_STEPS}, not {max_steps}")


def score_buffers(n_tables: int, envs_per_table: int, episodes: int, log: bool):
    """(by_code, steps_sum, ep_code or None, ep_steps or None) as the C calls fill them"""
    by_code = np.zeros((n_tables, len(SCORE_COLUMNS)), np.int64); steps_sum = np.zeros(n_tables, np.int64)
    ep_code = np.zeros((episodes, n_tables * envs_per_table), np.uint8) if log else None
    ep_steps = np.zeros((episodes, n_tables * envs_per_table), np.uint16) if log else None
    return by_code, steps_sum, ep_code, ep_steps


def score_result(lib, by_code, steps_sum, ep_code, ep_steps, timing):
    _last_call(lib, "score", "k_score", timing)
    return {"by_code": by_code, "steps_sum": steps_sum, "ep_code": ep_code, "ep_steps": ep_steps, "columns": SCORE_COLUMNS}


def rates_from_counts(by_code, column: str):
    """share of all episodes asked for (finished or not) that ended with the check code `column`, per table set: by_code[:, column] / by_code.sum(axis=1)"""
    by_code = np.atleast_2d(np.asarray(by_code, dtype=np.int64))
    if by_code.shape[1] != len(SCORE_COLUMNS):
        raise ValueError(f"by_code must have {len(SCORE_COLUMNS)} columns")
    total = by_code.sum(axis=1)
    if (total <= 0).any():
        raise ValueError("a row of by_code counts no episode")
    return by_code[:, SCORE_COLUMNS.index(column)] / total


def score(cfg: DqlConfig, qa, qb, envs_per_table: int, seed: int, episodes: int = 1, max_steps: int = 600, log: bool = False, device: int = 0, timing: dict = None):
    """How the greedy episodes of K table sets end, counted on the device in one launch (include/dql.h dql_score).

    `qa`, `qb`: float64 [K, 2835] (one set: [2835]).  Every set flies `envs_per_table` envs (env i has the RNG key and start of env i of
    `Engine(cfg, envs_per_table, seed)`), each until it has finished `episodes` episodes or `max_steps` periods are over.  Returns a dict: `by_code` int64
    [K, len(SCORE_COLUMNS)] (finished episodes by terminal code, last column the episodes not finished), `steps_sum` int64 [K], `columns`, and with `log`
    `ep_code` uint8 / `ep_steps` uint16 [episodes, K * envs_per_table] (0xff / 0: not finished), else None.  `timing`: receives `kernel_ms` and `instance`."""
    qa, qb = _table_pair(qa, qb)
    K, n, episodes, max_steps = len(qa), int(envs_per_table), int(episodes), int(max_steps)
    score_check_args(K, n, episodes, max_steps)
    lib = _lib.load()
    by_code, steps_sum, ep_code, ep_steps = score_buffers(K, n, episodes, log)
    c = cfg.to_c()
    _lib.check(lib.dql_score(C.byref(c), device, K, n, episodes, int(seed), max_steps, _p(qa), _p(qb), _p(by_code), _p(steps_sum),
                             None if ep_code is None else _p(ep_code), None if ep_steps is None else _p(ep_steps)))
    return score_result(lib, by_code, steps_sum, ep_code, ep_steps, timing)


SCORE_MAP_MAX_TABLES = 1 << 14  # include/dql.h DQL_SCORE_MAP_MAX_TABLES: the map is 22 680 B per table set
NO_CELL = 0xFFFF                # `ep_last_cell` of an episode that did not finish, and of the y plane without a y axis


def score_map_check_args(n_tables: int, envs_per_table: int, episodes: int, max_steps: int):
    """the argument checks of dql_score_map / dql_ensemble_score_map, made before the library is touched"""
    if not 1 <= n_tables <= SCORE_MAP_MAX_TABLES:
        raise ValueError(f"between 1 and {SCORE_MAP_MAX_TABLES} table sets per mapping call, not {n_tables}: slice the sets")
    score_check_args(n_tables, envs_per_table, episodes, max_steps)


def score_map_buffers(n_tables: int, envs_per_table: int, episodes: int, log: bool):
    """(by_code, steps_sum, visits, ep_code or None, ep_steps or None, ep_last_cell or None) as the C calls fill them"""
    by_code, steps_sum, ep_code, ep_steps = score_buffers(n_tables, envs_per_table, episodes, log)
    visits = np.zeros((n_tables, N_CELLS), np.int64)
    ep_last_cell = np.zeros((2, episodes, n_tables * envs_per_table), np.uint16) if log else None
    return by_code, steps_sum, visits, ep_code, ep_steps, ep_last_cell


def score_map_result(lib, by_code, steps_sum, visits, ep_code, ep_steps, ep_last_cell, timing):
    _last_call(lib, "score_map", "k_score_map", timing)
    return {"by_code": by_code, "steps_sum": steps_sum, "ep_code": ep_code, "ep_steps": ep_steps, "columns": SCORE_COLUMNS, "visits": visits, "ep_last_cell": ep_last_cell}


def score_map(cfg: DqlConfig, qa, qb, envs_per_table: int, seed: int, episodes: int = 1, max_steps: int = 600, log: bool = False, device: int = 0, timing: dict = None):
    """`score`, and where the greedy policy of every table set flew (include/dql.h dql_score_map): the same arguments fly the same episodes and give the same
    `by_code`, `steps_sum`, `ep_code` and `ep_steps`.  On top of them `visits` int64 [K, 2835]: how many greedy decisions set k made at each cell (state the
    action was decided from, times 3, plus the action; with two axes both axes' decisions), and with `log` `ep_last_cell` uint16 [2, episodes, K *
    envs_per_table]: the x and y cell of the decision in whose period the episode ended (0xffff: not finished, or no y axis), else None.  At most
    SCORE_MAP_MAX_TABLES sets per call.  `timing`: receives `kernel_ms` and `instance`."""
    qa, qb = _table_pair(qa, qb)
    K, n, episodes, max_steps = len(qa), int(envs_per_table), int(episodes), int(max_steps)
    score_map_check_args(K, n, episodes, max_steps)
    lib = _lib.load()
    by_code, steps_sum, visits, ep_code, ep_steps, ep_last_cell = score_map_buffers(K, n, episodes, log)
    c = cfg.to_c()
    opt = lambda a: None if a is None else _p(a)
    _lib.check(lib.dql_score_map(C.byref(c), device, K, n, episodes, int(seed), max_steps, _p(qa), _p(qb), _p(by_code), _p(steps_sum), _p(visits), opt(ep_code), opt(ep_steps),
                                 opt(ep_last_cell)))
    return score_map_result(lib, by_code, steps_sum, visits, ep_code, ep_steps, ep_last_cell, timing)


MODEL_MAX_TABLES = 16  # include/dql.h DQL_MODEL_MAX_TABLES: the pair table is 10.7 MB per table set
N_STATES = N_CELLS // 3


def model_check_args(cfg: DqlConfig, n_tables: int, envs_per_table: int, episodes: int, max_steps: int, eps: float):
    """the argument checks of dql_model / dql_ensemble_model, made before the library is touched"""
    if cfg.two_axis:
        raise ValueError("the transition model is the x MDP's (the reward is not kept per axis): a two-axis config is refused")
    if not 1 <= n_tables <= MODEL_MAX_TABLES:
        raise ValueError(f"between 1 and {MODEL_MAX_TABLES} table sets per model call, not {n_tables}: slice the sets")
    score_check_args(n_tables, envs_per_table, episodes, max_steps)
    if envs_per_table * (max_steps + 1) >= 1 << 32:
        raise ValueError(f"envs_per_table * (max_steps + 1) must be below 2^32 (a 32-bit pair count), not {envs_per_table * (max_steps + 1)}")
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"eps must be in [0, 1], not {eps}")


def model_buffers(n_tables: int):
    """(pairs, reward_fx, terminal, by_code, steps_sum) as the C calls fill them"""
    return (np.zeros((n_tables, N_CELLS, N_STATES), np.uint32), np.zeros((n_tables, N_CELLS), np.int64), np.zeros((n_tables, N_CELLS, len(CHECK_NAMES)), np.int64),
            np.zeros((n_tables, len(SCORE_COLUMNS)), np.int64), np.zeros(n_tables, np.int64))


def model_result(lib, pairs, reward_fx, terminal, by_code, steps_sum, timing):
    _last_call(lib, "model", "k_model", timing)
    return {"pairs": pairs, "reward_fx": reward_fx, "terminal": terminal, "by_code": by_code, "steps_sum": steps_sum, "columns": SCORE_COLUMNS,
            "visits": pairs.sum(axis=-1, dtype=np.int64) + terminal.sum(axis=-1)}


def transition_model(cfg: DqlConfig, qa, qb, envs_per_table: int, seed: int, eps: float, episodes: int = 1, max_steps: int = 600, device: int = 0, timing: dict = None):
    """The empirical transition model of the discretised x MDP under the eps-greedy policy of K table sets, counted on the device in one launch (include/dql.h
    dql_model).

    `qa`, `qb`: float64 [K, 2835] (one set: [2835]), K up to MODEL_MAX_TABLES.  The envs and periods are `score`'s; an env explores with probability `eps` (the
    action stream's draw, as in training) and takes its tables' greedy action otherwise; nothing is learnt.  With cell = state before the period * 3 + action,
    every decision adds to `pairs` uint32 [K, 2835, 945] at (cell, state after) if the episode went on, to `terminal` int64 [K, 2835, len(CHECK_NAMES)] at
    (cell, code) if it ended, and its reward times 2^26 (rounded to nearest even) to `reward_fx` int64 [K, 2835].  `by_code` and `steps_sum` are `score`'s;
    `visits` int64 [K, 2835] = pairs.sum(-1) + terminal.sum(-1).  Integer sums: bit-reproducible.  `timing`: receives `kernel_ms` and `instance`."""
    qa, qb = _table_pair(qa, qb)
    K, n, episodes, max_steps, eps = len(qa), int(envs_per_table), int(episodes), int(max_steps), float(eps)
    model_check_args(cfg, K, n, episodes, max_steps, eps)
    lib = _lib.load()
    pairs, reward_fx, terminal, by_code, steps_sum = model_buffers(K)
    c = cfg.to_c()
    _lib.check(lib.dql_model(C.byref(c), device, K, n, episodes, int(seed), max_steps, eps, _p(qa), _p(qb), _p(pairs), _p(reward_fx), _p(terminal), _p(by_code), _p(steps_sum)))
    return model_result(lib, pairs, reward_fx, terminal, by_code, steps_sum, timing)


MODEL_SPLIT_MAX_TABLES, SPLIT_FRAC_BITS = 8, 20  # include/dql.h DQL_MODEL_SPLIT_MAX_TABLES (21.4 MB of pair table per set), DQL_SPLIT_FRAC_BITS
# include/dql.h DQL_SPLIT_*: a feature's code is its place in this tuple
SPLIT_FEATURES = ("coin", "obs_p_x", "obs_v_x", "obs_a_x", "pitch_sp", "mp_phase", "mp_u", "altitude", "v_z", "step", "prev_action")


def split_feature_code(feature) -> int:
    """a DQL_SPLIT_* code from a code or a name ("pitch_sp", "PITCH_SP", "DQL_SPLIT_PITCH_SP")"""
    if isinstance(feature, str):
        name = feature.lower()
        name = name[len("dql_split_"):] if name.startswith("dql_split_") else name
        if name not in SPLIT_FEATURES:
            raise ValueError(f"no split feature named {feature!r}: one of {', '.join(SPLIT_FEATURES)}")
        return SPLIT_FEATURES.index(name)
    if isinstance(feature, (bool, float)) or not isinstance(feature, (int, np.integer)) or not 0 <= int(feature) < len(SPLIT_FEATURES):
        raise ValueError(f"a split feature is a name or a code in 0..{len(SPLIT_FEATURES) - 1}, not {feature!r}")
    return int(feature)


def split_cut_array(cut):
    """the per-state cut as the C calls take it: float64 [945] from a scalar or a [945] array; no NaN (+-inf are meaningful)"""
    c = np.asarray(cut, np.float64)
    if c.ndim == 0:
        c = np.full(N_STATES, float(c))
    if c.shape != (N_STATES,):
        raise ValueError(f"cut must be a scalar or have shape ({N_STATES},), not {c.shape}")
    if np.isnan(c).any():
        raise ValueError("cut holds a NaN (+-inf are allowed: with +inf everything is in half 0)")
    return np.ascontiguousarray(c)


def split_model_check_args(cfg: DqlConfig, n_tables: int, envs_per_table: int, episodes: int, max_steps: int, eps: float):
    """the argument checks of dql_model_split / dql_ensemble_model_split beyond feature and cut, made before the library is touched"""
    if not 1 <= n_tables <= MODEL_SPLIT_MAX_TABLES:
        raise ValueError(f"between 1 and {MODEL_SPLIT_MAX_TABLES} table sets per split-model call, not {n_tables}: slice the sets")
    model_check_args(cfg, n_tables, envs_per_table, episodes, max_steps, eps)
    if envs_per_table * (max_steps + 1) >= 1 << 30:
        raise ValueError(f"envs_per_table * (max_steps + 1) must be below 2^30 (a 64-bit feature sum), not {envs_per_table * (max_steps + 1)}")


def split_model_buffers(n_tables: int):
    """(pairs, reward_fx, terminal, feat_sum_fx, by_code, steps_sum) as the C calls fill them"""
    return (np.zeros((n_tables, 2, N_CELLS, N_STATES), np.uint32), np.zeros((n_tables, 2, N_CELLS), np.int64), np.zeros((n_tables, 2, N_CELLS, len(CHECK_NAMES)), np.int64),
            np.zeros((n_tables, N_STATES), np.int64), np.zeros((n_tables, len(SCORE_COLUMNS)), np.int64), np.zeros(n_tables, np.int64))


def split_model_result(lib, feature, cut, pairs, reward_fx, terminal, feat_sum_fx, by_code, steps_sum, timing):
    _last_call(lib, "model_split", "k_model_split", timing)
    visits = pairs.sum(axis=-1, dtype=np.int64) + terminal.sum(axis=-1)
    return {"pairs": pairs, "reward_fx": reward_fx, "terminal": terminal, "feat_sum_fx": feat_sum_fx, "by_code": by_code, "steps_sum": steps_sum, "columns": SCORE_COLUMNS,
            "visits": visits, "state_visits": visits.sum(axis=1).reshape(len(visits), N_STATES, 3).sum(axis=-1), "feature": SPLIT_FEATURES[feature], "cut": cut}


def split_model(cfg: DqlConfig, qa, qb, envs_per_table: int, seed: int, eps: float, feature, cut, episodes: int = 1, max_steps: int = 600, device: int = 0, timing: dict = None):
    """`transition_model` with every counted decision sent to one of two halves by one bit of hidden state (include/dql.h dql_model_split).

    The flights are `transition_model`'s for the same arguments; `feature` (a name of SPLIT_FEATURES or its code) and `cut` (a scalar or float64 [945], per state
    before the period; no NaN, +-inf allowed) touch none.  value = the feature read from the env as it stands before the period, half = value >= cut[state].
    `pairs` uint32 [K, 2, 2835, 945], `terminal` int64 [K, 2, 2835, codes] and `reward_fx` int64 [K, 2, 2835] are `transition_model`'s with the half as the second
    index (the halves sum to them); `feat_sum_fx` int64 [K, 945] sums rint(value * 2^20) per state; `by_code`, `steps_sum` as there.  Derived: `visits` int64
    [K, 2, 2835], `state_visits` int64 [K, 945].  K up to MODEL_SPLIT_MAX_TABLES.  Integer sums: bit-reproducible.  `timing`: receives `kernel_ms` and `instance`."""
    feature, cut = split_feature_code(feature), split_cut_array(cut)
    qa, qb = _table_pair(qa, qb)
    K, n, episodes, max_steps, eps = len(qa), int(envs_per_table), int(episodes), int(max_steps), float(eps)
    split_model_check_args(cfg, K, n, episodes, max_steps, eps)
    lib = _lib.load()
    pairs, reward_fx, terminal, feat_sum_fx, by_code, steps_sum = split_model_buffers(K)
    c = cfg.to_c()
    _lib.check(lib.dql_model_split(C.byref(c), device, K, n, episodes, int(seed), max_steps, eps, feature, _p(cut), _p(qa), _p(qb), _p(pairs), _p(reward_fx), _p(terminal),
                                   _p(feat_sum_fx), _p(by_code), _p(steps_sum)))
    return split_model_result(lib, feature, cut, pairs, reward_fx, terminal, feat_sum_fx, by_code, steps_sum, timing)


SCORE_REFINED_MAX_TABLES = 4096  # include/dql.h DQL_SCORE_REFINED_MAX_TABLES: 90 720 B of tables are uploaded per refined set


def refined_table_pair(qa, qb):
    """`qa`, `qb` as float64 [K, 2, 2835] arrays of the same K (one set: [2, 2835]), checked: refined table sets, the half the slow index"""
    qa, qb = _f64(qa), _f64(qb)
    if qa.ndim == 2:
        qa = qa[None]
    if qb.ndim == 2:
        qb = qb[None]
    if qa.ndim != 3 or qa.shape[1:] != (2, N_CELLS) or qb.shape != qa.shape:
        raise ValueError("qa and qb must be [K, 2, 2835] arrays of the same K: refined table sets, the half the slow index")
    return np.ascontiguousarray(qa), np.ascontiguousarray(qb)


def score_refined_check_args(cfg: DqlConfig, n_tables: int, envs_per_table: int, episodes: int, max_steps: int, max_tables: int = SCORE_REFINED_MAX_TABLES):
    """the argument checks of dql_score_refined / dql_ensemble_score_refined beyond feature and cut, made before the library is touched"""
    if not 1 <= n_tables <= max_tables:
        raise ValueError(f"between 1 and {max_tables} refined table sets per call, not {n_tables}: slice the sets")
    score_check_args(n_tables, envs_per_table, episodes, max_steps)
    if cfg.two_axis:
        raise ValueError("two-axis configs are refused: the refinement is the x MDP's")
    if cfg.trajectory != 0:
        raise ValueError("the figure-eight trajectory is refused: the refinement is the x MDP's, as the learners are")


def score_refined_result(lib, feature, cut, by_code, steps_sum, ep_code, ep_steps, timing):
    _last_call(lib, "score_refined", "k_score_refined", timing)
    return {"by_code": by_code, "steps_sum": steps_sum, "ep_code": ep_code, "ep_steps": ep_steps, "columns": SCORE_COLUMNS, "feature": SPLIT_FEATURES[feature], "cut": cut}


def score_refined(cfg: DqlConfig, qa, qb, feature, cut, envs_per_table: int, seed: int, episodes: int = 1, max_steps: int = 600, log: bool = False, device: int = 0,
                  timing: dict = None):
    """`score` of K REFINED table sets (include/dql.h dql_score_refined): `qa`, `qb` float64 [K, 2, 2835], the half the slow index.

    The envs and periods are `score`'s for the same arguments; the greedy row of a decision is that of the refined state half * 945 + idx_x, with
    half = value >= cut[idx_x] and value the `feature` (a name of SPLIT_FEATURES or its code) read from the env as it stands before the period — `split_model`'s
    half, decision for decision.  `cut`: a scalar or float64 [945], no NaN; +inf flies half 0's tables and -inf half 1's.  Returns `score`'s dict plus `feature`
    and `cut`.  K up to SCORE_REFINED_MAX_TABLES.  `timing`: receives `kernel_ms` and `instance`."""
    feature, cut = split_feature_code(feature), split_cut_array(cut)
    qa, qb = refined_table_pair(qa, qb)
    K, n, episodes, max_steps = len(qa), int(envs_per_table), int(episodes), int(max_steps)
    score_refined_check_args(cfg, K, n, episodes, max_steps)
    lib = _lib.load()
    by_code, steps_sum, ep_code, ep_steps = score_buffers(K, n, episodes, log)
    c = cfg.to_c()
    _lib.check(lib.dql_score_refined(C.byref(c), device, K, n, episodes, int(seed), max_steps, feature, _p(cut), _p(qa), _p(qb), _p(by_code), _p(steps_sum),
                                     None if ep_code is None else _p(ep_code), None if ep_steps is None else _p(ep_steps)))
    return score_refined_result(lib, feature, cut, by_code, steps_sum, ep_code, ep_steps, timing)


GRID_MAX_SCENARIOS, GRID_TOUCH_BINS = 1024, 8  # include/dql.h DQL_GRID_MAX_SCENARIOS, DQL_GRID_TOUCH_BINS
GRID_SHARED_FIELDS = ("dtype", "two_axis", "f_ag", "dt", "manager_div")  # what one launch must share: the kernel instance and the tick schedule


def grid_check_args(cfgs, n_tables: int, envs_per_table: int, episodes: int, max_steps: int):
    """the argument checks of dql_score_grid / dql_ensemble_score_grid, made before the library is touched"""
    if not 1 <= len(cfgs) <= GRID_MAX_SCENARIOS:
        raise ValueError(f"between 1 and {GRID_MAX_SCENARIOS} scenarios per call, not {len(cfgs)}")
    for s, c in enumerate(cfgs):
        if not isinstance(c, DqlConfig):
            raise ValueError(f"scenario {s} is not a DqlConfig")
        for f in GRID_SHARED_FIELDS:
            if getattr(c, f) != getattr(cfgs[0], f):
                raise ValueError(f"scenario {s} differs from scenario 0 in {f} ({getattr(c, f)!r} vs {getattr(cfgs[0], f)!r}), which one launch must share")
    score_check_args(n_tables, envs_per_table, episodes, max_steps)
    if len(cfgs) * n_tables * envs_per_table > SCORE_MAX_LANES:
        raise ValueError(f"scenarios x table sets x envs must be at most 2^30, not {len(cfgs) * n_tables * envs_per_table}")


def grid_configs_to_c(cfgs):
    """the scenarios as one contiguous dql_config array"""
    from .config import DqlConfigC
    arr = (DqlConfigC * len(cfgs))()
    for s, c in enumerate(cfgs):
        arr[s] = c.to_c()
    return arr


def grid_touch_edges(cfgs) -> np.ndarray:
    """float64 [S, 7]: the bin edges j * mp_half_x / 4, j = 1 .. 7, rounded to the scenarios' real type as the library rounds them (include/dql.h)"""
    t = np.float32 if cfgs[0].dtype == 0 else np.float64
    return np.array([[float(t(float(j) * c.mp_half_x * 0.25)) for j in range(1, GRID_TOUCH_BINS)] for c in cfgs], np.float64)


def grid_buffers(n_scenarios: int, n_tables: int, envs_per_table: int, episodes: int, log: bool, touch: bool):
    """(by_code, steps_sum, touch_hist or None, ep_code or None, ep_steps or None) as the C calls fill them"""
    S, K = n_scenarios, n_tables
    by_code = np.zeros((S, K, len(SCORE_COLUMNS)), np.int64); steps_sum = np.zeros((S, K), np.int64)
    touch_hist = np.zeros((S, K, GRID_TOUCH_BINS), np.int64) if touch else None
    ep_code = np.zeros((S, episodes, K * envs_per_table), np.uint8) if log else None
    ep_steps = np.zeros((S, episodes, K * envs_per_table), np.uint16) if log else None
    return by_code, steps_sum, touch_hist, ep_code, ep_steps


def grid_result(lib, cfgs, by_code, steps_sum, touch_hist, ep_code, ep_steps, timing):
    _last_call(lib, "score_grid", "k_score_grid", timing)
    return {"by_code": by_code, "steps_sum": steps_sum, "touch_hist": touch_hist, "touch_edges": grid_touch_edges(cfgs), "ep_code": ep_code, "ep_steps": ep_steps,
            "columns": SCORE_COLUMNS}


def score_grid(cfgs, qa, qb, envs_per_table: int, seed: int, episodes: int = 1, max_steps: int = 600, log: bool = False, touch: bool = True, device: int = 0,
               timing: dict = None):
    """`score` of K table sets under each of S scenarios in ONE launch, plus where on the platform the touchdowns land (include/dql.h dql_score_grid, DESIGN.md
    section 20).

    `cfgs`: a list of DqlConfig (`config.scenario_grid` builds one) that share dtype, two_axis, f_ag, dt and manager_div and may differ in anything else.
    Slice s of every output is what `score(cfgs[s], ...)` returns: `by_code` int64 [S, K, len(SCORE_COLUMNS)], `steps_sum` int64 [S, K], and with `log` `ep_code`
    uint8 / `ep_steps` uint16 [S, episodes, K * envs_per_table].  Env i of every (scenario, set) has the key (i, seed): first episodes are paired across both axes.
    With `touch`, `touch_hist` int64 [S, K, 8] counts the episodes that ended in TERMINAL_CONTACT by the drone's horizontal offset from the platform centre
    after the terminal period (two axes: the larger of the two offsets): bin = the number of `touch_edges[s]` (float64 [S, 7], j * mp_half_x / 4) the offset
    reaches, so bins 0 - 3 lie inside the half extent and 4 - 7 beyond it.  `timing`: receives `kernel_ms` and `instance`."""
    cfgs = list(cfgs)
    qa, qb = _table_pair(qa, qb)
    K, n, episodes, max_steps = len(qa), int(envs_per_table), int(episodes), int(max_steps)
    grid_check_args(cfgs, K, n, episodes, max_steps)
    lib = _lib.load()
    by_code, steps_sum, touch_hist, ep_code, ep_steps = grid_buffers(len(cfgs), K, n, episodes, log, touch)
    c = grid_configs_to_c(cfgs)
    _lib.check(lib.dql_score_grid(c, len(cfgs), device, K, n, episodes, int(seed), max_steps, _p(qa), _p(qb), _p(by_code), _p(steps_sum),
                                  None if touch_hist is None else _p(touch_hist), None if ep_code is None else _p(ep_code), None if ep_steps is None else _p(ep_steps)))
    return grid_result(lib, cfgs, by_code, steps_sum, touch_hist, ep_code, ep_steps, timing)


RETURNS_MAX_LOG_WORDS = 1 << 29  # include/dql.h: the decision log is one 64-bit word per possible decision, 4 GiB there


def returns_bound_fx(cfg: DqlConfig, gamma: float, max_steps: int) -> int:
    """ceil(B 2^26), B = R min(1 / (1 - gamma), max_steps + 1) (1 + 2^-10) with R = cfg.max_abs_reward(): no |return-to-go| in fixed point exceeds it"""
    horizon = float(max_steps + 1) if gamma >= 1.0 else min(1.0 / (1.0 - gamma), float(max_steps + 1))
    return math.ceil(cfg.max_abs_reward() * horizon * (1.0 + 2.0 ** -10) * float(1 << TARGET_FRAC_BITS))


def returns_check_args(cfg: DqlConfig, n_tables: int, envs_per_table: int, episodes: int, max_steps: int, eps: float, gamma: float):
    """the argument checks of dql_returns / dql_ensemble_returns, made before the library is touched"""
    if cfg.two_axis:
        raise ValueError("the returns are the x MDP's (the reward is not kept per axis): a two-axis config is refused")
    if not 1 <= n_tables <= SCORE_MAP_MAX_TABLES:
        raise ValueError(f"between 1 and {SCORE_MAP_MAX_TABLES} table sets per returns call, not {n_tables}: slice the sets")
    score_check_args(n_tables, envs_per_table, episodes, max_steps)
    if n_tables * envs_per_table * (max_steps + 1) > RETURNS_MAX_LOG_WORDS:
        raise ValueError(f"table sets x envs x (max_steps + 1) must be at most 2^29 (the decision log: one 64-bit word each), not {n_tables * envs_per_table * (max_steps + 1)}")
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"eps must be in [0, 1], not {eps}")
    if not 0.0 <= gamma <= 1.0:
        raise ValueError(f"gamma must be in [0, 1], not {gamma}")
    bound = returns_bound_fx(cfg, gamma, max_steps)
    if (bound + 1) * envs_per_table * (max_steps + 1) > (1 << 63) - 1:
        raise ValueError(f"{envs_per_table * (max_steps + 1)} returns of up to {bound} * 2^-26 could overflow one int64 cell of return_fx (at most "
                         f"{((1 << 63) - 1) // (bound + 1)} decisions per table set): fly fewer envs per call and add the results of several seeds")


def returns_buffers(n_tables: int):
    """(visits, return_fx, cut_decisions, by_code, steps_sum) as the C calls fill them"""
    return (np.zeros((n_tables, N_CELLS), np.int64), np.zeros((n_tables, N_CELLS), np.int64), np.zeros(n_tables, np.int64),
            np.zeros((n_tables, len(SCORE_COLUMNS)), np.int64), np.zeros(n_tables, np.int64))


def returns_result(lib, visits, return_fx, cut_decisions, by_code, steps_sum, timing):
    _last_call(lib, "returns", "k_returns_fly", timing, times=("fly_ms", "sweep_ms"))
    return {"visits": visits, "return_fx": return_fx, "cut_decisions": cut_decisions, "by_code": by_code, "steps_sum": steps_sum, "columns": SCORE_COLUMNS}


def returns_map(cfg: DqlConfig, qa, qb, envs_per_table: int, seed: int, eps: float, gamma: float, episodes: int = 1, max_steps: int = 600, device: int = 0,
                timing: dict = None):
    """The realised discounted return of every decision, summed per (state, action) cell, under the eps-greedy policy of K table sets (include/dql.h dql_returns,
    DESIGN.md section 21): what `evaluation.value_calibration` holds against the tables' own values.

    `qa`, `qb`: float64 [K, 2835] (one set: [2835]).  The flights are `transition_model`'s.  For every decision of an episode that finished, with cell = state
    before the period * 3 + action, `visits` int64 [K, 2835] gains 1 and `return_fx` int64 [K, 2835] the return-to-go g_t = r_t + gamma g_{t+1} (float64, in
    units of 2^-26, g = 0 after the terminal period) rounded to nearest even.  Decisions of episodes that `max_steps` cut off are counted in `cut_decisions`
    int64 [K] and nowhere else.  `by_code` and `steps_sum` are `score`'s.  Integer sums: bit-reproducible.  `timing`: receives `fly_ms`, `sweep_ms`, `instance`."""
    qa, qb = _table_pair(qa, qb)
    K, n, episodes, max_steps, eps, gamma = len(qa), int(envs_per_table), int(episodes), int(max_steps), float(eps), float(gamma)
    returns_check_args(cfg, K, n, episodes, max_steps, eps, gamma)
    lib = _lib.load()
    visits, return_fx, cut, by_code, steps_sum = returns_buffers(K)
    c = cfg.to_c()
    _lib.check(lib.dql_returns(C.byref(c), device, K, n, episodes, int(seed), max_steps, eps, gamma, _p(qa), _p(qb), _p(visits), _p(return_fx), _p(cut), _p(by_code),
                               _p(steps_sum)))
    return returns_result(lib, visits, return_fx, cut, by_code, steps_sum, timing)
