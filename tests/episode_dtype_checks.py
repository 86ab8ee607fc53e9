"""Whole first episodes in float32 against their float64 twins, decision by decision — one body for two backends: the CPU oracle
(tests/test_episode_dtypes.py) and the HIP engine (tests/test_gpu_episode_dtypes.py, -m gpu).  Float64 is the reference throughout.

tests/f32_step_checks.py compares the dtypes over 16 periods from a state handed over mid-flight, and its G13 flights are scripted.  Here the policy is the
greedy one on the reference's stage-4 tables, so a discrete index that differs becomes an action that differs and feeds back; the same seed gives env i the same
Philox draws in both dtypes, so flight i in float32 and flight i in float64 are a pair from reset to their terminals.  What the landing figures report — how
an episode ends, after how many periods, with which return — is compared across dtypes:

  conditions  decision-discordant envs <= 5 % of n; differing period slots <= 0.5 % of the float64 periods flown
  strict      on every decision-concordant env: terminal code and step count equal, no exception
  continuous  on every decision-concordant env, at the terminal: |float32 - float64| of each record field within BOUNDS[group]
  no bias     among the flights that part, z = 4: McNemar's balance of the landing outcome, paired means of steps and of the cumulative reward;
              among the concordant ones: |mean float32 - float64| of the cumulative reward within CONCORDANT_MEAN_BOUNDS[flavour] (4 x the measured mean)

A decision is the packed word of (idx_x, idx_y, action) `get_fields()` shows after a period, -1 once the env is done; an env is decision-concordant when its
column of the decision matrix is the same in both dtypes, the -1s included: a flight that ends a period earlier than its twin is discordant (a touchdown
within float32's error of a period's last tick does that; DESIGN.md section 30 counts them: 12 near-exceptions in 22 pairs of flights), and the period slots
are counted out of the float64 periods flown after the reset period.  A concordant env has therefore flown the same number of periods in both dtypes, and of
the strict check only the `code` half is independent of concordance (`steps` is asserted all the same: it is the env's own counter).

BOUNDS: 4 x the maxima of the float32 oracle against the float64 flight over every flavour and seed below, rounded up to one significant digit, measured on
the CPU and recorded one line per flavour and seed in profiles/f32_episodes_vs_f64.jsonl (tools/exp_f32_vs_f64.py episodes)."""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np

from dql_multirotor_landing_amd.config import F32, F64, Q_PAPER, Q_REFERENCE, TRAJ_EIGHT, as_launched_config, simulation_config, training_config

import rollout_checks as rc

PROFILE = Path(__file__).resolve().parent.parent / "profiles" / "f32_episodes_vs_f64.jsonl"
N_ENVS, MAX_STEPS, SEEDS = 4096, 600, (123, 7)
MAX_DISCORDANT_ENVS, MAX_DIFFERING_SLOTS, Z = 0.05, 0.005, 4.0
_CONFIGS4 = dict(per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1)
_SIM = dict(working_curriculum_step=4, quirks=Q_PAPER)
# name -> (config builder of the dtype, kind): kind decides the landing outcome and what the float64 flight must contain
FLAVOURS = {
    "sim": (lambda d: simulation_config(dtype=d, **_SIM), "simulation"),
    "sim_two_axis": (lambda d: simulation_config(two_axis=1, dtype=d, **_SIM), "simulation"),
    "sim_configs4": (lambda d: simulation_config(dtype=d, **_SIM, **_CONFIGS4), "simulation"),
    "sim_two_axis_configs4": (lambda d: simulation_config(two_axis=1, dtype=d, **_SIM, **_CONFIGS4), "simulation"),
    "sim_eight": (lambda d: simulation_config(trajectory=TRAJ_EIGHT, dtype=d, **_SIM), "simulation-mixed"),
    "train_l0": (lambda d: training_config(0, quirks=Q_PAPER, dtype=d), "training"),
    "train_l2": (lambda d: training_config(2, quirks=Q_PAPER, dtype=d), "training"),
    "train_l3": (lambda d: training_config(3, quirks=Q_PAPER, dtype=d), "training"),
    "train_l4": (lambda d: training_config(4, quirks=Q_PAPER, dtype=d), "training"),
    "train_l2_reference": (lambda d: training_config(2, quirks=Q_REFERENCE, dtype=d), "training-mixed"),
    "as_launched_l0": (lambda d: as_launched_config(0, dtype=d), "training"),
}
GROUPS = {"position": ("px", "py", "pz"), "velocity": ("vx", "vy", "vz"), "platform": ("mp_x", "mp_u", "mp_y", "mp_v"), "attitude": ("qw", "qx", "qy", "qz"),
          "setpoint": ("pitch_sp", "roll_sp"), "reward": ("reward",), "cum": ("cum_x", "cum_y")}
assert sorted(f for g in GROUPS.values() for f in g) == sorted(rc.RECORD_FIELDS)
# max |float32 - float64| at the terminal of the decision-concordant envs, per field group: 4 x the maximum over the lines of PROFILE, rounded up to one
# significant digit (bounds_from_profile() recomputes them; tests/test_episode_dtypes.py holds this table to the file)
BOUNDS = {"position": 5e-4, "velocity": 8e-5, "platform": 2e-3, "attitude": 5e-6, "setpoint": 2e-8, "reward": 8e-2, "cum": 6e-1}
# (measured: 1.1e-4 m, 2.0e-5 m/s, 5.0e-4 m | m/s — per-env platforms —, 1.1e-6, 4.6e-9 rad, 1.9e-2 and 1.3e-1 — both with observation noise on two axes;
# without noise 1.4e-2 and 8.1e-3)
# |mean over the decision-concordant envs of float32 - float64| of the cumulative reward, per flavour: 4 x the larger of the two seeds' lines of PROFILE (the
# larger of cum_x and cum_y), one significant digit up.  Measured, not derived: see balance().  The paired means of check_balance() leave the concordant pairs
# out, so this table is what holds their share of a return's bias.
CONCORDANT_MEAN_BOUNDS = {"sim": 4e-3, "sim_two_axis": 3e-3, "sim_configs4": 4e-4, "sim_two_axis_configs4": 6e-4, "sim_eight": 2e-3, "train_l0": 2e-3, "train_l2": 4e-3,
                          "train_l3": 2e-3, "train_l4": 2e-3, "train_l2_reference": 1e-3, "as_launched_l0": 5e-4}
# (measured, seed 123 | 7: 8.2e-4 | 7.9e-4, 7.5e-4 | 7.2e-4, 1.6e-5 | 8.5e-5, 1.4e-4 | 8.3e-5, 2.6e-4 | 3.3e-4, 4.5e-4 | 4.4e-4, 8.6e-4 | 8.4e-4, -2.5e-4 | -2.5e-4,
# 2.3e-4 | 2.6e-4, 1.6e-4 | 2.4e-4, -1.2e-4 | -1.2e-4)


def one_digit_up(x):
    """x rounded up to one significant digit"""
    if x == 0.0:
        return 0.0
    e = math.floor(math.log10(x))
    return float(f"{math.ceil(x / 10 ** e - 1e-12) * 10.0 ** e:.1g}")


def bounds_from_profile(path=PROFILE):
    import json
    rows = [json.loads(line) for line in Path(path).read_text().splitlines() if line.strip()]
    return {g: one_digit_up(4.0 * max(r["max_abs_at_terminal"][g] for r in rows)) for g in GROUPS}, rows


def concordant_mean_bounds_from_profile(path=PROFILE):
    _, rows = bounds_from_profile(path)
    return {name: one_digit_up(4.0 * max(abs(v) for r in rows if r["flavour"] == name for v in r["concordant_mean_difference"].values())) for name in FLAVOURS}


def landing_code(kind):
    return rc.CONTACT if kind.startswith("simulation") else rc.SUCCESS


def paired_flights(make_stepper, make_cfg, tables, n=N_ENVS, seed=SEEDS[0], max_steps=MAX_STEPS):
    """The first episodes of the same `n` envs in float32 and in float64, one agent period per call: {F32: flight, F64: flight}, a flight being what
    rollout_checks.stepwise_first_episodes returns with the decision matrix ("decisions", int32 [max_steps + 1][n], -1 once the env is done).
    `make_stepper(cfg, n, seed)`: a fresh Oracle or Engine."""
    out = {}
    for dt in (F32, F64):
        s = make_stepper(make_cfg(dt), n, seed)
        try:
            out[dt] = rc.stepwise_first_episodes(s, tables, max_steps, decisions=True)
            out[dt]["instance"] = s.step_instance() if hasattr(s, "step_instance") else None  # the engine's step-kernel instance
        finally:
            if hasattr(s, "close"):
                s.close()
    return out


def compare(pair):
    """the counts and maxima of one pair of flights (what a line of PROFILE records, and what check() asserts on)"""
    a, b = pair[F32], pair[F64]
    da, db = a["decisions"], b["decisions"]
    differ = da != db
    concordant = ~differ.any(axis=0)
    n = concordant.size
    both = (da >= 0) & (db >= 0)
    strict_bad = concordant & ((a["code"] != b["code"]) | (a["steps"] != b["steps"]))
    ok = concordant & ~strict_bad
    max_abs = {g: float(max(np.abs(a[f] - b[f])[ok].max(initial=0.0) for f in fields)) for g, fields in GROUPS.items()}
    per_field = {f: float(np.abs(a[f] - b[f])[ok].max(initial=0.0)) for f in rc.RECORD_FIELDS}
    conc_mean = {f: (float((a[f] - b[f])[ok].mean()) if ok.any() else 0.0) for f in ("cum_x", "cum_y")}
    return {"n": n, "concordant": concordant, "discordant_envs": int(n - concordant.sum()), "differing_slots": int(differ.sum()), "f64_periods_flown": int((db >= 0).sum()) - n,
            "discordant_while_both_fly": int((both & differ).any(axis=0).sum()), "strict_exceptions": np.flatnonzero(strict_bad), "terminal_code_differs": int((a["code"] != b["code"]).sum()),
            "max_abs_at_terminal": max_abs, "max_abs_per_field": per_field, "concordant_mean_difference": conc_mean}


def return_vs_offset(pair, m, cfg):
    """What the concordant pairs' difference of the return is made of, measured: d = float32 - float64 of cum_x against w_p / p_max times the difference of the
    terminal |mp_x - px| (the position shaping telescopes over an episode, so the return carries the float32 error of the final drone-platform offset, 22 per
    metre) -> mean and sd of d, the correlation of the two and the slope of d on the offset term, over the decision-concordant envs."""
    a, b = pair[F32], pair[F64]
    c = m["concordant"]
    if c.sum() < 3:
        return None
    d = (a["cum_x"] - b["cum_x"])[c]
    t = cfg.w_p / cfg.p_max * (np.abs(a["mp_x"] - a["px"]) - np.abs(b["mp_x"] - b["px"]))[c]
    if d.std() == 0.0 or t.std() == 0.0:
        return None
    return {"mean": float(d.mean()), "sd": float(d.std()), "offset_term_mean": float(t.mean()), "correlation": float(np.corrcoef(d, t)[0, 1]), "slope": float(np.polyfit(t, d, 1)[0])}


def parted_by_outcome(pair):
    """Where no decision matrix exists (one-launch roll-outs): the flights that must have parted — another code, another step count, or a cumulative reward
    further apart than BOUNDS["cum"], which no decision-concordant flight shows.  The selection is symmetric in the dtypes."""
    a, b = pair[F32], pair[F64]
    far = (np.abs(a["cum_x"] - b["cum_x"]) > BOUNDS["cum"]) | (np.abs(a["cum_y"] - b["cum_y"]) > BOUNDS["cum"])
    return (a["code"] != b["code"]) | (a["steps"] != b["steps"]) | far


def balance(pair, kind, two_axis, parted):
    """McNemar's b, c of the landing outcome, and (mean, standard error, flights that parted) of the paired differences d = float32 - float64 of steps and the
    cumulative rewards over all n pairs, with d taken as zero where the flights did not part: |mean d| <= z sd(d) / sqrt(n) is then the self-normalised sum
    over the flights that parted, sqrt(k) mean / rms (at most sqrt(k): it cannot exceed z = 4 while fewer than 16 flights part).
    The concordant pairs are left to an assertion of their own (CONCORDANT_MEAN_BOUNDS) because their d is no sample of a symmetric variable.  Measured
    (PROFILE, "concordant_return_difference_vs_terminal_offset"): without observation noise d of cum_x is w_p / p_max = 22 per metre times the float32 error of
    the final drone-platform offset, correlation 0.99 and slope 0.98 - 0.99 (the position shaping telescopes over the episode); its mean is +4.5e-4 at sd 5.4e-4
    at training level 0 and +8.2e-4 at sd 1.7e-3 in the plain simulation flavour, 52 and 30 standard errors of the concordant flights alone, because the envs
    share one platform and so one platform error.  With noise the reward reads the noisy observation and the correlation drops to 0.33 (as_launched level 0:
    -1.2e-4 at sd 7.5e-4, and, no flight parting at seed 123, 10.35 standard errors of all pairs: "paired_raw", recorded in every line, asserted nowhere)."""
    a, b = pair[F32], pair[F64]
    land = landing_code(kind)
    out = {"landing_f32_only": int(((a["code"] == land) & (b["code"] != land)).sum()), "landing_f64_only": int(((a["code"] != land) & (b["code"] == land)).sum()), "paired": {},
           "paired_raw": {}}
    for f in ("steps", "cum_x") + (("cum_y",) if two_axis else ()):
        d = a[f].astype(np.float64) - b[f].astype(np.float64)
        out["paired_raw"][f] = (float(d.mean()), float(d.std(ddof=1) / math.sqrt(d.size)), int(d.size))
        d = np.where(parted, d, 0.0)
        out["paired"][f] = (float(d.mean()), float(d.std(ddof=1) / math.sqrt(d.size)), int(parted.sum()))
    return out


def check_reference_flight(f64, name, kind):
    """what the case is there for, on the float64 flight alone"""
    h = rc.histogram(f64["code"])
    fly_zone = h["TERMINAL_FLYZONE_X"] + h["TERMINAL_FLYZONE_Y"] + h["TERMINAL_FLYZONE_Z"]
    if kind.startswith("simulation"):
        assert h["TERMINAL_CONTACT"] >= 1000 and h["TERMINAL_MINIMUM_ALTITUDE"] >= 1, f"{name}: {h}"
    if kind.startswith("training"):
        assert h["TERMINAL_SUCCESS"] >= 1 and fly_zone >= 1, f"{name}: {h}"
    if kind.endswith("-mixed"):
        assert sum(1 for k, v in h.items() if v and k != "unfinished") >= 3, f"{name}: {h}"
    return h


def check_balance(bal, what, n):
    b, c = bal["landing_f32_only"], bal["landing_f64_only"]
    assert abs(b - c) <= Z * math.sqrt(b + c), f"{what}: the landing outcome in float32 only {b} times, in float64 only {c} times of {n} pairs: beyond {Z} sqrt(b + c)"
    for f, (mean, se, k) in bal["paired"].items():
        assert abs(mean) <= Z * se, f"{what}: mean paired difference of {f} is {mean:.4g}, {abs(mean) / se:.2f} standard errors ({k} of {n} flights part)"


def check(pair, name, bounds=None, concordant_mean_bounds=None):
    """every assertion of the module's contract on one pair of flights; returns (compare(), balance()) for the record"""
    make_cfg, kind = FLAVOURS[name]
    bounds = BOUNDS if bounds is None else bounds
    check_reference_flight(pair[F64], name, kind)
    m = compare(pair)
    n = m["n"]
    assert m["discordant_envs"] <= MAX_DISCORDANT_ENVS * n, f"{name}: {m['discordant_envs']} of {n} envs differ in a decision"
    assert m["differing_slots"] <= MAX_DIFFERING_SLOTS * m["f64_periods_flown"], f"{name}: {m['differing_slots']} differing period slots of {m['f64_periods_flown']} float64 periods"
    bad = m["strict_exceptions"]
    if bad.size:
        i = int(bad[0])
        a, b = pair[F32], pair[F64]
        raise AssertionError(f"{name}: {bad.size} envs agree in every decision and differ at the terminal; first env {i}: float32 code {a['code'][i]} after {a['steps'][i]} steps, "
                             f"float64 code {b['code'][i]} after {b['steps'][i]}")
    for g, worst in m["max_abs_at_terminal"].items():
        assert worst <= bounds[g], f"{name}: {g} differs by {worst:.3g} > {bounds[g]:.3g} at the terminal of a decision-concordant env ({m['max_abs_per_field']})"
    for f, mean in m["concordant_mean_difference"].items():
        lim = (CONCORDANT_MEAN_BOUNDS if concordant_mean_bounds is None else concordant_mean_bounds)[name]
        assert abs(mean) <= lim, f"{name}: the decision-concordant envs' mean difference of {f} is {mean:.3g}, beyond {lim:.3g}"
    bal = balance(pair, kind, make_cfg(F64).two_axis, ~m["concordant"])
    check_balance(bal, name, n)
    return m, bal


def check_rollouts(r32, r64, name):
    """One launch per dtype, a larger sample (rows of ops.rollout's table set 0): terminal codes differ in <= 5 % of the envs, and the balance checks"""
    make_cfg, kind = FLAVOURS[name]
    pair = {F32: r32, F64: r64}
    check_reference_flight(r64, name, kind)
    n = r64["code"].size
    differs = int((r32["code"] != r64["code"]).sum())
    assert differs <= MAX_DISCORDANT_ENVS * n, f"{name}: the terminal code differs in {differs} of {n} envs"
    bal = balance(pair, kind, make_cfg(F64).two_axis, parted_by_outcome(pair))
    check_balance(bal, f"{name} (roll-out)", n)
    return differs, bal
