"""The step kernel's device code (csrc/dql_device.hpp) run on the CPU and held bit for bit to the oracle (CPU only, no GPU).

tests/host_emu/step_emu.cpp compiles the real device header as host C++ (against a stand-in runtime header that gives the gfx950-only
inline-asm macros their portable meaning; the kernel source has no build switch for it) and
emulates one launch of k_step lane by lane: the clamped acting-table row, load_env, P x agent_period<TICK, XMODE>, the un-staged
accumulation, store_env.  Every table read and every accumulator target is index-checked.  It is built twice: plain (bit-exact runs)
and with ASan + UBSan (the same kind of runs, smaller; any report fails); building, running a job and reading the result file are
tests/host_emu_harness.py's, shared with the other four emulation modules.  The GPU tests run this source only on the device, where an
out-of-range index either faults the card or silently moves counts, and the oracle is a separate restatement that cannot see an
addressing bug in the device header; this module closes that gap for every instance the source defines, the parked
k_step<float, *, TICK_PACKED_LITM, X_TWO> included.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_PAPER, TRAJ_EIGHT, DqlConfig
from oracle.oracle import Oracle

import host_emu_harness as heh
from host_emu_harness import NF_INT, NF_REAL, ROOT, SAN_ENV

GOLDEN = ROOT / "tests" / "golden" / "assets"

TICK_PLAIN, TICK_PACKED, TICK_LIT, TICK_PACKED_LITM = 0, 2, 3, 4  # dql_device.hpp
X_TWO, X_ONLY, X_RUNTIME = 0, 1, 2
MODE_TRAIN, MODE_EVAL, MODE_EXTERNAL = 0, 1, 2

emu = heh.emu_fixture("step_emu")


# ---------------------------------------------------------------------------------------------------------------------
# one launch through the emulator
# ---------------------------------------------------------------------------------------------------------------------
def _job_bytes(cfg, tick, xmode, snap):
    c = bytes(cfg.to_c())
    n = snap["ints"].shape[1]
    acts = snap.get("actions")
    hdr = struct.pack("<8i", len(c), cfg.dtype, tick, xmode, snap["mode"], snap["P"], int(acts is not None), 0)
    hdr += struct.pack("<4q", n, 0, snap["step_index"], snap["seed"]) + struct.pack("<d", snap["eps"])
    parts = [hdr, c, np.ascontiguousarray(snap["reals"], np.float64).tobytes(), np.ascontiguousarray(snap["ints"], np.int32).tobytes(),
             np.ascontiguousarray(snap["qa"], np.float64).tobytes(), np.ascontiguousarray(snap["qb"], np.float64).tobytes()]
    if acts is not None:
        parts.append(np.ascontiguousarray(acts, np.uint8).tobytes())
    return b"".join(parts)


def run_emu(exe, cfg, tick, xmode, snap, tmp, sanitized=False):
    """(reals, ints, acc [4 N_CELLS] int64, stats [12] int64, bad_actions): what one launch leaves behind"""
    what = f"tick {tick} xmode {xmode} mode {snap['mode']} P {snap['P']}"
    r = heh.Reader(heh.run(exe, _job_bytes(cfg, tick, xmode, snap), tmp, f"step_{tick}_{xmode}", sanitized, timeout=600, what=what))
    n = snap["ints"].shape[1]
    got = r.take(np.float64, (NF_REAL, n)), r.take(np.int32, (NF_INT, n)), r.take(np.int64, (4 * N_CELLS,)), r.take(np.int64, (12,)), int(r.take(np.int64, (1,))[0])
    r.done()
    return got


def admits(exe, cfg, tmp):
    """(refm, lit_ok) of the library's create_impl for this config: may TICK_PACKED_LITM / TICK_LIT serve it"""
    snap = dict(reals=np.zeros((NF_REAL, 1)), ints=np.zeros((NF_INT, 1), np.int32), qa=np.zeros(N_CELLS), qb=np.zeros(N_CELLS),
                mode=1, P=1, step_index=0, seed=0, eps=0.0)
    job = tmp / "admits.bin"
    job.write_bytes(_job_bytes(cfg, 0, 0, snap))
    r = subprocess.run([str(exe), "--admits", str(job)], capture_output=True, text=True, check=True)
    refm, lit = map(int, r.stdout.split())
    return bool(refm), bool(lit)


def instances(cfg, refm, lit_ok):
    """every (TICK, XMODE) the source defines that can fly this config: the host's auto choices and the run-time-axis forms.  The
    literal-table ticks only where dql_create would allow them; X_ONLY / X_TWO only for the axis count they are compiled for."""
    xs = [X_RUNTIME, X_TWO if cfg.two_axis else X_ONLY]
    if cfg.dtype == F64:
        return [(TICK_PLAIN, x) for x in xs]
    ticks = [TICK_PLAIN, TICK_PACKED] + ([TICK_LIT] if lit_ok else []) + ([TICK_PACKED_LITM] if refm else [])
    return [(t, x) for t in ticks for x in xs]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's launches, recorded
# ---------------------------------------------------------------------------------------------------------------------
def implied_bad_actions(cfg, mode, P, actions):
    """the action codes k_step counts as bad (StatsDev::bad_actions), from the job's actions alone: once per env and period of an external-action launch"""
    if mode != MODE_EXTERNAL:
        return 0
    a = np.asarray(actions, np.int64)
    ax, ay = a & 3, (a >> 2) & 3
    bad = (ax > 2) | (ay > 2) | ((a >> 4) != 0)
    if not cfg.two_axis:
        bad |= (ay != 0) & (ay != 2)
    return P * int(bad.sum())


def oracle_launch(orc, mode, eps=0.0, P=1, actions=None):
    """one launch of P periods on the oracle: its input (state, acting tables, step index) and what it computed"""
    reals, ints = orc.get_fields()
    snap = dict(reals=reals, ints=ints, qa=orc.qa_act.copy(), qb=orc.qb_act.copy(), step_index=orc.step_index, seed=orc.seed,
                mode=mode, eps=float(eps), P=P, actions=actions)
    st0 = orc.stats.copy()
    orc._period(mode, eps, actions, n_periods=P)
    o_r, o_i = orc.get_fields()
    acc = orc.pending.copy() if mode == MODE_TRAIN else np.zeros(4 * N_CELLS, np.int64)
    snap["out"] = (o_r, o_i, acc, orc.stats - st0)
    snap["bad_actions"] = implied_bad_actions(orc.cfg, mode, P, actions)
    assert snap["bad_actions"] == 0, "ext_actions and the soak draws make valid action codes only"
    return snap


def assert_launch_equal(got, snap, what):
    g_r, g_i, g_acc, g_st, g_bad = got
    o_r, o_i, o_acc, o_st = snap["out"]
    bad_i = [f for f in range(NF_INT) if not np.array_equal(g_i[f], o_i[f])]
    assert not bad_i, f"{what}: int fields {bad_i} differ from the oracle"
    # bitwise, NaN payloads and signed zeros included
    bad_r = [f for f in range(NF_REAL) if not np.array_equal(g_r[f].view(np.uint64), o_r[f].view(np.uint64))]
    assert not bad_r, f"{what}: real fields {bad_r} differ from the oracle"
    assert np.array_equal(g_acc, o_acc), f"{what}: accumulators differ in {np.count_nonzero(g_acc != o_acc)} entries"
    assert np.array_equal(g_st, o_st), f"{what}: statistics {g_st.tolist()} vs oracle {o_st.tolist()}"
    assert g_bad == snap["bad_actions"], f"{what}: {g_bad} bad action codes counted, the job's actions imply {snap['bad_actions']}"


def flown_oracle(cfg, n, seed, warm=40):
    orc = Oracle(cfg, n, seed=seed)
    qa, qb, cnt = (np.load(GOLDEN / f) for f in ("Q_table_a.npy", "Q_table_b.npy", "state_action_count.npy"))
    orc.set_tables(qa, qb, cnt)  # the reference's stage-4 tables: greedy actions and bootstraps are non-trivial
    orc.train_steps(warm, 0.2)
    return orc


def ext_actions(rng, cfg, n):
    a = rng.integers(0, 3, size=n).astype(np.uint8)
    if cfg.two_axis:
        a |= (rng.integers(0, 3, size=n) << 2).astype(np.uint8)
    return a


def recorded_launches(cfg, n, seed, periods=(1, 16)):
    """train (eps 0.2), eval and external-action launches of 1 and 16 periods from a flown state, as the oracle computes them"""
    orc = flown_oracle(cfg, n, seed)
    rng = np.random.default_rng(seed)
    snaps = []
    for P in periods:
        snaps.append(oracle_launch(orc, MODE_TRAIN, 0.2, P))
        snaps.append(oracle_launch(orc, MODE_EVAL, 0.0, P))
        snaps.append(oracle_launch(orc, MODE_EXTERNAL, 0.0, 1, ext_actions(rng, cfg, n)))
        snaps.append(oracle_launch(orc, MODE_TRAIN, 0.2, P))  # a launch that acts on tables the previous training launch folded into
    return snaps


# the configs of tests/test_gpu_parity.py::test_config_variants_bit_exact (block sizes do not exist here), the reference MDP in two axes,
# and float64
CONFIGS = [
    dict(), dict(working_curriculum_step=2), dict(working_curriculum_step=4, init_uniform=1, vz_setpoint=-0.4),
    dict(quirks=Q_PAPER), dict(trajectory=TRAJ_EIGHT), dict(per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1),
    dict(two_axis=1), dict(two_axis=1, working_curriculum_step=3, init_uniform=1), dict(two_axis=1, quirks=Q_PAPER, trajectory=TRAJ_EIGHT),
    dict(two_axis=1, goal_logic=0, vz_setpoint=-0.4, working_curriculum_step=4, init_uniform=1),
    dict(two_axis=1, per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1, t_max=4.0),
    dict(p_max=4.0, init_sigma=4.0 / 3), dict(f_ag=20.0, working_curriculum_step=1), dict(p_max=5.0, init_sigma=5.0 / 3, two_axis=1),
    dict(dtype=F64), dict(dtype=F64, two_axis=1, working_curriculum_step=3, init_uniform=1), dict(dtype=F64, quirks=Q_PAPER, trajectory=TRAJ_EIGHT),
]


def _cfg(kw):
    kw = dict(kw)
    return DqlConfig(**{"dtype": F32, **kw})


@pytest.mark.parametrize("kw", CONFIGS, ids=lambda kw: ",".join(f"{k}={v:g}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()) or "default")
def test_every_instance_bit_exact_vs_oracle(emu, kw, tmp_path):
    """Every (TICK, XMODE) instance that can fly the config — float32 PLAIN / PACKED / LIT / PACKED_LITM in the run-time-axis and the
    compiled-axis form, float64 PLAIN — computes the oracle's launch bit for bit: every real and int field, the accumulators (sums and
    visits of both tables), the statistics.  1 and 16 periods per launch, train / eval / external actions, episodes ending inside."""
    cfg = _cfg(kw)
    refm, lit_ok = admits(emu["plain"], cfg, tmp_path)
    insts = instances(cfg, refm, lit_ok)
    if cfg.dtype == F32 and not cfg.two_axis and "p_max" not in kw and "f_ag" not in kw:
        assert refm, "the reference MDP must admit the literal-table instances"
    if cfg.dtype == F32 and cfg.two_axis and refm:
        assert (TICK_PACKED_LITM, X_TWO) in insts  # the parked instance
    n = 96
    snaps = recorded_launches(cfg, n, seed=11)
    assert sum(int(s["out"][3][1]) for s in snaps) > 0, "no episode ended: the case would not reach resets"
    for tick, xmode in insts:
        for k, s in enumerate(snaps):
            got = run_emu(emu["plain"], cfg, tick, xmode, s, tmp_path)
            assert_launch_equal(got, s, f"{kw} tick {tick} xmode {xmode} launch {k} (mode {s['mode']}, P {s['P']})")


SAN_CONFIGS = [dict(), dict(two_axis=1), dict(two_axis=1, quirks=Q_PAPER, trajectory=TRAJ_EIGHT, per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1),
               dict(working_curriculum_step=4, init_uniform=1, quirks=Q_PAPER), dict(p_max=5.0, init_sigma=5.0 / 3, two_axis=1),
               dict(dtype=F64, two_axis=1)]


@pytest.mark.parametrize("kw", SAN_CONFIGS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "default")
def test_every_instance_clean_under_asan_and_ubsan(emu, kw, tmp_path):
    """The same launches, smaller, through the ASan + UBSan build: no report, and still the oracle's bits."""
    cfg = _cfg(kw)
    refm, lit_ok = admits(emu["plain"], cfg, tmp_path)
    snaps = recorded_launches(cfg, 24, seed=5, periods=(16,))
    for tick, xmode in instances(cfg, refm, lit_ok):
        for k, s in enumerate(snaps):
            got = run_emu(emu["san"], cfg, tick, xmode, s, tmp_path, sanitized=True)
            assert_launch_equal(got, s, f"sanitized {kw} tick {tick} xmode {xmode} launch {k}")


def test_sanitized_build_reports_a_heap_overread(emu):
    """The sanitized binary really is instrumented: one read past a heap array is reported and ends the run."""
    r = subprocess.run([str(emu["san"]), "--asan-selftest"], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV), timeout=120)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-3000:]
    r = subprocess.run([str(emu["plain"]), "--asan-selftest"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0  # (the plain build reads the byte and carries on: it is the sanitizer that reports)


# ---------------------------------------------------------------------------------------------------------------------
# round 5's evidence against k_step<float, *, TICK_PACKED_LITM, X_TWO>, replayed on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def _conservation(cfg, n, seed, launches, tmp, exe, insts):
    """train launches (eps 1.0, 1 period each) of tests/test_gpu_fullsize.py::test_two_axis_conservation_65536's config: every instance
    bit-exact with the oracle, and every launch's visits = (1 + two_axis) x its decisions"""
    orc = Oracle(cfg, n, seed=seed)
    fly_y = 0
    for j in range(launches):
        s = oracle_launch(orc, MODE_TRAIN, 1.0, 1)
        fly_y += int(s["out"][3][2 + 3])  # by_code[TERMINAL_FLYZONE_Y]
        for tick, xmode in insts:
            got = run_emu(exe, cfg, tick, xmode, s, tmp)
            assert_launch_equal(got, s, f"launch {j} tick {tick} xmode {xmode}")
            acc, st = got[2], got[3]
            visits = acc[N_CELLS:2 * N_CELLS].sum() + acc[3 * N_CELLS:].sum()
            assert visits == (1 + cfg.two_axis) * st[0], f"launch {j} tick {tick} xmode {xmode}: {visits} visits for {st[0]} decisions"
    return fly_y


def test_two_axis_conservation_replayed_on_the_parked_instance(emu, tmp_path):
    """tests/test_gpu_fullsize.py::test_two_axis_conservation_65536 (seed 7, eps 1.0, 40 launches), scaled to 4 096 envs: the parked
    instance and its neighbours visit exactly 2 x decisions cells and match the oracle in every launch"""
    cfg = DqlConfig(dtype=F32, two_axis=1)
    insts = [(TICK_PACKED_LITM, X_TWO), (TICK_PACKED, X_TWO), (TICK_LIT, X_TWO), (TICK_PLAIN, X_RUNTIME)]
    assert _conservation(cfg, 4096, 7, 40, tmp_path, emu["plain"], insts) > 0  # the y fly-zone is reached, as on the GPU


def soak_draws(count=30, seed=0):
    """the parameters tests/soak_parity.py draws for its configs 0 .. count-1 (seed 0: draw 21 faulted in round 5), re-derived with the
    same generator calls in the same order (its chunk loop included, assuming every chunk matched)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        kw = dict(dtype=int(rng.choice([F32, F32, F64])), working_curriculum_step=int(rng.integers(0, 5)), quirks=int(rng.choice([0x7F, 0x00, 0x40, 0x77, 0x60, int(rng.integers(0, 128))])),
                  two_axis=int(rng.random() < 0.3), fold_per_step=int(rng.random() < 0.2), t_max=float(rng.choice([20.0, 4.0, 2.0])))
        if rng.random() < 0.3: kw["trajectory"] = TRAJ_EIGHT
        if rng.random() < 0.3: kw.update(per_env_platform=1)
        if rng.random() < 0.3: kw.update(noise_pos_sd=0.25, noise_vel_sd=0.1)
        if rng.random() < 0.3: kw.update(init_uniform=1)
        n = int(rng.choice([1, 63, 64, 65, 200, 512, 700, 3000]))
        run_seed = int(rng.integers(0, 2**31))
        windowed = rng.random() < 0.3
        block = int(rng.choice([0, 0, 64, 128, 256, 512])) if kw["dtype"] == F32 else int(rng.choice([0, 0, 64, 128, 256]))
        tick = int(rng.choice([0, 1, 3, 4])) if kw["dtype"] == F32 else int(rng.choice([0, 1, 3]))
        ppl = int(rng.choice([1, 1, 2, 3, 4, 8, 13, 16, 24, 32]))
        rng.integers(-1, 2)  # fair_prio (scheduling only)
        chunks = []
        for _c in range(6):
            steps, eps = int(rng.integers(1, 60)), float(rng.choice([1.0, 0.5, 0.05, 0.0]))
            mode = rng.random()
            if mode < 0.75:
                chunks.append((MODE_TRAIN, steps, eps))
            elif mode < 0.9:
                chunks.append((MODE_EVAL, steps, 0.0))
            else:
                act = rng.integers(0, 3, size=n).astype(np.uint8)
                if kw["two_axis"]:
                    act = (act | (rng.integers(0, 3, size=n).astype(np.uint8) << 2)).astype(np.uint8)
                chunks.append((MODE_EXTERNAL, 1, act))
            if windowed:
                rng.random()
        out.append(dict(kw=kw, n=n, seed=run_seed, block=block, tick=tick, ppl=ppl, chunks=chunks))
    return out


def host_instance(dtype, n, block, tick, lit_ok, litm_ok, two):
    """the (TICK, XMODE) dql_hip.hip's launch_step_b / launch_step_t pick for options block / tick (0 = auto)"""
    if dtype == F64:
        return TICK_PLAIN, X_RUNTIME
    if block == 0:
        block = 64 if n <= 8192 else (256 if (n <= 196608 or tick == 3) else 512)
    if tick == 0:
        tick = 3 if n <= 65536 else (4 if lit_ok else 1)
    if tick == 4 and not lit_ok:
        tick = 1
    if block == 128 or (block == 512 and tick != 4):
        tick = 1
    if tick == 4:
        return TICK_LIT, X_TWO if two else X_ONLY
    if block in (128, 512) or tick != 3:
        return TICK_PLAIN, X_RUNTIME
    if litm_ok:
        return TICK_PACKED_LITM, X_ONLY
    return TICK_PACKED, X_TWO if two else X_ONLY


def test_soak_draws_0_to_29_replayed_on_the_cpu(emu, tmp_path):
    """tests/soak_parity.py's seeded draws 0 - 29, scaled down (at most 256 envs, 12 periods per chunk): the instance the host picked for each,
    and for two-axis configs on the reference MDP the parked TICK_PACKED_LITM / X_TWO as well, bit-exact with the oracle launch by launch,
    with (1 + two_axis) x decisions visits in every training launch"""
    draws = soak_draws()
    assert draws[21]["kw"]["dtype"] == F32  # (the draw that faulted; its parameters must come out of the generator as they did on the GPU)
    parked = 0
    for k, d in enumerate(draws):
        cfg = DqlConfig(**d["kw"])
        refm, lit_ok = admits(emu["plain"], cfg, tmp_path)
        insts = [host_instance(cfg.dtype, d["n"], d["block"], d["tick"], lit_ok, refm and not cfg.two_axis, cfg.two_axis)]
        if cfg.dtype == F32 and cfg.two_axis and refm:
            insts.append((TICK_PACKED_LITM, X_TWO)); parked += 1
        n = min(d["n"], 256)
        orc = Oracle(cfg, n, seed=d["seed"])
        P = d["ppl"]
        for c, (mode, steps, arg) in enumerate(d["chunks"]):
            left = min(steps, 12)
            while left > 0:
                p = min(left, P)
                if mode == MODE_EXTERNAL:
                    s = oracle_launch(orc, mode, 0.0, 1, arg[:n].copy())
                else:
                    s = oracle_launch(orc, mode, arg, p)
                left -= s["P"]
                for tick, xmode in insts:
                    got = run_emu(emu["plain"], cfg, tick, xmode, s, tmp_path)
                    assert_launch_equal(got, s, f"soak draw {k} chunk {c} tick {tick} xmode {xmode}")
                    if mode == MODE_TRAIN:
                        acc, st = got[2], got[3]
                        assert acc[N_CELLS:2 * N_CELLS].sum() + acc[3 * N_CELLS:].sum() == (1 + cfg.two_axis) * st[0], f"soak draw {k} chunk {c}"
    assert parked > 0
