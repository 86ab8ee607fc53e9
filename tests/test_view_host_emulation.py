"""The view kernel's per-env body (csrc/dql_view.hpp) run on the CPU and held to numpy on the same arrays with == (CPU only, no GPU).

tests/host_emu/view_emu.cpp compiles the real device header as host C++ and calls the real `env_view` for every lane of k_env_view's grid, the tail workgroup's
lanes beyond the batch included.  The state is synthetic: Quad<T>[16][n] and int4[n] of random bits with the awkward values planted where the view reads — NaN
payloads (quiet and signalling), infinities, denormals, -0.0, doubles that round up, round down, tie to even, overflow to infinity and land on float32 denormals
when cast — step_count words with their high half set, and every combination of the flag byte.  State and outputs are reached through checked references
exactly as long as the library's buffers (exit status 3 outside them), every output is poisoned before the launch, and the whole of every buffer comes back:
  * every output asked for == numpy's, floats by their bits (the cast contract is numpy's astype: the same type keeps the bits, float -> double is exact,
    double -> float is one round-to-nearest-even conversion);
  * every output not asked for (a NULL pointer of dql_view) is still poison;
  * nothing beyond n can have been written: the references end there.
Built twice: plain, and with ASan + UBSan as a stand-alone program (any report fails)."""
import struct

import numpy as np
import pytest

import host_emu_harness as heh

emu = heh.emu_fixture("view_emu")

POISON = 0xA5
F32, F64 = 0, 1
REAL = {F32: (np.float32, np.uint32), F64: (np.float64, np.uint64)}
OUTPUTS = ("obs", "reward", "cumulative_reward", "idx_x", "idx_y", "step_count", "done", "was_reset", "code", "bad_actions")  # dql_view's pointers, mask bit by position
ALL = (1 << len(OUTPUTS)) - 1
FL_DONE, FL_WAS_RESET = 1, 8  # dql_device.hpp
SIZES = (1, 63, 64, 65, 257, 777)
DTYPES = [(t, r) for t in (F32, F64) for r in (F32, F64)]
DTYPE_IDS = [f"{'f32' if t == F32 else 'f64'}-to-{'f32' if r == F32 else 'f64'}" for t, r in DTYPES]


def mask_of(*names):
    return sum(1 << OUTPUTS.index(k) for k in names)


def awkward(dtype):
    """bit patterns of `dtype` worth reading through the view"""
    if dtype == F32:
        return np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0xff8abcde,  # quiet and signalling NaNs with payloads
                         0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x00400000,   # infinities, denormals
                         0x80000000, 0x00000000, 0x7f7fffff, 0x00800000, 0x3f800001], np.uint32)
    f = lambda x: np.array([x], np.float64).view(np.uint64)[0]
    vals = [0x7ff8000000000000, 0x7ff8000012345678, 0xfff8000000000001, 0x7ff0000000000001, 0xfff000000abcdef0, 0x7ff4000000000000,  # NaNs; payload in low and high bits
            0x7ff0000000000000, 0xfff0000000000000, 0x0000000000000001, 0x800fffffffffffff,  # infinities, denormals
            0x8000000000000000, 0x0000000000000000,
            f(1.0 + 2.0**-24 + 2.0**-50), f(1.0 + 2.0**-24 - 2.0**-50),   # just above / below the midpoint of two floats: up / down
            f(1.0 + 2.0**-24), f(1.0 + 3 * 2.0**-24),                    # ties: to even = down / up
            f(-(1.0 + 2.0**-24 + 2.0**-50)), f(-(1.0 + 2.0**-23 - 2.0**-50)),
            f(1e39), f(-1e39), f(3.4028235677973366e38),                  # beyond float32: infinity; the midpoint above FLT_MAX ties to infinity
            f(1e-40), f(-1.4e-45), f(0.7e-45), f(0.71e-45), f(1e-60)]     # float32 denormals, the smallest one's midpoint, and underflow to zero
    return np.array(vals, np.uint64)


def synthetic_state(n, t, seed):
    """(sr uint bits [16, n, 4], si int32 [n, 4], bad) — random bits, with the awkward patterns planted in the quads the view reads"""
    rng = np.random.default_rng(seed)
    _, u = REAL[t]
    sr = rng.integers(0, np.iinfo(u).max, (16, n, 4), dtype=u, endpoint=True)
    aw = awkward(t)
    read = [(14, 0), (14, 1), (14, 2), (14, 3), (7, 3), (15, 0), (15, 1), (15, 2), (10, 1), (10, 2)]
    for j, (q, k) in enumerate(read):  # every read component meets every pattern once n is large enough; env 0 always gets one
        where = np.arange(0, n, 2)
        sr[q, where, k] = aw[(where // 2 + j) % len(aw)]
    si = rng.integers(-2**31, 2**31 - 1, (n, 4), dtype=np.int64, endpoint=True).astype(np.int32)
    i = np.arange(n)
    flags = (i + (FL_DONE | FL_WAS_RESET)) & 0xff  # every value of the flag byte once n >= 256; env 0: done and was_reset, nothing else
    code = (i * 7 + 250) & 0xff                    # codes above 127 included (int8 wraps)
    si[:, 3] = ((si[:, 3].astype(np.int64) & 0xffff0000) | (flags << 8) | code).astype(np.uint32).view(np.int32)
    si[:, 2] = (si[:, 2].astype(np.int64) | 0x80010000).astype(np.uint32).view(np.int32)  # the high half of the step_count word is never empty
    bad = int(rng.integers(1, 2**63))
    return sr, si, bad


def numpy_view(sr, si, bad, t, r):
    """what the view must write, from the same arrays (knows nothing of the header)"""
    ft, _ = REAL[t]
    fr, ur = REAL[r]
    x = sr.view(ft)
    with np.errstate(all="ignore"):
        obs = np.stack([x[14, :, 1], x[14, :, 2], x[14, :, 3], x[7, :, 3], x[15, :, 0], x[15, :, 1], x[15, :, 2], x[10, :, 2]], axis=1).astype(fr)
        reward, cum = x[14, :, 0].astype(fr), x[10, :, 1].astype(fr)
    fl = (si[:, 3] >> 8) & 0xff
    return {"obs": np.ascontiguousarray(obs).view(ur), "reward": np.ascontiguousarray(reward).view(ur), "cumulative_reward": np.ascontiguousarray(cum).view(ur),
            "idx_x": si[:, 0].copy(), "idx_y": si[:, 1].copy(), "step_count": si[:, 2] & 0xffff,
            "done": ((fl & FL_DONE) != 0).astype(np.uint8), "was_reset": ((fl & FL_WAS_RESET) != 0).astype(np.uint8),
            "code": (si[:, 3] & 0xff).astype(np.uint8).view(np.int8), "bad_actions": np.array([bad], np.uint64)}


def run_emu(exe, sr, si, bad, n, t, r, mask, tmp, sanitized=False):
    _, ur = REAL[r]
    job = struct.pack("<4i", t, r, mask, 0) + struct.pack("<q", n) + sr.tobytes() + si.tobytes() + struct.pack("<Q", bad)
    rd = heh.Reader(heh.run(exe, job, tmp, "view", sanitized, timeout=120, what=f"n {n}, mask {mask:#x}"))
    out = {"obs": rd.take(ur, (n, 8)), "reward": rd.take(ur, (n,)), "cumulative_reward": rd.take(ur, (n,)), "idx_x": rd.take(np.int32, (n,)), "idx_y": rd.take(np.int32, (n,)),
           "step_count": rd.take(np.int32, (n,)), "done": rd.take(np.uint8, (n,)), "was_reset": rd.take(np.uint8, (n,)), "code": rd.take(np.int8, (n,)),
           "bad_actions": rd.take(np.uint64, (1,))}
    rd.done()
    return out


def check(exe, n, t, r, mask, tmp, sanitized=False):
    sr, si, bad = synthetic_state(n, t, seed=1000 * n + 10 * t + r)
    want = numpy_view(sr, si, bad, t, r)
    got = run_emu(exe, sr, si, bad, n, t, r, mask, tmp, sanitized)
    for b, k in enumerate(OUTPUTS):
        if mask >> b & 1:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{k} differs at {np.argwhere(got[k] != want[k])[:5].tolist()} (n {n}, mask {mask:#x})"
        else:
            assert (np.frombuffer(got[k].tobytes(), np.uint8) == POISON).all(), f"{k} was not asked for and was written (n {n}, mask {mask:#x})"
    return want


@pytest.mark.parametrize("t,r", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_every_output_equals_numpy_on_the_same_arrays(emu, n, t, r, tmp_path):
    want = check(emu["plain"], n, t, r, ALL, tmp_path)
    if n >= 256:  # the events the synthetic state is there for (asserted on the yardstick)
        assert {(int(d), int(w)) for d, w in zip(want["done"], want["was_reset"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert (want["code"] < 0).any() and (want["step_count"] >= 0).all() and (want["step_count"] > 0x7fff).any()
        if t == F64 and r == F32:  # the cast rounded both ways: some results lie above, some below the double they came from
            sr, _, _ = synthetic_state(n, t, seed=1000 * n + 10 * t + r)
            src, dst = sr.view(np.float64)[14, :, 1], want["obs"].view(np.float32)[:, 0].astype(np.float64)
            fin = np.isfinite(src) & np.isfinite(dst)
            assert (dst[fin] > src[fin]).any() and (dst[fin] < src[fin]).any()


@pytest.mark.parametrize("t,r", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_view_clean_under_asan_and_ubsan(emu, n, t, r, tmp_path):
    """every shape through the ASan + UBSan build: no report, and still numpy's result"""
    check(emu["san"], n, t, r, ALL, tmp_path, sanitized=True)


SUBSETS = {"none": 0, "obs": mask_of("obs"), "done": mask_of("done"), "cum": mask_of("cumulative_reward"), "reward": mask_of("reward"),
           "mixed": mask_of("reward", "idx_y", "code", "bad_actions"), "no-bad": ALL & ~mask_of("bad_actions")}


@pytest.mark.parametrize("t,r", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("subset", SUBSETS)
def test_outputs_not_asked_for_stay_poisoned(emu, subset, t, r, tmp_path):
    """a subset of the outputs (the others are null references, as NULL pointers are): those asked for are right, the others untouched; plain and sanitized"""
    check(emu["plain"], 257, t, r, SUBSETS[subset], tmp_path)
    check(emu["san"], 257, t, r, SUBSETS[subset], tmp_path, sanitized=True)
