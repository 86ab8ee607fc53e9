"""Device-resident step outputs on the GPU (run with -m gpu on an MI355X): dql_view_dev / dql_reset_dev against the host path they stand beside.

Two engines of equal seed fly the same seeded random actions: A through the host (`step` + `step_outputs()` + `obs()` + `get_fields()`), B through the device
(`step_dev` + `view_dev` into buffers this file allocates).  After every period every output of B == A's, floats by their bits; the cast contract is numpy's
astype on the host's doubles (the same type keeps the bits, float -> double is exact, double -> float is one round-to-nearest-even conversion).
The file is torch-free: device memory comes from hipMalloc / hipMemcpy of the HIP runtime the library itself runs on."""
import ctypes as C

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib
from dql_multirotor_landing_amd.config import DqlConfig, F32, F64

pytestmark = pytest.mark.gpu

POISON = 0xA5
H2D, D2H = 1, 2  # hipMemcpyKind
NP_REAL = {F32: (np.float32, np.uint32), F64: (np.float64, np.uint64)}
OUTPUTS = _lib.VIEW_POINTERS
OBS_FIELDS = ("obs_p_x", "obs_v_x", "obs_a_x", "pitch_sp", "obs_p_y", "obs_v_y", "obs_a_y", "roll_sp")


class Dev:
    """device memory through the runtime libdql_hip.so is linked to (symbol lookup through the library's handle searches its dependencies)"""

    def __init__(self):
        self.hip = C.CDLL(str(_lib.LIB_PATH))
        self.ptrs = []

    def alloc(self, nbytes, fill=POISON):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        self.ptrs.append(p)
        assert self.hip.hipMemset(p, C.c_int(fill), C.c_size_t(nbytes)) == 0
        assert self.hip.hipDeviceSynchronize() == 0
        return p.value

    def up(self, ptr, a):
        a = np.ascontiguousarray(a)
        assert self.hip.hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), H2D) == 0

    def down(self, ptr, dtype, shape):
        a = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(a.nbytes), D2H) == 0
        return a

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.free()


class ViewBufs:
    """one buffer per output of dql_view, all allocated and poisoned; `which` are handed to view_dev, the others must keep their poison"""

    def __init__(self, dev, n, real_dtype, which=OUTPUTS):
        fr, ur = NP_REAL[real_dtype]
        self.dev, self.n, self.real_dtype, self.which = dev, n, real_dtype, tuple(which)
        self.spec = {"obs": (ur, (n, 8)), "reward": (ur, (n,)), "cumulative_reward": (ur, (n,)), "idx_x": (np.int32, (n,)), "idx_y": (np.int32, (n,)),
                     "step_count": (np.int32, (n,)), "done": (np.uint8, (n,)), "was_reset": (np.uint8, (n,)), "code": (np.int8, (n,)), "bad_actions": (np.uint64, (1,))}
        self.ptr = {k: dev.alloc(int(np.prod(s)) * np.dtype(d).itemsize) for k, (d, s) in self.spec.items()}

    def view(self, eng):
        eng.view_dev(real_dtype=self.real_dtype, **{k: self.ptr[k] for k in self.which})

    def read(self, eng):
        eng.sync()
        return {k: self.dev.down(self.ptr[k], d, s) for k, (d, s) in self.spec.items()}

    def poisoned(self, got, k):
        return bool((np.frombuffer(got[k].tobytes(), np.uint8) == POISON).all())


def host_outputs(eng, real_dtype):
    """engine A's side: what the view must hold, from step_outputs(), get_fields() and obs(), cast as the contract says"""
    fr, ur = NP_REAL[real_dtype]
    so = eng.step_outputs()
    reals, ints = eng.get_fields()
    names = eng.field_names()
    row = np.stack([reals[names.index(f)] for f in OBS_FIELDS], axis=1)
    o6 = eng.obs()  # rel_p_x, rel_p_y, rel_v_x, rel_v_y, rel_a_x, rel_a_y
    assert np.array_equal(row[:, [0, 4, 1, 5, 2, 6]].T, o6), "get_fields() and obs() disagree on the host"
    assert np.array_equal(so["reward"], reals[names.index("reward")]) and np.array_equal(so["cumulative_reward"], reals[names.index("cum_x")])
    cast = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).astype(fr)).view(ur)
    return {"obs": cast(row), "reward": cast(so["reward"]), "cumulative_reward": cast(so["cumulative_reward"]), "idx_x": so["idx_x"], "idx_y": so["idx_y"],
            "step_count": so["step_count"], "done": so["done"], "was_reset": so["was_reset"], "code": so["code"]}


def assert_view_equals(got, want, which, what):
    for k in which:
        if k == "bad_actions":
            continue
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{what}: {k} differs in envs {np.argwhere(got[k] != want[k])[:5].tolist()}"


def random_actions(rng, n, two_axis):
    ax = rng.integers(0, 3, n)
    return (ax | (rng.integers(0, 3, n) << 2 if two_axis else 0)).astype(np.uint8)


def fly_pair(dev, n, dtype, real_dtype, two_axis=0, periods=90, which=OUTPUTS, seed=3):
    from dql_multirotor_landing_amd.engine import Engine
    cfg = lambda: DqlConfig(dtype=dtype, t_max=3.0, two_axis=two_axis)
    a, b = Engine(cfg(), n, seed=seed), Engine(cfg(), n, seed=seed)
    bufs = ViewBufs(dev, n, real_dtype, which)
    d_act = dev.alloc(n)
    rng = np.random.default_rng(n + 10 * dtype + real_dtype)
    seen = {"done": 0, "was_reset": 0, "codes": set(), "idx_y": 0}
    try:
        for p in range(periods):
            act = random_actions(rng, n, two_axis)
            a.step(act)
            want = host_outputs(a, real_dtype)
            dev.up(d_act, act)
            b.step_dev(d_act)
            bufs.view(b)
            got = bufs.read(b)
            assert_view_equals(got, want, which, f"period {p}")
            for k in OUTPUTS:
                if k not in which:
                    assert bufs.poisoned(got, k), f"period {p}: {k} was not handed over and was written"
            if "bad_actions" in which:
                assert got["bad_actions"][0] == 0
            seen["done"] += int(want["done"].sum()); seen["was_reset"] += int(want["was_reset"].sum())
            seen["codes"] |= set(want["code"].tolist()); seen["idx_y"] += int((want["idx_y"] != 0).sum())
        for x, y in zip(a.get_fields(), b.get_fields()):
            np.testing.assert_array_equal(x, y)
    finally:
        b.sync()
        a.close(); b.close()
    return seen


@pytest.mark.parametrize("real_dtype", [F32, F64], ids=["to-f32", "to-f64"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [777, 1])
def test_device_path_equals_host_path_every_period(dev, n, dtype, real_dtype):
    seen = fly_pair(dev, n, dtype, real_dtype)
    # the events the comparison is there for occurred on the host path (engine A)
    assert seen["done"] >= 1 and seen["was_reset"] >= 1 and len(seen["codes"]) >= 2, seen


@pytest.mark.parametrize("two_axis", [0, 1])
def test_device_path_equals_host_path_on_both_axis_layouts(dev, two_axis):
    seen = fly_pair(dev, 320, F32, F32, two_axis=two_axis)
    assert seen["done"] >= 1 and seen["was_reset"] >= 1 and len(seen["codes"]) >= 2, seen
    assert not two_axis or seen["idx_y"] > 0, "no env had a non-zero idx_y in the two-axis case"


@pytest.mark.parametrize("which", [("obs",), ("done",), OUTPUTS], ids=["obs-only", "done-only", "all"])
def test_a_subset_of_the_outputs_leaves_the_other_buffers_poisoned(dev, which):
    seen = fly_pair(dev, 777, F64, F32, which=which)
    assert seen["done"] >= 1 and seen["was_reset"] >= 1, seen


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_view_after_train_and_eval_steps_equals_the_host_getters(dev, dtype):
    from dql_multirotor_landing_amd.engine import Engine
    n = 777
    eng = Engine(DqlConfig(dtype=dtype, t_max=3.0), n, seed=5)
    bufs = ViewBufs(dev, n, F64)
    try:
        for fly in (lambda: eng.train_steps(25, 0.5), lambda: eng.eval_steps(7)):
            fly()
            bufs.view(eng)
            got = bufs.read(eng)
            want = host_outputs(eng, F64)
            assert_view_equals(got, want, OUTPUTS, "after on-device action selection")
            idx = eng.states(); rew = eng.rewards(); dn, cd = eng.dones()
            assert np.array_equal(got["idx_x"], idx) and np.array_equal(got["reward"].view(np.float64), rew)
            assert np.array_equal(got["done"], dn) and np.array_equal(got["code"], cd)
        assert eng.stats()["episodes"] > 0
    finally:
        eng.close()


def test_bad_actions_word_is_reported_and_not_cleared(dev):
    from dql_multirotor_landing_amd.engine import Engine
    n, n_bad = 777, 41
    eng = Engine(DqlConfig(dtype=F32, t_max=3.0), n, seed=9)
    bufs = ViewBufs(dev, n, F32, ("bad_actions", "done"))
    d_act = dev.alloc(n)
    try:
        act = np.full(n, 2, np.uint8)
        dev.up(d_act, act)
        eng.step_dev(d_act)  # the reset period: the codes are checked all the same, so fly good ones first
        bufs.view(eng)
        assert bufs.read(eng)["bad_actions"][0] == 0
        act[np.random.default_rng(0).choice(n, n_bad, replace=False)] = 3
        dev.up(d_act, act)
        eng.step_dev(d_act)
        bufs.view(eng)
        assert bufs.read(eng)["bad_actions"][0] == n_bad
        bufs.view(eng)  # a second view: the word is not cleared
        assert bufs.read(eng)["bad_actions"][0] == n_bad
        with pytest.raises(ValueError, match=f"{n_bad} action"):  # the host's report, once, as before
            eng.stats()
        eng.stats()
        bufs.view(eng)
        assert bufs.read(eng)["bad_actions"][0] == 0
    finally:
        eng.close()


def test_reset_dev_equals_reset_with_the_same_mask(dev):
    from dql_multirotor_landing_amd.engine import Engine
    n = 777
    a, b = Engine(DqlConfig(dtype=F32, t_max=3.0), n, seed=11), Engine(DqlConfig(dtype=F32, t_max=3.0), n, seed=11)
    rng = np.random.default_rng(1)
    d_act, d_mask = dev.alloc(n), dev.alloc(n)
    try:
        def both(act):
            a.step(act); dev.up(d_act, act); b.step_dev(d_act)
        for _ in range(12):
            both(random_actions(rng, n, 0))
        mask = (rng.random(n) < 1 / 3).astype(np.uint8)
        assert 200 < mask.sum() < 320
        a.reset(mask)
        dev.up(d_mask, mask)
        b.reset_dev(d_mask)
        both(random_actions(rng, n, 0))
        so = a.step_outputs()
        assert (so["was_reset"][mask == 1] == 1).all() and so["was_reset"].sum() >= mask.sum(), "the masked envs spent the period in reset"
        for _ in range(9):
            both(random_actions(rng, n, 0))
        for x, y in zip(a.get_fields(), b.get_fields()):
            np.testing.assert_array_equal(x, y)
        with pytest.raises(ValueError, match="dql_reset"):  # the library's own refusal of a NULL mask
            _lib.check(b.lib.dql_reset_dev(b._h, None))
    finally:
        b.sync()
        a.close(); b.close()


def test_refusals_name_themselves_and_touch_nothing(dev):
    from dql_multirotor_landing_amd.engine import Engine
    from dql_multirotor_landing_amd.population import Population
    n = 65
    eng = Engine(DqlConfig(dtype=F32, t_max=3.0), n, seed=2)
    bufs = ViewBufs(dev, n, F32)
    d_act = dev.alloc(n, fill=2)
    lib = eng.lib
    try:
        eng.step_dev(d_act)
        good = dict(real_dtype=F32, reserved=0, **{k: bufs.ptr[k] for k in OUTPUTS})

        def refused(h, view, needle):
            rc = lib.dql_view_dev(h, None if view is None else C.byref(_lib.DqlViewC(**view)))
            msg = lib.dql_last_error().decode()
            assert rc == _lib.EINVAL and needle in msg and msg.rstrip().endswith(("launched", "context", ")")) and len(msg.split()) >= 2, (rc, msg)
            got = bufs.read(eng)
            assert all(bufs.poisoned(got, k) for k in OUTPUTS), f"a refused call wrote a buffer ({needle})"

        refused(None, good, "null context")
        refused(eng._h, None, "view must not be null")
        refused(eng._h, dict(good, real_dtype=2), "real_dtype")
        refused(eng._h, dict(good, real_dtype=-1), "real_dtype")
        refused(eng._h, dict(good, reserved=1), "reserved")
        refused(eng._h, dict(good, obs=bufs.ptr["obs"] + 8), "16-byte aligned")
        pop = Population(DqlConfig(dtype=F32), 2, 512, [1, 2])
        try:
            refused(pop._h, good, "population")
        finally:
            pop.close()
        # a view without outputs: DQL_OK, nothing launched
        assert lib.dql_view_dev(eng._h, C.byref(_lib.DqlViewC(real_dtype=F32, reserved=0))) == _lib.OK
        got = bufs.read(eng)
        assert all(bufs.poisoned(got, k) for k in OUTPUTS)
        # ... and a good call after all that is correct
        bufs.view(eng)
        got = bufs.read(eng)
        assert_view_equals(got, host_outputs(eng, F32), OUTPUTS, "after the refusals")
        assert got["was_reset"].all() and got["bad_actions"][0] == 0
    finally:
        eng.close()
