"""CPU legs of tests/det_math_checks.py: the ORACLE's restatement of the device's elementary functions and random draws — the code the kernels must
equal bit for bit — against numpy float64 / np.longdouble and a numpy Philox, exhaustively where the input space is 2^24 words.  The same checks on the HIP
library, with device == oracle asserted first: tests/test_gpu_det_math.py (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

import det_math_checks as dm


@pytest.fixture(scope="module")
def be():
    return dm.OracleBackend()


def test_det_math_accuracy(be):
    """(moved from tests/test_oracle_golden.py, assertions unchanged) 4 000 points in [-7, 7] against numpy float64"""
    dm.check_legacy_points(be)


@pytest.mark.parametrize("dtype", dm.DTYPES, ids=dm.DTYPE_NAME.get)
@pytest.mark.parametrize("name", list(dm.CHECKS))
def test_oracle(be, name, dtype):
    dm.CHECKS[name](be, dtype)


def test_philox_known_answers_random_pairs_and_structured_counters(be):
    dm.check_philox(be)


def test_numpy_philox_is_not_the_oracle_restated():
    """the reference implementation forms the products in uint64 and masks; a one-bit change of counter or key changes the block"""
    c = np.array([[1, 2, 3, 4]], dtype=np.uint32); k = np.array([[5, 6]], dtype=np.uint32)
    base = dm.philox_numpy(c, k)
    for j in range(4):
        c2 = c.copy(); c2[0, j] ^= 1
        assert (dm.philox_numpy(c2, k) != base).any()
    for j in range(2):
        k2 = k.copy(); k2[0, j] ^= 1
        assert (dm.philox_numpy(c, k2) != base).any()


def test_diagnostic_operators_fail_loudly_without_a_gpu():
    """no CPU fallback: DQL_EHIP from every new entry point; argument errors are reported before the device is touched"""
    from dql_multirotor_landing_amd import _lib, ops
    lib = _lib.load()
    one = np.zeros(1); w = np.zeros(1, np.uint32)
    with pytest.raises(ValueError):
        ops.det_math_run(one, one, 2)
    with pytest.raises(ValueError):
        ops.philox_run(np.zeros((1, 4), np.uint32), 0, 0, round_keys=2)
    with pytest.raises(ValueError):
        ops.box_muller_run(np.zeros(dm.N24 + 1, np.uint32), np.zeros(dm.N24 + 1, np.uint32), 0)
    n = C.c_int(0)
    if lib.dql_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    for call in (lambda: ops.det_math_run(one, one, 0), lambda: ops.box_muller_run(w, w, 1), lambda: ops.philox_run(np.zeros((1, 4), np.uint32), 0, 0),
                 lambda: ops.selftest_sqrt_ieee(1.0, 2.0)):
        with pytest.raises(RuntimeError):
            call()
