"""GPU legs of tests/det_math_checks.py: the functions at the top of csrc/dql_device.hpp called with chosen inputs through the library's diagnostic
operators.  Every call asserts device == oracle bit for bit on all of its inputs (det_math_checks.HipBackend) before the device's own output is held to
numpy float64 / np.longdouble / the numpy Philox."""
import pytest

import det_math_checks as dm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return dm.HipBackend()


def test_det_math_accuracy_on_hip(be):
    dm.check_legacy_points(be)


@pytest.mark.parametrize("dtype", dm.DTYPES, ids=dm.DTYPE_NAME.get)
@pytest.mark.parametrize("name", list(dm.CHECKS))
def test_hip(be, name, dtype):
    dm.CHECKS[name](be, dtype)


def test_philox_inline_and_round_key_forms(be):
    """the Random123 vectors, 2^16 random pairs and the structured counters (step_hi != 0, the carry, the last env id, every stream constant) through the
    oracle, the device's inline key schedule and the device's round keys in registers: all equal to the numpy implementation"""
    figs = dm.check_philox(be)
    assert len(figs["forms"]) == 3


def test_sqrt_ieee_is_correctly_rounded_on_its_domain(be):
    """sqrt_(float) (Box-Muller's radius) against (float)sqrt((double)x) — the oracle's sqrtf — at 0 and on every float32 from 2^-102 to FLT_MAX; the normal
    inputs below 2^-104 misround and are outside the documented domain (det_math_checks.check_sqrt_ieee)"""
    dm.check_sqrt_ieee(be)
