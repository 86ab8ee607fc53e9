"""GPU legs of tests/f32_step_checks.py: the HIP float32 ENGINE against the float64 oracle at the flavours the curriculum and landing figures fly, against
the float32 oracle bit for bit after the same hand-over, and against the reference's recorded env-class flights (G13)."""
import numpy as np
import pytest

import f32_step_checks as sc

pytestmark = pytest.mark.gpu


def _make(cfg, n, seed):
    from dql_multirotor_landing_amd.engine import Engine
    return Engine(cfg, n, seed=seed)


@pytest.mark.parametrize("flavour", list(sc.FLAVOURS))
def test_f32_engine_vs_f64_oracle_at_the_flown_flavours(flavour):
    """as tests/test_f32_step.py with the engine flying the float32 side (16 one-period launches of 2 048 envs), then assertion 4: every field of the engine
    == the float32 oracle's after the same hand-over and calls"""
    res = sc.fly(_make, flavour)
    try:
        sc.check_flavour(res, flavour)
        sc.check_same_dtype_parity(res, flavour)
    finally:
        res["side"].close()


@pytest.mark.parametrize("tag", list(sc.G13_CASES))
def test_g13_recorded_flights_in_float32_on_hip(golden_dir, tag):
    """three single-env flights of 300-500 periods through dql_step; bounds measured on the CPU float32 oracle (f32_step_checks.G13_BOUNDS)"""
    z = np.load(golden_dir / "g13_env.npz")
    sig, res = sc.g13_fly(_make, tag, z)
    sc.check_g13_flight(tag, z, sig, res)
