"""CPU legs of tests/f32_step_checks.py: the float32 ORACLE — the restatement the float32 kernel is held to bit for bit — against the float64 oracle at
the flavours the curriculum and landing figures fly, and against the reference's recorded env-class flights (G13).  The same checks with the HIP engine
as the float32 side: tests/test_gpu_f32_step.py (-m gpu)."""
import numpy as np
import pytest

import f32_step_checks as sc
from oracle.oracle import Oracle


def _make(cfg, n, seed):
    return Oracle(cfg, n, seed=seed, n_threads=8)


@pytest.mark.parametrize("flavour", list(sc.FLAVOURS))
def test_f32_oracle_vs_f64_oracle_at_the_flown_flavours(flavour):
    """16 periods from a mid-flight hand-over, integer fields compared after every period (<= 0.5 % of 2 048 envs may leave), continuous fields within
    test_f32_kernel_vs_f64_oracle's bounds after the first and the last — the acceleration pair within its difference-quotient bound where B19 is off and
    R = 0 —, and the window contains the touchdowns (simulation) or a TERMINAL_SUCCESS and a fly-zone end (training)."""
    sc.check_flavour(sc.fly(_make, flavour), flavour)


@pytest.mark.parametrize("tag", list(sc.G13_CASES))
def test_g13_recorded_flights_in_float32(golden_dir, tag):
    """train0 / train2 / sim4 re-flown with dtype = F32 under the fixture's scripted actions: states, reset periods, done and CheckResult as the reference's env
    classes returned them, signals within 4 x the measured maximum of the float64 recording, reward within what the signal differences explain"""
    z = np.load(golden_dir / "g13_env.npz")
    sig, res = sc.g13_fly(_make, tag, z)
    sc.check_g13_flight(tag, z, sig, res)
