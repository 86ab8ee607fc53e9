"""GPU legs of tests/episode_dtype_checks.py.  (1) The float32 and the float64 HIP ENGINE flown period by period from reset to every env's terminal, 4 096
pairs, at four flavours that pick different step-kernel instances: the same body of checks as the CPU oracle's (tests/test_episode_dtypes.py), with the
bounds measured there.  (2) One launch per dtype of the roll-out operator at 65 536 envs, for every flavour: at most 5 % of the terminal codes differ,
McNemar's balance of the landing outcome and the paired means of steps and cumulative reward at z = 4 — a bias of 0.2 % in a landing rate shows at this
size, at 4 096 pairs it needs 1 %.  The first 4 096 envs of a roll-out are the stepwise flights of (1), bit for bit (the contract of dql_rollout), in both
dtypes, which ties the halves together."""
import functools

import pytest

from dql_multirotor_landing_amd import ops
from dql_multirotor_landing_amd.config import F32, F64
from dql_multirotor_landing_amd.engine import Engine

import episode_dtype_checks as ec
import rollout_checks as rc

pytestmark = pytest.mark.gpu
SEED = ec.SEEDS[0]
STEPWISE = ("sim", "sim_two_axis_configs4", "train_l0", "train_l4")
ROLLOUT_ENVS = 65536


class _Engine(Engine):
    def step_instance(self):
        return super().step_instance() + (" level 0" if self.step_level0() else "")


def _make(cfg, n, seed):
    return _Engine(cfg, n, seed=seed)


@functools.lru_cache(maxsize=None)
def _stepwise(flavour):
    """flown once, shared by the stepwise test and the roll-out test of the flavour, and left unchanged"""
    return ec.paired_flights(_make, ec.FLAVOURS[flavour][0], rc.stage4_tables(), ec.N_ENVS, SEED, ec.MAX_STEPS)


@pytest.mark.parametrize("flavour", STEPWISE)
def test_f32_engine_episodes_against_their_f64_twins(flavour):
    pair = _stepwise(flavour)
    m, bal = ec.check(pair, flavour)
    print(flavour, pair[F32]["instance"], pair[F64]["instance"], {k: v for k, v in m.items() if k not in ("concordant", "strict_exceptions", "max_abs_per_field")}, bal)


def test_the_stepwise_flavours_ran_the_instances_they_are_there_for():
    """float32: the x-axis instance, the two-axis one, and the level-0 instance at level 0 only (float64 has none)"""
    seen = {f: _stepwise(f)[F32]["instance"] for f in STEPWISE}
    assert all("float" in v for v in seen.values()) and seen["sim"] != seen["sim_two_axis_configs4"], seen
    assert [f for f in STEPWISE if "level 0" in seen[f]] == ["train_l0"], seen
    seen64 = {f: _stepwise(f)[F64]["instance"] for f in STEPWISE}
    assert all("double" in v and "level 0" not in v for v in seen64.values()), seen64


@pytest.mark.parametrize("flavour", list(ec.FLAVOURS))
def test_rollouts_of_65536_pairs_show_no_bias_and_start_with_the_stepwise_flights(flavour):
    make_cfg = ec.FLAVOURS[flavour][0]
    tables = rc.stage4_tables()
    timing = {F32: {}, F64: {}}
    got = {dt: ops.rollout(make_cfg(dt), tables, ROLLOUT_ENVS, SEED, max_steps=ec.MAX_STEPS, timing=timing[dt]) for dt in (F32, F64)}
    row = {dt: {f: got[dt][f][0] for f in ("code", "steps") + rc.RECORD_FIELDS} for dt in (F32, F64)}
    differs, bal = ec.check_rollouts(row[F32], row[F64], flavour)
    print(flavour, "kernel ms", {("f32", "f64")[dt]: round(t["kernel_ms"], 1) for dt, t in timing.items()}, "codes differ in", differs, "of", ROLLOUT_ENVS, bal)
    if flavour in STEPWISE:
        for dt in (F32, F64):
            head = {f: v[:ec.N_ENVS] for f, v in row[dt].items()}
            rc.assert_rows_equal(head, _stepwise(flavour)[dt], f"{flavour}, {('float32', 'float64')[dt]}: the first {ec.N_ENVS} envs of the roll-out vs the stepwise engine")
