"""The level-0 instances of the step kernel on the MI355X (csrc/dql_hip.hip: k_step without the AnyLevel tag).

A launch of an x-axis config on a literal-MDP layout (TICK_LIT, TICK_PACKED_LITM) whose working level is 0 runs an instance in which the level is the compile-time
constant 0; every other launch runs the generic body.  Both must compute the oracle's bits: every real and int field, both tables and the visit
counters they are folded into, both tables' window accumulators (target sums and visits), the statistics — in TRAIN mode with 1 and 16 periods
per launch, for the reference's quirks (0x7f), Double Q-learning with the kept goal count (0x60) and none (0), with and without observation noise
on per-env platforms, at level 0 (the new instance) and at levels 1, 2 and 4 (the generic one, which the host must go on choosing there).
The instance follows the level: a context promoted between two launches changes instance, and its second launch is the oracle's.  A
population's kernel takes every agent's level from its descriptor and keeps the generic body for all of them, level 0 included.

Envs: 300 (one full and one ragged workgroup of 256) and 512 for the 256-thread literal layout, 128 (two one-wave workgroups) for the 64-thread
packed-literal one.  Episodes are short (t_max 1 s: 23 periods), so resets — the placement's level test — happen inside every case.
"""
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd.config import DqlConfig, F32

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "assets"
NOISY = dict(per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build_hip()


@pytest.fixture(scope="module")
def tables():
    """the reference's stage-4 tables: greedy actions and bootstraps are non-trivial at every level"""
    return tuple(np.load(GOLDEN / f) for f in ("Q_table_a.npy", "Q_table_b.npy", "state_action_count.npy"))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(eng, orc, what):
    er, ei = eng.get_fields()
    o_r, o_i = orc.get_fields()
    for k, nm in enumerate(eng.field_names(True)):
        assert np.array_equal(ei[k], o_i[k]), f"{what}: int field {nm} differs in envs {np.flatnonzero(ei[k] != o_i[k])[:5]}"
    for k, nm in enumerate(eng.field_names()):
        assert np.array_equal(_bits(er[k]), _bits(o_r[k])), f"{what}: field {nm} differs in envs {np.flatnonzero(_bits(er[k]) != _bits(o_r[k]))[:5]}"
    qa, qb, cnt = eng.get_tables()
    assert np.array_equal(_bits(qa.ravel()), _bits(orc.qa)), f"{what}: Q_table_a"
    assert np.array_equal(_bits(qb.ravel()), _bits(orc.qb)), f"{what}: Q_table_b"
    assert np.array_equal(_bits(cnt.ravel()), _bits(orc.count)), f"{what}: state_action_counter"
    se, so = eng.stats(), orc.stats_dict()
    assert se["decisions"] == so["decisions"] and se["episodes"] == so["episodes"], f"{what}: decisions / episodes"
    assert list(se["by_code"].values()) == so["by_code"], f"{what}: terminal histogram"
    assert se["reward_sum"] == so["reward_sum"], f"{what}: reward sum"


def _pair(cfg_kw, n, seed, block, tick, P, tables):
    from dql_multirotor_landing_amd.engine import Engine
    from oracle.oracle import Oracle
    cfg = dict(dtype=F32, t_max=1.0, **cfg_kw)
    eng, orc = Engine(DqlConfig(**cfg), n, seed=seed), Oracle(DqlConfig(**cfg), n, seed=seed)
    eng.set_option("block", block); eng.set_option("tick", tick)
    eng.set_option("periods_per_launch", P); orc.set_option("periods_per_launch", P)
    eng.set_tables(*tables); orc.set_tables(*tables)
    return eng, orc


def _run_case(n, block, tick, instance, P, quirks, noisy, working, tables):
    kw = dict(quirks=quirks, working_curriculum_step=working, **(NOISY if noisy else {}))
    what = f"n={n} block={block} P={P} quirks={quirks:#x} noisy={noisy} working={working}"
    eng, orc = _pair(kw, n, 17, block, tick, P, tables)
    try:
        steps = 26 if P == 1 else 32  # past the time-out at 23 periods: every env is reset and placed again
        eng.train_steps(steps, 0.3); orc.train_steps(steps, 0.3)
        assert eng.step_instance() == instance, what
        assert eng.step_level0() == (working == 0), f"{what}: the level-0 instance serves level 0 and only level 0"
        _same(eng, orc, what)
        assert eng.stats()["episodes"] >= n, f"{what}: no resets inside the case"
        # both tables' accumulators of a window: target sums and visits
        eng.set_windowed(True); orc.set_windowed(True)
        eng.train_steps(P, 0.3); orc.train_steps(P, 0.3)
        assert np.array_equal(eng.get_accum(), orc.get_accum()), f"{what}: window accumulators"
        _same(eng, orc, what + " (windowed)")
    finally:
        eng.close()


MATRIX = [(P, q, noisy, w) for P in (1, 16) for q in (0x7F, 0x60, 0) for noisy in (0, 1) for w in (0, 1, 2, 4)]
IDS = [f"P{P}-q{q:#x}-{'noisy' if noisy else 'plain'}-level{w}" for P, q, noisy, w in MATRIX]


@pytest.mark.parametrize("n", [300, 512])
@pytest.mark.parametrize("P,quirks,noisy,working", MATRIX, ids=IDS)
def test_literal_tick_block_256_bit_exact_at_every_level(tables, n, P, quirks, noisy, working):
    _run_case(n, 256, 4, "k_step<float,256,LIT,X_ONLY>", P, quirks, noisy, working, tables)


@pytest.mark.parametrize("P,quirks,noisy,working", MATRIX, ids=IDS)
def test_packed_literal_block_64_bit_exact_at_every_level(tables, P, quirks, noisy, working):
    _run_case(128, 64, 3, "k_step<float,64,PACKED_LITM,X_ONLY>", P, quirks, noisy, working, tables)


@pytest.mark.parametrize("block,tick,n", [(256, 4, 300), (64, 3, 128)])
def test_the_instance_follows_the_level_between_launches(tables, block, tick, n):
    """one context, promoted between two launches: level 0 runs the level-0 instance, the next launch the generic one, and both are the oracle's"""
    eng, orc = _pair(dict(NOISY), n, 5, block, tick, 16, tables)
    try:
        eng.train_steps(16, 0.3); orc.train_steps(16, 0.3)
        assert eng.step_level0()
        _same(eng, orc, "level 0")
        eng.transfer(1, 0.8172650252856599); orc.transfer(1, 0.8172650252856599)
        eng.set_curriculum(1); orc.set_curriculum(1)
        eng.train_steps(16, 0.3); orc.train_steps(16, 0.3)
        assert not eng.step_level0(), "a launch at level 1 ran the level-0 instance"
        _same(eng, orc, "level 1, second launch of the same context")
        eng.train_steps(32, 0.3); orc.train_steps(32, 0.3)
        _same(eng, orc, "level 1, later launches")
        assert (eng.states() // 189).max() == 1, "no env reached level 1's states: the case would not tell the instances apart"
        eng.set_curriculum(0); orc.set_curriculum(0)  # and back: the choice is made at every launch
        eng.train_steps(32, 0.3); orc.train_steps(32, 0.3)
        assert eng.step_level0()
        _same(eng, orc, "level 0 again")
    finally:
        eng.close()


@pytest.mark.parametrize("block,n", [(512, 1100), (256, 300), (64, 128)])
def test_two_axis_configs_keep_the_generic_body_at_level_0(tables, block, n):
    """the level-0 instances are x-axis instances (launch_step_t: the two-axis one of the 512-thread literal layout sent wrong targets to the tables):
    a two-axis context at level 0 runs the generic body in every workgroup size, and the oracle's bits"""
    eng, orc = _pair(dict(two_axis=1, **NOISY), n, 77, block, 4, 16, tables)
    try:
        for eps in (1.0, 0.2, 0.2):
            eng.train_steps(16, eps); orc.train_steps(16, eps)
            assert eng.step_instance() == f"k_step<float,{block},LIT,X_TWO>" and not eng.step_level0()
            _same(eng, orc, f"two-axis, block {block}")
    finally:
        eng.close()


def test_population_keeps_the_generic_body_for_agents_at_any_level(tables):
    """k_step_pop takes each agent's level from its descriptor: agents at levels 0, 1 and 3 in one launch equal contexts of their own — of which the
    one at level 0 runs the level-0 instance — and those equal the oracle"""
    from dql_multirotor_landing_amd.engine import Engine
    from dql_multirotor_landing_amd.population import Population
    from oracle.oracle import Oracle
    cfg = dict(dtype=F32, t_max=1.0, **NOISY)
    E, seeds, levels = 512, [3, 1009, 77], [0, 1, 3]
    pop = Population(DqlConfig(**cfg), 3, E, seeds)
    engs = [Engine(DqlConfig(**cfg), E, seed=s) for s in seeds]
    orcs = [Oracle(DqlConfig(**cfg), E, seed=s) for s in seeds]
    try:
        for x in [pop] + engs:
            x.set_option("block", 256); x.set_option("tick", 4); x.set_option("periods_per_launch", 16)
        for k in range(3):
            orcs[k].set_option("periods_per_launch", 16)
            pop.set_tables(k, *tables); engs[k].set_tables(*tables); orcs[k].set_tables(*tables)
            pop.set_curriculum(k, levels[k]); engs[k].set_curriculum(levels[k]); orcs[k].set_curriculum(levels[k])
        pop.pop_train_steps(32, {0: 0.3, 1: 0.3, 2: 0.3})
        assert pop.step_instance() == "k_step_pop<float,256,LIT,X_ONLY>" and not pop.step_level0()
        for k in range(3):
            engs[k].train_steps(32, 0.3); orcs[k].train_steps(32, 0.3)
            assert engs[k].step_level0() == (levels[k] == 0)
            _same(engs[k], orcs[k], f"context at level {levels[k]}")
            r, i = pop.agent_fields(k)
            r0, i0 = engs[k].get_fields()
            assert np.array_equal(i, i0) and np.array_equal(_bits(r), _bits(r0)), f"agent {k} (level {levels[k]}): fields"
            for a, b in zip(pop.get_tables(k), engs[k].get_tables()):
                assert np.array_equal(_bits(a), _bits(b)), f"agent {k} (level {levels[k]}): tables / counters"
            assert pop.agent_stats(k) == engs[k].stats() and pop.index_faults(k) == 0
    finally:
        pop.close()
        for e in engs:
            e.close()
