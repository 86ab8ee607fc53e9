"""The step kernel's epilogue against the CPU oracle, one launch at a time (run with -m gpu on an MI355X).

A staged launch (workgroups of 128 .. 512 threads) collects its TD targets in LDS, and its waves' statistics in eleven LDS slots, and moves
both to global memory behind its last barrier: every thread scans its share of the cells and sends a cell's sum and its count each on its
own, whenever it is non-zero; lanes 0 .. 10 of every wave add the wave's statistics to the LDS slots and threads 0 .. 10 of the
workgroup publish them.  A visit that is lost or doubled on the way, by this flush or by one that is split in time (an early flush inside
the period loop from 4 periods per launch was measured and dropped; the cases that would catch it stay), shows here: after
ONE launch the accumulators (target sums and visit counts of both tables), the tables folded from them, every per-env field and the
statistics equal the oracle's bit for bit, and the visit counts add up to decisions x axes.

Cases: workgroups of 128, 256 and 512 threads; an env count that is no multiple of any of them (the last workgroup has idle lanes
and idle waves, which still take their share of the flush); 1, 2, 3, 4, 5 and 16 periods per launch; eps = 1 (targets spread over
nearly all cells) and eps = 0 (greedy: many lanes on few cells); the two-axis config (two targets per env and period), the paper's
update rule (both tables receive targets) and curriculum level 4 (five levels' cells in the stage)."""
import numpy as np
import pytest

from dql_multirotor_landing_amd.config import DqlConfig, F32, Q_PAPER

pytestmark = pytest.mark.gpu

N_CELLS = 2835
N_ENVS = 5 * 512 + 64 + 37  # 2661: the last workgroup of 128 / 256 / 512 threads holds 101 envs = one full and one ragged wave


@pytest.fixture(scope="module")
def mods():
    from dql_multirotor_landing_amd.engine import Engine
    from oracle.oracle import Oracle
    return Engine, Oracle


def _stats_equal(eng, orc, what):
    se, so = eng.stats(), orc.stats_dict()
    assert se["decisions"] == so["decisions"] and se["episodes"] == so["episodes"], what
    assert list(se["by_code"].values()) == so["by_code"], what
    assert se["reward_sum"] == so["reward_sum"], what  # fixed-point sum: order independent
    return se["decisions"]


def _state_equal(eng, orc, what):
    er, ei = eng.get_fields()
    o_r, o_i = orc.get_fields()
    assert np.array_equal(ei, o_i), f"{what}: int fields"
    assert np.array_equal(er, o_r), f"{what}: real fields"
    qa, qb, cnt = eng.get_tables()
    assert np.array_equal(qa.ravel(), orc.qa) and np.array_equal(qb.ravel(), orc.qb) and np.array_equal(cnt.ravel(), orc.count), f"{what}: tables"


def _one_launch_at_a_time(mods, block, P, eps, kw, launches=3):
    Engine, Oracle = mods
    axes = 2 if kw.get("two_axis") else 1
    eng = Engine(DqlConfig(dtype=F32, **kw), N_ENVS, seed=5); orc = Oracle(DqlConfig(dtype=F32, **kw), N_ENVS, seed=5, n_threads=8)
    eng.set_option("block", block)
    eng.set_option("periods_per_launch", P); orc.set_option("periods_per_launch", P)
    # the window accumulators of a windowed context hold exactly what the launches since the last fold added
    eng.set_windowed(True); orc.set_windowed(True)
    decisions = 0
    for j in range(launches):  # launch 0 begins with the reset period (no decision in it), the later ones have decisions in every period
        what = f"block {block} P {P} eps {eps} {kw} launch {j}"
        eng.train_steps(P, eps); orc.train_steps(P, eps)
        assert eng.step_instance().startswith(f"k_step<float,{block},"), eng.step_instance()
        acc, ref = eng.get_accum(), orc.get_accum()
        assert acc.shape == (4 * N_CELLS,)
        a = acc.reshape(4, N_CELLS); r = ref.reshape(4, N_CELLS)
        assert np.array_equal(a[1], r[1]) and np.array_equal(a[3], r[3]), f"{what}: visit counts differ in {np.flatnonzero((a[1] != r[1]) | (a[3] != r[3]))[:8]}"
        assert np.array_equal(a[0], r[0]) and np.array_equal(a[2], r[2]), f"{what}: target sums differ in {np.flatnonzero((a[0] != r[0]) | (a[2] != r[2]))[:8]}"
        d = _stats_equal(eng, orc, what)
        assert int(a[1].sum() + a[3].sum()) == (d - decisions) * axes, f"{what}: {int(a[1].sum() + a[3].sum())} visits for {d - decisions} decisions x {axes}"
        assert d > decisions or P == 1, what
        decisions = d
        _state_equal(eng, orc, what + " inside the window")
        eng.apply_accum(); orc.apply_accum()
        assert not eng.get_accum().any(), what
        _state_equal(eng, orc, what + " after the fold")
    eng.close()


@pytest.mark.parametrize("eps", [1.0, 0.0])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 16])
@pytest.mark.parametrize("block", [128, 256, 512])
def test_one_launch_equals_the_oracle(mods, block, P, eps):
    _one_launch_at_a_time(mods, block, P, eps, {})


@pytest.mark.parametrize("eps", [1.0, 0.0])
@pytest.mark.parametrize("P", [1, 3, 4, 5, 16])
@pytest.mark.parametrize("block", [256, 512])
def test_one_launch_equals_the_oracle_two_axis(mods, block, P, eps):
    _one_launch_at_a_time(mods, block, P, eps, dict(two_axis=1))


@pytest.mark.parametrize("eps", [1.0, 0.0])
@pytest.mark.parametrize("P", [1, 4, 16])
@pytest.mark.parametrize("block", [128, 256, 512])
def test_one_launch_equals_the_oracle_both_tables(mods, block, P, eps):
    """the paper's Double Q-learning: the coin sends a target to table a or table b, so both halves of the LDS stage are flushed"""
    _one_launch_at_a_time(mods, block, P, eps, dict(quirks=Q_PAPER, fold_per_step=1))


def test_one_launch_equals_the_oracle_higher_level(mods):
    """curriculum level 4: five levels' cells in the stage (the flush loop makes 23 passes at 128 threads, not 5)"""
    for block in (128, 256):
        _one_launch_at_a_time(mods, block, 16, 1.0, dict(working_curriculum_step=4, quirks=Q_PAPER))
