"""Every step-kernel instance the host picks by itself, at the batch size that picks it, bit for bit against the CPU oracle over the WHOLE
batch (run with -m gpu on an MI355X); and the table fold of the multi-GPU window (k_apply_window -> fold_q) against the exact reference
of tests/fold_reference.py and against the oracle.

The parity matrix of test_gpu_parity.py forces `tick` and `block` at 70 .. 20 000 envs; here both stay on auto and each case asserts the
instance the host chose (Engine.step_instance), so a drift in the selection fails here too.  Each case starts from the reference's
stage-4 tables (greedy actions and bootstraps non-trivial), trains 16 periods per launch at eps = 1, then at eps = 0.2, and compares every
real and int field, both tables, the visit counter and the statistics.  Sizing: the oracle steps about 2.4e6 env-steps/s on 8 CPU
threads at 65 536 - 131 072 envs, float64 as fast as float32; the module steps about 2e8 env-steps over the whole batches."""
from pathlib import Path

import numpy as np
import pytest

import fold_reference as fr
from dql_multirotor_landing_amd.config import DqlConfig, F32, F64, Q_PAPER

pytestmark = pytest.mark.gpu

CFG4 = dict(per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1)  # BASELINE configs[4] flags
PPL = 16


@pytest.fixture(scope="module")
def mods():
    from dql_multirotor_landing_amd.engine import Engine
    from oracle.oracle import Oracle
    return Engine, Oracle


def _compare(eng, orc, what):
    er, ei = eng.get_fields()
    o_r, o_i = orc.get_fields()
    names = eng.field_names(); inames = eng.field_names(True)
    assert names == orc.field_names() and inames == orc.field_names(True)
    for k, nm in enumerate(inames):
        assert np.array_equal(ei[k], o_i[k]), f"{what}: int field {nm} differs in envs {np.flatnonzero(ei[k] != o_i[k])[:5]}"
    for k, nm in enumerate(names):
        assert np.array_equal(er[k], o_r[k]), f"{what}: field {nm} differs in envs {np.flatnonzero(er[k] != o_r[k])[:5]}, max abs diff {np.abs(er[k] - o_r[k]).max()}"
    del er, ei, o_r, o_i
    for nm, a, b in zip(("Q_table_a", "Q_table_b", "state_action_counter"), eng.get_tables(), (orc.qa, orc.qb, orc.count)):
        a = a.ravel()
        assert np.array_equal(a, b), f"{what}: {nm} differs in cells {np.flatnonzero(a != b)[:5]}"
    se, so = eng.stats(), orc.stats_dict()
    assert se["decisions"] == so["decisions"] > 0 and se["episodes"] == so["episodes"], what
    assert list(se["by_code"].values()) == so["by_code"], what
    assert se["reward_sum"] == so["reward_sum"], what


CASES = [  # envs, config, instance the host must pick, (periods at eps 1, periods at eps 0.2)
    (65536, {}, "k_step<float,256,PACKED_LITM,X_ONLY>", (16, 96)),
    (65536, dict(two_axis=1), "k_step<float,256,PACKED,X_TWO>", (16, 96)),                       # BASELINE configs[2]
    (131072, dict(CFG4, quirks=Q_PAPER, fold_per_step=1), "k_step<float,256,LIT,X_ONLY>", (16, 96)),  # the bench's headline
    (131072, dict(two_axis=1), "k_step<float,256,LIT,X_TWO>", (16, 96)),
    (262144, {}, "k_step<float,512,LIT,X_ONLY>", (16, 96)),                                      # 4-waves-per-SIMD register budget
    (262144, dict(CFG4, two_axis=1), "k_step<float,512,LIT,X_TWO>", (16, 96)),
    (262144, dict(mass=0.75), "k_step<float,512,PLAIN,X_RUNTIME>", (16, 96)),                   # not the reference vehicle: run-time constants
    (131072, dict(dtype=F64, two_axis=1), "k_step<double,256,PLAIN,X_RUNTIME>", (16, 96)),
    (1 << 20, CFG4, "k_step<float,512,LIT,X_ONLY>", (16, 16)),
]


@pytest.mark.parametrize("n,kw,instance,sched", CASES, ids=[f"{c[0]}-{c[2]}" + ("-" + "-".join(f"{k}{v}" for k, v in c[1].items()) if c[1] else "") for c in CASES])
def test_auto_selected_instance_bit_exact_at_full_batch(mods, n, kw, instance, sched):
    Engine, Oracle = mods
    cfg = dict(dtype=F32); cfg.update(kw)
    eng = Engine(DqlConfig(**cfg), n, seed=77)
    orc = Oracle(DqlConfig(**cfg), n, seed=77, n_threads=16)
    try:
        eng.set_option("periods_per_launch", PPL); orc.set_option("periods_per_launch", PPL)
        g = Path(__file__).parent / "golden" / "assets"
        qa, qb, cnt = (np.load(g / f) for f in ("Q_table_a.npy", "Q_table_b.npy", "state_action_count.npy"))
        eng.set_tables(qa, qb, cnt); orc.set_tables(qa, qb, cnt)
        assert eng.step_instance() == ""
        for steps, eps in zip(sched, (1.0, 0.2)):
            eng.train_steps(steps, eps); orc.train_steps(steps, eps)
            assert eng.step_instance() == instance
        _compare(eng, orc, f"{n} envs {kw} {instance}")
    finally:
        eng.close()


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("per_step,n_launch", [(0, 1), (1, 1), (1, 4), (1, 16), (1, 1000)])
def test_window_fold_against_exact_reference_and_oracle(mods, per_step, n_launch, with_b):
    """The crafted cells of tests/fold_reference.py through k_apply_window.  Call sequence: set_windowed(True), then (n_launch > 1) train
    n_launch periods so that the window covers n_launch launches' worth of periods, set_tables — which writes the master AND the window's
    base tables (dql_set_tables, in every mode) — set_accum with the crafted window, apply_accum, get_tables.  Each cell within its
    rounding bound of the exact fold, and every table bit-equal to the oracle's fold of the same inputs."""
    Engine, Oracle = mods
    cfg = DqlConfig(dtype=F32, fold_per_step=per_step)
    tab = cfg.alpha_table()
    cases = fr.fold_cases(len(tab))
    qa, qb, cnt, acc = fr.fold_inputs(cases, with_b)
    eng = Engine(cfg, 64, seed=3)
    try:
        eng.set_windowed(True)
        if n_launch > 1:
            eng.set_option("periods_per_launch", min(n_launch, PPL))
            eng.train_steps(n_launch, 1.0)
        eng.set_tables(qa, qb, cnt)
        eng.set_accum(acc)
        eng.apply_accum()
        ga, gb, gc = (t.ravel() for t in eng.get_tables())
        assert not eng.get_accum().any(), "the fold clears the window"
    finally:
        eng.close()
    o = Oracle(cfg, 1)
    oa, ob, oc, oacc = qa.copy(), qb.copy(), cnt.copy(), acc.copy()
    o._contract(oa, ob, oc, oacc, n_launch)
    fr.check_against_exact(cases, qa, qb, cnt, acc, ga, gb, gc, per_step, n_launch, tab, cfg.alpha_min, f"k_apply_window per_step={per_step} n_launch={n_launch}")
    for nm, a, b in (("Q_table_a", ga, oa), ("Q_table_b", gb, ob), ("state_action_counter", gc, oc)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{nm}: kernel vs oracle fold differ in cells {np.flatnonzero(a != b)[:5]}"
