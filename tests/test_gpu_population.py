"""Populations on the MI355X: agent k of a population (include/dql.h dql_pop_*) is bit-identical to a context of its own made with agent k's
seed and driven through the same calls, in every dtype, axis mode and step-kernel layout; a one-agent population is a plain context; the
single-agent calls are refused on a population of several; concurrent curriculum attempts choose what the sequential loop chooses."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu

from dql_multirotor_landing_amd.config import DqlConfig, F32, F64  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build_hip()


def _same_state(pop, k, eng):
    r, i = pop.agent_fields(k)
    r0, i0 = eng.get_fields()
    assert np.array_equal(i, i0), f"agent {k}: int fields"
    assert np.array_equal(r.view(np.uint64), r0.view(np.uint64)), f"agent {k}: real fields"
    for a, b in zip(pop.get_tables(k), eng.get_tables()):
        assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)), f"agent {k}: tables / counters"
    assert pop.agent_stats(k) == eng.stats(), f"agent {k}: stats"
    assert pop.agent_step_index(k) == eng.step_index()
    assert pop.index_faults(k) == 0


def _same_logs(pop, engs, ran):
    """pop's log against each context's; ran[k]: periods agent k ran since the last read"""
    done, goal = pop.episode_log_read()
    wpa = pop.envs_per_agent // 64
    assert done.shape[0] == max(ran)
    for k, e in enumerate(engs):
        d0, g0 = e.episode_log_read()
        assert d0.shape[0] == ran[k]
        assert np.array_equal(done[:ran[k], k * wpa:(k + 1) * wpa], d0) and np.array_equal(goal[:ran[k], k * wpa:(k + 1) * wpa], g0), f"agent {k}: episode log"
        assert not done[ran[k]:, k * wpa:(k + 1) * wpa].any()


def _same_outputs(pop, engs):
    so = pop.step_outputs()
    E = pop.envs_per_agent
    for k, e in enumerate(engs):
        s0 = e.step_outputs()
        for name, v in s0.items():
            assert np.array_equal(so[name][k * E:(k + 1) * E], v), f"agent {k}: step output {name}"


CASES = [  # dtype, two_axis, envs per agent, forced block, forced tick (0 = auto)
    (F32, 0, 4096, 0, 0),     # auto: the population (12 288 envs) flies block 256, its twins (4 096) block 64
    (F32, 1, 4096, 0, 0),
    (F32, 0, 512, 64, 1),
    (F32, 1, 512, 64, 3),
    (F32, 0, 1024, 128, 1),
    (F32, 0, 1024, 256, 4),
    (F32, 1, 1024, 256, 3),
    (F32, 0, 1024, 512, 4),
    (F64, 0, 512, 0, 0),
    (F64, 1, 1024, 128, 0),
    (F64, 0, 1024, 256, 0),
]


@pytest.mark.parametrize("dtype,two_axis,E,block,tick", CASES)
def test_population_agents_equal_contexts_of_their_own(dtype, two_axis, E, block, tick):
    from dql_multirotor_landing_amd.engine import Engine
    from dql_multirotor_landing_amd.population import Population
    cfg = DqlConfig(dtype=dtype, two_axis=two_axis, t_max=4.0)
    seeds, levels = [11, 20260, 7], [0, 2, 4]
    pop = Population(cfg, 3, E, seeds)
    engs = [Engine(cfg, E, seed=s) for s in seeds]
    try:
        for name, v in (("block", block), ("tick", tick)):
            if v:
                pop.set_option(name, v)
                for e in engs:
                    e.set_option(name, v)
        pop.episode_log_enable(64)
        for k, e in enumerate(engs):
            e.episode_log_enable(64)
            pop.set_curriculum(k, levels[k])
            e.set_curriculum(levels[k])
        eps = {0: 0.9, 1: 0.5, 2: 0.2}

        def train(n, active):
            pop.pop_train_steps(n, {k: eps[k] for k in active})
            for k in active:
                engs[k].train_steps(n, eps[k])

        train(3, [0, 1, 2])                       # one period per launch
        _same_logs(pop, engs, [3, 3, 3])
        for x in [pop] + engs:
            x.set_option("periods_per_launch", 16)
        train(20, [0, 1, 2])                      # 16 + 4
        _same_logs(pop, engs, [20, 20, 20])
        train(16, [0, 2]); train(16, [0, 2])      # agent 1 sits out two launches
        _same_logs(pop, engs, [32, 0, 32])
        for k in range(3):
            _same_state(pop, k, engs[k])
        # per-agent table surgery, a level switch and a masked reset mid-run
        pop.transfer(2, 3, 0.5); engs[2].transfer(3, 0.5)
        qa, qb, cnt = engs[0].get_tables()
        pop.set_tables(0, qa * 0.5, qb, cnt); engs[0].set_tables(qa * 0.5, qb, cnt)
        pop.set_curriculum(1, 3); engs[1].set_curriculum(3)
        mask = (np.random.default_rng(3).random(3 * E) < 0.3).astype(np.uint8)
        pop.reset(mask)
        for k, e in enumerate(engs):
            e.reset(mask[k * E:(k + 1) * E])
        eps = {0: 0.3, 1: 0.7, 2: 0.05}
        train(24, [0, 1, 2])
        _same_logs(pop, engs, [24, 24, 24])
        pop.pop_eval_steps(5)
        for e in engs:
            e.eval_steps(5)
        _same_logs(pop, engs, [5, 5, 5])
        _same_outputs(pop, engs)
        for k in range(3):
            _same_state(pop, k, engs[k])
            assert pop.agent_stats(k)["decisions"] > 0
    finally:
        pop.close()
        for e in engs:
            e.close()


CFG4 = dict(per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1)  # BASELINE configs[4] flags
SIZE_CASES = [  # agents, envs per agent, config flags, launches, instance of the population's launches, instance of its twins' launches
    (4, 32768, CFG4, 3, "k_step_pop<float,256,LIT,X_ONLY>", "k_step<float,256,PACKED_LITM,X_ONLY>"),   # tools/exp_population.py
    (16, 512, {}, 12, "k_step_pop<float,64,PACKED_LITM,X_ONLY>", "k_step<float,64,PACKED_LITM,X_ONLY>"),  # DQL_MAX_AGENTS
]


@pytest.mark.parametrize("K,E,kw,launches,pop_instance,twin_instance", SIZE_CASES, ids=["4x32768-configs4", "16x512"])
def test_population_at_product_sizes(K, E, kw, launches, pop_instance, twin_instance):
    """The measured population (4 x 32 768, whose whole batch picks the literal-constant 256-thread layout while each twin alone picks
    the packed one) and the DQL_MAX_AGENTS limit (16 agents), auto layout, 16 periods per launch, non-contiguous active subsets that
    change every launch, more launches than the descriptor ring (DQL_POP_RING = 8) has slots: every agent equals its twin context."""
    from dql_multirotor_landing_amd.engine import Engine
    from dql_multirotor_landing_amd.population import Population
    cfg = DqlConfig(dtype=F32, t_max=4.0, **kw)
    seeds = [1000 + 37 * k for k in range(K)]
    pop = Population(cfg, K, E, seeds)
    engs = [Engine(cfg, E, seed=s) for s in seeds]
    try:
        for x in [pop] + engs:
            x.set_option("periods_per_launch", 16)
        for k, e in enumerate(engs):
            pop.set_curriculum(k, k % 5)
            e.set_curriculum(k % 5)
        rng = np.random.default_rng(K)
        for j in range(launches):
            active = [0, K - 1] if j == 0 else sorted(int(a) for a in rng.choice(K, size=max(2, K // 2), replace=False))
            eps = {k: 1.0 if j == 0 else 0.1 + 0.05 * ((k + j) % 7) for k in active}
            pop.pop_train_steps(16, eps)
            assert pop.step_instance() == pop_instance
            for k in active:
                engs[k].train_steps(16, eps[k])
                assert engs[k].step_instance() == twin_instance
        for k in range(K):
            _same_state(pop, k, engs[k])
        assert sum(pop.agent_stats(k)["decisions"] > 0 for k in range(K)) >= 2
    finally:
        pop.close()
        for e in engs:
            e.close()


def test_one_agent_population_is_a_plain_context():
    from dql_multirotor_landing_amd.engine import Engine
    from dql_multirotor_landing_amd.population import Population
    cfg = DqlConfig(dtype=F32, t_max=4.0)
    pop = Population(cfg, 1, 1024, [99])
    eng = Engine(cfg, 1024, seed=99)
    try:
        for x in (pop, eng):  # the single-agent calls of the C ABI act on agent 0
            Engine.set_curriculum(x, 1)
            x.set_option("periods_per_launch", 8)
            Engine.train_steps(x, 20, 0.6)
            Engine.transfer(x, 2, 0.8)
            Engine.set_step_index(x, Engine.step_index(x) + 3)
            Engine.train_steps(x, 9, 0.1)
            Engine.eval_steps(x, 4)
        for a, b in zip(Engine.get_tables(pop), eng.get_tables()):
            assert np.array_equal(a, b)
        assert Engine.stats(pop) == eng.stats()
        r, i = pop.get_fields(); r0, i0 = eng.get_fields()
        assert np.array_equal(i, i0) and np.array_equal(r.view(np.uint64), r0.view(np.uint64))
        assert pop.index_faults(0) == 0
    finally:
        pop.close(); eng.close()


def test_single_agent_calls_are_refused_on_a_population():
    from dql_multirotor_landing_amd.engine import Engine
    from dql_multirotor_landing_amd.population import Population
    cfg = DqlConfig(dtype=F32)
    with pytest.raises(ValueError, match="multiple of 512"):
        Population(cfg, 2, 1000, [1, 2])
    with pytest.raises(ValueError):
        Population(cfg, 17, 512, list(range(17)))
    pop = Population(cfg, 2, 512, [1, 2])
    try:
        for call in (lambda: Engine.train_steps(pop, 1, 0.1), lambda: Engine.eval_steps(pop, 1), lambda: Engine.get_tables(pop),
                     lambda: Engine.set_tables(pop, np.zeros((5, 3, 3, 3, 7, 3))), lambda: Engine.transfer(pop, 1, 0.5),
                     lambda: Engine.set_curriculum(pop, 1), lambda: Engine.stats(pop), lambda: Engine.step_index(pop),
                     lambda: Engine.set_step_index(pop, 0), lambda: Engine.publish_tables(pop)):
            with pytest.raises(ValueError, match="dql_pop_"):
                call()
        for call in (lambda: Engine.step(pop, np.full(1024, 2, np.uint8)), lambda: pop.set_windowed(True), lambda: pop.get_accum()):
            with pytest.raises(ValueError, match="population"):
                call()
        with pytest.raises(ValueError):
            pop.get_tables(2)  # agent index out of range
        # the whole-context calls still serve
        pop.pop_train_steps(2, {0: 0.5, 1: 0.5})
        assert pop.get_fields()[1].shape[1] == 1024
    finally:
        pop.close()


def test_concurrent_attempts_on_the_hip_engine_equal_the_sequential_loop(tmp_path):
    from dql_multirotor_landing_amd.attempts import attempt_seed, curriculum_attempts
    from dql_multirotor_landing_amd.trainer import Trainer
    kw = dict(curriculum_steps=3, n_envs=2048, chunk_steps=8, checkpoint_every=10**9, max_num_episodes=3000, t_max=3,
              successive_successful_episodes=10, success_rate=0.0, mode="paper", judge_envs=70)

    def run(c):
        hashes = {}

        def make(j, engine_factory=None):
            return Trainer(seed=attempt_seed(5, j), save_path=tmp_path / str(c) / str(j) / "run", engine_factory=engine_factory, **kw)

        def score(tr):
            h = hashlib.sha256(b"".join(np.ascontiguousarray(t).tobytes() for t in tr._engine.get_tables())).hexdigest()
            hashes[tr._seed] = h
            return {"touchdown_rate": (int(h[:8], 16) % 1000) / 1000.0, "goal_hold_rate": 0.0}
        res = curriculum_attempts(make, score, max_attempts=3, accept_touchdown=2.0, concurrency=c)  # nothing accepted: all three fly
        return res, hashes

    seq, h1 = run(1)
    con, h3 = run(3)
    strip = lambda hist: [{k: v for k, v in h.items() if not k.startswith("wall")} for h in hist]
    assert con["chosen"] == seq["chosen"] and con["accepted"] == seq["accepted"]
    assert strip(con["history"]) == strip(seq["history"])
    assert h3 == h1 and len(h1) == 3
