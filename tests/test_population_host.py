"""Populations on the CPU: the launch barrier that lets K Trainers in threads share one population, driven over per-agent oracle engines
(population.SeparateEngines), and curriculum_attempts(concurrency=K) against the sequential loop."""
import hashlib
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from dql_multirotor_landing_amd.attempts import attempt_seed, curriculum_attempts  # noqa: E402
from dql_multirotor_landing_amd.population import AgentView, LaunchBarrier, SeparateEngines  # noqa: E402

KW = dict(curriculum_steps=3, n_envs=96, chunk_steps=8, checkpoint_every=10**9, max_num_episodes=150, t_max=3,
          successive_successful_episodes=10, success_rate=0.0, mode="paper", judge_envs=70)


def _oracle_engine_class():
    from dql_multirotor_landing_amd.config import CHECK_NAMES
    from oracle.oracle import Oracle

    class OracleEngine:  # the Engine surface the Trainer uses, computed by the CPU oracle
        def __init__(self, cfg, n, seed=42, device=0, env_id_offset=0):
            self.o = Oracle(cfg, n, seed=seed, env_id_offset=env_id_offset)
            self.n = n
        def __getattr__(self, name):
            return getattr(self.o, name)
        def step_index(self):
            return self.o.step_index
        def set_step_index(self, j):
            self.o.publish_tables(); self.o.step_index = int(j)
        def get_tables(self):
            return self.o.qa.copy(), self.o.qb.copy(), self.o.count.copy()
        def stats(self):
            d = self.o.stats_dict()
            d["by_code"] = {CHECK_NAMES[i]: d["by_code"][i] for i in range(len(CHECK_NAMES))}
            return d
        def close(self):
            pass
    return OracleEngine


def _strip(x):
    if isinstance(x, dict):
        return {k: _strip(v) for k, v in x.items() if not k.startswith("wall") and k != "beyond_choice"}
    if isinstance(x, list):
        return [_strip(v) for v in x]
    return x


def _tables_hash(eng):
    return hashlib.sha256(b"".join(np.ascontiguousarray(t, dtype=np.float64).tobytes() for t in eng.get_tables())).hexdigest()


def _run(tmp_path, tag, concurrency, monkeypatch):
    import dql_multirotor_landing_amd.trainer as T
    OE = _oracle_engine_class()
    monkeypatch.setattr(T, "Engine", OE)
    scores, hashes = {}, {}

    def make(j, engine_factory=None):
        return T.Trainer(seed=attempt_seed(5, j), save_path=tmp_path / tag / str(j) / "run", engine_factory=engine_factory, **KW)

    def score(tr):
        h = _tables_hash(tr._engine)
        hashes[tr._seed] = h
        # a landing score that depends on the tables alone (here: attempt 0 scores too low, attempt 1 is accepted, attempt 2 flies beside it in the wave)
        td = 1.0 - (int(h[:8], 16) % 1000) / 1000.0
        scores[tr._seed] = td
        return {"touchdown_rate": td, "goal_hold_rate": 0.5}

    make_pop = lambda cfg, k, e, seeds, dev: SeparateEngines(lambda c, n, s: OE(c, n, seed=s), cfg, k, e, seeds)
    res = curriculum_attempts(make, score, max_attempts=4, accept_touchdown=0.3, close=lambda tr: None, concurrency=concurrency, make_population=make_pop)
    return res, hashes


def test_concurrent_attempts_choose_what_the_sequential_loop_chooses(tmp_path, monkeypatch):
    seq, h_seq = _run(tmp_path, "seq", 1, monkeypatch)
    con, h_con = _run(tmp_path, "con", 3, monkeypatch)
    assert con["chosen"] == seq["chosen"] == 1 and con["accepted"] and seq["accepted"]
    assert _strip(con["history"]) == _strip(seq["history"])
    assert _tables_hash(con["trainer"]._engine) == _tables_hash(seq["trainer"]._engine)
    # every attempt the sequential loop flew was flown alike in its wave; the wave's later attempts are marked
    n = len(seq["attempts"])
    assert _strip(con["attempts"][:n]) == _strip(seq["attempts"])
    assert all(r.get("beyond_choice") for r in con["attempts"][n:])
    assert all(not r.get("beyond_choice") for r in con["attempts"][:n])
    for s, h in h_seq.items():
        assert h_con[s] == h
    assert con["concurrency"] == 3


def test_chosen_attempt_of_a_wave_is_the_lowest_accepted(tmp_path, monkeypatch):
    # accept nothing: every attempt flies, the fallback rule picks, in waves of 3 exactly as one by one
    import dql_multirotor_landing_amd.trainer as T
    OE = _oracle_engine_class()
    monkeypatch.setattr(T, "Engine", OE)
    out = {}
    for c in (1, 3):
        def make(j, engine_factory=None):
            return T.Trainer(seed=attempt_seed(9, j), save_path=tmp_path / str(c) / str(j) / "run", engine_factory=engine_factory, **KW)
        make_pop = lambda cfg, k, e, seeds, dev: SeparateEngines(lambda cc, n, s: OE(cc, n, seed=s), cfg, k, e, seeds)
        out[c] = curriculum_attempts(make, lambda tr: {"touchdown_rate": float(np.sum(tr._engine.get_tables()[2]) % 7) / 7, "goal_hold_rate": 0.0},
                                     max_attempts=4, accept_touchdown=2.0, close=lambda tr: None, concurrency=c, make_population=make_pop)
    assert out[3]["chosen"] == out[1]["chosen"] and not out[3]["accepted"]
    assert _strip(out[3]["attempts"]) == _strip(out[1]["attempts"])


def test_launch_barrier_serves_every_live_view_in_one_launch_and_lets_finished_ones_go():
    class Rec:
        lock = threading.RLock()
        envs_per_agent = 64
        def __init__(self):
            self.launches = []
        def launch(self, n, eps, words=None):
            self.launches.append((n, dict(eps)))
            return {k: None for k in eps}
    pop = Rec()
    bar = LaunchBarrier(pop, 3)
    views = [AgentView(pop, k, bar) for k in range(3)]
    chunks = {0: 2, 1: 4, 2: 3}

    def fly(k):
        for _ in range(chunks[k]):
            views[k].train_steps(8, 0.1 * (k + 1))
        views[k].close()
    th = [threading.Thread(target=fly, args=(k,)) for k in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join(30)
    assert not any(t.is_alive() for t in th)
    assert [sorted(e) for _, e in pop.launches] == [[0, 1, 2], [0, 1, 2], [1, 2], [1]]
    assert pop.launches[0][1] == {0: 0.1, 1: 0.2, 2: pytest.approx(0.3)}


def test_engine_factory_is_refused_with_a_reducer_or_windowed_schedule(tmp_path):
    from dql_multirotor_landing_amd.trainer import Trainer
    with pytest.raises(ValueError):
        Trainer(save_path=tmp_path, engine_factory=lambda *a: None, sync_period=2, **KW)
    with pytest.raises(ValueError):
        Trainer(save_path=tmp_path, engine_factory=lambda *a: None, reducer_factory=lambda e: None, **KW)
