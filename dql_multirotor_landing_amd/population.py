"""Populations: K independent agents stepped together (include/dql.h dql_pop_*).

`Population` is one context of K agents x E envs: every agent has its own Q tables, visit counters, level, seed, step index, statistics and
exploration rate, and all active agents' envs are stepped by ONE kernel launch.  Agent k is bit-identical to `Engine(cfg, E, seeds[k])` driven
through the same calls (launches it sits out do not touch it).

`AgentView(pop, k)` is the `Engine` surface the `Trainer` uses, for one agent.  `LaunchBarrier` lets K trainers run in threads on one population:
each view's `train_steps` waits until every live trainer has asked for its next chunk, then ONE launch serves all of them (per-agent eps, the
trainers that asked as the active set) and each view gets its own slice of the episode log.  A trainer's decisions depend on its own agent's
results only, so the interleaving of the threads cannot change what any of them computes.

`SeparateEngines` is the same per-agent interface over K engines of their own (one context per agent): the reference a population is held to,
and a way to run the scheduler on CPU engines (the tests do).
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .config import CHECK_NAMES, DqlConfig, N_CELLS, TABLE_SHAPE
from .engine import Engine, _p


class Population(Engine):
    """K agents x `envs_per_agent` envs in one context (agent-major).  Whole-context methods inherited from `Engine` (get_fields, reset,
    step_outputs, set_option, episode_log_*) act on all K E envs; the per-agent methods take the agent index first."""

    def __init__(self, cfg: DqlConfig, n_agents: int, envs_per_agent: int, seeds: Sequence[int], device: int = 0, alpha_table=None):
        self.lib = _lib.load()
        self.cfg = cfg
        self.n_agents, self.envs_per_agent = int(n_agents), int(envs_per_agent)
        if len(seeds) != self.n_agents:
            raise ValueError("one seed per agent")
        self.n = self.n_agents * self.envs_per_agent
        self._c = cfg.to_c()
        s = (C.c_uint64 * self.n_agents)(*[int(v) for v in seeds])
        h = C.c_void_p()
        _lib.check(self.lib.dql_pop_create(C.byref(self._c), device, self.n_agents, self.envs_per_agent, s, C.byref(h)))
        self._h = h
        self.lock = threading.RLock()  # every call on the shared context takes it (LaunchBarrier: trainers in threads)
        tab = cfg.alpha_table() if alpha_table is None else np.ascontiguousarray(alpha_table, dtype=np.float64)
        _lib.check(self.lib.dql_set_alpha_table(self._h, _p(tab), len(tab)))

    def _mask(self, active):
        if active is None:
            return None
        m = np.zeros(self.n_agents, dtype=np.uint8)
        m[list(active)] = 1
        return m

    # ---- stepping ----
    def pop_train_steps(self, n_steps: int, eps: Dict[int, float]):
        """one call, the agents in `eps` active (each with its own exploration rate)"""
        e = np.zeros(self.n_agents, dtype=np.float64)
        for k, v in eps.items():
            e[k] = float(v)
        m = self._mask(eps.keys())
        _lib.check(self.lib.dql_pop_train_steps(self._h, int(n_steps), _p(e), _p(m)))

    def pop_eval_steps(self, n_steps: int, active=None):
        m = self._mask(active)
        _lib.check(self.lib.dql_pop_eval_steps(self._h, int(n_steps), _p(m)))

    def launch(self, n_steps: int, eps: Dict[int, float], words: Optional[Dict[int, int]] = None):
        """LaunchBarrier's launch: train the agents in `eps` for n_steps periods and hand each its episode-log slice
        (done, goal: uint64[n_steps, words]) when the log is on"""
        self.pop_train_steps(n_steps, eps)
        if not getattr(self, "_elog_cap", 0):
            return {k: None for k in eps}
        done, goal = self.episode_log_read()
        wpa = self.envs_per_agent // 64
        out = {}
        for k in eps:
            w = wpa if words is None or words.get(k) is None else max(0, min(int(words[k]), wpa))
            out[k] = (done[:n_steps, k * wpa:k * wpa + w].copy(), goal[:n_steps, k * wpa:k * wpa + w].copy())
        return out

    # ---- per agent ----
    def set_curriculum(self, k: int, level: int):
        _lib.check(self.lib.dql_pop_set_curriculum(self._h, int(k), int(level)))

    def get_tables(self, k: int):
        qa = np.zeros(N_CELLS); qb = np.zeros(N_CELLS); cnt = np.zeros(N_CELLS)
        _lib.check(self.lib.dql_pop_get_tables(self._h, int(k), _p(qa), _p(qb), _p(cnt)))
        return qa.reshape(TABLE_SHAPE), qb.reshape(TABLE_SHAPE), cnt.reshape(TABLE_SHAPE)

    def get_counts(self, k: int):
        cnt = np.zeros(N_CELLS)
        _lib.check(self.lib.dql_pop_get_tables(self._h, int(k), None, None, _p(cnt)))
        return cnt.reshape(TABLE_SHAPE)

    def set_tables(self, k: int, qa=None, qb=None, count=None):
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ravel()
        qa, qb, count = f(qa), f(qb), f(count)
        for a in (qa, qb, count):
            if a is not None and a.size != N_CELLS:
                raise ValueError(f"tables must have shape {TABLE_SHAPE}")
        _lib.check(self.lib.dql_pop_set_tables(self._h, int(k), _p(qa), _p(qb), _p(count)))

    def transfer(self, k: int, level: int, ratio: float):
        _lib.check(self.lib.dql_pop_transfer(self._h, int(k), int(level), float(ratio)))

    def publish_tables(self, k: int):
        _lib.check(self.lib.dql_pop_publish_tables(self._h, int(k)))

    def agent_stats(self, k: int):
        s = _lib.DqlStatsC()
        _lib.check(self.lib.dql_pop_stats_get(self._h, int(k), C.byref(s)))
        return {"agent_steps": s.agent_steps, "decisions": s.decisions, "episodes": s.episodes,
                "by_code": {CHECK_NAMES[i]: s.by_code[i] for i in range(len(CHECK_NAMES))},
                "reward_sum": s.reward_sum, "physics_ticks": s.physics_ticks}

    def agent_step_index(self, k: int) -> int:
        v = C.c_int64()
        _lib.check(self.lib.dql_pop_get_step_index(self._h, int(k), C.byref(v)))
        return v.value

    def set_agent_step_index(self, k: int, j: int):
        _lib.check(self.lib.dql_pop_set_step_index(self._h, int(k), int(j)))

    def index_faults(self, k: int) -> int:
        v = C.c_int64()
        _lib.check(self.lib.dql_pop_index_faults(self._h, int(k), C.byref(v)))
        return v.value

    def agent_fields(self, k: int):
        r, i = self.get_fields()
        s = slice(k * self.envs_per_agent, (k + 1) * self.envs_per_agent)
        return r[:, s].copy(), i[:, s].copy()

    def set_agent_fields(self, k: int, reals, ints):
        r, i = self.get_fields()
        s = slice(k * self.envs_per_agent, (k + 1) * self.envs_per_agent)
        r[:, s] = reals; i[:, s] = ints
        self.set_fields(r, i)


class SeparateEngines:
    """The per-agent interface of `Population` over K engines of their own (make_engine(cfg, n, seed) -> an Engine-like object, e.g. a CPU
    engine in the tests): what a population must equal, and the scheduler's CPU stand-in."""

    def __init__(self, make_engine: Callable, cfg: DqlConfig, n_agents: int, envs_per_agent: int, seeds: Sequence[int]):
        self.n_agents, self.envs_per_agent = int(n_agents), int(envs_per_agent)
        self.engines = [make_engine(cfg, self.envs_per_agent, int(s)) for s in seeds]
        self.lock = threading.RLock()
        self._elog_cap = 0

    def launch(self, n_steps: int, eps: Dict[int, float], words: Optional[Dict[int, int]] = None):
        out = {}
        for k in sorted(eps):
            e = self.engines[k]
            e.train_steps(int(n_steps), float(eps[k]))
            if self._elog_cap:
                done, goal = e.episode_log_read()
                w = done.shape[1] if words is None or words.get(k) is None else max(0, min(int(words[k]), done.shape[1]))
                out[k] = (np.asarray(done)[:, :w].copy(), np.asarray(goal)[:, :w].copy())
            else:
                out[k] = None
        return out

    def episode_log_enable(self, cap: int):
        self._elog_cap = int(cap)
        for e in self.engines:
            e.episode_log_enable(cap)

    def set_option(self, name, value):
        for e in self.engines:
            e.set_option(name, value)

    def field_names(self, is_int=False):
        return self.engines[0].field_names(is_int)

    def set_curriculum(self, k, level): self.engines[k].set_curriculum(level)
    def get_tables(self, k): return self.engines[k].get_tables()
    def get_counts(self, k): return self.engines[k].get_tables()[2]
    def set_tables(self, k, qa=None, qb=None, count=None): self.engines[k].set_tables(qa, qb, count)
    def transfer(self, k, level, ratio): self.engines[k].transfer(level, ratio)
    def publish_tables(self, k): self.engines[k].publish_tables()
    def agent_stats(self, k): return self.engines[k].stats()
    def agent_step_index(self, k): return self.engines[k].step_index()
    def set_agent_step_index(self, k, j): self.engines[k].set_step_index(j)
    def index_faults(self, k): return 0
    def agent_fields(self, k): return self.engines[k].get_fields()
    def set_agent_fields(self, k, reals, ints): self.engines[k].set_fields(reals, ints)

    def close(self):
        for e in self.engines:
            if hasattr(e, "close"):
                e.close()


class LaunchBarrier:
    """K trainers in threads on one population: a launch runs once every live view has asked for its chunk (`train`), the views that asked are
    its active agents.  Views that are done `leave`."""

    def __init__(self, pop, n_agents: int):
        self.pop = pop
        self._cv = threading.Condition()
        self._live = set(range(int(n_agents)))
        self._req: Dict[int, tuple] = {}
        self._res: Dict[int, object] = {}
        self._gen = 0
        self._error: Optional[BaseException] = None

    def _launch_if_complete(self):
        if not self._live or set(self._req) != self._live:
            return
        reqs, self._req = self._req, {}
        try:
            by_n: Dict[int, Dict[int, float]] = {}
            for k, (n, eps, _) in reqs.items():
                by_n.setdefault(n, {})[k] = eps
            with self.pop.lock:
                for n, eps in sorted(by_n.items()):
                    self._res.update(self.pop.launch(n, eps, {k: reqs[k][2] for k in eps}))
        except BaseException as e:  # every waiting view raises it
            self._error = e
        self._gen += 1
        self._cv.notify_all()

    def train(self, k: int, n_steps: int, eps: float, words: Optional[int] = None):
        with self._cv:
            if self._error is not None:
                raise RuntimeError("a population launch failed") from self._error
            gen = self._gen
            self._req[k] = (int(n_steps), float(eps), words)
            self._launch_if_complete()
            while self._gen == gen:
                self._cv.wait()
            if self._error is not None:
                raise RuntimeError("a population launch failed") from self._error
            return self._res.pop(k)

    def leave(self, k: int):
        with self._cv:
            self._live.discard(k)
            self._req.pop(k, None)
            self._launch_if_complete()


class AgentView:
    """Agent k of a population, with the `Engine` surface the `Trainer` uses.  With a `LaunchBarrier`, `train_steps` waits for the other
    trainers' chunks and runs in the shared launch; without one it is a launch of this agent alone."""

    def __init__(self, pop, k: int, barrier: Optional[LaunchBarrier] = None, on_close: Optional[Callable[["AgentView"], None]] = None):
        self.pop, self.k, self.barrier = pop, int(k), barrier
        self.n = pop.envs_per_agent
        self._elog_cap = 0
        self._log: List = []
        self._on_close = on_close
        self._closed = False

    # ---- stepping ----
    def train_steps(self, n_steps: int, eps: float, _words: Optional[int] = None):
        if self.barrier is not None:
            got = self.barrier.train(self.k, n_steps, eps, _words)
        else:
            with self.pop.lock:
                got = self.pop.launch(int(n_steps), {self.k: float(eps)}, {self.k: _words})[self.k]
        if got is not None:
            self._log.append(got)

    # ---- episode log: this agent's words of every period it ran ----
    def episode_log_enable(self, capacity_periods: int):
        with self.pop.lock:
            if capacity_periods > getattr(self.pop, "_elog_cap", 0):
                self.pop.episode_log_enable(int(capacity_periods))
        self._elog_cap = int(capacity_periods)
        self._log = []

    def episode_log_read(self, words=None):
        wpa = self.n // 64 if self.n % 64 == 0 else (self.n + 63) // 64
        w = wpa if words is None else max(0, min(int(words), wpa))
        if not self._log:
            z = np.zeros((0, w), dtype=np.uint64)
            return z, z.copy()
        done = np.concatenate([d[:, :w] for d, _ in self._log]); goal = np.concatenate([g[:, :w] for _, g in self._log])
        self._log = []
        return done, goal

    # ---- per agent ----
    def stats(self):
        with self.pop.lock:
            return self.pop.agent_stats(self.k)

    def get_tables(self):
        with self.pop.lock:
            return self.pop.get_tables(self.k)

    def get_counts(self):
        with self.pop.lock:
            return self.pop.get_counts(self.k)

    def set_tables(self, qa=None, qb=None, count=None):
        with self.pop.lock:
            self.pop.set_tables(self.k, qa, qb, count)

    def transfer(self, k: int, ratio: float):
        with self.pop.lock:
            self.pop.transfer(self.k, k, ratio)

    def set_curriculum(self, level: int):
        with self.pop.lock:
            self.pop.set_curriculum(self.k, level)

    def publish_tables(self):
        with self.pop.lock:
            self.pop.publish_tables(self.k)

    def step_index(self) -> int:
        with self.pop.lock:
            return self.pop.agent_step_index(self.k)

    def set_step_index(self, j: int):
        with self.pop.lock:
            self.pop.set_agent_step_index(self.k, j)

    def index_faults(self) -> int:
        with self.pop.lock:
            return self.pop.index_faults(self.k)

    def get_fields(self):
        with self.pop.lock:
            return self.pop.agent_fields(self.k)

    def set_fields(self, reals, ints):
        with self.pop.lock:
            self.pop.set_agent_fields(self.k, reals, ints)

    def field_names(self, is_int=False):
        with self.pop.lock:
            return self.pop.field_names(is_int)

    def set_option(self, name: str, value: int):
        """options are the population's (one launch serves every agent): the trainers of a population must agree on them"""
        with self.pop.lock:
            self.pop.set_option(name, value)

    def close(self):
        if self._closed:
            return
        self._closed = True
        if self.barrier is not None:
            self.barrier.leave(self.k)
        if self._on_close is not None:
            self._on_close(self)


class PopulationWave:
    """K trainers built before any of them flies: trainer k gets `engine_factory(k)` as its Trainer(engine_factory=...).  The population is made
    once all K have asked for their engine (same config, each its own seed), by `make_population(cfg, n_agents, envs_per_agent, seeds, device)`; it is
    closed when the last view closes."""

    def __init__(self, n_agents: int, make_population: Callable):
        self.n_agents = int(n_agents)
        self._make = make_population
        self._cv = threading.Condition()
        self._asks: Dict[int, tuple] = {}
        self._views: Optional[List[AgentView]] = None
        self._error: Optional[BaseException] = None
        self._open = self.n_agents
        self.pop = None

    def engine_factory(self, k: int) -> Callable:
        def make(cfg, n_envs, seed, device):
            with self._cv:
                self._asks[k] = (cfg, int(n_envs), int(seed), device)
                if len(self._asks) == self.n_agents and self._views is None and self._error is None:
                    try:
                        cfgs = [self._asks[j][0] for j in range(self.n_agents)]
                        if any(bytes(c.to_c()) != bytes(cfgs[0].to_c()) for c in cfgs) or len({self._asks[j][1] for j in range(self.n_agents)}) != 1:
                            raise ValueError("the trainers of a population must share config and n_envs (only the seed differs)")
                        self.pop = self._make(cfgs[0], self.n_agents, self._asks[0][1], [self._asks[j][2] for j in range(self.n_agents)], self._asks[0][3])
                        barrier = LaunchBarrier(self.pop, self.n_agents)
                        self._views = [AgentView(self.pop, j, barrier, on_close=self._closed) for j in range(self.n_agents)]
                    except BaseException as e:
                        self._error = e
                    self._cv.notify_all()
                while self._views is None and self._error is None:
                    self._cv.wait()
                if self._error is not None:
                    raise RuntimeError("the population could not be made") from self._error
                return self._views[k]
        return make

    def abandon(self, k: int):
        """trainer k is done (or failed, or never asked for its engine): nobody waits for it any more"""
        with self._cv:
            if self._views is None and k not in self._asks:
                self._error = self._error or RuntimeError(f"trainer {k} of the population ended before it asked for its engine")
                self._cv.notify_all()
        if self._views is not None:
            self._views[k].barrier.leave(k)  # (the view stays usable — scoring reads its tables — until it is closed)

    def _closed(self, view):
        self._open -= 1
        if self._open == 0 and self.pop is not None and hasattr(self.pop, "close"):
            self.pop.close()
