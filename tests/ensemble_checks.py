"""Shared by the sequential-ensemble tests (CPU emulation and GPU): the reference loop and the `==` comparison.

`Reference` is the ensemble's equality contract spelled out with the unchanged oracle: ONE `Oracle(cfg, L, seed)` stepped with external actions, the action
word from `oracle.philox((j_lo, j_hi, l, STREAM_ACTION), (seed_lo, seed_hi))`, the greedy choice from `oracle.agent_predict` on per-learner numpy tables,
the update from `oracle.agent_update(..., coin=, done=)` with alpha at the pre-increment count, and the freeze rules applied with a literal `deque`.  A frozen
learner's env is put back to its bytes at the freeze point after every oracle step (the oracle steps all L envs), so it is untouched until re-armed."""
import math
from collections import deque
from pathlib import Path

import numpy as np

from dql_multirotor_landing_amd.config import CHECK_NAMES, N_CELLS
from oracle import oracle as orc
from oracle.oracle import Oracle

GOAL = CHECK_NAMES.index("TERMINAL_SUCCESS")
N_CODES = len(CHECK_NAMES)
STREAM_ACTION = 0
EPS_TABLE = [1.0, 1.0, 0.5, 0.1, 0.0]  # per episode index within the level
STATE_REAL_FIELDS = ("cum_x", "reward", "px", "py", "pz", "vx", "vy", "vz", "mp_x", "mp_u", "qw", "qx", "qy", "qz", "pitch_sp")
STATE_INT_FIELDS = ("idx_x", "step_count", "code", "flags", "action")
Q_REFERENCE, Q_BENCH, Q_PAPER = 0x7F, 0x60, 0x40  # the reference; the bench recipe (B1/B2 update, paper reward and mask); Double Q-learning with the coin


def eps_thr(eps):
    return 0 if not eps > 0.0 else min(int(math.ceil(eps * 16777216.0)), 16777216)


# ---- trained starting tables: the reference's stage-4 tables (tests/golden/assets), every learner with its own small perturbation ----
GOLDEN_ASSETS = Path(__file__).resolve().parent / "golden" / "assets"
TRAINED_SEED, TRAINED_NOISE = 5, 0.01


def trained_tables(n):
    """(qa, qb, count), float64 [n][N_CELLS]: learner l starts from Q * (1 + TRAINED_NOISE * N(0, 1)) per cell, the visit counts as stored (up to 1 955, beyond
    the learning-rate table of 1 536 entries).  The noise is drawn [learner][table][cell], so learner l's tables do not depend on n."""
    qa, qb, cnt = (np.load(GOLDEN_ASSETS / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy", "state_action_count.npy"))
    assert qa.size == qb.size == cnt.size == N_CELLS
    z = np.random.default_rng(TRAINED_SEED).standard_normal((int(n), 2, N_CELLS))
    return qa * (1.0 + TRAINED_NOISE * z[:, 0]), qb * (1.0 + TRAINED_NOISE * z[:, 1]), np.tile(cnt, (int(n), 1))


# ---- plain learners from trained tables (tests/test_gpu_ensemble.py and tests/test_learner_host_emulation.py): greedy, window 4, 2 successes, 6 episodes ----
TRAINED_LEARNERS_CASE = dict(eps=[0.0], window=4, min_successes=2, max_episodes=6, log_capacity=32)
TRAINED_LEARNERS_SEED, TRAINED_LEARNERS_PERIODS, TRAINED_LEARNERS_SPLIT = 11, 400, (7, 393)


def trained_reference(cfg, n):
    """the result of the reference loop flown from `trained_tables(n)` at the config's level, after asserting ON IT what the case is for"""
    tables = trained_tables(n)
    ref = Reference(cfg, n, TRAINED_LEARNERS_SEED, tables=tables, **TRAINED_LEARNERS_CASE)
    ref.run(TRAINED_LEARNERS_PERIODS)
    want = ref.result()
    promoted, failures = want["promotion_episode"] >= 0, int((want["episodes"] - want["successes"]).sum())
    print(f"level {cfg.working_curriculum_step} quirks {cfg.quirks:#x}: promoted", int(promoted.sum()), "of", n, "live", int((~want["frozen"]).sum()), "successes", int(want["successes"].sum()),
          "failures", failures, "cells written a / b", int((want["qa"] != tables[0]).sum()), int((want["qb"] != tables[1]).sum()), "updates inside / beyond the learning-rate table",
          ref.updates_inside, ref.updates_beyond, "same-state periods", ref.same_state)
    assert cfg.working_curriculum_step >= 1 and promoted.any() and not want["frozen"].all(), "a learner promoting through the ring above level 0 and a live one are needed"
    assert want["successes"].sum() >= 1 and failures >= 1, "successes and failures are both needed"
    assert (want["qa"] != tables[0]).any() and ((want["qb"] != tables[1]).any() or cfg.quirks != Q_PAPER), "under the coin both tables are to be written"
    assert ref.updates_inside >= 1 and ref.updates_beyond >= 1 and (want["count"] > len(ref.alpha)).any(), "learning rates from the table and alpha_min beyond it are both needed"
    return want, tables


class Reference:
    def __init__(self, cfg, n, seed, eps=EPS_TABLE, window=100, min_successes=97, max_episodes=1 << 30, log_capacity=64, alpha_tab=None, tables=None):
        """tables: initial (qa, qb, count), [n][N_CELLS] each (copied); default zeros"""
        self.cfg, self.n, self.seed = cfg, int(n), int(seed)
        self.o = Oracle(cfg, self.n, seed=self.seed)
        self.qa, self.qb, self.cnt = (np.zeros((self.n, N_CELLS)) for _ in range(3)) if tables is None else (np.array(t, np.float64).reshape(self.n, N_CELLS) for t in tables)
        self.alpha = cfg.alpha_table() if alpha_tab is None else np.asarray(alpha_tab, np.float64)
        self.thr = [eps_thr(e) for e in eps]
        self.W, self.min_successes, self.max_episodes, self.cap = int(window), int(min_successes), int(max_episodes), int(log_capacity)
        self.j = 0
        self.same_state = 0  # transitions with s' == s: the carried row of the next greedy choice must show the write
        self.updates_inside, self.updates_beyond = 0, 0  # updates whose learning rate came from the table / was alpha_min beyond its end
        self.decisions, self.episodes, self.successes = (np.zeros(self.n, np.int64) for _ in range(3))
        self.by_code = np.zeros((N_CODES, self.n), np.int64)
        self.log_code = np.zeros((self.n, self.cap), np.uint8); self.log_len = np.zeros((self.n, self.cap), np.uint16); self.log_n = np.zeros(self.n, np.int32)
        rn, inn = self.o.field_names(False), self.o.field_names(True)
        self.ri = {f: rn.index(f) for f in STATE_REAL_FIELDS}
        self.ii = {f: inn.index(f) for f in STATE_INT_FIELDS}
        self.es = self.o.env_size
        self.rearm()

    def rearm(self):
        self.level_episodes = np.zeros(self.n, np.int32)
        self.windows = [deque([], maxlen=self.W) for _ in range(self.n)]
        self.promoted = np.full(self.n, -1, np.int32)
        self.frozen = np.zeros(self.n, bool)
        self.freeze_period = np.full(self.n, -1, np.int64)  # the period index in which the learner froze (not part of result(): the ensemble does not keep it)
        self.snap = {}

    def set_schedules(self, eps, window, min_successes, max_episodes):
        """`SequentialEnsemble.set_schedules` without the learning rates: a new exploration table and new freeze rules for the learners as they stand.  A deque
        cannot change its length with entries in it, so the window may only change while every deque is empty (right after the start or a `set_level`)."""
        self.thr = [eps_thr(e) for e in eps]
        if int(window) != self.W:
            assert all(len(w) == 0 for w in self.windows), "the window length changes with outcomes in a deque"
            self.W = int(window)
            self.windows = [deque([], maxlen=self.W) for _ in range(self.n)]
        self.min_successes, self.max_episodes = int(min_successes), int(max_episodes)

    def set_level(self, k):
        for l, b in self.snap.items():  # the frozen envs as they were left, then every env re-enters through reset
            self.o.envs[l * self.es:(l + 1) * self.es] = b
        self.o.set_curriculum(k)
        self.rearm()

    def transfer(self, k, ratio):
        for l in range(self.n):
            orc.transfer(self.qa[l], self.qb[l], k, ratio)

    def run(self, periods):
        o, n = self.o, self.n
        i_idx, i_fl, i_code, i_sc, i_rew = self.ii["idx_x"], self.ii["flags"], self.ii["code"], self.ii["step_count"], self.ri["reward"]
        k0, k1 = self.seed & 0xffffffff, (self.seed >> 32) & 0xffffffff
        act = np.zeros(n, np.uint8)
        for _ in range(int(periods)):
            j = self.j
            _, ints = o.get_fields()
            s = ints[i_idx].copy(); was_done = (ints[i_fl] & 1) != 0
            words = {}
            for l in range(n):
                act[l] = 2
                if self.frozen[l] or was_done[l]:
                    continue
                r = orc.philox((j & 0xffffffff, (j >> 32) & 0xffffffff, l, STREAM_ACTION), (k0, k1))
                words[l] = r
                e = int(self.level_episodes[l])
                if (int(r[0]) >> 8) < self.thr[min(e, len(self.thr) - 1)]:
                    act[l] = (int(r[1]) * 3) >> 32
                else:
                    act[l] = int(orc.agent_predict(self.qa[l], self.qb[l], [int(s[l])])[0])
            o.step(act)
            for l, b in self.snap.items():
                o.envs[l * self.es:(l + 1) * self.es] = b
            reals, ints = o.get_fields()
            for l, r in words.items():
                a, ns = int(act[l]), int(ints[i_idx][l])
                sa = 3 * int(s[l]) + a
                c = int(self.cnt[l][sa])
                al = self.alpha[c] if c < len(self.alpha) else self.cfg.alpha_min
                self.updates_inside += c < len(self.alpha); self.updates_beyond += c >= len(self.alpha)
                done = bool(ints[i_fl][l] & 1)
                orc.agent_update(self.qa[l], self.qb[l], self.cnt[l], [sa], [ns], [al], self.cfg.gamma, [reals[i_rew][l]], quirks=self.cfg.quirks,
                                 coin=[int(r[2]) >> 31], done=[int(done)])
                self.decisions[l] += 1
                self.same_state += int(ns == int(s[l]))
                if done:
                    code = int(ints[i_code][l])
                    self.episodes[l] += 1; self.successes[l] += code == GOAL; self.by_code[code][l] += 1
                    if self.log_n[l] < self.cap:
                        self.log_code[l][self.log_n[l]] = code; self.log_len[l][self.log_n[l]] = int(ints[i_sc][l])
                    self.log_n[l] += 1
                    self.windows[l].append(int(code == GOAL)); self.level_episodes[l] += 1
                    if sum(self.windows[l]) >= self.min_successes:
                        self.promoted[l] = self.level_episodes[l]; self.frozen[l] = True
                    elif self.level_episodes[l] >= self.max_episodes:
                        self.frozen[l] = True
                    if self.frozen[l]:
                        self.freeze_period[l] = j
                        self.snap[l] = o.envs[l * self.es:(l + 1) * self.es].copy()
            self.j += 1

    def result(self):
        reals, ints = self.o.get_fields()
        out = {"qa": self.qa, "qb": self.qb, "count": self.cnt, "decisions": self.decisions, "episodes": self.episodes, "successes": self.successes,
               "by_code": self.by_code, "promotion_episode": self.promoted, "level_episodes": self.level_episodes, "frozen": self.frozen,
               "log_code": self.log_code, "log_len": self.log_len, "log_n": self.log_n}
        out.update({f: reals[k] for f, k in self.ri.items()})
        out.update({f: ints[k] for f, k in self.ii.items()})
        return {k: np.array(v, copy=True) for k, v in out.items()}


def ensemble_result(ens):
    """the same dictionary from a SequentialEnsemble"""
    qa, qb, cnt = ens.get_tables()
    out = {"qa": qa, "qb": qb, "count": cnt}
    out.update(ens.counters())
    code, length, n = ens.episode_log()
    out.update({"log_code": code, "log_len": length, "log_n": n})
    out.update(ens.state())
    return out


def assert_equal(got, want, what, learners=None):
    """`==` on every table, counter, log entry, promotion episode and state field (floats by their bits); `learners`: (rows of got, rows of want) to compare"""
    assert set(want) <= set(got), sorted(set(want) - set(got))
    for k, w in want.items():
        g = np.asarray(got[k]); w = np.asarray(w)
        if learners is not None:
            ax = 1 if k == "by_code" else 0
            g, w = np.take(g, learners[0], axis=ax), np.take(w, learners[1], axis=ax)
        assert g.shape == w.shape, f"{what}: {k} has shape {g.shape}, want {w.shape}"
        if w.dtype.kind == "f":
            bad = np.ascontiguousarray(g, np.float64).view(np.uint64) != np.ascontiguousarray(w, np.float64).view(np.uint64)
        else:
            bad = g.astype(np.int64) != w.astype(np.int64)
        assert not bad.any(), f"{what}: {k} differs in {np.count_nonzero(bad)} of {w.size} entries, first at {tuple(int(v[0]) for v in np.nonzero(bad))}: {g[bad][0]!r} vs {w[bad][0]!r}"


# ---- the long case shared by tests/test_gpu_ensemble_long.py and tests/test_learner_host_emulation.py ----
# 16 learners at level 0 with a promotion window of 72 episodes (two ring words), 28 successes to promote, 100 episodes at most, and 8 200 periods: three
# launches (4 096 + 4 096 + 8) in one call.  On the reference loop the learners fall into four classes, each of which takes another path through the ring.
RING_CASE = dict(eps=[0.3], window=72, min_successes=28, max_episodes=100, log_capacity=128)
RING_LEARNERS, RING_SEED, RING_PERIODS = 16, 11, 8200


def ring_classes(res):
    """learner masks by where the promotion ring stood when the learner froze: promoted with only word 0 written (episode <= 64), promoted by an episode
    written to word 1 (65 .. window), promoted after the ring wrapped and evicted (> window), out of episodes"""
    p, w = res["promotion_episode"], RING_CASE["window"]
    return {"word 0": (p >= 1) & (p <= 64), "word 1": (p >= 65) & (p <= w), "wrapped": p > w,
            "exhausted": (p < 0) & res["frozen"] & (res["level_episodes"] == RING_CASE["max_episodes"])}


def ring_reference(cfg):
    """(result, freeze periods) of the reference loop on the long case, after asserting ON IT that every path the case is for is taken"""
    ref = Reference(cfg, RING_LEARNERS, RING_SEED, **RING_CASE)
    ref.run(RING_PERIODS)
    want = ref.result()
    classes = ring_classes(want)
    print("ring case:", {k: int(v.sum()) for k, v in classes.items()}, "promotion episodes", want["promotion_episode"].tolist(), "largest visit count", want["count"].max())
    for name, m in classes.items():
        assert m.sum() >= 1, f"no learner of the class '{name}': {want['promotion_episode'].tolist()}"
    assert sum(int(m.sum()) for m in classes.values()) == RING_LEARNERS and want["frozen"].all()
    assert want["log_n"].max() == RING_CASE["max_episodes"] and want["log_n"].max() < RING_CASE["log_capacity"]
    # a learner flies one reset period per episode and one decision in every other period until it freezes: the identity the GPU test dates the waves with
    assert np.array_equal(ref.freeze_period, want["decisions"] + want["episodes"] - 1)
    # frozen in different periods, some in the first launch of 4 096 periods and some beyond it
    assert ref.freeze_period.min() < 4096 < ref.freeze_period.max() and len(set(ref.freeze_period.tolist())) == RING_LEARNERS
    return want, ref.freeze_period.copy()
