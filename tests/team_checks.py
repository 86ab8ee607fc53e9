"""Shared by the team-ensemble tests (CPU emulation and GPU): the reference loop for learners that own E envs, the events it counts, and the cases.

`TeamReference` stands beside `ensemble_checks.Reference` and is the team ensemble's equality contract spelled out with the unchanged oracle: ONE
`Oracle(cfg, L * E, seed)` stepped with external actions, env g's action word from `oracle.philox((j_lo, j_hi, g, STREAM_ACTION), seed)`, the greedy choice from
`oracle.agent_predict` on learner `g // E`'s tables BEFORE the step, and after the step, for g ascending, `oracle.agent_update` on those shared tables — so
the row of s' and the visit count are whatever the updates of the envs before g left — with a literal `deque` per learner.  Once a learner's level is decided
in a period, episodes its later envs finish in that period go to the totals and the log only; the learner freezes at the period's end and its E envs are put
back to their bytes at that point after every later oracle step.

The reference counts, per run, the events a kernel can get wrong (`events`); every case asserts on them before anything else is looked at."""
from collections import deque

import numpy as np

from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, training_config
from oracle import oracle as orc
from oracle.oracle import Oracle

import ensemble_checks as ec

TEAM_SIZES = (1, 2, 4, 8, 16, 32, 64)
EVENTS = ("same_cell", "next_row_after_write", "greedy_row_written", "multi_end_periods", "mid_period_decisions", "episodes_after_decision")


class TeamReference:
    def __init__(self, cfg, n_learners, envs_per_learner, seed, eps=ec.EPS_TABLE, window=100, min_successes=97, max_episodes=1 << 30, log_capacity=64, alpha_tab=None,
                 tables=None):
        """tables: initial (qa, qb, count), [n_learners][N_CELLS] each (copied); default zeros"""
        self.cfg, self.n, self.E, self.seed = cfg, int(n_learners), int(envs_per_learner), int(seed)
        assert self.E in TEAM_SIZES
        self.n_envs = self.n * self.E
        self.o = Oracle(cfg, self.n_envs, seed=self.seed)
        self.qa, self.qb, self.cnt = (np.zeros((self.n, N_CELLS)) for _ in range(3)) if tables is None else (np.array(t, np.float64).reshape(self.n, N_CELLS) for t in tables)
        self.alpha = cfg.alpha_table() if alpha_tab is None else np.asarray(alpha_tab, np.float64)
        self.thr = [ec.eps_thr(e) for e in eps]
        self.W, self.min_successes, self.max_episodes, self.cap = int(window), int(min_successes), int(max_episodes), int(log_capacity)
        self.j = 0
        self.events = dict.fromkeys(EVENTS, 0)
        self.learners_with_episodes_after_decision = set()
        self.decisions, self.episodes, self.successes = (np.zeros(self.n, np.int64) for _ in range(3))
        self.by_code = np.zeros((ec.N_CODES, self.n), np.int64)
        self.log_code = np.zeros((self.n, self.cap), np.uint8); self.log_len = np.zeros((self.n, self.cap), np.uint16); self.log_n = np.zeros(self.n, np.int32)
        rn, inn = self.o.field_names(False), self.o.field_names(True)
        self.ri = {f: rn.index(f) for f in ec.STATE_REAL_FIELDS}
        self.ii = {f: inn.index(f) for f in ec.STATE_INT_FIELDS}
        self.es = self.o.env_size
        self.written = [dict() for _ in range(self.n)]  # per learner: state -> envs that wrote its row in the period before
        self.rearm()

    def rearm(self):
        self.level_episodes = np.zeros(self.n, np.int32)
        self.windows = [deque([], maxlen=self.W) for _ in range(self.n)]
        self.promoted = np.full(self.n, -1, np.int32)
        self.frozen = np.zeros(self.n, bool)
        self.freeze_period = np.full(self.n, -1, np.int64)
        self.snap = {}

    def set_schedules(self, eps, window, min_successes, max_episodes):
        self.thr = [ec.eps_thr(e) for e in eps]
        if int(window) != self.W:
            assert all(len(w) == 0 for w in self.windows), "the window length changes with outcomes in a deque"
            self.W = int(window)
            self.windows = [deque([], maxlen=self.W) for _ in range(self.n)]
        self.min_successes, self.max_episodes = int(min_successes), int(max_episodes)

    def set_level(self, k):
        for g, b in self.snap.items():  # the frozen envs as they were left, then every env re-enters through reset
            self.o.envs[g * self.es:(g + 1) * self.es] = b
        self.o.set_curriculum(k)
        self.rearm()

    def transfer(self, k, ratio):
        for l in range(self.n):
            orc.transfer(self.qa[l], self.qb[l], k, ratio)

    def run(self, periods):
        o, E, ev = self.o, self.E, self.events
        i_idx, i_fl, i_code, i_sc, i_rew = self.ii["idx_x"], self.ii["flags"], self.ii["code"], self.ii["step_count"], self.ri["reward"]
        k0, k1 = self.seed & 0xffffffff, (self.seed >> 32) & 0xffffffff
        act = np.zeros(self.n_envs, np.uint8)
        for _ in range(int(periods)):
            j = self.j
            _, ints = o.get_fields()
            s = ints[i_idx].copy(); was_done = (ints[i_fl] & 1) != 0
            words = {}
            for l in range(self.n):
                act[l * E:(l + 1) * E] = 2
                if self.frozen[l]:
                    continue
                thr = self.thr[min(int(self.level_episodes[l]), len(self.thr) - 1)]  # one threshold per learner and period
                for g in range(l * E, (l + 1) * E):
                    if was_done[g]:
                        continue
                    r = orc.philox((j & 0xffffffff, (j >> 32) & 0xffffffff, g, ec.STREAM_ACTION), (k0, k1))
                    words[g] = r
                    ev["greedy_row_written"] += any(w != g for w in self.written[l].get(int(s[g]), ()))
                    if (int(r[0]) >> 8) < thr:
                        act[g] = (int(r[1]) * 3) >> 32
                    else:
                        act[g] = int(orc.agent_predict(self.qa[l], self.qb[l], [int(s[g])])[0])
            o.step(act)
            for g, b in self.snap.items():
                o.envs[g * self.es:(g + 1) * self.es] = b
            reals, ints = o.get_fields()
            for l in range(self.n):
                if self.frozen[l]:
                    continue
                mine = [g for g in range(l * E, (l + 1) * E) if g in words]
                cells, rows, ended, decided, decided_at = set(), {}, 0, False, None
                for g in mine:  # env order
                    r = words[g]
                    a, ns = int(act[g]), int(ints[i_idx][g])
                    sa = 3 * int(s[g]) + a
                    c = int(self.cnt[l][sa])
                    al = self.alpha[c] if c < len(self.alpha) else self.cfg.alpha_min
                    done = bool(ints[i_fl][g] & 1)
                    ev["same_cell"] += sa in cells
                    ev["next_row_after_write"] += ns in rows
                    if decided and decided_at is not None:
                        ev["mid_period_decisions"] += 1
                        decided_at = None
                    orc.agent_update(self.qa[l], self.qb[l], self.cnt[l], [sa], [ns], [al], self.cfg.gamma, [reals[i_rew][g]], quirks=self.cfg.quirks,
                                     coin=[int(r[2]) >> 31], done=[int(done)])
                    cells.add(sa); rows.setdefault(int(s[g]), []).append(g)
                    self.decisions[l] += 1
                    if done:
                        ended += 1
                        code = int(ints[i_code][g])
                        self.episodes[l] += 1; self.successes[l] += code == ec.GOAL; self.by_code[code][l] += 1
                        if self.log_n[l] < self.cap:
                            self.log_code[l][self.log_n[l]] = code; self.log_len[l][self.log_n[l]] = int(ints[i_sc][g])
                        self.log_n[l] += 1
                        if decided:  # the level is decided: totals and log only
                            ev["episodes_after_decision"] += 1
                            self.learners_with_episodes_after_decision.add(l)
                            continue
                        self.windows[l].append(int(code == ec.GOAL)); self.level_episodes[l] += 1
                        if sum(self.windows[l]) >= self.min_successes:
                            self.promoted[l] = self.level_episodes[l]; decided = True
                        elif self.level_episodes[l] >= self.max_episodes:
                            decided = True
                        if decided:
                            decided_at = g
                ev["multi_end_periods"] += ended >= 2
                self.written[l] = rows
                if decided:  # frozen at the period's end: all E updates applied, all E envs as they are now
                    self.frozen[l] = True
                    self.freeze_period[l] = j
                    for g in range(l * E, (l + 1) * E):
                        self.snap[g] = o.envs[g * self.es:(g + 1) * self.es].copy()
            self.j += 1

    def result(self):
        reals, ints = self.o.get_fields()
        out = {"qa": self.qa, "qb": self.qb, "count": self.cnt, "decisions": self.decisions, "episodes": self.episodes, "successes": self.successes,
               "by_code": self.by_code, "promotion_episode": self.promoted, "level_episodes": self.level_episodes, "frozen": self.frozen,
               "log_code": self.log_code, "log_len": self.log_len, "log_n": self.log_n}
        out.update({f: reals[k] for f, k in self.ri.items()})
        out.update({f: ints[k] for f, k in self.ii.items()})
        return {k: np.array(v, copy=True) for k, v in out.items()}


PER_ENV = ec.STATE_REAL_FIELDS + ec.STATE_INT_FIELDS


def assert_equal(got, want, what, learners=None, envs_per_learner=1):
    """`ensemble_checks.assert_equal`; `learners`: (rows of got, rows of want) for the per-learner entries — the per-env entries take those learners' envs"""
    if learners is None:
        return ec.assert_equal(got, want, what)
    E = int(envs_per_learner)
    envs = tuple([l * E + k for l in rows for k in range(E)] for rows in learners)
    ec.assert_equal({k: v for k, v in got.items() if k not in PER_ENV}, {k: v for k, v in want.items() if k not in PER_ENV}, what, learners=learners)
    ec.assert_equal({k: got[k] for k in PER_ENV}, {k: want[k] for k in PER_ENV}, what, learners=envs)


# ---- the cases (seed 11, training_config(level, quirks)): shape, schedules, and what the reference must show before a case is worth comparing ----
SEED = 11
CASES = {
    # every hazard of the serial section at full team width, all five learners promoting in the middle of a period
    "A": dict(level=0, quirks=ec.Q_REFERENCE, trained=False, L=5, E=64, periods=200, dtypes=(F32,),
              sched=dict(eps=[1.0, 0.5, 0.1], window=8, min_successes=3, max_episodes=40, log_capacity=64),
              need=dict(same_cell=100, next_row_after_write=100, greedy_row_written=100, multi_end_periods=1, mid_period_decisions=1), promoted="all"),
    # the coin and non-trivial rows at level 4, both dtypes
    "B": dict(level=4, quirks=ec.Q_PAPER, trained=True, L=10, E=16, periods=300, dtypes=(F32, F64),
              sched=dict(eps=[0.0], window=8, min_successes=6, max_episodes=40, log_capacity=64),
              need=dict(same_cell=100, next_row_after_write=100, greedy_row_written=100, multi_end_periods=1, mid_period_decisions=1), both_tables=True),
    # 160 envs: the third wave half filled; frozen teams beside live ones in one wave
    "C": dict(level=2, quirks=ec.Q_REFERENCE, trained=True, L=40, E=4, periods=300, dtypes=(F32,),
              sched=dict(eps=[0.0], window=4, min_successes=3, max_episodes=10, log_capacity=32),
              need=dict(same_cell=1, next_row_after_write=1, greedy_row_written=1), promoted="some", live="some"),
    # a budget of 3 episodes against up to a dozen ending in the deciding period: the "totals only" path
    "D": dict(level=0, quirks=ec.Q_REFERENCE, trained=False, L=5, E=64, periods=120, dtypes=(F32,),
              sched=dict(eps=[1.0], window=8, min_successes=8, max_episodes=3, log_capacity=64),
              need=dict(episodes_after_decision=3, multi_end_periods=1), after_decision_learners=2),
    # window 72: promotions out of the second ring word, exhausted learners
    "E": dict(level=0, quirks=ec.Q_PAPER, trained=False, L=6, E=32, periods=400, dtypes=(F32,),
              sched=dict(eps=[0.3], window=72, min_successes=28, max_episodes=100, log_capacity=128),
              need=dict(multi_end_periods=10, same_cell=100), second_word=True),
    "F": dict(level=4, quirks=ec.Q_PAPER, trained=True, L=9, E=8, periods=300, dtypes=(F32,),
              sched=dict(eps=[0.0], window=4, min_successes=4, max_episodes=9, log_capacity=32),
              need=dict(same_cell=1, next_row_after_write=1, greedy_row_written=1), promoted="some"),
    "F2": dict(level=4, quirks=ec.Q_PAPER, trained=True, L=9, E=2, periods=300, dtypes=(F32,),
               sched=dict(eps=[0.0], window=4, min_successes=4, max_episodes=9, log_capacity=32),
               need=dict(greedy_row_written=1), promoted="some"),
}
CASE_IDS = [(name, dt) for name, c in CASES.items() for dt in c["dtypes"]]


def case_config(name, dtype):
    c = CASES[name]
    return training_config(c["level"], quirks=c["quirks"], dtype=dtype)


def case_tables(name):
    c = CASES[name]
    return ec.trained_tables(c["L"]) if c["trained"] else None


_cache = {}


def case_reference(name, dtype, periods=None):
    """(result, TeamReference) of a case on the reference loop — computed once per process and never changed — after asserting ON IT what the case is for"""
    key = (name, dtype, periods)
    if key in _cache:
        return _cache[key]
    c = CASES[name]
    tables = case_tables(name)
    ref = TeamReference(case_config(name, dtype), c["L"], c["E"], SEED, tables=tables, **c["sched"])
    ref.run(c["periods"] if periods is None else periods)
    want = ref.result()
    promoted = want["promotion_episode"] >= 0
    print(f"case {name} dtype {dtype}: events {ref.events}, promoted {int(promoted.sum())} of {c['L']} at {want['promotion_episode'].tolist()}, live {int((~want['frozen']).sum())},"
          f" episodes {want['episodes'].tolist()}, learners with episodes after the decision {sorted(ref.learners_with_episodes_after_decision)}")
    if periods is None:
        for k, v in c["need"].items():
            assert ref.events[k] >= v, f"case {name}: {k} occurred {ref.events[k]} times on the reference, {v} are needed"
        if c.get("promoted") == "all":
            assert promoted.all()
        if c.get("promoted") == "some":
            assert promoted.any()
        if c.get("live") == "some":
            assert (~want["frozen"]).any() and want["frozen"].any(), "frozen teams beside live ones are needed"
        if c.get("both_tables"):
            assert (want["qa"] != tables[0]).any() and (want["qb"] != tables[1]).any(), "under the coin both tables are to be written"
        if c.get("after_decision_learners"):
            assert len(ref.learners_with_episodes_after_decision) >= c["after_decision_learners"]
            assert (want["episodes"] > want["level_episodes"]).any() and (want["level_episodes"] <= c["sched"]["max_episodes"]).all()
        if c.get("second_word"):
            p = want["promotion_episode"]
            assert ((p > 64) & (p <= 72)).any() and ((p >= 1) & (p <= 64)).any(), f"promotions out of both ring words are needed: {p.tolist()}"
            assert ((p < 0) & want["frozen"]).any(), "a learner out of episodes is needed"
        assert (want["level_episodes"] <= c["sched"]["max_episodes"]).all() and (want["promotion_episode"] <= c["sched"]["max_episodes"]).all()
    _cache[key] = (want, ref)
    return _cache[key]
