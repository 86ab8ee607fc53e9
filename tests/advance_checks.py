"""Shared by the per-learner curriculum tests (CPU emulation and GPU): the yardstick, the case and the `==` comparison.

`Yardstick` is the contract of curriculum mode spelled out with the unchanged oracle, in the spirit of `ensemble_checks.Reference`: ONE `Oracle(cfg_k, L, seed)`
per level k, all stepped every period (so their period indices agree); learner l's env lives in the oracle of ITS level.  At an advance point (a period index
that is a multiple of E, before that period is flown) a frozen learner below the last level that promoted — or ran out of episodes, where those advance —
records its history entry, has `oracle.transfer` applied to its own tables, and its env's bytes move to the next level's oracle with the done flag set (what
`Oracle.set_curriculum` does to the flags).  Tables are per-learner numpy arrays updated with `oracle.agent_update`; the freeze rule is a literal `deque` per
learner, emptied on advance.  Every comparison is `==`, floats by their bits (`ensemble_checks.assert_equal`), the history arrays included."""
import copy
import ctypes as C
from collections import deque

import numpy as np

from dql_multirotor_landing_amd import ensemble
from dql_multirotor_landing_amd.config import F32, N_CELLS, training_config
from oracle import oracle as orc
from oracle.oracle import Oracle

import ensemble_checks as ec

LEVELS = 5
CELLS_PER_LEVEL = N_CELLS // LEVELS
HISTORY = ("level", "promoted_at", "episodes_at", "entered_period")


class Yardstick:
    def __init__(self, cfg, n, seed, schedules, ratios, last_level, advance_every, advance_exhausted=True, log_capacity=64, tables=None):
        """schedules: per level 0..4 a dict(eps=, window=, min_successes=, max_episodes=); cfg: the config of the starting level; tables: initial (qa, qb,
        count), [n][N_CELLS] each (copied), default zeros"""
        self.cfg, self.n, self.seed = cfg, int(n), int(seed)
        self.start = int(cfg.working_curriculum_step)
        self.os = []
        for k in range(LEVELS):
            c = copy.deepcopy(cfg)
            c.working_curriculum_step = k
            self.os.append(Oracle(c, self.n, seed=self.seed))
        self.sched = [dict(thr=[ec.eps_thr(e) for e in s["eps"]], W=int(s["window"]), ms=int(s["min_successes"]), me=int(s["max_episodes"])) for s in schedules]
        self.ratios, self.last_level, self.E, self.advance_exhausted = [float(r) for r in ratios], int(last_level), int(advance_every), bool(advance_exhausted)
        self.qa, self.qb, self.cnt = (np.zeros((self.n, N_CELLS)) for _ in range(3)) if tables is None else (np.array(t, np.float64).reshape(self.n, N_CELLS) for t in tables)
        self.alpha = cfg.alpha_table()
        self.cap = int(log_capacity)
        self.j = 0
        self.decisions, self.episodes, self.successes = (np.zeros(self.n, np.int64) for _ in range(3))
        self.by_code = np.zeros((ec.N_CODES, self.n), np.int64)
        self.log_code = np.zeros((self.n, self.cap), np.uint8); self.log_len = np.zeros((self.n, self.cap), np.uint16); self.log_n = np.zeros(self.n, np.int32)
        o = self.os[0]
        rn, inn = o.field_names(False), o.field_names(True)
        self.ri = {f: rn.index(f) for f in ec.STATE_REAL_FIELDS}
        self.ii = {f: inn.index(f) for f in ec.STATE_INT_FIELDS}
        self.es = o.env_size
        self.level = np.full(self.n, self.start, np.int32)
        self.level_episodes = np.zeros(self.n, np.int32)
        self.windows = [deque([], maxlen=self.sched[self.start]["W"]) for _ in range(self.n)]
        self.promoted = np.full(self.n, -1, np.int32)
        self.frozen = np.zeros(self.n, bool)
        self.freeze_period = np.full(self.n, -1, np.int64)
        self.snap = {}
        self.promoted_at = np.full((LEVELS, self.n), -1, np.int32)
        self.episodes_at = np.zeros((LEVELS, self.n), np.int32)
        self.entered_period = np.full((LEVELS, self.n), -1, np.int64)
        self.entered_period[self.start] = 0
        # what the case's conditions are asserted on: per launch (period index, live learners per level, learners per level), and who advanced how
        self.launches = []
        self.advanced_promoted, self.advanced_exhausted = 0, 0
        self.promoted_from, self.exhausted_from = np.zeros(LEVELS, np.int64), np.zeros(LEVELS, np.int64)  # advances by the level they left
        self.wrap_sources = []       # per advance from level 0: (level-4 block of qa has a non-zero cell, the same of qb) before the transfer
        self.qb_blocks_moved = 0     # transfers whose source block of qb has a non-zero cell
        self.arrived_promoted = {}   # learner -> the level it promoted from, until its first episode at the next level ends
        self.first_failed_after_promotion = np.zeros(LEVELS, np.int64)  # by the level promoted from: that first episode was no success
        self.finished_by_promotion_beside_lower = 0  # learners that promoted at the last level while another learner stood below it

    def _slot(self, l):
        return slice(l * self.es, (l + 1) * self.es)

    def _mark_done(self, b):
        """the done flag of ONE env's bytes, through the oracle's own field access (Oracle.set_curriculum: ints[5] |= 1)"""
        o = self.os[0]
        nr, ni = o.n_fields()
        reals, ints = np.zeros((nr, 1), np.float64), np.zeros((ni, 1), np.int32)
        o._fn("get_fields")(orc._p(b), C.c_int64(1), orc._p(reals), orc._p(ints))
        ints[5] |= 1
        o._fn("set_fields")(orc._p(b), C.c_int64(1), orc._p(reals), orc._p(ints))

    def finished(self, l):
        return bool(self.frozen[l]) and (self.level[l] >= self.last_level or (self.promoted[l] < 0 and not self.advance_exhausted))

    def n_unfinished(self):
        return sum(not self.finished(l) for l in range(self.n))

    def advance(self):
        j = self.j
        for l in range(self.n):
            k = int(self.level[l])
            if not self.frozen[l] or k >= self.last_level:
                continue
            if self.promoted[l] < 0 and not self.advance_exhausted:
                continue
            if self.promoted[l] >= 0:
                self.advanced_promoted += 1; self.promoted_from[k] += 1; self.arrived_promoted[l] = k
            else:
                self.advanced_exhausted += 1; self.exhausted_from[k] += 1; self.arrived_promoted.pop(l, None)
            src = slice(((k - 1) % LEVELS) * CELLS_PER_LEVEL, ((k - 1) % LEVELS + 1) * CELLS_PER_LEVEL)
            if k == 0:
                self.wrap_sources.append((bool(self.qa[l][src].any()), bool(self.qb[l][src].any())))
            self.qb_blocks_moved += bool(self.qb[l][src].any())
            self.promoted_at[k][l] = self.promoted[l]; self.episodes_at[k][l] = self.level_episodes[l]
            orc.transfer(self.qa[l], self.qb[l], k, self.ratios[k])
            b = np.ascontiguousarray(self.snap.pop(l)).copy()
            self._mark_done(b)
            self.os[k + 1].envs[self._slot(l)] = b
            self.level[l] = k + 1; self.entered_period[k + 1][l] = j
            self.level_episodes[l] = 0; self.windows[l] = deque([], maxlen=self.sched[k + 1]["W"]); self.promoted[l] = -1; self.frozen[l] = False
            self.freeze_period[l] = -1

    def run(self, periods):
        n = self.n
        i_idx, i_fl, i_code, i_sc, i_rew = self.ii["idx_x"], self.ii["flags"], self.ii["code"], self.ii["step_count"], self.ri["reward"]
        k0, k1 = self.seed & 0xffffffff, (self.seed >> 32) & 0xffffffff
        first = True
        for _ in range(int(periods)):
            j = self.j
            if j % self.E == 0:
                self.advance()
            if j % self.E == 0 or first:
                live = [int(((self.level == k) & ~self.frozen).sum()) for k in range(LEVELS)]
                self.launches.append((j, live, [int((self.level == k).sum()) for k in range(LEVELS)]))
            first = False
            before = [o.get_fields()[1] for o in self.os]
            acts = [np.full(n, 2, np.uint8) for _ in range(LEVELS)]
            words, s = {}, {}
            for l in range(n):
                k = int(self.level[l])
                if self.frozen[l] or (before[k][i_fl][l] & 1) != 0:
                    continue
                r = orc.philox((j & 0xffffffff, (j >> 32) & 0xffffffff, l, ec.STREAM_ACTION), (k0, k1))
                words[l] = r
                s[l] = int(before[k][i_idx][l])
                thr = self.sched[k]["thr"]
                if (int(r[0]) >> 8) < thr[min(int(self.level_episodes[l]), len(thr) - 1)]:
                    acts[k][l] = (int(r[1]) * 3) >> 32
                else:
                    acts[k][l] = int(orc.agent_predict(self.qa[l], self.qb[l], [s[l]])[0])
            for k, o in enumerate(self.os):
                o.step(acts[k])
            for l, b in self.snap.items():
                self.os[int(self.level[l])].envs[self._slot(l)] = b
            after = [o.get_fields() for o in self.os]
            for l, r in words.items():
                k = int(self.level[l])
                reals, ints = after[k]
                a, ns = int(acts[k][l]), int(ints[i_idx][l])
                sa = 3 * s[l] + a
                c = int(self.cnt[l][sa])
                al = self.alpha[c] if c < len(self.alpha) else self.cfg.alpha_min
                done = bool(ints[i_fl][l] & 1)
                orc.agent_update(self.qa[l], self.qb[l], self.cnt[l], [sa], [ns], [al], self.cfg.gamma, [reals[i_rew][l]], quirks=self.cfg.quirks,
                                 coin=[int(r[2]) >> 31], done=[int(done)])
                self.decisions[l] += 1
                if done:
                    code = int(ints[i_code][l])
                    self.episodes[l] += 1; self.successes[l] += code == ec.GOAL; self.by_code[code][l] += 1
                    if self.log_n[l] < self.cap:
                        self.log_code[l][self.log_n[l]] = code; self.log_len[l][self.log_n[l]] = int(ints[i_sc][l])
                    self.log_n[l] += 1
                    self.windows[l].append(int(code == ec.GOAL)); self.level_episodes[l] += 1
                    if l in self.arrived_promoted:
                        self.first_failed_after_promotion[self.arrived_promoted.pop(l)] += code != ec.GOAL
                    if sum(self.windows[l]) >= self.sched[k]["ms"]:
                        self.promoted[l] = self.level_episodes[l]; self.frozen[l] = True
                        self.finished_by_promotion_beside_lower += k == self.last_level and bool((self.level < self.last_level).any())
                    elif self.level_episodes[l] >= self.sched[k]["me"]:
                        self.frozen[l] = True
                    if self.frozen[l]:
                        self.freeze_period[l] = j
                        self.snap[l] = self.os[k].envs[self._slot(l)].copy()
            self.j += 1

    def result(self):
        fields = [o.get_fields() for o in self.os]
        lv = self.level.astype(int)
        idx = np.arange(self.n)
        out = {"qa": self.qa, "qb": self.qb, "count": self.cnt, "decisions": self.decisions, "episodes": self.episodes, "successes": self.successes,
               "by_code": self.by_code, "promotion_episode": self.promoted, "level_episodes": self.level_episodes, "frozen": self.frozen,
               "log_code": self.log_code, "log_len": self.log_len, "log_n": self.log_n, "level": self.level, "entered_period": self.entered_period}
        out.update({f: np.stack([fields[k][0][i] for k in range(LEVELS)])[lv, idx] for f, i in self.ri.items()})
        out.update({f: np.stack([fields[k][1][i] for k in range(LEVELS)])[lv, idx] for f, i in self.ii.items()})
        pa, ea = self.promoted_at.copy(), self.episodes_at.copy()
        pa[lv, idx] = self.promoted; ea[lv, idx] = self.level_episodes  # the current level's row shows the counters as they stand
        out["promoted_at"], out["episodes_at"] = pa, ea
        return {k: np.array(v, copy=True) for k, v in out.items()}


def ensemble_result(ens):
    """`ensemble_checks.ensemble_result` plus the per-level history"""
    out = ec.ensemble_result(ens)
    out.update(ens.levels())
    return out


def assert_equal(got, want, what, learners=None):
    """`ensemble_checks.assert_equal`; the history arrays are [level][learner], so a learner subset is taken along their second axis"""
    hist = ("promoted_at", "episodes_at", "entered_period")
    ec.assert_equal({k: v for k, v in got.items() if k not in hist}, {k: v for k, v in want.items() if k not in hist}, what, learners)
    for k in hist:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if learners is not None:
            g, w = g[:, learners[0]], w[:, learners[1]]
        assert g.shape == w.shape and np.array_equal(g.astype(np.int64), w.astype(np.int64)), f"{what}: {k} differs: {g.tolist()} vs {w.tolist()}"


# ---- the case shared by tests/test_gpu_ensemble_advance.py and tests/test_advance_host_emulation.py ----
# From the CURRICULUM case of tests/test_gpu_ensemble_long.py: the reference's quirks at level 0, a promotion window of 4 episodes, success rate 0.5 (3
# successes), 6 episodes at level 0 — and ONE episode per level above it, so that within 1 024 periods learners reach and finish level 4 while others are still
# at level 2, and a level between two populated ones runs empty (settled on the yardstick: with 6 episodes at every level no learner passes level 3 in
# 1 024 periods and no level runs empty).  80 learners, E = 64: 16 advance points, two waves at level 0, padded segments everywhere.
CASE = dict(n=80, seed=11, E=64, periods=1024, window=4, success_rate=0.5, max_episodes=(6, 1, 1, 1, 1), last_level=4, log_capacity=64)
SMALL = 24  # the first learners of the case as an ensemble of their own (and the host emulation's size)
# A second, smaller case for the window ring: a budget of 3 episodes above level 0, where ONE success in the window promotes.  A learner arrives at level 1
# with successes of level 0 in its ring (three where it promoted, often one or two where it ran out of episodes): a ring that is not cleared on advance
# promotes it at the end of its first episode there, the yardstick's emptied deque does not.  (Settled on the yardstick: no learner lands at level 1 or above
# within these 768 periods, with 6 episodes per level and one success asked for neither, so no affordable case has a PROMOTED advance above level 0.)
RING_CASE = dict(CASE, n=SMALL, periods=768, max_episodes=(6, 3, 3, 3, 3), min_successes=(None, 1, 1, 1, 1))


# Two cases that start from TRAINED tables (`ensemble_checks.trained_tables`: the reference's stage-4 tables, perturbed per learner, the stored visit counts):
# greedy at every level, learners land, so they promote through the ring above level 0, the transfer moves non-zero blocks of BOTH tables, and the k = 0 wrap
# reads a level-4 block that is not zero.  TRAINED_CASE's ratios are not the reference's and hold no 1.0, so every ratio shows in the tables, ratios[0]
# included.  E = 32: 32 advance points in 1 024 periods; 80 learners are two waves at level 0.  Quirks 0x7f (table A alone is updated, learners also run out of
# episodes) or 0x40 (the coin: both tables are updated).
TRAINED_RATIOS = (0.75, 0.5, 1.25, 0.625, 0.875)
TRAINED_CASE = dict(n=80, seed=11, E=32, periods=1024, window=2, min_successes=(1,) * 5, max_episodes=(3,) * 5, eps=((0.0,),) * 5, last_level=4, log_capacity=64,
                    start_level=0, quirks=ec.Q_REFERENCE, ratios=TRAINED_RATIOS, trained=True)
TRAINED_CASE_PAPER = dict(TRAINED_CASE, quirks=ec.Q_PAPER)
# An ensemble CREATED at level 3 (the config's level is the starting level), the reference's ratios: someone finishes at level 4 by promotion while others are
# still at level 3 (settled on the yardstick: the first learner to do so promotes at level 4 between periods 1 024 and 1 280).
TRAINED_FROM_3 = dict(TRAINED_CASE, n=SMALL, periods=1280, window=4, min_successes=(2,) * 5, max_episodes=(6,) * 5, start_level=3, ratios=ensemble.REFERENCE_RATIOS)


def level0(dtype=F32):
    return training_config(0, quirks=ec.Q_REFERENCE, dtype=dtype)


def case_config(case=CASE, dtype=F32):
    """the config of the case's starting level with the case's quirks (default: level 0, the reference's quirks)"""
    return training_config(case.get("start_level", 0), quirks=case.get("quirks", ec.Q_REFERENCE), dtype=dtype)


def case_ratios(case=CASE):
    return tuple(case.get("ratios", ensemble.REFERENCE_RATIOS))


def case_tables(case, n):
    """the case's initial (qa, qb, count) for n learners, or None where it starts from zeros"""
    return ec.trained_tables(n) if case.get("trained") else None


def case_schedules(case=CASE):
    own = case.get("min_successes", (None,) * LEVELS)  # a level's own figure where the case names one
    ms = None if all(m is not None for m in own) else ensemble.min_successes_for(case["window"], case["success_rate"])
    eps = case.get("eps", (None,) * LEVELS)  # a level's own exploration table where the case names one
    return [dict(eps=ensemble.exploration_rates(k) if eps[k] is None else np.asarray(eps[k], np.float64), window=case["window"],
                 min_successes=ms if own[k] is None else own[k], max_episodes=case["max_episodes"][k]) for k in range(LEVELS)]


def case_yardstick(dtype=F32, n=None, periods=None, checkpoint_every=None, **over):
    """the yardstick flown through the case; -> the Yardstick (its result(), launches and advance counts).  checkpoint_every: fly in runs of that many periods
    and keep, after each, (period index, n_unfinished(), what `SequentialEnsemble.levels()` shows) in `y.checkpoints`"""
    c = dict(CASE, **over)
    n = c["n"] if n is None else n
    y = Yardstick(case_config(c, dtype), n, c["seed"], case_schedules(c), case_ratios(c), c["last_level"], c["E"], c.get("advance_exhausted", True),
                  c["log_capacity"], tables=case_tables(c, n))
    periods = c["periods"] if periods is None else periods
    if checkpoint_every is None:
        y.run(periods)
        return y
    assert periods % checkpoint_every == 0
    y.checkpoints = []
    for _ in range(periods // checkpoint_every):
        y.run(checkpoint_every)
        r = y.result()
        y.checkpoints.append((y.j, y.n_unfinished(), {k: r[k] for k in ("level",) + HISTORY[1:]}))
    return y


def case_ensemble(n=None, dtype=F32, **over):
    """a SequentialEnsemble set up for the case (curriculum mode on), not yet run"""
    from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
    c = dict(CASE, **over)
    n = c["n"] if n is None else n
    ens = SequentialEnsemble(case_config(c, dtype), n, seed=c["seed"], log_capacity=c["log_capacity"])
    for k, s in enumerate(case_schedules(c)):
        ens.set_level_schedules(k, s["eps"], s["window"], s["min_successes"], s["max_episodes"])
    ens.set_curriculum(c["last_level"], c["E"], case_ratios(c), c.get("advance_exhausted", True))
    tables = case_tables(c, n)
    if tables is not None:
        ens.set_tables(*tables)
    return ens


def assert_case_conditions(y):
    """what the case is for, asserted ON THE YARDSTICK before an ensemble is looked at"""
    print("launches (period, live per level, learners per level):", y.launches)
    print("advanced promoted", y.advanced_promoted, "exhausted", y.advanced_exhausted, "levels at the end", np.bincount(y.level, minlength=LEVELS).tolist(),
          "finished", sum(y.finished(l) for l in range(y.n)))
    points = [(j, live, allv) for j, live, allv in y.launches if j % y.E == 0]
    assert any(sum(1 for c in allv if c > 0) >= 3 for _, _, allv in points), "learners never stand on three levels at once at an advance point"
    assert any(c > 64 for _, live, _ in y.launches for c in live), "no level ever holds more than 64 live learners (two waves of one level)"
    assert any(c % 64 != 0 for _, live, _ in y.launches for c in live), "no padded segment"

    def gap(live):
        pop = [k for k, c in enumerate(live) if c > 0]
        return len(pop) >= 2 and any(live[k] == 0 for k in range(pop[0], pop[-1]))
    assert any(gap(live) for _, live, _ in y.launches), "never an empty level between two populated ones"
    assert y.advanced_promoted >= 1 and y.advanced_exhausted >= 1, "both ways of advancing are needed"
    at_last = [l for l in range(y.n) if y.frozen[l] and y.level[l] == y.last_level]
    assert at_last and (y.level < y.last_level).any(), "someone finished at the last level while others are still below it"


def assert_ring_case_conditions(y, want):
    """RING_CASE on the yardstick: learners reach level 1 and above with level-0 successes behind them, promoted ones and exhausted ones, and nobody promotes there"""
    up = want["level"] >= 1
    print("levels at the end", np.bincount(y.level, minlength=LEVELS).tolist(), "advanced promoted", y.advanced_promoted, "exhausted", y.advanced_exhausted,
          "successes of the learners above level 0", want["successes"][up].tolist())
    assert y.advanced_promoted >= 1 and (up & (want["promoted_at"][0] < 0) & (want["successes"] >= 1)).any(), "nobody carries successes into level 1"
    assert (want["episodes_at"][1][want["level"] >= 2] == 3).all() and (want["level"] >= 2).any(), "a learner left level 1 before its budget ran out"
    assert (want["promoted_at"][1:] == -1).all()


def assert_trained_case_conditions(y, case):
    """what TRAINED_CASE / TRAINED_FROM_3 are for, asserted ON THE YARDSTICK before an ensemble or an emulation is looked at"""
    start = int(case.get("start_level", 0))
    print("promoted advances by level left", y.promoted_from.tolist(), "exhausted", y.exhausted_from.tolist(), "levels at the end", np.bincount(y.level, minlength=LEVELS).tolist(),
          "advances from level 0 (qa, qb level-4 block non-zero)", len(y.wrap_sources), "transfers of a non-zero qb block", y.qb_blocks_moved,
          "failed first episodes after a promotion, by level left", y.first_failed_after_promotion.tolist(), "promoted at the last level beside lower learners",
          y.finished_by_promotion_beside_lower, "unfinished", y.n_unfinished())
    assert len(set(case_ratios(case))) == LEVELS or start > 0, "two levels share a ratio: one taken for the other would not show"
    if start == 0:
        assert 1.0 not in case_ratios(case), "a ratio of 1.0 does not show in the tables"
        assert y.promoted_from[0] >= 1 and (y.promoted_from[1:] > 0).sum() >= 2, "promoted advances at level 0 and at two levels above it are needed"
        assert y.wrap_sources and all(a and b for a, b in y.wrap_sources), "an advance from level 0 reads a level-4 block of zeros"
    else:
        assert y.promoted_from[start] >= 1 and not y.promoted_from[:start].any() and (y.entered_period[:start] == -1).all()
    assert y.qb_blocks_moved >= 1, "no transfer moves a non-zero block of Q_table_b"
    assert y.first_failed_after_promotion[1:].sum() >= 1, "no promoted advance from a level >= 1 is followed by a failed first episode: an uncleared ring would not show"
    assert y.finished_by_promotion_beside_lower >= 1, "nobody finishes at the last level by promotion while others are below it"
    if case["quirks"] == ec.Q_REFERENCE:
        assert y.advanced_exhausted >= 1 and y.advanced_promoted >= 1, "both ways of advancing are needed"
    else:
        assert (y.qb != case_tables(case, y.n)[1])[:, start * CELLS_PER_LEVEL:(start + 1) * CELLS_PER_LEVEL].any(), "the coin never picked Q_table_b"
    if y.n > 64:
        assert any(c > 64 for _, live, _ in y.launches for c in live), "no level ever holds more than 64 live learners (two waves of one level)"
        assert any(c % 64 != 0 for _, live, _ in y.launches for c in live), "no padded segment"
