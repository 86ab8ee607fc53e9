"""Shared by the team-curriculum tests (CPU emulation and GPU): the yardstick, the cases and the `==` comparison.

`TeamLevelsYardstick` is the contract of `SequentialEnsemble.set_team_curriculum` spelled out with the unchanged oracle.  It has `advance_checks.Yardstick`'s
structure: ONE `Oracle(cfg_k, L * E, seed)` per level k, all stepped every period (so their period indices agree); team l's E envs live in the oracle of ITS
level.  At an advance point (a period index that is a multiple of `advance_every`, before that period is flown) a frozen team below the last level that
promoted — or ran out of episodes, where those advance — records its history entry, has `oracle.transfer` applied to its own tables (order 0: of level k with
ratios[k]; order 1: of level k + 1 with ratios[k + 1]), its E envs' byte blocks move to the next level's oracle with the done flag set, and its envs' pending
windows are emptied.  In between it runs `team_checks.TeamReference`'s period: one threshold per team and period, the greedy choice from `oracle.agent_predict`
on the team's tables before the step, then for the team's envs in env order `oracle.agent_update` (nstep 0) or `team_nstep_checks.TeamNstepReference`'s
literal per-env windows and its `_update`, called as it stands (nstep >= 1); a level once decided takes no further outcome into its ring in that period; the
team freezes at the period's end.  Every comparison is `==`, floats by their bits.  It knows nothing of the kernels."""
import copy
import ctypes as C
from collections import Counter, deque

import numpy as np

from dql_multirotor_landing_amd import ensemble
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_BOOTSTRAP_ON_POS_CHANGE as Q_POS_CHANGE, training_config
from oracle import oracle as orc
from oracle.oracle import Oracle

import advance_checks as ac
import ensemble_checks as ec
import team_checks as tc
import team_nstep_checks as tn

LEVELS = ac.LEVELS
HISTORY = ac.HISTORY


class TeamLevelsYardstick:
    def __init__(self, cfg, n_teams, envs_per_team, seed, schedules, ratios, last_level, advance_every, advance_exhausted=True, transfer_order=0, nstep=0,
                 log_capacity=64, tables=None):
        """schedules: per level 0..4 a dict(eps=, window=, min_successes=, max_episodes=); cfg: the config of the starting level; nstep: 0 for the one-step
        update, 1..16 for the per-env windows; tables: initial (qa, qb, count), [n_teams][N_CELLS] each (copied), default zeros"""
        self.cfg, self.n, self.E, self.seed = cfg, int(n_teams), int(envs_per_team), int(seed)
        assert self.E in tc.TEAM_SIZES and 0 <= int(nstep) <= tn.NSTEP_MAX and transfer_order in (0, 1)
        self.n_envs = self.n * self.E
        self.start = int(cfg.working_curriculum_step)
        self.os = []
        for k in range(LEVELS):
            c = copy.deepcopy(cfg)
            c.working_curriculum_step = k
            self.os.append(Oracle(c, self.n_envs, seed=self.seed))
        self.sched = [dict(thr=[ec.eps_thr(e) for e in s["eps"]], W=int(s["window"]), ms=int(s["min_successes"]), me=int(s["max_episodes"])) for s in schedules]
        self.ratios, self.last_level, self.every = [float(r) for r in ratios], int(last_level), int(advance_every)
        self.advance_exhausted, self.order, self.nstep = bool(advance_exhausted), int(transfer_order), int(nstep)
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
        self.snap = {}  # env -> its bytes at the period's end in which its team froze
        self.promoted_at = np.full((LEVELS, self.n), -1, np.int32)
        self.episodes_at = np.zeros((LEVELS, self.n), np.int32)
        self.entered_period = np.full((LEVELS, self.n), -1, np.int64)
        self.entered_period[self.start] = 0
        # what TeamNstepReference._update reads and keeps beside the tables: the windows, its event counts and its write stamps
        self.win = [[] for _ in range(self.n_envs)]
        self.events = Counter()
        self.stamp = np.zeros(self.n, np.int64)
        self.last_write = [dict() for _ in range(self.n)]
        # what the cases' conditions are asserted on
        self.launches = []           # per launch (period index, live teams per level, teams per level)
        self.advanced_promoted, self.advanced_exhausted = 0, 0
        self.promoted_from, self.exhausted_from = np.zeros(LEVELS, np.int64), np.zeros(LEVELS, np.int64)
        self.advanced_mid_episode = 0        # advances with at least one env of the team in the middle of an episode (step_count > 0, not done)
        self.advanced_with_open_windows = 0  # advances that dropped at least one pending entry
        self.dropped_entries = 0
        self.nonzero_blocks_moved = 0        # transfers whose source block of both tables has a non-zero cell
        self.finished_by_promotion_beside_lower = 0

    def _env(self, g):
        return slice(g * self.es, (g + 1) * self.es)

    def _fields_of(self, b):
        o = self.os[0]
        nr, ni = o.n_fields()
        reals, ints = np.zeros((nr, 1), np.float64), np.zeros((ni, 1), np.int32)
        o._fn("get_fields")(orc._p(b), C.c_int64(1), orc._p(reals), orc._p(ints))
        return reals, ints

    def _mark_done(self, b):
        """the done flag of ONE env's bytes, through the oracle's own field access (Oracle.set_curriculum: ints[5] |= 1); -> whether the env was mid-episode"""
        reals, ints = self._fields_of(b)
        mid = int(ints[self.ii["step_count"]][0]) > 0 and not (int(ints[self.ii["flags"]][0]) & 1)
        ints[5] |= 1
        self.os[0]._fn("set_fields")(orc._p(b), C.c_int64(1), orc._p(reals), orc._p(ints))
        return mid

    def finished(self, l):
        return bool(self.frozen[l]) and (self.level[l] >= self.last_level or (self.promoted[l] < 0 and not self.advance_exhausted))

    def n_unfinished(self):
        return sum(not self.finished(l) for l in range(self.n))

    def pending_lengths(self):
        return np.array([len(w) for w in self.win], np.int32)

    def advance(self):
        j, E = self.j, self.E
        for l in range(self.n):
            k = int(self.level[l])
            if not self.frozen[l] or k >= self.last_level:
                continue
            if self.promoted[l] < 0 and not self.advance_exhausted:
                continue
            if self.promoted[l] >= 0:
                self.advanced_promoted += 1; self.promoted_from[k] += 1
            else:
                self.advanced_exhausted += 1; self.exhausted_from[k] += 1
            self.promoted_at[k][l] = self.promoted[l]; self.episodes_at[k][l] = self.level_episodes[l]
            dst = k + 1 if self.order == 1 else k
            src = slice(((dst - 1) % LEVELS) * ac.CELLS_PER_LEVEL, ((dst - 1) % LEVELS + 1) * ac.CELLS_PER_LEVEL)
            self.nonzero_blocks_moved += bool(self.qa[l][src].any() and self.qb[l][src].any())
            orc.transfer(self.qa[l], self.qb[l], dst, self.ratios[dst])
            mid = False
            for g in range(l * E, (l + 1) * E):
                b = np.ascontiguousarray(self.snap.pop(g)).copy()
                mid = self._mark_done(b) or mid
                self.os[k + 1].envs[self._env(g)] = b
            self.advanced_mid_episode += mid
            dropped = sum(len(self.win[g]) for g in range(l * E, (l + 1) * E))
            self.advanced_with_open_windows += dropped > 0; self.dropped_entries += dropped
            for g in range(l * E, (l + 1) * E):
                self.win[g] = []
            self.level[l] = k + 1; self.entered_period[k + 1][l] = j
            self.level_episodes[l] = 0; self.windows[l] = deque([], maxlen=self.sched[k + 1]["W"]); self.promoted[l] = -1; self.frozen[l] = False

    def _episode_end(self, l, k, code, steps, decided):
        """the books of an episode's end (team_checks.TeamReference's); -> whether the level is decided now"""
        self.episodes[l] += 1; self.successes[l] += code == ec.GOAL; self.by_code[code][l] += 1
        if self.log_n[l] < self.cap:
            self.log_code[l][self.log_n[l]] = code; self.log_len[l][self.log_n[l]] = steps
        self.log_n[l] += 1
        if decided:  # the level is decided: totals and log only
            return True
        self.windows[l].append(int(code == ec.GOAL)); self.level_episodes[l] += 1
        if sum(self.windows[l]) >= self.sched[k]["ms"]:
            self.promoted[l] = self.level_episodes[l]
            self.finished_by_promotion_beside_lower += k == self.last_level and bool((self.level < self.last_level).any())
            return True
        return bool(self.level_episodes[l] >= self.sched[k]["me"])

    def run(self, periods):
        E, N = self.E, self.nstep
        i_idx, i_fl, i_code, i_sc, i_rew = self.ii["idx_x"], self.ii["flags"], self.ii["code"], self.ii["step_count"], self.ri["reward"]
        k0, k1 = self.seed & 0xffffffff, (self.seed >> 32) & 0xffffffff
        first = True
        for _ in range(int(periods)):
            j = self.j
            if j % self.every == 0:
                self.advance()
            if j % self.every == 0 or first:
                live = [int(((self.level == k) & ~self.frozen).sum()) for k in range(LEVELS)]
                self.launches.append((j, live, [int((self.level == k).sum()) for k in range(LEVELS)]))
            first = False
            before = [o.get_fields()[1] for o in self.os]
            acts = [np.full(self.n_envs, 2, np.uint8) for _ in range(LEVELS)]
            words, s = {}, {}
            for l in range(self.n):
                if self.frozen[l]:
                    continue
                k = int(self.level[l])
                thr = self.sched[k]["thr"]
                thr = thr[min(int(self.level_episodes[l]), len(thr) - 1)]  # one threshold per team and period
                for g in range(l * E, (l + 1) * E):
                    if before[k][i_fl][g] & 1:
                        continue
                    r = orc.philox((j & 0xffffffff, (j >> 32) & 0xffffffff, g, ec.STREAM_ACTION), (k0, k1))
                    words[g] = r
                    s[g] = int(before[k][i_idx][g])
                    if (int(r[0]) >> 8) < thr:
                        acts[k][g] = (int(r[1]) * 3) >> 32
                    else:
                        acts[k][g] = int(orc.agent_predict(self.qa[l], self.qb[l], [s[g]])[0])
            for k, o in enumerate(self.os):
                o.step(acts[k])
            for g, b in self.snap.items():
                self.os[int(self.level[g // E])].envs[self._env(g)] = b
            after = [o.get_fields() for o in self.os]
            for l in range(self.n):
                if self.frozen[l]:
                    continue
                k = int(self.level[l])
                reals, ints = after[k]
                decided, rows = False, {}
                for g in range(l * E, (l + 1) * E):  # env order
                    if g not in words:
                        continue
                    r = words[g]
                    a, ns = int(acts[k][g]), int(ints[i_idx][g])
                    sa = 3 * s[g] + a
                    done = bool(ints[i_fl][g] & 1)
                    if N == 0:
                        c = int(self.cnt[l][sa])
                        al = self.alpha[c] if c < len(self.alpha) else self.cfg.alpha_min
                        orc.agent_update(self.qa[l], self.qb[l], self.cnt[l], [sa], [ns], [al], self.cfg.gamma, [reals[i_rew][g]], quirks=self.cfg.quirks,
                                         coin=[int(r[2]) >> 31], done=[int(done)])
                    else:  # team_nstep_checks.TeamNstepReference.run's steps 1 - 4, its _update as it stands
                        w = self.win[g]
                        self.stamp[l] += 1
                        w.append([sa, float(reals[i_rew][g]), int(r[2]) >> 31, int(self.stamp[l])])
                        assert len(w) <= N
                        row_a, row_b = self.qa[l][3 * ns:3 * ns + 3].copy(), self.qb[l][3 * ns:3 * ns + 3].copy()
                        mask = ((s[g] // 63) % 3 != (ns // 63) % 3) if (self.cfg.quirks & Q_POS_CHANGE) else (not done)
                        if done:
                            for i in range(len(w)):
                                tn.TeamNstepReference._update(self, l, g, i, row_a, row_b, mask, rows)
                            w.clear()
                        elif len(w) == N:
                            tn.TeamNstepReference._update(self, l, g, 0, row_a, row_b, mask, rows)
                            w.pop(0)
                    self.decisions[l] += 1
                    if done:
                        decided = self._episode_end(l, k, int(ints[i_code][g]), int(ints[i_sc][g]), decided)
                if decided:  # frozen at the period's end: all E records applied, all E envs — and their windows — as they are now
                    self.frozen[l] = True
                    for g in range(l * E, (l + 1) * E):
                        self.snap[g] = self.os[k].envs[self._env(g)].copy()
            self.j += 1

    def result(self):
        fields = [o.get_fields() for o in self.os]
        lv = self.level.astype(int)
        idx, env_lv, env = np.arange(self.n), np.repeat(lv, self.E), np.arange(self.n_envs)
        out = {"qa": self.qa, "qb": self.qb, "count": self.cnt, "decisions": self.decisions, "episodes": self.episodes, "successes": self.successes,
               "by_code": self.by_code, "promotion_episode": self.promoted, "level_episodes": self.level_episodes, "frozen": self.frozen,
               "log_code": self.log_code, "log_len": self.log_len, "log_n": self.log_n, "level": self.level, "entered_period": self.entered_period,
               "team_pending_len": self.pending_lengths()}
        out.update({f: np.stack([fields[k][0][i] for k in range(LEVELS)])[env_lv, env] for f, i in self.ri.items()})
        out.update({f: np.stack([fields[k][1][i] for k in range(LEVELS)])[env_lv, env] for f, i in self.ii.items()})
        pa, ea = self.promoted_at.copy(), self.episodes_at.copy()
        pa[lv, idx] = self.promoted; ea[lv, idx] = self.level_episodes  # the current level's row shows the counters as they stand
        out["promoted_at"], out["episodes_at"] = pa, ea
        return {k: np.array(v, copy=True) for k, v in out.items()}


PER_ENV = tc.PER_ENV + ("team_pending_len",)
PERIOD_KEY = "period_index"


def ensemble_result(ens):
    """`team_nstep_checks.ensemble_result` plus the per-level history, from a SequentialEnsemble"""
    out = tn.ensemble_result(ens)
    out.update(ens.levels())
    return out


def assert_equal(got, want, what, teams=None, envs_per_team=1):
    """tables, counters, ring, log, env state, history arrays and pending lengths, `==`; `teams`: (rows of got, rows of want) — the per-env entries take those
    teams' envs, the history arrays their columns"""
    hist = HISTORY[1:]
    flat = lambda d: {k: v for k, v in d.items() if k not in hist}
    if teams is None:
        ec.assert_equal(flat(got), flat(want), what)
    else:
        E = int(envs_per_team)
        envs = tuple([l * E + k for l in rows for k in range(E)] for rows in teams)
        ec.assert_equal({k: v for k, v in flat(got).items() if k not in PER_ENV}, {k: v for k, v in flat(want).items() if k not in PER_ENV}, what, learners=teams)
        ec.assert_equal({k: got[k] for k in PER_ENV}, {k: want[k] for k in PER_ENV}, what, learners=envs)
    for k in hist:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if teams is not None:
            g, w = g[:, teams[0]], w[:, teams[1]]
        assert g.shape == w.shape and np.array_equal(g.astype(np.int64), w.astype(np.int64)), f"{what}: {k} differs: {g.tolist()} vs {w.tolist()}"


# ---- the cases (tests/test_gpu_ensemble_team_levels.py and tests/test_team_levels_host_emulation.py) ----
# In the style of advance_checks.CASE: the reference's quirks from level 0, a promotion window of 4 episodes, success rate 0.5 (3 successes), advance_every 64,
# a budget of episodes at level 0 and a smaller one above it, seed 11.  `need` names what the case is there for; every name is asserted ON THE YARDSTICK
# (assert_case_conditions) before anything is compared:
#   three_levels   at some launch live teams stand on at least three different levels
#   padding        at some launch a level's live teams are no multiple of 64 / E
#   both_ways      a team advanced by promotion and one by exhaustion
#   mid_episode    a team advanced while at least one of its envs was in the middle of an episode
#   open_windows   a team advanced with a non-empty window whose entries were dropped (n-step cases)
#   last_beside    a team promoted at the last level while another stood below it
#   moved_nonzero  a transfer moved a block that is non-zero in both tables (the cases from trained tables)
BASE = dict(seed=11, every=64, window=4, success_rate=0.5, last_level=4, log_capacity=64, quirks=ec.Q_REFERENCE, start_level=0, order=0, nstep=0, trained=False,
            advance_exhausted=True, ratios=ensemble.REFERENCE_RATIOS)
# Settled on the yardstick (2 - 15 s a case on one CPU core): from zero tables nobody lands above level 0 within 1 024 periods, so no team promotes at the
# last level there, and teams of 16 or 64 envs spend any small budget within one advance interval and walk the levels in lockstep.  The cases that need
# promotions above level 0 therefore start from trained tables (`ensemble_checks.trained_tables`, greedy at every level) with `advance_checks.TRAINED_RATIOS`,
# which are distinct and hold no 1.0, so a wrong block or ratio shows; one success in the window promotes in the E = 4 cases, so that teams promote at level 4
# while others stand below it.  With one team per wave (E = 64) no segment can need padding, and a team of one env freezes at its episode's end, never mid-episode.
TRAINED = dict(trained=True, eps=(0.0,), ratios=ac.TRAINED_RATIOS)
ALWAYS = ("three_levels", "both_ways")
CASES = {
    "E4": dict(TRAINED, L=40, E=4, periods=1024, min_successes=1, max_episodes=(3, 3, 3, 3, 16), need=ALWAYS + ("padding", "mid_episode", "last_beside", "moved_nonzero")),
    "E4-paper": dict(TRAINED, L=40, E=4, periods=1024, min_successes=1, max_episodes=(3, 3, 3, 3, 16), order=1,
                     need=ALWAYS + ("padding", "mid_episode", "last_beside", "moved_nonzero")),
    "E64": dict(TRAINED, L=5, E=64, periods=704, min_successes=3, max_episodes=(128,) * 5, ratios=ensemble.REFERENCE_RATIOS, need=ALWAYS + ("mid_episode", "moved_nonzero")),
    "E1": dict(L=70, E=1, periods=1024, max_episodes=(6, 1, 1, 1, 1), need=ALWAYS + ("padding",)),
    "N3": dict(TRAINED, L=9, E=16, periods=1024, min_successes=3, max_episodes=(32,) * 5, nstep=3, need=ALWAYS + ("padding", "mid_episode", "open_windows", "moved_nonzero")),
    "N16": dict(TRAINED, L=9, E=16, periods=1024, min_successes=3, max_episodes=(32,) * 5, nstep=16, need=ALWAYS + ("padding", "mid_episode", "open_windows", "moved_nonzero")),
    "N4": dict(L=12, E=4, periods=768, max_episodes=(6, 3, 3, 3, 3), nstep=4, need=ALWAYS + ("padding", "mid_episode", "open_windows")),  # (flown in float64)
}


def case(name):
    return dict(BASE, **CASES[name])


def case_config(c, dtype):
    return training_config(c["start_level"], quirks=c["quirks"], dtype=dtype)


def case_schedules(c):
    ms = ensemble.min_successes_for(c["window"], c["success_rate"]) if c.get("min_successes") is None else c["min_successes"]
    eps = c.get("eps")
    return [dict(eps=ensemble.exploration_rates(k) if eps is None else np.asarray(eps, np.float64), window=c["window"], min_successes=ms, max_episodes=c["max_episodes"][k])
            for k in range(LEVELS)]


def case_tables(c, n):
    return ec.trained_tables(n) if c["trained"] else None


def make_yardstick(c, dtype=F32, n=None):
    n = c["L"] if n is None else n
    return TeamLevelsYardstick(case_config(c, dtype), n, c["E"], c["seed"], case_schedules(c), c["ratios"], c["last_level"], c["every"], c["advance_exhausted"], c["order"],
                               c["nstep"], c["log_capacity"], tables=case_tables(c, n))


def assert_case_conditions(y, need):
    tpw = 64 // y.E
    print("launches (period, live per level, teams per level):", y.launches)
    print("advanced promoted", y.advanced_promoted, "by level", y.promoted_from.tolist(), "exhausted", y.advanced_exhausted, "by level", y.exhausted_from.tolist(),
          "mid-episode", y.advanced_mid_episode, "with open windows", y.advanced_with_open_windows, "entries dropped", y.dropped_entries, "non-zero blocks moved",
          y.nonzero_blocks_moved, "promoted at the last level beside lower teams", y.finished_by_promotion_beside_lower, "levels at the end",
          np.bincount(y.level, minlength=LEVELS).tolist(), "unfinished", y.n_unfinished())
    holds = {
        "three_levels": any(sum(1 for c in live if c > 0) >= 3 for _, live, _ in y.launches),
        "padding": any(c % tpw != 0 for _, live, _ in y.launches for c in live),
        "both_ways": y.advanced_promoted >= 1 and y.advanced_exhausted >= 1,
        "mid_episode": y.advanced_mid_episode >= 1,
        "open_windows": y.advanced_with_open_windows >= 1 and y.dropped_entries >= 1,
        "last_beside": y.finished_by_promotion_beside_lower >= 1,
        "moved_nonzero": y.nonzero_blocks_moved >= 1,
    }
    for k in need:
        assert holds[k], f"the case does not show '{k}' on the yardstick"
    assert not y.events["dropped"]


_cache = {}


def case_reference(name, dtype=F32, n=None, periods=None):
    """(result, yardstick) of a case — computed once per process and never changed — after asserting ON THE YARDSTICK what the case is for (whole cases only)"""
    key = (name, dtype, n, periods)
    if key not in _cache:
        c = case(name)
        y = make_yardstick(c, dtype, n)
        y.run(c["periods"] if periods is None else periods)
        if n is None and periods is None:
            assert_case_conditions(y, c["need"])
        _cache[key] = (y.result(), y)
    return _cache[key]


def case_ensemble(name, dtype=F32, n=None, **kw):
    """a SequentialEnsemble set up for the case (team curriculum mode on, team_nstep set), not yet run"""
    from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
    c = case(name)
    n = c["L"] if n is None else n
    ens = SequentialEnsemble(case_config(c, dtype), n, seed=c["seed"], log_capacity=c["log_capacity"], envs_per_learner=c["E"], teams=True, **kw)
    for k, s in enumerate(case_schedules(c)):
        ens.set_level_schedules(k, s["eps"], s["window"], s["min_successes"], s["max_episodes"])
    if c["nstep"]:
        ens.set_team_nstep(c["nstep"])
    ens.set_team_curriculum(c["last_level"], c["every"], c["ratios"], c["advance_exhausted"], c["order"])
    tables = case_tables(c, n)
    if tables is not None:
        ens.set_tables(*tables)
    return ens
