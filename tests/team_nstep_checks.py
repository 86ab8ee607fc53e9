"""Shared by the team n-step tests (CPU emulation and GPU): the yardstick for `SequentialEnsemble.set_team_nstep` (include/dql.h).

`TeamNstepReference` is `team_checks.TeamReference` with ONE thing changed, the update: `run` is restated with step (4) replaced.  Per ENV a literal Python
list of pending entries [cell, reward, coin], the n-step return written out in Python floats (IEEE double, one rounding per operation), `self.cnt` /
`self.alpha` for the learning rate as it stands at the moment of each update, both tables' row of s' copied ONCE at the env's turn — after the writes of the
envs before it in the period, before its own.  `set_level` empties the lists; `rearm` leaves them alone.  It knows nothing of the kernels.  While it runs
it counts the events a kernel can get wrong (`events`); every row asserts ON IT that its events occurred, then the counts are pinned to the digit
(`EXPECTED`)."""
from collections import Counter

import numpy as np

from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_BOOTSTRAP_ON_POS_CHANGE as Q_POS_CHANGE, Q_UPDATE_TABLE_A_ONLY as Q_A_ONLY, training_config
from oracle import oracle as orc

import ensemble_checks as ec
import team_checks as tc
from nstep_checks import NSTEP_MAX, argmax3


class TeamNstepReference(tc.TeamReference):
    def __init__(self, cfg, n_learners, envs_per_learner, seed, nstep, watch=(), **kw):
        """nstep: 1 .. 16; watch: period counts after which the windows' lengths are kept in `len_after[count]`"""
        super().__init__(cfg, n_learners, envs_per_learner, seed, **kw)
        assert 1 <= int(nstep) <= NSTEP_MAX
        self.nstep = int(nstep)
        self.win = [[] for _ in range(self.n_envs)]  # per env: [cell, reward, coin, the team's write stamp at the append] per pending decision, oldest first
        self.events = Counter(self.events)
        self.stamp = np.zeros(self.n, np.int64)         # (event bookkeeping only) per learner: its appends and writes, counted
        self.last_write = [dict() for _ in range(self.n)]  # per learner: cell -> (stamp, env) of the cell's last write
        self.watch, self.len_after = set(int(w) for w in watch), {}

    def set_level(self, k):
        super().set_level(k)
        self.win = [[] for _ in range(self.n_envs)]  # every env re-enters through reset: the windows are discarded

    def pending_lengths(self):
        return np.array([len(w) for w in self.win], np.int32)

    def _update(self, l, g, k, row_a, row_b, mask, rows):
        """the entry at position k of env g's window, against the row of s' as it was read at this env's turn"""
        w, gamma, ev = self.win[g], self.cfg.gamma, self.events
        sa, _, coin, appended = w[k]
        dbl = not (self.cfg.quirks & Q_A_ONLY)
        sel_b = bool(dbl and coin)
        sel, val = (row_b, row_a) if sel_b else (row_a, row_b if dbl else row_a)
        best = val[argmax3(sel[0], sel[1], sel[2])]
        ret = best * float(mask)
        for i in range(len(w) - 1, k - 1, -1):
            ret = w[i][1] + (gamma * ret)
        ev["repeated_cell"] += sum(1 for x in w if x[0] == sa) >= 2
        last = self.last_write[l].get(sa)
        ev["cell_written_by_mate_since_append"] += last is not None and last[0] > appended and last[1] != g  # the value that stands now is a team-mate's
        if not 0 <= sa < N_CELLS:
            ev["dropped"] += 1
            return
        c = int(self.cnt[l][sa])  # as it stands now: team-mates may have counted this cell since the entry was appended
        al = float(self.alpha[c]) if c < len(self.alpha) else float(self.cfg.alpha_min)
        self.cnt[l][sa] += 1
        q = self.qb[l] if sel_b else self.qa[l]
        old = float(q[sa])
        q[sa] = old + al * (ret - old)
        ev["writes_b" if sel_b else "writes_a"] += 1
        rows.setdefault(sa // 3, []).append(g)
        self.stamp[l] += 1
        self.last_write[l][sa] = (int(self.stamp[l]), g)

    def run(self, periods):
        o, E, ev, N = self.o, self.E, self.events, self.nstep
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
                rows, ended, decided, decided_at = {}, 0, False, None
                kinds = set()
                for g in mine:  # env order
                    r = words[g]
                    a, ns = int(act[g]), int(ints[i_idx][g])
                    done = bool(ints[i_fl][g] & 1)
                    w = self.win[g]
                    if decided and decided_at is not None:
                        ev["mid_period_decisions"] += 1
                        decided_at = None
                    # 1. the decision's entry
                    self.stamp[l] += 1
                    w.append([3 * int(s[g]) + a, float(reals[i_rew][g]), int(r[2]) >> 31, int(self.stamp[l])])
                    assert len(w) <= N
                    # 2. both tables' row of s', once, at this env's turn: after the writes of the envs before it in this period, before its own
                    row_a, row_b = self.qa[l][3 * ns:3 * ns + 3].copy(), self.qb[l][3 * ns:3 * ns + 3].copy()
                    after_write = ns in rows
                    # 3. the mask
                    mask = ((int(s[g]) // 63) % 3 != (ns // 63) % 3) if (self.cfg.quirks & Q_POS_CHANGE) else (not done)
                    # 4. the updates
                    if done:
                        m = len(w)
                        ev["flushes"] += 1; ev["flush_entries"] += m; ev["short_flushes"] += m < N; ev["flushes_with_mask_1"] += bool(mask)
                        ev["row_after_write_at_flush"] += after_write
                        kinds.add("flush")
                        for k in range(m):
                            self._update(l, g, k, row_a, row_b, mask, rows)
                        w.clear()
                    elif len(w) == N:
                        ev["full_window_updates"] += 1
                        ev["row_after_write_at_full"] += after_write
                        kinds.add("full")
                        self._update(l, g, 0, row_a, row_b, mask, rows)
                        w.pop(0)
                    else:
                        kinds.add("none")
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
                ev["mixed_team_periods"] += len(kinds) == 3
                self.written[l] = rows
                if decided:  # frozen at the period's end: all E records applied, all E envs — and their windows — as they are now
                    self.frozen[l] = True
                    self.freeze_period[l] = j
                    for g in range(l * E, (l + 1) * E):
                        self.snap[g] = o.envs[g * self.es:(g + 1) * self.es].copy()
            self.j += 1
            if self.j in self.watch:
                self.len_after[self.j] = self.pending_lengths()

    def result(self):
        out = super().result()
        out["team_pending_len"] = self.pending_lengths()
        return out


def ensemble_result(ens):
    """`ensemble_checks.ensemble_result` plus the envs' window lengths, from a SequentialEnsemble"""
    out = ec.ensemble_result(ens)
    out["team_pending_len"] = ens.team_pending_lengths()
    return out


# ---- the rows: team_checks.CASES unchanged (seed 11, their schedules, tables and periods), each with an n ----
ROWS = [("A", F32, 3), ("A", F32, 16), ("B", F32, 16), ("B", F64, 4), ("C", F32, 5), ("D", F32, 2), ("E", F32, 16), ("F", F32, 8), ("F2", F32, 3)]
ROW_IDS = [f"{name}-{'f64' if d == F64 else 'f32'}-n{n}" for name, d, n in ROWS]
SPLIT = 7
EVENT_KEYS = ("full_window_updates", "flush_entries", "flushes", "short_flushes", "row_after_write_at_full", "row_after_write_at_flush", "repeated_cell",
              "cell_written_by_mate_since_append", "mixed_team_periods", "open_in_frozen_teams", "longest_in_frozen_teams", "open_at_end", "open_after_7", "promoted", "frozen",
              "flushes_with_mask_1", "multi_end_periods", "episodes_after_decision", "writes_a", "writes_b")
# what each row is there for, asserted on the yardstick before its counts are looked at (each >= 1 unless a larger need is written here)
NEED = ("full_window_updates", "flush_entries", "short_flushes", "row_after_write_at_full", "repeated_cell", "cell_written_by_mate_since_append", "open_in_frozen_teams", "open_after_7")
NEED_NOT = {("A", 3): ("short_flushes",), ("D", 2): ("short_flushes",)}  # n = 3 and 2: no episode of these rows is shorter than n decisions
NEED_MORE = {("A", 3): dict(row_after_write_at_flush=1, mixed_team_periods=1, multi_end_periods=1), ("B", 16): dict(writes_a=1000, writes_b=1000, mixed_team_periods=1),
             ("B", 4): dict(writes_a=1000, writes_b=1000), ("D", 2): dict(episodes_after_decision=3), ("E", 16): dict(multi_end_periods=10, mixed_team_periods=10)}
# (case, dtype, n) -> the yardstick's own counts, in EVENT_KEYS' order (printed by row_reference; DESIGN.md section 24 has the table)
EXPECTED = {
    ("A", F32, 3): (6651, 150, 50, 0, 2404, 22, 2451, 3239, 2, 276, 2, 276, 320, 5, 5, 0, 5, 28, 6801, 0),
    ("A", F32, 16): (2482, 778, 49, 2, 400, 29, 1910, 1755, 6, 277, 15, 277, 320, 5, 5, 0, 5, 27, 3260, 0),
    ("B", F32, 16): (15332, 1050, 71, 8, 1160, 13, 9650, 6444, 41, 146, 15, 146, 160, 10, 10, 0, 3, 2, 8140, 8242),
    ("B", F64, 4): (19369, 268, 69, 5, 1592, 6, 9829, 4940, 13, 150, 3, 150, 160, 10, 10, 0, 2, 0, 9744, 9893),
    ("C", F32, 5): (39884, 1319, 269, 11, 657, 1, 23761, 2369, 26, 56, 4, 139, 160, 10, 19, 0, 4, 1, 41203, 0),
    ("D", F32, 2): (6860, 82, 41, 0, 2689, 20, 1670, 2615, 1, 284, 1, 284, 320, 0, 5, 0, 4, 26, 6942, 0),
    ("E", F32, 16): (19015, 5962, 373, 2, 4497, 97, 15204, 14123, 278, 180, 15, 180, 192, 6, 6, 0, 79, 2, 12442, 12535),
    ("F", F32, 8): (8577, 294, 38, 2, 385, 1, 4821, 1731, 9, 63, 7, 63, 72, 9, 9, 0, 1, 0, 4370, 4501),
    ("F2", F32, 3): (5143, 79, 27, 1, 51, 0, 2526, 110, 0, 1, 2, 17, 18, 1, 1, 0, 0, 0, 2628, 2594),
}


def count_events(ref):
    ev = dict(ref.events)
    E = ref.E
    end = ref.pending_lengths()
    frozen_envs = np.repeat(ref.frozen, E)
    ev["open_in_frozen_teams"] = int((end[frozen_envs] > 0).sum())
    ev["longest_in_frozen_teams"] = int(end[frozen_envs].max()) if frozen_envs.any() else 0
    ev["open_at_end"] = int((end > 0).sum())
    ev["open_after_7"] = int((ref.len_after[SPLIT] > 0).sum()) if SPLIT in ref.len_after else -1
    ev["promoted"], ev["frozen"] = int((ref.promoted >= 0).sum()), int(ref.frozen.sum())
    return tuple(int(ev.get(k, 0)) for k in EVENT_KEYS)


def make_reference(name, dtype, nstep, learners=None, watch=(SPLIT,)):
    c = tc.CASES[name]
    n = c["L"] if learners is None else learners
    tables = tc.case_tables(name)
    if tables is not None:
        tables = tuple(t[:n] for t in tables)
    return TeamNstepReference(tc.case_config(name, dtype), n, c["E"], tc.SEED, nstep, watch=watch, tables=tables, **c["sched"])


_cache = {}


def row_reference(name, dtype, nstep):
    """(result, events as a dict, the reference) of a row on the yardstick — computed once per process and never changed — after asserting ON IT what the row is for"""
    key = (name, dtype, nstep)
    if key in _cache:
        return _cache[key]
    c = tc.CASES[name]
    ref = make_reference(name, dtype, nstep)
    ref.run(c["periods"])
    want = ref.result()
    counts = count_events(ref)
    ev = dict(zip(EVENT_KEYS, counts))
    print(f"row {name} dtype {dtype} n {nstep}:", ev, "dropped", ref.events["dropped"], "mid-period decisions", ref.events["mid_period_decisions"])
    assert ref.events["dropped"] == 0
    for k in NEED:
        if k not in NEED_NOT.get((name, nstep), ()):
            assert ev[k] >= 1, f"row {name} n {nstep}: {k} never occurred on the yardstick"
    for k, v in NEED_MORE.get((name, nstep), {}).items():
        assert ev[k] >= v, f"row {name} n {nstep}: {k} occurred {ev[k]} times on the yardstick, {v} are needed"
    if c.get("live") == "some":
        assert (~want["frozen"]).any() and want["frozen"].any(), "frozen teams beside live ones are needed"
    assert (want["level_episodes"] <= c["sched"]["max_episodes"]).all() and (want["promotion_episode"] <= c["sched"]["max_episodes"]).all()
    if key in EXPECTED:
        assert counts == EXPECTED[key], f"the yardstick's event counts moved: {ev} vs {dict(zip(EVENT_KEYS, EXPECTED[key]))}"
    _cache[key] = (want, ev, ref)
    return _cache[key]


# ---- the launch boundary: one run of 4 100 periods is launches of 4 096 + 4 ----
# L = 2, E = 16, n = 16, eps 0.3, window 100, 97 successes, seed 11, level 0 under the reference's quirk word (case A's config).  Under evaluation.Q_PAPER a
# team of 16 envs at level 0 reaches 97 of 100 within 300 to 640 episodes — both teams were frozen long before period 4 096 for each of 53 seeds tried — so
# the boundary would be crossed by nobody; under 0x7f both teams are still live there (904 and 1 001 episodes, 446 and 441 successes) with all 32 windows open.
BOUNDARY = dict(L=2, E=16, nstep=16, periods=4100, sched=dict(eps=[0.3], window=100, min_successes=97, log_capacity=128))


def boundary_reference():
    if "boundary" in _cache:
        return _cache["boundary"]
    b = BOUNDARY
    cfg = training_config(0, quirks=ec.Q_REFERENCE, dtype=F32)
    ref = TeamNstepReference(cfg, b["L"], b["E"], tc.SEED, b["nstep"], watch=(4096,), **b["sched"])
    ref.run(b["periods"])
    at = ref.len_after[4096].reshape(b["L"], b["E"])
    live_then = (ref.freeze_period < 0) | (ref.freeze_period >= 4096)
    print("launch boundary: open windows per team at period 4096", (at > 0).sum(axis=1).tolist(), "live then", live_then.tolist())
    assert (live_then & ((at > 0).sum(axis=1) > 0)).any(), "no live team with an open window at the launch boundary"
    _cache["boundary"] = (ref.result(), cfg)
    return _cache["boundary"]
