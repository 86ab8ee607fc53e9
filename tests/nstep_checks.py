"""Shared by the n-step tests (CPU emulation and GPU): the yardstick for `SequentialEnsemble.set_nstep` (include/dql.h).

`NstepReference` is `ensemble_checks.Reference` with ONE thing changed, the update: per learner a literal Python list of pending entries (cell, reward, coin),
the n-step return written out in Python floats (IEEE double, one rounding per operation), `oracle.agent_predict` for the action as before.  It knows nothing of
the kernels.  While it runs it counts the events a kernel can get wrong (`events`), and every row asserts ON IT that its events occurred before anything else
is looked at (`EXPECTED`: the counts of the main rows, pinned to the digit)."""
import functools
from collections import Counter

import numpy as np

from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_BOOTSTRAP_ON_POS_CHANGE as Q_POS_CHANGE, Q_UPDATE_TABLE_A_ONLY as Q_A_ONLY, training_config
from oracle import oracle as orc

import ensemble_checks as ec

NSTEP_MAX = 16


def argmax3(a, b, c):
    k, v = 0, a
    if b > v:
        v, k = b, 1
    if c > v:
        k = 2
    return k


class NstepReference(ec.Reference):
    def __init__(self, cfg, n, seed, nstep, watch=(), **kw):
        """nstep: 1 .. 16; watch: period counts after which the windows' lengths are kept in `len_after[count]`"""
        super().__init__(cfg, n, seed, **kw)
        assert 1 <= int(nstep) <= NSTEP_MAX
        self.nstep = int(nstep)
        self.win = [[] for _ in range(self.n)]  # per learner: [cell, reward, coin] per pending decision, oldest first
        self.events = Counter()
        self.ep_len = np.zeros(self.n, np.int64)  # decisions of the running episode
        self.actions = [[] for _ in range(self.n)]  # every decision's action, for "did n change what was flown"
        self.watch, self.len_after = set(int(w) for w in watch), {}

    def set_level(self, k):
        super().set_level(k)
        self.win = [[] for _ in range(self.n)]  # every env re-enters through reset: the windows are discarded
        self.ep_len[:] = 0

    def pending_lengths(self):
        return np.array([len(w) for w in self.win], np.int32)

    def _update(self, l, k, row_a, row_b, mask, ns, newest):
        """the entry at position k of learner l's window, against the row of s' = ns as it was read before the period's first write"""
        w, gamma, ev = self.win[l], self.cfg.gamma, self.events
        sa, _, coin = w[k]
        dbl = not (self.cfg.quirks & Q_A_ONLY)
        sel_b = bool(dbl and coin)
        sel, val = (row_b, row_a) if sel_b else (row_a, row_b if dbl else row_a)
        best = val[argmax3(sel[0], sel[1], sel[2])]
        g = best * float(mask)
        for i in range(len(w) - 1, k - 1, -1):
            g = w[i][1] + (gamma * g)
        ev["repeated_cell"] += sum(1 for x in w if x[0] == sa) >= 2
        ev["older_entry_patch"] += (not newest) and sa // 3 == ns
        if not 0 <= sa < N_CELLS:
            ev["dropped"] += 1
            return
        c = int(self.cnt[l][sa])
        al = float(self.alpha[c]) if c < len(self.alpha) else float(self.cfg.alpha_min)
        self.updates_inside += c < len(self.alpha); self.updates_beyond += c >= len(self.alpha)
        self.cnt[l][sa] += 1
        q = self.qb[l] if sel_b else self.qa[l]
        old = float(q[sa])
        q[sa] = old + al * (g - old)
        ev["writes_b" if sel_b else "writes_a"] += 1

    def run(self, periods):
        o, n, N = self.o, self.n, self.nstep
        i_idx, i_fl, i_code, i_sc, i_rew = self.ii["idx_x"], self.ii["flags"], self.ii["code"], self.ii["step_count"], self.ri["reward"]
        k0, k1 = self.seed & 0xffffffff, (self.seed >> 32) & 0xffffffff
        act = np.zeros(n, np.uint8)
        ev = self.events
        for _ in range(int(periods)):
            j = self.j
            _, ints = o.get_fields()
            s = ints[i_idx].copy(); was_done = (ints[i_fl] & 1) != 0
            words = {}
            for l in range(n):
                act[l] = 2
                if self.frozen[l] or was_done[l]:
                    continue
                r = orc.philox((j & 0xffffffff, (j >> 32) & 0xffffffff, l, ec.STREAM_ACTION), (k0, k1))
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
                done = bool(ints[i_fl][l] & 1)
                w = self.win[l]
                self.actions[l].append(a)
                # 1. the decision's entry
                w.append([3 * int(s[l]) + a, float(reals[i_rew][l]), int(r[2]) >> 31])
                assert len(w) <= N
                self.ep_len[l] += 1
                # 2. both tables' row of s', once, before this period's first write
                row_a, row_b = self.qa[l][3 * ns:3 * ns + 3].copy(), self.qb[l][3 * ns:3 * ns + 3].copy()
                # 3. the mask
                mask = ((int(s[l]) // 63) % 3 != (ns // 63) % 3) if (self.cfg.quirks & Q_POS_CHANGE) else (not done)
                # 4. the updates
                if done:
                    m = len(w)
                    ev["flushes"] += 1; ev["flush_entries"] += m; ev["short_flushes"] += m < N; ev["flushes_with_mask_1"] += bool(mask)
                    ev["episodes_longer_than_2n"] += self.ep_len[l] > 2 * N
                    for k in range(m):
                        self._update(l, k, row_a, row_b, mask, ns, newest=k == m - 1)
                    w.clear()
                    self.ep_len[l] = 0
                elif len(w) == N:
                    ev["full_window_updates"] += 1
                    self._update(l, 0, row_a, row_b, mask, ns, newest=N == 1)
                    w.pop(0)
                self.decisions[l] += 1
                self.same_state += int(ns == int(s[l]))
                if done:
                    code = int(ints[i_code][l])
                    self.episodes[l] += 1; self.successes[l] += code == ec.GOAL; self.by_code[code][l] += 1
                    if self.log_n[l] < self.cap:
                        self.log_code[l][self.log_n[l]] = code; self.log_len[l][self.log_n[l]] = int(ints[i_sc][l])
                    self.log_n[l] += 1
                    self.windows[l].append(int(code == ec.GOAL)); self.level_episodes[l] += 1
                    if sum(self.windows[l]) >= self.min_successes:
                        self.promoted[l] = self.level_episodes[l]; self.frozen[l] = True
                    elif self.level_episodes[l] >= self.max_episodes:
                        self.frozen[l] = True
                    if self.frozen[l]:
                        self.freeze_period[l] = j
                        self.snap[l] = o.envs[l * self.es:(l + 1) * self.es].copy()
            self.j += 1
            if self.j in self.watch:
                self.len_after[self.j] = self.pending_lengths()

    def result(self):
        out = super().result()
        out["pending_len"] = self.pending_lengths()
        assert not (out["pending_len"][out["frozen"]] != 0).any(), "a frozen learner with a pending window"
        return out


def ensemble_result(ens):
    """`ensemble_checks.ensemble_result` plus the windows' lengths, from a SequentialEnsemble"""
    out = ec.ensemble_result(ens)
    out["pending_len"] = ens.pending_lengths()
    return out


# ---- the main rows: level 0, tables of zeros, EPS_TABLE, seed 2024, 300 periods (flown as 300 and as 7 + 293) ----
MAIN_SEED, MAIN_PERIODS, MAIN_SPLIT, MAIN_LOG = 2024, 300, (7, 293), 32
MAIN_ROWS = [(ec.Q_PAPER, F32, 3), (ec.Q_PAPER, F32, 16), (ec.Q_PAPER, F64, 3), (ec.Q_REFERENCE, F32, 3), (ec.Q_BENCH, F64, 16)]
MAIN_IDS = [f"quirks-{q:#x}-{'f32' if d == F32 else 'f64'}-n{n}" for q, d, n in MAIN_ROWS]
EVENT_KEYS = ("full_window_updates", "flush_entries", "short_flushes", "repeated_cell", "older_entry_patch", "episodes_longer_than_2n", "flushes_with_mask_1",
              "open_after_7", "open_after_300", "longest_after_300", "learners_acting_differently_than_n1")
# (quirks, dtype, n, learners) -> the yardstick's own counts, in EVENT_KEYS' order (printed by main_reference; see DESIGN.md section 22 for the table)
EXPECTED = {
    (0x40, F32, 3, 70): (19538, 950, 2, 8957, 6857, 316, 0, 70, 64, 2, 70),
    (0x40, F32, 16, 70): (14179, 5564, 4, 13120, 2624, 261, 0, 70, 68, 15, 70),
    (0x40, F64, 3, 70): (19538, 950, 2, 8959, 6858, 316, 0, 70, 64, 2, 70),
    (0x7f, F32, 3, 70): (19495, 972, 3, 9593, 7063, 323, 0, 70, 69, 2, 70),
    (0x60, F64, 16, 70): (14187, 5506, 2, 13151, 2723, 265, 0, 70, 68, 15, 70),
    (0x40, F32, 3, 26): (7264, 347, 2, 3272, 2458, 115, 0, 26, 24, 2, 26),
    (0x40, F32, 16, 26): (5325, 1964, 4, 4816, 876, 94, 0, 26, 26, 15, 26),
    (0x40, F64, 3, 26): (7264, 347, 2, 3272, 2457, 115, 0, 26, 24, 2, 26),
    (0x7f, F32, 3, 26): (7250, 353, 2, 3582, 2668, 117, 0, 26, 26, 2, 26),
    (0x60, F64, 16, 26): (5297, 2018, 2, 4883, 1039, 98, 0, 26, 25, 15, 26),
}


@functools.lru_cache(maxsize=None)
def _actions_n1(quirks, dtype, learners):
    ref = ec.Reference(training_config(0, quirks=quirks, dtype=dtype), learners, MAIN_SEED, log_capacity=MAIN_LOG)
    acts = [[] for _ in range(learners)]
    step = ref.o.step

    def spy(act):  # the one-step reference loop has no action log: the actions are read where it hands them to the oracle
        spy.last = np.array(act, copy=True)
        step(act)
    ref.o.step = spy
    for _ in range(MAIN_PERIODS):
        before = ref.decisions.copy()
        ref.run(1)
        for l in np.nonzero(ref.decisions != before)[0]:
            acts[l].append(int(spy.last[l]))
    return acts, ref.result()


def count_events(ref, n1_actions=None):
    ev = dict(ref.events)
    ev["open_after_7"] = int((ref.len_after[MAIN_SPLIT[0]] > 0).sum()) if MAIN_SPLIT[0] in ref.len_after else -1
    end = ref.pending_lengths()
    ev["open_after_300"], ev["longest_after_300"] = int((end > 0).sum()), int(end.max())
    ev["learners_acting_differently_than_n1"] = -1 if n1_actions is None else sum(1 for a, b in zip(ref.actions, n1_actions) if a != b)
    return tuple(int(ev.get(k, 0)) for k in EVENT_KEYS)


@functools.lru_cache(maxsize=None)
def main_reference(quirks, dtype, nstep, learners):
    """(result, events as a dict) of the yardstick on a main row, after asserting ON IT that the row's events occurred"""
    cfg = training_config(0, quirks=quirks, dtype=dtype)
    ref = NstepReference(cfg, learners, MAIN_SEED, nstep, watch=MAIN_SPLIT[:1], log_capacity=MAIN_LOG)
    ref.run(MAIN_PERIODS)
    want = ref.result()
    counts = count_events(ref, _actions_n1(quirks, dtype, learners)[0])
    ev = dict(zip(EVENT_KEYS, counts))
    print(f"main row quirks {quirks:#x} dtype {dtype} n {nstep} learners {learners}:", ev, "cells written a / b", int((want["qa"] != 0).sum()), int((want["qb"] != 0).sum()),
          "dropped", ref.events["dropped"])
    assert ref.events["dropped"] == 0
    assert ev["full_window_updates"] >= 1 and ev["flush_entries"] >= 1 and ev["repeated_cell"] >= 1 and ev["older_entry_patch"] >= 1, ev
    assert ev["open_after_7"] >= 1 and ev["open_after_300"] >= 1 and ev["learners_acting_differently_than_n1"] >= 1, ev
    assert ev["episodes_longer_than_2n"] >= 1, ev
    assert (want["qa"] != 0).any() and ((want["qb"] != 0).any() or (quirks & Q_A_ONLY)), "under the coin both tables are to be written"
    key = (quirks, dtype, nstep, learners)
    if key in EXPECTED:
        assert counts == EXPECTED[key], f"the yardstick's event counts moved: {dict(zip(EVENT_KEYS, counts))} vs {dict(zip(EVENT_KEYS, EXPECTED[key]))}"
    return want, ev


# ---- from trained tables (ensemble_checks.trained_tables, TRAINED_LEARNERS_CASE): 400 periods, flown as 400 and as 7 + 393 ----
TRAINED_ROWS = [(4, ec.Q_PAPER, F32, 4), (2, ec.Q_BENCH, F32, 16)]
TRAINED_IDS = ["level-4-quirks-0x40-n4", "level-2-quirks-0x60-n16"]


@functools.lru_cache(maxsize=None)
def trained_reference(level, quirks, dtype, nstep, learners):
    cfg = training_config(level, quirks=quirks, dtype=dtype)
    tables = ec.trained_tables(learners)
    ref = NstepReference(cfg, learners, ec.TRAINED_LEARNERS_SEED, nstep, tables=tables, **ec.TRAINED_LEARNERS_CASE)
    ref.run(ec.TRAINED_LEARNERS_PERIODS)
    want = ref.result()
    ev = dict(zip(EVENT_KEYS, count_events(ref)))
    print(f"trained row level {level} quirks {quirks:#x} n {nstep} learners {learners}:", ev, "promoted", int((want["promotion_episode"] >= 0).sum()), "frozen", int(want["frozen"].sum()),
          "updates inside / beyond the learning-rate table", ref.updates_inside, ref.updates_beyond)
    assert ref.events["dropped"] == 0
    assert ev["short_flushes"] >= 1 and ev["flush_entries"] >= 1 and ev["full_window_updates"] >= 1 and ev["repeated_cell"] >= 1, ev
    assert want["frozen"].any() and ref.updates_inside >= 1 and ref.updates_beyond >= 1
    return want, tables, ev


# ---- the launch boundary: one run of 4 100 periods is launches of 4 096 + 4 ----
BOUNDARY_CASE = dict(eps=[0.3], window=100, min_successes=97, log_capacity=128)
BOUNDARY_SEED, BOUNDARY_PERIODS, BOUNDARY_N = 11, 4100, 16


@functools.lru_cache(maxsize=None)
def boundary_reference(learners):
    cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
    ref = NstepReference(cfg, learners, BOUNDARY_SEED, BOUNDARY_N, watch=(4096,), **BOUNDARY_CASE)
    ref.run(BOUNDARY_PERIODS)
    want = ref.result()
    at = ref.len_after[4096]
    live_then = (ref.freeze_period < 0) | (ref.freeze_period >= 4096)
    print("launch boundary: windows at period 4096", at.tolist(), "live then", live_then.tolist(), "episodes", want["episodes"].tolist())
    assert (live_then & (at > 0)).any(), "no live learner with a non-empty window at the launch boundary"
    return want
