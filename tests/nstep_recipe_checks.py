"""Shared by the tests of per-recipe n-step targets (CPU emulation and GPU): the yardstick, the case and its events (include/dql.h
dql_ensemble_set_recipe_nstep).

`NstepRecipeYardstick` is `recipe_checks.RecipeYardstick` — one recipe flown over all n learners, one unchanged oracle per level — whose `run` restates
`advance_checks.Yardstick.run` with the ONE difference `nstep_checks.NstepReference` has from `ensemble_checks.Reference`: per learner a literal Python list of
pending entries [cell, reward, coin], the n-step return written out in Python floats, the recipe's `CountingTable` for the learning rates, and the window
asserted empty whenever a learner advances.  It knows nothing of the kernels.  While it runs it counts the events a kernel can get wrong; every row asserts ON
IT that its events occurred, pinned to the digit (`EXPECTED`), before an emulation or an ensemble is looked at."""
import dataclasses
import functools
from collections import Counter

import numpy as np

from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, Q_BOOTSTRAP_ON_POS_CHANGE as Q_POS_CHANGE, Q_UPDATE_TABLE_A_ONLY as Q_A_ONLY
from oracle import oracle as orc

import advance_checks as ac
import ensemble_checks as ec
import nstep_checks as nc
import recipe_checks as rc

LEVELS = ac.LEVELS
CELLS_PER_LEVEL = ac.CELLS_PER_LEVEL
NSTEP_MAX = nc.NSTEP_MAX


class NstepRecipeYardstick(rc.RecipeYardstick):
    def __init__(self, cfg, n, seed, recipe, members, advance_every, nstep, log_capacity=64, tables=None):
        super().__init__(cfg, n, seed, recipe, members, advance_every, log_capacity, tables)
        assert 1 <= int(nstep) <= NSTEP_MAX
        self.nstep = int(nstep)
        self.win = [[] for _ in range(self.n)]  # per learner: [cell, reward, coin] per pending decision, oldest first
        self.events = Counter()
        self.block_updates = np.zeros(LEVELS, np.int64)  # updates by the level block of the cell they wrote
        self.open_at_boundaries, self.longest_at_boundaries = 0, 0

    def pending_lengths(self):
        return np.array([len(w) for w in self.win], np.int32)

    def advance(self):
        for l in np.nonzero(self.members)[0]:
            assert not (self.frozen[l] and self.win[int(l)]), "a frozen learner with a pending window at an advance point"
        super().advance()

    def _update(self, l, k, row_a, row_b, mask):
        """the entry at position k of learner l's window, against the row of s' as it was read before the period's first write"""
        w, gamma, ev = self.win[l], self.cfg.gamma, self.events
        sa, _, coin = w[k]
        dbl = not (self.cfg.quirks & Q_A_ONLY)
        sel_b = bool(dbl and coin)
        sel, val = (row_b, row_a) if sel_b else (row_a, row_b if dbl else row_a)
        best = val[nc.argmax3(sel[0], sel[1], sel[2])]
        g = best * float(mask)
        for i in range(len(w) - 1, k - 1, -1):
            g = w[i][1] + (gamma * g)
        if not 0 <= sa < N_CELLS:
            ev["dropped"] += 1
            return
        c = int(self.cnt[l][sa])
        al = float(self.alpha[c]) if c < len(self.alpha) else float(self.cfg.alpha_min)
        self.cnt[l][sa] += 1
        q = self.qb[l] if sel_b else self.qa[l]
        old = float(q[sa])
        q[sa] = old + al * (g - old)
        ev["writes_b" if sel_b else "writes_a"] += 1
        self.block_updates[sa // CELLS_PER_LEVEL] += 1

    def run(self, periods):
        n, N, ev = self.n, self.nstep, self.events
        i_idx, i_fl, i_code, i_sc, i_rew = self.ii["idx_x"], self.ii["flags"], self.ii["code"], self.ii["step_count"], self.ri["reward"]
        k0, k1 = self.seed & 0xffffffff, (self.seed >> 32) & 0xffffffff
        first = True
        for _ in range(int(periods)):
            j = self.j
            if j % self.E == 0:
                self.advance()
                lens = self.pending_lengths()
                self.open_at_boundaries += int((lens > 0).sum()); self.longest_at_boundaries = max(self.longest_at_boundaries, int(lens.max()))
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
                done = bool(ints[i_fl][l] & 1)
                w = self.win[l]
                # 1. the decision's entry
                w.append([3 * s[l] + a, float(reals[i_rew][l]), int(r[2]) >> 31])
                assert len(w) <= N
                # 2. both tables' row of s', once, before this period's first write
                row_a, row_b = self.qa[l][3 * ns:3 * ns + 3].copy(), self.qb[l][3 * ns:3 * ns + 3].copy()
                # 3. the mask
                mask = ((s[l] // 63) % 3 != (ns // 63) % 3) if (self.cfg.quirks & Q_POS_CHANGE) else (not done)
                # 4. the updates
                if done:
                    m = len(w)
                    ev["flushes"] += 1; ev["flush_entries"] += m; ev["short_flushes"] += m < N; ev["flushes_with_mask_1"] += bool(mask)
                    for i in range(m):
                        self._update(l, i, row_a, row_b, mask)
                    w.clear()
                elif len(w) == N:
                    ev["full_window_updates"] += 1
                    self._update(l, 0, row_a, row_b, mask)
                    w.pop(0)
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
        out = super().result()
        out["pending_len"] = self.pending_lengths()
        assert not (out["pending_len"][out["frozen"]] != 0).any(), "a frozen learner with a pending window"
        return out


# ---- the case: `recipe_checks.CASE` unchanged (trained tables, seed 11, E = 32, 1 024 periods, the three case recipes dealt 5 : 1 : 1), each recipe with an n ----
CASE = rc.CASE
N_BIG, N_SMALL = rc.N_BIG, rc.N_SMALL
NSTEPS_F32, NSTEPS_F64, NSTEPS_WITH_ZERO = (3, 16, 5), (16, 4, 2), (3, 0, 16)


def case_recipes(nsteps, dtype=F32):
    return [dataclasses.replace(r, nstep=int(n)) for r, n in zip(rc.case_recipes(dtype), nsteps)]


def make_yardstick(recipe, n, members, dtype=F32):
    """the yardstick of one recipe (with its own n; n = 0: `RecipeYardstick` itself, the parent path) over n learners, not yet run"""
    args = (rc.case_config(dtype), n, CASE["seed"], recipe, members, CASE["E"])
    if recipe.nstep == 0:
        return rc.RecipeYardstick(*args, CASE["log_capacity"], tables=ec.trained_tables(n))
    return NstepRecipeYardstick(*args, recipe.nstep, CASE["log_capacity"], tables=ec.trained_tables(n))


def case_yardsticks(n, nsteps, dtype=F32, recipes=None, recipe_of=None, periods=None):
    recipes = case_recipes(nsteps, dtype) if recipes is None else recipes
    of = rc.case_recipe_of(n) if recipe_of is None else np.asarray(recipe_of)
    out = []
    for r, recipe in enumerate(recipes):
        y = make_yardstick(recipe, n, of == r, dtype)
        y.run(CASE["periods"] if periods is None else periods)
        out.append(y)
    return out


def yard_result(y):
    """`result()` with the windows' lengths for every yardstick (an n = 0 recipe's are zeros)"""
    out = y.result()
    out.setdefault("pending_len", np.zeros(y.n, np.int32))
    return out


def assert_equal_by_recipe(got, yards, what, recipe_of=None, got_learners=None):
    """`recipe_checks.assert_equal_by_recipe` with `pending_len` among the outputs"""
    n = yards[0].n
    of = rc.case_recipe_of(n) if recipe_of is None else np.asarray(recipe_of)
    for r, y in enumerate(yards):
        rows = [int(l) for l in np.nonzero(of == r)[0]]
        ac.assert_equal(got, yard_result(y), f"{what}, recipe {r}", learners=(rows if got_learners is None else [got_learners[l] for l in rows], rows))


def ensemble_result(ens):
    out = ac.ensemble_result(ens)
    out["pending_len"] = ens.pending_lengths()
    return out


def case_ensemble(n, nsteps, dtype=F32, recipes=None, recipe_of=None):
    return rc.case_ensemble(n, dtype, case_recipes(nsteps, dtype) if recipes is None else recipes, recipe_of)


EVENT_KEYS = ("promoted_from", "exhausted_from", "full_window_updates", "flush_entries", "short_flushes", "open_at_boundaries", "longest_at_boundaries", "open_at_the_end",
              "writes_b", "flushes_with_mask_1")
# (dtype, learners, nsteps) -> per recipe the yardstick's own counts, in EVENT_KEYS' order
EXPECTED = {
    (F32, 28, NSTEPS_F32): (([20, 11, 2, 1, 0], [0, 9, 16, 12, 0], 17950, 552, 3, 521, 2, 14, 0, 0),
                            ([4, 4, 4, 3, 0], [0, 0, 0, 0, 0], 3214, 546, 1, 109, 15, 3, 1922, 0),
                            ([4, 2, 0, 0, 0], [0, 0, 0, 0, 0], 1642, 90, 0, 51, 4, 0, 0, 0)),
    (F32, 112, NSTEPS_F32): (([78, 44, 13, 6, 0], [2, 36, 63, 41, 0], 72797, 2158, 7, 2109, 2, 61, 0, 0),
                             ([16, 16, 16, 13, 0], [0, 0, 0, 0, 0], 12747, 2175, 6, 428, 15, 13, 7544, 0),
                             ([15, 10, 0, 0, 0], [0, 0, 0, 0, 0], 6320, 365, 0, 186, 4, 0, 0, 0)),
}
# float64 at 28 learners with n = (16, 4, 2): what is pinned of it (recipe -> {key: count})
EXPECTED_F64 = {0: dict(full_window_updates=15658, flush_entries=2622, short_flushes=10, open_at_boundaries=525, longest_at_boundaries=15), 1: dict(short_flushes=1)}


def count_events(y):
    if not isinstance(y, NstepRecipeYardstick):
        return None
    end, ev = y.pending_lengths(), y.events
    return (y.promoted_from.tolist(), y.exhausted_from.tolist(), ev["full_window_updates"], ev["flush_entries"], ev["short_flushes"], y.open_at_boundaries,
            y.longest_at_boundaries, int((end > 0).sum()), ev["writes_b"], ev["flushes_with_mask_1"])


def assert_case_events(yards, dtype, n, nsteps):
    """what the case is for, asserted ON THE YARDSTICKS: section 16's conditions, then the n-step events, pinned where the case pins them"""
    rc.assert_case_conditions(yards)
    counts = [count_events(y) for y in yards]
    for r, (y, c) in enumerate(zip(yards, counts)):
        print(f"recipe {r} n {nsteps[r]}:", None if c is None else dict(zip(EVENT_KEYS, c)), "updates by level block", getattr(y, "block_updates", np.zeros(0)).tolist())
        if c is None:
            continue
        ev = dict(zip(EVENT_KEYS, c))
        assert y.events["dropped"] == 0
        assert ev["full_window_updates"] >= 1 and ev["flush_entries"] >= 1 and ev["open_at_boundaries"] >= 1, ev
    key = (dtype, n, tuple(nsteps))
    if key in EXPECTED:
        assert tuple(counts) == EXPECTED[key], f"the yardsticks' event counts moved: {counts} vs {EXPECTED[key]}"
        assert (yards[0].block_updates > 0).all() and (yards[1].block_updates > 0).all(), "updates are to land in all five level blocks in recipes 0 and 1"
    if key == (F64, 28, NSTEPS_F64):
        for r, want in EXPECTED_F64.items():
            ev = dict(zip(EVENT_KEYS, counts[r]))
            assert {k: ev[k] for k in want} == want, f"recipe {r}: the yardstick's event counts moved: {ev} vs {want}"


@functools.lru_cache(maxsize=None)
def case_reference(n, nsteps, dtype=F32):
    """the yardsticks of the case flown through its 1 024 periods, their events asserted (computed once, shared, left unchanged)"""
    yards = case_yardsticks(n, nsteps, dtype)
    assert_case_events(yards, dtype, n, nsteps)
    return yards
