"""Shared by the flush-bootstrap tests (CPU host checks, CPU emulations and GPU): flights on which an n-step learner's episode-end flush bootstraps
(DESIGN.md section 25).

On the default config a terminal period never changes the position bin (fly-zone exits and touchdowns), so under DQL_Q_BOOTSTRAP_ON_POS_CHANGE the mask of
every flush is 0 and both coins' chains are the same number.  `bootstrap_config` ends episodes by timeout after one second, wherever the drone is, and flies
with the as-launched observation noise, which makes the position bin flicker: about one flush in ten then has mask 1.

Nothing here knows of the kernels.  The yardsticks are the UNCHANGED ones of nstep_checks, team_nstep_checks and nstep_recipe_checks; `Counting*` subclass
them to count what happens at a flush with mask 1 (`_FlushWatch`, which only looks), and three MUTANTS per yardstick, subclasses again, make the three
mistakes a body can make there.  Every row asserts ON THE YARDSTICK that its events occurred, pins the counts to the digit (`EXPECTED`, from the yardstick's
own print), and is cached: computed once per process, shared, left unchanged.

The flush counters (all of flushes with mask 1; the last five of those with at least two entries, side by side, not nested):
  mask_1               flushes with mask 1
  two_entries          ... whose window holds at least two entries
  both_coins           ... whose entries carry both coins (the drawn coin bit; it selects a table only where DQL_Q_UPDATE_TABLE_A_ONLY is clear)
  distinct_bootstraps  ... whose two bootstraps — `best` by coin a, `best` by coin b, from the row of s' as read — differ in their bits
  nonzero_bootstrap    ... with a bootstrap that is not zero
  stale_row_entries    updated entries of those flushes for which the row of s' in the tables no longer has the bits it was read with
  row_after_write      (teams) ... whose row of s' was read after a team-mate's write of the same period"""
import functools

import numpy as np

from dql_multirotor_landing_amd.config import F32, F64, Q_BOOTSTRAP_ON_POS_CHANGE as Q_POS_CHANGE, Q_UPDATE_TABLE_A_ONLY as Q_A_ONLY, training_config
from dql_multirotor_landing_amd.ensemble import LevelSchedule, Recipe, SequentialEnsemble

import ensemble_checks as ec
import nstep_checks as nc
import nstep_recipe_checks as nr
import recipe_checks as rc
import team_checks as tc
import team_nstep_checks as tn

Q_POS_COIN, Q_REFERENCE = 0x50, ec.Q_REFERENCE  # the position-change mask with the coin (bit 4 set, bit 5 clear); the reference's word (bit 4 set, table a alone)


def bootstrap_config(level, quirks, dtype):
    return training_config(level, quirks=quirks, dtype=dtype, t_max=1.0, noise_pos_sd=0.25, noise_vel_sd=0.1)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).tobytes()


# ---- the counters and the mutants ----
MUTANTS = ("reread", "nomask", "swapcoin")
FLUSH_KEYS = ("mask_1", "two_entries", "both_coins", "distinct_bootstraps", "nonzero_bootstrap", "stale_row_entries")


class _FlushWatch:
    """Mixed in before a yardstick: `_watch` is called at the head of `_update` with the update's arguments.  It tells a flush's updates from a full window's
    (the yardsticks count `flushes` before a flush's first update, and a flush updates positions 0 .. m - 1 of a window of m entries), counts FLUSH_KEYS, and
    — in a mutant only — hands back changed arguments:
      reread    the row of s' as the tables stand at this entry's update (not as it was read once, before the first)
      nomask    mask 0 at a flush ("terminal, so no bootstrap")
      swapcoin  at a flush with mask 1 under Double Q-learning, the OTHER coin's bootstrap for the entry's value (rows a and b swapped: `best` is then the
                selecting and the valuing table exchanged); the table written is the entry's own"""
    mutant = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._fb_seen, self._fb_left, self._fb_counted, self._fb_ns = 0, 0, False, -1

    def _watch(self, l, env, k, row_a, row_b, mask, ns=None, written=None):
        ev = self.events
        if ev["flushes"] != self._fb_seen:  # the first update of a flush
            assert k == 0 and self._fb_left == 0
            w = self.win[env]
            self._fb_seen, self._fb_left = ev["flushes"], len(w)
            self._fb_ns = self._next_state(l, env) if ns is None else int(ns)
            self._fb_counted = bool(mask)
            if mask:
                dbl = not (self.cfg.quirks & Q_A_ONLY)
                best_a = (row_b if dbl else row_a)[nc.argmax3(*row_a)]
                best_b = row_a[nc.argmax3(*(row_b if dbl else row_a))]
                ev["mask_1"] += 1
                if len(w) >= 2:
                    ev["two_entries"] += 1
                    ev["both_coins"] += len({x[2] for x in w}) == 2
                    ev["distinct_bootstraps"] += _bits(best_a) != _bits(best_b)
                    ev["nonzero_bootstrap"] += bool(best_a != 0.0 or best_b != 0.0)
                if written is not None:
                    ev["row_after_write"] += self._fb_ns in written
        if self._fb_left == 0:
            return row_a, row_b, mask  # a full window's single update
        self._fb_left -= 1
        s = 3 * self._fb_ns
        now_a, now_b = self.qa[l][s:s + 3], self.qb[l][s:s + 3]
        if self._fb_counted:
            ev["stale_row_entries"] += _bits(now_a) != _bits(row_a) or _bits(now_b) != _bits(row_b)
        if self.mutant == "reread":
            return now_a.copy(), now_b.copy(), mask
        if self.mutant == "nomask":
            return row_a, row_b, False
        if self.mutant == "swapcoin" and mask and not (self.cfg.quirks & Q_A_ONLY):
            return row_b, row_a, mask
        return row_a, row_b, mask


class CountingNstep(_FlushWatch, nc.NstepReference):
    def _update(self, l, k, row_a, row_b, mask, ns, newest):
        row_a, row_b, mask = self._watch(l, l, k, row_a, row_b, mask, ns=ns)
        return super()._update(l, k, row_a, row_b, mask, ns, newest)


class CountingTeamNstep(_FlushWatch, tn.TeamNstepReference):
    def _next_state(self, l, g):
        return int(self.o.get_fields()[1][self.ii["idx_x"]][g])

    def _update(self, l, g, k, row_a, row_b, mask, rows):
        row_a, row_b, mask = self._watch(l, g, k, row_a, row_b, mask, written=rows)
        return super()._update(l, g, k, row_a, row_b, mask, rows)


class CountingNstepRecipe(_FlushWatch, nr.NstepRecipeYardstick):
    def _next_state(self, l, env):
        return int(self.os[int(self.level[l])].get_fields()[1][self.ii["idx_x"]][l])

    def _update(self, l, k, row_a, row_b, mask):
        row_a, row_b, mask = self._watch(l, l, k, row_a, row_b, mask)
        return super()._update(l, k, row_a, row_b, mask)


def mutant_of(base, name):
    """the subclass of a Counting* yardstick that makes the mistake `name`"""
    assert name in MUTANTS
    return type(f"{base.__name__}_{name}", (base,), {"mutant": name})


def applicable_mutants(quirks):
    return MUTANTS if not (quirks & Q_A_ONLY) else MUTANTS[:2]


def cells_changed(mutant, ref):
    """cells of qa and qb in which a mutant's flight differs from the unmutated yardstick's (by their bits)"""
    return sum(int((np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).sum()) for a, b in ((mutant.qa, ref.qa), (mutant.qb, ref.qb)))


def assert_conditions(ev, quirks, what):
    """what every row is for — not measurements: the probe behind the rows meets each with room to spare"""
    assert quirks & Q_POS_CHANGE, what
    assert ev["dropped"] == 0, what
    assert ev["mask_1"] >= 20, f"{what}: {ev['mask_1']} flushes with mask 1, 20 are needed"
    assert ev["two_entries"] == ev["mask_1"], f"{what}: a flush with mask 1 has a single entry"
    assert ev["full_window_updates"] >= 1000, f"{what}: {ev['full_window_updates']} full-window updates, 1000 are needed"
    if not (quirks & Q_A_ONLY):
        assert ev["both_coins"] >= 10 and ev["distinct_bootstraps"] >= 10, f"{what}: both coins {ev['both_coins']}, distinct bootstraps {ev['distinct_bootstraps']}, 10 of each are needed"


def _counts(ref, keys):
    ev = dict(ref.events)
    return tuple(int(ev.get(k, 0)) for k in keys)


def _name(dtype):
    return "f64" if dtype == F64 else "f32"


# ---- plain n-step learners (set_nstep, k_learn_nstep): seed 2024, EPS_TABLE, 300 periods, flown as 300 and as 7 + 293 ----
PLAIN_SEED, PLAIN_PERIODS, PLAIN_SPLIT, PLAIN_LOG = nc.MAIN_SEED, 300, (7, 293), nc.MAIN_LOG
PLAIN_ROWS = [(0, Q_POS_COIN, F32, 16), (4, Q_POS_COIN, F32, 4), (4, Q_POS_COIN, F64, 16), (3, Q_REFERENCE, F32, 16), (0, Q_REFERENCE, F32, 4)]  # level (>= 1: trained tables), quirks, dtype, n
PLAIN_IDS = [f"level-{lv}-quirks-{q:#x}-{_name(d)}-n{n}" for lv, q, d, n in PLAIN_ROWS]
PLAIN_KEYS = ("flushes", "full_window_updates", "flush_entries", "short_flushes") + FLUSH_KEYS
# (level, quirks, dtype, n, learners) -> the yardstick's own counts, in PLAIN_KEYS' order (printed by plain_reference; DESIGN.md section 25 has the table)
PLAIN_EXPECTED = {
    (0, 0x50, F32, 16, 26): (313, 2162, 4998, 2, 32, 32, 32, 13, 13, 100),
    (0, 0x50, F32, 16, 70): (845, 5812, 13457, 9, 76, 76, 76, 32, 32, 244),
    (4, 0x50, F32, 4, 26): (347, 6016, 1341, 20, 38, 38, 33, 38, 38, 5),
    (4, 0x50, F32, 4, 70): (928, 16226, 3585, 55, 122, 122, 108, 122, 122, 26),
    (4, 0x50, F64, 16, 26): (346, 2119, 5081, 41, 38, 38, 38, 38, 38, 38),
    (4, 0x50, F64, 16, 70): (927, 5741, 13611, 111, 125, 125, 125, 125, 125, 58),
    (3, 0x7f, F32, 16, 26): (346, 2115, 5111, 42, 30, 30, 30, 0, 30, 39),
    (3, 0x7f, F32, 16, 70): (936, 5692, 13710, 122, 84, 84, 84, 0, 84, 76),
    (0, 0x7f, F32, 4, 26): (313, 6133, 1252, 0, 23, 23, 22, 0, 8, 20),
    (0, 0x7f, F32, 4, 70): (848, 16493, 3389, 2, 62, 62, 55, 0, 21, 34),
}


def plain_tables(level, learners):
    return ec.trained_tables(learners) if level >= 1 else None


def fly_plain(cls, level, quirks, dtype, nstep, learners, periods=PLAIN_PERIODS):
    ref = cls(bootstrap_config(level, quirks, dtype), learners, PLAIN_SEED, nstep, log_capacity=PLAIN_LOG, tables=plain_tables(level, learners))
    ref.run(periods)
    return ref


@functools.lru_cache(maxsize=None)
def _plain_flight(level, quirks, dtype, nstep, learners):
    return fly_plain(CountingNstep, level, quirks, dtype, nstep, learners)


@functools.lru_cache(maxsize=None)
def plain_reference(level, quirks, dtype, nstep, learners):
    """(result, events as a dict) of the yardstick on a plain row, after asserting ON IT what the row is for and its pinned counts"""
    ref = _plain_flight(level, quirks, dtype, nstep, learners)
    want = ref.result()
    counts = _counts(ref, PLAIN_KEYS)
    ev = dict(zip(PLAIN_KEYS, counts), dropped=ref.events["dropped"])
    what = f"plain row level {level} quirks {quirks:#x} {_name(dtype)} n {nstep} learners {learners}"
    print(what + ":", ev, "counts", counts)
    assert_conditions(ev, quirks, what)
    key = (level, quirks, dtype, nstep, learners)
    assert key in PLAIN_EXPECTED and counts == PLAIN_EXPECTED[key], f"{what}: the yardstick's event counts moved: {counts} vs {PLAIN_EXPECTED.get(key)}"
    return want, ev


@functools.lru_cache(maxsize=None)
def plain_mutant_cells(level, quirks, dtype, nstep, learners, name):
    return cells_changed(fly_plain(mutant_of(CountingNstep, name), level, quirks, dtype, nstep, learners), _plain_flight(level, quirks, dtype, nstep, learners))


# ---- team n-step learners (set_team_nstep, k_learn_team_nstep): seed 11, eps 0.3, window 100, 97 successes, 150 periods, flown as 150 and as 7 + 143 ----
TEAM_SEED, TEAM_PERIODS, TEAM_SPLIT = tc.SEED, 150, (7, 143)
TEAM_SCHED = dict(eps=[0.3], window=100, min_successes=97, max_episodes=1 << 30, log_capacity=64)
TEAM_ROWS = [(4, Q_POS_COIN, 3, 16, 16, F32), (4, Q_POS_COIN, 2, 64, 4, F32), (4, Q_POS_COIN, 2, 64, 4, F64), (0, Q_REFERENCE, 2, 64, 4, F32), (0, Q_POS_COIN, 3, 16, 16, F32)]  # level, quirks, L, E, n, dtype
TEAM_IDS = [f"level-{lv}-quirks-{q:#x}-L{L}xE{E}-n{n}-{_name(d)}" for lv, q, L, E, n, d in TEAM_ROWS]
TEAM_KEYS = PLAIN_KEYS + ("row_after_write", "row_after_write_at_flush", "row_after_write_at_full")
# row -> the yardstick's own counts, in TEAM_KEYS' order (printed by team_reference)
TEAM_EXPECTED = {
    (4, 0x50, 3, 16, 16, F32): (313, 1947, 4646, 32, 33, 33, 33, 33, 33, 14, 1, 52, 53),
    (4, 0x50, 2, 64, 4, F32): (844, 14652, 3244, 55, 91, 91, 77, 91, 91, 27, 9, 211, 2721),
    (4, 0x50, 2, 64, 4, F64): (844, 14652, 3244, 55, 91, 91, 77, 91, 91, 27, 9, 211, 2721),
    (0, 0x7f, 2, 64, 4, F32): (772, 14840, 3077, 4, 64, 64, 55, 0, 58, 42, 36, 407, 5198),
    (0, 0x50, 3, 16, 16, F32): (290, 1995, 4611, 2, 26, 26, 26, 23, 23, 51, 12, 156, 134),
}


def fly_team(cls, level, quirks, L, E, nstep, dtype, periods=TEAM_PERIODS):
    ref = cls(bootstrap_config(level, quirks, dtype), L, E, TEAM_SEED, nstep, tables=plain_tables(level, L), **TEAM_SCHED)
    ref.run(periods)
    return ref


@functools.lru_cache(maxsize=None)
def _team_flight(level, quirks, L, E, nstep, dtype):
    return fly_team(CountingTeamNstep, level, quirks, L, E, nstep, dtype)


@functools.lru_cache(maxsize=None)
def team_reference(level, quirks, L, E, nstep, dtype):
    """(result, events as a dict) of the yardstick on a team row, after asserting ON IT what the row is for and its pinned counts"""
    ref = _team_flight(level, quirks, L, E, nstep, dtype)
    want = ref.result()
    counts = _counts(ref, TEAM_KEYS)
    ev = dict(zip(TEAM_KEYS, counts), dropped=ref.events["dropped"])
    what = f"team row level {level} quirks {quirks:#x} L {L} E {E} n {nstep} {_name(dtype)}"
    print(what + ":", ev, "counts", counts, "frozen", int(want["frozen"].sum()))
    assert_conditions(ev, quirks, what)
    assert ev["row_after_write"] >= 1, f"{what}: no flush with mask 1 read its row after a team-mate's write of the same period"
    assert not want["frozen"].any()
    key = (level, quirks, L, E, nstep, dtype)
    assert key in TEAM_EXPECTED and counts == TEAM_EXPECTED[key], f"{what}: the yardstick's event counts moved: {counts} vs {TEAM_EXPECTED.get(key)}"
    return want, ev


@functools.lru_cache(maxsize=None)
def team_mutant_cells(level, quirks, L, E, nstep, dtype, name):
    return cells_changed(fly_team(mutant_of(CountingTeamNstep, name), level, quirks, L, E, nstep, dtype), _team_flight(level, quirks, L, E, nstep, dtype))


def team_ensemble(level, quirks, L, E, nstep, dtype):
    """a team SequentialEnsemble set up for a team row (nstep 0: k_learn_team), not yet run"""
    ens = SequentialEnsemble(bootstrap_config(level, quirks, dtype), L, seed=TEAM_SEED, envs_per_learner=E, team_nstep=nstep, **TEAM_SCHED)
    if level >= 1:
        ens.set_tables(*ec.trained_tables(L))
    return ens


# ---- per-recipe n-step (set_recipe_nstep, k_learn_recipes_nstep): one ensemble, five recipes that differ in quirks and n, dealt round-robin ----
# `recipe_checks.CASE`'s seed, advance interval, log capacity and trained tables; every learner starts at level RECIPE_LEVEL and stays there: under
# `bootstrap_config` episodes end by timeout, nobody lands, and 97 successes of 100 are out of reach, so nobody freezes and nobody advances (asserted).  The
# advance rule is not what is under test here.
RECIPE_SPECS = ((Q_POS_COIN, 4), (Q_POS_COIN, 16), (Q_REFERENCE, 16), (ec.Q_PAPER, 4), (Q_POS_COIN, 0))  # (quirks, n) per recipe
RECIPE_CASE = dict(rc.CASE, periods=600)
RECIPE_LEVEL, RECIPE_N, RECIPE_SPLIT = 4, 60, (7, 593)
RECIPE_KEYS = PLAIN_KEYS
# per recipe with n >= 1 the yardstick's own counts, in RECIPE_KEYS' order (printed by recipe_reference)
RECIPE_EXPECTED = {
    0: (321, 5594, 1237, 21, 35, 35, 27, 35, 35, 19),
    1: (318, 2034, 4729, 30, 46, 46, 46, 46, 46, 9),
    2: (341, 1921, 4837, 61, 29, 29, 29, 0, 29, 16),
    3: (322, 5587, 1249, 17, 0, 0, 0, 0, 0, 0),
}


def recipe_config(dtype=F32):
    return bootstrap_config(RECIPE_LEVEL, Q_REFERENCE, dtype)


def recipe_recipes():
    lv = tuple(LevelSchedule(eps=(0.3,), window=100, min_successes=97, max_episodes=1 << 30) for _ in range(rc.LEVELS))
    return [Recipe(quirks=q, levels=lv, nstep=n) for q, n in RECIPE_SPECS]


def recipe_of(n=RECIPE_N):
    return (np.arange(int(n)) % len(RECIPE_SPECS)).astype(np.int32)


def fly_recipe(r, cls=CountingNstepRecipe, n=RECIPE_N):
    """the yardstick of recipe r over its members of the n learners, flown through the case"""
    recipe, c = recipe_recipes()[r], RECIPE_CASE
    args = (recipe_config(), n, c["seed"], recipe, recipe_of(n) == r, c["E"])
    y = rc.RecipeYardstick(*args, c["log_capacity"], tables=ec.trained_tables(n)) if recipe.nstep == 0 else cls(*args, recipe.nstep, c["log_capacity"], tables=ec.trained_tables(n))
    y.run(c["periods"])
    return y


@functools.lru_cache(maxsize=None)
def _recipe_flight(r):
    return fly_recipe(r)


@functools.lru_cache(maxsize=None)
def recipe_reference():
    """the five yardsticks of the recipe case, after asserting ON THEM what the case is for and its pinned counts"""
    yards = [_recipe_flight(r) for r in range(len(RECIPE_SPECS))]
    for r, (y, (quirks, nstep)) in enumerate(zip(yards, RECIPE_SPECS)):
        res = y.result()
        assert not res["frozen"][y.members].any() and (res["level"][y.members] == RECIPE_LEVEL).all() and res["episodes"][y.members].min() >= 1, f"recipe {r}: its learners were to fly on at their level"
        if nstep == 0:
            assert type(y) is rc.RecipeYardstick
            continue
        counts = _counts(y, RECIPE_KEYS)
        ev = dict(zip(RECIPE_KEYS, counts), dropped=y.events["dropped"])
        what = f"recipe {r} quirks {quirks:#x} n {nstep} members {int(y.members.sum())}"
        print(what + ":", ev, "counts", counts)
        if quirks & Q_POS_CHANGE:
            assert_conditions(ev, quirks, what)
        else:
            assert ev["mask_1"] == 0 and ev["flushes"] >= 20 and ev["dropped"] == 0, f"{what}: without the position-change mask a flush's mask is 0"
        assert r in RECIPE_EXPECTED and counts == RECIPE_EXPECTED[r], f"{what}: the yardstick's event counts moved: {counts} vs {RECIPE_EXPECTED.get(r)}"
    return yards


@functools.lru_cache(maxsize=None)
def recipe_mutant_cells(r, name):
    return cells_changed(fly_recipe(r, mutant_of(CountingNstepRecipe, name)), _recipe_flight(r))


def recipe_ensemble(n=RECIPE_N, dtype=F32):
    """a SequentialEnsemble set up for the recipe case (curriculum mode on, the recipes installed), not yet run"""
    c = RECIPE_CASE
    ens = SequentialEnsemble(recipe_config(dtype), n, seed=c["seed"], log_capacity=c["log_capacity"])
    ens.set_curriculum(4, c["E"])
    ens.set_recipes(recipe_recipes(), recipe_of(n))
    ens.set_tables(*ec.trained_tables(n))
    return ens


# ---- the one-step anchors under the same config: level 4 from trained tables, so that a terminal's bootstrap is not zero ----
ANCHOR_LEVEL = 4
ANCHOR_ROWS = [(Q_POS_COIN, F32), (Q_REFERENCE, F32), (Q_POS_COIN, F64)]
ANCHOR_IDS = [f"quirks-{q:#x}-{_name(d)}" for q, d in ANCHOR_ROWS]
ANCHOR_TEAM = dict(L=3, E=16)


def _assert_anchor(ref, what):
    ev = ref.events
    print(what + ":", {k: int(ev[k]) for k in ("flushes", "terminal_nonzero_bootstrap") + FLUSH_KEYS})
    assert ev["dropped"] == 0 and ev["two_entries"] == 0
    assert ev["mask_1"] >= 20, f"{what}: {ev['mask_1']} terminal transitions with mask 1, 20 are needed"


@functools.lru_cache(maxsize=None)
def plain_anchor(quirks, dtype, learners):
    """(the one-step reference loop's result, terminal transitions with mask 1) on `bootstrap_config`: `ensemble_checks.Reference`, with `NstepReference` at
    n = 1 — asserted `==` to it here — counting the terminal transitions with mask 1 and the non-zero bootstraps among them"""
    cfg, tables = bootstrap_config(ANCHOR_LEVEL, quirks, dtype), ec.trained_tables(learners)
    one = ec.Reference(cfg, learners, PLAIN_SEED, log_capacity=PLAIN_LOG, tables=tables)
    one.run(PLAIN_PERIODS)
    want = one.result()
    ref = _AnchorNstep(cfg, learners, PLAIN_SEED, 1, log_capacity=PLAIN_LOG, tables=tables)
    ref.run(PLAIN_PERIODS)
    _assert_anchor(ref, f"plain anchor quirks {quirks:#x} {_name(dtype)} learners {learners}")
    assert ref.events["terminal_nonzero_bootstrap"] >= 10
    got = ref.result()
    assert (got.pop("pending_len") == 0).all()
    ec.assert_equal(got, want, "NstepReference at n = 1 against the one-step reference loop")
    return want, int(ref.events["mask_1"])


@functools.lru_cache(maxsize=None)
def team_anchor(quirks, dtype):
    cfg, L, E = bootstrap_config(ANCHOR_LEVEL, quirks, dtype), ANCHOR_TEAM["L"], ANCHOR_TEAM["E"]
    one = tc.TeamReference(cfg, L, E, TEAM_SEED, tables=ec.trained_tables(L), **TEAM_SCHED)
    one.run(TEAM_PERIODS)
    want = one.result()
    ref = _AnchorTeamNstep(cfg, L, E, TEAM_SEED, 1, tables=ec.trained_tables(L), **TEAM_SCHED)
    ref.run(TEAM_PERIODS)
    _assert_anchor(ref, f"team anchor quirks {quirks:#x} {_name(dtype)}")
    assert ref.events["terminal_nonzero_bootstrap"] >= 10
    got = ref.result()
    assert (got.pop("team_pending_len") == 0).all()
    tc.assert_equal(got, want, "TeamNstepReference at n = 1 against the team reference loop")
    return want, int(ref.events["mask_1"])


class _AnchorWatch:
    """at n = 1 every window has one entry, so `two_entries` and what hangs on it stay 0: the non-zero bootstraps of terminal transitions are counted apart"""

    def _watch(self, l, env, k, row_a, row_b, mask, ns=None, written=None):
        if self.events["flushes"] != self._fb_seen and mask:
            dbl = not (self.cfg.quirks & Q_A_ONLY)
            best_a, best_b = (row_b if dbl else row_a)[nc.argmax3(*row_a)], row_a[nc.argmax3(*(row_b if dbl else row_a))]
            self.events["terminal_nonzero_bootstrap"] += bool(best_a != 0.0 and best_b != 0.0)
        return super()._watch(l, env, k, row_a, row_b, mask, ns=ns, written=written)


class _AnchorNstep(_AnchorWatch, CountingNstep):
    pass


class _AnchorTeamNstep(_AnchorWatch, CountingTeamNstep):
    pass
