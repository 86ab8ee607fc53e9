"""Shared by the per-learner recipe tests (CPU emulation and GPU): the yardstick, the case and its conditions.

`RecipeYardstick` is `advance_checks.Yardstick` — the unchanged oracle, one per level — for ONE recipe flown over all n learners of the ensemble: the recipe's
quirks in the config (env side and update), its learning-rate table, its per-level schedules, its rule, and its transfer order (`paper_order`:
`oracle.transfer(qa, qb, k + 1, ratios[k + 1])` on entering level k + 1, the level-k block untouched).  Learners outside the member mask start frozen and are
never advanced, so they keep their tables, fly nothing and cost nothing.  The ensemble's learner l is compared with the yardstick of `recipe_of[l]`
(`assert_equal_by_recipe`); every comparison is `==`, floats by their bits (`advance_checks.assert_equal`)."""
import copy
from collections import deque

import numpy as np

from dql_multirotor_landing_amd import ensemble
from dql_multirotor_landing_amd.config import F32, training_config
from dql_multirotor_landing_amd.ensemble import LevelSchedule, Recipe, SequentialEnsemble
from oracle import oracle as orc

import advance_checks as ac
import ensemble_checks as ec

LEVELS = ac.LEVELS
CELLS_PER_LEVEL = ac.CELLS_PER_LEVEL


class CountingTable:
    """a learning-rate table that counts the rates taken from it (the yardstick reads `table[c] if c < len(table) else alpha_min`)"""

    def __init__(self, values):
        self.values, self.taken = np.asarray(values, np.float64), 0

    def __len__(self):
        return len(self.values)

    def __getitem__(self, i):
        self.taken += 1
        return self.values[i]


class RecipeYardstick(ac.Yardstick):
    def __init__(self, cfg, n, seed, recipe: Recipe, members, advance_every, log_capacity=64, tables=None):
        c = copy.deepcopy(cfg)
        c.quirks = int(recipe.quirks)
        if recipe.alpha_min is not None:
            c.alpha_min = float(recipe.alpha_min)
        alpha, _, ratios, lv = recipe.checked(cfg)
        schedules = [dict(eps=e, window=w, min_successes=ms, max_episodes=me) for e, w, ms, me in lv]
        super().__init__(c, n, seed, schedules, ratios, recipe.last_level, advance_every, recipe.advance_exhausted, log_capacity, tables)
        self.alpha = CountingTable(alpha)
        self.paper_order = recipe.transfer_order == ensemble.ORDER_PAPER
        self.members = np.asarray(members, bool).copy()
        assert self.members.shape == (self.n,)
        self.frozen[~self.members] = True  # never flown, never advanced
        self.initial = tuple(t.copy() for t in (self.qa, self.qb, self.cnt))

    def finished(self, l):
        return bool(self.members[l]) and super().finished(l)

    def n_unfinished(self):
        return sum(bool(self.members[l]) and not super(RecipeYardstick, self).finished(l) for l in range(self.n))

    def advance(self):
        """`Yardstick.advance` for the members, with the recipe's transfer order"""
        j = self.j
        for l in np.nonzero(self.members)[0]:
            l = int(l)
            k = int(self.level[l])
            if not self.frozen[l] or k >= self.last_level:
                continue
            if self.promoted[l] < 0 and not self.advance_exhausted:
                continue
            if self.promoted[l] >= 0:
                self.advanced_promoted += 1; self.promoted_from[k] += 1; self.arrived_promoted[l] = k
            else:
                self.advanced_exhausted += 1; self.exhausted_from[k] += 1; self.arrived_promoted.pop(l, None)
            self.promoted_at[k][l] = self.promoted[l]; self.episodes_at[k][l] = self.level_episodes[l]
            if self.paper_order:
                orc.transfer(self.qa[l], self.qb[l], k + 1, self.ratios[k + 1])
            else:
                orc.transfer(self.qa[l], self.qb[l], k, self.ratios[k])
            b = np.ascontiguousarray(self.snap.pop(l)).copy()
            self._mark_done(b)
            self.os[k + 1].envs[self._slot(l)] = b
            self.level[l] = k + 1; self.entered_period[k + 1][l] = j
            self.level_episodes[l] = 0; self.windows[l] = deque([], maxlen=self.sched[k + 1]["W"]); self.promoted[l] = -1; self.frozen[l] = False
            self.freeze_period[l] = -1

    def updates_beyond_the_table(self):
        return int(self.decisions[self.members].sum()) - self.alpha.taken


# ---- the case shared by tests/test_gpu_ensemble_recipes.py and tests/test_recipes_host_emulation.py ----
# On `advance_checks.TRAINED_CASE` (trained tables, seed 11, E = 32, 1 024 periods, level 0 start, log capacity 64): three recipes, dealt 5 : 1 : 1.
#   0: the reference's quirks and order, TRAINED_RATIOS, window 2 / 1 success / 3 episodes, greedy, the config's learning rates (TRAINED_CASE's recipe);
#   1: the coin (Q_PAPER), the paper's order, ratios of its own, window 4 / 2 successes / 6 episodes, greedy, the learning-rate table cut to 32 entries;
#   2: the reference's quirks with the paper's order, TRAINED_RATIOS, last_level 2, exhausted learners stay, exploration (0.25, 0.0) at level 1.
# With n = 112 there are 80 / 16 / 16 members: recipe 0's 80 live learners at level 0 are one segment of two waves, the second padded, in the first launch.
CASE = dict(seed=11, E=32, periods=1024, log_capacity=64)
N_BIG, N_SMALL = 112, 28
PAPER_RATIOS = (0.875, 0.625, 1.25, 0.5, 0.75)


def case_config(dtype=F32):
    return training_config(0, quirks=ec.Q_REFERENCE, dtype=dtype)


def case_recipe_of(n):
    m = np.arange(int(n)) % 7
    return np.where(m < 5, 0, np.where(m == 5, 1, 2)).astype(np.int32)


def case_recipes(dtype=F32):
    greedy = lambda w, ms, me: tuple(LevelSchedule(eps=(0.0,), window=w, min_successes=ms, max_episodes=me) for _ in range(LEVELS))
    r2 = list(greedy(2, 1, 3))
    r2[1] = LevelSchedule(eps=(0.25, 0.0), window=2, min_successes=1, max_episodes=3)
    return [Recipe(quirks=ec.Q_REFERENCE, transfer_order=ensemble.ORDER_REFERENCE, ratios=ac.TRAINED_RATIOS, levels=greedy(2, 1, 3)),
            Recipe(quirks=ec.Q_PAPER, transfer_order=ensemble.ORDER_PAPER, ratios=PAPER_RATIOS, levels=greedy(4, 2, 6), alpha_table=tuple(case_config(dtype).alpha_table()[:32].tolist())),
            Recipe(quirks=ec.Q_REFERENCE, transfer_order=ensemble.ORDER_PAPER, ratios=ac.TRAINED_RATIOS, last_level=2, advance_exhausted=False, levels=tuple(r2))]


def case_yardsticks(n, dtype=F32, periods=None, checkpoint_every=None, recipes=None, recipe_of=None):
    """one yardstick per recipe over all n learners, flown through the case; with checkpoint_every, `y.checkpoints` holds after every run of that many periods
    (period index, n_unfinished(), what `SequentialEnsemble.levels()` shows, the recipe's entry of `recipe_summary()`)"""
    recipes = case_recipes(dtype) if recipes is None else recipes
    of = case_recipe_of(n) if recipe_of is None else np.asarray(recipe_of)
    periods = CASE["periods"] if periods is None else periods
    out = []
    for r, recipe in enumerate(recipes):
        y = RecipeYardstick(case_config(dtype), n, CASE["seed"], recipe, of == r, CASE["E"], CASE["log_capacity"], tables=ec.trained_tables(n))
        y.checkpoints = []
        for _ in range(periods // (checkpoint_every or periods)):
            y.run(checkpoint_every or periods)
            res = y.result()
            y.checkpoints.append((y.j, y.n_unfinished(), {k: res[k] for k in ("level",) + ac.HISTORY[1:]}, summary_entry(y)))
        out.append(y)
    return out


def case_ensemble(n, dtype=F32, recipes=None, recipe_of=None):
    """a SequentialEnsemble set up for the case (curriculum mode on, the recipes installed), not yet run"""
    ens = SequentialEnsemble(case_config(dtype), n, seed=CASE["seed"], log_capacity=CASE["log_capacity"])
    ens.set_curriculum(4, CASE["E"])
    ens.set_recipes(case_recipes(dtype) if recipes is None else recipes, case_recipe_of(n) if recipe_of is None else recipe_of)
    ens.set_tables(*ec.trained_tables(n))
    return ens


def assert_equal_by_recipe(got, yards, what, recipe_of=None, got_learners=None):
    """learner l of `got` against the yardstick of its recipe; got_learners: the rows of `got` that hold the yardsticks' learners 0 .. (default: the same)"""
    n = yards[0].n
    of = case_recipe_of(n) if recipe_of is None else np.asarray(recipe_of)
    for r, y in enumerate(yards):
        rows = [int(l) for l in np.nonzero(of == r)[0]]
        ac.assert_equal(got, y.result(), f"{what}, recipe {r}", learners=(rows if got_learners is None else [got_learners[l] for l in rows], rows))


def summary_entry(y):
    """a recipe's entry of `SequentialEnsemble.recipe_summary`, from its yardstick: a learner counts at level k once it has left it or stands frozen on it"""
    m, res = y.members, y.result()
    left = lambda k: m & ((res["level"] > k) | ((res["level"] == k) & res["frozen"]))
    return {"members": int(m.sum()), "learners_per_level": np.bincount(res["level"][m], minlength=LEVELS).tolist(),
            "promoted_per_level": [int((left(k) & (res["promoted_at"][k] >= 0)).sum()) for k in range(LEVELS)],
            "exhausted_per_level": [int((left(k) & (res["promoted_at"][k] < 0)).sum()) for k in range(LEVELS)], "finished": sum(bool(y.finished(l)) for l in range(y.n))}


def assert_case_conditions(yards):
    """what the case is for, asserted ON THE YARDSTICKS before an ensemble or an emulation is looked at"""
    y0, y1, y2 = yards
    for r, y in enumerate(yards):
        res = y.result()
        print(f"recipe {r}: members", int(y.members.sum()), "promoted advances by level left", y.promoted_from.tolist(), "exhausted", y.exhausted_from.tolist(),
              "levels at the end", np.bincount(res["level"][y.members], minlength=LEVELS).tolist(), "finished", sum(y.finished(l) for l in range(y.n)), "unfinished", y.n_unfinished(),
              "updates beyond the learning-rate table", y.updates_beyond_the_table(), "first launch (period, live per level)", y.launches[0][:2])
        assert (y.promoted_from > 0).sum() >= 2, f"recipe {r}: promoted advances from at least two levels are needed"
        out = ~y.members  # non-members keep their tables and fly nothing
        assert all(np.array_equal(t[out], t0[out]) for t, t0 in zip((res["qa"], res["qb"], res["count"]), y.initial)) and not res["decisions"][out].any()
    assert y0.exhausted_from.sum() >= 1, "recipe 0: exhausted advances are needed as well"
    r1 = y1.result()
    start = slice(0, CELLS_PER_LEVEL)
    assert (r1["qb"][y1.members][:, start] != y1.initial[1][y1.members][:, start]).any(), "recipe 1: the coin never picked Q_table_b"
    assert y1.updates_beyond_the_table() >= 1 and y1.alpha.taken >= 1, "recipe 1: no learning rate was taken from beyond the 32-entry table"
    r2 = y2.result()
    m2 = y2.members
    assert r2["level"][m2].max() <= 2 and (r2["entered_period"][3:, m2] == -1).all(), "recipe 2: somebody above level 2"
    exhausted = m2 & r2["frozen"] & (r2["promotion_episode"] < 0) & (r2["level"] < 2)
    assert exhausted.sum() >= 1 and y2.exhausted_from.sum() == 0, "recipe 2: one learner finished by exhaustion (out of episodes below last_level, staying for good) is needed"
    if y0.n > 64:
        live0 = y0.launches[0][1][0]
        assert live0 > 64 and live0 % 64 != 0, "recipe 0: the first launch has no segment of two waves, the second padded"
