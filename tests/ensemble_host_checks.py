"""What the host code of the sequential learners does around its kernels, as two tables (tests/golden/ensemble_host.json holds both as the library answered
when the fixture was recorded, tests/golden/make_ensemble_host.py --record; tests/test_gpu_ensemble_host.py holds every later build to it, to the letter).

REFUSALS: for every dql_ensemble_* / dql_diag_ensemble_* call that can refuse (the two creators included; the five greedy twins are
tests/greedy_refusal_checks.py's) one call per argument check with that one argument bad, calls with TWO bad arguments that pin the order of the checks, and
the refusals that depend on the ensemble's state (a pending window that holds entries, a recipe without a rule, learners on different levels ...).  A row is
(entry point, case) -> (return code, dql_last_error text).  A case names the STATE the ensemble is in (STATES) and the keyword arguments that differ from the
call's valid ones.  After every refused call rows_of() asserts that nothing moved: n and the pending lengths, recipe_of, every recipe's n, the level history,
the period index, n_unfinished and the launches triple are what they were before the call.  4 learners, float32, log_capacity 2; teams: 2 learners x 2 envs.

RUNS: per mode a short script of dql_ensemble_run calls on 70 learners (two waves, the second partial; the team mode: 18 learners x 4 envs), recorded call by
call: the launches triple, period_index, n_live, n_unfinished and a SHA-256 over tables, counters, level history, env state and pending lengths.  The kernels
are deterministic and held bit for bit to their yardsticks elsewhere; here the hash only says "the host flew the same launches on the same learners".  Every
script has a call that ends before the next advance point, one that crosses three, one that starts exactly on one (the worklist modes, advance_every 8), and a
second ensemble on which every learner finishes mid-call: the period index advances by the whole call, the launch count does not.  The plain-loop scripts
have one call of 4097 periods (two launches, 4096 + 1) and calls on an all-frozen ensemble."""
import ctypes as C
import dataclasses
import hashlib
import math

import numpy as np

from dql_multirotor_landing_amd import _lib
from dql_multirotor_landing_amd.config import F32, F64, training_config
from dql_multirotor_landing_amd.ensemble import LevelSchedule, ORDER_PAPER, REFERENCE_RATIOS, Recipe, SequentialEnsemble

import ensemble_checks as ec

LEARNERS, LOG_CAP, SEED = 4, 2, 7
NAN = float("nan")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cfg(dtype=F32, **kw):
    return training_config(0, quirks=ec.Q_PAPER, dtype=dtype, **kw)


# ---- the states a refused call finds the ensemble in ----
def _plain(**kw):
    return SequentialEnsemble(_cfg(), LEARNERS, seed=SEED, log_capacity=LOG_CAP, eps=[0.0], **kw)


def _levels(ens, upto=5, **kw):
    for k in range(upto):
        ens.set_level_schedules(k, [0.0], **kw)
    return ens


def _curriculum(ens=None, last_level=4, upto=5, **kw):
    ens = _levels(_plain() if ens is None else ens, upto, **kw)
    ens.set_curriculum(last_level, 8)
    return ens


def _recipe(last_level=4, nstep=0, order=0):
    return Recipe(quirks=ec.Q_PAPER, last_level=last_level, transfer_order=order, nstep=nstep, levels=tuple(LevelSchedule(eps=[0.0]) for _ in range(5)))


RECIPE_OF = np.array([0, 1, 0, 1], dtype=np.int32)


def _recipes(r0=None, r1=None):
    ens = _curriculum()
    ens.set_recipes([r0 or _recipe(), r1 or _recipe(order=ORDER_PAPER)], RECIPE_OF)
    return ens


def _recipes_bare(rules=False):
    """recipes installed by the library call alone: no rule (or, with `rules`, the rules and the level-0 schedules, nothing for the levels on the way up)"""
    ens, lib = _curriculum(), _lib.load()
    _lib.check(lib.dql_ensemble_set_recipes(ens._h, 2, _ptr(RECIPE_OF)))
    alpha, ratios, eps = np.array([0.1]), np.array(REFERENCE_RATIOS), np.array([0.0])
    for r in range(2 if rules else 0):
        _lib.check(lib.dql_ensemble_set_recipe(ens._h, r, ec.Q_PAPER, _ptr(alpha), 1, 0.1, _ptr(ratios), 4, 1, 0))
        _lib.check(lib.dql_ensemble_set_recipe_level_schedules(ens._h, r, 0, _ptr(eps), 1, 100, 97, 50000))
    return ens


def _ran(ens, periods, want_open=False):
    ens.run(periods)
    assert ens.n_live() == ens.n and ens.index_faults() == 0
    assert not want_open or (ens.pending_lengths() > 0).all(), "every window should hold entries"
    return ens


def _nstep(n=4):
    ens = _plain()
    ens.set_nstep(n)
    return ens


def _spread():
    """curriculum mode from trained tables, one episode per level: after 1 024 periods learners stand on levels that are not the config's"""
    ens = _curriculum(window=1, min_successes=1, max_episodes=1)
    ens.set_tables(*ec.trained_tables(LEARNERS))
    ens.run(1024)
    assert (ens.levels()["level"] != 0).any()
    return ens


def _at_level(ens, k):
    ens.set_level(k)
    return ens


def _team1_curriculum():
    return _curriculum(SequentialEnsemble(_cfg(), LEARNERS, seed=SEED, log_capacity=LOG_CAP, eps=[0.0], teams=True))


STATES = {
    "none": lambda: None,
    "plain": _plain,
    "no log": lambda: SequentialEnsemble(_cfg(), LEARNERS, seed=SEED, eps=[0.0]),
    "team": lambda: SequentialEnsemble(_cfg(), 2, seed=SEED, log_capacity=LOG_CAP, eps=[0.0], envs_per_learner=2),
    "teams of one in curriculum mode": _team1_curriculum,
    "curriculum": _curriculum,
    "curriculum, last_level 2": lambda: _curriculum(last_level=2),
    "curriculum, level 1 without schedules": lambda: _curriculum(upto=1),
    "curriculum, everyone on level 2": lambda: _at_level(_curriculum(), 2),
    "curriculum, learners on different levels": _spread,
    "nstep 4": _nstep,
    "nstep 4, windows open": lambda: _ran(_nstep(), 3, want_open=True),
    "recipes": _recipes,
    "recipes, recipe 0 with last_level 2": lambda: _recipes(r0=_recipe(last_level=2)),
    "recipes, everyone on level 2": lambda: _at_level(_recipes(), 2),
    "recipes without rules": _recipes_bare,
    "recipes without schedules above level 0": lambda: _recipes_bare(rules=True),
    "recipes with n 4, windows open": lambda: _ran(_recipes(_recipe(nstep=4), _recipe(nstep=4, order=ORDER_PAPER)), 3, want_open=True),
    "recipes with n (4, 0), recipe 0's windows open": lambda: _ran(_recipes(_recipe(nstep=4), _recipe(order=ORDER_PAPER)), 3),
}


class _Args:
    """what the calls share: the library, the handle, valid tables and output arrays"""

    def __init__(self, ens):
        self.lib, self.ens = _lib.load(), ens
        self.x = None if ens is None else ens._h
        self.n = LEARNERS if ens is None else ens.n
        self.cfg = _cfg().to_c()
        self.alpha, self.eps, self.ratios, self.of = np.array([0.1]), np.array([0.0]), np.array(REFERENCE_RATIOS), RECIPE_OF.copy()
        self.i64, self.i32, self.dbl = C.c_int64(-7), C.c_int32(-7), C.c_double(-7.0)
        self.out = np.zeros(8 * 2835 * LEARNERS, dtype=np.float64)  # any output array fits in it


def snapshot(a):
    """what a refused call must leave as it was"""
    lib, x, n = a.lib, a.x, a.n
    v, j, u = C.c_int32(), C.c_int64(), C.c_int64()
    lens, of, level = (np.zeros(n, dtype=np.int32) for _ in range(3))
    pa, ea, ent = np.zeros((5, n), dtype=np.int32), np.zeros((5, n), dtype=np.int32), np.zeros((5, n), dtype=np.int64)
    _lib.check(lib.dql_ensemble_get_nstep(x, C.byref(v), _ptr(lens)))
    _lib.check(lib.dql_ensemble_get_recipes(x, _ptr(of)))
    rn = []
    for r in range(int(of.max()) + 1):
        w = C.c_int32()
        _lib.check(lib.dql_ensemble_get_recipe_nstep(x, r, C.byref(w)))
        rn.append(w.value)
    _lib.check(lib.dql_ensemble_get_levels(x, _ptr(level), _ptr(pa), _ptr(ea), _ptr(ent)))
    _lib.check(lib.dql_ensemble_get_period_index(x, C.byref(j)))
    _lib.check(lib.dql_ensemble_n_unfinished(x, C.byref(u)))
    return [v.value, lens.tolist(), of.tolist(), rn, level.tolist(), pa.tolist(), ea.tolist(), ent.tolist(), j.value, u.value, list(a.ens.launches())]


# ---- the calls: keyword arguments with valid defaults; a case overrides the ones it makes bad.  null=(...): those pointers are passed as null ----
def _tab(a, name, v, null):
    """(pointer, length) of a table argument: "ok" is the valid one, a list is that table"""
    if name in null:
        return None, 1
    arr = getattr(a, name) if isinstance(v, str) else np.array(v, dtype=np.float64)
    return arr, arr.size


def _create(a, cfg=None, n=LEARNERS, log_capacity=LOG_CAP, null=()):
    h = C.c_void_p()
    rcode = a.lib.dql_ensemble_create(None if "cfg" in null else C.byref(cfg or a.cfg), 0, n, SEED, log_capacity, None if "out" in null else C.byref(h))
    assert h.value is None
    return rcode


def _create_teams(a, cfg=None, n=2, E=2, log_capacity=LOG_CAP, null=()):
    h = C.c_void_p()
    rcode = a.lib.dql_ensemble_create_teams(None if "cfg" in null else C.byref(cfg or a.cfg), 0, n, E, SEED, log_capacity, None if "out" in null else C.byref(h))
    assert h.value is None
    return rcode


def _set_schedules(a, alpha="ok", eps="ok", n_alpha=None, n_eps=None, window=100, ms=97, me=50000, null=()):
    (al, na), (e, ne) = _tab(a, "alpha", alpha, null), _tab(a, "eps", eps, null)
    return a.lib.dql_ensemble_set_schedules(a.x, _ptr(al), na if n_alpha is None else n_alpha, _ptr(e), ne if n_eps is None else n_eps, window, ms, me)


def _set_level_schedules(a, level=0, eps="ok", n_eps=None, window=100, ms=97, me=50000, null=()):
    e, ne = _tab(a, "eps", eps, null)
    return a.lib.dql_ensemble_set_level_schedules(a.x, level, _ptr(e), ne if n_eps is None else n_eps, window, ms, me)


def _set_curriculum(a, last_level=4, every=8, ratios="ok", exhausted=1, null=()):
    r, _ = _tab(a, "ratios", ratios, null)
    return a.lib.dql_ensemble_set_curriculum(a.x, last_level, every, _ptr(r), exhausted)


def _set_recipes(a, n_recipes=2, of="ok", null=()):
    o = None if "of" in null else (a.of if isinstance(of, str) else np.array(of, dtype=np.int32))
    return a.lib.dql_ensemble_set_recipes(a.x, n_recipes, _ptr(o))


def _set_recipe(a, r=0, quirks=ec.Q_PAPER, alpha="ok", n_alpha=None, alpha_min=0.1, ratios="ok", last_level=4, exhausted=1, order=0, null=()):
    (al, na), (ra, _) = _tab(a, "alpha", alpha, null), _tab(a, "ratios", ratios, null)
    return a.lib.dql_ensemble_set_recipe(a.x, r, quirks, _ptr(al), na if n_alpha is None else n_alpha, alpha_min, _ptr(ra), last_level, exhausted, order)


def _set_recipe_level_schedules(a, r=0, level=0, eps="ok", n_eps=None, window=100, ms=97, me=50000, null=()):
    e, ne = _tab(a, "eps", eps, null)
    return a.lib.dql_ensemble_set_recipe_level_schedules(a.x, r, level, _ptr(e), ne if n_eps is None else n_eps, window, ms, me)


def _get_levels(a, null=()):
    return a.lib.dql_ensemble_get_levels(a.x, *(None if k in null else _ptr(a.out) for k in ("level", "promoted_at", "episodes_at", "entered_period")))


def _tables(a, which, first=0, count=1, counters=None, null=()):
    cnt = a.out if counters is None else np.array(counters, dtype=np.float64)
    fn = a.lib.dql_ensemble_get_tables if which == "get" else a.lib.dql_ensemble_set_tables
    return fn(a.x, first, count, None, None, _ptr(cnt))


def _get_counters(a, null=()):
    names = ("decisions", "episodes", "successes", "by_code", "promoted", "level_episodes", "frozen")
    return a.lib.dql_ensemble_get_counters(a.x, *(None if k in null else _ptr(a.out) for k in names))


def _get_episode_log(a, capacity=LOG_CAP, null=()):
    return a.lib.dql_ensemble_get_episode_log(a.x, *(None if k in null else _ptr(a.out) for k in ("code", "length")), capacity, None if "n" in null else _ptr(a.out))


def _get_state(a, null=()):
    return a.lib.dql_ensemble_get_state(a.x, *(None if k in null else _ptr(a.out) for k in ("reals", "ints")))


def _one_out(name, ctype):
    """a call (x, *ints, pointer to one number)"""
    def call(a, args=(), null=()):
        return getattr(a.lib, name)(a.x, *args, None if "out" in null else C.byref(getattr(a, ctype)))
    return call


def _launches(a, null=()):
    return a.lib.dql_diag_ensemble_launches(a.x, *(None if k in null else C.byref(C.c_int64()) for k in ("launches", "periods", "wave_periods")))


CALLS = {
    "dql_ensemble_create": _create,
    "dql_ensemble_create_teams": _create_teams,
    "dql_ensemble_n_learners": _one_out("dql_ensemble_n_learners", "i64"),
    "dql_ensemble_envs_per_learner": _one_out("dql_ensemble_envs_per_learner", "i32"),
    "dql_ensemble_set_schedules": _set_schedules,
    "dql_ensemble_rearm": lambda a: a.lib.dql_ensemble_rearm(a.x),
    "dql_ensemble_set_level": lambda a, k=0: a.lib.dql_ensemble_set_level(a.x, k),
    "dql_ensemble_n_live": _one_out("dql_ensemble_n_live", "i64"),
    "dql_ensemble_run": lambda a, periods=8: a.lib.dql_ensemble_run(a.x, periods),
    "dql_ensemble_set_curriculum": _set_curriculum,
    "dql_ensemble_set_level_schedules": _set_level_schedules,
    "dql_ensemble_get_levels": _get_levels,
    "dql_ensemble_n_unfinished": _one_out("dql_ensemble_n_unfinished", "i64"),
    "dql_ensemble_get_period_index": _one_out("dql_ensemble_get_period_index", "i64"),
    "dql_ensemble_transfer": lambda a, k=1: a.lib.dql_ensemble_transfer(a.x, k, 0.5),
    "dql_ensemble_get_tables": lambda a, **kw: _tables(a, "get", **kw),
    "dql_ensemble_set_tables": lambda a, **kw: _tables(a, "set", **kw),
    "dql_ensemble_get_counters": _get_counters,
    "dql_ensemble_get_episode_log": _get_episode_log,
    "dql_ensemble_get_state": _get_state,
    "dql_ensemble_index_faults": _one_out("dql_ensemble_index_faults", "i64"),
    "dql_diag_ensemble_launches": _launches,
    "dql_diag_ensemble_last": _one_out("dql_diag_ensemble_last", "dbl"),
    "dql_ensemble_set_recipes": _set_recipes,
    "dql_ensemble_set_recipe": _set_recipe,
    "dql_ensemble_set_recipe_level_schedules": _set_recipe_level_schedules,
    "dql_ensemble_get_recipes": lambda a, null=(): a.lib.dql_ensemble_get_recipes(a.x, None if "of" in null else _ptr(a.out)),
    "dql_ensemble_set_nstep": lambda a, n=2: a.lib.dql_ensemble_set_nstep(a.x, n),
    "dql_ensemble_get_nstep": lambda a, null=(): a.lib.dql_ensemble_get_nstep(a.x, None if "n" in null else C.byref(a.i32), None),
    "dql_ensemble_set_recipe_nstep": lambda a, r=0, n=2: a.lib.dql_ensemble_set_recipe_nstep(a.x, r, n),
    "dql_ensemble_get_recipe_nstep": lambda a, r=0, null=(): a.lib.dql_ensemble_get_recipe_nstep(a.x, r, None if "n" in null else C.byref(a.i32)),
}
ENTRY_POINTS = tuple(CALLS)

# ---- the cases: case name -> (state, keyword arguments).  " + " in a name: two bad arguments, the first check that fails speaks ----
P, NULL_X = "plain", ("none", {})
_TWO_AXES, _EIGHT, _LEVEL_9 = (lambda: _cfg(two_axis=1).to_c()), (lambda: _cfg(trajectory=1).to_c()), (lambda: dataclasses.replace(_cfg(), working_curriculum_step=9).to_c())
_RULE = {  # the promotion rule and the exploration table, shared by three calls
    "window 0": dict(window=0), "window 129": dict(window=129), "min_successes 0": dict(ms=0), "max_episodes 0": dict(me=0), "eps 1.5": dict(eps=[0.0, 1.5]),
    "eps -0.1": dict(eps=[-0.1]), "eps nan": dict(eps=[NAN]), "null eps": dict(null=("eps",)), "n_eps 0": dict(n_eps=0), "n_eps 2^22+1": dict(n_eps=(1 << 22) + 1),
    "window 0 + min_successes 0": dict(window=0, ms=0), "min_successes 0 + eps 1.5": dict(ms=0, eps=[1.5]), "n_eps 0 + window 0": dict(n_eps=0, window=0),
    "null eps + n_eps 0": dict(null=("eps",), n_eps=0),
}
_RATIOS = {"null ratios": dict(null=("ratios",)), "a ratio nan": dict(ratios=[1.0, NAN, 1.0, 1.0, 1.0]), "a ratio inf": dict(ratios=[1.0, 1.0, 1.0, 1.0, math.inf]),
           "advance_exhausted 2": dict(exhausted=2), "last_level 5": dict(last_level=5), "last_level -1": dict(last_level=-1),
           "null ratios + advance_exhausted 2": dict(null=("ratios",), exhausted=2), "advance_exhausted 2 + last_level 5": dict(exhausted=2, last_level=5)}
_CREATE = {"null config": dict(null=("cfg",)), "bad config": dict(cfg=_LEVEL_9), "null out": dict(null=("out",)), "two axes": dict(cfg=_TWO_AXES), "figure eight": dict(cfg=_EIGHT),
           "n_learners 0": dict(n=0), "log_capacity -1": dict(log_capacity=-1), "log_capacity 2^20+1": dict(log_capacity=(1 << 20) + 1),
           "bad config + null out": dict(cfg=_LEVEL_9, null=("out",)), "null out + two axes": dict(cfg=_TWO_AXES, null=("out",)), "two axes + n_learners 0": dict(cfg=_TWO_AXES, n=0),
           "n_learners 0 + log_capacity -1": dict(n=0, log_capacity=-1)}
_SLICE = {"first -1": dict(first=-1), "count 0": dict(count=0), "first beyond the end": dict(first=5), "slice beyond the end": dict(first=3, count=2)}


def _on(state, cases):
    return {what: (state, kw) for what, kw in cases.items()}


def _getter(state="plain"):
    return {"null ensemble": NULL_X, "null pointer": (state, dict(null=("out",)))}


CASES = {
    "dql_ensemble_create": _on("none", {**_CREATE, "n_learners 2^20+1": dict(n=(1 << 20) + 1)}),
    "dql_ensemble_create_teams": _on("none", {**_CREATE, "envs_per_learner 3": dict(E=3), "envs_per_learner 0": dict(E=0), "envs_per_learner 128": dict(E=128),
                                              "n_learners 2^19+1 of 2 envs": dict(n=(1 << 19) + 1), "figure eight + envs_per_learner 3": dict(cfg=_EIGHT, E=3),
                                              "envs_per_learner 3 + n_learners 0": dict(E=3, n=0)}),
    "dql_ensemble_n_learners": _getter(),
    "dql_ensemble_envs_per_learner": _getter(),
    "dql_ensemble_set_schedules": {
        "null ensemble": NULL_X,
        **_on(P, {**_RULE, "null alpha": dict(null=("alpha",)), "n_alpha 0": dict(n_alpha=0), "n_alpha 2^22+1": dict(n_alpha=(1 << 22) + 1), "alpha 1.5": dict(alpha=[0.1, 1.5]),
                  "alpha nan": dict(alpha=[NAN]), "null alpha + n_alpha 0": dict(null=("alpha",), n_alpha=0), "n_alpha 0 + window 129": dict(n_alpha=0, window=129),
                  "window 129 + alpha 1.5": dict(window=129, alpha=[1.5]), "max_episodes 0 + alpha 1.5": dict(me=0, alpha=[1.5]), "alpha 1.5 + eps 1.5": dict(alpha=[1.5], eps=[1.5])}),
    },
    "dql_ensemble_rearm": {"null ensemble": NULL_X},
    "dql_ensemble_set_level": {
        "null ensemble": NULL_X, "level -1": (P, dict(k=-1)), "level 5": (P, dict(k=5)),
        "above last_level": ("curriculum, last_level 2", dict(k=3)), "above the recipes' smallest last_level": ("recipes, recipe 0 with last_level 2", dict(k=3)),
        "level 5 with recipes": ("recipes, recipe 0 with last_level 2", dict(k=5)),
    },
    "dql_ensemble_n_live": _getter(),
    "dql_ensemble_run": {
        "null ensemble": NULL_X, "periods 0": (P, dict(periods=0)), "periods -1": (P, dict(periods=-1)), "periods 2^40+1": (P, dict(periods=(1 << 40) + 1)),
        "periods 0 in curriculum mode": ("curriculum, level 1 without schedules", dict(periods=0)),
        "a level schedule is missing": ("curriculum, level 1 without schedules", {}), "a recipe without a rule": ("recipes without rules", {}),
        "a recipe without a level schedule on a member's way up": ("recipes without schedules above level 0", {}),
    },
    "dql_ensemble_set_curriculum": {
        "null ensemble": NULL_X, "a team ensemble": ("team", {}), "a team ensemble + advance_every -1": ("team", dict(every=-1)), "a team ensemble, switching off": ("team", dict(every=0)),
        **_on(P, {**_RATIOS, "advance_every -1": dict(every=-1), "advance_every 4097": dict(every=4097), "advance_every 4097 + null ratios": dict(every=4097, null=("ratios",))}),
        "with n-step targets": ("nstep 4", {}), "with n-step targets + null ratios": ("nstep 4", dict(null=("ratios",))), "advance_every -1 with n-step targets": ("nstep 4", dict(every=-1)),
        "off while recipes are installed": ("recipes", dict(every=0)), "off while learners stand on different levels": ("curriculum, learners on different levels", dict(every=0)),
        "last_level below a learner's level": ("curriculum, everyone on level 2", dict(last_level=1)),
        "advance_exhausted 2 + last_level below a learner's level": ("curriculum, everyone on level 2", dict(last_level=1, exhausted=2)),
    },
    "dql_ensemble_set_level_schedules": {"null ensemble": NULL_X, **_on(P, {**_RULE, "level -1": dict(level=-1), "level 5": dict(level=5), "level 5 + window 0": dict(level=5, window=0),
                                                                            "level 5 + null eps": dict(level=5, null=("eps",))})},
    "dql_ensemble_get_levels": {"null ensemble": NULL_X, **_on(P, {f"null {k}": dict(null=(k,)) for k in ("level", "promoted_at", "episodes_at", "entered_period")})},
    "dql_ensemble_n_unfinished": {**_getter(), "null pointer in curriculum mode": ("curriculum", dict(null=("out",)))},
    "dql_ensemble_get_period_index": _getter(),
    "dql_ensemble_transfer": {"null ensemble": NULL_X, "level -1": (P, dict(k=-1)), "level 5": (P, dict(k=5))},
    "dql_ensemble_get_tables": {"null ensemble": NULL_X, **_on(P, _SLICE)},
    "dql_ensemble_set_tables": {"null ensemble": NULL_X, **_on(P, {**_SLICE, "a counter of -1": dict(counters=[-1.0] * 2835), "a counter of 2^53": dict(counters=[0.0] * 2834 + [2.0 ** 53]),
                                                                   "a counter nan": dict(counters=[NAN] * 2835), "first -1 + a counter of -1": dict(first=-1, counters=[-1.0] * 2835)})},
    "dql_ensemble_get_counters": {"null ensemble": NULL_X, **_on(P, {f"null {k}": dict(null=(k,)) for k in ("decisions", "episodes", "successes", "by_code", "promoted", "level_episodes", "frozen")})},
    "dql_ensemble_get_episode_log": {
        "null ensemble": NULL_X, **_on(P, {"null code": dict(null=("code",)), "null length": dict(null=("length",)), "null n_episodes": dict(null=("n",)), "capacity 3": dict(capacity=3),
                                           "capacity 1": dict(capacity=1), "capacity 0": dict(capacity=0), "null code + capacity 3": dict(null=("code",), capacity=3)}),
        "an ensemble without a log": ("no log", dict(capacity=0)), "an ensemble without a log, capacity 1": ("no log", dict(capacity=1)),
    },
    "dql_ensemble_get_state": {"null ensemble": NULL_X, "null reals": (P, dict(null=("reals",))), "null ints": (P, dict(null=("ints",)))},
    "dql_ensemble_index_faults": _getter(),
    "dql_diag_ensemble_launches": {"null ensemble": NULL_X, **_on(P, {f"null {k}": dict(null=(k,)) for k in ("launches", "periods", "wave_periods")})},
    "dql_diag_ensemble_last": {**_getter(), "before any run": (P, {}), "before any run in curriculum mode": ("curriculum", {})},
    "dql_ensemble_set_recipes": {
        "null ensemble": NULL_X, "a team ensemble": ("team", {}), "a team ensemble + n_recipes 65": ("team", dict(n_recipes=65)), "a team ensemble, uninstalling": ("team", dict(n_recipes=0)),
        "with n-step targets + without curriculum mode": ("nstep 4", {}), "n_recipes 65 with n-step targets": ("nstep 4", dict(n_recipes=65)),
        "without curriculum mode": (P, {}), "without curriculum mode + null recipe_of": (P, dict(null=("of",))), "n_recipes -1": (P, dict(n_recipes=-1)),
        **_on("curriculum", {"n_recipes -1": dict(n_recipes=-1), "n_recipes 65": dict(n_recipes=65), "null recipe_of": dict(null=("of",)), "a recipe_of of -1": dict(of=[0, 1, -1, 1]),
                             "a recipe_of of n_recipes": dict(of=[0, 1, 0, 2]), "n_recipes 65 + null recipe_of": dict(n_recipes=65, null=("of",))}),
        "installing while a window holds entries": ("recipes with n 4, windows open", {}), "uninstalling while a window holds entries": ("recipes with n 4, windows open", dict(n_recipes=0)),
        "a recipe_of of -1 while a window holds entries": ("recipes with n 4, windows open", dict(of=[0, 1, -1, 1])),
        "uninstalling while recipe 0's windows hold entries": ("recipes with n (4, 0), recipe 0's windows open", dict(n_recipes=0)),
    },
    "dql_ensemble_set_recipe": {
        "null ensemble": NULL_X, "no recipes are installed": ("curriculum", {}), "no recipes are installed + null alpha": ("curriculum", dict(null=("alpha",))),
        **_on("recipes", {**_RATIOS, "recipe -1": dict(r=-1), "recipe 2": dict(r=2), "recipe 2 + null alpha": dict(r=2, null=("alpha",)), "null alpha": dict(null=("alpha",)),
                          "quirks 0xffffffff + null alpha": dict(quirks=0xFFFFFFFF, null=("alpha",)), "n_alpha 0": dict(n_alpha=0), "n_alpha 2^22+1": dict(n_alpha=(1 << 22) + 1),
                          "alpha 1.5": dict(alpha=[1.5]), "alpha nan": dict(alpha=[NAN]), "alpha_min 1.5": dict(alpha_min=1.5), "alpha_min nan": dict(alpha_min=NAN),
                          "transfer_order 2": dict(order=2), "transfer_order -1": dict(order=-1), "null alpha + n_alpha 0": dict(null=("alpha",), n_alpha=0),
                          "n_alpha 0 + alpha_min 1.5": dict(n_alpha=0, alpha_min=1.5), "alpha 1.5 + alpha_min 1.5": dict(alpha=[1.5], alpha_min=1.5),
                          "alpha_min 1.5 + null ratios": dict(alpha_min=1.5, null=("ratios",)), "advance_exhausted 2 + transfer_order 2": dict(exhausted=2, order=2),
                          "transfer_order 2 + last_level 5": dict(order=2, last_level=5)}),
        "last_level below a member's level": ("recipes, everyone on level 2", dict(last_level=1)),
        "transfer_order 2 + last_level below a member's level": ("recipes, everyone on level 2", dict(last_level=1, order=2)),
    },
    "dql_ensemble_set_recipe_level_schedules": {
        "null ensemble": NULL_X, "no recipes are installed": ("curriculum", {}), "no recipes are installed + level 5": ("curriculum", dict(level=5)),
        **_on("recipes", {**_RULE, "recipe -1": dict(r=-1), "recipe 2": dict(r=2), "recipe 2 + level 5": dict(r=2, level=5), "level -1": dict(level=-1), "level 5": dict(level=5),
                          "level 5 + window 0": dict(level=5, window=0), "level 5 + null eps": dict(level=5, null=("eps",))}),
    },
    "dql_ensemble_get_recipes": {"null ensemble": NULL_X, "null recipe_of": (P, dict(null=("of",))), "null recipe_of with recipes": ("recipes", dict(null=("of",)))},
    "dql_ensemble_set_nstep": {
        "null ensemble": NULL_X, "n -1": (P, dict(n=-1)), "n 17": (P, dict(n=17)), "a team ensemble": ("team", {}), "n 17 + a team ensemble": ("team", dict(n=17)),
        "in curriculum mode": ("curriculum", {}), "with recipes installed": ("recipes", {}), "a team ensemble + in curriculum mode": ("teams of one in curriculum mode", {}),
        "n 17 + in curriculum mode": ("curriculum", dict(n=17)), "another n while a window holds entries": ("nstep 4, windows open", dict(n=2)),
        "n 0 while a window holds entries": ("nstep 4, windows open", dict(n=0)), "n 17 while a window holds entries": ("nstep 4, windows open", dict(n=17)),
    },
    "dql_ensemble_get_nstep": {"null ensemble": NULL_X, "null n": (P, dict(null=("n",)))},
    "dql_ensemble_set_recipe_nstep": {
        "null ensemble": NULL_X, "no recipes are installed": ("curriculum", {}), "no recipes are installed + n 17": ("curriculum", dict(n=17)),
        **_on("recipes", {"recipe -1": dict(r=-1), "recipe 2": dict(r=2), "n -1": dict(n=-1), "n 17": dict(n=17), "recipe 2 + n 17": dict(r=2, n=17)}),
        "another n while a member's window holds entries": ("recipes with n 4, windows open", dict(r=1, n=2)),
        "n 0 while a member's window holds entries": ("recipes with n 4, windows open", dict(n=0)),
        "n 17 while a member's window holds entries": ("recipes with n 4, windows open", dict(n=17)),
        "recipe 0 while its members' windows hold entries and recipe 1's do not": ("recipes with n (4, 0), recipe 0's windows open", dict(r=0, n=2)),
    },
    "dql_ensemble_get_recipe_nstep": {
        "null ensemble": NULL_X, "no recipes are installed": (P, {}), "no recipes are installed + null n": (P, dict(null=("n",))),
        **_on("recipes", {"recipe -1": dict(r=-1), "recipe 2": dict(r=2), "null n": dict(null=("n",)), "recipe 2 + null n": dict(r=2, null=("n",))}),
    },
}


def rows_of(entry, states=None):
    """{case name: [return code, dql_last_error text]} of one entry point.  states: a dict that keeps the ensembles between entry points (the refused calls
    leave them as they were, which every row asserts); the caller closes them."""
    own = states is None
    states = {} if own else states
    lib, rows = _lib.load(), {}
    try:
        for what, (state, kw) in CASES[entry].items():
            if state not in states:
                states[state] = STATES[state]()
            a = _Args(states[state])
            kw = {k: (v() if callable(v) else v) for k, v in kw.items()}
            before = None if a.x is None else snapshot(a)
            rcode = CALLS[entry](a, **kw)
            rows[what] = [int(rcode), lib.dql_last_error().decode()]
            assert rcode != 0, f"{entry}, {what}: the call was accepted"
            assert a.x is None or snapshot(a) == before, f"{entry}, {what}: the refused call moved something"
            assert (a.i64.value, a.i32.value, a.dbl.value) == (-7, -7, -7.0) and not a.out.any(), f"{entry}, {what}: an output was written"
        return rows
    finally:
        if own:
            close_all(states)


def close_all(states):
    for ens in states.values():
        if ens is not None:
            ens.close()
    states.clear()


# ---- RUNS ----
RUN_LEARNERS, TEAM_LEARNERS, TEAM_ENVS, ADVANCE_EVERY = 70, 18, 4, 8
MODES = ("plain", "team", "nstep", "curriculum", "recipes", "recipes nstep")
SCRIPTS = tuple((m, d) for m in MODES for d in ((F32, F64) if m in ("plain", "recipes nstep") else (F32,)))
SCRIPT_IDS = tuple(f"{m}-{'f32' if d == F32 else 'f64'}" for m, d in SCRIPTS)
WORKLIST_MODES = ("curriculum", "recipes", "recipes nstep")
# the worklist modes: 5 ends before the first advance point, 20 crosses three (8, 16, 24), 7 ends on one and 8 starts on it; the same again once learners
# have spread over the levels (from period 512 on), then a long stretch
WORKLIST_CALLS = (5, 20, 7, 8, 472, 5, 20, 7, 8, 1, 1000)
PLAIN_CALLS = (5, 20, 4097, 1, 1000)
FINISH_CALLS = (1000, 1000, 1000, 1000)  # every learner finishes in one of these calls; the later ones find nothing to fly
FROZEN_CALLS = (1000, 1000, 1000, 4097, 1)  # the plain loop: a call's first launch is made whatever is frozen, the second of the 4097 is not


def _digest(ens):
    h = hashlib.sha256()
    lv, c, st = ens.levels(), ens.counters(), ens.state()
    for a in (*ens.get_tables(), *(c[k] for k in sorted(c)), *(lv[k] for k in sorted(lv)), *(st[k] for k in sorted(st)), ens.pending_lengths()):
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _run_recipes(nsteps, max_episodes, last_level):
    lv = lambda k: LevelSchedule(eps=[0.0], window=1 if k == 0 else 2, min_successes=1 if k == 0 else 2, max_episodes=max_episodes)
    return [Recipe(quirks=q, last_level=last_level, transfer_order=o, nstep=n, levels=tuple(lv(k) for k in range(5)))
            for q, o, n in ((ec.Q_PAPER, 0, nsteps[0]), (ec.Q_REFERENCE, ORDER_PAPER, nsteps[1]))]


def script_ensemble(mode, dtype, finishing):
    """the ensemble of a script, from trained tables, greedy.  finishing: one episode per level (the plain-loop modes: one episode) and last_level 1, so that
    every learner is finished for good within a few hundred periods; else three episodes per level in the worklist modes, and a rule nobody meets (window 128,
    128 successes, no budget to speak of) in the plain-loop ones"""
    team = mode == "team"
    n = TEAM_LEARNERS if team else RUN_LEARNERS
    rule = dict(window=1, min_successes=1, max_episodes=1) if finishing else dict(window=128, min_successes=128, max_episodes=1 << 20)
    ens = SequentialEnsemble(_cfg(dtype), n, seed=11, eps=[0.0], envs_per_learner=TEAM_ENVS if team else 1, nstep=4 if mode == "nstep" else 0, **rule)
    ens.set_tables(*ec.trained_tables(n))
    if mode in WORKLIST_MODES:
        budget, last = (1, 1) if finishing else (3, 4)
        for k in range(5):
            ens.set_level_schedules(k, [0.0], 1 if k == 0 else 2, 1 if k == 0 else 2, budget)
        ens.set_curriculum(last, ADVANCE_EVERY)
        if mode != "curriculum":
            ens.set_recipes(_run_recipes((0, 4) if mode == "recipes nstep" else (0, 0), budget, last), np.arange(n) % 2)
    return ens


def _fly(ens, calls):
    out = []
    for k in calls:
        ens.run(k)
        out.append({"run": k, "launches": list(ens.launches()), "period_index": ens.period_index(), "n_live": ens.n_live(), "n_unfinished": ens.n_unfinished(),
                    "learners_per_level": np.bincount(ens.levels()["level"], minlength=5).tolist(), "sha256": _digest(ens)})
    assert ens.index_faults() == 0
    return out


def script_of(mode, dtype):
    """{"main": [...], "finishing": [...]}: per dql_ensemble_run call what the library shows after it"""
    out = {}
    for part, calls in (("main", WORKLIST_CALLS if mode in WORKLIST_MODES else PLAIN_CALLS), ("finishing", FINISH_CALLS if mode in WORKLIST_MODES else FROZEN_CALLS)):
        ens = script_ensemble(mode, dtype, part == "finishing")
        try:
            out[part] = _fly(ens, calls)
        finally:
            ens.close()
    return out


def assert_script_is_what_it_is_for(mode, rec):
    """on a recorded script: the cases the table promises are in it"""
    main, fin = rec["main"], rec["finishing"]
    if mode in WORKLIST_MODES:
        assert main[0]["launches"][:2] == [1, 5] and main[1]["launches"][:2] == [5, 25], "5 periods in one launch, then 20 cut at 8, 16 and 24"
        assert main[3]["launches"][0] == main[2]["launches"][0] + 1 and main[2]["period_index"] == 32, "the call that starts on an advance point is one launch"
        spread = [sum(1 for v in r["learners_per_level"] if v) for r in main[4:9]]
        assert min(spread) >= 2 and main[4]["n_live"] > 0, f"from period 512 on the learners should stand on several levels (populated levels: {spread})"
        done = [i for i, r in enumerate(fin) if r["n_unfinished"] == 0]
        assert done and done[0] + 1 < len(fin), "every learner finishes within the script, with a call to spare"
        i = done[0]
        flown = fin[i]["launches"][1] - (fin[i - 1]["launches"][1] if i else 0)
        assert 0 < flown < 1000 and fin[i]["period_index"] == 1000 * (i + 1), "the call in which the last learner finishes ends early; the period index advances by the whole call"
        assert fin[i + 1]["launches"] == fin[i]["launches"] and fin[i + 1]["period_index"] == 1000 * (i + 2), "nothing is launched once everyone is finished"
    else:
        assert main[2]["launches"][0] == main[1]["launches"][0] + 2 and main[2]["launches"][1] == main[1]["launches"][1] + 4097, "4097 periods: launches of 4096 and 1"
        assert main[-1]["n_live"] > 0
        assert fin[2]["n_live"] == 0, "everyone is frozen after 3 000 periods"
        assert fin[3]["launches"][:2] == [fin[2]["launches"][0] + 1, fin[2]["launches"][1] + 4096] and fin[3]["period_index"] == 3000 + 4097, "all frozen: the 4097's second launch is not made"
        assert fin[4]["launches"][0] == fin[3]["launches"][0] + 1, "a call's first launch is made whatever is frozen"
