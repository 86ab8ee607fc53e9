"""`SequentialEnsemble`: L independent copies of the reference's OWN training loop — one env, one agent, update after every step
(pkg/trainer.py:187-236) — flown by one kernel launch, one learner per GPU lane (include/dql.h dql_ensemble_*).

Where `Engine` trains one set of tables on N envs with the batched mean-target fold, every learner here keeps its own `Q_table_a`, `Q_table_b` and
`state_action_counter` and applies `DoubleQLearningAgent.update` right after each of its agent periods.  A learner freezes when the reference's
promotion rule fires for it (successes among its last `window` episodes at the level reach `min_successes`) or when its episode budget is spent;
`train_level` / `curriculum` are `Trainer.curriculum_training` for the whole ensemble: run until all learners are frozen, transfer, next level.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field, replace
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .config import CHECK_NAMES, DqlConfig, N_CELLS

MAX_PERIODS_PER_LAUNCH = 4096  # include/dql.h DQL_ENSEMBLE_MAX_PERIODS
MAX_WINDOW = 128               # DQL_ENSEMBLE_MAX_WINDOW
MAX_LEARNERS = 1 << 20         # DQL_ENSEMBLE_MAX_LEARNERS
MAX_LEVELS = 5
MAX_ADVANCE_EVERY = 4096       # csrc/dql_advance.hpp ADV_MAX_EVERY
MAX_RECIPES = 64               # include/dql.h DQL_ENSEMBLE_MAX_RECIPES
NSTEP_MAX = 16                 # include/dql.h DQL_NSTEP_MAX
NSTEP_PLAIN_ONLY = "n-step targets (nstep >= 1) are for the plain mode, where every learner flies the config's level: no teams, no per-learner curriculum, no recipes"
TEAM_NSTEP_TEAMS_ONLY = "team_nstep is for an ensemble made through the team kernel (envs_per_learner > 1 or teams=True); a plain ensemble takes nstep"
TEAM_NSTEP_BARRIER_ONLY = "team n-step targets (team_nstep >= 1) are for the barrier mode, where every learner flies the config's level: no per-learner curriculum, no recipes"
TEAM_CURRICULUM_TEAMS_ONLY = "team curriculum mode is for an ensemble made through the team kernel (envs_per_learner > 1 or teams=True); a plain ensemble takes set_curriculum"
TEAM_CURRICULUM_ONE_MODE = "team curriculum mode and per-learner curriculum mode (set_curriculum, recipes) refuse each other: a team ensemble of one env per learner flies one of them at a time"
TEAM_SIZES = (1, 2, 4, 8, 16, 32, 64)  # envs per learner (include/dql.h dql_ensemble_create_teams): a team is consecutive lanes of one wave
TEAMS_BARRIER_ONLY = "an ensemble with more than one env per learner flies the barrier mode only (train_level / curriculum): teams have no per-learner curriculum and no recipes"
ORDER_REFERENCE, ORDER_PAPER = 0, 1  # Recipe.transfer_order
REFERENCE_RATIOS = (1.0, 0.8172650252856599, 0.8211253690681617, 0.8257273369742982, 0.8311571820651724)  # Trainer.transfer_learning_ratio(k), k = 0 .. 4
N_CODES = len(CHECK_NAMES)
GOAL = CHECK_NAMES.index("TERMINAL_SUCCESS")
STATE_REAL_FIELDS = ("cum_x", "reward", "px", "py", "pz", "vx", "vy", "vz", "mp_x", "mp_u", "qw", "qx", "qy", "qz", "pitch_sp")
STATE_INT_FIELDS = ("idx_x", "step_count", "code", "flags", "action")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def eps_threshold(eps: float) -> int:
    """csrc/dql_host_consts.hpp eps_threshold: the number of k in [0, 2^24) with k 2^-24 < eps; explore <=> (r >> 8) < threshold"""
    if not eps > 0.0:
        return 0
    return min(int(math.ceil(eps * 16777216.0)), 16777216)


def exploration_rates(level: int, n: int = 2001) -> np.ndarray:
    """`Trainer.exploration_rate(e, level)` for the episode index e = 0 .. n - 1 within the level (pkg/trainer.py:112-126); a learner past the table's end
    keeps its last entry (2 001 entries reach the 0.01 floor of level 0).  Levels above 0 do not explore: one zero."""
    from .trainer import Trainer
    if level > 0:
        return np.zeros(1)
    me = SimpleNamespace()
    return np.array([Trainer.exploration_rate(me, e, level) for e in range(int(n))], dtype=np.float64)


def eps_threshold_table(level: int, n: int = 2001) -> np.ndarray:
    """the thresholds the kernel compares the action word with, per episode index within the level"""
    return np.array([eps_threshold(float(e)) for e in exploration_rates(level, n)], dtype=np.uint32)


def min_successes_for(window: int = 100, success_rate: float = 0.96) -> int:
    """The reference promotes when `sum(deque) / window > success_rate`, with the divisor `window` also while the deque fills (pkg/trainer.py:219-236):
    the smallest success count that does it — 97 for (100, 0.96)."""
    if window < 1 or not 0.0 <= success_rate < 1.0:
        raise ValueError("window must be positive and success_rate in [0, 1)")
    k = 0
    while not k / window > success_rate:
        k += 1
    return k


def _checked_rule(eps, level: int, window, min_successes, max_episodes, bad_eps: str, ranged: bool = False):
    """-> (eps float64[], window, min_successes, max_episodes) as the library takes them.  eps None: `exploration_rates(level)`; min_successes None: the
    reference's 0.96 of the window.  ValueError on what the library refuses; `bad_eps` is the caller's sentence for an empty (`ranged`: or out-of-range) table."""
    e = exploration_rates(level) if eps is None else np.ascontiguousarray(eps, dtype=np.float64).ravel()
    window = int(window)
    if not 1 <= window <= MAX_WINDOW:
        raise ValueError(f"window must be in 1..{MAX_WINDOW}")
    ms = min_successes_for(window) if min_successes is None else int(min_successes)
    if ms < 1 or int(max_episodes) < 1:
        raise ValueError("min_successes and max_episodes must be positive")
    if e.size < 1 or (ranged and not ((e >= 0.0) & (e <= 1.0)).all()):
        raise ValueError(bad_eps)
    return e, window, ms, int(max_episodes)


@dataclass
class LevelSchedule:
    """what one level of a recipe flies with (`SequentialEnsemble.set_level_schedules`' arguments); eps None: `exploration_rates(level)`; min_successes None:
    the reference's 0.96 of the window"""
    eps: Optional[Sequence[float]] = None
    window: int = 100
    min_successes: Optional[int] = None
    max_episodes: int = 50000


@dataclass
class Recipe:
    """What the learners of one recipe share (include/dql.h).  The defaults are the reference's recipe: its quirks, the config's
    learning rates, its exploration and promotion rule per level, its ratios, `Q[k] = Q[k-1] ratio` after level k with the k = 0 wrap (transfer_order 0).
    transfer_order 1 is the paper's: `Q[k+1] = Q[k] ratios[k+1]` on entering level k + 1, the level-k block kept, no wrap.
    nstep: the recipe's learners update with the uncorrected n-step Double-Q return of their pending windows (`SequentialEnsemble.set_nstep`'s update, DESIGN.md
    section 23); 0, the default, is the one-step update."""
    quirks: int = 0x7F
    alpha_table: Optional[Sequence[float]] = None   # None: the ensemble config's
    alpha_min: Optional[float] = None               # None: the ensemble config's
    ratios: Sequence[float] = REFERENCE_RATIOS
    last_level: int = 4
    advance_exhausted: bool = True
    transfer_order: int = ORDER_REFERENCE
    levels: Sequence[LevelSchedule] = field(default_factory=lambda: tuple(LevelSchedule() for _ in range(MAX_LEVELS)))
    nstep: int = 0                                  # 0: the one-step update; 1..NSTEP_MAX: the n-step return as this recipe's target

    def checked(self, cfg: DqlConfig):
        """-> (alpha float64[], alpha_min, ratios float64[5], per level (eps float64[], window, min_successes, max_episodes)); ValueError on what the library refuses"""
        if not 0 <= int(self.nstep) <= NSTEP_MAX:
            raise ValueError(f"a recipe's nstep must be in 0..{NSTEP_MAX} (0: the one-step update)")
        alpha = cfg.alpha_table() if self.alpha_table is None else np.ascontiguousarray(self.alpha_table, dtype=np.float64).ravel()
        alpha_min = float(cfg.alpha_min if self.alpha_min is None else self.alpha_min)
        if alpha.size < 1 or not ((alpha >= 0.0) & (alpha <= 1.0)).all() or not 0.0 <= alpha_min <= 1.0:
            raise ValueError("the learning-rate table must not be empty and every learning rate (alpha_min included) must be in [0, 1]")
        if not 0 <= int(self.quirks) < (1 << 32):
            raise ValueError("quirks must be a 32-bit word")
        r = np.ascontiguousarray(self.ratios, dtype=np.float64).ravel()
        if r.size != MAX_LEVELS or not np.isfinite(r).all():
            raise ValueError("ratios must be five finite numbers")
        if not 0 <= int(self.last_level) < MAX_LEVELS:
            raise ValueError("last_level must be in 0..4")
        if self.transfer_order not in (ORDER_REFERENCE, ORDER_PAPER):
            raise ValueError("transfer_order must be 0 (the reference's) or 1 (the paper's)")
        if len(self.levels) != MAX_LEVELS:
            raise ValueError("a recipe has five level schedules")
        lv = [_checked_rule(s.eps, k, s.window, s.min_successes, s.max_episodes, "the eps table must not be empty and exploration rates must be in [0, 1]", ranged=True)
              for k, s in enumerate(self.levels)]
        return alpha, alpha_min, r, lv


class SequentialEnsemble:
    def __init__(self, cfg: DqlConfig, n_learners: int, seed: int = 42, device: int = 0, log_capacity: int = 0, alpha_table=None, eps=None, window: int = 100,
                 min_successes: Optional[int] = None, max_episodes: int = 50000, envs_per_learner: int = 1, teams: Optional[bool] = None, nstep: int = 0,
                 team_nstep: int = 0):
        """nstep: 0 for the reference's one-step update, 1..NSTEP_MAX for the n-step return as the target (`set_nstep`).
        team_nstep: the same for a team ensemble, one pending window per env (`set_team_nstep`).
        envs_per_learner: E envs per learner (`TEAM_SIZES`), whose transitions the learner takes in env order every period; learner l
        owns envs l E .. l E + E - 1 and `state()` returns [L E] arrays.  teams: create through dql_ensemble_create_teams (the team kernel) — default: when E > 1;
        True with E = 1 flies the team kernel with teams of one, which equals the plain ensemble bit for bit."""
        n_learners, log_capacity, envs_per_learner = int(n_learners), int(log_capacity), int(envs_per_learner)
        if envs_per_learner not in TEAM_SIZES:
            raise ValueError(f"envs_per_learner must be one of {TEAM_SIZES}")
        teams = envs_per_learner > 1 if teams is None else bool(teams)
        if envs_per_learner > 1 and not teams:
            raise ValueError("more than one env per learner needs the team kernel (teams=False was asked for)")
        if cfg.two_axis:
            raise ValueError("two-axis configs are refused: the reference's learner is x-only")
        if cfg.trajectory != 0:
            raise ValueError("the figure-eight trajectory is refused: the reference's learner is x-only")
        if not 1 <= n_learners <= MAX_LEARNERS // envs_per_learner:
            raise ValueError(f"n_learners must be positive and n_learners * envs_per_learner at most {MAX_LEARNERS}")
        if log_capacity < 0:
            raise ValueError("log_capacity must not be negative")
        self._check_nstep(int(nstep), teams)
        self._check_team_nstep(int(team_nstep), teams)
        self.lib = _lib.load()
        self.cfg = cfg
        self.n = n_learners
        self.envs_per_learner, self.n_envs, self.teams = envs_per_learner, n_learners * envs_per_learner, teams
        self.log_capacity = log_capacity
        self._c = cfg.to_c()
        h = C.c_void_p()
        if teams:
            _lib.check(self.lib.dql_ensemble_create_teams(C.byref(self._c), int(device), self.n, envs_per_learner, int(seed), log_capacity, C.byref(h)))
        else:
            _lib.check(self.lib.dql_ensemble_create(C.byref(self._c), int(device), self.n, int(seed), log_capacity, C.byref(h)))
        self._h = h
        self._nstep, self._advance_every, self._team_nstep, self._team_every = 0, 0, 0, 0
        self.set_schedules(alpha_table, eps, window, min_successes, max_episodes)
        if int(nstep):
            self.set_nstep(nstep)
        if int(team_nstep):
            self.set_team_nstep(team_nstep)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.dql_ensemble_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- schedules and level ----
    def set_schedules(self, alpha_table=None, eps=None, window: int = 100, min_successes: Optional[int] = None, max_episodes: int = 50000):
        """alpha_table: alpha(count), default the config's; eps: exploration rate per episode index within the level, default the reference's for the
        config's level; window / min_successes: the promotion rule (default: the reference's 0.96 of the window); max_episodes: budget per level"""
        alpha = self.cfg.alpha_table() if alpha_table is None else np.ascontiguousarray(alpha_table, dtype=np.float64).ravel()
        e, window, ms, max_episodes = _checked_rule(eps, self.cfg.working_curriculum_step, window, min_successes, max_episodes, "the alpha and eps tables must not be empty")
        if alpha.size < 1:
            raise ValueError("the alpha and eps tables must not be empty")
        _lib.check(self.lib.dql_ensemble_set_schedules(self._h, _p(alpha), alpha.size, _p(e), e.size, window, ms, max_episodes))
        self.window, self.min_successes, self.max_episodes = window, ms, max_episodes

    def set_level(self, level: int):
        """new working level: every env re-enters through reset, per-level episode counts and windows are cleared, all learners re-armed"""
        _lib.check(self.lib.dql_ensemble_set_level(self._h, int(level)))
        self.cfg.working_curriculum_step = int(level)

    def rearm(self):
        _lib.check(self.lib.dql_ensemble_rearm(self._h))

    # ---- n-step targets (include/dql.h) ----
    @staticmethod
    def _check_nstep(n: int, teams: bool, curriculum: bool = False):
        if not 0 <= n <= NSTEP_MAX:
            raise ValueError(f"nstep must be in 0..{NSTEP_MAX} (0: the one-step update)")
        if n >= 1 and (teams or curriculum):
            raise ValueError(NSTEP_PLAIN_ONLY)

    def set_nstep(self, n: int):
        """n = 0: `run` flies the one-step kernel, as after creation.  1 <= n <= NSTEP_MAX: every learner updates with the uncorrected n-step Double-Q return of
        its pending window (include/dql.h); n = 1 equals n = 0 bit for bit.  Refused on a team ensemble, in per-learner curriculum or recipe mode, and
        (by the library) while a learner's window holds entries: change n after creation, after `set_level`, or when every learner is frozen."""
        n = int(n)
        self._check_nstep(n, getattr(self, "teams", False) or getattr(self, "envs_per_learner", 1) > 1, bool(getattr(self, "_advance_every", 0)) or bool(getattr(self, "_recipes", [])))
        _lib.check(self.lib.dql_ensemble_set_nstep(self._h, n))
        self._nstep = n

    @property
    def nstep(self) -> int:
        v = C.c_int32()
        _lib.check(self.lib.dql_ensemble_get_nstep(self._h, C.byref(v), None))
        return int(v.value)

    def pending_lengths(self) -> np.ndarray:
        """int32 [L]: the entries in each learner's pending window (0 with nstep = 0, for a frozen learner, and right after `set_level`)"""
        v, out = C.c_int32(), np.zeros(self.n, dtype=np.int32)
        _lib.check(self.lib.dql_ensemble_get_nstep(self._h, C.byref(v), _p(out)))
        return out

    # ---- n-step targets for team ensembles: one pending window per env (include/dql.h) ----
    @staticmethod
    def _check_team_nstep(n: int, teams: bool, curriculum: bool = False):
        if not 0 <= n <= NSTEP_MAX:
            raise ValueError(f"team_nstep must be in 0..{NSTEP_MAX} (0: the one-step team update)")
        if not teams and n >= 1:
            raise ValueError(TEAM_NSTEP_TEAMS_ONLY)
        if n >= 1 and curriculum:
            raise ValueError(TEAM_NSTEP_BARRIER_ONLY)

    def set_team_nstep(self, n: int):
        """n = 0: `run` flies the one-step team kernel, as after creation.  1 <= n <= NSTEP_MAX: every ENV keeps a pending window of its own and the learner
        updates with the uncorrected n-step Double-Q return, the E records of a period still in env order (include/dql.h); n = 1 equals n = 0 bit for bit, E = 1
        equals a plain ensemble's `set_nstep(n)`.  A frozen team's windows are generally NOT empty: the library refuses a change of n while any env's window
        holds entries, so change it after creation or after `set_level` (n = 0 and n = 1 leave every window empty after every period, so a change from them
        is accepted at any time).  Refused in per-learner curriculum mode and with recipes installed, which a team ensemble of one env per learner can enter."""
        n = int(n)
        teams = bool(getattr(self, "teams", False))
        if not teams:
            raise ValueError(TEAM_NSTEP_TEAMS_ONLY)
        self._check_team_nstep(n, teams, bool(self.__dict__.get("_advance_every", 0)) or bool(self.__dict__.get("_recipes", [])))
        _lib.check(self.lib.dql_ensemble_set_team_nstep(self._h, n))
        self._team_nstep = n

    @property
    def team_nstep(self) -> int:
        v = C.c_int32()
        _lib.check(self.lib.dql_ensemble_get_team_nstep(self._h, C.byref(v), None))
        return int(v.value)

    def team_pending_lengths(self) -> np.ndarray:
        """int32 [L E]: the entries in each env's pending window, in env order (0 with team_nstep = 0 and right after `set_level`; a frozen team's stay open)"""
        v, out = C.c_int32(), np.zeros(self.n_envs, dtype=np.int32)
        _lib.check(self.lib.dql_ensemble_get_team_nstep(self._h, C.byref(v), _p(out)))
        return out

    # ---- per-learner curriculum levels (include/dql.h) ----
    def set_curriculum(self, last_level: int = 4, advance_every: int = MAX_ADVANCE_EVERY, ratios=None, advance_exhausted: bool = True):
        """Curriculum mode: at every period index that is a multiple of `advance_every`, a frozen learner below `last_level` that promoted (or ran out of
        episodes, with `advance_exhausted`) transfers ITS finished level with `ratios[level]`, moves up a level and flies on.  advance_every = 0: mode off.
        ratios: five transfer ratios, default the reference's."""
        last_level, advance_every = int(last_level), int(advance_every)
        if getattr(self, "envs_per_learner", 1) > 1:
            raise ValueError(TEAMS_BARRIER_ONLY)
        if not 0 <= advance_every <= MAX_ADVANCE_EVERY:
            raise ValueError(f"advance_every must be in 0..{MAX_ADVANCE_EVERY}")
        if advance_every and getattr(self, "_nstep", 0):
            raise ValueError(NSTEP_PLAIN_ONLY)
        if advance_every and self.__dict__.get("_team_nstep", 0):
            raise ValueError(TEAM_NSTEP_BARRIER_ONLY)
        if self.__dict__.get("_team_every", 0):
            raise ValueError(TEAM_CURRICULUM_ONE_MODE)
        r = np.ascontiguousarray(REFERENCE_RATIOS if ratios is None else ratios, dtype=np.float64).ravel()
        if advance_every:
            if not 0 <= last_level < MAX_LEVELS:
                raise ValueError("last_level must be in 0..4")
            if r.size != MAX_LEVELS or not np.isfinite(r).all():
                raise ValueError("ratios must be five finite numbers")
        _lib.check(self.lib.dql_ensemble_set_curriculum(self._h, last_level, advance_every, _p(r), 1 if advance_exhausted else 0))
        self._advance_every = advance_every

    # ---- team curriculum mode: every team walks the levels by itself (include/dql.h) ----
    def set_team_curriculum(self, last_level: int = 4, advance_every: int = MAX_ADVANCE_EVERY, ratios=None, advance_exhausted: bool = True,
                            transfer_order: int = ORDER_REFERENCE):
        """`set_curriculum` for a team ensemble: at every period index that is a multiple of `advance_every`, a frozen team below `last_level` that promoted
        (or ran out of episodes, with `advance_exhausted`) transfers ITS finished level, moves up a level with all E of its envs re-entering through reset
        and their pending windows emptied, and flies on; each launch flies the live teams regrouped by level.  transfer_order: `ORDER_REFERENCE`
        (`Q[k] = Q[k-1] ratios[k]`, the k = 0 wrap) or `ORDER_PAPER` (`Q[k+1] = Q[k] ratios[k+1]`).  advance_every = 0: mode off.  The levels' schedules are
        `set_level_schedules`'; `set_team_nstep` may be called before or after.  Every argument is checked before the library is touched."""
        last_level, advance_every, r, transfer_order = self._checked_team_curriculum(last_level, advance_every, ratios, transfer_order)
        _lib.check(self.lib.dql_ensemble_set_team_curriculum(self._h, last_level, advance_every, _p(r), 1 if advance_exhausted else 0, transfer_order))
        self._team_every = advance_every

    def _checked_team_curriculum(self, last_level, advance_every, ratios, transfer_order):
        """-> (last_level, advance_every, ratios float64[5], transfer_order) as the library takes them; ValueError on what it refuses"""
        last_level, advance_every, transfer_order = int(last_level), int(advance_every), int(transfer_order)
        if not self.__dict__.get("teams", False):
            raise ValueError(TEAM_CURRICULUM_TEAMS_ONLY)
        if not 0 <= advance_every <= MAX_ADVANCE_EVERY:
            raise ValueError(f"advance_every must be in 0..{MAX_ADVANCE_EVERY}")
        if self.__dict__.get("_advance_every", 0) or self.__dict__.get("_recipes", []):
            raise ValueError(TEAM_CURRICULUM_ONE_MODE)
        r = np.ascontiguousarray(REFERENCE_RATIOS if ratios is None else ratios, dtype=np.float64).ravel()
        if advance_every:
            if not 0 <= last_level < MAX_LEVELS:
                raise ValueError("last_level must be in 0..4")
            if r.size != MAX_LEVELS or not np.isfinite(r).all():
                raise ValueError("ratios must be five finite numbers")
            if transfer_order not in (ORDER_REFERENCE, ORDER_PAPER):
                raise ValueError("transfer_order must be 0 (the reference's) or 1 (the paper's)")
        return last_level, advance_every, r, transfer_order

    def set_level_schedules(self, level: int, eps=None, window: int = 100, min_successes: Optional[int] = None, max_episodes: int = 50000):
        """`set_schedules` without the learning rates, for the learners that stand on `level` in curriculum mode (eps default: the reference's for it)"""
        level = int(level)
        if not 0 <= level < MAX_LEVELS:
            raise ValueError("level must be in 0..4")
        e, window, ms, max_episodes = _checked_rule(eps, level, window, min_successes, max_episodes, "the eps table must not be empty")
        _lib.check(self.lib.dql_ensemble_set_level_schedules(self._h, level, _p(e), e.size, window, ms, max_episodes))

    def levels(self):
        """{"level": int32 [L], "promoted_at": int32 [5][L] (episode at level k at which the learner promoted, or -1), "episodes_at": int32 [5][L],
        "entered_period": int64 [5][L] (or -1)}; the row of a learner's current level shows its counters as they stand"""
        level = np.zeros(self.n, dtype=np.int32)
        promoted_at, episodes_at = (np.zeros((MAX_LEVELS, self.n), dtype=np.int32) for _ in range(2))
        entered = np.zeros((MAX_LEVELS, self.n), dtype=np.int64)
        _lib.check(self.lib.dql_ensemble_get_levels(self._h, _p(level), _p(promoted_at), _p(episodes_at), _p(entered)))
        return {"level": level, "promoted_at": promoted_at, "episodes_at": episodes_at, "entered_period": entered}

    def n_unfinished(self) -> int:
        """learners that still have something to fly or a level to advance to (curriculum mode off: `n_live`)"""
        v = C.c_int64()
        _lib.check(self.lib.dql_ensemble_n_unfinished(self._h, C.byref(v)))
        return int(v.value)

    # ---- per-learner recipes (include/dql.h) ----
    def set_recipes(self, recipes, recipe_of):
        """In curriculum mode: learner l flies by `recipes[recipe_of[l]]` (up to 64 `Recipe`s) instead of the ensemble's one quirk word, schedules and rule.
        An empty list uninstalls them.  Every argument is checked before the library is touched."""
        recipes = list(recipes)
        if getattr(self, "envs_per_learner", 1) > 1:
            raise ValueError(TEAMS_BARRIER_ONLY)
        if len(recipes) > MAX_RECIPES:
            raise ValueError(f"at most {MAX_RECIPES} recipes")
        if recipes and getattr(self, "_nstep", 0):
            raise ValueError(NSTEP_PLAIN_ONLY)
        if recipes and self.__dict__.get("_team_nstep", 0):
            raise ValueError(TEAM_NSTEP_BARRIER_ONLY)
        if self.__dict__.get("_team_every", 0):
            raise ValueError(TEAM_CURRICULUM_ONE_MODE)
        if not recipes:
            _lib.check(self.lib.dql_ensemble_set_recipes(self._h, 0, None))
            self._recipes = []
            return
        of = np.ascontiguousarray(recipe_of, dtype=np.int32).ravel()
        if of.size != self.n or of.min() < 0 or of.max() >= len(recipes):
            raise ValueError("recipe_of needs one index in 0..len(recipes) - 1 per learner")
        checked = [r.checked(self.cfg) for r in recipes]
        _lib.check(self.lib.dql_ensemble_set_recipes(self._h, len(recipes), _p(of)))
        self._recipes = []
        for i, (r, (alpha, alpha_min, ratios, lv)) in enumerate(zip(recipes, checked)):
            _lib.check(self.lib.dql_ensemble_set_recipe(self._h, i, int(r.quirks), _p(alpha), alpha.size, alpha_min, _p(ratios), int(r.last_level), 1 if r.advance_exhausted else 0,
                                                        int(r.transfer_order)))
            for k, (e, window, ms, me) in enumerate(lv):
                _lib.check(self.lib.dql_ensemble_set_recipe_level_schedules(self._h, i, k, _p(e), e.size, window, ms, me))
            if int(r.nstep):  # (fresh recipes have n = 0)
                _lib.check(self.lib.dql_ensemble_set_recipe_nstep(self._h, i, int(r.nstep)))
        self._recipes = recipes

    def recipes(self):
        """(the installed `Recipe`s, each with the n-step setting the library holds for it, recipe_of int32 [L]); ([], all -1) while none are installed"""
        of = np.zeros(self.n, dtype=np.int32)
        _lib.check(self.lib.dql_ensemble_get_recipes(self._h, _p(of)))
        if not (of >= 0).all():
            return [], of
        out = []
        for i, r in enumerate(getattr(self, "_recipes", [])):
            v = C.c_int32()
            _lib.check(self.lib.dql_ensemble_get_recipe_nstep(self._h, i, C.byref(v)))
            out.append(replace(r, nstep=int(v.value)))
        return out, of

    def recipe_summary(self):
        """per installed recipe: {"members", "learners_per_level" [5], "promoted_per_level" [5], "exhausted_per_level" [5] (learners that left level k — or
        stand frozen on it — after promoting / out of episodes), "finished"}"""
        recipes, of = self.recipes()
        lv, c = self.levels(), self.counters()
        level, frozen, promoted = lv["level"], c["frozen"], c["promotion_episode"]
        out = []
        for i, r in enumerate(recipes):
            m = of == i
            left = lambda k: m & ((level > k) | ((level == k) & frozen))
            done = m & frozen & ((level >= r.last_level) | ((promoted < 0) & (not r.advance_exhausted)))
            out.append({"members": int(m.sum()), "learners_per_level": np.bincount(level[m], minlength=MAX_LEVELS).tolist(),
                        "promoted_per_level": [int((left(k) & (lv["promoted_at"][k] >= 0)).sum()) for k in range(MAX_LEVELS)],
                        "exhausted_per_level": [int((left(k) & (lv["promoted_at"][k] < 0)).sum()) for k in range(MAX_LEVELS)], "finished": int(done.sum())})
        return out

    def transfer(self, k: int, ratio: float):
        """`DoubleQLearningAgent.transfer_learning` on every learner's tables (k = 0 wraps to the last level, B6)"""
        _lib.check(self.lib.dql_ensemble_transfer(self._h, int(k), float(ratio)))

    # ---- stepping ----
    def run(self, periods: int):
        if int(periods) < 1:
            raise ValueError("periods must be positive")
        _lib.check(self.lib.dql_ensemble_run(self._h, int(periods)))

    def n_live(self) -> int:
        v = C.c_int64()
        _lib.check(self.lib.dql_ensemble_n_live(self._h, C.byref(v)))
        return int(v.value)

    def period_index(self) -> int:
        v = C.c_int64()
        _lib.check(self.lib.dql_ensemble_get_period_index(self._h, C.byref(v)))
        return int(v.value)

    def launches(self):
        """(launches, periods, wave_periods) of the learner kernels since creation (dql_diag_ensemble_launches): the periods summed over the launches, and waves x periods"""
        n, p, wp = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.lib.dql_diag_ensemble_launches(self._h, C.byref(n), C.byref(p), C.byref(wp)))
        return int(n.value), int(p.value), int(wp.value)

    def index_faults(self) -> int:
        v = C.c_int64()
        _lib.check(self.lib.dql_ensemble_index_faults(self._h, C.byref(v)))
        return int(v.value)

    # ---- tables ----
    def _slice(self, first, count):
        first = int(first)
        count = self.n - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.n:
            raise ValueError(f"the slice [first, first + count) must lie inside [0, {self.n}) and hold at least one learner")
        return first, count

    def get_tables(self, first: int = 0, count: Optional[int] = None):
        """(Q_table_a, Q_table_b, state_action_counter), float64 [count][N_CELLS] each, of learners first .. first + count - 1"""
        first, count = self._slice(first, count)
        qa, qb, cnt = (np.empty((count, N_CELLS), dtype=np.float64) for _ in range(3))
        _lib.check(self.lib.dql_ensemble_get_tables(self._h, first, count, _p(qa), _p(qb), _p(cnt)))
        return qa, qb, cnt

    def set_tables(self, qa=None, qb=None, count=None, first: int = 0):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1, N_CELLS) for a in (qa, qb, count)]
        given = [a for a in arrs if a is not None]
        if not given:
            raise ValueError("no table given")
        if len({a.shape[0] for a in given}) != 1:
            raise ValueError("the tables must cover the same learners")
        first, n = self._slice(first, given[0].shape[0])
        _lib.check(self.lib.dql_ensemble_set_tables(self._h, first, n, *(_p(a) for a in arrs)))

    # ---- a state split by one bit of hidden state (include/dql.h dql_ensemble_set_refinement) ----
    def set_refinement(self, feature, cut):
        """From now on every learner learns on the refined state half * 945 + idx_x, half = value >= cut[idx_x] with value the `feature` (a name of
        `ops.SPLIT_FEATURES` or its code) read from the env as it stands before the period — `split_model`'s half, decision for decision.  `cut`: a scalar or
        float64 [945], no NaN; +inf keeps everything in half 0, which then equals a plain ensemble bit for bit.  Accepted once, on a plain ensemble (no teams)
        before its first `run`, with no recipes, curriculum mode or n-step targets; the tables are then `get_refined_tables` / `set_refined_tables`'s
        [L][2][2835] and scoring is `score_refined`.  A bad name, shape or NaN raises ValueError before the library is touched."""
        from . import ops
        feature, cut = ops.split_feature_code(feature), ops.split_cut_array(cut)
        if self.teams or self.envs_per_learner > 1:
            raise ValueError("a refinement is for a plain ensemble: one env per learner, no teams")
        if self._nstep or self._advance_every or self._team_nstep or self._team_every or self.__dict__.get("_recipes", []):
            raise ValueError("refined learners fly the plain mode only: no recipes, no curriculum mode, no n-step targets may be installed")
        _lib.check(self.lib.dql_ensemble_set_refinement(self._h, feature, _p(cut)))

    def refinement(self):
        """(feature name, cut float64 [945]) of the installed refinement, or None"""
        from . import ops
        f, cut = C.c_int32(), np.zeros(N_CELLS // 3, dtype=np.float64)
        _lib.check(self.lib.dql_ensemble_get_refinement(self._h, C.byref(f), _p(cut)))
        return None if f.value < 0 else (ops.SPLIT_FEATURES[f.value], cut)

    def get_refined_tables(self, first: int = 0, count: Optional[int] = None):
        """(Q_table_a, Q_table_b, state_action_counter), float64 [count][2][N_CELLS] each, of learners first .. first + count - 1: the half is the slow index"""
        first, count = self._slice(first, count)
        qa, qb, cnt = (np.empty((count, 2, N_CELLS), dtype=np.float64) for _ in range(3))
        _lib.check(self.lib.dql_ensemble_get_refined_tables(self._h, first, count, _p(qa), _p(qb), _p(cnt)))
        return qa, qb, cnt

    def set_refined_tables(self, qa=None, qb=None, count=None, first: int = 0):
        """`set_tables` for a refined ensemble: each array float64 [K][2][N_CELLS] (or None), for learners first .. first + K - 1"""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (qa, qb, count)]
        given = [a for a in arrs if a is not None]
        if not given:
            raise ValueError("no table given")
        if any(a.ndim != 3 or a.shape[1:] != (2, N_CELLS) for a in given):
            raise ValueError(f"refined tables are [K][2][{N_CELLS}] arrays: the half is the slow index")
        if len({a.shape[0] for a in given}) != 1:
            raise ValueError("the tables must cover the same learners")
        first, n = self._slice(first, given[0].shape[0])
        _lib.check(self.lib.dql_ensemble_set_refined_tables(self._h, first, n, *(_p(a) for a in arrs)))

    def score_refined(self, eval_cfg: DqlConfig, envs_per_learner: int = 64, seed: int = 123, episodes: int = 1, max_steps: int = 600, log: bool = False, first: int = 0,
                      count: Optional[int] = None, timing: dict = None):
        """`ops.score_refined` of learners first .. first + count - 1 on their refined tables where they live (no host copy), with the ensemble's own feature
        and cut, under `eval_cfg`.  The ensemble is left as it was.  Returns what `ops.score_refined` returns, table set k = learner first + k."""
        from . import ops
        first, count = self._slice(first, count)
        n, episodes, max_steps = int(envs_per_learner), int(episodes), int(max_steps)
        ops.score_refined_check_args(eval_cfg, count, n, episodes, max_steps, max_tables=ops.SCORE_MAX_TABLES)
        r = self.refinement()
        if r is None:
            raise ValueError("the ensemble has no refinement: set_refinement first, or use score")
        by_code, steps_sum, ep_code, ep_steps = ops.score_buffers(count, n, episodes, log)
        c = eval_cfg.to_c()
        _lib.check(self.lib.dql_ensemble_score_refined(self._h, C.byref(c), first, count, n, episodes, int(seed), max_steps, _p(by_code), _p(steps_sum), _p(ep_code),
                                                       _p(ep_steps)))
        return ops.score_refined_result(self.lib, ops.SPLIT_FEATURES.index(r[0]), r[1], by_code, steps_sum, ep_code, ep_steps, timing)

    def refined_landing_rates(self, n_envs: int = 4096, episodes: int = 1, level: int = 4, seed: int = 123, dtype=None, quirks=None, max_steps: int = 600, first: int = 0,
                              count: Optional[int] = None, timing: dict = None):
        """`landing_rates` of a refined ensemble: `touchdown_rate` and `goal_hold_rate` per learner through `score_refined`, two launches"""
        from . import evaluation
        quirks = evaluation.Q_PAPER if quirks is None else quirks
        return evaluation.landing_rates_with(lambda cfg, n, sd, ep, ms, t: self.score_refined(cfg, n, sd, ep, ms, first=first, count=count, timing=t),
                                             n_envs, episodes, level, seed, dtype, quirks, max_steps, timing)

    # ---- greedy scoring of the resident tables (include/dql.h dql_ensemble_score) ----
    def score(self, eval_cfg: DqlConfig, envs_per_learner: int = 64, seed: int = 123, episodes: int = 1, max_steps: int = 600, log: bool = False, first: int = 0,
              count: Optional[int] = None, timing: dict = None):
        """`ops.score` of learners first .. first + count - 1 on their tables where they live (no host copy), under `eval_cfg` — any valid config, not
        necessarily the ensemble's own.  The ensemble is left as it was.  Returns what `ops.score` returns, table set k = learner first + k."""
        from . import ops
        first, count = self._slice(first, count)
        n, episodes, max_steps = int(envs_per_learner), int(episodes), int(max_steps)
        ops.score_check_args(count, n, episodes, max_steps)
        by_code, steps_sum, ep_code, ep_steps = ops.score_buffers(count, n, episodes, log)
        c = eval_cfg.to_c()
        _lib.check(self.lib.dql_ensemble_score(self._h, C.byref(c), first, count, n, episodes, int(seed), max_steps, _p(by_code), _p(steps_sum), _p(ep_code), _p(ep_steps)))
        return ops.score_result(self.lib, by_code, steps_sum, ep_code, ep_steps, timing)

    def score_map(self, eval_cfg: DqlConfig, envs_per_learner: int = 64, seed: int = 123, episodes: int = 1, max_steps: int = 600, log: bool = False, first: int = 0,
                  count: Optional[int] = None, timing: dict = None):
        """`ops.score_map` of learners first .. first + count - 1 on their tables where they live (no host copy): `score`'s result plus `visits` int64 [count,
        2835] and, with `log`, `ep_last_cell`.  The ensemble is left as it was.  At most ops.SCORE_MAP_MAX_TABLES learners per call: slice with first / count."""
        from . import ops
        first, count = self._slice(first, count)
        n, episodes, max_steps = int(envs_per_learner), int(episodes), int(max_steps)
        ops.score_map_check_args(count, n, episodes, max_steps)
        by_code, steps_sum, visits, ep_code, ep_steps, ep_last_cell = ops.score_map_buffers(count, n, episodes, log)
        c = eval_cfg.to_c()
        _lib.check(self.lib.dql_ensemble_score_map(self._h, C.byref(c), first, count, n, episodes, int(seed), max_steps, _p(by_code), _p(steps_sum), _p(visits), _p(ep_code),
                                                   _p(ep_steps), _p(ep_last_cell)))
        return ops.score_map_result(self.lib, by_code, steps_sum, visits, ep_code, ep_steps, ep_last_cell, timing)

    def model(self, eval_cfg: DqlConfig, envs_per_learner: int = 64, seed: int = 123, eps: float = 0.1, episodes: int = 1, max_steps: int = 600, first: int = 0,
              count: Optional[int] = None, timing: dict = None):
        """`ops.transition_model` of learners first .. first + count - 1 on their tables where they live (no host copy).  The ensemble is left as it was.  At
        most ops.MODEL_MAX_TABLES learners per call (the pair table is 10.7 MB per learner): slice with first / count."""
        from . import ops
        first, count = self._slice(first, count)
        n, episodes, max_steps, eps = int(envs_per_learner), int(episodes), int(max_steps), float(eps)
        ops.model_check_args(eval_cfg, count, n, episodes, max_steps, eps)
        pairs, reward_fx, terminal, by_code, steps_sum = ops.model_buffers(count)
        c = eval_cfg.to_c()
        _lib.check(self.lib.dql_ensemble_model(self._h, C.byref(c), first, count, n, episodes, int(seed), max_steps, eps, _p(pairs), _p(reward_fx), _p(terminal), _p(by_code),
                                               _p(steps_sum)))
        return ops.model_result(self.lib, pairs, reward_fx, terminal, by_code, steps_sum, timing)

    def split_model(self, eval_cfg: DqlConfig, feature, cut, envs_per_learner: int = 64, seed: int = 123, eps: float = 0.1, episodes: int = 1, max_steps: int = 600,
                    first: int = 0, count: Optional[int] = None, timing: dict = None):
        """`ops.split_model` of learners first .. first + count - 1 on their tables where they live (no host copy).  The ensemble is left as it was.  At most
        ops.MODEL_SPLIT_MAX_TABLES learners per call (21.4 MB of pair table per learner): slice with first / count."""
        from . import ops
        feature, cut = ops.split_feature_code(feature), ops.split_cut_array(cut)
        first, count = self._slice(first, count)
        n, episodes, max_steps, eps = int(envs_per_learner), int(episodes), int(max_steps), float(eps)
        ops.split_model_check_args(eval_cfg, count, n, episodes, max_steps, eps)
        pairs, reward_fx, terminal, feat_sum_fx, by_code, steps_sum = ops.split_model_buffers(count)
        c = eval_cfg.to_c()
        _lib.check(self.lib.dql_ensemble_model_split(self._h, C.byref(c), first, count, n, episodes, int(seed), max_steps, eps, feature, _p(cut), _p(pairs), _p(reward_fx),
                                                     _p(terminal), _p(feat_sum_fx), _p(by_code), _p(steps_sum)))
        return ops.split_model_result(self.lib, feature, cut, pairs, reward_fx, terminal, feat_sum_fx, by_code, steps_sum, timing)

    def returns_map(self, eval_cfg: DqlConfig, envs_per_learner: int = 64, seed: int = 123, eps: float = 0.1, gamma: float = 0.99, episodes: int = 1, max_steps: int = 600,
                    first: int = 0, count: Optional[int] = None, timing: dict = None):
        """`ops.returns_map` of learners first .. first + count - 1 on their tables where they live (no host copy).  The ensemble is left as it was.  At most
        ops.SCORE_MAP_MAX_TABLES learners per call, and count * envs_per_learner * (max_steps + 1) <= 2^29: slice with first / count."""
        from . import ops
        first, count = self._slice(first, count)
        n, episodes, max_steps, eps, gamma = int(envs_per_learner), int(episodes), int(max_steps), float(eps), float(gamma)
        ops.returns_check_args(eval_cfg, count, n, episodes, max_steps, eps, gamma)
        visits, return_fx, cut, by_code, steps_sum = ops.returns_buffers(count)
        c = eval_cfg.to_c()
        _lib.check(self.lib.dql_ensemble_returns(self._h, C.byref(c), first, count, n, episodes, int(seed), max_steps, eps, gamma, _p(visits), _p(return_fx), _p(cut),
                                                 _p(by_code), _p(steps_sum)))
        return ops.returns_result(self.lib, visits, return_fx, cut, by_code, steps_sum, timing)

    def score_grid(self, eval_cfgs, envs_per_learner: int = 64, seed: int = 123, episodes: int = 1, max_steps: int = 600, log: bool = False, touch: bool = True,
                   first: int = 0, count: Optional[int] = None, timing: dict = None):
        """`ops.score_grid` of learners first .. first + count - 1 on their tables where they live (no host copy), under every config of `eval_cfgs` in one
        launch.  The ensemble is left as it was.  Returns what `ops.score_grid` returns, table set k = learner first + k."""
        from . import ops
        eval_cfgs = list(eval_cfgs)
        first, count = self._slice(first, count)
        n, episodes, max_steps = int(envs_per_learner), int(episodes), int(max_steps)
        ops.grid_check_args(eval_cfgs, count, n, episodes, max_steps)
        by_code, steps_sum, touch_hist, ep_code, ep_steps = ops.grid_buffers(len(eval_cfgs), count, n, episodes, log, touch)
        c = ops.grid_configs_to_c(eval_cfgs)
        _lib.check(self.lib.dql_ensemble_score_grid(self._h, c, len(eval_cfgs), first, count, n, episodes, int(seed), max_steps, _p(by_code), _p(steps_sum), _p(touch_hist),
                                                    _p(ep_code), _p(ep_steps)))
        return ops.grid_result(self.lib, eval_cfgs, by_code, steps_sum, touch_hist, ep_code, ep_steps, timing)

    def landing_rates(self, n_envs: int = 4096, episodes: int = 1, level: int = 4, seed: int = 123, dtype=None, quirks=None, max_steps: int = 600, first: int = 0,
                      count: Optional[int] = None, timing: dict = None):
        """`evaluation.landing_rates` of the resident tables: `touchdown_rate` and `goal_hold_rate` per learner, two launches"""
        from . import evaluation
        quirks = evaluation.Q_PAPER if quirks is None else quirks
        return evaluation.landing_rates_with(lambda cfg, n, sd, ep, ms, t: self.score(cfg, n, sd, ep, ms, first=first, count=count, timing=t),
                                             n_envs, episodes, level, seed, dtype, quirks, max_steps, timing)

    def flight_maps(self, n_envs: int = 4096, episodes: int = 1, level: int = 4, seed: int = 123, dtype=None, quirks=None, max_steps: int = 600, log: bool = False,
                    first: int = 0, count: Optional[int] = None, timing: dict = None):
        """`evaluation.flight_maps` of the resident tables: `landing_rates`' figures and both flavours' maps per learner, two launches"""
        from . import evaluation
        quirks = evaluation.Q_PAPER if quirks is None else quirks
        return evaluation.flight_maps_with(lambda cfg, n, sd, ep, ms, t: self.score_map(cfg, n, sd, ep, ms, log=log, first=first, count=count, timing=t),
                                           n_envs, episodes, level, seed, dtype, quirks, max_steps, timing)

    # ---- outputs ----
    def counters(self):
        n = self.n
        dec, eps, suc = (np.zeros(n, dtype=np.int64) for _ in range(3))
        by_code = np.zeros((N_CODES, n), dtype=np.int64)
        promoted, lvl = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        frozen = np.zeros(n, dtype=np.uint8)
        _lib.check(self.lib.dql_ensemble_get_counters(self._h, _p(dec), _p(eps), _p(suc), _p(by_code), _p(promoted), _p(lvl), _p(frozen)))
        return {"decisions": dec, "episodes": eps, "successes": suc, "by_code": by_code, "promotion_episode": promoted, "level_episodes": lvl,
                "frozen": frozen.astype(bool)}

    def episode_log(self):
        """(code uint8 [L][capacity], length uint16 [L][capacity], n int32 [L]): learner l's episode k < min(n[l], capacity); n counts on beyond it"""
        if self.log_capacity < 1:
            raise ValueError("the ensemble was created without an episode log (log_capacity = 0)")
        code = np.zeros((self.n, self.log_capacity), dtype=np.uint8)
        length = np.zeros((self.n, self.log_capacity), dtype=np.uint16)
        cnt = np.zeros(self.n, dtype=np.int32)
        _lib.check(self.lib.dql_ensemble_get_episode_log(self._h, _p(code), _p(length), self.log_capacity, _p(cnt)))
        return code, length, cnt

    def state(self):
        """the env state after the last period: {field: float64 [L E]} for STATE_REAL_FIELDS, {field: int32 [L E]} for STATE_INT_FIELDS, in env order (learner
        l's envs are l E .. l E + E - 1; E = 1 unless the ensemble was made with envs_per_learner)"""
        reals = np.zeros((64, self.n_envs), dtype=np.float64)
        ints = np.zeros((7, self.n_envs), dtype=np.int32)
        _lib.check(self.lib.dql_ensemble_get_state(self._h, _p(reals), _p(ints)))
        rn = [self.lib.dql_field_name(i, 0).decode() for i in range(64)]
        inn = [self.lib.dql_field_name(i, 1).decode() for i in range(7)]
        out = {f: reals[rn.index(f)].copy() for f in STATE_REAL_FIELDS}
        out.update({f: ints[inn.index(f)].copy() for f in STATE_INT_FIELDS})
        return out

    def learning_curve(self, block: int = 1000):
        """Per learner, in the shape of tests/g14_learning_curve.py::curve: goal share and mean length per `block` logged episodes, and the first promotion
        episode (None where the window never filled)."""
        code, length, cnt = self.episode_log()
        promoted = self.counters()["promotion_episode"]
        out = []
        for l in range(self.n):
            m = min(int(cnt[l]), self.log_capacity)
            goal = (code[l, :m] == GOAL).astype(int)
            steps = length[l, :m].astype(np.float64)
            starts = range(0, m - block + 1, block)
            out.append({"goal_share_per_1000_episodes" if block == 1000 else f"goal_share_per_{block}_episodes": [round(float(goal[a:a + block].mean()), 3) for a in starts],
                        "mean_steps_per_1000_episodes" if block == 1000 else f"mean_steps_per_{block}_episodes": [round(float(steps[a:a + block].mean()), 1) for a in starts],
                        "first_promotion_episode": int(promoted[l]) if promoted[l] >= 0 else None})
        return out


def _run_until(ens: SequentialEnsemble, still_running, chunk_periods: int, max_periods: Optional[int], on_chunk) -> int:
    """`ens.run` in chunks while `still_running()` counts a learner and fewer than `max_periods` are flown; -> periods flown"""
    flown = 0
    while still_running() > 0 and (max_periods is None or flown < max_periods):
        k = int(chunk_periods) if max_periods is None else min(int(chunk_periods), int(max_periods) - flown)
        ens.run(k)
        flown += k
        if on_chunk is not None:
            on_chunk(ens, flown)
    return flown


def train_level(ens: SequentialEnsemble, chunk_periods: int = 16 * MAX_PERIODS_PER_LAUNCH, max_periods: Optional[int] = None, on_chunk=None) -> int:
    """Run the current level until every learner is frozen (promoted, or out of episodes) or `max_periods` are flown; -> periods flown."""
    return _run_until(ens, ens.n_live, chunk_periods, max_periods, on_chunk)


def curriculum(ens: SequentialEnsemble, levels: int = 5, first_level: int = 0, ratios=None, max_episodes: Optional[int] = None, max_periods_per_level: Optional[int] = None,
               window: int = 100, success_rate: float = 0.96, on_level=None, nstep: Optional[int] = None, team_nstep: Optional[int] = None):
    """`Trainer.curriculum_training` for the ensemble: per level, run until all learners are frozen, `transfer_learning` of the finished level with the
    reference's ratio, next level.  -> per level, the counters at its end.  nstep: `ens.set_nstep(nstep)` before the first level (the windows must be
    empty: a fresh ensemble, or one whose learners are all frozen); None leaves the ensemble's setting.  team_nstep: `ens.set_team_nstep(team_nstep)` before
    the first level, for a team ensemble (every env's window must be empty: a fresh ensemble, or right after `set_level`)."""
    from .trainer import Trainer
    if nstep is not None:
        ens.set_nstep(nstep)
    if team_nstep is not None:
        ens.set_team_nstep(team_nstep)
    me = SimpleNamespace(_scale_modification_value=(0.8172650252856599, 0.8211253690681617, 0.8257273369742982, 0.8311571820651724))
    history = []
    for k in range(int(first_level), int(levels)):
        if k != ens.cfg.working_curriculum_step or k != first_level:
            ens.set_level(k)
        ens.set_schedules(eps=exploration_rates(k), window=window, min_successes=min_successes_for(window, success_rate),
                          max_episodes=ens.max_episodes if max_episodes is None else max_episodes)
        flown = train_level(ens, max_periods=max_periods_per_level)
        c = ens.counters()
        history.append({"level": k, "periods": flown, "promotion_episode": c["promotion_episode"].copy(), "level_episodes": c["level_episodes"].copy()})
        if on_level is not None:
            on_level(ens, history[-1])
        ratio = float(ratios[k]) if ratios is not None else float(Trainer.transfer_learning_ratio(me, k))
        ens.transfer(k, ratio)
    return history


def curriculum_per_learner(ens: SequentialEnsemble, last_level: int = 4, advance_every: int = MAX_ADVANCE_EVERY, ratios=None, advance_exhausted: bool = True,
                           max_episodes: Optional[int] = None, window: int = 100, success_rate: float = 0.96, chunk_periods: int = 16 * MAX_PERIODS_PER_LAUNCH,
                           max_periods: Optional[int] = None, on_chunk=None):
    """`curriculum` without the ensemble-wide barrier: every learner walks the levels by itself (`SequentialEnsemble.set_curriculum`).  The five levels get
    the schedules `curriculum` gives them (`exploration_rates(k)`, `min_successes_for`, the reference's ratios), then the ensemble runs until nobody is
    unfinished or `max_periods` are flown.  -> `ens.levels()` plus "periods", the periods run."""
    if getattr(ens, "envs_per_learner", 1) > 1:
        raise ValueError(TEAMS_BARRIER_ONLY)
    ms = min_successes_for(window, success_rate)
    budget = ens.max_episodes if max_episodes is None else int(max_episodes)
    for k in range(MAX_LEVELS):
        ens.set_level_schedules(k, exploration_rates(k), window, ms, budget)
    ens.set_curriculum(last_level, advance_every, ratios, advance_exhausted)
    flown = _run_until(ens, ens.n_unfinished, chunk_periods, max_periods, on_chunk)
    out = ens.levels()
    out["periods"] = flown
    return out


def curriculum_per_team(ens: SequentialEnsemble, last_level: int = 4, advance_every: int = MAX_ADVANCE_EVERY, ratios=None, advance_exhausted: bool = True,
                        transfer_order: int = ORDER_REFERENCE, max_episodes: Optional[int] = None, window: int = 100, success_rate: float = 0.96,
                        chunk_periods: int = 16 * MAX_PERIODS_PER_LAUNCH, max_periods: Optional[int] = None, on_chunk=None, team_nstep: Optional[int] = None):
    """`curriculum_per_learner` for a team ensemble: every team walks the levels by itself (`SequentialEnsemble.set_team_curriculum`), with the one-step update
    or, with `team_nstep`, the per-env pending windows (`ens.set_team_nstep(team_nstep)` first: every env's window must be empty; None leaves the ensemble's
    setting).  The five levels get the schedules `curriculum` gives them, then the ensemble runs until no team is unfinished or `max_periods` are flown.
    -> `ens.levels()` plus "periods", the periods run."""
    if not getattr(ens, "teams", False):
        raise ValueError(TEAM_CURRICULUM_TEAMS_ONLY)
    ens._checked_team_curriculum(last_level, advance_every, ratios, transfer_order)
    if int(advance_every) < 1:
        raise ValueError("advance_every must be positive: curriculum_per_team switches the mode on")
    ms = min_successes_for(window, success_rate)
    budget = ens.max_episodes if max_episodes is None else int(max_episodes)
    for k in range(MAX_LEVELS):
        _checked_rule(None, k, window, ms, budget, "the eps table must not be empty")
    if int(chunk_periods) < 1 or (max_periods is not None and int(max_periods) < 0):
        raise ValueError("chunk_periods must be positive and max_periods not negative")
    if team_nstep is not None:
        ens._check_team_nstep(int(team_nstep), True)
        ens.set_team_nstep(team_nstep)
    for k in range(MAX_LEVELS):
        ens.set_level_schedules(k, exploration_rates(k), window, ms, budget)
    ens.set_team_curriculum(last_level, advance_every, ratios, advance_exhausted, transfer_order)
    flown = _run_until(ens, ens.n_unfinished, chunk_periods, max_periods, on_chunk)
    out = ens.levels()
    out["periods"] = flown
    return out


def curriculum_recipes(ens: SequentialEnsemble, recipes, recipe_of, advance_every: int = MAX_ADVANCE_EVERY, chunk_periods: int = 16 * MAX_PERIODS_PER_LAUNCH,
                       max_periods: Optional[int] = None, on_chunk=None):
    """`curriculum_per_learner` with a recipe per learner (`SequentialEnsemble.set_recipes`): curriculum mode on with `advance_every`, the recipes installed,
    then the ensemble runs until nobody is unfinished by its own recipe's rule or `max_periods` are flown.  -> `ens.levels()` plus "periods" and
    "recipe_of"."""
    if getattr(ens, "envs_per_learner", 1) > 1:
        raise ValueError(TEAMS_BARRIER_ONLY)
    ens.set_curriculum(MAX_LEVELS - 1, advance_every)
    ens.set_recipes(recipes, recipe_of)
    flown = _run_until(ens, ens.n_unfinished, chunk_periods, max_periods, on_chunk)
    out = ens.levels()
    out["periods"] = flown
    out["recipe_of"] = ens.recipes()[1]
    return out
