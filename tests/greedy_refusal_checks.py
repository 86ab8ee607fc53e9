"""The refusals of the greedy-flight family, as a table: for each of its 11 entry points (dql_rollout, dql_score, dql_score_map, dql_model, dql_returns,
dql_score_grid and the five dql_ensemble_* twins) one call per argument check with that one argument bad, and a few calls with TWO bad arguments that pin the
order of the checks (the first check that fails decides the sentence).  A row is (entry point, case name) -> (return code, dql_last_error text);
tests/golden/greedy_refusals.json holds the rows as the library answered them when the fixture was recorded (tests/golden/make_greedy_refusals.py --record).
Every row is refused on the host before any launch.  rows_of() also asserts, row by row, that the sentinel-filled output arrays are untouched and that the
operator's dql_diag_*_last answer is what the valid call made first left behind."""
import ctypes as C
import dataclasses

import numpy as np

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import F32, F64, N_CELLS, N_CHECK_CODES, Q_PAPER, simulation_config, training_config
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble

import rollout_checks as rc

SEED, N, EPISODES, MAX_STEPS, LEARNERS = 123, 64, 1, 8, 4
SENTINEL = 77
N_CODES, N_COLS, N_STATES, TOUCH_BINS = N_CHECK_CODES, N_CHECK_CODES + 1, N_CELLS // 3, ops.GRID_TOUCH_BINS  # include/dql.h: the outputs' shapes
OPERATORS = ("rollout", "score", "score_map", "model", "returns", "score_grid")
ENTRY_POINTS = tuple("dql_" + op for op in OPERATORS) + tuple("dql_ensemble_" + op for op in OPERATORS[1:])


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cfg(**kw):
    return simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32, **kw)


def _full(shape, dtype):
    return np.full(shape, SENTINEL, dtype)


class _Setup:
    """what every entry point's rows share: the configs, the tables, the sentinel-filled outputs (sized for the valid call: 1 table set x 64 envs)"""

    def __init__(self):
        self.lib = _lib.load()
        self.cfg = _cfg()
        self.c, self.two = self.cfg.to_c(), _cfg(two_axis=1).to_c()
        self.bad = dataclasses.replace(self.cfg, working_curriculum_step=9).to_c()  # check_config refuses it
        self.qa, self.qb = (np.ascontiguousarray(t) for t in rc.stage4_tables())
        self.scen = [self.cfg, dataclasses.replace(self.cfg, noise_pos_sd=0.1), dataclasses.replace(self.cfg, noise_pos_sd=0.2)]
        self.o = {
            "code": _full(N, np.int32), "steps": _full(N, np.int32), "rec": _full((19, N), np.float64), "trace": _full((MAX_STEPS + 1, 22, 64), np.float64),
            "by_code": _full((3, 1, N_COLS), np.int64), "steps_sum": _full((3, 1), np.int64), "ep_code": _full((3, EPISODES, N), np.uint8),
            "ep_steps": _full((3, EPISODES, N), np.uint16), "ep_last": _full((2, EPISODES, N), np.uint16), "visits": _full((1, N_CELLS), np.int64),
            "pairs": _full((1, N_CELLS, N_STATES), np.uint32), "reward_fx": _full((1, N_CELLS), np.int64), "terminal": _full((1, N_CELLS, N_CODES), np.int64),
            "return_fx": _full((1, N_CELLS), np.int64), "cut": _full(1, np.int64), "touch": _full((3, 1, TOUCH_BINS), np.int64),
        }

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.o.values())

    def scenarios(self, cs):
        return None if cs is None else ops.grid_configs_to_c(cs)


# ---- the calls: keyword arguments with valid defaults; a case overrides the ones it makes bad.  x: the ensemble handle of a twin ----
def _call_rollout(s, x, cfg=None, n_tables=1, envs=N, max_steps=MAX_STEPS, trace_envs=0, trace="absent", **null):
    o = {k: (None if k in null else s.o[k]) for k in ("code", "steps", "rec")}
    qa, qb = (None if "qa" in null else s.qa), (None if "qb" in null else s.qb)
    return s.lib.dql_rollout(C.byref(cfg or s.c), 0, n_tables, envs, SEED, max_steps, _ptr(qa), _ptr(qb), _ptr(o["code"]), _ptr(o["steps"]), _ptr(o["rec"]), trace_envs,
                             None if trace == "absent" else _ptr(s.o["trace"]))


def _outs(s, names, null):
    return [None if k in null else _ptr(s.o[k]) for k in names]


def _tables(s, null):
    return [None if "qa" in null else _ptr(s.qa), None if "qb" in null else _ptr(s.qb)]


def _call_score(s, x, cfg=None, n_tables=1, first=0, envs=N, episodes=EPISODES, max_steps=MAX_STEPS, **null):
    outs = _outs(s, ("by_code", "steps_sum", "ep_code", "ep_steps"), null)
    if x is not None:
        return s.lib.dql_ensemble_score(x, C.byref(cfg or s.c), first, n_tables, envs, episodes, SEED, max_steps, *outs)
    return s.lib.dql_score(C.byref(cfg or s.c), 0, n_tables, envs, episodes, SEED, max_steps, *_tables(s, null), *outs)


def _call_score_map(s, x, cfg=None, n_tables=1, first=0, envs=N, episodes=EPISODES, max_steps=MAX_STEPS, **null):
    outs = _outs(s, ("by_code", "steps_sum", "visits", "ep_code", "ep_steps", "ep_last"), null)
    if x is not None:
        return s.lib.dql_ensemble_score_map(x, C.byref(cfg or s.c), first, n_tables, envs, episodes, SEED, max_steps, *outs)
    return s.lib.dql_score_map(C.byref(cfg or s.c), 0, n_tables, envs, episodes, SEED, max_steps, *_tables(s, null), *outs)


def _call_model(s, x, cfg=None, n_tables=1, first=0, envs=N, episodes=EPISODES, max_steps=MAX_STEPS, eps=0.1, **null):
    outs = _outs(s, ("pairs", "reward_fx", "terminal", "by_code", "steps_sum"), null)
    if x is not None:
        return s.lib.dql_ensemble_model(x, C.byref(cfg or s.c), first, n_tables, envs, episodes, SEED, max_steps, eps, *outs)
    return s.lib.dql_model(C.byref(cfg or s.c), 0, n_tables, envs, episodes, SEED, max_steps, eps, *_tables(s, null), *outs)


def _call_returns(s, x, cfg=None, n_tables=1, first=0, envs=N, episodes=EPISODES, max_steps=MAX_STEPS, eps=0.1, gamma=0.99, **null):
    outs = _outs(s, ("visits", "return_fx", "cut", "by_code", "steps_sum"), null)
    if x is not None:
        return s.lib.dql_ensemble_returns(x, C.byref(cfg or s.c), first, n_tables, envs, episodes, SEED, max_steps, eps, gamma, *outs)
    return s.lib.dql_returns(C.byref(cfg or s.c), 0, n_tables, envs, episodes, SEED, max_steps, eps, gamma, *_tables(s, null), *outs)


def _call_score_grid(s, x, cs="three", n_scen=None, n_tables=1, first=0, envs=N, episodes=EPISODES, max_steps=MAX_STEPS, **null):
    cs = s.scen if cs == "three" else cs
    arr, S = s.scenarios(cs), (len(cs) if n_scen is None else n_scen)
    outs = _outs(s, ("by_code", "steps_sum", "touch", "ep_code", "ep_steps"), null)
    if x is not None:
        return s.lib.dql_ensemble_score_grid(x, arr, S, first, n_tables, envs, episodes, SEED, max_steps, *outs)
    return s.lib.dql_score_grid(arr, S, 0, n_tables, envs, episodes, SEED, max_steps, *_tables(s, null), *outs)


CALLS = {"rollout": _call_rollout, "score": _call_score, "score_map": _call_score_map, "model": _call_model, "returns": _call_returns, "score_grid": _call_score_grid}
NULL = dict  # NULL(by_code=1): that array is passed as a null pointer


# ---- the cases.  A value is the keyword arguments of the call, or a function of the set-up that returns them (configs are made there) ----
_SHAPE = {  # score_check's part, shared by every operator but the roll-outs
    "envs 0": dict(envs=0), "envs -64": dict(envs=-64), "envs 100": dict(envs=100), "episodes 0": dict(episodes=0), "episodes 65": dict(episodes=65),
    "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097), "null by_code": NULL(by_code=1), "null steps_sum": NULL(steps_sum=1),
}
_HOST = {"null qa": NULL(qa=1), "null qb": NULL(qb=1), "bad config": lambda s: dict(cfg=s.bad)}
_LOG2 = {"log code without steps": NULL(ep_steps=1), "log steps without code": NULL(ep_code=1)}
_LOG3 = {
    "log without code": NULL(ep_code=1), "log without steps": NULL(ep_steps=1), "log without last cells": NULL(ep_last=1), "only code": NULL(ep_steps=1, ep_last=1),
    "only steps": NULL(ep_code=1, ep_last=1), "only last cells": NULL(ep_code=1, ep_steps=1),
}
_SLICE = {  # the twins, on an ensemble of LEARNERS = 4 learners; n_tables is their `count`
    "null ensemble": dict(), "count 0": dict(n_tables=0), "first -1": dict(first=-1), "slice beyond the end": dict(first=3, n_tables=2),
    "first beyond the end": dict(first=5), "bad config": lambda s: dict(cfg=s.bad),
}
_TWO_AXES = {"two axes": lambda s: dict(cfg=s.two)}
_EPS = {"eps -0.1": dict(eps=-0.1), "eps 1.5": dict(eps=1.5), "eps nan": dict(eps=float("nan"))}
_GAMMA = {"gamma -0.1": dict(gamma=-0.1), "gamma 1.5": dict(gamma=1.5), "gamma nan": dict(gamma=float("nan"))}


def _differs(field, value):
    return lambda s: dict(cs=[s.scen[0], s.scen[1], dataclasses.replace(s.scen[2], **{field: value})])


_GRID = {
    "n_scenarios 0": dict(n_scen=0), "n_scenarios 1025": lambda s: dict(cs=[s.cfg] * 1025), "null cfgs": dict(cs=None, n_scen=3),
    "scenario 1 fails check_config": lambda s: dict(cs=[s.scen[0], dataclasses.replace(s.scen[1], working_curriculum_step=9), s.scen[2]]),
    "dtype": _differs("dtype", F64), "two_axis": _differs("two_axis", 1), "f_ag": _differs("f_ag", 20.0), "dt": _differs("dt", 0.001), "manager_div": _differs("manager_div", 4),
    "S K n > 2^30": dict(n_tables=1 << 14, envs=1 << 15), "K n = 2^30, S = 3": dict(envs=1 << 30),
}

CASES = {
    "dql_rollout": {
        "n_tables 0": dict(n_tables=0), "n_tables 17": dict(n_tables=17), "envs 0": dict(envs=0), "envs -64": dict(envs=-64), "envs 100": dict(envs=100),
        "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097), "trace_envs -1": dict(trace_envs=-1, trace="given"),
        "trace_envs 65": dict(trace_envs=65, trace="given"), "trace without a buffer": dict(trace_envs=8), "null code": NULL(code=1), "null steps": NULL(steps=1),
        "null rec": NULL(rec=1), **_HOST,
        # two bad arguments: the first check that fails speaks
        "n_tables 0 + envs 100": dict(n_tables=0, envs=100), "envs 100 + max_steps 0": dict(envs=100, max_steps=0), "max_steps 0 + trace_envs 65": dict(max_steps=0, trace_envs=65),
        "trace without a buffer + null qa": dict(trace_envs=8, qa=1), "bad config + null code": lambda s: dict(cfg=s.bad, code=1),
    },
    "dql_score": {
        "n_tables 0": dict(n_tables=0), "n_tables 2^20+1": dict(n_tables=(1 << 20) + 1), "2^31 lanes": dict(n_tables=1 << 20, envs=2048), **_SHAPE, **_LOG2, **_HOST,
        "n_tables 0 + envs 100": dict(n_tables=0, envs=100), "episodes 0 + max_steps 0": dict(episodes=0, max_steps=0),
        "log code without steps + null by_code": NULL(ep_steps=1, by_code=1), "max_steps 0 + null qa": dict(max_steps=0, qa=1), "bad config + null by_code": lambda s: dict(cfg=s.bad, by_code=1),
    },
    "dql_ensemble_score": {
        **_SLICE, **_SHAPE, **_LOG2,
        "slice beyond the end + episodes 65": dict(first=3, n_tables=2, episodes=65), "null by_code + first -1": dict(by_code=1, first=-1),
        "bad config + first -1": lambda s: dict(cfg=s.bad, first=-1), "count 0 + first -1": dict(n_tables=0, first=-1),
    },
    "dql_score_map": {
        "n_tables 0": dict(n_tables=0), "n_tables 2^14+1": dict(n_tables=(1 << 14) + 1), "n_tables 2^20+1": dict(n_tables=(1 << 20) + 1),
        "2^31 lanes": dict(n_tables=1 << 14, envs=1 << 17), **_SHAPE, "null visits": NULL(visits=1), **_LOG3, **_HOST,
        "n_tables 2^14+1 + log without code": dict(n_tables=(1 << 14) + 1, ep_code=1), "log without code + n_tables 0": dict(ep_code=1, n_tables=0),
        "n_tables 0 + null visits": dict(n_tables=0, visits=1), "null visits + null qa": NULL(visits=1, qa=1), "bad config + null visits": lambda s: dict(cfg=s.bad, visits=1),
    },
    "dql_ensemble_score_map": {
        **_SLICE, "count 2^14+1": dict(n_tables=(1 << 14) + 1), **_SHAPE, "null visits": NULL(visits=1), **_LOG3,
        "slice beyond the end + episodes 65": dict(first=3, n_tables=2, episodes=65), "null visits + first -1": dict(visits=1, first=-1),
        "log without code + count 0": dict(ep_code=1, n_tables=0), "bad config + count 0": lambda s: dict(cfg=s.bad, n_tables=0),
    },
    "dql_model": {
        **_TWO_AXES, "n_tables 0": dict(n_tables=0), "n_tables 17": dict(n_tables=17), "n_tables -1": dict(n_tables=-1), **_SHAPE,
        "2^20 envs x 4097 periods": dict(envs=1 << 20, max_steps=4096), "2^20 envs x 4096 periods": dict(envs=1 << 20, max_steps=4095), **_EPS,
        "null pairs": NULL(pairs=1), "null reward_fx": NULL(reward_fx=1), "null terminal": NULL(terminal=1), **_HOST,
        "two axes + n_tables 0": lambda s: dict(cfg=s.two, n_tables=0), "n_tables 17 + null pairs": dict(n_tables=17, pairs=1), "null pairs + envs 100": dict(pairs=1, envs=100),
        "envs 100 + eps 1.5": dict(envs=100, eps=1.5), "2^20 envs x 4097 periods + eps nan": dict(envs=1 << 20, max_steps=4096, eps=float("nan")),
        "eps 1.5 + null qa": dict(eps=1.5, qa=1),
    },
    "dql_ensemble_model": {
        **_SLICE, **_TWO_AXES, "count 17": dict(n_tables=17), **_SHAPE, "eps 2": dict(eps=2.0), "null pairs": NULL(pairs=1), "null reward_fx": NULL(reward_fx=1),
        "null terminal": NULL(terminal=1),
        "slice beyond the end + eps 2": dict(first=3, n_tables=2, eps=2.0), "two axes + first -1": lambda s: dict(cfg=s.two, first=-1),
        "null pairs + count 0": dict(pairs=1, n_tables=0), "bad config + two axes": lambda s: dict(cfg=dataclasses.replace(_cfg(two_axis=1), working_curriculum_step=9).to_c()),
    },
    "dql_returns": {
        **_TWO_AXES, "n_tables 0": dict(n_tables=0), "n_tables 2^14+1": dict(n_tables=(1 << 14) + 1), "n_tables -1": dict(n_tables=-1), **_SHAPE, **_EPS, **_GAMMA,
        "a log of 2^29+2^20 words": dict(envs=1 << 20, max_steps=512), "131 072 envs x 601 periods at gamma 0.99": dict(envs=131072, max_steps=600),
        "16 384 envs x 601 periods at gamma 1": dict(envs=16384, max_steps=600, gamma=1.0),
        "null visits": NULL(visits=1), "null return_fx": NULL(return_fx=1), "null cut_decisions": NULL(cut=1), **_HOST,
        "two axes + n_tables 0": lambda s: dict(cfg=s.two, n_tables=0), "null visits + envs 100": dict(visits=1, envs=100), "eps 1.5 + gamma 1.5": dict(eps=1.5, gamma=1.5),
        "a log of 2^29+2^20 words + eps nan": dict(envs=1 << 20, max_steps=512, eps=float("nan")), "gamma nan + null qa": dict(gamma=float("nan"), qa=1),
    },
    "dql_ensemble_returns": {
        **_SLICE, **_TWO_AXES, **_SHAPE, "eps 2": dict(eps=2.0), "gamma 2": dict(gamma=2.0), "null visits": NULL(visits=1), "null return_fx": NULL(return_fx=1),
        "null cut_decisions": NULL(cut=1),
        "slice beyond the end + gamma 2": dict(first=3, n_tables=2, gamma=2.0), "eps 2 + gamma 2": dict(eps=2.0, gamma=2.0), "null cut_decisions + first -1": dict(cut=1, first=-1),
        "bad config + count 0": lambda s: dict(cfg=s.bad, n_tables=0),
    },
    "dql_score_grid": {
        **_GRID, "n_tables 0": dict(n_tables=0), **_SHAPE, **_LOG2, "null qa": NULL(qa=1), "null qb": NULL(qb=1),
        "null cfgs + n_scenarios 0": dict(cs=None, n_scen=0), "n_scenarios 0 + n_tables 0": dict(n_scen=0, n_tables=0),
        "scenario 1 fails check_config + dtype": lambda s: dict(cs=[s.scen[0], dataclasses.replace(s.scen[1], working_curriculum_step=9), dataclasses.replace(s.scen[2], dtype=F64)]),
        "dt + envs 100": lambda s: dict(envs=100, **_differs("dt", 0.001)(s)), "envs 100 + null qa": dict(envs=100, qa=1), "S K n > 2^30 + null qa": dict(n_tables=1 << 14, envs=1 << 15, qa=1),
    },
    "dql_ensemble_score_grid": {
        **{k: v for k, v in _SLICE.items() if k != "bad config"}, **_GRID, **_SHAPE, **_LOG2,
        "slice beyond the end + episodes 65": dict(first=3, n_tables=2, episodes=65), "null cfgs + first -1": dict(cs=None, n_scen=3, first=-1),
        "dt + count 0": lambda s: dict(n_tables=0, **_differs("dt", 0.001)(s)), "S K n > 2^30 + first -1": dict(n_tables=1 << 14, envs=1 << 15, first=-1),
    },
}


def operator_of(entry):
    return entry[len("dql_ensemble_"):] if entry.startswith("dql_ensemble_") else entry[len("dql_"):]


def _last_record(s, op):
    """(return code, times, instance) of the operator's dql_diag_*_last"""
    a, b, inst = C.c_double(-5.0), C.c_double(-5.0), (C.c_int32 * 3)()
    fn = getattr(s.lib, f"dql_diag_{op}_last")
    rcode = fn(C.byref(a), C.byref(b), inst) if op == "returns" else fn(C.byref(a), inst)
    return rcode, a.value, b.value, list(inst)


def rows_of(entry, need_device=True):
    """{case name: [return code, dql_last_error text]} of one entry point.  With need_device the operator first makes one valid call (1 table set x 64 envs, 1
    episode, max_steps 8) so that its last-call record holds something a refused call could spoil, and a twin gets an ensemble of 4 learners; without, only the
    rows of a host entry point can be taken (none of them reaches the device)."""
    s = _Setup()
    op, twin = operator_of(entry), entry.startswith("dql_ensemble_")
    call = CALLS[op]
    ens = None
    try:
        if need_device:
            assert call(s, None) == 0, s.lib.dql_last_error().decode()
            assert not s.untouched()
            for a in s.o.values():
                a[...] = SENTINEL
            if twin:
                ens = SequentialEnsemble(training_config(0, quirks=Q_PAPER, dtype=F32), LEARNERS, seed=7)
        else:
            assert not twin
        before = _last_record(s, op)
        assert before[0] == (0 if need_device else _lib.ESTATE)
        rows = {}
        for what, kw in CASES[entry].items():
            kw = kw(s) if callable(kw) else kw
            x = None if not twin or what == "null ensemble" else ens._h
            # (a twin's call with x = None goes to the host entry point in CALLS: the null ensemble is passed by hand)
            rcode = _null_ensemble(s, op) if twin and x is None else call(s, x, **kw)
            rows[what] = [int(rcode), s.lib.dql_last_error().decode()]
            assert s.untouched(), f"{entry}, {what}: an output array was written"
            assert _last_record(s, op) == before, f"{entry}, {what}: the last-call record changed"
        return rows
    finally:
        if ens is not None:
            ens.close()


def _null_ensemble(s, op):
    o = {k: _ptr(v) for k, v in s.o.items()}
    c, lib = C.byref(s.c), s.lib
    if op == "score":
        return lib.dql_ensemble_score(None, c, 0, 1, N, EPISODES, SEED, MAX_STEPS, o["by_code"], o["steps_sum"], None, None)
    if op == "score_map":
        return lib.dql_ensemble_score_map(None, c, 0, 1, N, EPISODES, SEED, MAX_STEPS, o["by_code"], o["steps_sum"], o["visits"], None, None, None)
    if op == "model":
        return lib.dql_ensemble_model(None, c, 0, 1, N, EPISODES, SEED, MAX_STEPS, 0.1, o["pairs"], o["reward_fx"], o["terminal"], o["by_code"], o["steps_sum"])
    if op == "returns":
        return lib.dql_ensemble_returns(None, c, 0, 1, N, EPISODES, SEED, MAX_STEPS, 0.1, 0.99, o["visits"], o["return_fx"], o["cut"], o["by_code"], o["steps_sum"])
    return lib.dql_ensemble_score_grid(None, s.scenarios(s.scen), 3, 0, 1, N, EPISODES, SEED, MAX_STEPS, o["by_code"], o["steps_sum"], o["touch"], None, None)
