"""Every kernel family on the MI355X over the table of tests/config_sweep.py — one row per `dql_config` member and array element, each shown live on the
oracle by tests/test_config_sweep_host.py — and late in a run.  Every comparison is `==`, reals by their bits.  There is no tolerance in this module.

Step kernel (k_step): per row, Engine against Oracle at 320 envs (five waves; a ragged second workgroup at block 256).  T0 / T4 rows: 3 periods per launch, 80
training periods at eps 0.2 from the published tables, then 20 eval periods.  S4 / S4xy rows (platform geometry, altitude floor, PID limits, rotor_max): such a
flight never reaches the platform, so they fly greedily from reset, 16 periods per launch, 192 + 48 eval periods and 16 training periods: touchdowns and
ground contacts fall inside (config_sweep.step_flight).  float32: the automatic layout, option tick 1, tick 3, and tick 4 where the row's class admits it, at
block 0; tick 4 once more at block 256 (the bench's instance).  float64: its one layout, 128 envs, 40 + 10 periods (T4 rows 80 + 20: the time-out of t_max 4 s
comes after 92).  The instance every launch ran (layout, axis form, level-0 instance) is asserted from the row's admission class, and `set_option("tick", 4)`
raises exactly for vehicle and mdp rows.
Population (k_step_pop): the same rows, 2 agents x 512 envs (the smallest population the library makes: an agent is a multiple of 512 envs), each agent
against an Oracle of its own seed, 48 + 12 periods (T4 and S4 rows as above), both real types, the population's instance asserted from the class.
Every step, population and learner case first asserts that the oracle's result at the row differs from the unperturbed base's AT THE SHAPE FLOWN (one cached
base flight per base, real type, shape and seed): a later change of shape cannot make a row vacuous without a failure.
Greedy kernels: `ops.score`, `ops.score_map` and `ops.transition_model` (eps 0) per greedy row (config_sweep.greedy_rows) against the oracle yardstick
score_checks.stepwise_episodes, 64 envs x 2 episodes, 400 periods; one `ops.score_grid` launch of the S4 base and every grid row as scenarios, and a second
in reversed order, slice by slice against `ops.score` and the yardstick; the rows that change f_ag, dt or manager_div are refused by the grid.
Sequential learners (k_learn): SequentialEnsemble against ensemble_checks.Reference, 64 learners, 120 periods, every x-axis T0 / T4 row in float32 but
fold_per_step, which a sequential learner never reads.
float64 subsets (one row or more per admission class; the float32 side keeps every row): GREEDY_F64 and LEARNER_F64 below.

Late in a run: the step kernel from step indices 4 000 000, 2^31 - 8, 2^32 - 8 and 2^40 + 3 (the Philox counter halves, the 64-bit manager-tick index and its
float32 conversion), a population with one agent of two moved there, and a checkpoint / resume across 2^32.

Refusal rows (a derivative gain): ValueError from the engine, the population, the ensemble and every stateless operator that takes a config."""
import collections
import ctypes as C
import dataclasses

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ops
from dql_multirotor_landing_amd.config import DqlConfig, F32, F64

import config_sweep as cs
import ensemble_checks as ec
import score_checks as sc

pytestmark = pytest.mark.gpu

FLOWN = collections.Counter()  # (kernel family, dtype) -> (row, layout) cases flown
IDS = dict(ids=lambda r: r.id)
DT = dict(ids=["f32", "f64"])


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build_hip()


@pytest.fixture(scope="module")
def tables():
    return cs.tables()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# what an oracle, an engine or one agent of a population holds, and their equality
# ---------------------------------------------------------------------------------------------------------------------
def _stats(st):
    return st["decisions"], st["episodes"], tuple(st["by_code"].values()), st["reward_sum"]


def engine_state(eng):
    reals, ints = eng.get_fields()
    qa, qb, cnt = eng.get_tables()
    return {"reals": reals, "ints": ints, "qa": qa.ravel(), "qb": qb.ravel(), "count": cnt.ravel(), "stats": _stats(eng.stats())}


def agent_state(pop, k):
    reals, ints = pop.agent_fields(k)
    qa, qb, cnt = pop.get_tables(k)
    return {"reals": reals, "ints": ints, "qa": qa.ravel(), "qb": qb.ravel(), "count": cnt.ravel(), "stats": _stats(pop.agent_stats(k))}


def assert_state(got, want, names, inames, what):
    for k, nm in enumerate(inames):
        bad = np.flatnonzero(got["ints"][k] != want["ints"][k])
        assert not len(bad), f"{what}: int field {nm} differs in envs {bad[:5]}"
    for k, nm in enumerate(names):
        bad = np.flatnonzero(_bits(got["reals"][k]) != _bits(want["reals"][k]))
        assert not len(bad), f"{what}: field {nm} differs in envs {bad[:5]} ({got['reals'][k][bad[:3]]} vs {want['reals'][k][bad[:3]]})"
    for t in ("qa", "qb", "count"):
        bad = np.flatnonzero(_bits(got[t]) != _bits(want[t]))
        assert not len(bad), f"{what}: table {t} differs in {len(bad)} cells, first {bad[:5]}"
    assert got["stats"] == want["stats"], f"{what}: statistics {got['stats']} vs the oracle's {want['stats']}"


oracle_flight = cs.oracle_flight


def fly(stepper, legs, state_of, want, names, inames, what, after_first=None):
    for k, (periods, eps) in enumerate(legs):
        stepper.train_steps(periods, eps) if eps is not None else stepper.eval_steps(periods)
        if k == 0 and after_first:
            after_first()
        assert_state(state_of(), want[k], names, inames, f"{what}, leg {k} ({periods} periods, eps {eps})")


# ---------------------------------------------------------------------------------------------------------------------
# the step kernel over the table
# ---------------------------------------------------------------------------------------------------------------------
def expected_instance(cfg, cls, tick, block):
    """(the template arguments dql_hip.hip's launch_step_b / launch_step_t pick for a float32 context of at most 8 192 envs, is it the level-0 instance) from
    the row's admission class alone"""
    block = block or 64
    axes = "X_TWO" if cfg.two_axis else "X_ONLY"
    if tick == 1:
        layout, axes = "PLAIN", "X_RUNTIME"
    elif tick == 4:
        assert cls == "runtime"
        layout = "LIT"
    elif cls in ("runtime", "vehicle") and not cfg.two_axis:
        layout, axes = "PACKED_LITM", "X_ONLY"
    else:
        layout = "PACKED"
    level0 = layout in ("LIT", "PACKED_LITM") and axes == "X_ONLY" and cfg.working_curriculum_step == 0
    return f"k_step<float,{block},{layout},{axes}>", level0


STEP_LAYOUTS = ((0, 0), (1, 0), (3, 0), (4, 0), (4, 256))  # (option tick, option block)


@pytest.mark.parametrize("row", cs.PARITY_ROWS, **IDS)
def test_step_kernel_f32_every_layout(row, tables):
    from dql_multirotor_landing_amd.engine import Engine
    cfg, seed, (n, ppl, legs) = row.config(F32), cs.FLIGHT_SEED, cs.step_flight(row, "f32")
    want = oracle_flight(cfg, n, seed, ppl, legs, tables)
    cs.assert_flight_live(row, F32, "f32", want)
    for tick, block in STEP_LAYOUTS:
        eng = Engine(row.config(F32), n, seed=seed)
        try:
            if tick == 4 and row.cls != "runtime":
                with pytest.raises(ValueError, match="tick 4"):
                    eng.set_option("tick", 4)
                continue
            eng.set_option("tick", tick); eng.set_option("block", block)
            eng.set_option("periods_per_launch", ppl)
            eng.set_tables(*tables)
            inst, level0 = expected_instance(cfg, row.cls, tick or 3, block)

            def chosen():
                assert eng.step_instance() == inst, f"{row.id} tick {tick} block {block}: ran {eng.step_instance()}, the class {row.cls} says {inst}"
                assert eng.step_level0() == level0, f"{row.id} tick {tick} block {block}: level-0 instance {eng.step_level0()}, expected {level0}"
            fly(eng, legs, lambda: engine_state(eng), want, eng.field_names(), eng.field_names(True), f"{row.id} tick {tick} block {block}", chosen)
            chosen()
            FLOWN["k_step", "f32"] += 1
        finally:
            eng.close()
    print(row.id, "float32 layouts flown so far:", FLOWN["k_step", "f32"])


@pytest.mark.parametrize("row", cs.PARITY_ROWS, **IDS)
def test_step_kernel_f64(row, tables):
    from dql_multirotor_landing_amd.engine import Engine
    cfg, seed, (n, ppl, legs) = row.config(F64), cs.FLIGHT_SEED, cs.step_flight(row, "f64")
    want = oracle_flight(cfg, n, seed, ppl, legs, tables)
    cs.assert_flight_live(row, F64, "f64", want)
    eng = Engine(row.config(F64), n, seed=seed)
    try:
        eng.set_option("periods_per_launch", ppl)
        eng.set_tables(*tables)
        fly(eng, legs, lambda: engine_state(eng), want, eng.field_names(), eng.field_names(True), f"{row.id} float64")
        assert eng.step_instance() == "k_step<double,64,PLAIN,X_RUNTIME>" and not eng.step_level0()
        FLOWN["k_step", "f64"] += 1
    finally:
        eng.close()


POP_SEEDS = cs.POP_SEEDS
POP_ENVS = cs.TRAIN_FLIGHTS["pop"][0]  # dql_pop_create: envs_per_agent is a multiple of 512


def expected_pop_instance(cfg, cls):
    """the population's launch of 1 024 envs in the automatic layout: the packed tick at block 64, on the literal MDP table where the class admits it; a
    population keeps the generic body at every level"""
    if cfg.dtype == F64:
        return "k_step_pop<double,64,PLAIN,X_RUNTIME>"
    return expected_instance(cfg, cls, 3, 0)[0].replace("k_step<", "k_step_pop<")


def fly_population(cfg, tabs, legs, ppl, start, what, cls="runtime", row=None):
    """a population of two agents against one oracle per agent; start[k]: agent k's step index before the first launch; row: the table's row, whose
    flight must differ from its base's for both agents"""
    from dql_multirotor_landing_amd.population import Population
    wants = [oracle_flight(cfg, POP_ENVS, s, ppl, legs, tabs, step_index=start[k]) for k, s in enumerate(POP_SEEDS)]
    if row is not None:
        for k, s in enumerate(POP_SEEDS):
            cs.assert_flight_live(row, cfg.dtype, "pop", wants[k], seed=s)
    pop = Population(dataclasses.replace(cfg), 2, POP_ENVS, list(POP_SEEDS))
    try:
        pop.set_option("periods_per_launch", ppl)
        for k in range(2):
            pop.set_tables(k, *tabs)
            if start[k]:
                pop.set_agent_step_index(k, start[k])
        names, inames = pop.field_names(), pop.field_names(True)
        done = list(start)
        for leg, (periods, eps) in enumerate(legs):
            pop.pop_train_steps(periods, {0: eps, 1: eps}) if eps is not None else pop.pop_eval_steps(periods)
            assert pop.step_instance() == expected_pop_instance(cfg, cls) and not pop.step_level0(), f"{what}: ran {pop.step_instance()}"
            for k in range(2):
                done[k] += periods
                assert_state(agent_state(pop, k), wants[k][leg], names, inames, f"{what}: agent {k} (seed {POP_SEEDS[k]}), leg {leg}")
                assert pop.agent_step_index(k) == done[k] and pop.index_faults(k) == 0
                assert pop.agent_stats(k)["physics_ticks"] == cfg.ticks_before(done[k])
        assert not np.array_equal(wants[0][-1]["ints"], wants[1][-1]["ints"]), "the two agents flew the same envs"
    finally:
        pop.close()


@pytest.mark.parametrize("dtype", [F32, F64], **DT)
@pytest.mark.parametrize("row", cs.PARITY_ROWS, **IDS)
def test_population_agents_equal_oracles_of_their_own(row, dtype, tables):
    _, ppl, legs = cs.step_flight(row, "pop")
    fly_population(row.config(dtype), tables, legs, ppl, (0, 0), f"{row.id} dtype {dtype}", row.cls, row)
    FLOWN["k_step_pop", "f32" if dtype == F32 else "f64"] += 1


# ---------------------------------------------------------------------------------------------------------------------
# the greedy kernels over the greedy rows
# ---------------------------------------------------------------------------------------------------------------------
GREEDY = cs.greedy_rows()
# float64: the S4 rows of every class, and re-based rows of every class (the grid's refused members among them)
GREEDY_F64 = ("S4-mp_top_z", "S4-mp_half_x=0.3", "S4-rotor_max=512", "S4-pid_vz[4]=7.25", "S4xy-mp_half_y=0.3", "S4-minimum_altitude=0.25",
              "S4-vz_setpoint", "S4-mp_t_x", "S4-mass", "S4-k_f", "S4-v_max", "S4-lim_p[4]", "S4-f_ag", "S4-dt", "S4-manager_div=6")
_SCORES = {}


def greedy_row(row_id):
    return next(r for r in GREEDY if r.id == row_id)


def yardstick(row, dtype):
    """the oracle's stepwise episodes of the row (a string: of that base), computed once"""
    return cs.base_run(row, dtype) if isinstance(row, str) else cs.row_run(row, dtype)


def greedy_tables():
    qa, qb, _ = cs.tables()
    return np.ascontiguousarray(qa.ravel()), np.ascontiguousarray(qb.ravel())


def score_of(row, dtype):
    key = (row if isinstance(row, str) else row.id), dtype
    if key not in _SCORES:
        cfg = cs.base_config(row, dtype) if isinstance(row, str) else row.config(dtype)
        _SCORES[key] = ops.score(cfg, *greedy_tables(), cs.S4_ENVS, cs.S4_SEED, episodes=cs.S4_EPISODES, max_steps=cs.S4_MAX_STEPS, log=True)
    return _SCORES[key]


def check_greedy_row(row, dtype):
    want, what = yardstick(row, dtype), f"{row.id} dtype {dtype}"
    assert not cs.same_run(want, yardstick(row.base, dtype)), f"{what}: the yardstick does not see the row"
    got = score_of(row, dtype)
    sc.assert_set_equal(got, 0, cs.S4_ENVS, want, f"ops.score {what}")
    cfg, (qa, qb) = row.config(dtype), greedy_tables()
    kw = dict(episodes=cs.S4_EPISODES, max_steps=cs.S4_MAX_STEPS)
    m = ops.score_map(cfg, qa, qb, cs.S4_ENVS, cs.S4_SEED, log=True, **kw)
    sc.assert_set_equal(m, 0, cs.S4_ENVS, want, f"ops.score_map {what}")
    tag = "f32" if dtype == F32 else "f64"
    FLOWN["k_score", tag] += 1; FLOWN["k_score_map", tag] += 1
    if not cfg.two_axis:  # the transition model is the x MDP's: a two-axis config is refused (ops.model_check_args)
        t = ops.transition_model(cfg, qa, qb, cs.S4_ENVS, cs.S4_SEED, 0.0, **kw)
        assert t["by_code"][0].tolist() == want["by_code"].tolist() and int(t["steps_sum"][0]) == want["steps_sum"], f"ops.transition_model {what}"
        FLOWN["k_model", tag] += 1
    else:
        with pytest.raises(ValueError, match="two-axis config is refused"):
            ops.transition_model(cfg, qa, qb, cs.S4_ENVS, cs.S4_SEED, 0.0, **kw)
        lib = _lib.load()
        pairs, reward_fx, terminal, by_code, steps_sum = ops.model_buffers(1)
        ptr, c = (lambda a: a.ctypes.data_as(C.c_void_p)), cfg.to_c()
        rc = lib.dql_model(C.byref(c), 0, 1, cs.S4_ENVS, cs.S4_EPISODES, cs.S4_SEED, cs.S4_MAX_STEPS, C.c_double(0.0), ptr(qa), ptr(qb), ptr(pairs), ptr(reward_fx), ptr(terminal),
                           ptr(by_code), ptr(steps_sum))
        msg = lib.dql_last_error().decode()
        assert rc == _lib.EINVAL and "two-axis config is refused" in msg and "nothing was launched" in msg and not by_code.any(), msg


@pytest.mark.parametrize("row", GREEDY, **IDS)
def test_greedy_kernels_f32(row):
    check_greedy_row(row, F32)


@pytest.mark.parametrize("row_id", GREEDY_F64)
def test_greedy_kernels_f64(row_id):
    check_greedy_row(greedy_row(row_id), F64)


def test_the_f64_subsets_hold_every_admission_class():
    assert {greedy_row(i).cls for i in GREEDY_F64} == {"runtime", "vehicle", "mdp"}
    assert {cs.BY_ID[i].cls for i in LEARNER_F64} == {"runtime", "vehicle", "mdp"}


@pytest.mark.parametrize("dtype", [F32, F64], **DT)
@pytest.mark.parametrize("order", ["table-order", "reversed"])
def test_one_grid_launch_holds_every_row_as_a_scenario(order, dtype):
    """scenario 0 (or the last) is the S4 base, the others the grid rows: slice s is ops.score of row s alone and the oracle yardstick of row s"""
    rows, _ = cs.grid_rows()
    if dtype == F64:
        rows = [r for r in rows if r.id in GREEDY_F64]
    scen = ["S4"] + rows
    if order == "reversed":
        scen = scen[::-1]
    cfgs = [cs.base_config(s, dtype) if isinstance(s, str) else s.config(dtype) for s in scen]
    timing = {}
    got = ops.score_grid(cfgs, *greedy_tables(), cs.S4_ENVS, cs.S4_SEED, episodes=cs.S4_EPISODES, max_steps=cs.S4_MAX_STEPS, log=True, timing=timing)
    assert timing["instance"] == f"k_score_grid<{'float' if dtype == F32 else 'double'}, 0, 1>"
    print(len(cfgs), "scenarios x", cs.S4_ENVS, "envs in one launch,", order)
    rows_seen = set()
    for s, r in enumerate(scen):
        what = f"scenario {s} of {len(scen)} ({r if isinstance(r, str) else r.id}), {order}, dtype {dtype}"
        one = {"ep_code": got["ep_code"][s], "ep_steps": got["ep_steps"][s], "by_code": got["by_code"][s], "steps_sum": got["steps_sum"][s]}
        sc.assert_set_equal(one, 0, cs.S4_ENVS, yardstick(r, dtype), f"the oracle yardstick, {what}")
        alone = score_of(r, dtype)
        for f in ("ep_code", "ep_steps", "by_code", "steps_sum"):
            assert np.array_equal(np.asarray(one[f]).reshape(np.asarray(alone[f]).shape), alone[f]), f"{f} of ops.score alone, {what}"
        rows_seen.add(tuple(one["by_code"][0].tolist()) + (int(one["steps_sum"][0]),))
    assert len(rows_seen) >= len(scen) // 2, "most scenarios end differently: a slice taken from a neighbour would show"
    FLOWN["k_score_grid", "f32" if dtype == F32 else "f64"] += len(scen)


@pytest.mark.parametrize("row", cs.grid_rows()[1], **IDS)
def test_the_grid_refuses_a_row_that_changes_the_tick_schedule(row):
    """include/dql.h: scenarios of one launch share f_ag, dt and manager_div; the refusal names the scenario and the member, and nothing is launched"""
    cfgs = [cs.base_config("S4"), cs.base_config("S4"), row.config(F32)]
    qa, qb = greedy_tables()
    with pytest.raises(ValueError, match=f"scenario 2 differs from scenario 0 in {row.field}"):
        ops.score_grid(cfgs, qa, qb, cs.S4_ENVS, cs.S4_SEED)
    lib = _lib.load()
    by_code, steps_sum, touch, _, _ = ops.grid_buffers(3, 1, cs.S4_ENVS, 1, False, True)
    by_code[:] = 77
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dql_score_grid(ops.grid_configs_to_c(cfgs), 3, 0, 1, cs.S4_ENVS, 1, cs.S4_SEED, 50, ptr(qa), ptr(qb), ptr(by_code), ptr(steps_sum), ptr(touch), None, None)
    msg = lib.dql_last_error().decode()
    assert rc == _lib.EINVAL and "dql_score_grid" in msg and "scenario 2" in msg and f"in {row.field}," in msg and "nothing was launched" in msg, msg
    assert (by_code == 77).all()


# ---------------------------------------------------------------------------------------------------------------------
# the sequential learners over the x-axis T0 / T4 rows
# ---------------------------------------------------------------------------------------------------------------------
# dql_ensemble_create refuses what the reference's x-only learner cannot fly: two axes and the figure-eight trajectory (refusal test below)
LEARNER_REFUSED = [r for r in cs.PARITY_ROWS if r.base in ("T0", "T4") and r.field in ("two_axis", "trajectory")]
# fold_per_step chooses how the batched step folds a launch's accumulators into the tables; a sequential learner updates its table in place and never
# reads it, so the reference loop's result does not change with it: no learner row (the liveness assertion in check_learners would refuse it)
LEARNER_NOT_READ = [r for r in cs.PARITY_ROWS if r.field == "fold_per_step"]
LEARNER_ROWS = [r for r in cs.PARITY_ROWS if r.base in ("T0", "T4") and r not in LEARNER_REFUSED and r not in LEARNER_NOT_READ]
LEARNER_F64 = ("T0-mass", "T0-dt", "T0-v_max", "T0-f_ag", "T0-mp_t_x", "T0-manager_div=6", "T4-lim_v[2]", "T4-kalman_q", "T4-t_max")
LEARNERS, LEARNER_SEED, LEARNER_PERIODS, LEARNER_LOG = 64, 2024, 120, 32


_LEARNER_BASES = {}


def reference_result(cfg):
    ref = ec.Reference(cfg, LEARNERS, LEARNER_SEED, log_capacity=LEARNER_LOG)
    ref.run(LEARNER_PERIODS)
    return ref.result()


def check_learners(row, dtype):
    from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
    want = reference_result(row.config(dtype))
    assert (want["qa"] != 0).any() and want["decisions"].min() > 0
    if (row.base, dtype) not in _LEARNER_BASES:
        _LEARNER_BASES[row.base, dtype] = reference_result(cs.base_config(row.base, dtype))
    assert not cs.same_run(want, _LEARNER_BASES[row.base, dtype]), f"{row.id} dtype {dtype}: the reference loop's result does not change with the row"
    ens = SequentialEnsemble(row.config(dtype), LEARNERS, seed=LEARNER_SEED, log_capacity=LEARNER_LOG, eps=ec.EPS_TABLE, max_episodes=1 << 30)
    try:
        ens.run(LEARNER_PERIODS)
        ec.assert_equal(ec.ensemble_result(ens), want, f"{row.id} dtype {dtype}")
        assert ens.index_faults() == 0 and ens.period_index() == LEARNER_PERIODS
        FLOWN["k_learn", "f32" if dtype == F32 else "f64"] += 1
    finally:
        ens.close()


@pytest.mark.parametrize("row", LEARNER_ROWS, **IDS)
def test_sequential_learners_f32(row):
    check_learners(row, F32)


@pytest.mark.parametrize("row_id", LEARNER_F64)
def test_sequential_learners_f64(row_id):
    check_learners(cs.BY_ID[row_id], F64)


@pytest.mark.parametrize("row", LEARNER_REFUSED, **IDS)
def test_the_ensemble_refuses_what_the_x_only_learner_cannot_fly(row):
    from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
    assert [r.id for r in LEARNER_REFUSED] == ["T0-two_axis=1", "T0-trajectory=1"]
    with pytest.raises(ValueError, match="two-axis configs are refused" if row.field == "two_axis" else "figure-eight trajectory is refused"):
        SequentialEnsemble(row.config(F32), LEARNERS, seed=LEARNER_SEED)


# ---------------------------------------------------------------------------------------------------------------------
# refusal rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], **DT)
@pytest.mark.parametrize("row", cs.REFUSAL_ROWS, **IDS)
def test_a_derivative_gain_is_refused_everywhere(row, dtype):
    from dql_multirotor_landing_amd.engine import Engine
    from dql_multirotor_landing_amd.ensemble import SequentialEnsemble
    from dql_multirotor_landing_amd.population import Population
    cfg = row.config(dtype)
    qa, qb = greedy_tables()
    z = np.zeros(4)
    calls = {
        "Engine": lambda: Engine(cfg, 64), "Population": lambda: Population(cfg, 2, 512, [1, 2]), "SequentialEnsemble": lambda: SequentialEnsemble(cfg, 64),
        "discretise": lambda: ops.discretise(cfg, z, z, z, z),
        "mdp_transition": lambda: ops.mdp_transition(cfg, np.zeros(4, np.uint8), np.zeros((7, 4)), np.zeros((8, 4)), np.zeros(4, np.int32)),
        "manager_run": lambda: ops.manager_run(cfg, np.zeros((1, 4, 14)), np.zeros((1, 4), np.uint8)),
        "plant_run": lambda: ops.plant_run(cfg, np.zeros((1, 21)), np.zeros((1, 4, 4))),
        "butterworth_run": lambda: ops.butterworth_run(cfg, z), "kalman_run": lambda: ops.kalman_run(cfg, np.zeros((4, 3)), np.zeros(4, np.uint8)),
        "pid_run": lambda: ops.pid_run(cfg, np.zeros(7), z), "attitude_run": lambda: ops.attitude_run(cfg, np.zeros((4, 4)), np.zeros((4, 3)), np.zeros((4, 4))),
        "platform_run": lambda: ops.platform_run(cfg, 4), "place": lambda: ops.place(cfg, z, z),
        "rollout": lambda: ops.rollout(cfg, (qa, qb), 64, 1, max_steps=5), "score": lambda: ops.score(cfg, qa, qb, 64, 1, max_steps=5),
        "score_map": lambda: ops.score_map(cfg, qa, qb, 64, 1, max_steps=5), "transition_model": lambda: ops.transition_model(cfg, qa, qb, 64, 1, 0.0, max_steps=5),
        "score_grid": lambda: ops.score_grid([cfg], qa, qb, 64, 1, max_steps=5),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="Kd != 0"):
            call()
        print(row.id, name, "refused")


# ---------------------------------------------------------------------------------------------------------------------
# late in a run
# ---------------------------------------------------------------------------------------------------------------------
LATE_INDICES = (4_000_000, 2**31 - 8, 2**32 - 8, 2**40 + 3)
LATE_LEGS = ((16, 0.2), (16, 0.2), (16, None))
LATE_CASES = [(F32, 0), (F32, 1), (F32, 3), (F32, 4), (F64, 0)]


@pytest.mark.parametrize("dtype,tick", LATE_CASES, ids=["f32-auto", "f32-tick1", "f32-tick3", "f32-tick4", "f64"])
@pytest.mark.parametrize("j0", LATE_INDICES, ids=["4e6", "2^31-8", "2^32-8", "2^40+3"])
def test_step_kernel_late_in_a_run(j0, dtype, tick, tables):
    from dql_multirotor_landing_amd.engine import Engine
    cfg, n, seed = DqlConfig(dtype=dtype, t_max=4.0), 320, 11
    want = oracle_flight(cfg, n, seed, 16, LATE_LEGS, tables, step_index=j0)
    assert want[-1]["stats"][1] > 0, "no episode ended inside the launches"
    eng = Engine(DqlConfig(dtype=dtype, t_max=4.0), n, seed=seed)
    try:
        eng.set_option("tick", tick); eng.set_option("periods_per_launch", 16)
        eng.set_tables(*tables)
        eng.publish_tables()
        eng.set_step_index(j0)
        assert eng.step_index() == j0 and eng.stats()["physics_ticks"] == cfg.ticks_before(j0)
        names, inames = eng.field_names(), eng.field_names(True)
        done = j0
        for k, (periods, eps) in enumerate(LATE_LEGS):
            eng.train_steps(periods, eps) if eps is not None else eng.eval_steps(periods)
            done += periods
            assert_state(engine_state(eng), want[k], names, inames, f"step index {j0} + leg {k}, dtype {dtype} tick {tick}")
            assert eng.step_index() == done and eng.stats()["physics_ticks"] == cfg.ticks_before(done)
        if dtype == F32:
            assert eng.step_instance() == expected_instance(cfg, "runtime", tick or 3, 0)[0]
        FLOWN["k_step late", "f32" if dtype == F32 else "f64"] += 1
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", [F32, F64], **DT)
@pytest.mark.parametrize("j0", LATE_INDICES[2:], ids=["2^32-8", "2^40+3"])
def test_population_with_one_agent_late_in_a_run(j0, dtype, tables):
    """agent 1 of two starts at j0 (dql_pop_set_step_index), agent 0 at 0: each equals an oracle of its own"""
    fly_population(DqlConfig(dtype=dtype, t_max=4.0), tables, LATE_LEGS, 16, (0, j0), f"agent 1 at {j0}, dtype {dtype}")
    FLOWN["k_step_pop late", "f32" if dtype == F32 else "f64"] += 1


def test_resume_across_the_high_counter_word():
    """tests/test_gpu_parity.py::test_engine_resume_equals_uninterrupted_run's scheme from step index 2^32 - 8: the checkpoint lies 3 periods before the
    boundary, so the resumed context crosses it by itself"""
    from dql_multirotor_landing_amd.engine import Engine
    j0, k1, k2, n = 2**32 - 8, 5, 27, 1500

    def make():
        e = Engine(DqlConfig(dtype=F32, t_max=4.0, fold_per_step=1), n, seed=9, env_id_offset=77)
        e.set_option("periods_per_launch", 4)
        return e

    full = make()
    full.set_step_index(j0)
    full.train_steps(k1, 0.7); full.publish_tables()
    s_mid = full.stats()
    full.train_steps(k2, 0.3)
    part = make()
    part.set_step_index(j0)
    part.train_steps(k1, 0.7); part.publish_tables()
    tabs, (reals, ints), j = part.get_tables(), part.get_fields(), part.step_index()
    assert j == j0 + k1 < 2**32
    part.close()
    back = make()
    back.set_tables(*tabs); back.set_fields(reals, ints); back.set_step_index(j)
    assert back.step_index() == j and back.stats()["agent_steps"] == 0
    back.train_steps(k2, 0.3)
    assert back.step_index() == full.step_index() == j0 + k1 + k2 > 2**32
    for a, b in zip(back.get_tables(), full.get_tables()):
        assert np.array_equal(_bits(a), _bits(b))
    for a, b in zip(back.get_fields(), full.get_fields()):
        assert np.array_equal(_bits(a), _bits(b))
    s_full, s_back = full.stats(), back.stats()
    assert s_back["agent_steps"] == k2 and s_full["agent_steps"] == k1 + k2 and s_back["physics_ticks"] == s_full["physics_ticks"]
    for key in ("decisions", "episodes"):
        assert s_back[key] == s_full[key] - s_mid[key]
    assert s_back["by_code"] == {c: s_full["by_code"][c] - s_mid["by_code"][c] for c in s_full["by_code"]} and s_full["episodes"] > 0
    full.close(); back.close()


def expected_cases():
    """the (row, kernel family, dtype, layout) cases a whole run of this module flies, from the table alone"""
    rows, runtime = len(cs.PARITY_ROWS), sum(r.cls == "runtime" for r in cs.PARITY_ROWS)
    g64 = [greedy_row(i) for i in GREEDY_F64]
    grid64 = 1 + sum(r in cs.grid_rows()[0] for r in g64)
    return {("k_step", "f32"): 3 * rows + 2 * runtime, ("k_step", "f64"): rows, ("k_step_pop", "f32"): rows, ("k_step_pop", "f64"): rows,
            ("k_score", "f32"): len(GREEDY), ("k_score_map", "f32"): len(GREEDY), ("k_model", "f32"): sum(r.base != "S4xy" for r in GREEDY),
            ("k_score", "f64"): len(g64), ("k_score_map", "f64"): len(g64), ("k_model", "f64"): sum(r.base != "S4xy" for r in g64),
            ("k_score_grid", "f32"): 2 * (1 + len(cs.grid_rows()[0])), ("k_score_grid", "f64"): 2 * grid64,
            ("k_learn", "f32"): len(LEARNER_ROWS), ("k_learn", "f64"): len(LEARNER_F64),
            ("k_step late", "f32"): 4 * len(LATE_INDICES), ("k_step late", "f64"): len(LATE_INDICES), ("k_step_pop late", "f32"): 2, ("k_step_pop late", "f64"): 2}


N_CASES = 1149  # the figure DESIGN.md section 2 gives


def test_the_case_count_is_the_tables():
    """the number of cases written into DESIGN.md is what the table and this module's lists give (no flight needed, any order)"""
    exp = expected_cases()
    print({f"{k[0]} {k[1]}": v for k, v in exp.items()})
    assert sum(exp.values()) == N_CASES, sum(exp.values())


def test_zz_the_cases_flown():
    """a report only: prints the cases this run of the module flew so far; a whole run in one process flies `expected_cases()`, which then is asserted"""
    print(f"{len(cs.ROWS)} rows ({len(cs.PARITY_ROWS)} parity, {len(cs.REFUSAL_ROWS)} refusal), {len(GREEDY)} greedy rows, {len(LEARNER_ROWS)} learner rows")
    print("cases flown:", {f"{k[0]} {k[1]}": v for k, v in sorted(FLOWN.items())}, "total", sum(FLOWN.values()))
    exp = expected_cases()
    assert all(FLOWN[k] <= v for k, v in exp.items()) and set(FLOWN) <= set(exp)
    if sum(FLOWN.values()) >= sum(exp.values()):
        assert dict(FLOWN) == exp
