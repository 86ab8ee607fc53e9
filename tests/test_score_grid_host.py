"""The host side of the scenario grid that needs no GPU: `config.scenario_grid` (order, labels, bad field), every refusal `ops.grid_check_args` makes before
the library is touched, the buffers and bindings, and `evaluation.robustness_table` on hand-made counts."""
import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import CHECK_NAMES, F32, F64, Q_PAPER, TRAJ_EIGHT, TRAJ_RPM, DqlConfigC, scenario_grid, simulation_config

import rollout_checks as rc

ROOT = Path(__file__).resolve().parent.parent
N_COLS = len(CHECK_NAMES) + 1
CONTACT, SUCCESS, UNFINISHED = CHECK_NAMES.index("TERMINAL_CONTACT"), CHECK_NAMES.index("TERMINAL_SUCCESS"), len(CHECK_NAMES)


def base_cfg(**kw):
    return simulation_config(working_curriculum_step=4, quirks=Q_PAPER, dtype=F32, **kw)


# ---- config.scenario_grid ----
def test_scenario_grid_is_the_cartesian_product_first_keyword_slowest():
    base = base_cfg()
    cfgs, labels = scenario_grid(base, mp_t_x=[0.4, 0.8, 1.2], trajectory=[TRAJ_RPM, TRAJ_EIGHT])
    assert len(cfgs) == len(labels) == 6
    assert labels == [{"mp_t_x": t, "trajectory": j} for t in (0.4, 0.8, 1.2) for j in (TRAJ_RPM, TRAJ_EIGHT)]
    for c, lab in zip(cfgs, labels):
        assert dataclasses.replace(c, **{f: getattr(base, f) for f in lab}) == base, "a scenario differs from the base in the varied fields only"
        assert all(getattr(c, f) == v for f, v in lab.items())
    assert base.mp_t_x == 1.6 and base.trajectory == TRAJ_RPM, "the base is left as it was"
    one, lab1 = scenario_grid(base)
    assert one == [base] and lab1 == [{}]
    single, lab2 = scenario_grid(base, noise_pos_sd=(0.0, 0.25))
    assert [c.noise_pos_sd for c in single] == [0.0, 0.25] and lab2 == [{"noise_pos_sd": 0.0}, {"noise_pos_sd": 0.25}]


def test_scenario_grid_refuses_an_unknown_field_and_an_empty_axis():
    with pytest.raises(ValueError, match="platform_speed"):
        scenario_grid(base_cfg(), platform_speed=[1.0])
    with pytest.raises(ValueError, match="mp_t_x"):
        scenario_grid(base_cfg(), mp_t_x=[])
    with pytest.raises(ValueError, match="mp_t_x"):
        scenario_grid(base_cfg(), mp_t_x=0.8)


# ---- refusals before the library is touched ----
def test_bad_arguments_are_refused_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded for a call that must be refused on the host")

    monkeypatch.setattr(_lib, "load", no_library)
    cfgs, _ = scenario_grid(base_cfg(), mp_t_x=[0.8, 1.6])
    qa, qb = rc.stage4_tables()
    good = dict(envs_per_table=64, seed=1, episodes=1, max_steps=600)
    bad = {
        "envs 0": dict(envs_per_table=0), "envs 100": dict(envs_per_table=100), "envs -64": dict(envs_per_table=-64), "episodes 0": dict(episodes=0),
        "episodes 65": dict(episodes=65), "max_steps 0": dict(max_steps=0), "max_steps 4097": dict(max_steps=4097), "S K n > 2^30": dict(envs_per_table=1 << 30),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            ops.score_grid(cfgs, qa, qb, **dict(good, **kw))
            pytest.fail(what)
    with pytest.raises(ValueError, match="between 1 and 1024 scenarios"):
        ops.score_grid([], qa, qb, **good)
    with pytest.raises(ValueError, match="between 1 and 1024 scenarios"):
        ops.score_grid([cfgs[0]] * 1025, qa, qb, **good)
    with pytest.raises(ValueError, match="scenario 1 is not a DqlConfig"):
        ops.score_grid([cfgs[0], cfgs[0].to_c()], qa, qb, **good)
    # the five shared fields: the sentence names the scenario and the field
    for field, value in (("dtype", F64), ("two_axis", 1), ("f_ag", 20.0), ("dt", 0.001), ("manager_div", 4)):
        assert field in ops.GRID_SHARED_FIELDS
        with pytest.raises(ValueError, match=f"scenario 2 differs from scenario 0 in {field}"):
            ops.score_grid([cfgs[0], cfgs[1], dataclasses.replace(cfgs[0], **{field: value})], qa, qb, **good)
    assert len(ops.GRID_SHARED_FIELDS) == 5
    for tables in ((qa[:-1], qb[:-1]), (np.stack([qa, qa]), qb), (np.zeros((0, 2835)), np.zeros((0, 2835)))):
        with pytest.raises(ValueError):
            ops.score_grid(cfgs, *tables, **good)
    # S K n = 2^30 exactly passes, one wave more does not
    ops.grid_check_args([cfgs[0]] * 1024, 1, 1 << 20, 64, 4096)
    ops.grid_check_args([cfgs[0]] * 4, 1 << 20, 256, 1, 1)
    with pytest.raises(ValueError, match="2\\^30"):
        ops.grid_check_args([cfgs[0]] * 1024, 1, (1 << 20) + 64, 1, 600)
    with pytest.raises(ValueError, match="2\\^30"):
        ops.grid_check_args([cfgs[0]] * 3, 1 << 20, 512, 1, 600)
    with pytest.raises(AssertionError):  # and a well-formed call does reach the library
        ops.score_grid(cfgs, qa, qb, **good)


# ---- buffers and bindings ----
def test_buffers_have_the_shapes_and_types_of_the_abi():
    by_code, steps_sum, touch, ep_code, ep_steps = ops.grid_buffers(5, 3, 128, 2, True, True)
    assert (by_code.shape, by_code.dtype) == ((5, 3, N_COLS), np.int64) and (steps_sum.shape, steps_sum.dtype) == ((5, 3), np.int64)
    assert (touch.shape, touch.dtype) == ((5, 3, 8), np.int64)
    assert (ep_code.shape, ep_code.dtype) == ((5, 2, 384), np.uint8) and (ep_steps.shape, ep_steps.dtype) == ((5, 2, 384), np.uint16)
    assert all(a.flags.c_contiguous for a in (by_code, steps_sum, touch, ep_code, ep_steps))
    none = ops.grid_buffers(5, 3, 128, 2, False, False)
    assert none[2] is None and none[3] is None and none[4] is None
    hdr = (ROOT / "include" / "dql.h").read_text()
    assert re.search(r"#define DQL_GRID_MAX_SCENARIOS 1024\b", hdr) and re.search(r"#define DQL_GRID_TOUCH_BINS 8\b", hdr) and re.search(r"#define DQL_ABI_VERSION 6\b", hdr)
    assert ops.GRID_MAX_SCENARIOS == 1024 and ops.GRID_TOUCH_BINS == 8


def test_the_scenarios_travel_as_one_contiguous_config_array():
    cfgs, _ = scenario_grid(base_cfg(), mp_t_x=[0.8, 1.6], mass=[0.7, 0.9])
    arr = ops.grid_configs_to_c(cfgs)
    assert len(arr) == 4 and bytes(arr) == b"".join(bytes(c.to_c()) for c in cfgs)
    assert [arr[s].mp_t_x for s in range(4)] == [0.8, 0.8, 1.6, 1.6] and [arr[s].mass for s in range(4)] == [0.7, 0.9, 0.7, 0.9]
    assert isinstance(arr[0], DqlConfigC)


def test_touch_edges_are_rounded_to_the_scenarios_real_type():
    cfgs, _ = scenario_grid(base_cfg(), mp_half_x=[0.55, 0.3])
    e32 = ops.grid_touch_edges(cfgs)
    assert e32.shape == (2, 7) and e32.dtype == np.float64
    assert e32[0].tolist() == [float(np.float32(j * 0.55 * 0.25)) for j in range(1, 8)] and e32[1, 3] == float(np.float32(0.3))
    e64 = ops.grid_touch_edges([dataclasses.replace(c, dtype=F64) for c in cfgs])
    assert e64[0].tolist() == [j * 0.55 * 0.25 for j in range(1, 8)] and e64[0, 3] == 0.55 and (e32 != e64).any()


def test_the_new_symbols_are_declared_and_bound():
    hdr = (ROOT / "include" / "dql.h").read_text()
    diag = (ROOT / "include" / "dql_diag.h").read_text()
    n_args = lambda text, name: re.search(r"\bint %s\(([^;]*)\);" % name, text).group(1).count(",") + 1
    assert n_args(hdr, "dql_score_grid") == len(_lib.SYMBOLS["dql_score_grid"][1]) == 15
    assert n_args(hdr, "dql_ensemble_score_grid") == len(_lib.SYMBOLS["dql_ensemble_score_grid"][1]) == 14
    assert n_args(diag, "dql_diag_score_grid_last") == len(_lib.SYMBOLS["dql_diag_score_grid_last"][1]) == 2
    import __graft_entry__ as g
    g.build_hip()
    lib = _lib.load()
    for name in ("dql_score_grid", "dql_ensemble_score_grid", "dql_diag_score_grid_last"):
        assert getattr(lib, name) is not None
    # the scripts' flags
    assert '"--grid-out"' in (ROOT / "scripts" / "simulation.py").read_text() and '"--score-grid"' in (ROOT / "scripts" / "ensemble_training.py").read_text()


# ---- evaluation.robustness_table ----
def row(**kw):
    r = np.zeros(N_COLS, np.int64)
    for name, v in kw.items():
        r[UNFINISHED if name == "unfinished" else CHECK_NAMES.index(name)] = v
    return r


def test_robustness_table_on_hand_made_counts():
    """3 scenarios x 2 sets, 10 episodes each"""
    by_code = np.array([[row(TERMINAL_CONTACT=8, TERMINAL_FLYZONE_X=2), row(TERMINAL_CONTACT=5, unfinished=5)],
                        [row(TERMINAL_CONTACT=4, TERMINAL_TIMEOUT=1, unfinished=5), row(TERMINAL_CONTACT=5, TERMINAL_FLYZONE_X=5)],
                        [row(TERMINAL_SUCCESS=10), row(unfinished=10)]])
    steps_sum = np.array([[1000, 400], [450, 900], [2000, 0]])
    touch = np.zeros((3, 2, 8), np.int64)
    touch[0, 0] = [4, 2, 1, 1, 0, 0, 0, 0]; touch[0, 1] = [0, 0, 0, 0, 5, 0, 0, 0]; touch[1, 0] = [1, 0, 1, 1, 0, 0, 0, 1]; touch[1, 1] = [5, 0, 0, 0, 0, 0, 0, 0]
    labels = [{"mp_t_x": 0.8}, {"mp_t_x": 1.6}, {"mp_t_x": 2.0}]
    t = evaluation.robustness_table({"by_code": by_code, "steps_sum": steps_sum, "touch_hist": touch}, labels)
    assert t["column"] == "TERMINAL_CONTACT"
    assert t["rate"].tolist() == [[0.8, 0.5], [0.4, 0.5], [0.0, 0.0]]
    assert t["unfinished"].tolist() == [[0.0, 0.5], [0.5, 0.0], [0.0, 1.0]]
    assert t["mean_steps"][:, 0].tolist() == [100.0, 90.0, 200.0] and t["mean_steps"][:2, 1].tolist() == [80.0, 90.0]
    assert np.isnan(t["mean_steps"][2, 1]), "all unfinished: no finished episode has a length"
    assert t["touch_centre"][:2].tolist() == [[0.75, 0.0], [0.25, 1.0]] and t["touch_outside"][:2].tolist() == [[0.0, 1.0], [0.25, 0.0]]
    assert np.isnan(t["touch_centre"][2]).all() and np.isnan(t["touch_outside"][2]).all(), "zero touchdowns: no share"
    assert t["worst_scenario"].tolist() == [2, 2] and t["worst_rate"].tolist() == [0.0, 0.0] and t["worst_label"] == [labels[2], labels[2]]
    # another column; a tie goes to the first scenario
    s = evaluation.robustness_table({"by_code": by_code, "steps_sum": steps_sum}, labels, column="TERMINAL_SUCCESS")
    assert s["rate"].tolist() == [[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]] and s["worst_scenario"].tolist() == [0, 0] and s["worst_label"] == [labels[0], labels[0]]
    assert s["touch_centre"] is None and s["touch_outside"] is None
    # the worst scenario per set, where the sets disagree
    w = evaluation.robustness_table({"by_code": by_code[:2], "steps_sum": steps_sum[:2], "touch_hist": touch[:2]}, labels[:2])
    assert w["worst_scenario"].tolist() == [1, 0] and w["worst_rate"].tolist() == [0.4, 0.5] and w["worst_label"] == [labels[1], labels[0]]


def test_robustness_table_refuses_malformed_input():
    by_code = np.zeros((2, 1, N_COLS), np.int64); by_code[:, :, CONTACT] = 1
    ok = {"by_code": by_code, "steps_sum": np.ones((2, 1), np.int64)}
    evaluation.robustness_table(ok, ["a", "b"])
    with pytest.raises(ValueError, match="labels"):
        evaluation.robustness_table(ok, ["a"])
    with pytest.raises(ValueError):
        evaluation.robustness_table({"by_code": by_code[:, :, :-1], "steps_sum": ok["steps_sum"]}, ["a", "b"])
    with pytest.raises(ValueError):
        evaluation.robustness_table({"by_code": by_code, "steps_sum": np.ones((2, 2), np.int64)}, ["a", "b"])
    with pytest.raises(ValueError, match="no episode"):
        evaluation.robustness_table({"by_code": np.zeros((2, 1, N_COLS), np.int64), "steps_sum": ok["steps_sum"]}, ["a", "b"])
    with pytest.raises(ValueError, match="touch_hist"):
        evaluation.robustness_table(dict(ok, touch_hist=np.zeros((2, 1, 7), np.int64)), ["a", "b"])
    with pytest.raises(ValueError):
        evaluation.robustness_table(ok, ["a", "b"], column="NO_SUCH_CODE")
