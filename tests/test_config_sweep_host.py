"""The config sweep's table (tests/config_sweep.py) held to the struct, to the oracle and to the step kernel's device code run on the CPU (no GPU).

Completeness: every member of `dql_config`, arrays element by element, has a row or a written exemption, so a new member fails here until it has a row.
Liveness: the oracle's run at every row differs from its run at the row's unperturbed base, in both real types; that is what keeps every parity test over
the table, on the CPU and on the GPU, from passing vacuously.  The list of rows the greedy kernels fly (the S4 rows and the re-based rows the S4 yardstick
shows live) is held to the oracle in both directions.
Admission and emulation: tests/host_emu/step_emu.cpp's `--admits` (the library's own create_impl decision, dql_host_consts.hpp) gives every row the class
the table says, and every (TICK, XMODE) instance that test_step_host_emulation.instances lists for the row's config computes the oracle's launches bit
for bit: float32 in every admitted layout, in the run-time-axis and the compiled-axis form, and float64 PLAIN.  96 envs; T0 rows: train / eval / external /
train launches of 16 periods from a state flown for 40 periods (test_step_host_emulation.recorded_launches); T4 rows: the same from 80 periods, so that the
time-out at 92 falls inside; S4 rows: greedy launches from period 192, where the touchdowns and ground contacts are, and a training launch.  The oracle's
launches of every row differ from its base's: asserted, so no instance passes a row vacuously.
Liveness at the device's shapes: the flights tests/test_gpu_config_sweep.py compares k_step and k_step_pop with (config_sweep.step_flight) differ from the
base's for every row, real type and population seed.
Late in a run: the same instances from step indices 4 000 000, 2^31 - 8, 2^32 - 8 and 2^40 + 3 (a training and an eval launch of 16 periods, t_max 4 s): the
Philox counter halves, the 64-bit manager-tick index and its float32 conversion, as the device source computes them.
The scenario grid: tests/host_emu/grid_emu.cpp flies the S4 base and every grid row as the scenarios of one launch, in table order and reversed; slice s is
the oracle yardstick of row s.  This is where a record of constants taken from a neighbouring scenario shows on the CPU."""
import collections

import pytest

from dql_multirotor_landing_amd.config import DqlConfig, F32, F64

import numpy as np

from oracle.oracle import Oracle

import config_sweep as cs
import score_checks as sc
import test_score_grid_host_emulation as sge
import test_step_host_emulation as she
from test_score_grid_host_emulation import emu as grid_emu  # noqa: F401  (the module-scoped builds of grid_emu)
from test_step_host_emulation import emu  # noqa: F401  (the module-scoped builds of step_emu)

ADMITS = {"runtime": (True, True), "vehicle": (True, False), "mdp": (False, False)}  # class -> (refm, lit_ok)


def test_every_member_of_the_struct_has_a_row_or_an_exemption():
    have = collections.Counter(r.key for r in cs.ROWS)
    elements = cs.struct_elements()
    missing = [e for e in elements if e not in have and e[0] not in cs.EXEMPT]
    assert not missing, f"dql_config members without a row in tests/config_sweep.py: {missing}"
    assert not [k for k in have if k not in elements], "a row names something that is no member of dql_config"
    assert not [n for n in cs.EXEMPT if any(k[0] == n for k in have)], "an exempted member has a row"
    assert list(cs.EXEMPT) == ["dtype"] and all(len(reason) > 20 for reason in cs.EXEMPT.values())
    assert {r.cls for r in cs.ROWS} == {"runtime", "vehicle", "mdp", "refused"}
    assert sorted(r.id for r in cs.REFUSAL_ROWS) == ["T0-pid_vz[2]=0.5", "T0-pid_yaw[2]=0.5"]
    print(f"{len(elements)} struct elements, {len(cs.ROWS)} rows ({len(cs.PARITY_ROWS)} parity, {len(cs.REFUSAL_ROWS)} refusal):",
          dict(collections.Counter(r.cls for r in cs.ROWS)))


def test_the_s4_base_flies_what_the_table_says():
    """the S4 yardstick on the float32 oracle: 42 contacts, 57 fly-zone-x, 12 minimum-altitude, 17 unfinished"""
    assert cs.base_run("S4", F32)["by_code"].tolist() == [42, 0, 57, 0, 0, 12, 0, 0, 0, 17]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("row", cs.PARITY_ROWS, ids=lambda r: r.id)
def test_every_row_is_live_on_the_oracle(row, dtype):
    assert cs.is_live(row, dtype), f"{row.id}: the oracle's run does not change with the row"


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_the_greedy_rows_are_the_rebased_rows_the_s4_yardstick_shows_live(dtype):
    cand = cs.rebase_candidates()
    live = {r.id for r in cand if cs.is_live(r, dtype)}
    want = {r.id for r in cs.greedy_rows() if not r.id.startswith("S4xy")} - {r.id for r in cs.PARITY_ROWS}
    assert live == want, f"live but not listed: {sorted(live - want)}; listed but not live: {sorted(want - live)}"
    assert {f"S4-{s}" for s in cs.REBASED_NOT_LIVE} == {r.id for r in cand} - live
    classes = collections.Counter(r.cls for r in cs.greedy_rows())
    assert min(classes[c] for c in ADMITS) >= 10, classes
    grid, refused = cs.grid_rows()
    print(f"{len(cs.greedy_rows())} greedy rows {dict(classes)}; {len(grid)} in one grid launch, {len(refused)} the grid refuses")


@pytest.mark.parametrize("family,dtype,seed", [("f32", F32, cs.FLIGHT_SEED), ("f64", F64, cs.FLIGHT_SEED)] + [("pop", d, s) for d in (F32, F64) for s in cs.POP_SEEDS],
                         ids=lambda v: str(v))
def test_every_row_is_live_at_the_shapes_the_device_flies(family, dtype, seed):
    for row in cs.PARITY_ROWS:
        n, ppl, legs = cs.step_flight(row, family)
        cs.assert_flight_live(row, dtype, family, cs.oracle_flight(row.config(dtype), n, seed, ppl, legs), seed=seed)


FLOWN = collections.Counter()
EMU_ENVS, EMU_SEED = 96, 11


def emu_launches(cfg, base):
    """the oracle's launches an instance is held to, by base (module docstring)"""
    if base == "T0":
        return she.recorded_launches(cfg, EMU_ENVS, seed=EMU_SEED, periods=(16,))
    rng = np.random.default_rng(EMU_SEED)
    if base == "T4":
        orc = she.flown_oracle(cfg, EMU_ENVS, EMU_SEED, warm=80)
        plan = [(she.MODE_TRAIN, 0.2, 16), (she.MODE_EVAL, 0.0, 16), (she.MODE_EXTERNAL, 0.0, 1), (she.MODE_TRAIN, 0.2, 16)]
    else:
        orc = Oracle(cfg, EMU_ENVS, seed=EMU_SEED)
        orc.set_tables(*cs.tables())
        orc.set_option("periods_per_launch", 16)
        orc.eval_steps(192)
        plan = [(she.MODE_EVAL, 0.0, 16)] * 3 + [(she.MODE_EXTERNAL, 0.0, 1), (she.MODE_TRAIN, 0.2, 16)]
    return [she.oracle_launch(orc, mode, eps, P, she.ext_actions(rng, cfg, EMU_ENVS) if mode == she.MODE_EXTERNAL else None) for mode, eps, P in plan]


def same_launches(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for s, t in zip(a, b) for x, y in zip(s["out"], t["out"]))


_BASE_LAUNCHES = {}


@pytest.mark.parametrize("row", cs.PARITY_ROWS, ids=lambda r: r.id)
def test_admission_class_and_every_instance_bit_exact_vs_oracle(emu, row, tmp_path):  # noqa: F811
    cfg = row.config(F32)
    refm, lit_ok = she.admits(emu["plain"], cfg, tmp_path)
    assert (refm, lit_ok) == ADMITS[row.cls], f"{row.id}: create_impl answers refm {refm}, lit_ok {lit_ok}; the table says {row.cls}"
    for dtype in (F32, F64):
        cfg = row.config(dtype)
        snaps = emu_launches(cfg, row.base)
        if (row.base, dtype) not in _BASE_LAUNCHES:
            _BASE_LAUNCHES[row.base, dtype] = emu_launches(cs.base_config(row.base, dtype), row.base)
        assert not same_launches(snaps, _BASE_LAUNCHES[row.base, dtype]), f"{row.id} dtype {dtype}: the oracle's launches do not change with the row"
        for tick, xmode in she.instances(cfg, refm, lit_ok):
            for k, s in enumerate(snaps):
                got = she.run_emu(emu["plain"], cfg, tick, xmode, s, tmp_path)
                she.assert_launch_equal(got, s, f"{row.id} dtype {dtype} tick {tick} xmode {xmode} launch {k} (mode {s['mode']}, P {s['P']})")
            FLOWN[row.cls, dtype, tick] += 1
    if row is cs.PARITY_ROWS[-1]:
        print("instances flown per (class, dtype, tick):", dict(FLOWN), "total", sum(FLOWN.values()))


LATE_INDICES = (4_000_000, 2**31 - 8, 2**32 - 8, 2**40 + 3)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("j0", LATE_INDICES, ids=["4e6", "2^31-8", "2^32-8", "2^40+3"])
def test_every_instance_bit_exact_late_in_a_run(emu, j0, dtype, tmp_path):  # noqa: F811
    cfg = DqlConfig(dtype=dtype, t_max=4.0)
    refm, lit_ok = she.admits(emu["plain"], cfg, tmp_path)
    orc = she.flown_oracle(cfg, 96, 11)
    orc.publish_tables()
    orc.step_index = j0
    snaps = [she.oracle_launch(orc, she.MODE_TRAIN, 0.2, 16), she.oracle_launch(orc, she.MODE_EVAL, 0.0, 16)]
    assert sum(int(s["out"][3][1]) for s in snaps) > 0, "no episode ended inside the launches"
    assert orc.step_index == j0 + 32
    for tick, xmode in she.instances(cfg, refm, lit_ok):
        for k, s in enumerate(snaps):
            got = she.run_emu(emu["plain"], cfg, tick, xmode, s, tmp_path)
            she.assert_launch_equal(got, s, f"step index {s['step_index']} dtype {dtype} tick {tick} xmode {xmode} launch {k}")


@pytest.mark.parametrize("order", ["table-order", "reversed"])
def test_one_grid_launch_holds_every_row_as_a_scenario(grid_emu, order, tmp_path):  # noqa: F811
    rows, refused = cs.grid_rows()
    assert {r.field for r in refused} == set(cs.GRID_SHARED)
    scen = ["S4"] + rows
    if order == "reversed":
        scen = scen[::-1]
    cfgs = [cs.base_config(s) if isinstance(s, str) else s.config(F32) for s in scen]
    qa, qb, _ = cs.tables()
    got = sge.run_emu(grid_emu["plain"], cfgs, [(qa, qb)], cs.S4_ENVS, cs.S4_SEED, cs.S4_MAX_STEPS, cs.S4_EPISODES, tmp_path, touch=False)
    for s, r in enumerate(scen):
        want = cs.base_run("S4", F32) if isinstance(r, str) else cs.row_run(r, F32)
        one = {"ep_code": got["ep_code"][s], "ep_steps": got["ep_steps"][s], "by_code": got["by_code"][s], "steps_sum": got["steps_sum"][s]}
        sc.assert_set_equal(one, 0, cs.S4_ENVS, want, f"scenario {s} of {len(scen)} ({r if isinstance(r, str) else r.id}), {order}")
