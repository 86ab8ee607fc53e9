"""Shared by the score-map tests (CPU emulation and GPU): the stepwise yardstick of `dql_score_map` / `dql_ensemble_score_map` (include/dql.h).

`stepwise_map` sits beside `score_checks.stepwise_episodes`: it drives anything with the Engine / Oracle interface one agent period at a time — the reset
period, then `max_steps` more — and builds `visits` and the last cells from `get_fields()` exactly as the header says: an env counts in a period if it has
finished fewer than `episodes` episodes before it and the period is not one of its reset periods; the cell is the index it stood at AFTER THE PREVIOUS period
times 3 plus the action of this one.  It knows nothing of the kernel.  It also counts the events a kernel can get wrong (`events`), so that every case can
assert, before anything else is looked at, that what it is there for occurred."""
import numpy as np

from dql_multirotor_landing_amd.config import N_CELLS

import rollout_checks as rc
import score_checks as sc

FL_WAS_RESET = 8                 # dql_device.hpp
NO_CELL = 0xFFFF                 # ep_last_cell of an episode that did not finish, and of the y plane without a y axis
TAIL = (N_CELLS // 64) * 64      # 2 816: the first cell of the flush's last, partial sweep
LEVEL0_CELLS = 567               # cells of level 0: 189 states x 3 actions


def stepwise_map(stepper, tables, max_steps, episodes, two_axis):
    """{"visits" int64 [N_CELLS], "ep_last_cell" uint16 [2][episodes][n], "ep_code", "ep_steps", "by_code", "steps_sum" as stepwise_episodes gives them, "events"}
    of `stepper`'s first `episodes` episodes per env within periods 0 .. max_steps.  `stepper`: a fresh Engine or Oracle (step index 0, no period flown)."""
    stepper.set_tables(tables[0], tables[1], None)
    inames = stepper.field_names(True)
    ii = {f: inames.index(f) for f in ("code", "step_count", "flags", "action", "idx_x", "idx_y")}
    visits = np.zeros(N_CELLS, np.int64)
    ev = {"same_cell_periods": 0, "tail_decisions": 0, "unfinished_decisions": 0, "early_lanes": 0, "reset_periods": 0, "xy_differ": 0, "decisions": 0,
          "ends_outside_a_decision": 0, "periods": 0}
    n = None
    for j in range(max_steps + 1):
        stepper.eval_steps(1)
        _, ints = stepper.get_fields()
        ints = np.array(ints, dtype=np.int64)
        if n is None:
            n = ints.shape[1]
            ep_code = np.full((episodes, n), sc.NO_CODE, np.uint8); ep_steps = np.full((episodes, n), sc.NO_STEPS, np.uint16)
            last = np.full((2, episodes, n), NO_CELL, np.uint16)
            finished = np.zeros(n, np.int64); open_decisions = np.zeros(n, np.int64); stopped_at = np.full(n, -1, np.int64)
            prev_x = np.full(n, -1, np.int64); prev_y = np.full(n, -1, np.int64)
        flags, action = ints[ii["flags"]], ints[ii["action"]]
        live = finished < episodes                        # before this period
        was_reset = (flags & FL_WAS_RESET) != 0
        counts = live & ~was_reset
        ev["reset_periods"] += int((live & was_reset).sum()); ev["periods"] = j + 1
        cx = prev_x * 3 + (action & 3)
        cy = prev_y * 3 + ((action >> 2) & 3)
        assert ((action[counts] & 3) < 3).all() and (cx[counts] >= 0).all() and (cx[counts] < N_CELLS).all(), "the yardstick met a decision outside the table"
        np.add.at(visits, cx[counts], 1)
        cells = [cx]
        if two_axis:
            assert (((action[counts] >> 2) & 3) < 3).all() and (cy[counts] >= 0).all() and (cy[counts] < N_CELLS).all(), "the yardstick met a y decision outside the table"
            np.add.at(visits, cy[counts], 1)
            cells.append(cy)
            ev["xy_differ"] += int((cx[counts] != cy[counts]).sum())
        for w in range(0, n, 64):                          # a wave: 64 consecutive envs of the set
            m = counts[w:w + 64]
            here = np.concatenate([c[w:w + 64][m] for c in cells])
            if here.size != np.unique(here).size:
                ev["same_cell_periods"] += 1
        for c in cells:
            ev["tail_decisions"] += int((c[counts] >= TAIL).sum()); ev["decisions"] += int(counts.sum())
        open_decisions[counts] += len(cells)
        done = ((flags & rc.FL_DONE) != 0) & live
        ev["ends_outside_a_decision"] += int((done & ~counts).sum())
        env = np.flatnonzero(done)
        ep_code[finished[env], env] = ints[ii["code"]][env]
        ep_steps[finished[env], env] = ints[ii["step_count"]][env] & 0xFFFF
        last[0, finished[env], env] = cx[env]
        if two_axis:
            last[1, finished[env], env] = cy[env]
        finished[env] += 1
        open_decisions[env] = 0
        stopped_at[env[finished[env] >= episodes]] = j
        prev_x, prev_y = ints[ii["idx_x"]].copy(), ints[ii["idx_y"]].copy()
        if (finished >= episodes).all():
            break
    ev["unfinished_decisions"] = int(open_decisions[finished < episodes].sum())
    ev["early_lanes"] = int(((stopped_at >= 0) & (stopped_at < ev["periods"] - 1)).sum())
    out = {"visits": visits, "ep_last_cell": last, "ep_code": ep_code, "ep_steps": ep_steps, "events": ev}
    out.update(sc.sums_of_log(ep_code, ep_steps))
    return out


def assert_map_set_equal(got, k, n, want, what):
    """table set `k` of a score-map result (with its log) against the yardstick of that set: the score's outputs, the map and the last cells, all =="""
    sc.assert_set_equal(got, k, n, want, what)
    g, w = got["visits"][k], want["visits"]
    assert g.dtype == np.int64 and g.shape == w.shape, f"{what}: visits is {g.dtype}{g.shape}"
    bad = np.flatnonzero(g != w)
    assert not len(bad), f"{what}: visits differs in {len(bad)} cells (first: cell {bad[0]}, {g[bad[0]]} vs {w[bad[0]]}; sums {int(g.sum())} vs {int(w.sum())})"
    gl, wl = got["ep_last_cell"][:, :, k * n:(k + 1) * n], want["ep_last_cell"]
    assert gl.dtype == wl.dtype and gl.shape == wl.shape, f"{what}: ep_last_cell is {gl.dtype}{gl.shape}, not {wl.dtype}{wl.shape}"
    bad = np.argwhere(gl != wl)
    assert not len(bad), f"{what}: ep_last_cell differs in {len(bad)} of {wl.size} entries (first: plane {bad[0][0]} episode {bad[0][1]} env {bad[0][2]}, {gl[tuple(bad[0])]} vs {wl[tuple(bad[0])]})"
