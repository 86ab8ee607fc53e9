"""Shared by the scoring tests (CPU emulation and GPU): the stepwise yardstick of `dql_score` / `dql_ensemble_score` (include/dql.h).

`stepwise_episodes` is the multi-episode extension of `rollout_checks.stepwise_first_episodes`: it drives anything with the Engine / Oracle interface one
agent period at a time — the reset period, then `max_steps` more — and notes, the m-th time an env shows FL_DONE (m < episodes), its code and step count.
The sums are taken from exactly those notes."""
import numpy as np

from dql_multirotor_landing_amd.config import CHECK_NAMES

import rollout_checks as rc

N_CODES = len(CHECK_NAMES)
UNFINISHED = N_CODES            # the last column of by_code
NO_CODE, NO_STEPS = 0xFF, 0     # log entries of an episode that did not finish


def stepwise_episodes(stepper, tables, max_steps, episodes):
    """{"ep_code" uint8 [episodes][n], "ep_steps" uint16 [episodes][n], "by_code" int64 [N_CODES + 1], "steps_sum" int} of `stepper`'s first `episodes`
    episodes per env within periods 0 .. max_steps.  `stepper`: a fresh Engine or Oracle (step index 0, no period flown)."""
    qa, qb = tables[0], tables[1]
    stepper.set_tables(qa, qb, None)
    inames = stepper.field_names(True)
    ii = {f: inames.index(f) for f in ("code", "step_count", "flags")}
    ep_code = ep_steps = finished = None
    for _ in range(max_steps + 1):
        stepper.eval_steps(1)
        _, ints = stepper.get_fields()
        if finished is None:
            n = ints.shape[1]
            ep_code = np.full((episodes, n), NO_CODE, np.uint8); ep_steps = np.full((episodes, n), NO_STEPS, np.uint16)
            finished = np.zeros(n, np.int64)
        done = ((ints[ii["flags"]] & rc.FL_DONE) != 0) & (finished < episodes)
        env = np.flatnonzero(done)
        ep_code[finished[env], env] = ints[ii["code"]][env]
        ep_steps[finished[env], env] = ints[ii["step_count"]][env] & 0xFFFF
        finished[env] += 1
        if (finished >= episodes).all():
            break
    out = {"ep_code": ep_code, "ep_steps": ep_steps}
    out.update(sums_of_log(ep_code, ep_steps))
    return out


def sums_of_log(ep_code, ep_steps):
    """by_code [N_CODES + 1] and steps_sum of one table set's log [episodes][n]"""
    by_code = np.array([int((ep_code == k).sum()) for k in range(N_CODES)] + [int((ep_code == NO_CODE).sum())], np.int64)
    assert int(by_code.sum()) == ep_code.size, "a log entry is neither a check code nor 0xff"
    return {"by_code": by_code, "steps_sum": int(ep_steps.astype(np.int64).sum())}


def lane_sums(want):
    """(unfinished episodes, total length of the finished ones) per env of a yardstick: what a lane of the kernel hands to the wave's sums over bit planes"""
    return (want["ep_code"] == NO_CODE).sum(axis=0).astype(np.int64), want["ep_steps"].astype(np.int64).sum(axis=0)


def assert_set_equal(got, k, n, want, what):
    """table set `k` (log columns [k n, (k + 1) n)) of a score result against the yardstick of that set: log, by_code and steps_sum, all =="""
    gc, gs = got["ep_code"][:, k * n:(k + 1) * n], got["ep_steps"][:, k * n:(k + 1) * n]
    for name, g, w in (("ep_code", gc, want["ep_code"]), ("ep_steps", gs, want["ep_steps"])):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, not {w.dtype}{w.shape}"
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: {name} differs in {len(bad)} of {w.size} entries (first: episode {bad[0][0]} env {bad[0][1]}, {g[tuple(bad[0])]} vs {w[tuple(bad[0])]})"
    assert np.array_equal(got["by_code"][k], want["by_code"]), f"{what}: by_code {got['by_code'][k].tolist()} vs {want['by_code'].tolist()}"
    assert int(got["steps_sum"][k]) == want["steps_sum"], f"{what}: steps_sum {int(got['steps_sum'][k])} vs {want['steps_sum']}"
