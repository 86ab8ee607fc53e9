"""`Trainer.load(dir).curriculum_training()` == the uninterrupted run, at every kind of checkpoint (CPU, oracle engine).

The harness is tests/trainer_resume_checks.py: each scenario is flown once uninterrupted (module-wide, never changed), then a fresh run is
cut off right after one checkpoint, loaded and finished, and `assert_same_run` holds histories, the three tables, the episode count and
the engine's counters and period index to the uninterrupted run's with `==`.

Scenarios P / P2 (no restarts; unwindowed / windowed tables) are interrupted at EVERY checkpoint: 17 and 12.  Scenarios R (restarts),
B (steps back) and F (a re-learnt level falls back to its promoted tables) at the first checkpoint of every distinct class
(kind, level, restarts > 0, steps back, re-learning): 5, 18 and 17 classes.  The numbers are those of the runs and are asserted."""
import json
import shutil
import warnings

import numpy as np
import pytest

import trainer_resume_checks as H
from test_dist_gloo import _oracle_engine_class

N_CHECKPOINTS = {"P": 17, "P2": 12}      # P, P2: every checkpoint
N_CLASSES = {"R": 5, "B": 18, "F": 17}   # R, B, F: the first checkpoint of every class


@pytest.fixture(scope="module")
def T():
    import dql_multirotor_landing_amd.trainer as T
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, "Engine", _oracle_engine_class())
        yield T


@pytest.fixture(scope="module")
def uninterrupted(T, tmp_path_factory):
    """name -> (outcome, checkpoint rows, run directory) of the scenario's uninterrupted run: flown once, shared, left unchanged"""
    flown = {}
    def get(name):
        if name not in flown:
            d = tmp_path_factory.mktemp(f"full_{name}")
            with H.scenario(T, name) as (make, _):
                flown[name] = H.record(make, d) + (d / H.RUN_NAME,)
        return flown[name]
    return get


def _resume(T, name, tmp_path, ordinal):
    with H.scenario(T, name) as (make, load), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # (the trainer's category) a complete checkpoint resumes without a word
        return H.resume_from(make, tmp_path, ordinal, load)


def _mid(rows, level, **want):
    return [r for r in rows if r["kind"] == "mid" and r["level"] == level and all(r[k] == v for k, v in want.items())]


def _between(rows, level, **want):
    return [r for r in rows if r["kind"] == "between" and r["level"] == level and all(r[k] == v for k, v in want.items())]


# ---- what the uninterrupted runs must contain, so that nothing below passes vacuously ----
@pytest.mark.parametrize("name", ["P", "P2"])
def test_plain_run_has_checkpoints_of_both_kinds_at_every_level(uninterrupted, name):
    full, rows, _ = uninterrupted(name)
    h = full["history"]
    assert [e["level"] for e in h] == [0, 1, 2] and any(e["promoted"] for e in h)
    assert all(e["restarts"] == 0 and e["step_backs"] == 0 for e in h)
    for level in (0, 1, 2):
        assert len(_mid(rows, level)) >= 2
    assert len(_between(rows, 1)) == 1 and len(_between(rows, 2)) == 1 and len(_between(rows, 3)) == 1
    assert len(rows) == N_CHECKPOINTS[name]
    assert ("between", 1, False, 0, False) in H.first_of_each_class(rows)   # between levels 0 and 1: the first of the three interruptions that used to differ


def test_restart_run_hands_over_its_best_attempt(uninterrupted):
    full, rows, run = uninterrupted("R")
    h = full["history"]
    assert [e["promoted"] for e in h] == [False, False] and h[1]["restarts"] >= 3 and h[1]["exhausted"]
    with open(run / "logs" / "scalars.csv") as f:
        last = [r for r in __import__("csv").DictReader(f) if r["Curriculum step"] == "1"][-1]
    # the level's last chunk logged the rate of the attempt the budget ended in; the entry holds a better one: the best attempt was handed over
    assert h[1]["success_rate"] > float(last["Episode/Success Rate"])
    assert _mid(rows, 1, restarts=0) and [r for r in _mid(rows, 1) if r["restarts"] >= 3]
    assert len(H.first_of_each_class(rows)) == N_CLASSES["R"]


def test_step_back_run_has_checkpoints_inside_everything_a_step_back_touches(uninterrupted):
    full, rows, _ = uninterrupted("B")
    h = full["history"]
    assert [e["level"] for e in h] == [0, 1, 2] and h[2]["step_backs"] == 2
    classes = H.first_of_each_class(rows)
    assert ("mid", 2, True, 0, False) in classes                                   # inside level 2 after a restart
    assert ("mid", 1, False, 1, True) in classes                                   # inside level 1 while it is learnt again
    assert ("between", 2, False, 1, False) in classes                              # between levels after a step back
    assert len(classes) == N_CLASSES["B"]


def test_fall_back_run_restores_the_promoted_entry_and_tables(uninterrupted):
    full, rows, _ = uninterrupted("F")
    h = full["history"]
    assert h[0]["promoted"] and h[1]["promoted"] and not h[2]["promoted"] and h[2]["exhausted"] and h[2]["step_backs"] == 2
    classes = H.first_of_each_class(rows)
    assert ("mid", 1, False, 1, True) in classes and ("between", 2, False, 1, False) in classes   # inside the re-learning, and after the fall-back
    (first,), (fell_back,) = _between(rows, 2, step_backs=0), _between(rows, 2, step_backs=1)
    # level 1 was learnt again, not promoted, and the run went on from the entry and the tables level 1 WAS promoted with
    assert fell_back["history"][1] == dict(first["history"][1], step_backs=1) and h[1] == dict(first["history"][1], step_backs=2)
    for a, b in zip(first["tables"], fell_back["tables"]):
        assert (a == b).all()
    assert len(classes) == N_CLASSES["F"]


# ---- resume == uninterrupted ----
@pytest.mark.parametrize("name,ordinal", [(n, o) for n, k in N_CHECKPOINTS.items() for o in range(k)])
def test_plain_run_resumes_from_every_checkpoint(T, uninterrupted, tmp_path, name, ordinal):
    full, rows, _ = uninterrupted(name)
    back = _resume(T, name, tmp_path, ordinal)
    H.assert_same_run(full, back, engine=ordinal != len(rows) - 1)   # (loaded from the last checkpoint the run is over: no engine is built)


@pytest.mark.parametrize("name,i", [(n, i) for n, k in N_CLASSES.items() for i in range(k)])
def test_run_resumes_from_the_first_checkpoint_of_every_class(T, uninterrupted, tmp_path, name, i):
    full, rows, _ = uninterrupted(name)
    ordinal = list(H.first_of_each_class(rows).values())[i]
    back = _resume(T, name, tmp_path, ordinal)
    H.assert_same_run(full, back, engine=ordinal != len(rows) - 1)


# ---- checkpoints that are not complete ----
def test_trainer_json_written_before_the_bookkeeping_was_carried_still_loads(T, uninterrupted, tmp_path):
    """No "curriculum" / "save_generation" in trainer.json, no curriculum_state.npz, a shard without counters that holds its real fields itself = what the trainer wrote before: the
    run loads with a warning that the restart and step-back bookkeeping starts afresh, and the level in flight goes on as it always did."""
    full, rows, _ = uninterrupted("P")
    ordinal = _mid(rows, 1)[0]["ordinal"]
    with H.scenario(T, "P") as (make, load):
        H.interrupt_after(make, tmp_path, ordinal)
        run = tmp_path / H.RUN_NAME
        st = json.loads((run / "trainer.json").read_text())
        del st["curriculum"], st["save_generation"]
        (run / "trainer.json").write_text(json.dumps(st))
        (run / "curriculum_state.npz").unlink()
        z = dict(np.load(run / "env_state_rank0.npz"))
        z["reals"] = np.load(run / str(z["reals_file"]))   # the real fields used to be a member of the shard itself
        (run / str(z["reals_file"])).unlink()
        del z["stats"], z["reals_file"]
        np.savez(run / "env_state_rank0.npz", **z)
        with pytest.warns(RuntimeWarning, match="restart and step-back bookkeeping: it starts afresh"):
            back = load(tmp_path)
        assert back._resume_run is None and back._resume["level"] == 1
        out = H.finish(back)
    assert out["history"] == full["history"]   # (scenario P has no restarts: nothing of the bookkeeping was needed)
    for a, b in zip(out["tables"], full["tables"]):
        assert (a == b).all()


def test_curriculum_state_of_another_checkpoint_is_not_used(T, uninterrupted, tmp_path):
    """The choice made for a mixed checkpoint (the run was stopped between curriculum_state.npz and trainer.json, so the .npz is one checkpoint
    ahead; here: one behind, which the tag tells apart just as well): the load is NOT refused.  The scalars of trainer.json stand — steps back
    taken still count against max_step_backs — and the best attempts and promoted tables, which are nothing without their tables, start afresh,
    with a warning; as a level resumes without an env-state shard of another checkpoint."""
    full, rows, _ = uninterrupted("B")
    ordinal = H.first_of_each_class(rows)[("mid", 2, True, 1, False)]   # level 2 again after the first step back, one attempt given up
    with H.scenario(T, "B") as (make, load):
        H.interrupt_after(make, tmp_path / "earlier", ordinal - 1)
        H.interrupt_after(make, tmp_path / "run", ordinal)
        shutil.copy(tmp_path / "earlier" / H.RUN_NAME / "curriculum_state.npz", tmp_path / "run" / H.RUN_NAME / "curriculum_state.npz")
        with pytest.warns(RuntimeWarning, match="curriculum_state.npz .* belongs to checkpoint"):
            back = load(tmp_path / "run")
        run = back._resume_run
        assert run["step_backs"] == 1 and run["first_level"] == 0 and run["best_attempt"] is None and run["best_of_level"] == {} and run["promoted_snap"] == {}
        try:
            hist = back.curriculum_training()
        finally:
            H.close(back)
    assert [e["level"] for e in hist] == [0, 1, 2] and hist[2]["step_backs"] == 2   # one more step back, not two: max_step_backs held


def test_shard_whose_real_fields_are_gone_is_not_flown(T, uninterrupted, tmp_path):
    """The real fields of a shard live in a plain .npy beside it, named by the checkpoint's generation; the shard names the file.  Without it the
    level resumes from its tables with a warning, as without the shard — and only the two newest of these files are kept."""
    _, rows, _ = uninterrupted("P")
    ordinal = _mid(rows, 1)[1]["ordinal"]
    with H.scenario(T, "P") as (make, load):
        H.interrupt_after(make, tmp_path, ordinal)
        run = tmp_path / H.RUN_NAME
        st = json.loads((run / "trainer.json").read_text())
        g = st["progress"]["tag"]["generation"]
        assert g == ordinal + 1 and sorted(q.name for q in run.glob("env_state_rank0.reals.g*.npy")) == [f"env_state_rank0.reals.g{g - 1}.npy", f"env_state_rank0.reals.g{g}.npy"]
        (run / f"env_state_rank0.reals.g{g}.npy").unlink()
        back = load(tmp_path)
        try:
            with pytest.warns(RuntimeWarning, match="cannot be read"):
                hist = back.curriculum_training()
        finally:
            H.close(back)
    assert [e["level"] for e in hist] == [0, 1, 2]
