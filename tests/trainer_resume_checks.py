"""Resume == uninterrupted, at every kind of checkpoint: the harness shared by test_trainer_resume.py (CPU oracle engine),
test_dist_gloo.py (two ranks) and test_gpu_trainer_resume.py (HIP engine).

`record(make_trainer)` flies a run to its end and lists its checkpoints through a wrapped `Trainer.save`;
`resume_from(make_trainer, ordinal)` flies a fresh run, cuts the power right after checkpoint `ordinal` is complete (trainer.json
replaced), `Trainer.load`s the directory and finishes the run; `assert_same_run(a, b)` holds the two to each other with `==`.

What a checkpoint IS is read from what an observer of `save()` sees — `_progress`, the history, the order of the levels — not from the
trainer's own step-back bookkeeping, so the harness describes the checkpoints of any Trainer; where trainer.json carries that
bookkeeping, `record` asserts that the two agree.

`make_trainer(save_path)` builds the Trainer of a scenario; SCENARIOS holds the keywords (all 48-64 envs, t_max 3, 8 periods per
chunk, a checkpoint every 3 chunks, paper mode)."""
from __future__ import annotations

import contextlib
import json
from pathlib import Path

import numpy as np

RUN_NAME = "01-01-2026 10:00:00"   # Trainer.load picks the latest directory named like a date

_P = dict(curriculum_steps=3, n_envs=64, chunk_steps=8, checkpoint_every=3, max_num_episodes=120, t_max=3,
          successive_successful_episodes=10, success_rate=0.25, mode="paper", judge_envs=48, eps_floor=0.3)
_STEP_BACK = dict(curriculum_steps=3, n_envs=48, chunk_steps=8, checkpoint_every=3, t_max=3, mode="paper", judge_envs=16,
                  successive_successful_episodes=10, eps_floor=0.3, restart_after=1.5, step_back_after=1, max_step_backs=2)
SCENARIOS = {
    # the keywords of test_trainer_resume_equals_uninterrupted_run, unwindowed and on the windowed table schedule
    "P": dict(_P, sync_period=None),
    "P2": dict(_P, sync_period=2),
    # test_level_restart_on_plateau: level 1 restarts until its budget ends
    "R": dict(curriculum_steps=2, n_envs=48, chunk_steps=8, checkpoint_every=3, max_num_episodes=400, t_max=3, mode="paper", judge_envs=16,
              successive_successful_episodes=10, eps_floor=0.3, success_rate=2.0, restart_after=1.5),
    # test_step_back_after_failed_restarts: nothing is ever promoted, level 2 steps back twice
    "B": dict(_STEP_BACK, max_num_episodes=500, success_rate=2.0),
    # test_step_back_falls_back_...: scripted_window() promotes levels 0 and 1 once; level 1 learnt again falls back to its promoted tables
    "F": dict(_STEP_BACK, max_num_episodes=600),
}


class PowerCut(Exception):
    pass


def scripted_window(T):
    """PromotionWindow of scenario F: levels 0 and 1 pass at their first judged episodes as long as the run has not stepped back, nothing
    passes after.  A function of what a checkpoint carries (working level, steps back) — a resumed process plays the same script."""
    real = T.PromotionWindow

    class Scripted(real):
        trainer = None   # the Trainer whose curriculum_training() builds this window: set by the scenario's make_trainer

        def push_flags(self, flags):
            super().push_flags(flags)
            tr = Scripted.trainer
            return 0 if len(flags) and tr._working_curriculum_step <= 1 and tr._step_backs == 0 else None
    return Scripted


@contextlib.contextmanager
def scenario(T, name, **over):
    """(make_trainer, load) of a scenario on the trainer module `T` (whose `Engine` the caller has chosen); `over`: keywords on top of the
    scenario's.  Scenario F flies under its scripted promotion window, put into `T` for the duration."""
    kw = dict(SCENARIOS[name], **over)
    real = T.PromotionWindow
    window = scripted_window(T) if name == "F" else real

    def make(save_path):
        tr = T.Trainer(save_path=save_path, **kw)
        if name == "F":
            window.trainer = tr
        return tr

    def load(directory, **load_kw):
        tr = T.Trainer.load(directory, **load_kw)
        if name == "F":
            window.trainer = tr
        return tr
    T.PromotionWindow = window
    try:
        yield make, load
    finally:
        T.PromotionWindow = real


def strip(hist):
    """history without the wall-clock fields; of `wall_first_promoted_s` only whether it is there"""
    out = []
    for h in hist:
        e = {k: v for k, v in h.items() if not k.startswith("wall")}
        e["first_promoted"] = h.get("wall_first_promoted_s") is not None
        out.append(e)
    return json.loads(json.dumps(out))


def close(tr):
    """the engine (a HIP context) and the scalar log of a Trainer that finished or was cut off"""
    fh = getattr(tr, "_log_fh", None)
    if fh is not None and not fh.closed:
        fh.close()
    eng = getattr(tr, "_engine", None)
    if eng is not None and hasattr(eng, "close"):
        eng.close()


def outcome(tr):
    """what assert_same_run compares, copied out of a finished Trainer (which can then be closed).  A run loaded from its LAST checkpoint has
    nothing left to train and builds no engine: "engine" is None."""
    a, eng = tr._double_q_learning_agent, tr._engine
    out = {"history": strip(tr.history),
           "tables": tuple(np.array(t, dtype=np.float64) for t in (a.Q_table_a, a.Q_table_b, a.state_action_counter)),
           "curriculum_episode_count": int(tr._curriculum_episode_count), "engine": None}
    if eng is not None:
        st = eng.stats()
        out["engine"] = {"tables": tuple(np.array(t, dtype=np.float64).reshape(-1) for t in eng.get_tables()),
                         "decisions": int(st["decisions"]), "episodes": int(st["episodes"]), "step_index": int(eng.step_index())}
    return out


def assert_same_run(a, b, engine=True):
    """engine=False only where one of the two was loaded from the run's last checkpoint (no engine: see outcome)"""
    assert a["history"] == b["history"]
    for name, x, y in zip(("Q_table_a", "Q_table_b", "state_action_counter"), a["tables"], b["tables"]):
        assert x.shape == y.shape and (x == y).all(), f"{name}: {int((x != y).sum())} cells differ"
    assert a["curriculum_episode_count"] == b["curriculum_episode_count"]
    if engine:
        ea, eb = a["engine"], b["engine"]
        for x, y in zip(ea["tables"], eb["tables"]):
            assert (x == y).all()
        assert (ea["decisions"], ea["episodes"], ea["step_index"]) == (eb["decisions"], eb["episodes"], eb["step_index"])
    else:
        assert (a["engine"] is None) != (b["engine"] is None)


class _Observer:
    """Describes every checkpoint from outside: what `save()` leaves visible."""

    def __init__(self, tr):
        self.tr, self.rows = tr, []
        self._cur, self._step_backs, self._relearning = None, 0, None

    def after_save(self):
        tr = self.tr
        pr = tr._progress
        mid = pr is not None
        last = tr.history[-1]["level"] if tr.history else None
        cur = int(pr["level"]) if mid else last          # the level in flight / the level that just ended
        if self._cur is not None and cur is not None and cur < self._cur:
            self._step_backs += 1                        # the levels only ever go down by a step back: `cur` is learnt again
            self._relearning = cur
        if not mid and cur == self._relearning:
            self._relearning = None                      # learnt again (or fallen back): over
        self._cur = cur
        row = {"ordinal": len(self.rows), "kind": "mid" if mid else "between", "level": int(pr["level"]) if mid else int(tr._working_curriculum_step),
               "restarts": int(pr.get("restarts", 0)) if mid else 0, "step_backs": self._step_backs,
               "relearning": mid and self._relearning == cur, "last_history_level": last, "history": strip(tr.history)}
        if not mid:  # the tables the next level starts from, as the checkpoint holds them
            a = tr._double_q_learning_agent
            row["tables"] = tuple(np.array(t, dtype=np.float64) for t in (a.Q_table_a, a.Q_table_b, a.state_action_counter))
        carried = json.loads((Path(tr._save_path) / "trainer.json").read_text()).get("curriculum") if tr._rank == 0 else None
        if carried is not None:  # the trainer's own bookkeeping, as checkpointed, says the same
            assert carried["step_backs"] == row["step_backs"]
            assert (carried["relearning"] is not None and carried["relearning"] == row["level"]) == row["relearning"]
        self.rows.append(row)
        return row


def checkpoint_class(row):
    return (row["kind"], row["level"], row["restarts"] > 0, row["step_backs"], row["relearning"])


def first_of_each_class(rows):
    """{class: ordinal of its first checkpoint}, in the order the run meets them"""
    out = {}
    for r in rows:
        out.setdefault(checkpoint_class(r), r["ordinal"])
    return out


def record(make_trainer, save_path):
    """Fly a run to its end.  Returns (outcome, one row per checkpoint)."""
    tr = make_trainer(Path(save_path) / RUN_NAME)
    try:
        obs = _Observer(tr)
        real_save = tr.save
        def save():
            real_save()
            obs.after_save()
        tr.save = save
        tr.curriculum_training()
        return outcome(tr), obs.rows
    finally:
        close(tr)


def interrupt_after(make_trainer, save_path, ordinal):
    """Fly a fresh run until checkpoint `ordinal` is complete, then cut the power.  Returns that checkpoint's row."""
    tr = make_trainer(Path(save_path) / RUN_NAME)
    try:
        obs = _Observer(tr)
        real_save = tr.save
        def save():
            real_save()
            if obs.after_save()["ordinal"] == ordinal:
                raise PowerCut()
        tr.save = save
        try:
            tr.curriculum_training()
        except PowerCut:
            return obs.rows[-1]
        raise AssertionError(f"the run ended after {len(obs.rows)} checkpoints, before checkpoint {ordinal}")
    finally:
        close(tr)


def resume_from(make_trainer, save_path, ordinal, load):
    """interrupt_after + `load(directory)` (Trainer.load, with whatever the scenario's make_trainer adds that a checkpoint cannot hold)
    + the rest of the run.  Returns the resumed run's outcome."""
    interrupt_after(make_trainer, save_path, ordinal)
    return finish(load(Path(save_path)))


def finish(tr):
    """the rest of a loaded run -> its outcome"""
    try:
        tr.curriculum_training()
        return outcome(tr)
    finally:
        close(tr)
