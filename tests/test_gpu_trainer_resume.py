"""Resume == uninterrupted on the HIP engine, in float32 (the dtype the curriculum leg flies), at the three kinds of checkpoint that used to
give another run: between two levels, inside a level after a restart, inside a level that is learnt again after a step back.

The harness and the scenarios are those of test_trainer_resume.py (tests/trainer_resume_checks.py).  Per scenario the uninterrupted HIP
run is flown once and held to the oracle engine's run of the same keywords — history, tables, counters, period index — so the
checkpoint classes found on the CPU are the ones interrupted here; every resumed HIP run is then held to the uninterrupted HIP run.
Every Trainer's engine is closed in a `finally` (the harness's record / interrupt_after / finish)."""
import warnings

import pytest

import trainer_resume_checks as H
from dql_multirotor_landing_amd.config import F32
from test_dist_gloo import _oracle_engine_class

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uninterrupted(tmp_path_factory):
    """name -> (outcome of the HIP run, its checkpoint rows): flown once per scenario, held to the oracle engine's run, shared, left unchanged"""
    import dql_multirotor_landing_amd.trainer as T
    flown = {}
    def get(name):
        if name not in flown:
            with H.scenario(T, name, dtype=F32) as (make, _):
                hip, rows = H.record(make, tmp_path_factory.mktemp(f"hip_{name}"))
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(T, "Engine", _oracle_engine_class())
                with H.scenario(T, name, dtype=F32) as (make, _):
                    orc, rows_orc = H.record(make, tmp_path_factory.mktemp(f"orc_{name}"))
            H.assert_same_run(hip, orc)
            assert [H.checkpoint_class(r) for r in rows] == [H.checkpoint_class(r) for r in rows_orc]
            flown[name] = (hip, rows)
        return flown[name]
    return get


@pytest.mark.parametrize("name,cls", [("P", ("between", 1, False, 0, False)),    # between levels 0 and 1
                                      ("B", ("mid", 2, True, 0, False)),         # inside level 2 after a restart
                                      ("B", ("mid", 1, False, 1, True))])        # inside level 1 while it is learnt again after a step back
def test_hip_run_resumes_as_the_uninterrupted_hip_run(uninterrupted, tmp_path, name, cls):
    import dql_multirotor_landing_amd.trainer as T
    full, rows = uninterrupted(name)
    if name == "B":
        assert full["history"][2]["step_backs"] == 2
    ordinal = H.first_of_each_class(rows)[cls]
    with H.scenario(T, name, dtype=F32) as (make, load), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # (the trainer's category) a complete checkpoint resumes without a word
        back = H.resume_from(make, tmp_path, ordinal, load)
    H.assert_same_run(full, back)
