"""The host code of the sequential learners, pinned to the letter (tests/ensemble_host_checks.py): every refusal of the dql_ensemble_* / dql_diag_ensemble_*
calls with its return code and dql_last_error text, one bad argument per check, two where the order of two checks shows, and the refusals that depend on the
ensemble's state; and what dql_ensemble_run does between its launches in each of the six modes: where it cuts, when it ends early, what it counts, and a hash
of the learners after every call.  tests/golden/ensemble_host.json recorded both from the library before the learners' host code was folded onto one launch
path and one advancing run loop.  After every refused call rows_of asserts that nothing moved."""
import json

import pytest

import ensemble_host_checks as ehc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.loads((golden_dir / "ensemble_host.json").read_text())


@pytest.fixture(scope="module")
def states():
    """the ensembles the refused calls are made on, shared between the entry points (a refused call leaves them as they were)"""
    kept = {}
    yield kept
    ehc.close_all(kept)


def test_the_fixture_holds_the_tables_rows_and_no_others(recorded):
    assert sorted(recorded["refusals"]) == sorted(ehc.ENTRY_POINTS) and sorted(recorded["runs"]) == sorted(ehc.SCRIPT_IDS) and len(ehc.SCRIPT_IDS) == 8
    for entry in ehc.ENTRY_POINTS:
        assert sorted(recorded["refusals"][entry]) == sorted(ehc.CASES[entry]), entry
        assert all(rcode != 0 and text for rcode, text in recorded["refusals"][entry].values()), entry
    for entry in ("dql_ensemble_set_schedules", "dql_ensemble_set_level_schedules", "dql_ensemble_set_recipe_level_schedules", "dql_ensemble_set_recipe",
                  "dql_ensemble_set_curriculum", "dql_ensemble_set_recipes", "dql_ensemble_set_nstep"):
        assert sum(" + " in what for what in ehc.CASES[entry]) >= 2, f"{entry}: calls with two bad arguments"
    for (mode, _), name in zip(ehc.SCRIPTS, ehc.SCRIPT_IDS):
        ehc.assert_script_is_what_it_is_for(mode, recorded["runs"][name])


@pytest.mark.parametrize("entry", ehc.ENTRY_POINTS)
def test_every_refusal_is_the_recorded_one_to_the_letter(entry, recorded, states):
    got = ehc.rows_of(entry, states)
    for what, want in recorded["refusals"][entry].items():
        assert got[what] == want, f"{entry}, {what}: {got[what]!r}, recorded {want!r}"


@pytest.mark.parametrize("mode, dtype", ehc.SCRIPTS, ids=ehc.SCRIPT_IDS)
def test_every_run_call_leaves_what_was_recorded(mode, dtype, recorded):
    got, want = ehc.script_of(mode, dtype), recorded["runs"][ehc.SCRIPT_IDS[ehc.SCRIPTS.index((mode, dtype))]]
    for part in ("main", "finishing"):
        assert len(got[part]) == len(want[part])
        for i, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, f"{mode}, {part}, call {i} (run({w['run']})): {g!r}, recorded {w!r}"
