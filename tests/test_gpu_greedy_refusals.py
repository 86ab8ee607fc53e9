"""Every refusal of the greedy-flight family, pinned to the letter: the 11 entry points (dql_rollout, dql_score, dql_score_map, dql_model, dql_returns,
dql_score_grid and the five dql_ensemble_* twins) answer each refused call of tests/greedy_refusal_checks.py with the return code and the dql_last_error text
that tests/golden/greedy_refusals.json recorded from the library before the family's host code was folded onto shared helpers.  One bad argument per check, and
calls with two bad arguments whose answer shows which check comes first.  No call here is meant to reach the device: every row is refused on the host, the
sentinel-filled outputs stay untouched and the operator's dql_diag_*_last answer stays what one small valid call left (asserted row by row in rows_of)."""
import json

import pytest

import greedy_refusal_checks as grc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.loads((golden_dir / "greedy_refusals.json").read_text())


def test_the_fixture_holds_the_table_s_rows_and_no_others(recorded):
    assert sorted(recorded) == sorted(grc.ENTRY_POINTS) and len(grc.ENTRY_POINTS) == 11
    for entry in grc.ENTRY_POINTS:
        assert sorted(recorded[entry]) == sorted(grc.CASES[entry]), entry
        pairs = [what for what in grc.CASES[entry] if " + " in what]
        assert len(pairs) >= 3, f"{entry}: {len(pairs)} calls with two bad arguments"
        assert all(rcode != 0 and text for rcode, text in recorded[entry].values()), entry


@pytest.mark.parametrize("entry", grc.ENTRY_POINTS)
def test_every_refusal_is_the_recorded_one_to_the_letter(entry, recorded):
    got = grc.rows_of(entry)
    for what, want in recorded[entry].items():
        assert got[what] == want, f"{entry}, {what}: {got[what]!r}, recorded {want!r}"
