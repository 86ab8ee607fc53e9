"""Flushes that bootstrap, on the yardsticks alone (CPU only, no GPU, no device text): every row of tests/flush_bootstrap_checks.py meets its conditions and
its pinned counts, every mistake a body can make at such a flush (the mutants: the row of s' re-read per entry, the bootstrap dropped at a terminal, the
other coin's bootstrap taken for the value) changes the yardstick's tables on that row, and at n = 1 the n-step yardsticks equal the one-step reference loops
under the same config.  """
import pytest

from dql_multirotor_landing_amd.config import F32

import flush_bootstrap_checks as fb

L = 26  # the emulations' size


@pytest.mark.parametrize("learners", [L, 70], ids=["26-learners", "70-learners"])
@pytest.mark.parametrize("level,quirks,dtype,nstep", fb.PLAIN_ROWS, ids=fb.PLAIN_IDS)
def test_plain_rows_meet_their_conditions_on_the_yardstick(level, quirks, dtype, nstep, learners):
    fb.plain_reference(level, quirks, dtype, nstep, learners)


@pytest.mark.parametrize("level,quirks,dtype,nstep", fb.PLAIN_ROWS, ids=fb.PLAIN_IDS)
def test_every_mutant_changes_a_plain_row(level, quirks, dtype, nstep):
    for name in fb.applicable_mutants(quirks):
        cells = fb.plain_mutant_cells(level, quirks, dtype, nstep, L, name)
        print(f"mutant {name}: {cells} cells of qa and qb differ")
        assert cells >= 1, f"the mutant '{name}' flies this row exactly as the yardstick does: the row cannot catch that mistake"


@pytest.mark.parametrize("level,quirks,L_,E,nstep,dtype", fb.TEAM_ROWS, ids=fb.TEAM_IDS)
def test_team_rows_meet_their_conditions_on_the_yardstick(level, quirks, L_, E, nstep, dtype):
    fb.team_reference(level, quirks, L_, E, nstep, dtype)


@pytest.mark.parametrize("level,quirks,L_,E,nstep,dtype", fb.TEAM_ROWS, ids=fb.TEAM_IDS)
def test_every_mutant_changes_a_team_row(level, quirks, L_, E, nstep, dtype):
    for name in fb.applicable_mutants(quirks):
        cells = fb.team_mutant_cells(level, quirks, L_, E, nstep, dtype, name)
        print(f"mutant {name}: {cells} cells of qa and qb differ")
        assert cells >= 1, f"the mutant '{name}' flies this row exactly as the yardstick does: the row cannot catch that mistake"


def test_the_recipe_case_meets_its_conditions_on_the_yardsticks():
    fb.recipe_reference()


@pytest.mark.parametrize("r", [r for r, (q, n) in enumerate(fb.RECIPE_SPECS) if n >= 1 and q & fb.Q_POS_CHANGE])
def test_every_mutant_changes_its_recipes_members(r):
    for name in fb.applicable_mutants(fb.RECIPE_SPECS[r][0]):
        cells = fb.recipe_mutant_cells(r, name)
        print(f"recipe {r}, mutant {name}: {cells} cells of qa and qb differ")
        assert cells >= 1, f"recipe {r}: the mutant '{name}' flies exactly as the yardstick does"


def test_the_plain_yardstick_at_n_1_equals_the_one_step_reference_loop():
    """level 4 from trained tables under 0x50: terminal transitions with mask 1 and a non-zero bootstrap (asserted inside)"""
    _, mask_1 = fb.plain_anchor(fb.Q_POS_COIN, F32, L)
    assert mask_1 >= 20


def test_the_team_yardstick_at_n_1_equals_the_team_reference_loop():
    _, mask_1 = fb.team_anchor(fb.Q_POS_COIN, F32)
    assert mask_1 >= 20
