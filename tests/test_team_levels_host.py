"""Team curriculum mode, the Python side alone (no GPU, no library): `SequentialEnsemble.set_team_curriculum` and
`ensemble.curriculum_per_team` check every argument before the library is touched, and the per-learner drivers still refuse ensembles with more than one env
per learner with the sentences they always had."""
import numpy as np
import pytest

from dql_multirotor_landing_amd import ensemble
from dql_multirotor_landing_amd.config import F32, training_config
from dql_multirotor_landing_amd.ensemble import Recipe, SequentialEnsemble


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def fake(envs_per_learner=4, teams=True, n=8, **state):
    ens = object.__new__(SequentialEnsemble)
    ens.n, ens.lib, ens._h = n, Untouchable(), None
    ens.envs_per_learner, ens.n_envs, ens.teams = envs_per_learner, n * envs_per_learner, teams
    ens.cfg, ens.max_episodes = training_config(0, dtype=F32), 50
    ens._nstep, ens._advance_every, ens._team_nstep, ens._team_every = 0, 0, 0, 0
    ens.__dict__.update(state)
    return ens


GOOD = dict(last_level=4, advance_every=64, ratios=None, advance_exhausted=True, transfer_order=0)
BAD = [dict(advance_every=-1), dict(advance_every=4097), dict(last_level=5), dict(last_level=-1), dict(ratios=[1.0] * 4), dict(ratios=[1.0, np.nan, 1.0, 1.0, 1.0]),
       dict(ratios=[1.0, 1.0, np.inf, 1.0, 1.0]), dict(transfer_order=2), dict(transfer_order=-1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}" for k in b))
def test_set_team_curriculum_checks_its_arguments_first(bad):
    with pytest.raises(ValueError):
        fake().set_team_curriculum(**{**GOOD, **bad})


def test_set_team_curriculum_is_for_team_ensembles_and_one_mode_at_a_time():
    with pytest.raises(ValueError, match="made through the team kernel"):
        fake(envs_per_learner=1, teams=False).set_team_curriculum(**GOOD)
    with pytest.raises(ValueError, match="refuse each other"):
        fake(envs_per_learner=1, _advance_every=64).set_team_curriculum(**GOOD)
    with pytest.raises(ValueError, match="refuse each other"):
        fake(envs_per_learner=1, _recipes=[Recipe()]).set_team_curriculum(**GOOD)
    # ... and the other way round, on an ensemble whose team curriculum mode is on
    on = fake(envs_per_learner=1, _team_every=64)
    with pytest.raises(ValueError, match="refuse each other"):
        on.set_curriculum(4, 64)
    with pytest.raises(ValueError, match="refuse each other"):
        on.set_recipes([Recipe()], np.zeros(on.n, np.int32))


@pytest.mark.parametrize("bad", BAD + [dict(advance_every=0), dict(window=0), dict(window=129), dict(max_episodes=0), dict(success_rate=1.0), dict(chunk_periods=0),
                                        dict(max_periods=-1), dict(team_nstep=17), dict(team_nstep=-1)], ids=lambda b: "-".join(f"{k}" for k in b))
def test_curriculum_per_team_checks_its_arguments_first(bad):
    with pytest.raises(ValueError):
        ensemble.curriculum_per_team(fake(), **{**GOOD, "window": 4, "success_rate": 0.5, **bad})


def test_curriculum_per_team_is_for_team_ensembles():
    with pytest.raises(ValueError, match="made through the team kernel"):
        ensemble.curriculum_per_team(fake(envs_per_learner=1, teams=False))


def test_the_per_learner_drivers_still_refuse_teams_with_their_sentences():
    for call in (lambda e: ensemble.curriculum_per_learner(e), lambda e: ensemble.curriculum_recipes(e, [Recipe()], np.zeros(e.n, np.int32)),
                 lambda e: e.set_curriculum(4, 64), lambda e: e.set_recipes([Recipe()], np.zeros(e.n, np.int32))):
        with pytest.raises(ValueError, match="barrier mode only") as err:
            call(fake())
        assert str(err.value) == ensemble.TEAMS_BARRIER_ONLY
        with pytest.raises(ValueError, match="barrier mode only"):  # whether or not its team curriculum mode is on
            call(fake(_team_every=64))
    assert "teams have no per-learner curriculum and no recipes" in ensemble.TEAMS_BARRIER_ONLY
