"""Team ensembles without a GPU: what `SequentialEnsemble` and the drivers refuse before the library is touched, the bindings, and the flag conflicts of
scripts/ensemble_training.py."""
import subprocess
import sys
from pathlib import Path

import pytest

from dql_multirotor_landing_amd import _lib, ensemble
from dql_multirotor_landing_amd.config import F32, training_config
from dql_multirotor_landing_amd.ensemble import Recipe, SequentialEnsemble, TEAM_SIZES, curriculum_per_learner, curriculum_recipes

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture
def no_library(monkeypatch):
    """any touch of the library fails the test"""
    def load():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("envs_per_learner", [0, -1, 3, 5, 48, 128])
def test_team_sizes_other_than_the_seven_are_refused(no_library, envs_per_learner):
    with pytest.raises(ValueError, match="envs_per_learner must be one of"):
        SequentialEnsemble(training_config(0, dtype=F32), 4, envs_per_learner=envs_per_learner)


def test_the_env_count_is_bounded_and_teams_cannot_be_switched_off(no_library):
    assert TEAM_SIZES == (1, 2, 4, 8, 16, 32, 64)
    with pytest.raises(ValueError, match="n_learners \\* envs_per_learner at most"):
        SequentialEnsemble(training_config(0, dtype=F32), ensemble.MAX_LEARNERS // 64 + 1, envs_per_learner=64)
    with pytest.raises(ValueError, match="needs the team kernel"):
        SequentialEnsemble(training_config(0, dtype=F32), 4, envs_per_learner=2, teams=False)
    for bad in (training_config(0, dtype=F32, two_axis=1), training_config(0, dtype=F32, trajectory=1)):
        with pytest.raises(ValueError, match="x-only"):
            SequentialEnsemble(bad, 4, envs_per_learner=8)


class Untouchable:
    """stands for an ensemble with teams of 8: every attribute but the ones the argument checks read is a touch of the library"""
    envs_per_learner, n, max_episodes = 8, 4, 10

    def __getattr__(self, name):
        raise AssertionError(f"the ensemble's {name} was used")


def test_per_learner_drivers_refuse_teams_before_the_library_is_touched(no_library):
    ens = Untouchable()
    for call in (lambda: curriculum_per_learner(ens), lambda: curriculum_recipes(ens, [Recipe()], [0] * 4),
                 lambda: SequentialEnsemble.set_curriculum(ens, 4, 256), lambda: SequentialEnsemble.set_recipes(ens, [Recipe()], [0] * 4)):
        with pytest.raises(ValueError, match="barrier mode only"):
            call()


def test_the_new_symbols_are_bound():
    for name in ("dql_ensemble_create_teams", "dql_ensemble_envs_per_learner"):
        assert name in _lib.SYMBOLS
    header = (ROOT / "include" / "dql.h").read_text()
    assert "int dql_ensemble_create_teams(" in header and "int dql_ensemble_envs_per_learner(" in header and "#define DQL_ABI_VERSION 6 " in header


@pytest.mark.parametrize("flags,message", [(["--envs-per-learner", "8", "--per-learner"], "cannot be combined"),
                                           (["--envs-per-learner", "64", "--recipes", "r.json"], "cannot be combined"),
                                           (["--envs-per-learner", "3"], "must be one of")])
def test_the_script_refuses_flag_conflicts_before_anything_is_created(flags, message, tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "ensemble_training.py"), "--learners", "4", "--out", str(tmp_path / "x.npz"), *flags], capture_output=True, text=True)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "x.npz").exists()
