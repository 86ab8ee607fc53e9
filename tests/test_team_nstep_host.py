"""Team n-step targets without a GPU: what `SequentialEnsemble` refuses before the library is touched, the bindings, the shape of `team_pending_lengths`, the
plumbing of `curriculum(team_nstep=)`, and the flag conflicts of scripts/ensemble_training.py."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ensemble
from dql_multirotor_landing_amd.config import F32, training_config
from dql_multirotor_landing_amd.ensemble import NSTEP_MAX, Recipe, SequentialEnsemble

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture
def no_library(monkeypatch):
    """any touch of the library fails the test"""
    def load():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("n", [-1, 17, 1 << 20])
def test_n_outside_0_to_16_is_refused_at_construction(no_library, n):
    assert NSTEP_MAX == 16
    with pytest.raises(ValueError, match="team_nstep must be in 0..16"):
        SequentialEnsemble(training_config(0, dtype=F32), 4, envs_per_learner=8, team_nstep=n)


def test_a_plain_ensemble_is_refused_at_construction(no_library):
    with pytest.raises(ValueError, match="made through the team kernel"):
        SequentialEnsemble(training_config(0, dtype=F32), 4, team_nstep=2)
    with pytest.raises(ValueError, match="made through the team kernel"):
        SequentialEnsemble(training_config(0, dtype=F32), 4, envs_per_learner=1, teams=False, team_nstep=2)


def test_nstep_on_a_team_ensemble_still_raises(no_library):
    with pytest.raises(ValueError, match="plain mode"):
        SequentialEnsemble(training_config(0, dtype=F32), 4, envs_per_learner=2, nstep=2)
    with pytest.raises(ValueError, match="plain mode"):
        SequentialEnsemble(training_config(0, dtype=F32), 4, envs_per_learner=2, nstep=2, team_nstep=2)


class Standin:
    """stands for an ensemble: every attribute but the ones the argument checks read is a touch of the library"""
    envs_per_learner, teams, n, n_envs = 8, True, 4, 32
    _check_team_nstep = staticmethod(SequentialEnsemble._check_team_nstep)  # the argument check itself: no state, no library

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getattr__(self, name):
        if name in ("_nstep", "_advance_every", "_recipes", "_team_nstep"):
            raise AttributeError(name)
        raise AssertionError(f"the ensemble's {name} was used")


def test_set_team_nstep_refuses_before_the_library_is_touched(no_library):
    for bad in (-1, 17):
        with pytest.raises(ValueError, match="team_nstep must be in 0..16"):
            SequentialEnsemble.set_team_nstep(Standin(), bad)
    for n in (0, 2):  # an ensemble not made through the team kernel: any n, as the library says
        with pytest.raises(ValueError, match="made through the team kernel"):
            SequentialEnsemble.set_team_nstep(Standin(envs_per_learner=1, teams=False, n_envs=4), n)


class FakeLib:
    """dql_ensemble_set_team_nstep / _get_team_nstep as the library answers them, for the wrapper's plumbing"""
    def __init__(self, lengths):
        self.n, self.lengths, self.calls = 0, np.asarray(lengths, np.int32), []

    def dql_ensemble_set_team_nstep(self, h, n):
        self.calls.append(("set", n)); self.n = n
        return 0

    def dql_ensemble_get_team_nstep(self, h, n, out):
        self.calls.append(("get", out is not None))
        n._obj.value = self.n
        if out is not None:
            C.memmove(out, self.lengths.ctypes.data, self.lengths.nbytes)
        return 0


def test_team_nstep_and_the_per_learner_modes_refuse_each_other_before_the_library_is_touched(no_library):
    """a team ensemble of one env per learner can enter curriculum mode and take recipes: those fly the one-step learners, so they and team_nstep >= 1 are refused"""
    one = dict(envs_per_learner=1, teams=True, n_envs=4)
    for ens in (Standin(_advance_every=256, **one), Standin(_recipes=[Recipe()], **one)):
        with pytest.raises(ValueError, match="barrier mode"):
            SequentialEnsemble.set_team_nstep(ens, 2)
    with pytest.raises(ValueError, match="barrier mode"):
        SequentialEnsemble.set_curriculum(Standin(_team_nstep=3, **one), 4, 256)
    with pytest.raises(ValueError, match="barrier mode"):
        SequentialEnsemble.set_recipes(Standin(_team_nstep=3, **one), [Recipe()], [0] * 4)


def test_the_wrapper_passes_n_and_returns_one_int32_length_per_env():
    lengths = np.arange(32) % 16
    ens = Standin(lib=FakeLib(lengths), _h=C.c_void_p(1))
    SequentialEnsemble.set_team_nstep(ens, 16)
    assert ens.lib.calls == [("set", 16)] and ens._team_nstep == 16
    assert SequentialEnsemble.team_nstep.fget(ens) == 16
    got = SequentialEnsemble.team_pending_lengths(ens)
    assert got.shape == (32,) and got.dtype == np.int32 and got.tolist() == lengths.tolist()


def test_the_new_symbols_are_bound():
    for name in ("dql_ensemble_set_team_nstep", "dql_ensemble_get_team_nstep"):
        assert name in _lib.SYMBOLS
    header = (ROOT / "include" / "dql.h").read_text()
    assert "int dql_ensemble_set_team_nstep(" in header and "int dql_ensemble_get_team_nstep(" in header and "#define DQL_NSTEP_MAX 16" in header
    assert "#define DQL_ABI_VERSION 6 " in header
    import __graft_entry__ as g
    g.build_hip()
    lib = _lib.load()
    n = C.c_int32()
    assert lib.dql_ensemble_set_team_nstep(None, 1) == _lib.EINVAL and b"nothing was changed" in lib.dql_last_error()  # a null ensemble: no device call
    assert lib.dql_ensemble_get_team_nstep(None, C.byref(n), None) == _lib.EINVAL


def test_the_curriculum_driver_sets_team_nstep_first():
    calls = []
    ens = Standin(set_team_nstep=lambda n: calls.append(n) or (_ for _ in ()).throw(RuntimeError("stop")))
    with pytest.raises(RuntimeError, match="stop"):
        ensemble.curriculum(ens, team_nstep=4)
    assert calls == [4]


@pytest.mark.parametrize("flags,message", [(["--team-nstep", "4", "--envs-per-learner", "8", "--nstep", "2"], "--team-nstep cannot be combined with --nstep"),
                                           (["--team-nstep", "4", "--per-learner"], "--team-nstep cannot be combined with --per-learner"),
                                           (["--team-nstep", "4", "--recipes", "r.json"], "--team-nstep cannot be combined with --recipes"),
                                           (["--team-nstep", "4"], "--team-nstep needs a team ensemble"),
                                           (["--team-nstep", "17", "--envs-per-learner", "8"], "--team-nstep must be in 0..16"),
                                           (["--team-nstep", "-1", "--envs-per-learner", "8"], "--team-nstep must be in 0..16")])
def test_the_script_refuses_flag_conflicts_before_anything_is_created(flags, message, tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "ensemble_training.py"), "--learners", "4", "--out", str(tmp_path / "x.npz"), *flags], capture_output=True, text=True)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "x.npz").exists()
