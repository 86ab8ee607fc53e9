"""n-step targets without a GPU: what `SequentialEnsemble` refuses before the library is touched, the bindings, the shape of `pending_lengths`, and the flag
conflicts of scripts/ensemble_training.py."""
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


@pytest.mark.parametrize("nstep", [-1, 17, 1 << 20])
def test_n_outside_0_to_16_is_refused(no_library, nstep):
    assert NSTEP_MAX == 16
    with pytest.raises(ValueError, match="nstep must be in 0..16"):
        SequentialEnsemble(training_config(0, dtype=F32), 4, nstep=nstep)


def test_teams_are_refused_at_construction(no_library):
    for kw in (dict(envs_per_learner=2), dict(envs_per_learner=1, teams=True)):
        with pytest.raises(ValueError, match="plain mode"):
            SequentialEnsemble(training_config(0, dtype=F32), 4, nstep=2, **kw)


class Standin:
    """stands for a plain ensemble: every attribute but the ones the argument checks read is a touch of the library"""
    envs_per_learner, teams, n = 1, False, 4
    _check_nstep = staticmethod(SequentialEnsemble._check_nstep)  # the argument check itself: no state, no library

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getattr__(self, name):
        if name in ("_nstep", "_advance_every", "_recipes"):
            raise AttributeError(name)
        raise AssertionError(f"the ensemble's {name} was used")


def test_set_nstep_refuses_before_the_library_is_touched(no_library):
    for bad in (-1, 17):
        with pytest.raises(ValueError, match="nstep must be in 0..16"):
            SequentialEnsemble.set_nstep(Standin(), bad)
    for ens in (Standin(envs_per_learner=8, teams=True), Standin(teams=True), Standin(_advance_every=256), Standin(_recipes=[Recipe()])):
        with pytest.raises(ValueError, match="plain mode"):
            SequentialEnsemble.set_nstep(ens, 2)


def test_curriculum_mode_and_recipes_are_refused_while_n_is_set(no_library):
    ens = Standin(_nstep=3)
    with pytest.raises(ValueError, match="plain mode"):
        SequentialEnsemble.set_curriculum(ens, 4, 256)
    with pytest.raises(ValueError, match="plain mode"):
        SequentialEnsemble.set_recipes(ens, [Recipe()], [0] * 4)


class FakeLib:
    """dql_ensemble_set_nstep / _get_nstep as the library answers them, for the wrapper's plumbing"""
    def __init__(self, lengths):
        self.n, self.lengths, self.calls = 0, np.asarray(lengths, np.int32), []

    def dql_ensemble_set_nstep(self, h, n):
        self.calls.append(("set", n)); self.n = n
        return 0

    def dql_ensemble_get_nstep(self, h, n, out):
        self.calls.append(("get", out is not None))
        n._obj.value = self.n
        if out is not None:
            C.memmove(out, self.lengths.ctypes.data, self.lengths.nbytes)
        return 0


def test_the_wrapper_passes_n_and_returns_one_int32_length_per_learner():
    ens = Standin(lib=FakeLib([0, 3, 15, 1]), _h=C.c_void_p(1), _nstep=0, _advance_every=0)
    SequentialEnsemble.set_nstep(ens, 16)
    assert ens.lib.calls == [("set", 16)] and ens._nstep == 16
    assert SequentialEnsemble.nstep.fget(ens) == 16
    got = SequentialEnsemble.pending_lengths(ens)
    assert got.shape == (4,) and got.dtype == np.int32 and got.tolist() == [0, 3, 15, 1]


def test_the_new_symbols_are_bound():
    for name in ("dql_ensemble_set_nstep", "dql_ensemble_get_nstep"):
        assert name in _lib.SYMBOLS
    header = (ROOT / "include" / "dql.h").read_text()
    assert "int dql_ensemble_set_nstep(" in header and "int dql_ensemble_get_nstep(" in header and "#define DQL_NSTEP_MAX 16" in header
    assert "#define DQL_ABI_VERSION 6 " in header
    import __graft_entry__ as g
    g.build_hip()
    lib = _lib.load()
    assert lib.dql_ensemble_set_nstep is not None and lib.dql_ensemble_get_nstep is not None
    n = C.c_int32()
    assert lib.dql_ensemble_set_nstep(None, 1) == _lib.EINVAL and lib.dql_ensemble_get_nstep(None, C.byref(n), None) == _lib.EINVAL  # a null ensemble: no device call


def test_the_curriculum_driver_sets_n_first():
    calls = []
    ens = Standin(set_nstep=lambda n: calls.append(n) or (_ for _ in ()).throw(RuntimeError("stop")))
    with pytest.raises(RuntimeError, match="stop"):
        ensemble.curriculum(ens, nstep=4)
    assert calls == [4]


@pytest.mark.parametrize("flags,message", [(["--nstep", "4", "--per-learner"], "cannot be combined"),
                                           (["--nstep", "4", "--recipes", "r.json"], "cannot be combined"),
                                           (["--nstep", "16", "--envs-per-learner", "8"], "cannot be combined"),
                                           (["--nstep", "17"], "must be in 0..16"), (["--nstep", "-1"], "must be in 0..16")])
def test_the_script_refuses_flag_conflicts_before_anything_is_created(flags, message, tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "ensemble_training.py"), "--learners", "4", "--out", str(tmp_path / "x.npz"), *flags], capture_output=True, text=True)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "x.npz").exists()
