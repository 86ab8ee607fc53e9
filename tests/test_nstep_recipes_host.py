"""Per-recipe n-step targets without a GPU: what `Recipe` refuses before the library is touched, the bindings, the wrapper's plumbing, the recipes file's
"nstep" key and the flag conflict of scripts/ensemble_training.py that stays."""
import ctypes as C
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib
from dql_multirotor_landing_amd.config import F32, training_config
from dql_multirotor_landing_amd.ensemble import NSTEP_MAX, Recipe, SequentialEnsemble

ROOT = Path(__file__).resolve().parent.parent


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def bare_ensemble(lib, n=8):
    ens = object.__new__(SequentialEnsemble)
    ens.n, ens.lib, ens._h, ens.cfg = n, lib, None, training_config(0, dtype=F32)
    return ens


@pytest.mark.parametrize("nstep", [17, -1])
def test_a_recipe_with_n_outside_0_to_16_is_refused_before_the_library_is_touched(nstep):
    assert NSTEP_MAX == 16
    bad = Recipe(nstep=nstep)
    with pytest.raises(ValueError, match="nstep must be in 0..16"):
        bad.checked(training_config(0, dtype=F32))
    ens = bare_ensemble(Untouchable())
    with pytest.raises(ValueError, match="nstep must be in 0..16"):
        ens.set_recipes([Recipe(), bad], np.zeros(8, np.int32))
    ens._h = None  # (nothing to close)


def test_the_field_is_the_last_one_defaults_to_0_and_counts_in_equality():
    import dataclasses
    assert [f.name for f in dataclasses.fields(Recipe)][-1] == "nstep" and Recipe().nstep == 0
    assert Recipe(nstep=4) != Recipe() and Recipe(nstep=4) == Recipe(nstep=4)
    assert len(Recipe(nstep=16).checked(training_config(0, dtype=F32))) == 4  # checked() keeps returning its four values


def test_set_nstep_on_a_recipe_ensemble_stays_refused_before_the_library_is_touched():
    ens = bare_ensemble(Untouchable())
    ens._recipes, ens._advance_every, ens._nstep = [Recipe(nstep=4)], 32, 0
    with pytest.raises(ValueError, match="plain mode"):
        ens.set_nstep(2)
    ens._h = None


class FakeLib:
    """the recipe calls as the library answers them, for the wrapper's plumbing"""
    def __init__(self, n):
        self.n, self.nstep, self.calls = n, {}, []

    def dql_ensemble_set_recipes(self, h, n_recipes, of):
        self.nstep = {r: 0 for r in range(n_recipes)}  # fresh recipes have n = 0
        return 0

    def dql_ensemble_set_recipe(self, *a):
        return 0

    def dql_ensemble_set_recipe_level_schedules(self, *a):
        return 0

    def dql_ensemble_set_recipe_nstep(self, h, r, n):
        self.calls.append((r, n)); self.nstep[r] = n
        return 0

    def dql_ensemble_get_recipe_nstep(self, h, r, out):
        out._obj.value = self.nstep[r]
        return 0

    def dql_ensemble_get_recipes(self, h, of):
        C.memmove(of, np.zeros(self.n, np.int32).ctypes.data, 4 * self.n)
        return 0


def test_set_recipes_passes_each_n_and_recipes_returns_it():
    ens = bare_ensemble(FakeLib(8))
    ens._h = C.c_void_p(1)
    recipes = [Recipe(nstep=3), Recipe(), Recipe(nstep=16)]
    ens.set_recipes(recipes, np.arange(8) % 3)
    assert ens.lib.calls == [(0, 3), (2, 16)]  # n = 0 is what a fresh recipe has
    got, of = ens.recipes()
    assert got == recipes and [r.nstep for r in got] == [3, 0, 16]
    ens.lib.nstep[1] = 5  # what the library holds is what is returned
    assert [r.nstep for r in ens.recipes()[0]] == [3, 5, 16]
    ens._h = None


def test_the_new_symbols_are_bound():
    for name in ("dql_ensemble_set_recipe_nstep", "dql_ensemble_get_recipe_nstep"):
        assert name in _lib.SYMBOLS
    header = (ROOT / "include" / "dql.h").read_text()
    assert "int dql_ensemble_set_recipe_nstep(dql_ensemble* ens, int32_t recipe, int32_t n);" in header
    assert "int dql_ensemble_get_recipe_nstep(dql_ensemble* ens, int32_t recipe, int32_t* n);" in header
    assert "#define DQL_ABI_VERSION 6 " in header
    import __graft_entry__ as g
    g.build_hip()
    lib = _lib.load()
    n = C.c_int32()
    # a null ensemble: no device call
    assert lib.dql_ensemble_set_recipe_nstep(None, 0, 1) == _lib.EINVAL and lib.dql_ensemble_get_recipe_nstep(None, 0, C.byref(n)) == _lib.EINVAL


def load_script():
    spec = importlib.util.spec_from_file_location("ensemble_training_script", ROOT / "scripts" / "ensemble_training.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_a_recipes_file_with_nstep_loads(tmp_path):
    f = tmp_path / "r.json"
    f.write_text(json.dumps(["paper", {"preset": "paper", "name": "paper n = 8", "nstep": 8}, {"nstep": 16}]))
    names, recipes = load_script().load_recipes(f, 100)
    assert names == ["paper", "paper n = 8", "recipe 2"] and [r.nstep for r in recipes] == [0, 8, 16]
    assert recipes[1].quirks == recipes[0].quirks and recipes[1] != recipes[0]
    for r in recipes:
        r.checked(training_config(0, dtype=F32))
    f.write_text(json.dumps([{"nstep": 17}]))
    with pytest.raises(ValueError, match="nstep must be in 0..16"):
        load_script().load_recipes(f, 100)[1][0].checked(training_config(0, dtype=F32))


def test_nstep_with_recipes_is_still_refused_and_the_help_names_the_files_key(tmp_path):
    script = str(ROOT / "scripts" / "ensemble_training.py")
    r = subprocess.run([sys.executable, script, "--learners", "4", "--out", str(tmp_path / "x.npz"), "--nstep", "4", "--recipes", "r.json"], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot be combined" in r.stderr and not (tmp_path / "x.npz").exists(), r.stderr[-2000:]
    h = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and '"nstep"' in " ".join(h.stdout.split())
