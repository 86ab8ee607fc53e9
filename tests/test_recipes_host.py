"""Host side of the per-learner recipes (CPU only, no GPU): the `Recipe` defaults are the reference's recipe, the presets of scripts/ensemble_training.py,
its round-robin deal, and the C calls' null-handle refusals."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ensemble, evaluation
from dql_multirotor_landing_amd.config import F32, Q_REFERENCE, training_config

ROOT = Path(__file__).resolve().parent.parent


def script():
    spec = importlib.util.spec_from_file_location("ensemble_training", ROOT / "scripts" / "ensemble_training.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_default_recipe_is_the_reference_s():
    cfg = training_config(0, dtype=F32)
    r = ensemble.Recipe()
    alpha, alpha_min, ratios, lv = r.checked(cfg)
    assert r.quirks == Q_REFERENCE == 0x7F and r.transfer_order == ensemble.ORDER_REFERENCE and r.last_level == 4 and r.advance_exhausted
    assert np.array_equal(alpha, cfg.alpha_table()) and alpha_min == cfg.alpha_min and tuple(ratios) == ensemble.REFERENCE_RATIOS
    for k, (e, window, ms, me) in enumerate(lv):
        assert np.array_equal(e, ensemble.exploration_rates(k)) and (window, ms, me) == (100, 97, 50000)


def test_script_presets_and_round_robin_deal(tmp_path):
    m = script()
    assert m.preset_recipe("reference", 123) == ensemble.Recipe(levels=tuple(ensemble.LevelSchedule(max_episodes=123) for _ in range(5)))
    p = m.preset_recipe("paper", 123)
    assert p.quirks == evaluation.Q_PAPER == 0x40 and p.transfer_order == ensemble.ORDER_PAPER
    f = tmp_path / "recipes.json"
    f.write_text(json.dumps(["reference", "paper", {"preset": "paper", "quirks": 127, "levels": {"1": {"eps": [0.1] * 3 + [0.0], "window": 10}}}]))
    names, recipes = m.load_recipes(f, 77)
    assert names == ["reference", "paper", "recipe 2"] and len(recipes) == 3
    assert recipes[2].quirks == 0x7F and recipes[2].transfer_order == ensemble.ORDER_PAPER
    assert recipes[2].levels[1] == ensemble.LevelSchedule(eps=[0.1, 0.1, 0.1, 0.0], window=10, max_episodes=77) and recipes[2].levels[0] == ensemble.LevelSchedule(max_episodes=77)
    assert m.deal(7, 3).tolist() == [0, 1, 2, 0, 1, 2, 0]
    for bad in ('"reference"', '[]', '[{"preset": "nobody"}]', '[{"colour": 1}]', json.dumps(["reference"] * 65)):
        f.write_text(bad)
        with pytest.raises(ValueError):
            m.load_recipes(f, 77)


def test_null_handles_are_refused():
    lib = _lib.load()
    assert lib.dql_ensemble_set_recipes(None, 0, None) == _lib.EINVAL
    assert lib.dql_ensemble_set_recipe(None, 0, 0x7F, None, 0, 0.0, None, 4, 1, 0) == _lib.EINVAL
    assert lib.dql_ensemble_set_recipe_level_schedules(None, 0, 0, None, 0, 1, 1, 1) == _lib.EINVAL
    assert lib.dql_ensemble_get_recipes(None, None) == _lib.EINVAL
