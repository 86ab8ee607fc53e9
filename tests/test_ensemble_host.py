"""Host side of the sequential ensemble (CPU only, no GPU): argument checking of `SequentialEnsemble`, the loud failure without a device, the eps-threshold
table against `Trainer.exploration_rate`, and the promotion count derived from the reference's (100, 0.96)."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, ensemble
from dql_multirotor_landing_amd.config import F32, training_config
from dql_multirotor_landing_amd.trainer import Trainer


def test_eps_threshold_table_is_the_trainer_s_exploration_rate_through_eps_threshold():
    tab = ensemble.eps_threshold_table(0, 2101)
    assert tab.dtype == np.uint32 and tab.shape == (2101,)
    me = SimpleNamespace()
    for e in range(2101):
        eps = Trainer.exploration_rate(me, e, 0)
        want = 0 if not eps > 0.0 else min(int(math.ceil(eps * 16777216.0)), 16777216)  # csrc/dql_host_consts.hpp eps_threshold
        assert int(tab[e]) == want, e
    assert tab[0] == tab[800] == 1 << 24 and tab[801] < 1 << 24 and tab[2000] == tab[2100] == math.ceil(0.01 * (1 << 24))
    # the default table (2 001 entries) ends on the floor, so min(e, n - 1) continues it
    assert int(ensemble.eps_threshold_table(0)[-1]) == int(tab[2100])
    for level in (1, 2, 3, 4):
        assert ensemble.eps_threshold_table(level).tolist() == [0] and ensemble.exploration_rates(level).tolist() == [0.0]


def test_min_successes_of_the_reference_rule_is_97():
    assert ensemble.min_successes_for(100, 0.96) == 97
    assert ensemble.min_successes_for(4, 0.5) == 3 and ensemble.min_successes_for(1, 0.0) == 1
    with pytest.raises(ValueError):
        ensemble.min_successes_for(0, 0.96)
    with pytest.raises(ValueError):
        ensemble.min_successes_for(100, 1.0)


def test_arguments_are_checked_before_the_library_is_called():
    cfg = training_config(0, dtype=F32)
    for bad_cfg in (training_config(0, dtype=F32, two_axis=1), training_config(0, dtype=F32, trajectory=1)):
        with pytest.raises(ValueError, match="x-only"):
            ensemble.SequentialEnsemble(bad_cfg, 4)
    for n in (0, -1, ensemble.MAX_LEARNERS + 1):
        with pytest.raises(ValueError, match="n_learners"):
            ensemble.SequentialEnsemble(cfg, n)
    with pytest.raises(ValueError, match="log_capacity"):
        ensemble.SequentialEnsemble(cfg, 4, log_capacity=-1)


def test_no_cpu_fallback_without_gpu():
    lib = _lib.load()
    n = C.c_int(0)
    rc = lib.dql_device_count(C.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    cfg = training_config(0, dtype=F32)
    h = C.c_void_p()
    c = cfg.to_c()
    assert lib.dql_ensemble_create(C.byref(c), 0, 4, 1, 0, C.byref(h)) == _lib.EHIP and not h.value
    with pytest.raises(RuntimeError):
        ensemble.SequentialEnsemble(cfg, 4)
    # the argument errors come first, also without a device
    bad = training_config(0, dtype=F32, two_axis=1).to_c()
    assert lib.dql_ensemble_create(C.byref(bad), 0, 4, 1, 0, C.byref(h)) == _lib.EINVAL
    assert lib.dql_ensemble_run(None, 1) == _lib.EINVAL


def test_module_keeps_to_numpy_and_the_library():
    src = open(ensemble.__file__).read()
    assert "import torch" not in src and "from torch" not in src
