"""Host side of the roll-out operator (CPU only, no GPU): `evaluation.episode_report` on hand-made records, the argument errors of `ops.rollout` (raised
before the library is called) and the histogram keys of `rollout_outcomes` against those of `first_episode_outcomes`."""
import numpy as np
import pytest

from dql_multirotor_landing_amd import _lib, evaluation, ops
from dql_multirotor_landing_amd.config import CHECK_NAMES, F32, Q_PAPER, simulation_config

CONTACT, FLY_X, MIN_ALT = (CHECK_NAMES.index(n) for n in ("TERMINAL_CONTACT", "TERMINAL_FLYZONE_X", "TERMINAL_MINIMUM_ALTITUDE"))


def handmade_records(seed=3, n=200):
    """two table sets: set 0 with contacts, fly-zone exits, ground hits and unfinished envs; set 1 without a single contact"""
    rng = np.random.default_rng(seed)
    code = np.stack([rng.choice([CONTACT, CONTACT, FLY_X, MIN_ALT, -1], size=n), rng.choice([FLY_X, MIN_ALT], size=n)]).astype(np.int32)
    rec = {"code": code, "steps": rng.integers(1, 400, size=(2, n)).astype(np.int32)}
    for f in ops.ROLLOUT_RECORD_FIELDS:
        rec[f] = rng.normal(size=(2, n))
    return rec


def test_episode_report_quantiles_and_contact_only_selection():
    rec = handmade_records()
    rep = evaluation.episode_report(rec)
    assert len(rep) == 2
    code = rec["code"][0]
    fin, td = code >= 0, code == CONTACT
    assert 0 < td.sum() < fin.sum() < code.size  # the case has contacts, other endings and unfinished envs
    r = rep[0]
    assert r["histogram"]["TERMINAL_CONTACT"] == td.sum() and r["histogram"]["unfinished"] == (~fin).sum()
    assert set(r["histogram"]) == set(CHECK_NAMES) | {"unfinished"} and sum(r["histogram"].values()) == code.size
    q = (0.05, 0.5, 0.95)
    keys = ("q05", "q50", "q95")
    want = {
        "steps": np.quantile(rec["steps"][0][fin].astype(np.float64), q),
        "return": np.quantile((rec["cum_x"][0] + rec["cum_y"][0])[fin], q),
    }
    for name, w in want.items():
        assert [r[name][k] for k in keys] == list(w), name
    t = r["touchdown"]
    assert t["n"] == td.sum()
    offset = np.hypot(rec["px"][0] - rec["mp_x"][0], rec["py"][0] - rec["mp_y"][0])
    speed = np.hypot(rec["vx"][0] - rec["mp_u"][0], rec["vy"][0] - rec["mp_v"][0])
    sink = -rec["vz"][0]
    for name, x in (("offset", offset), ("rel_speed", speed), ("sink_rate", sink)):
        assert [t[name][k] for k in keys] == list(np.quantile(x[td], q)), name
        assert [t[name][k] for k in keys] != list(np.quantile(x[fin], q)), f"{name}: the selection must be the contact episodes only"


def test_episode_report_without_a_contact_gives_none():
    rep = evaluation.episode_report(handmade_records())
    assert rep[1]["touchdown"] is None and rep[1]["histogram"]["TERMINAL_CONTACT"] == 0
    assert rep[1]["steps"] is not None and rep[1]["return"] is not None
    # nothing finished at all: every quantile block is None, no exception
    rec = handmade_records()
    rec["code"][:] = -1
    for r in evaluation.episode_report(rec):
        assert r["touchdown"] is None and r["steps"] is None and r["return"] is None and r["histogram"]["unfinished"] == rec["code"].shape[1]
    # one table set given as 1-D arrays
    one = {k: v[0] for k, v in handmade_records().items()}
    assert evaluation.episode_report(one) == evaluation.episode_report(handmade_records())[:1]


def test_rollout_argument_errors_are_raised_before_the_library_is_called(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded for a call whose arguments are wrong")
    monkeypatch.setattr(_lib, "load", no_library)
    cfg = simulation_config(dtype=F32, quirks=Q_PAPER)
    t = (np.zeros(2835), np.zeros(2835))
    bad = [
        dict(tables=[], envs_per_table=64),                      # no table set
        dict(tables=[t] * 17, envs_per_table=64),                # more than 16
        dict(tables=(np.zeros(10), np.zeros(2835)), envs_per_table=64),
        dict(tables=[(np.zeros(2835),)], envs_per_table=64),
        dict(tables=t, envs_per_table=0), dict(tables=t, envs_per_table=-64), dict(tables=t, envs_per_table=100),
        dict(tables=t, envs_per_table=64, max_steps=0), dict(tables=t, envs_per_table=64, max_steps=4097),
        dict(tables=t, envs_per_table=64, trace_envs=-1), dict(tables=t, envs_per_table=64, trace_envs=65),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.rollout(cfg, kw.pop("tables"), kw.pop("envs_per_table"), 123, **kw)
    with pytest.raises(AssertionError):  # (a well-formed call does reach the library)
        ops.rollout(cfg, t, 64, 123)
    with pytest.raises(ValueError):
        evaluation.first_episode_outcomes(t + (np.zeros(2835),), 64, method="sideways")


def test_rollout_outcomes_has_the_histogram_keys_of_first_episode_outcomes(monkeypatch):
    """both harnesses on stand-ins for the device (a stub Engine, a stub ops.rollout) that end every episode the same way: the same dict, key for key"""
    n = 128
    codes = np.resize(np.array([CONTACT, FLY_X, MIN_ALT, -1], np.int32), n)

    class StubEngine:
        def __init__(self, cfg, n_envs, seed=0, device=0):
            assert n_envs == n
            self.k = 0
        def set_tables(self, *a): pass
        def eval_steps(self, k): self.k += k
        def dones(self):  # every env that finishes does so at the third period after the reset period
            d = ((codes >= 0) & (self.k == 4)).astype(np.uint8)
            return d, np.where(d != 0, codes, 8).astype(np.int8)
        def close(self): pass

    def stub_rollout(cfg, tables, envs_per_table, seed, max_steps=600, trace_envs=0, device=0, timing=None):
        assert envs_per_table == n and len(tables) == 1
        return {"code": codes[None, :].copy()}

    monkeypatch.setattr(evaluation, "Engine", StubEngine)
    monkeypatch.setattr(ops, "rollout", stub_rollout)
    t = (np.zeros(2835), np.zeros(2835), np.zeros(2835))
    for flavour in ("simulation", "training"):
        a = evaluation.first_episode_outcomes(t, n, 4, max_steps=10, flavour=flavour, quirks=Q_PAPER)
        b = evaluation.rollout_outcomes(t, n, 4, max_steps=10, flavour=flavour, quirks=Q_PAPER)
        c = evaluation.first_episode_outcomes(t, n, 4, max_steps=10, flavour=flavour, quirks=Q_PAPER, method="rollout")
        assert list(a) == list(b) == list(c) == list(CHECK_NAMES) + ["unfinished"]
        assert a == b == c and a["unfinished"] == n // 4 and a["TERMINAL_CONTACT"] == n // 4
