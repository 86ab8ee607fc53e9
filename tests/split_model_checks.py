"""Shared by the split transition-model tests (CPU emulation and GPU): the stepwise yardstick of `dql_model_split` / `dql_ensemble_model_split` (include/dql.h).

ONE `Oracle` per case stepped with EXTERNAL actions exactly as `model_checks.stepwise_model` steps it (same cases, seed, eps rule and counting rule, imported from
there), but every feature's field is read BEFORE each step and recorded per counted decision, so that one oracle flight per case serves all eleven features and
any cut: `expected(case, feature, cut)` only sorts the recorded decisions into halves.  It knows nothing of the kernel.  `flight(case)` asserts on the recorded
decisions, before anything is compared, that what the cases are there for occurred (occurrence, not counts)."""
import numpy as np

from dql_multirotor_landing_amd.config import F32, N_CELLS, TARGET_FRAC_BITS
from oracle import oracle as orc
from oracle.oracle import Oracle

import ensemble_checks as ec
import model_checks as mc

N_STATES, N_CODES, N_COLS, SEED = mc.N_STATES, mc.N_CODES, mc.N_COLS, mc.SEED
CASE_IDS = ("A", "B64", "C", "D")
FRAC_BITS = 20
# code -> name, as include/dql.h's DQL_SPLIT_*; the oracle's field of features 1 .. 8
FEATURES = ("coin", "obs_p_x", "obs_v_x", "obs_a_x", "pitch_sp", "mp_phase", "mp_u", "altitude", "v_z", "step", "prev_action")
REAL_FIELD = {1: "obs_p_x", 2: "obs_v_x", 3: "obs_a_x", 4: "pitch_sp", 5: "mp_phase", 6: "mp_u", 7: "pz", 8: "vz"}
COIN, STEP, PREV_ACTION = 0, 9, 10
FIELDS = ("pairs", "reward_fx", "terminal", "feat_sum_fx", "by_code", "steps_sum", "visits", "state_visits")
EQUAL_TO_CUT_FEATURE = 2  # obs_v_x: continuous, so a value equals its cut only where the cut was made from it


def coin(env_id, j, seed):
    """the coin of include/dql.h, vectorised over env ids: 0 or 1"""
    with np.errstate(over="ignore"):
        x = np.asarray(env_id, np.uint32) * np.uint32(0x9E3779B1) + np.uint32(j & 0xffffffff) * np.uint32(0x85EBCA77) + np.uint32(seed & 0xffffffff)
        x ^= x >> np.uint32(16); x *= np.uint32(0x85EBCA6B); x ^= x >> np.uint32(13); x *= np.uint32(0xC2B2AE35); x ^= x >> np.uint32(16)
    return (x >> np.uint32(31)).astype(np.float64)


def _features(o, names_r, names_i, j, seed):
    """[11][n] float64: every feature of every env as the oracle's envs stand now"""
    reals, ints = o.get_fields()
    v = np.zeros((len(FEATURES), o.n))
    v[COIN] = coin(np.arange(o.n), j, seed)
    for code, f in REAL_FIELD.items():
        v[code] = reals[names_r.index(f)]
    v[STEP] = ints[names_i.index("step_count")] & 0xffff
    v[PREV_ACTION] = ints[names_i.index("action")] & 3
    return v


def stepwise_decisions(cfg, tables, n, seed, eps, max_steps, episodes):
    """every counted decision of one table set flown by `n` envs, in period order: {"env", "j", "s", "act", "ns", "done", "code", "fx", "len" (the episode's length
    where done), "first" (the episode's first decision: the period before was a reset period), "value" [11][N] (before the period), "after" [11][N]}, and
    "by_code" / "steps_sum" of the flight"""
    qa, qb = (np.ascontiguousarray(t, np.float64).ravel() for t in tables)
    o = Oracle(cfg, n, seed=seed)
    rn, inn = o.field_names(False), o.field_names(True)
    i_rew = rn.index("reward")
    i_idx, i_fl, i_code, i_sc = (inn.index(f) for f in ("idx_x", "flags", "code", "step_count"))
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    thr = ec.eps_thr(eps)
    finished = np.zeros(n, np.int64)
    prev_reset = np.zeros(n, bool)
    ctr = np.zeros((n, 4), np.uint32); ctr[:, 2] = np.arange(n); ctr[:, 3] = mc.STREAM_ACTION
    rec = {k: [] for k in ("env", "j", "s", "act", "ns", "done", "code", "fx", "len", "first", "value", "after")}
    by_code = np.zeros(N_COLS, np.int64)
    for j in range(max_steps + 1):
        _, ints = o.get_fields()
        s = ints[i_idx].astype(np.int64); was_done = (ints[i_fl] & mc.FL_DONE) != 0
        before = _features(o, rn, inn, j, seed)
        ctr[:, 0] = j & 0xffffffff; ctr[:, 1] = (j >> 32) & 0xffffffff
        w = orc.philox_n(ctr, (k0, k1))
        explore = (w[:, 0] >> 8) < thr
        greedy = orc.agent_predict(qa, qb, np.where(was_done, 0, s)).astype(np.int64)
        act = np.where(explore, ((w[:, 1].astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int64), greedy)
        act[was_done] = 2  # a reset period takes no action
        o.step(act.astype(np.uint8))
        reals, ints = o.get_fields()
        after = _features(o, rn, inn, j, seed)
        flags = ints[i_fl]
        was_reset, done = (flags & mc.FL_WAS_RESET) != 0, (flags & mc.FL_DONE) != 0
        assert np.array_equal(was_reset, was_done), "a reset period is the period after a done one"
        counts = (finished < episodes) & ~was_reset
        ns, code = ints[i_idx].astype(np.int64), ints[i_code].astype(np.int64)
        fx = np.rint(reals[i_rew] * float(1 << TARGET_FRAC_BITS)).astype(np.int64)
        m = np.flatnonzero(counts)
        for k, a in (("env", m), ("j", np.full(m.size, j)), ("s", s[m]), ("act", act[m]), ("ns", ns[m]), ("done", done[m]), ("code", code[m]), ("fx", fx[m]),
                     ("len", ints[i_sc][m] & 0xffff), ("first", prev_reset[m]), ("value", before[:, m]), ("after", after[:, m])):
            rec[k].append(a)
        end = counts & done
        np.add.at(by_code, code[end], 1)
        finished[end] += 1
        prev_reset = was_reset
        if (finished >= episodes).all():
            break
    by_code[N_CODES] = n * episodes - int(finished.sum())
    out = {k: np.concatenate(v, axis=-1) for k, v in rec.items()}
    out["by_code"] = by_code
    out["steps_sum"] = int(out["len"][out["done"]].sum())
    out["n"] = n
    return out


def expected(d, feature, cut, strict=False):
    """the outputs of one table set for `feature` and `cut` ([945] or a scalar) from the recorded decisions `d`; strict: the WRONG rule `>` (to show that a case
    tells it from `>=`)"""
    cut = np.broadcast_to(np.asarray(cut, np.float64), (N_STATES,))
    v = d["value"][feature]
    at = cut[d["s"]]
    half = (v > at if strict else v >= at).astype(np.int64)
    cell = d["s"] * 3 + d["act"]
    go, end = ~d["done"], d["done"]
    pairs = np.zeros((2, N_CELLS, N_STATES), np.uint32); reward_fx = np.zeros((2, N_CELLS), np.int64); terminal = np.zeros((2, N_CELLS, N_CODES), np.int64)
    feat = np.zeros(N_STATES, np.int64)
    np.add.at(pairs, (half[go], cell[go], d["ns"][go]), 1)
    np.add.at(terminal, (half[end], cell[end], d["code"][end]), 1)
    np.add.at(reward_fx, (half, cell), d["fx"])
    scaled = v * float(1 << FRAC_BITS)
    assert np.isfinite(v).all() and (np.abs(v) < 8192.0).all()
    np.add.at(feat, d["s"], np.rint(scaled).astype(np.int64))
    visits = pairs.sum(axis=-1, dtype=np.int64) + terminal.sum(axis=-1)
    return {"pairs": pairs, "reward_fx": reward_fx, "terminal": terminal, "feat_sum_fx": feat, "by_code": d["by_code"], "steps_sum": d["steps_sum"], "visits": visits,
            "state_visits": visits.sum(axis=0).reshape(N_STATES, 3).sum(axis=-1), "half": half}


def mean_cut(d, feature):
    """the yardstick's own per-state means of a feature, computed as the caller of dql_model_split computes them: feat_sum_fx / 2^20 / visits; +inf where unvisited"""
    feat = np.zeros(N_STATES, np.int64); sv = np.zeros(N_STATES, np.int64)
    np.add.at(feat, d["s"], np.rint(d["value"][feature] * float(1 << FRAC_BITS)).astype(np.int64))
    np.add.at(sv, d["s"], 1)
    return np.where(sv > 0, feat.astype(np.float64) / float(1 << FRAC_BITS) / np.where(sv > 0, sv, 1), np.inf)


def cut_of(d, feature):
    """the cut a case is compared at: 0.5 for the coin, the yardstick's own means elsewhere"""
    return np.full(N_STATES, 0.5) if feature == COIN else mean_cut(d, feature)


def equal_to_cut(d, feature=EQUAL_TO_CUT_FEATURE):
    """a crafted cut: the feature's means, but in the most visited state the exact value of one recorded decision taken there (the median one), so that this
    decision has value == cut[state]: `>=` puts it in half 1, `>` in half 0"""
    cut = mean_cut(d, feature)
    s = int(np.bincount(d["s"], minlength=N_STATES).argmax())
    vals = np.sort(d["value"][feature][d["s"] == s])
    cut[s] = vals[len(vals) // 2]
    return cut


def same_pair_in_both_halves(d, half):
    """whether some wave (64 consecutive envs) in some period holds two lanes with the same (cell, s') in different halves"""
    go = ~d["done"]
    key = ((d["j"][go] * (d["n"] // 64 + 1) + d["env"][go] // 64) * N_CELLS + d["s"][go] * 3 + d["act"][go]) * N_STATES + d["ns"][go]
    h = half[go]
    return np.intersect1d(key[h == 0], key[h == 1]).size > 0


_FLIGHTS, _MODEL_SUM_CHECKED = {}, set()


def flight(case_id):
    """the case's recorded decisions, flown once and left unchanged; asserts ON THEM that the events the cases are there for occurred"""
    if case_id not in _FLIGHTS:
        cfg, tables, eps, n, max_steps, episodes = mc.case_args(case_id)
        d = stepwise_decisions(cfg, tables, n, SEED, eps, max_steps, episodes)
        assert d["env"].size > 0 and d["done"].any() and (~d["done"]).any()
        # both halves are used: for every feature at its cut, both halves hold decisions
        halves = {}
        for f in range(len(FEATURES)):
            halves[f] = expected(d, f, cut_of(d, f))["half"]
            assert (halves[f] == 0).any() and (halves[f] == 1).any(), f"case {case_id}: {FEATURES[f]} leaves a half empty at its cut"
        # a value equals its cut, and `>` for `>=` would change the result
        c = equal_to_cut(d)
        v = d["value"][EQUAL_TO_CUT_FEATURE]
        assert (v == c[d["s"]]).any(), f"case {case_id}: no decision sits on the crafted cut"
        assert not np.array_equal(expected(d, EQUAL_TO_CUT_FEATURE, c)["pairs"], expected(d, EQUAL_TO_CUT_FEATURE, c, strict=True)["pairs"]) or \
            not np.array_equal(expected(d, EQUAL_TO_CUT_FEATURE, c)["terminal"], expected(d, EQUAL_TO_CUT_FEATURE, c, strict=True)["terminal"])
        if case_id == "A":  # the merge must keep the half in the key
            assert same_pair_in_both_halves(d, halves[COIN]), "case A: no wave holds the same (cell, s') in both halves of the coin"
            assert any(same_pair_in_both_halves(d, halves[f]) for f in range(1, len(FEATURES))), "case A: no wave holds the same (cell, s') in both halves of a feature"
        # the episode's first decision: before differs from after for the two integer features
        first = d["first"]
        assert first.any()
        for f in (PREV_ACTION, STEP):
            assert (d["value"][f][first] != d["after"][f][first]).any(), f"case {case_id}: {FEATURES[f]} never differs across an episode's first period"
        print("split case", case_id, "decisions", d["env"].size, "first decisions", int(first.sum()), "half-1 shares",
              {FEATURES[f]: round(float(halves[f].mean()), 3) for f in halves})
        _FLIGHTS[case_id] = d
    return _FLIGHTS[case_id]


def assert_halves_sum_to_the_model(case_id, got, k=0, what=""):
    """`got`'s two halves summed == model_checks.yardstick(case) in pairs, reward_fx, terminal; by_code and steps_sum equal: the split changes no flight"""
    want = mc.yardstick(case_id)
    for f in ("pairs", "reward_fx", "terminal"):
        assert np.array_equal(np.asarray(got[f][k]).astype(np.int64).sum(axis=0), np.asarray(want[f]).astype(np.int64)), f"{what}: the halves of {f} do not sum to the model's"
    assert np.array_equal(got["by_code"][k], want["by_code"]) and int(got["steps_sum"][k]) == int(want["steps_sum"]), f"{what}: by_code / steps_sum"


def assert_split_set_equal(got, k, want, what):
    """table set `k` of a split-model result against the yardstick of that set: every output =="""
    for f in FIELDS:
        g, w = np.asarray(got[f][k]), np.asarray(want[f])
        assert g.shape == w.shape, f"{what}: {f} has shape {g.shape}, want {w.shape}"
        if f == "pairs":
            assert g.dtype == np.uint32, f"{what}: pairs is {g.dtype}"
        bad = np.argwhere(g.astype(np.int64) != w.astype(np.int64))
        assert not len(bad), (f"{what}: {f} differs in {len(bad)} of {w.size} entries (first at {tuple(int(v) for v in bad[0])}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}; "
                              f"sums {int(g.astype(np.int64).sum())} vs {int(w.astype(np.int64).sum())})")
