"""Shared by the refined-state tests (CPU emulation and GPU): the yardsticks of the refined learners and of `dql_score_refined` (include/dql.h).

`RefinedReference` is `ensemble_checks.Reference`'s loop on tables [n][2 * N_CELLS] with the unchanged oracle: the half of a decision is read from the oracle's
fields BEFORE each `o.step` with `split_model_checks._features`, greedy is `orc.agent_predict(qa[l], qb[l], [half * 945 + s])`, the update `orc.agent_update` with
`sa = r * 3 + a`, `ns = r'` (945 is a multiple of 63 and of 189, so the oracle's position-bin mask still reads the position bin), transfer `orc.transfer` on each
half's slice.  `stepwise_refined_score` is the stepwise greedy flight of refined table sets.  Neither knows anything of the kernels.  Both record what the cases are
there for, and `assert_*` helpers assert it ON THE RECORDS before anything is compared."""
import numpy as np

from dql_multirotor_landing_amd.config import N_CELLS
from oracle import oracle as orc
from oracle.oracle import Oracle

import ensemble_checks as ec
import model_checks as mc
import split_model_checks as smc

N_STATES = N_CELLS // 3
R_CELLS = 2 * N_CELLS
FEATURES = smc.FEATURES
ALL_FEATURES = tuple(range(len(FEATURES)))
F = {name: k for k, name in enumerate(FEATURES)}
OBS_FEATURES = (F["obs_p_x"], F["obs_v_x"], F["obs_a_x"])  # what load_env zeroes: the launch-boundary trap
TABLE_FIELDS = ("qa", "qb", "count")


# ---- cuts: the per-state means of one recorded flight; unvisited states get the feature's global mean (NOT +inf: every state splits) ----
_CUTS = {}


def mean_cut(case_id, feature):
    """float64 [945]: the coin's 0.5, else the per-state means of `feature` over split_model_checks' recorded flight `case_id`, the global mean where unvisited"""
    if (case_id, feature) not in _CUTS:
        if feature == smc.COIN:
            c = np.full(N_STATES, 0.5)
        else:
            d = smc.flight(case_id)
            c = smc.mean_cut(d, feature)
            c = np.where(np.isfinite(c), c, float(d["value"][feature].mean()))
        assert np.isfinite(c).all()
        _CUTS[(case_id, feature)] = c
    return _CUTS[(case_id, feature)]


def merged_cut(case_ids, feature):
    """the first finite per-state mean among the flights `case_ids` (levels differ per flight), the first flight's global mean elsewhere"""
    if feature == smc.COIN:
        return np.full(N_STATES, 0.5)
    out = np.full(N_STATES, np.inf)
    for cid in case_ids:
        c = smc.mean_cut(smc.flight(cid), feature)
        out = np.where(np.isfinite(out), out, c)
    return np.where(np.isfinite(out), out, float(smc.flight(case_ids[0])["value"][feature].mean()))


# ---- starting tables ----
def refined_trained_tables(n):
    """(qa, qb, count) float64 [n][2][N_CELLS]: learner l, half h = `ensemble_checks.trained_tables(2 n)` row 2 l + h, so the halves disagree from the first decision on"""
    return tuple(np.ascontiguousarray(t.reshape(int(n), 2, N_CELLS)) for t in ec.trained_tables(2 * int(n)))


class RefinedReference(ec.Reference):
    def __init__(self, cfg, n, seed, feature, cut, tables=None, strict=False, watch=(), **kw):
        """feature: a code; cut: a scalar or [945]; tables: initial (qa, qb, count), [n][2][N_CELLS] each (copied), default zeros; strict: the WRONG rule `>`;
        watch: period indices at which every learner's half (and whether it stands in a reset period) is recorded, `half_at[j]`"""
        super().__init__(cfg, n, seed, **kw)
        self.qa, self.qb, self.cnt = ((np.zeros((self.n, R_CELLS)) for _ in range(3)) if tables is None else
                                      (np.array(t, np.float64).reshape(self.n, R_CELLS) for t in tables))
        self.feature, self.strict = int(feature), bool(strict)
        self.cut = np.ascontiguousarray(np.broadcast_to(np.asarray(cut, np.float64), (N_STATES,)))
        assert not np.isnan(self.cut).any()
        self.rn, self.inn = self.o.field_names(False), self.o.field_names(True)
        self.watch, self.half_at = set(int(j) for j in watch), {}
        self.ev = {"written": [0, 0], "greedy_reads": [0, 0], "same_state_other_half": 0, "same_refined_state": 0, "value_on_cut": 0, "decisions": 0}

    def _halves(self, j):
        """(half [n], value [n]) of every env as the oracle's envs stand now, for the decision period j takes"""
        v = smc._features(self.o, self.rn, self.inn, j & 0xffffffff if self.feature == smc.COIN else j, self.seed)[self.feature]
        s = self.o.get_fields()[1][self.ii["idx_x"]]
        at = self.cut[np.clip(s, 0, N_STATES - 1)]
        assert np.isfinite(v).all() and (np.abs(v) < 8192.0).all(), "a value out of range: the kernels count a fault here"
        return (v > at if self.strict else v >= at).astype(np.int64), v, at

    def transfer(self, k, ratio):
        for l in range(self.n):
            for h in range(2):
                orc.transfer(self.qa[l][h * N_CELLS:(h + 1) * N_CELLS], self.qb[l][h * N_CELLS:(h + 1) * N_CELLS], k, ratio)

    def run(self, periods):
        o, n = self.o, self.n
        i_idx, i_fl, i_code, i_sc, i_rew = self.ii["idx_x"], self.ii["flags"], self.ii["code"], self.ii["step_count"], self.ri["reward"]
        k0, k1 = self.seed & 0xffffffff, (self.seed >> 32) & 0xffffffff
        act = np.zeros(n, np.uint8)
        half, value, at = self._halves(self.j)
        for _ in range(int(periods)):
            j = self.j
            _, ints = o.get_fields()
            s = ints[i_idx].copy(); was_done = (ints[i_fl] & 1) != 0
            if j in self.watch:
                self.half_at[j] = (half.copy(), (was_done | self.frozen).copy())
            words = {}
            for l in range(n):
                act[l] = 2
                if self.frozen[l] or was_done[l]:
                    continue
                r = orc.philox((j & 0xffffffff, (j >> 32) & 0xffffffff, l, ec.STREAM_ACTION), (k0, k1))
                words[l] = r
                e = int(self.level_episodes[l])
                if (int(r[0]) >> 8) < self.thr[min(e, len(self.thr) - 1)]:
                    act[l] = (int(r[1]) * 3) >> 32
                else:
                    act[l] = int(orc.agent_predict(self.qa[l], self.qb[l], [int(half[l]) * N_STATES + int(s[l])])[0])
                    self.ev["greedy_reads"][int(half[l])] += 1
            o.step(act)
            for l, b in self.snap.items():
                o.envs[l * self.es:(l + 1) * self.es] = b
            reals, ints = o.get_fields()
            half_n, value_n, at_n = self._halves(j + 1)  # of the state just entered, from the env as it stands, with j + 1
            for l, r in words.items():
                a, ns = int(act[l]), int(ints[i_idx][l])
                rs, rns = int(half[l]) * N_STATES + int(s[l]), int(half_n[l]) * N_STATES + ns
                sa = 3 * rs + a
                c = int(self.cnt[l][sa])
                al = self.alpha[c] if c < len(self.alpha) else self.cfg.alpha_min
                self.updates_inside += c < len(self.alpha); self.updates_beyond += c >= len(self.alpha)
                done = bool(ints[i_fl][l] & 1)
                orc.agent_update(self.qa[l], self.qb[l], self.cnt[l], [sa], [rns], [al], self.cfg.gamma, [reals[i_rew][l]], quirks=self.cfg.quirks,
                                 coin=[int(r[2]) >> 31], done=[int(done)])
                self.decisions[l] += 1
                self.same_state += int(ns == int(s[l]))
                self.ev["decisions"] += 1; self.ev["written"][int(half[l])] += 1
                self.ev["same_state_other_half"] += int(ns == int(s[l]) and rns != rs); self.ev["same_refined_state"] += int(rns == rs)
                self.ev["value_on_cut"] += int(value[l] == at[l])
                if done:
                    code = int(ints[i_code][l])
                    self.episodes[l] += 1; self.successes[l] += code == ec.GOAL; self.by_code[code][l] += 1
                    if self.log_n[l] < self.cap:
                        self.log_code[l][self.log_n[l]] = code; self.log_len[l][self.log_n[l]] = int(ints[i_sc][l])
                    self.log_n[l] += 1
                    self.windows[l].append(int(code == ec.GOAL)); self.level_episodes[l] += 1
                    if sum(self.windows[l]) >= self.min_successes:
                        self.promoted[l] = self.level_episodes[l]; self.frozen[l] = True
                    elif self.level_episodes[l] >= self.max_episodes:
                        self.frozen[l] = True
                    if self.frozen[l]:
                        self.freeze_period[l] = j
                        self.snap[l] = o.envs[l * self.es:(l + 1) * self.es].copy()
            half, value, at = half_n, value_n, at_n
            self.j += 1

    def result(self):
        out = super().result()
        for k in TABLE_FIELDS:
            out[k] = out[k].reshape(self.n, 2, N_CELLS)
        return out


def assert_learner_events(ref, what, both_halves=True, same_state=True):
    """ON THE YARDSTICK's records: both halves written and read greedily, a transition that changes half with idx' == idx and one that keeps both"""
    ev = ref.ev
    print(what, ev)
    assert ev["decisions"] > 0, what
    if both_halves:
        assert min(ev["written"]) > 0, f"{what}: a half is never written {ev}"
    if same_state:
        assert ev["same_state_other_half"] > 0 and ev["same_refined_state"] > 0, f"{what}: no transition with idx' == idx that changes half, or none that keeps both {ev}"


def refined_ensemble_result(ens):
    """`ensemble_checks.ensemble_result` of a refined SequentialEnsemble: the tables are the refined ones"""
    qa, qb, cnt = ens.get_refined_tables()
    out = {"qa": qa, "qb": qb, "count": cnt}
    out.update(ens.counters())
    code, length, n = ens.episode_log()
    out.update({"log_code": code, "log_len": length, "log_n": n})
    out.update(ens.state())
    return out


# ---- scoring: a stepwise greedy flight of refined table sets, in the shapes of model_checks' cases A and D ----
SCORE_CASES = ("A", "D")
SCORE_SEED = mc.SEED


def score_case(case_id):
    """(cfg, n, max_steps, episodes) of a scoring case: model_checks' case without its eps"""
    cfg, _, _, n, max_steps, episodes = mc.case_args(case_id)
    return cfg, n, max_steps, episodes


def score_tables(n_sets, first=0):
    """(qa, qb) float64 [n_sets][2][N_CELLS]: set k, half h = trained_tables row 2 (first + k) + h"""
    qa, qb, _ = refined_trained_tables(first + n_sets)
    return np.ascontiguousarray(qa[first:]), np.ascontiguousarray(qb[first:])


def stepwise_refined_score(cfg, qa2, qb2, feature, cut, n, seed, max_steps, episodes, strict=False, always_half0=False):
    """one refined table set (qa2, qb2: [2][N_CELLS]) flown greedily by `n` envs: {"by_code", "steps_sum", "ep_code" uint8 [episodes][n], "ep_steps" uint16
    [episodes][n], "reads" (greedy choices per half), "on_cut"}; strict / always_half0: WRONG rules, to show that a case tells them from the right one"""
    qa, qb = (np.ascontiguousarray(t, np.float64).ravel() for t in (qa2, qb2))
    assert qa.size == qb.size == R_CELLS
    cut = np.ascontiguousarray(np.broadcast_to(np.asarray(cut, np.float64), (N_STATES,)))
    o = Oracle(cfg, n, seed=seed)
    rn, inn = o.field_names(False), o.field_names(True)
    i_idx, i_fl, i_code, i_sc = (inn.index(f) for f in ("idx_x", "flags", "code", "step_count"))
    finished = np.zeros(n, np.int64)
    by_code = np.zeros(mc.N_COLS, np.int64)
    ep_code = np.full((episodes, n), 0xff, np.uint8); ep_steps = np.zeros((episodes, n), np.uint16)
    reads, on_cut, steps_sum = [0, 0], 0, 0
    for j in range(max_steps + 1):
        _, ints = o.get_fields()
        s = ints[i_idx].astype(np.int64); was_done = (ints[i_fl] & mc.FL_DONE) != 0
        v = smc._features(o, rn, inn, j, seed)[feature]
        assert np.isfinite(v).all() and (np.abs(v) < 8192.0).all()
        at = cut[np.clip(s, 0, N_STATES - 1)]
        half = (v > at if strict else v >= at).astype(np.int64)
        if always_half0:
            half[:] = 0
        act = orc.agent_predict(qa, qb, np.where(was_done, 0, half * N_STATES + s)).astype(np.int64)
        act[was_done] = 2  # a reset period takes no action
        live = finished < episodes
        counts = live & ~was_done
        for h in range(2):
            reads[h] += int((counts & (half == h)).sum())
        on_cut += int((counts & (v == at)).sum())
        o.step(act.astype(np.uint8))
        _, ints = o.get_fields()
        done = (ints[i_fl] & mc.FL_DONE) != 0
        end = counts & done
        code = ints[i_code].astype(np.int64)
        np.add.at(by_code, code[end], 1)
        lens = ints[i_sc] & 0xffff
        steps_sum += int(lens[end].sum())
        for i in np.flatnonzero(end):
            ep_code[finished[i], i] = code[i]; ep_steps[finished[i], i] = lens[i]
        finished[end] += 1
        if (finished >= episodes).all():
            break
    by_code[mc.N_CODES] = n * episodes - int(finished.sum())
    return {"by_code": by_code, "steps_sum": steps_sum, "ep_code": ep_code, "ep_steps": ep_steps, "reads": reads, "on_cut": on_cut}


_SCORES = {}


def score_yardstick(case_id, feature, k=0):
    """the stepwise flight of table set `k` of `score_tables` under the case, `feature` at its mean cut (flight: the same case id where split_model_checks has it,
    else "B64"), computed once; asserts ON IT that both halves are read greedily"""
    key = (case_id, feature, k)
    if key not in _SCORES:
        cfg, n, max_steps, episodes = score_case(case_id)
        qa, qb = score_tables(1, first=k)
        w = stepwise_refined_score(cfg, qa[0], qb[0], feature, score_cut(case_id, feature), n, SCORE_SEED, max_steps, episodes)
        print("refined score case", case_id, FEATURES[feature], "set", k, "reads", w["reads"], "by_code", w["by_code"].tolist(), "steps_sum", w["steps_sum"])
        assert min(w["reads"]) > 0, f"case {case_id}, {FEATURES[feature]}: a half is never read greedily {w['reads']}"
        _SCORES[key] = w
    return _SCORES[key]


def score_cut(case_id, feature):
    return mean_cut(case_id, feature)


def assert_score_equal(got, k, want, n, what, log=True):
    """table set `k` of an `ops.score_refined` result against the yardstick of that set: every output =="""
    assert np.array_equal(np.asarray(got["by_code"][k]), want["by_code"]), f"{what}: by_code {np.asarray(got['by_code'][k]).tolist()} vs {want['by_code'].tolist()}"
    assert int(got["steps_sum"][k]) == int(want["steps_sum"]), f"{what}: steps_sum {int(got['steps_sum'][k])} vs {want['steps_sum']}"
    if log:
        for f in ("ep_code", "ep_steps"):
            g = np.asarray(got[f])[:, k * n:(k + 1) * n]
            assert np.array_equal(g, want[f]), f"{what}: {f} differs in {int((g != want[f]).sum())} entries"


# ---- the learner cases, shared by the CPU emulation and the GPU tests: flown once per process, left unchanged ----
LOG_CAP = 32
_REFS = {}


def zeros_reference(dtype, quirks, feature, n, seed, periods, watch=(), cut=None, strict=False):
    """(result, the reference, cut) of `n` learners from zeros at level 0 with `ensemble_checks.EPS_TABLE`; cut None: the feature's means over flight "C" """
    from dql_multirotor_landing_amd.config import training_config
    key = ("zeros", dtype, quirks, feature, n, seed, periods, None if cut is None else float(cut), strict)
    if key not in _REFS:
        cfg = training_config(0, quirks=quirks, dtype=dtype)
        c = mean_cut("C", feature) if cut is None else cut
        ref = RefinedReference(cfg, n, seed, feature, c, strict=strict, watch=watch, log_capacity=LOG_CAP)
        ref.run(periods)
        _REFS[key] = (ref.result(), ref, c)
    return _REFS[key]


def trained_reference(dtype, feature, n, watch=(ec.TRAINED_LEARNERS_SPLIT[0],)):
    """(result, the reference, cut, tables) of `n` learners from `refined_trained_tables(n)` at level 4 under quirks 0x40, greedy, window 4 / 2 successes / 6
    episodes, 400 periods, the cut the feature's means over flight "B64"; asserts ON IT that successes and failures both occur and both halves are written and
    read greedily"""
    from dql_multirotor_landing_amd.config import training_config
    key = ("trained", dtype, feature, n)
    if key not in _REFS:
        cfg = training_config(4, quirks=ec.Q_PAPER, dtype=dtype)
        tables = refined_trained_tables(n)
        cut = mean_cut("B64", feature)
        ref = RefinedReference(cfg, n, ec.TRAINED_LEARNERS_SEED, feature, cut, tables=tables, watch=watch, **ec.TRAINED_LEARNERS_CASE)
        ref.run(ec.TRAINED_LEARNERS_PERIODS)
        want = ref.result()
        failures = int((want["episodes"] - want["successes"]).sum())
        print("trained", FEATURES[feature], "n", n, "successes", int(want["successes"].sum()), "failures", failures, ref.ev)
        assert want["successes"].sum() >= 1 and failures >= 1, "successes and failures are both needed"
        assert min(ref.ev["written"]) > 0 and min(ref.ev["greedy_reads"]) > 0, f"both halves are to be written and read greedily {ref.ev}"
        _REFS[key] = (want, ref, cut, tables)
    return _REFS[key]


def assert_half_one_at_the_boundary(ref, j, what):
    """ON THE YARDSTICK: a learner that flies (not frozen, not in a reset period) at the launch boundary `j` stands in half 1"""
    half, idle = ref.half_at[j]
    assert ((half == 1) & ~idle).any(), f"{what}: no flying learner stands in half 1 at the launch boundary {j}"


# levels 0 -> 2 through set_level / run(400) / transfer by hand, 24 learners, window 4, 6 episodes
CURRICULUM_L, CURRICULUM_SEED, CURRICULUM_PERIODS = 24, 7, 400
CURRICULUM_RULE = dict(window=4, min_successes=2, max_episodes=6)
CURRICULUM_EPS = ([0.3], [0.05], [0.05])
CURRICULUM_RATIOS = (1.0, 0.8172650252856599)  # Trainer.transfer_learning_ratio(k), k = 0, 1


def curriculum_reference(feature):
    """(result, cut) of the curriculum case; asserts ON IT that both halves of levels 0 .. 2 hold values"""
    from dql_multirotor_landing_amd.config import F32, training_config
    key = ("curriculum", feature)
    if key not in _REFS:
        cfg = training_config(0, quirks=ec.Q_PAPER, dtype=F32)
        cut = merged_cut(("C", "D", "B64"), feature)
        ref = RefinedReference(cfg, CURRICULUM_L, CURRICULUM_SEED, feature, cut, eps=CURRICULUM_EPS[0], log_capacity=LOG_CAP, **CURRICULUM_RULE)
        for k in range(3):
            if k:
                ref.set_level(k)
                ref.set_schedules(CURRICULUM_EPS[k], **CURRICULUM_RULE)
            ref.run(CURRICULUM_PERIODS)
            if k < 2:
                ref.transfer(k, CURRICULUM_RATIOS[k])
        want = ref.result()
        lvl = np.arange(N_CELLS) // 567
        print("curriculum", FEATURES[feature], ref.ev, "cells holding values per level, half 0 / 1",
              [[int((want["qa"][:, h, lvl == k] != 0).sum()) for h in range(2)] for k in range(3)])
        assert all((want["qa"][:, h, lvl == k] != 0).any() for h in range(2) for k in range(3)), "both halves of levels 0 .. 2 are to hold values"
        _REFS[key] = (want, cut)
    return _REFS[key]
