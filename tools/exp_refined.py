#!/usr/bin/env python3
"""Sequential learners on a state split by one bit of hidden state on the GPU: what the refinement costs per period, and whether it lands
better.

    python tools/exp_refined.py timing [--sizes 4096,65536] [--periods 512] [--repeats 7] [--out profiles/refined_timing.jsonl]
    python tools/exp_refined.py landing [--learners 1024] [--episodes 50000] [--score 1024] [--arms plain,pitch_sp,coin] [--out profiles/refined_landing.jsonl]

timing: float32, `training_config(0)` with the reference's quirks, tables of zeros, exploration rate 1 and no promotion, so every learner stays live.  Per size one
plain ensemble (k_learn) and one refined by `pitch_sp` at the scalar cut 0.0 (k_learn_refined) live in one process; after a warm-up run each, the two alternate
`--repeats` times with runs of `--periods` periods.  Per way the median of `dql_diag_ensemble_last` (HIP events around the run call's launches) is written as
microseconds per period.  EXPECTATION, written before the first run: within a few per cent of each other — the refined lane does one more row load (the row of
r', 48 B) and one 8-byte load of the cut per period and strides its tables by 2 x 22 680 B instead of 22 680 B; a period is 21 - 22 physics ticks of arithmetic.

landing: `as_launched_config`, float32, the "paper" preset (evaluation.Q_PAPER; on entering level k + 1, `Q[k+1] = Q[k] ratio(k + 1)`), level by level with the
reference's schedules and `--episodes` per level, `--learners` learners per arm, then every learner's tables flown greedily where they live (`--score` envs per
learner and flavour).  Arms: "plain" (no refinement), "pitch_sp" (the cut: per level 0 .. 4 one `ops.split_model` pass over the published tables' eps = 0.1
flights in the training flavour, cut = +inf, merged by `evaluation.refinement_cut`), "coin" (cut 0.5: the table doubled for no information — the control).  Per arm
one line: touchdown and goal-hold quantiles over learners, the share at or above the bar, per level the promoted learners and the quantiles of their
first-promotion episode, the periods flown and the wall clock of the curriculum (a host clock around calls that end in a device synchronise; scoring outside).
Committed so far: the run with `--episodes 4000 --out profiles/refined_landing_4000.jsonl`; the default budget's file does not exist yet."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dql_multirotor_landing_amd import _lib, evaluation, ops  # noqa: E402
from dql_multirotor_landing_amd.config import F32, as_launched_config, training_config  # noqa: E402
from dql_multirotor_landing_amd.ensemble import REFERENCE_RATIOS, SequentialEnsemble, exploration_rates, min_successes_for, train_level  # noqa: E402

ASSETS = ROOT / "tests" / "golden" / "assets"


def last_ms(ens):
    v = C.c_double()
    _lib.check(ens.lib.dql_diag_ensemble_last(ens._h, C.byref(v)))
    return float(v.value)


def timing(a):
    rows = []
    for L in [int(s) for s in a.sizes.split(",")]:
        cfg = training_config(0, quirks=0x7F, dtype=F32)
        kw = dict(seed=a.seed, eps=[1.0], window=100, min_successes=101, max_episodes=1 << 30)
        ways = {"k_learn": SequentialEnsemble(cfg, L, **kw), "k_learn_refined": SequentialEnsemble(cfg, L, **kw)}
        try:
            ways["k_learn_refined"].set_refinement("pitch_sp", 0.0)
            ms = {w: [] for w in ways}
            for e in ways.values():
                e.run(a.periods)  # warm-up (period 0, the reset period, included)
            for _ in range(a.repeats):
                for w, e in ways.items():
                    e.run(a.periods)
                    ms[w].append(last_ms(e))
            med = {w: statistics.median(v) for w, v in ms.items()}
            for w, e in ways.items():
                rows.append({"what": "SequentialEnsemble.run", "kernel": w, "dtype": "float32", "learners": L, "periods_per_run": a.periods, "repeats": a.repeats,
                             "us_per_period": round(med[w] / a.periods * 1e3, 3), "us_per_period_min_max": [round(min(ms[w]) / a.periods * 1e3, 3), round(max(ms[w]) / a.periods * 1e3, 3)],
                             "ratio_to_k_learn": round(med[w] / med["k_learn"], 4), "decisions": int(e.counters()["decisions"].sum()), "index_faults": e.index_faults(),
                             "method": "median of dql_diag_ensemble_last over the timed runs, the two ways alternating in one process after a warm-up run each",
                             "expectation_written_before_the_run": "within a few per cent: one more row load and a larger table stride per period"})
                print(json.dumps(rows[-1]), flush=True)
        finally:
            for e in ways.values():
                e.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in rows))


def published_cut(feature, n_envs=4096, eps=0.1, seed=123):
    qa, qb = (np.load(ASSETS / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
    results = [ops.split_model(evaluation._flavour_config("training", k, F32, {"quirks": evaluation.Q_PAPER}), qa, qb, n_envs, seed, eps, feature, np.inf) for k in range(5)]
    return evaluation.refinement_cut(results)


def quantiles(x):
    x = np.asarray(x, dtype=np.float64)
    return {"mean": round(float(x.mean()), 4), **{k: round(float(v), 4) for k, v in zip(("min", "q05", "q25", "q50", "q75", "q95", "max"), np.quantile(x, (0, 0.05, 0.25, 0.5, 0.75, 0.95, 1)))}}


def landing(a):
    rows = []
    for arm in a.arms.split(","):
        cfg = as_launched_config(dtype=F32, quirks=evaluation.Q_PAPER)
        ens = SequentialEnsemble(cfg, a.learners, seed=a.seed, max_episodes=a.episodes)
        try:
            cut = None
            if arm != "plain":
                cut = published_cut(arm) if arm != "coin" else np.full(945, 0.5)
                ens.set_refinement(arm, cut)
            levels, t0 = [], time.perf_counter()
            for k in range(5):
                if k:
                    ens.set_level(k)
                ens.set_schedules(eps=exploration_rates(k), window=100, min_successes=min_successes_for(100), max_episodes=a.episodes)
                flown = train_level(ens, on_chunk=lambda e, f: print(f"{arm} level {k}: {f} periods, {e.n_live()} live, {time.perf_counter() - t0:.1f} s", flush=True))
                p = ens.counters()["promotion_episode"]
                levels.append({"level": k, "periods": int(flown), "promoted": int((p >= 0).sum()),
                               "promotion_episode": None if not (p >= 0).any() else {q: int(np.quantile(p[p >= 0], float(q))) for q in ("0.05", "0.25", "0.5", "0.75", "0.95")}})
                if k < 4:
                    ens.transfer(k + 1, REFERENCE_RATIOS[k + 1])
            wall = time.perf_counter() - t0
            t = {}
            kw = dict(n_envs=a.score, episodes=1, level=4, seed=123, timing=t)
            r = ens.landing_rates(**kw) if arm == "plain" else ens.refined_landing_rates(**kw)
            td, gh = r["touchdown_rate"], r["goal_hold_rate"]
            rows.append({"what": "refined_landing", "arm": arm, "learners": a.learners, "seed": a.seed, "episode_budget_per_level": a.episodes, "config": "as_launched_config, float32, quirks 0x40, paper transfer order",
                         "cut": None if cut is None else {"finite_states_per_level": [int(np.isfinite(cut[189 * k:189 * (k + 1)]).sum()) for k in range(5)]},
                         "score_envs_per_learner": a.score, "touchdown_rate": quantiles(td), "goal_hold_rate": quantiles(gh), "share_at_or_above_bar": round(float((td >= evaluation.LANDING_BAR).mean()), 4),
                         "levels": levels, "periods": int(sum(lv["periods"] for lv in levels)), "curriculum_wall_s": round(wall, 1), "score_kernel_ms": round(t["kernel_ms"], 1),
                         "index_faults": ens.index_faults()})
            print(json.dumps(rows[-1]), flush=True)
        finally:
            ens.close()
    qa, qb = (np.load(ASSETS / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))
    rr = evaluation.landing_rates(qa, qb, n_envs=a.score, episodes=1, level=4, seed=123)
    rows.append({"what": "refined_landing", "arm": "published tables", "touchdown_rate": round(float(rr["touchdown_rate"][0]), 4), "goal_hold_rate": round(float(rr["goal_hold_rate"][0]), 4)})
    print(json.dumps(rows[-1]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("timing", "landing"))
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--periods", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--learners", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=50000)
    ap.add_argument("--score", type=int, default=1024)
    ap.add_argument("--arms", default="plain,pitch_sp,coin")
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args()
    a.out = a.out or str(ROOT / "profiles" / ("refined_timing.jsonl" if a.what == "timing" else "refined_landing.jsonl"))
    (timing if a.what == "timing" else landing)(a)
