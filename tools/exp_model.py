"""The transition-model operator measured -> profiles/model_timing.jsonl and profiles/model_findings.jsonl.

    python tools/exp_model.py timing   [--runs 7] [--timeout 300]
    python tools/exp_model.py findings [--envs 262144] [--episodes 8] [--score-envs 4096] [--timeout 600]

`timing`: k_model at eps = 0 against k_score_map on identical arguments — the same flights, `visits` the only work k_score_map does on top of scoring — for
16 table sets x 4 096 envs and 1 x 65 536, float32, level 4, both flavours, one episode per env.  The two kernels alternate in one process: one warm-up, then
the median of 7 runs with min and max; kernel time (HIP events around the launch) beside the wall clock of the call, which for the model includes the copy of
the pair tables (10.7 MB per set).  `visits`, `by_code` and `steps_sum` of the two calls must be equal.

`findings`: one large sample per flavour from the reference's tables (tests/golden/assets), eps in {0.1, 1.0} and a second eps = 0.1 sample under another
seed.  Recorded: coverage of each model; `model_divergence` between eps 0.1 and eps 1.0 beside the divergence of the two eps = 0.1 samples (what sampling
alone produces); and, for min_visits in {1, 30, 200}, `solve_model` on the eps = 1.0 and on the pooled model, its greedy policy flown by `ops.score`, beside the
reference's own tables on the same envs.

Every GPU step runs in a child process of its own under `--timeout` seconds; a child that fails or runs out of time ends the tool."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
LEVEL, SEED, MAX_STEPS = 4, 123, 600
SHAPES = ((16, 4096), (1, 65536))
FLAVOURS = ("simulation", "training")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def reference_tables():
    assets = ROOT / "tests" / "golden" / "assets"
    return tuple(np.load(assets / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))


def timing_child(a):
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import F32, Q_PAPER
    qa, qb = reference_tables()
    sets3 = [(qa, qb), (np.zeros_like(qa), np.zeros_like(qb)), (qa, -qb)]
    K, n = a.sets, a.envs
    QA = np.stack([sets3[k % 3][0] for k in range(K)]); QB = np.stack([sets3[k % 3][1] for k in range(K)])
    cfg = evaluation._flavour_config(a.flavour, LEVEL, F32, {"quirks": Q_PAPER})
    calls = {"k_score_map": lambda t: ops.score_map(cfg, QA, QB, n, SEED, episodes=1, max_steps=MAX_STEPS, timing=t),
             "k_model": lambda t: ops.transition_model(cfg, QA, QB, n, SEED, 0.0, episodes=1, max_steps=MAX_STEPS, timing=t)}
    wall = {k: [] for k in calls}; kern = {k: [] for k in calls}; res = {}
    for run in range(a.runs + 1):  # run 0 warms both kernels up
        for name, fn in calls.items():
            t = {}
            t0 = time.perf_counter()
            res[name] = fn(t)
            w = (time.perf_counter() - t0) * 1e3
            if run:
                wall[name].append(w); kern[name].append(t["kernel_ms"])
    for f in ("visits", "by_code", "steps_sum"):
        assert np.array_equal(res["k_model"][f], res["k_score_map"][f]), f
    m = res["k_model"]
    for name in calls:
        print(json.dumps({"what": "model_vs_score_map", "kernel": name, "flavour": a.flavour, "table_sets": K, "envs_per_table": n, "episodes_per_env": 1, "level": LEVEL, "seed": SEED,
                          "eps": 0.0, "dtype": "float32", "max_steps": MAX_STEPS, "kernel_ms": spread(kern[name]), "wall_ms": spread(wall[name])}), flush=True)
    ks, km = statistics.median(kern["k_score_map"]), statistics.median(kern["k_model"])
    print(json.dumps({"what": "model_over_score_map", "flavour": a.flavour, "table_sets": K, "envs_per_table": n, "kernel_ratio": km / ks, "kernel_ms_difference": km - ks,
                      "k_score_map_min_max_spread_ms": max(kern["k_score_map"]) - min(kern["k_score_map"]),
                      "wall_ratio": statistics.median(wall["k_model"]) / statistics.median(wall["k_score_map"]), "pair_table_bytes": int(m["pairs"].nbytes),
                      "decisions": int(m["visits"].sum()), "distinct_pairs_set0": int((m["pairs"][0] > 0).sum()), "largest_pair_set0": int(m["pairs"][0].max()),
                      "added_work": "per wave and counted period: one returnless 32-bit global atomic per distinct pair (equal pairs merged in the wave), one LDS 64-bit add per lane with a non-zero reward, one 64-bit global atomic per terminal; at the end at most 45 sweeps of 64-bit global atomics"}),
          flush=True)


def coverage(m):
    v = m["visits"][0]
    return {"decisions": int(v.sum()), "cells_visited": int((v > 0).sum()), "cells_30": int((v >= 30).sum()), "cells_200": int((v >= 200).sum()),
            "distinct_pairs": int((m["pairs"][0] > 0).sum()), "terminal_decisions": int(m["terminal"].sum()), "by_code": m["by_code"][0].tolist()}


def divergence_summary(d, weights):
    ok = ~np.isnan(d)
    if not ok.any():
        return {"cells": 0}
    w = weights[ok].astype(np.float64)
    return {"cells": int(ok.sum()), "median": float(np.median(d[ok])), "mean": float(d[ok].mean()), "visit_weighted_mean": float((d[ok] * w).sum() / w.sum()),
            "q95": float(np.quantile(d[ok], 0.95)), "share_above_0.1": float((d[ok] > 0.1).mean()), "share_above_0.25": float((d[ok] > 0.25).mean())}


def findings_child(a):
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import F32, Q_PAPER
    qa, qb = reference_tables()
    cfg = evaluation._flavour_config(a.flavour, LEVEL, F32, {"quirks": Q_PAPER})
    good = "TERMINAL_CONTACT" if a.flavour == "simulation" else "TERMINAL_SUCCESS"
    base = {"flavour": a.flavour, "level": LEVEL, "envs": a.envs, "episodes_per_env": a.episodes, "max_steps": MAX_STEPS, "dtype": "float32", "tables": "tests/golden/assets"}
    models = {}
    for name, eps, seed in (("eps0.1", 0.1, SEED), ("eps0.1_other_seed", 0.1, SEED + 1), ("eps1.0", 1.0, SEED)):
        t = {}
        models[name] = ops.transition_model(cfg, qa, qb, a.envs, seed, eps, episodes=a.episodes, max_steps=MAX_STEPS, timing=t)
        print(json.dumps(dict(base, what="model_coverage", model=name, eps=eps, seed=seed, kernel_ms=t["kernel_ms"], **coverage(models[name]))), flush=True)
    m01, m01b, m10 = (models[k] for k in ("eps0.1", "eps0.1_other_seed", "eps1.0"))
    for mv in (30, 200, 1000):
        between = evaluation.model_divergence(m01["pairs"][0], m01["terminal"][0], m10["pairs"][0], m10["terminal"][0], mv)
        noise = evaluation.model_divergence(m01["pairs"][0], m01["terminal"][0], m01b["pairs"][0], m01b["terminal"][0], mv)
        both = ~np.isnan(between) & ~np.isnan(noise)
        w = np.minimum(m01["visits"][0], m10["visits"][0])
        print(json.dumps(dict(base, what="model_divergence", min_visits=mv, eps01_vs_eps10=divergence_summary(between, w),
                              eps01_vs_eps01_other_seed=divergence_summary(noise, np.minimum(m01["visits"][0], m01b["visits"][0])),
                              cells_in_both=int(both.sum()), median_excess_over_sampling=float(np.median(between[both] - noise[both])) if both.any() else None)), flush=True)
    ref = ops.score(cfg, qa, qb, a.score_envs, SEED, episodes=1, max_steps=MAX_STEPS)
    columns = list(ref["columns"])
    print(json.dumps(dict(base, what="reference_tables_flown", score_envs=a.score_envs, by_code=dict(zip(columns, ref["by_code"][0].tolist())),
                          rate=float(ops.rates_from_counts(ref["by_code"], good)[0]), rate_of=good)), flush=True)
    pooled = {f: m01[f][0].astype(np.int64) + m01b[f][0] + m10[f][0] for f in ("pairs", "reward_fx", "terminal")}
    for source, m in (("eps1.0", {f: m10[f][0] for f in ("pairs", "reward_fx", "terminal")}), ("pooled", pooled)):
        for mv in (1, 30, 200):
            q, solved = evaluation.solve_model(m["pairs"], m["reward_fx"], m["terminal"], cfg.gamma, min_visits=mv)
            r = ops.score(cfg, q, q, a.score_envs, SEED, episodes=1, max_steps=MAX_STEPS)
            agree = evaluation.greedy_actions(q, q)[0] == evaluation.greedy_actions(qa, qb)[0]
            states_solved = solved.reshape(-1, 3).any(axis=1)
            print(json.dumps(dict(base, what="solved_policy_flown", model=source, min_visits=mv, gamma=cfg.gamma, cells_solved=int(solved.sum()), states_with_a_solved_action=int(states_solved.sum()),
                                  agrees_with_reference_on_solved_states=float(agree[states_solved].mean()), score_envs=a.score_envs,
                                  by_code=dict(zip(columns, r["by_code"][0].tolist())), rate=float(ops.rates_from_counts(r["by_code"], good)[0]), rate_of=good)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "findings"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--envs", type=int, default=262144)
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--score-envs", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=None, help="seconds a child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--flavour", default="simulation", help=argparse.SUPPRESS)
    ap.add_argument("--sets", type=int, default=16, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return timing_child(a) if a.what == "timing" else findings_child(a)
    import __graft_entry__ as g
    g.build_hip()
    timeout = a.timeout or (300 if a.what == "timing" else 600)
    me = [sys.executable, str(Path(__file__).resolve()), a.what, "--child"]
    if a.what == "timing":
        jobs = [me + ["--flavour", fl, "--sets", str(K), "--envs", str(n), "--runs", str(a.runs)] for K, n in SHAPES for fl in FLAVOURS]
    else:
        jobs = [me + ["--flavour", fl, "--envs", str(a.envs), "--episodes", str(a.episodes), "--score-envs", str(a.score_envs)] for fl in FLAVOURS]
    out = Path(a.out or ROOT / "profiles" / ("model_timing.jsonl" if a.what == "timing" else "model_findings.jsonl"))
    lines = []
    for cmd in jobs:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)  # a time-out or a failure ends the tool: nothing more is started on the GPU
        if r.returncode != 0:
            sys.exit(f"{' '.join(cmd[2:])} failed with status {r.returncode}:\n{r.stderr[-4000:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln); print(ln, flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
