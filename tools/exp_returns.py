"""The realised-returns operator measured -> profiles/returns_timing.jsonl and profiles/returns_findings.jsonl.

    python tools/exp_returns.py timing   [--runs 7] [--timeout 300] [--variant NAME --out FILE]
    python tools/exp_returns.py findings [--envs 65536] [--episodes 4] [--timeout 600]

`timing`: the two kernels of dql_returns (k_returns_fly, k_returns_sweep) against k_model and k_score_map on identical arguments at eps = 0 — the same flights —
for 16 table sets x 4 096 envs and 1 x 65 536, float32, level 4, both flavours, one episode per env, max_steps 600, gamma 0.99.  Each shape and flavour runs in
a child process of its own; the three calls alternate: one warm-up, then the median of 7 runs with min and max; kernel times (HIP events around each launch)
beside the wall clock of the call.  `by_code` and `steps_sum` of the three calls must be equal, `visits + cut_decisions` must sum to the model's visits.

`findings`: one run per flavour on the reference's tables (tests/golden/assets) at level 4: `evaluation.value_calibration` of the realised returns at eps 0 and
eps 0.1, gamma 0.99, each under two seeds (the second is the sampling floor: how far two samples of the same policy differ).

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
LEVEL, SEED, MAX_STEPS, GAMMA = 4, 123, 600, 0.99
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
             "k_model": lambda t: ops.transition_model(cfg, QA, QB, n, SEED, 0.0, episodes=1, max_steps=MAX_STEPS, timing=t),
             "k_returns": lambda t: ops.returns_map(cfg, QA, QB, n, SEED, 0.0, GAMMA, episodes=1, max_steps=MAX_STEPS, timing=t)}
    wall = {k: [] for k in calls}; kern = {k: [] for k in calls}; sweep = []; res = {}
    for run in range(a.runs + 1):  # run 0 warms the kernels up
        for name, fn in calls.items():
            t = {}
            t0 = time.perf_counter()
            res[name] = fn(t)
            w = (time.perf_counter() - t0) * 1e3
            if run:
                wall[name].append(w); kern[name].append(t["fly_ms"] if name == "k_returns" else t["kernel_ms"])
                if name == "k_returns":
                    sweep.append(t["sweep_ms"])
    for f in ("by_code", "steps_sum"):
        assert np.array_equal(res["k_returns"][f], res["k_score_map"][f]) and np.array_equal(res["k_returns"][f], res["k_model"][f]), f
    r = res["k_returns"]
    assert int(r["visits"].sum()) + int(r["cut_decisions"].sum()) == int(res["k_model"]["visits"].sum())
    base = {"flavour": a.flavour, "table_sets": K, "envs_per_table": n, "episodes_per_env": 1, "level": LEVEL, "seed": SEED, "eps": 0.0, "gamma": GAMMA, "dtype": "float32",
            "max_steps": MAX_STEPS}
    for name in calls:
        row = dict(base, what="returns_vs_model_vs_score_map", kernel="k_returns_fly" if name == "k_returns" else name, kernel_ms=spread(kern[name]), wall_ms=spread(wall[name]))
        if name == "k_returns":
            row.update(sweep_ms=spread(sweep), sweep_block=256 if n % 256 == 0 else 64)
        print(json.dumps(row), flush=True)
    ks, km, kf, sw = (statistics.median(x) for x in (kern["k_score_map"], kern["k_model"], kern["k_returns"], sweep))
    print(json.dumps(dict(base, what="returns_summary", fly_over_score_map=kf / ks, fly_over_model=kf / km, sweep_over_fly=sw / kf, fly_minus_score_map_ms=kf - ks,
                          k_score_map_min_max_spread_ms=max(kern["k_score_map"]) - min(kern["k_score_map"]), decisions_kept=int(r["visits"].sum()),
                          decisions_cut=int(r["cut_decisions"].sum()), log_bytes=int(K * n * (MAX_STEPS + 1) * 8),
                          wall_ratio_over_score_map=statistics.median(wall["k_returns"]) / statistics.median(wall["k_score_map"]))), flush=True)


def summary_json(s):
    return {k: summary_json(v) if isinstance(v, dict) else ([None if np.isnan(x) else float(x) for x in v] if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def findings_child(a):
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import F32, Q_PAPER
    qa, qb = reference_tables()
    cfg = evaluation._flavour_config(a.flavour, LEVEL, F32, {"quirks": Q_PAPER})
    greedy = evaluation.greedy_actions(qa, qb)[0]
    base = {"flavour": a.flavour, "level": LEVEL, "envs": a.envs, "episodes_per_env": a.episodes, "max_steps": MAX_STEPS, "gamma": GAMMA, "dtype": "float32",
            "tables": "tests/golden/assets", "min_visits": 30}
    cal = {}
    for eps in (0.0, 0.1):
        for seed in (SEED, SEED + 1):
            t = {}
            r = ops.returns_map(cfg, qa, qb, a.envs, seed, eps, GAMMA, episodes=a.episodes, max_steps=MAX_STEPS, timing=t)
            c = cal[(eps, seed)] = evaluation.value_calibration(qa, qb, r["visits"][0], r["return_fx"][0], greedy=greedy)
            print(json.dumps(dict(base, what="value_calibration", eps=eps, seed=seed, fly_ms=t["fly_ms"], sweep_ms=t["sweep_ms"], decisions_kept=int(r["visits"].sum()),
                                  decisions_cut=int(r["cut_decisions"][0]), cells_visited=int((r["visits"][0] > 0).sum()), by_code=r["by_code"][0].tolist(),
                                  summary=summary_json(c["summary"]))), flush=True)
        # the sampling floor: the same policy under two seeds, cell by cell
        m0, m1 = cal[(eps, SEED)]["mean_return"], cal[(eps, SEED + 1)]["mean_return"]
        both = ~np.isnan(m0) & ~np.isnan(m1)
        d = np.abs(m0 - m1)[both]
        b = np.abs(cal[(eps, SEED)]["bias_mean"])[both]
        print(json.dumps(dict(base, what="sampling_floor", eps=eps, seeds=[SEED, SEED + 1], cells_in_both=int(both.sum()), median_abs_difference_of_mean_returns=float(np.median(d)),
                              q95_abs_difference=float(np.quantile(d, 0.95)), median_abs_bias_mean=float(np.median(b)), q95_abs_bias_mean=float(np.quantile(b, 0.95)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "findings"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=None, help="seconds a child process may take")
    ap.add_argument("--variant", default=None, help="tag every row with this name: an A/B build of the library loaded through DQL_LIB_PATH")
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
        jobs = [me + ["--flavour", fl, "--envs", str(a.envs), "--episodes", str(a.episodes)] for fl in FLAVOURS]
    out = Path(a.out or ROOT / "profiles" / ("returns_timing.jsonl" if a.what == "timing" else "returns_findings.jsonl"))
    lines = []
    for cmd in jobs:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)  # a time-out or a failure ends the tool: nothing more is started on the GPU
        if r.returncode != 0:
            sys.exit(f"{' '.join(cmd[2:])} failed with status {r.returncode}:\n{r.stderr[-4000:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                if a.variant:
                    ln = json.dumps(dict(json.loads(ln), variant=a.variant))
                lines.append(ln); print(ln, flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
