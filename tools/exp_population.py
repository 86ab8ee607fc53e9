"""Populations on one GPU: what K agents in one launch cost, and what concurrent curriculum attempts save.

  throughput -> profiles/population_throughput.jsonl: us per agent period and env-steps/s of populations of K = 1, 2, 4 agents x 32 768 envs,
                beside a context of 32 768 envs and one of 131 072, P = 16, bench.py's configs[4] workload (per-env platforms + noise, f32)
  attempts   -> profiles/population_attempts.jsonl: wall clock of curriculum_attempts over bench.py's curriculum seeds at concurrency 1, 2, 3,
                with a hash of the chosen tables per seed (equal across concurrency settings).  bench.py's recipe except its sync period: a
                population folds every launch (the windowed schedule is single-agent), so the recipe here is CURRICULUM_KW with sync_period None.

python tools/exp_population.py [--what throughput|attempts|both] [--seeds 12]"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _cfg():
    from dql_multirotor_landing_amd.config import DqlConfig, F32
    return DqlConfig(dtype=F32, per_env_platform=1, fold_per_step=1, noise_pos_sd=0.25, noise_vel_sd=0.1)


def _time(eng, train, stats, steps, warmup):
    train(warmup); eng.sync()
    d0 = stats(); t0 = time.perf_counter()
    train(steps); eng.sync()
    wall = time.perf_counter() - t0
    return wall, stats() - d0


def throughput(out, steps, warmup):
    from dql_multirotor_landing_amd.engine import Engine
    from dql_multirotor_landing_amd.population import Population
    import bench
    E, P, eps = 32768, 16, 0.1
    rows = []
    for envs in (E, 4 * E):
        eng = Engine(_cfg(), envs, seed=42)
        eng.set_option("periods_per_launch", P)
        wall, dec = _time(eng, lambda n: eng.train_steps(n, eps), lambda: eng.stats()["decisions"], steps, warmup)
        eng.close()
        rows.append({"what": "context", "envs": envs, "agents": 1})
        rows[-1].update(us_per_period=wall * 1e6 / steps, env_steps_per_s=dec / wall)
    for K in (1, 2, 4):
        pop = Population(_cfg(), K, E, [42 + 7919 * k for k in range(K)])
        pop.set_option("periods_per_launch", P)
        wall, dec = _time(pop, lambda n: pop.pop_train_steps(n, {k: eps for k in range(K)}),
                          lambda: sum(pop.agent_stats(k)["decisions"] for k in range(K)), steps, warmup)
        faults = sum(pop.index_faults(k) for k in range(K))
        pop.close()
        rows.append({"what": "population", "envs": K * E, "agents": K, "envs_per_agent": E, "index_faults": faults,
                     "us_per_period": wall * 1e6 / steps, "env_steps_per_s": dec / wall})
    base = rows[0]["env_steps_per_s"]
    with open(out, "w") as f:
        for r in rows:
            r.update(periods_per_launch=P, steps=steps, warmup=warmup, vs_one_context=r["env_steps_per_s"] / base,
                     workload="bench.py configs[4] flavour (per-env platforms + noise), f32, eps 0.1", library_source_sha16=bench.lib_source_sha16())
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


def attempts(out, n_seeds):
    import tempfile
    import bench
    from dql_multirotor_landing_amd.attempts import SELECTION_SEED, attempt_seed, curriculum_attempts
    from dql_multirotor_landing_amd.config import F32, Q_PAPER
    from dql_multirotor_landing_amd.evaluation import landing_score
    from dql_multirotor_landing_amd.trainer import Trainer
    n = 32768
    budget = bench.CURRICULUM_BUDGET_PER_ENV * n
    with open(out, "w") as f:
        for conc in (1, 2, 3):
            for seed in bench.CURRICULUM_SEEDS[:n_seeds]:
                with tempfile.TemporaryDirectory() as d:
                    def make(j, engine_factory=None):
                        return Trainer(mode="paper", n_envs=n, dtype=F32, save_path=Path(d) / f"run{j}" / "tables", chunk_steps=64, max_num_episodes=budget,
                                       checkpoint_every=10**9, seed=attempt_seed(seed, j), engine_factory=engine_factory, **bench.CURRICULUM_KW)

                    def score(tr):
                        return landing_score(tr._double_q_learning_agent._padded(), 4096, 4, seed=SELECTION_SEED, device=0, quirks=Q_PAPER)
                    t0 = time.perf_counter()
                    res = curriculum_attempts(make, score, max_attempts=bench.CURRICULUM_ATTEMPTS, accept_touchdown=bench.CURRICULUM_ACCEPT_TOUCHDOWN, concurrency=conc)
                    wall = time.perf_counter() - t0
                    tabs = res["trainer"]._double_q_learning_agent._padded()
                    h = hashlib.sha256(b"".join(np.ascontiguousarray(t, dtype=np.float64).tobytes() for t in tabs)).hexdigest()[:16]
                    r = {"concurrency": conc, "seed": seed, "wall_s": wall, "attempts_flown": len(res["attempts"]), "chosen": res["chosen"], "accepted": res["accepted"],
                         "chosen_tables_sha16": h, "recipe": "bench.CURRICULUM_KW, 32 768 envs, sync_period None", "library_source_sha16": bench.lib_source_sha16()}
                    f.write(json.dumps(r) + "\n"); f.flush()
                    print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="both", choices=["throughput", "attempts", "both"])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--seeds", type=int, default=12)
    ap.add_argument("--out-dir", default=str(ROOT / "profiles"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    if a.what in ("throughput", "both"):
        throughput(Path(a.out_dir) / "population_throughput.jsonl", a.steps, a.warmup)
    if a.what in ("attempts", "both"):
        attempts(Path(a.out_dir) / "population_attempts.jsonl", a.seeds)


if __name__ == "__main__":
    main()
