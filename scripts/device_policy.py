#!/usr/bin/env python3
"""A policy that lives on the GPU flies the vectorised simulator without a copy to the host: the worked example of
dql_multirotor_landing_amd.tensor_env.TensorEnv.

    python scripts/device_policy.py [--envs 4096] [--steps 600] [--random] [--tables DIR] [--sync]

The policy is the published stage-4 tables (tests/golden/assets) held as torch tensors on the GPU: it gathers the three action values of every env's state
`idx_x` and applies the greedy rule of the device code (q_k = (qa + qb) / 2 in float64; action 0, action 1 if q_1 > q_0, action 2 if q_2 > the larger of the
two — comparisons, no library tie rule).  --random flies a uniform policy instead.  Actions are written by torch kernels, read by the step kernel, the outputs
written by the view kernel and read by torch kernels: one stream waits for the other, the host waits for nobody until the end (--sync: a synchronise on either
side of every step instead).  Prints the touchdown share of the episodes that ended and env-steps/s as one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch  # before the package loads the HIP library: torch's HIP runtime has to be the process's

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def greedy_policy(qa, qb):
    """tables [2835] float64 on the device -> policy(idx_x, done) -> uint8 actions; code 2 where the next period is a reset period (the action is ignored there)"""
    q = ((qa + qb) / 2).reshape(-1, 3)

    def policy(idx_x, done):
        s = idx_x.long().clamp(min=0)  # an env that has not flown yet has no state (-1)
        q0, q1, q2 = q[s, 0], q[s, 1], q[s, 2]
        one = q1 > q0
        a = torch.where(q2 > torch.where(one, q1, q0), torch.full_like(s, 2), one.long())
        return torch.where(done.bool(), torch.full_like(a, 2), a).to(torch.uint8)
    return policy


def random_policy(n, device, seed=0):
    g = torch.Generator(device=device); g.manual_seed(seed)
    return lambda idx_x, done: torch.randint(0, 3, (n,), generator=g, device=device, dtype=torch.uint8)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--random", action="store_true", help="a uniform random policy instead of the tables' greedy one")
    ap.add_argument("--tables", default=str(ROOT / "tests" / "golden" / "assets"))
    ap.add_argument("--sync", action="store_true", help="order the two streams with a synchronise on either side of every step instead of stream waits")
    ap.add_argument("--seed", type=int, default=123)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    import numpy as np
    from dql_multirotor_landing_amd.config import CHECK_NAMES, F32, Q_PAPER, simulation_config
    from dql_multirotor_landing_amd.tensor_env import TensorEnv
    env = TensorEnv(simulation_config(working_curriculum_step=4, dtype=F32, quirks=Q_PAPER), a.envs, seed=a.seed, ordering="sync" if a.sync else "stream")
    dev = env.device
    if a.random:
        policy = random_policy(a.envs, dev)
    else:
        qa, qb = (torch.from_numpy(np.load(Path(a.tables) / f).ravel().astype(np.float64)).to(dev) for f in ("Q_table_a.npy", "Q_table_b.npy"))
        policy = greedy_policy(qa, qb)
    by_code = torch.zeros(len(CHECK_NAMES), dtype=torch.long, device=dev)
    decisions = torch.zeros((), dtype=torch.long, device=dev)
    env.reset()
    done, info = env.done, env.info
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        _, _, done, info = env.step(policy(info["idx_x"], done))
        by_code.index_add_(0, info["code"].long().clamp(0, len(CHECK_NAMES) - 1), done.long())  # the codes of the episodes that ended in this period
        decisions += (info["was_reset"] == 0).sum()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    h = by_code.tolist()
    episodes = sum(h)
    print(json.dumps({"policy": "random" if a.random else "greedy on the stage-4 tables", "envs": a.envs, "steps": a.steps, "ordering": env.ordering, "episodes": episodes,
                      "touchdown_share": (h[CHECK_NAMES.index("TERMINAL_CONTACT")] / episodes) if episodes else None,
                      "by_code": {CHECK_NAMES[k]: h[k] for k in range(len(CHECK_NAMES)) if h[k]}, "env_steps_per_s": int(decisions.item()) / dt,
                      "bad_actions": int(info["bad_actions"].item())}))
    env.close()
