#!/usr/bin/env python3
"""The reference's curriculum training (`Trainer.curriculum_training`: one env, one agent, update after every step) for many independent seeds at once,
one learner per GPU lane (dql_multirotor_landing_amd/ensemble.py).

    python scripts/ensemble_training.py --learners 4096 --seed 42 [--launched] [--levels 5] [--episodes 50000] --out run.npz

--launched: the parameters the reference's manager node ran with under roslaunch (config.as_launched_config) instead of the launch file's.
Writes every learner's tables and, per level, its first-promotion episode (-1: the episode budget ran out first)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dql_multirotor_landing_amd.config import F32, F64, Q_REFERENCE, as_launched_config, training_config  # noqa: E402
from dql_multirotor_landing_amd.ensemble import SequentialEnsemble, curriculum  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--learners", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--launched", action="store_true")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=50000, help="episode budget per level and learner")
    ap.add_argument("--f64", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dtype = F64 if a.f64 else F32
    cfg = as_launched_config(dtype=dtype, quirks=Q_REFERENCE) if a.launched else training_config(0, dtype=dtype, quirks=Q_REFERENCE)
    ens = SequentialEnsemble(cfg, a.learners, seed=a.seed, device=a.device, max_episodes=a.episodes)
    try:
        def report(e, h):
            p = h["promotion_episode"]
            print(json.dumps({"level": h["level"], "periods": h["periods"], "promoted": int((p >= 0).sum()), "of": int(p.size),
                              "median_promotion_episode": None if not (p >= 0).any() else int(np.median(p[p >= 0]))}), flush=True)
        hist = curriculum(ens, levels=a.levels, max_episodes=a.episodes, on_level=report)
        qa, qb, cnt = ens.get_tables()
        np.savez_compressed(a.out, Q_table_a=qa, Q_table_b=qb, state_action_counter=cnt,
                            promotion_episode=np.stack([h["promotion_episode"] for h in hist]), periods=np.array([h["periods"] for h in hist]))
    finally:
        ens.close()


if __name__ == "__main__":
    main()
