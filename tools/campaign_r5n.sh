#!/bin/bash
# round 5, attempts: bench.py's curriculum leg with up to 6 whole curricula per seed (first accepted kept), 12 seeds, and the training script's --attempts
set -e
O=${1:?usage: bash tools/campaign_r5n.sh OUT_DIR}; mkdir -p $O
python3 bench.py --full --gpus 1 --steps 200 --warmup 20 --small-envs 0 --large-envs 0 --no-f64-block --cpu-steps 60 > $O/bench_attempts.json 2> $O/bench_attempts.err
cp bench_detail.json $O/bench_attempts_detail.json 2>/dev/null || true
python3 scripts/training.py --recipe bench --envs 32768 --attempts 4 --out $O/train_out > $O/training_attempts.json 2> $O/training_attempts.err
python3 -m pytest tests/test_gpu_dropin.py -q -m gpu -x -k "evaluation or simulation or greedy" > $O/pytest.log 2>&1
