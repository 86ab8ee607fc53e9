"""The checks of tests/test_gpu_tensor_env.py, run as a child process of their own: torch is imported FIRST here (it brings its own HIP runtime, which has to
be the one the process uses), then the package.  Prints one JSON report line; any failed check ends the process with a non-zero status and its message.

  closed loop   TensorEnv at 192 envs, simulation_config(working_curriculum_step=4, dtype=F32) with the paper quirks (case A of tests/model_checks.py), the
                reference's stage-4 tables as float64 tensors on the GPU.  The policy is the greedy rule of dql_device.hpp's agent_predict / argmax3, written with
                comparisons: q_k = (qa[s, k] + qb[s, k]) / 2 in float64; action 0, action 1 if q_1 > q_0, action 2 if q_2 > the larger of the two; code 2 in
                reset periods.  Periods 0 .. 320.  Per env, code and length of its first two episodes are gathered ON THE DEVICE from done, code and step_count
                and must == ops.score(..., episodes=2, max_steps=320, log=True): ep_code, ep_steps and by_code.  A view read before its step ran, or a step that
                read its actions before the policy wrote them, flies other episodes.  Run once per ordering mechanism ("stream", "sync").
  twin          every tensor TensorEnv.step returns == Engine.step_outputs() / obs() / get_fields() of a twin engine fed the same actions through the host,
                for both obs dtypes, with a reset_envs(mask) against the twin's reset(mask) on the way.
"""
import json
import sys
from pathlib import Path

import torch  # first

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from dql_multirotor_landing_amd import ops  # noqa: E402
from dql_multirotor_landing_amd.config import DqlConfig, F32, Q_PAPER, simulation_config  # noqa: E402
from dql_multirotor_landing_amd.engine import Engine  # noqa: E402
from dql_multirotor_landing_amd.tensor_env import OBS_FIELDS, TensorEnv  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "assets"
N, SEED, MAX_STEPS, EPISODES = 192, 11, 320, 2
NO_CODE = 0xFF


def stage4_tables():
    return tuple(np.load(GOLDEN / f).ravel().astype(np.float64) for f in ("Q_table_a.npy", "Q_table_b.npy"))


def greedy(q, idx_x, done):
    """q: float64 [945, 3] = (qa + qb) / 2 on the device; the arg-max with the device code's tie rule, by comparisons; code 2 where the period will be a reset"""
    s = idx_x.long().clamp(min=0)  # a fresh env has no state yet (-1): its period is a reset period
    q0, q1, q2 = q[s, 0], q[s, 1], q[s, 2]
    one = q1 > q0
    best = torch.where(one, q1, q0)
    a = torch.where(q2 > best, torch.full_like(s, 2), one.long())
    return torch.where(done.bool(), torch.full_like(a, 2), a).to(torch.uint8)


def closed_loop(ordering):
    cfg = lambda: simulation_config(working_curriculum_step=4, dtype=F32, quirks=Q_PAPER)
    qa, qb = stage4_tables()
    env = TensorEnv(cfg(), N, seed=SEED, ordering=ordering)
    dev = env.device
    q = ((torch.from_numpy(qa).to(dev) + torch.from_numpy(qb).to(dev)) / 2).reshape(-1, 3)
    ep_code = torch.full((EPISODES, N), NO_CODE, dtype=torch.uint8, device=dev)
    ep_steps = torch.zeros((EPISODES, N), dtype=torch.int32, device=dev)
    finished = torch.zeros(N, dtype=torch.long, device=dev)
    idx_x = torch.full((N,), -1, dtype=torch.int32, device=dev)
    done = torch.ones(N, dtype=torch.uint8, device=dev)  # period 0 is every env's reset period
    for _ in range(MAX_STEPS + 1):
        _, _, done, info = env.step(greedy(q, idx_x, done))
        idx_x = info["idx_x"]
        new = done.bool() & (finished < EPISODES)
        for e in range(EPISODES):  # selects, no indexing by a mask: nothing here makes the host wait for the device
            m = new & (finished == e)
            ep_code[e] = torch.where(m, info["code"].to(torch.uint8), ep_code[e])
            ep_steps[e] = torch.where(m, info["step_count"], ep_steps[e])
        finished = finished + new.long()
    got_code, got_steps, bad = ep_code.cpu().numpy(), ep_steps.cpu().numpy().astype(np.uint16), int(info["bad_actions"].item())
    used = env.ordering
    env.close()
    want = ops.score(cfg(), qa, qb, N, SEED, episodes=EPISODES, max_steps=MAX_STEPS, log=True)
    assert bad == 0, f"{bad} actions of the policy were out of range"
    assert (want["ep_code"] != NO_CODE).sum() >= N and len(set(want["ep_code"].ravel().tolist()) - {NO_CODE}) >= 2, "the scorer's episodes: too few, or of one kind"
    diff = np.argwhere((got_code != want["ep_code"]) | (got_steps != want["ep_steps"]))
    assert diff.size == 0, f"ordering {used}: episodes differ from dql_score's at (episode, env) {diff[:8].tolist()}"
    by_code = [int((got_code == k).sum()) for k in range(want["by_code"].shape[1] - 1)] + [int((got_code == NO_CODE).sum())]
    assert by_code == want["by_code"][0].tolist(), (by_code, want["by_code"][0].tolist())
    return {"asked": ordering, "ran": used, "by_code": by_code, "steps_sum": int(got_steps.astype(np.int64).sum())}


def twin(obs_dtype, dtype):
    n, periods = 320, 70
    cfg = lambda: DqlConfig(dtype=dtype, t_max=3.0)
    env, eng = TensorEnv(cfg(), n, seed=5, obs_dtype=obs_dtype), Engine(cfg(), n, seed=5)
    npt = np.float32 if obs_dtype == torch.float32 else np.float64
    names = eng.field_names()
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    seen_done = 0

    def compare(what):
        so = eng.step_outputs()
        reals, _ = eng.get_fields()
        row = np.stack([reals[names.index(f)] for f in OBS_FIELDS], axis=1).astype(npt)
        o6 = eng.obs()
        assert np.array_equal(row[:, [0, 4, 1, 5, 2, 6]].T, o6.astype(npt))
        got = {"obs": env.obs, "reward": env.reward, "done": env.done, **env.info}
        want = {"obs": row, "reward": so["reward"].astype(npt), "done": so["done"], "code": so["code"], "idx_x": so["idx_x"], "idx_y": so["idx_y"],
                "step_count": so["step_count"], "was_reset": so["was_reset"], "cumulative_reward": so["cumulative_reward"].astype(npt), "bad_actions": np.zeros(1, np.int64)}
        for k, w in want.items():
            t = got[k].cpu().numpy()
            assert t.dtype == w.dtype and t.shape == w.shape and t.tobytes() == w.tobytes(), f"{what}: {k} differs from the twin engine's"
        return int(so["done"].sum())

    obs = env.reset()
    assert obs is env.obs and tuple(obs.shape) == (n, 8) and obs.dtype == obs_dtype and obs.device == env.device
    eng.reset(); eng.step(np.full(n, 2, np.uint8))
    compare("reset")
    for p in range(periods):
        act = torch.randint(0, 3, (n,), generator=g, dtype=torch.uint8)
        out = env.step(act.to(env.device))
        assert out[0] is env.obs and out[1] is env.reward and out[2] is env.done and out[3] is env.info
        eng.step(act.numpy())
        seen_done += compare(f"period {p}")
        if p == 20:
            mask = torch.rand(n, generator=g) < 0.3
            env.reset_envs(mask.to(env.device))
            eng.reset(mask.numpy().astype(np.uint8))
    assert seen_done > 0, "no episode ended on the twin engine"
    for bad in (act, act.to(env.device)[:-1], act.to(env.device).to(torch.int32)):  # a host tensor, a wrong shape, a wrong dtype
        try:
            env.step(bad)
        except ValueError:
            continue
        raise AssertionError("a wrong action tensor was accepted")
    env.close(); eng.close()
    return seen_done


def main():
    from dql_multirotor_landing_amd.config import F64
    report = {"torch": torch.__version__, "closed_loop": [closed_loop("stream"), closed_loop("sync")]}
    report["twin_done"] = [twin(torch.float32, F32), twin(torch.float64, F32), twin(torch.float32, F64)]
    print("TENSOR_ENV_REPORT " + json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
