"""`TensorEnv`: the vectorised landing environment with every input and output a torch tensor on the GPU, so that a policy that lives there — a network, a
table held as a tensor — closes the act / step / observe loop without a copy to the host and without a host wait.

This is the only module of the package that imports torch; `import dql_multirotor_landing_amd` does not import it.  torch ships its own HIP runtime and that
runtime has to be the one the process uses, so torch must be imported BEFORE libdql_hip.so is loaded: import this module (or torch) first.  A `TensorEnv` made in
a process that loaded the library first is refused.

    import torch
    from dql_multirotor_landing_amd.tensor_env import TensorEnv
    env = TensorEnv(cfg, 4096)
    obs = env.reset()                                   # [n, 8] on cuda:0
    obs, reward, done, info = env.step(actions)         # actions: uint8 CUDA tensor [n], the codes of Engine.step

`step` is `Engine.step_dev` on the action tensor's memory followed by `Engine.view_dev` into the adapter's own tensors (include/dql.h dql_view_dev).  Auto-reset
is the step kernel's own: the period after a done one is a reset period, the action is ignored in it and `was_reset` is set; nothing is added here.

EVERY TENSOR RETURNED IS THE ADAPTER'S OWN BUFFER AND IS OVERWRITTEN BY THE NEXT CALL (as Engine.step_outputs_view's arrays are): clone what must survive.

Ordering needs no host wait (`ordering="stream"`): the engine's stream is wrapped as a torch.cuda.ExternalStream; before a step it waits for torch's current
stream (the policy that wrote the actions), after the view torch's current stream waits for it (whoever reads the outputs).  The action tensor is kept referenced
until the next step.  `ordering="sync"` synchronises on either side instead; it is chosen by itself when the ExternalStream cannot be made (`TensorEnv.ordering`
says which one runs).
"""
from __future__ import annotations

import torch

from . import _lib
from .config import DqlConfig, F32, F64
from .engine import Engine

OBS_FIELDS = Engine.VIEW_OBS_FIELDS
HOLD = 2  # the action code flown in reset(): it is ignored in a reset period


class TensorEnv:
    def __init__(self, cfg: DqlConfig, n_envs: int, seed: int = 42, device: int = 0, obs_dtype=torch.float32, ordering: str = "stream"):
        if _lib._lib is not None and not _lib.torch_came_first:  # recorded by _lib.load()
            raise RuntimeError("libdql_hip.so was loaded before torch in this process: torch ships its own HIP runtime, which must be the one the process uses. "
                               "Import torch (or dql_multirotor_landing_amd.tensor_env) before anything loads the library")
        if obs_dtype not in (torch.float32, torch.float64):
            raise ValueError("obs_dtype must be torch.float32 or torch.float64")
        if ordering not in ("stream", "sync"):
            raise ValueError('ordering must be "stream" (an ExternalStream around the engine\'s stream) or "sync" (a synchronise on either side)')
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU is visible to torch (there is no CPU fallback)")
        self.device = torch.device("cuda", int(device))
        self.n = int(n_envs)
        self.obs_dtype = obs_dtype
        with torch.cuda.device(self.device):
            torch.cuda.current_stream()  # torch's runtime owns the device before the library asks for it
            self.engine = Engine(cfg, self.n, seed=seed, device=int(device))
        self.ordering = ordering
        self._ext = None
        if ordering == "stream":
            try:
                self._ext = torch.cuda.ExternalStream(self.engine.stream_handle(), device=self.device)
            except Exception:  # no such class, or the handle is refused: the synchronising form
                self.ordering = "sync"
        n, dev = self.n, self.device
        self.obs = torch.zeros((n, _lib.VIEW_OBS), dtype=obs_dtype, device=dev)
        self.reward = torch.zeros(n, dtype=obs_dtype, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.info = {"code": torch.zeros(n, dtype=torch.int8, device=dev), "idx_x": torch.zeros(n, dtype=torch.int32, device=dev),
                     "idx_y": torch.zeros(n, dtype=torch.int32, device=dev), "step_count": torch.zeros(n, dtype=torch.int32, device=dev),
                     "was_reset": torch.zeros(n, dtype=torch.uint8, device=dev), "cumulative_reward": torch.zeros(n, dtype=obs_dtype, device=dev),
                     "bad_actions": torch.zeros(1, dtype=torch.int64, device=dev)}  # one word: out-of-range actions flown as "hold" so far (not cleared here)
        self._view = dict(real_dtype=F32 if obs_dtype == torch.float32 else F64, obs=self.obs.data_ptr(), reward=self.reward.data_ptr(), done=self.done.data_ptr(),
                          cumulative_reward=self.info["cumulative_reward"].data_ptr(), idx_x=self.info["idx_x"].data_ptr(), idx_y=self.info["idx_y"].data_ptr(),
                          step_count=self.info["step_count"].data_ptr(), was_reset=self.info["was_reset"].data_ptr(), code=self.info["code"].data_ptr(),
                          bad_actions=self.info["bad_actions"].data_ptr())
        self._hold = torch.full((n,), HOLD, dtype=torch.uint8, device=dev)
        self._actions = self._mask = None  # the caller's tensors the engine's stream may still be reading
        torch.cuda.current_stream(dev).synchronize()  # the buffers above are filled before the engine's stream first touches them

    # ---- ordering: the engine's stream after torch's current stream, and back ----
    def _engine_after_torch(self):
        if self._ext is not None:
            self._ext.wait_stream(torch.cuda.current_stream(self.device))
        else:
            torch.cuda.current_stream(self.device).synchronize()

    def _torch_after_engine(self):
        if self._ext is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._ext)
        else:
            self.engine.sync()

    def _check(self, t, what, dtypes):
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype not in dtypes or tuple(t.shape) != (self.n,) or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {' or '.join(str(d) for d in dtypes)} tensor of shape ({self.n},) on {self.device}")

    def _step(self, actions):
        self._engine_after_torch()
        self.engine.step_dev(actions.data_ptr())
        self._actions = actions  # kept until the next step: the step kernel reads it on the engine's stream
        self.engine.view_dev(**self._view)
        self._torch_after_engine()

    # ---- the environment ----
    def reset(self):
        """every env re-enters (as TrainingLandingEnv.reset: one agent period of simulation); returns obs [n, 8]"""
        self.engine.reset()
        self._step(self._hold)
        return self.obs

    def step(self, actions):
        """actions: uint8 CUDA tensor [n], ax | ay << 2 with ax, ay in 0 (increase), 1 (decrease), 2 (hold), checked by the step kernel (info["bad_actions"]).
        Returns (obs [n, 8], reward [n], done [n] uint8, info) — the adapter's own tensors, overwritten by the next call."""
        self._check(actions, "actions", (torch.uint8,))
        self._step(actions)
        return self.obs, self.reward, self.done, self.info

    def reset_envs(self, mask):
        """mark the envs where `mask` (uint8 or bool CUDA tensor [n]) is non-zero for reset; the reset is flown by the next step"""
        self._check(mask, "mask", (torch.uint8, torch.bool))
        self._engine_after_torch()
        self.engine.reset_dev(mask.data_ptr())
        self._mask = mask
        self._torch_after_engine()

    def close(self):
        if getattr(self, "engine", None) is not None:
            self.engine.sync()
            self.engine.close()
            self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
