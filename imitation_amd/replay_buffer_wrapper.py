"""`policies/replay_buffer_wrapper.py`: `ReplayBufferRewardWrapper` relabels the rewards of transitions when they are
SAMPLED from a replay ring, so that a row collected under last iteration's reward model is trained on under the current
one (the reference's `train_preference_comparisons` / `train_adversarial` scripts give every off-policy learner this
buffer with `reward_fn=functools.partial(reward_net.predict_processed, update_stats=False)`).

The rows live in device memory (`dqn.ReplayBuffer`) and the learners' update kernels read `table.reward[idx]`, so the
wrapper keeps a second float32 column of the ring's row count, `relabelled`, and its `table` is a view that shares
`obs / next_obs / action / done` with the inner table and whose `.reward` is that column; the environment rewards stored
in `wrapper.replay_buffer.table.reward` stay untouched, as in the reference. `DQN.train`, `TD3.train` and `SAC.train`
call the wrapper between their index draws and the update (`OffPolicyAlgorithm._run_updates`):

* device path -- `reward_fn` is the bound `predict_processed` of a `reward_nets.RewardNet` (possibly inside a
  `functools.partial` whose only keyword is `update_stats`) and the call is a pure row function (`device_plan`): all
  `G * B` sampled rows of the `train` call are relabelled at their ring rows before ONE update over all `G` steps, in one
  `ia_replay_relabel` launch (csrc/relabel.hip, fp32 MFMA) where the kernel covers the net, else in one
  `ia_replay_relabel_general` launch (any stack; one thread per row, the forward in float64, so the stored reward is the
  rounding of the float64 forward); `IA_RELABEL_FUSED=0` in the environment forces the general kernel;
* per-step path -- any other callable (and a `NormalizedRewardNet` with `update_stats=True`, whose statistics move with
  every call): per gradient step the step's rows go to host arrays, `reward_fn` is called exactly as the reference's
  `sample` calls it, the result is scattered and the update runs for that one step.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Callable, Optional, Tuple

import numpy as np
import torch as th

from imitation_amd import _lib as L
from imitation_amd.cnn_policy import _is_image_space
from imitation_amd.dqn import ReplayBuffer, ReplayBufferSamples, _Table
from imitation_amd.networks import RunningNorm
from imitation_amd.reward_nets import BasicRewardNet, NormalizedRewardNet, PredictProcessedWrapper, RewardNet


def fused_enabled() -> bool:
    """`IA_RELABEL_FUSED=0` sends every shape to the general kernel."""
    return os.environ.get("IA_RELABEL_FUSED", "1") != "0"


def device_plan(reward_fn: Callable) -> Optional[Tuple[BasicRewardNet, Optional[RunningNorm]]]:
    """`(BasicRewardNet, output norm or None)` when `reward_fn(state, action, next_state, done)` is, row by row, that net's
    stack in eval mode followed by the frozen output norm -- what the device path computes; None: the per-step path.

    Accepted: the bound `predict_processed` of a `RewardNet`, bare or in a `functools.partial` with no positional argument
    and no keyword but `update_stats`; the chain below it made of exactly `PredictProcessedWrapper` / `NormalizedRewardNet`
    (`type(...) is`: a subclass may override `predict_processed` / `predict` / `predict_th`) down to exactly one
    `BasicRewardNet`. A `NormalizedRewardNet` reached through `predict_processed` counts only with `update_stats=False`
    (the default, True, moves its statistics with every call); below a plain `PredictProcessedWrapper` the chain is
    walked through `predict`, which passes every wrapper by."""
    fn, update_stats = reward_fn, True
    if isinstance(fn, functools.partial):
        if fn.args or set(fn.keywords) - {"update_stats"}:
            return None
        update_stats = fn.keywords.get("update_stats", True)
        fn = fn.func
    net = getattr(fn, "__self__", None)
    if not isinstance(net, RewardNet) or getattr(fn, "__func__", None) is not type(net).predict_processed:
        return None
    out_norm, via_predict = None, False
    while True:
        if any(k in vars(net) for k in ("predict_processed", "predict", "predict_th", "forward", "_forward_table")):
            return None   # (patched on the instance)
        cls = type(net)
        if cls is BasicRewardNet:
            return net, out_norm
        if cls is NormalizedRewardNet:
            if not via_predict:
                if update_stats is not False or out_norm is not None:
                    return None   # (an inner one is called without `update_stats`: its statistics move)
                out_norm = net.normalize_output_layer
        elif cls is PredictProcessedWrapper:
            via_predict = True    # `RewardNet.predict_processed` -> `predict` -> `base.predict`
        else:
            return None
        net = net.base


class _TableView:
    """A `_Table`-shaped view of the inner table whose `.reward` is the wrapper's relabelled column."""

    def __init__(self, inner: _Table, reward: th.Tensor):
        self.rows, self.obs_dim, self.act_dim, self.frames = inner.rows, inner.obs_dim, inner.act_dim, inner.frames
        self.obs, self.next_obs, self.action, self.done = inner.obs, inner.next_obs, inner.action, inner.done
        self.reward = reward

    pointers = _Table.pointers


class ReplayBufferRewardWrapper(ReplayBuffer):
    """Relabel the rewards in transitions sampled from a `ReplayBuffer` (`policies/replay_buffer_wrapper.py:26-103`)."""

    def __init__(self, buffer_size: int, observation_space, action_space, *, replay_buffer_class, reward_fn: Callable,
                 **kwargs):
        assert replay_buffer_class is ReplayBuffer, "only ReplayBuffer is supported"
        if _is_image_space(observation_space):
            raise NotImplementedError("ReplayBufferRewardWrapper over an image space is not implemented: the relabel "
                                      "kernels read float32 rows, an image ring holds uint8 frames")
        self.frames = False
        # (dict observations: the inner buffer refuses anything but a flat Box)
        self.replay_buffer = replay_buffer_class(buffer_size, observation_space, action_space, **kwargs)
        self.reward_fn = reward_fn
        # (the base class's fields are the inner buffer's: a second table is never allocated)
        inner = self.replay_buffer
        self.observation_space, self.action_space = inner.observation_space, inner.action_space
        self.obs_dim, self.act_dim, self.device, self.n_envs = inner.obs_dim, inner.act_dim, inner.device, inner.n_envs
        self.index, self.buffer_size = inner.index, inner.buffer_size
        self.handle_timeout_termination = inner.handle_timeout_termination
        self.reward_source = None
        self.relabelled = th.zeros(inner.table.rows, device=self.device)
        self.table = _TableView(inner.table, self.relabelled)
        self.relabel_launches = {"fused": 0, "general": 0, "host": 0}   # relabelling passes so far, by path (tests)
        self._args = None
        self._general_ws: Optional[th.Tensor] = None

    @property
    def pos(self) -> int:
        return self.replay_buffer.index.pos

    @pos.setter
    def pos(self, pos: int) -> None:
        self.replay_buffer.index.pos = pos

    @property
    def full(self) -> bool:
        return self.replay_buffer.index.full

    @full.setter
    def full(self, full: bool) -> None:
        self.replay_buffer.index.full = full

    def size(self) -> int:
        return self.replay_buffer.size()

    def add(self, *args, **kwargs) -> None:
        self.replay_buffer.add(*args, **kwargs)

    def sample_rows(self, batch_size: int):
        return self.replay_buffer.sample_rows(batch_size)

    def _get_samples(self):
        raise NotImplementedError("_get_samples() is intentionally not implemented."
                                  "This method should not be called.")

    # ---- what `reward_fn` sees: the reference's `_samples_to_reward_fn_input` -------------------------------------------
    def _host_rewards(self, samples: ReplayBufferSamples) -> np.ndarray:
        return np.asarray(self.reward_fn(state=samples.observations.cpu().numpy(), action=samples.actions.cpu().numpy(),
                                         next_state=samples.next_observations.cpu().numpy(),
                                         done=samples.dones.cpu().numpy()))

    def sample(self, *args, **kwargs) -> ReplayBufferSamples:
        samples = self.replay_buffer.sample(*args, **kwargs)
        rewards = th.as_tensor(self._host_rewards(samples)).reshape(samples.rewards.shape).to(samples.rewards.device)
        return ReplayBufferSamples(samples.observations, samples.actions, samples.next_observations, samples.dones, rewards)

    # ---- the learners' hook ---------------------------------------------------------------------------------------------
    def plan(self) -> Optional[Tuple[BasicRewardNet, Optional[RunningNorm]]]:
        """`device_plan(reward_fn)` when the net also lives on the ring's device and reads the ring's row layout."""
        p = device_plan(self.reward_fn)
        if p is None:
            return None
        base, out_norm = p
        A = self.act_dim if self.act_dim is not None else int(self.action_space.n)
        if base.device != self.relabelled.device or base.obs_dim != self.obs_dim or base.act_dim != A:
            return None
        return p

    def fused_ok(self, base: BasicRewardNet, out_norm: Optional[RunningNorm]) -> bool:
        nrm = base.mlp.norm
        return (fused_enabled() and (nrm is None or nrm.is_chan) and
                bool(L.load().ia_replay_relabel_ok(C.byref(base.mlp.desc), base.obs_dim, base.act_dim,
                                                   *[int(f) for f in base.flags])))

    def relabel_for_train(self, idx_dev: th.Tensor) -> bool:
        """Device path: the rows `idx_dev` (int64, any shape: all the minibatches of a `train` call) relabelled at their
        ring rows. False (nothing done): `reward_fn` takes the per-step path (`relabel_step`)."""
        p = self.plan()
        if p is None:
            return False
        base, out_norm = p
        idx = idx_dev.reshape(-1)
        if self.fused_ok(base, out_norm):
            self._relabel_fused(base, out_norm, idx)
        else:
            self._relabel_general(base, out_norm, idx)
        return True

    def _relabel_args(self, base: BasicRewardNet, out_norm: Optional[RunningNorm], idx: th.Tensor):
        """The argument record of both kernels; refilled when a buffer it points to has moved."""
        t, mlp = self.replay_buffer.table, base.mlp
        nrm = mlp.norm
        key = (id(base), mlp.flat.data_ptr(), None if nrm is None else nrm.running_mean.data_ptr(),
               None if out_norm is None else out_norm.running_mean.data_ptr())
        if self._args is None or self._args[0] != key:
            a = L.ReplayRelabelArgs()
            a.obs, a.next_obs, a.done, a.ring_rows = L.ptr(t.obs), L.ptr(t.next_obs), L.ptr(t.done), t.rows
            a.act_f32 = None if t.act_dim is None else L.ptr(t.action)
            a.act_i64 = L.ptr(t.action) if t.act_dim is None else None
            a.obs_dim, a.act_dim = base.obs_dim, base.act_dim
            a.use_state, a.use_action, a.use_next_state, a.use_done = (int(f) for f in base.flags)
            a.desc, a.params = C.pointer(mlp.desc), L.ptr(mlp.flat)
            if nrm is not None:
                a.norm_mean, a.norm_var, a.norm_eps = L.ptr(nrm.running_mean), L.ptr(nrm.running_var), float(nrm.eps)
            if out_norm is not None:
                a.out_mean, a.out_var = L.ptr(out_norm.running_mean), L.ptr(out_norm.running_var)
                a.out_eps = float(out_norm.eps)
            a.reward = L.ptr(self.relabelled)
            self._args = (key, a, base)   # (`base` kept: the record points into its descriptor)
        a = self._args[1]
        a.idx, a.n = L.ptr(idx), idx.numel()
        return a

    def _relabel_fused(self, base: BasicRewardNet, out_norm: Optional[RunningNorm], idx: th.Tensor) -> None:
        a = self._relabel_args(base, out_norm, idx)
        L.check(L.load().ia_replay_relabel(C.byref(a), L.stream()), "ia_replay_relabel")
        self.relabel_launches["fused"] += 1

    def _relabel_general(self, base: BasicRewardNet, out_norm: Optional[RunningNorm], idx: th.Tensor) -> None:
        """Any stack, one launch: one thread per row, the forward in float64 (`ia_replay_relabel_general`)."""
        a = self._relabel_args(base, out_norm, idx)
        need = int(L.load().ia_replay_relabel_general_ws_doubles(C.byref(base.mlp.desc), idx.numel()))
        if self._general_ws is None or self._general_ws.numel() < need:
            self._general_ws = th.empty(need, dtype=th.float64, device=self.relabelled.device)
        nrm = base.mlp.norm
        L.check(L.load().ia_replay_relabel_general(
            C.byref(a), 0.0 if nrm is None else float(nrm.eps), 0.0 if out_norm is None else float(out_norm.eps),
            L.ptr(self._general_ws), self._general_ws.numel(), L.stream()), "ia_replay_relabel_general")
        self.relabel_launches["general"] += 1

    def relabel_step(self, rows: np.ndarray, idx_dev: th.Tensor) -> None:
        """Per-step path: one gradient step's rows to the host, `reward_fn` as the reference's `sample` calls it, the
        result scattered to the rows."""
        samples = self.replay_buffer._gather(self.replay_buffer.table, np.asarray(rows, np.int64))
        rewards = th.as_tensor(self._host_rewards(samples)).reshape(-1).to(th.float32).to(self.relabelled.device)
        self.relabelled[idx_dev.reshape(-1)] = rewards
        self.relabel_launches["host"] += 1
