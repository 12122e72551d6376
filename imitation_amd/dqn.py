"""What SQIL needs of stable-baselines3's DQN (`algorithms/sqil.py:12-19,77-83`): `DQN`, `DQNPolicy` ("MlpPolicy"),
`QNetwork`, SB3's `ReplayBuffer` and the off-policy loop -- a restatement of stable-baselines3 2.2.x from its documented
behaviour ([SB3 dqn/dqn.py, dqn/policies.py, common/off_policy_algorithm.py, common/buffers.py]).

Layout, as everywhere in this package: every index decision (ring position, sampled rows, exploration
coin, random actions) is made on the host with SB3's own draw sequence from NumPy's GLOBAL stream; the learner ring and
the expert table live in device memory and rows never come back -- a step uploads its transition and reads back the
arg-max, a `train` call uploads ONE int64 index array for all its gradient steps and reads back one block of statistics.

The update itself is `ia_dqn_update` (csrc/dqn.hip): all gradient steps of a `train` call in one launch of one workgroup,
for `net_arch=[H, H]`, H in {32, 64}, ReLU, D <= 64, A <= 16, batch <= 256. Every other Q-net runs the same update from
the general kernels (`ia_gather_rows`, `ia_mlp_forward` twice, `ia_dqn_td_loss`, `ia_mlp_backward` + `ia_reduce_partials`,
`ia_clip_grad_norm`, `ia_dqn_adam_step`); `IA_DQN_FUSED=0` in the environment forces that path (tests, tools).

Image observations ("CnnPolicy"): `CnnQNetwork` is SB3's `QNetwork` over `NatureCNN` on the trunk of
`cnn_policy.NatureCnnTrunk`; the ring and the expert table of an image space hold uint8 frames, and the update's third
route, `DQNPolicy.update_frames`, assembles each step's minibatch with one `ia_dqn_assemble_u8` launch (csrc/dqn_frames.hip).
"""
from __future__ import annotations

import collections
import copy
import ctypes as C
import os
import sys
import time
import warnings
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch as th
from torch import nn

from imitation_amd import _lib as L
from imitation_amd import logger as imit_logger
from imitation_amd import spaces
from imitation_amd.cnn_policy import NatureCNN, NatureCnnTrunk, _is_image_space
from imitation_amd.networks import require_device
from imitation_amd.policies import FlattenExtractor
from imitation_amd.ppo import _CallbackList, _NullCallback, _schedule, set_random_seed


def fused_enabled() -> bool:
    """`IA_DQN_FUSED=0` sends every shape down the general path."""
    return os.environ.get("IA_DQN_FUSED", "1") != "0"


def get_linear_fn(start: float, end: float, end_fraction: float):
    """[SB3 utils.get_linear_fn]: from `start` to `end` while `1 - progress_remaining` goes from 0 to `end_fraction`."""

    def func(progress_remaining: float) -> float:
        if (1 - progress_remaining) > end_fraction:
            return end
        return start + (1 - progress_remaining) * (end - start) / end_fraction

    return func


class ReplayBufferSamples(NamedTuple):
    """[SB3 type_aliases.ReplayBufferSamples]"""
    observations: th.Tensor
    actions: th.Tensor
    next_observations: th.Tensor
    dones: th.Tensor
    rewards: th.Tensor


class ReplayIndex:
    """The index logic of [SB3 buffers.ReplayBuffer], host only (no tensor, no GPU): a ring of
    `max(buffer_size // n_envs, 1)` positions of `n_envs` rows each; `add` returns the position it wrote and wraps;
    `sample` makes SB3's two draws from NumPy's GLOBAL stream (`np.random.randint(0, upper, size=b)`, then
    `np.random.randint(0, high=n_envs, size=(b,))`); the row of (position, env) in a flat table is
    `position * n_envs + env`."""

    def __init__(self, buffer_size: int, n_envs: int = 1):
        self.n_envs = int(n_envs)
        self.buffer_size = max(int(buffer_size) // self.n_envs, 1)
        self.pos = 0
        self.full = False

    def size(self) -> int:
        return self.buffer_size if self.full else self.pos

    def add(self) -> int:
        at = self.pos
        self.pos += 1
        if self.pos == self.buffer_size:
            self.full = True
            self.pos = 0
        return at

    def fill(self) -> None:
        """The state after `buffer_size` adds (the expert table: one add per demonstration)."""
        self.pos, self.full = 0, True

    def sample(self, batch_size: int) -> Tuple[np.ndarray, np.ndarray]:
        upper_bound = self.buffer_size if self.full else self.pos
        batch_inds = np.random.randint(0, upper_bound, size=batch_size)
        env_indices = np.random.randint(0, high=self.n_envs, size=(len(batch_inds),))
        return batch_inds, env_indices

    def rows(self, batch_inds: np.ndarray, env_indices: np.ndarray) -> np.ndarray:
        return batch_inds.astype(np.int64) * self.n_envs + env_indices.astype(np.int64)


class _Table:
    """Flat device table of transitions: obs / next_obs [N, D] float32 -- or uint8 for an image space (`frames`: D = C*H*W
    bytes per row, the frames as the environment hands them over) --, action int64 [N] (Discrete) or float32 [N, A]
    (Box, `act_dim` = A), reward, done float32 [N]."""

    def __init__(self, rows: int, obs_dim: int, device, act_dim: Optional[int] = None, frames: bool = False):
        self.rows, self.obs_dim, self.act_dim, self.frames = int(rows), int(obs_dim), act_dim, bool(frames)
        self.obs_np = np.uint8 if self.frames else np.float32
        obs_dtype = th.uint8 if self.frames else th.float32
        self.obs = th.zeros(self.rows, obs_dim, dtype=obs_dtype, device=device)
        self.next_obs = th.zeros(self.rows, obs_dim, dtype=obs_dtype, device=device)
        if act_dim is None:
            self.action = th.zeros(self.rows, dtype=th.int64, device=device)
        else:
            self.action = th.zeros(self.rows, int(act_dim), device=device)
        self.reward = th.zeros(self.rows, device=device)
        self.done = th.zeros(self.rows, device=device)

    def write(self, lo: int, obs, next_obs, action, reward, done) -> None:
        n = len(obs)
        act = (np.int64, (n,)) if self.act_dim is None else (np.float32, (n, self.act_dim))
        if self.frames and not (np.asarray(obs).dtype == np.uint8 and np.asarray(next_obs).dtype == np.uint8):
            raise ValueError("a frame table stores uint8 frames as they come: the observations must be uint8 arrays")
        for dst, src, dtype, shape in ((self.obs, obs, self.obs_np, (n, -1)), (self.next_obs, next_obs, self.obs_np, (n, -1)),
                                       (self.action, action) + act, (self.reward, reward, np.float32, (n,)),
                                       (self.done, done, np.float32, (n,))):
            dst[lo:lo + n].copy_(th.from_numpy(np.array(src, dtype).reshape(shape)))


def _device(device) -> th.device:
    return th.device("cuda" if device == "auto" else device)


class ReplayBuffer:
    """[SB3 buffers.ReplayBuffer] for flat Box observations (float32 rows) or uint8 image observations (uint8 rows of
    C*H*W bytes, `frames`) and Discrete or flat Box actions, its rows in device memory.
    `handle_timeout_termination`: a `done` that is a time-limit truncation does not cut the bootstrap (the product
    `done * (1 - timeout)` SB3 forms when sampling is formed when the row is stored)."""

    def __init__(self, buffer_size: int, observation_space, action_space, device="auto", n_envs: int = 1,
                 optimize_memory_usage: bool = False, handle_timeout_termination: bool = True):
        if optimize_memory_usage:
            raise NotImplementedError("optimize_memory_usage is not implemented")
        if not isinstance(observation_space, spaces.Box) or not isinstance(action_space, (spaces.Discrete, spaces.Box)):
            raise NotImplementedError("the replay buffer holds flat Box observations and Discrete or Box actions")
        self.observation_space, self.action_space = observation_space, action_space
        self.obs_dim = int(np.prod(observation_space.shape))
        # Box actions: a float32 [rows, A] column; Discrete: the int64 [rows] column
        self.act_dim = int(np.prod(action_space.shape)) if isinstance(action_space, spaces.Box) else None
        self.device = _device(device)
        self.n_envs = int(n_envs)
        self.index = ReplayIndex(buffer_size, n_envs)
        self.buffer_size = self.index.buffer_size
        self.handle_timeout_termination = handle_timeout_termination
        # an image space's frames stay uint8 end to end: uint8 [rows, C*H*W] tables, no float round trip
        self.frames = _is_image_space(observation_space)
        self.table = _Table(self.buffer_size * self.n_envs, self.obs_dim, self.device, self.act_dim, frames=self.frames)
        # `RewardStepSource`: `add` then ignores its `reward` and stores the step with one `ia_offpolicy_step` launch
        self.reward_source: Optional["RewardStepSource"] = None

    @property
    def pos(self) -> int:
        return self.index.pos

    @property
    def full(self) -> bool:
        return self.index.full

    def size(self) -> int:
        return self.index.size()

    def add(self, obs, next_obs, action, reward, done, infos) -> None:
        done = np.asarray(done, np.float32).reshape(-1)
        if self.handle_timeout_termination:
            timeouts = np.array([info.get("TimeLimit.truncated", False) for info in infos], np.float32)
            done = done * (1 - timeouts)
        if self.reward_source is not None:
            self.reward_source.require_staged()   # (before the ring position moves)
            self.reward_source.store_step(self.index.add() * self.n_envs, obs, next_obs, action, done)
            return
        reward = np.array(np.broadcast_to(np.asarray(reward, np.float32), (self.n_envs,)))
        at = self.index.add()
        self.table.write(at * self.n_envs, obs, next_obs, action, reward, done)

    def sample_rows(self, batch_size: int) -> Tuple[np.ndarray, int]:
        """The flat rows of one minibatch and how many of them (the first) index the learner ring: all here."""
        return self.index.rows(*self.index.sample(batch_size)), batch_size

    def expert_table(self) -> Optional[_Table]:
        return None

    def _gather(self, table: _Table, rows: np.ndarray) -> ReplayBufferSamples:
        idx = th.from_numpy(rows).to(self.device)
        obs, next_obs = table.obs[idx], table.next_obs[idx]
        if self.frames:   # (uint8 [b, C, H, W], as SB3's buffer returns them)
            shape = (-1,) + tuple(self.observation_space.shape)
            obs, next_obs = obs.reshape(shape), next_obs.reshape(shape)
        return ReplayBufferSamples(obs, table.action[idx].reshape(-1, table.act_dim or 1), next_obs,
                                   table.done[idx].reshape(-1, 1), table.reward[idx].reshape(-1, 1))

    def sample(self, batch_size: int, env=None) -> ReplayBufferSamples:
        """[SB3 ReplayBuffer.sample] as tensors (the training loop itself passes `sample_rows` to the kernels)."""
        if env is not None:
            raise NotImplementedError("VecNormalize is not implemented")
        rows, _ = ReplayBuffer.sample_rows(self, batch_size)
        return self._gather(self.table, rows)


class RewardStepSource:
    """The reward source of a learner ring under a learned reward (`AdversarialTrainer` installs it on
    `ReplayBuffer.reward_source`): one `ia_offpolicy_step` launch per environment step (csrc/offpolicy.hip) relabels the
    step's rows and writes them to the ring, to a per-round device tile (what the trainer's own replay ring is filled
    from) and to a pinned host tile of rewards (the wrapper's episode bookkeeping), instead of a reward prediction with
    its read-back followed by five small copies.

    The step's rows go in through a ring of `SLOTS` pinned host records; a record is rewritten only after the launch that
    read it has completed (one event per record, waited on only when the ring of records wraps). `RewardVecEnvWrapper`
    stages the action the environment saw and the raw dones (`stage`); `ReplayBuffer.add` passes the learner's view of the
    step (`store_step`). With a net whose `forward_plan` the kernel covers the reward is computed in the launch; any other
    net's `predict_th` stays on the device and the launch reads it from there."""

    SLOTS = 8

    def __init__(self, ring: "ReplayBuffer", reward_net, slots: Optional[int] = None, tile_steps: int = 64):
        if ring.frames:
            raise NotImplementedError("a learned reward on a uint8 frame ring is not implemented (ia_offpolicy_step reads "
                                      "and writes float32 rows)")
        self.ring, self.net = ring, reward_net
        self.device = ring.device
        self.n, self.od = ring.n_envs, ring.obs_dim
        self.discrete = ring.act_dim is None
        self.A = 1 if self.discrete else ring.act_dim
        lib = L.load()
        plan = reward_net.forward_plan()
        self.base, self.out_act = None, L.ACT_NONE
        if plan is not None:
            base, out_act = plan
            if lib.ia_offpolicy_step_ok(C.byref(base.mlp.desc), base.obs_dim, base.act_dim, *[int(f) for f in base.flags]):
                self.base, self.out_act = base, out_act
        self.act_dim = self.base.act_dim if self.base is not None else self.A
        n, od, A = self.n, self.od, self.A
        pin = lambda *shape, dtype=th.float32: th.zeros(*shape, dtype=dtype).pin_memory()
        self.slots = []
        for _ in range(int(slots or self.SLOTS)):
            rec = dict(obs=pin(n, od), next_obs=pin(n, od), dones=pin(n, dtype=th.uint8), ring_done=pin(n),
                       act=pin(n, dtype=th.int64) if self.discrete else pin(n, A),
                       ring_act=None if self.discrete else pin(n, A))
            rec["np"] = {k: v.numpy() for k, v in rec.items() if v is not None}
            self.slots.append(rec)
        self.events: List[Optional[th.cuda.Event]] = [None] * len(self.slots)
        self.launches = 0          # `ia_offpolicy_step` calls so far (tests count them)
        self._slot_checked = -1
        self._staged = -1          # the `launches` count at the latest `stage`
        self.event_waits = 0       # records found still in flight when the ring of records wrapped
        self.tile_step = 0         # steps in the round tile
        self._alloc_tile(int(tile_steps))
        self._args: List[Any] = [None] * len(self.slots)   # per record: (key, `OffpolicyStepArgs` with its pointers filled in)

    def _alloc_tile(self, steps: int) -> None:
        n, od, dev = self.n, self.od, self.device
        old = getattr(self, "tile_obs", None)
        olds = (self.tile_obs, self.tile_next, self.tile_act, self.tile_dones, self.rewards_host) if old is not None else None
        self.tile_cap = steps
        self.tile_obs = th.zeros((steps + 1) * n, od, device=dev)   # (one spare row block: `store_from_rollout`'s view)
        self.tile_next = th.zeros(steps * n, od, device=dev)
        self.tile_act = (th.zeros(steps * n, dtype=th.int64, device=dev) if self.discrete
                         else th.zeros(steps * n, self.A, device=dev))
        self.tile_dones = th.zeros(steps * n, dtype=th.uint8, device=dev)
        self.rewards_host = th.zeros(steps, n).pin_memory()
        self.rewards_np = self.rewards_host.numpy()
        if olds is not None:   # a longer round than any before: the written rows move over (rare; one synchronisation)
            th.cuda.current_stream().synchronize()
            for new, o in zip((self.tile_obs, self.tile_next, self.tile_act, self.tile_dones, self.rewards_host), olds):
                m = min(len(o), len(new))
                new[:m].copy_(o[:m])
            th.cuda.current_stream().synchronize()

    def reward_row(self) -> np.ndarray:
        """The row of the pinned reward tile the NEXT stored step fills (valid once that launch has completed)."""
        if self.tile_step == self.tile_cap:
            self._alloc_tile(2 * self.tile_cap)
        return self.rewards_np[self.tile_step]

    def _slot(self):
        k = self.launches % len(self.slots)
        if self._slot_checked != self.launches:   # (once per step: `stage` and `store_step` fill the same record)
            self._slot_checked = self.launches
            ev = self.events[k]
            if ev is not None and not ev.query():
                self.event_waits += 1
                ev.synchronize()
        return k, self.slots[k]["np"]

    def stage(self, actions, dones) -> None:
        """The action the environment executed (what the discriminator sees) and the raw dones of the step."""
        _, rec = self._slot()
        rec["act"][...] = np.asarray(actions).reshape(rec["act"].shape)
        rec["dones"][...] = np.asarray(dones).reshape(-1)
        self._staged = self.launches

    def require_staged(self) -> None:
        """A step can be stored only behind its `stage`: the record's discriminator action and raw dones would otherwise be
        those of an earlier step."""
        if self._staged != self.launches:
            raise RuntimeError("ReplayBuffer.add on a ring with a reward source needs the step staged by the "
                               "RewardVecEnvWrapper the trainer built (stage() was not called for this step)")

    def store_step(self, ring_row: int, obs, next_obs, ring_action, ring_done) -> None:
        self.require_staged()
        k, rec = self._slot()
        n = self.n
        rec["obs"][...] = np.asarray(obs).reshape(n, -1)
        rec["next_obs"][...] = np.asarray(next_obs).reshape(n, -1)
        rec["ring_done"][...] = ring_done
        if not self.discrete:
            rec["ring_act"][...] = np.asarray(ring_action).reshape(n, -1)
        if self.tile_step == self.tile_cap:
            self._alloc_tile(2 * self.tile_cap)
        rewards_in = None
        if self.base is None:   # any other net: its prediction stays on the device
            so, sa = tuple(self.ring.observation_space.shape), tuple(self.ring.action_space.shape)
            rewards_in = self.net.predict_th(rec["obs"].reshape((n,) + so), rec["act"].reshape((n,) + sa),
                                             rec["next_obs"].reshape((n,) + so), rec["dones"].astype(bool)).contiguous()
        a = self._slot_args(k)
        if rewards_in is not None:
            a.rewards_in = rewards_in.data_ptr()
        a.ring_row, a.tile_row = int(ring_row), self.tile_step * n
        a.rewards_host = self.rewards_host.data_ptr() + 4 * self.tile_step * n
        L.check(L.load().ia_offpolicy_step(C.byref(a), L.stream()), "ia_offpolicy_step")
        if self.events[k] is None:
            self.events[k] = th.cuda.Event()
        self.events[k].record()
        self.last_event = self.events[k]
        self.launches += 1
        self.tile_step += 1

    def _slot_args(self, k: int):
        """The argument record of pinned record `k`; refilled when a buffer it points to has moved (a longer round tile,
        a reward net moved to another device)."""
        b = self.base
        nrm = None if b is None else b.mlp.norm
        key = (self.tile_obs.data_ptr(), None if b is None else b.mlp.flat.data_ptr(),
               None if nrm is None else nrm.running_mean.data_ptr())
        if self._args[k] is not None and self._args[k][0] == key:
            return self._args[k][1]
        slot, t, n, a = self.slots[k], self.ring.table, self.n, L.OffpolicyStepArgs()
        a.obs, a.next_obs = slot["obs"].data_ptr(), slot["next_obs"].data_ptr()
        a.act_i64 = slot["act"].data_ptr() if self.discrete else None
        a.act_f32 = None if self.discrete else slot["act"].data_ptr()
        a.ring_act_f32 = None if self.discrete else slot["ring_act"].data_ptr()
        a.dones, a.ring_done = slot["dones"].data_ptr(), slot["ring_done"].data_ptr()
        a.n, a.obs_dim, a.act_dim = n, self.od, self.act_dim
        if b is not None:
            a.use_state, a.use_action, a.use_next_state, a.use_done = (int(f) for f in b.flags)
            a.desc, a.params = C.pointer(b.mlp.desc), b.mlp.flat.data_ptr()
            a.norm_mean = None if nrm is None else nrm.running_mean.data_ptr()
            a.norm_var = None if nrm is None else nrm.running_var.data_ptr()
            a.norm_eps, a.out_act = (0.0 if nrm is None else float(nrm.eps)), self.out_act
        a.ring_obs, a.ring_next_obs = t.obs.data_ptr(), t.next_obs.data_ptr()
        a.ring_action_i64 = t.action.data_ptr() if self.discrete else None
        a.ring_action_f32 = None if self.discrete else t.action.data_ptr()
        a.ring_reward, a.ring_done_out, a.ring_rows = t.reward.data_ptr(), t.done.data_ptr(), t.rows
        a.tile_obs, a.tile_next_obs = self.tile_obs.data_ptr(), self.tile_next.data_ptr()
        a.tile_act_i64 = self.tile_act.data_ptr() if self.discrete else None
        a.tile_act_f32 = None if self.discrete else self.tile_act.data_ptr()
        a.tile_dones, a.tile_rows = self.tile_dones.data_ptr(), self.tile_cap * n
        self._args[k] = (key, a)
        return a

    def wait(self) -> None:
        """Until the latest launch has completed (its rewards are then in the pinned tile)."""
        if self.launches:
            self.last_event.synchronize()

    def rollout_view(self):
        """The round tile with the fields `buffer.ReplayBuffer.store_from_rollout` reads."""
        T, n = self.tile_step, self.n
        return _RoundTile(self.tile_obs[:(T + 1) * n], self.tile_next[:T * n], self.tile_act[:T * n].reshape(T * n, -1),
                          self.tile_dones[:T * n], T, n)

    def reset_tile(self) -> None:
        self.tile_step = 0


class _RoundTile(NamedTuple):
    obs: th.Tensor
    next_fixed: th.Tensor
    clipped: th.Tensor
    dones: th.Tensor
    buffer_size: int
    n_envs: int


def frame_reward_plan(reward_net):
    """(cnn_net, softplus) when `reward_net` is what the frame path's reward launch covers -- `modules.CnnRewardNet` over
    channel-first frames with `normalize_images`, plain or under GAIL's `RewardNetFromDiscriminatorLogit` --, else None."""
    from imitation_amd import modules
    net, softplus = reward_net, False
    if type(net) is modules.RewardNetFromDiscriminatorLogit:
        net, softplus = net.base, True
    if type(net) is not modules.CnnRewardNet or net.hwc_format or not net.normalize_images:
        return None
    return net, softplus


class FrameRewardStepSource:
    """`RewardStepSource` for a uint8 frame ring under a `modules.CnnRewardNet` (csrc/offpolicy_frames.hip): per environment
    step ONE `ia_offpolicy_frames_step` launch reads the step's frames once from a pinned host record and writes them to the
    learner's ring, to the uint8 round tile and, as channel-last fp32 through the byte table, to the reward CNN's input;
    the CNN runs under `no_grad` (`forward_nhwc`, the convolution ops); ONE `ia_offpolicy_frames_reward` launch selects
    the action's (and done's) output, applies GAIL's softplus and writes the rewards to the ring and to the pinned host
    reward tile. Same surface, same ring of pinned records with one event per record as `RewardStepSource`."""

    SLOTS = 8

    def __init__(self, ring: "ReplayBuffer", reward_net, slots: Optional[int] = None, tile_steps: int = 64):
        from imitation_amd import ops
        if not ring.frames or ring.act_dim is not None:
            raise TypeError("FrameRewardStepSource stores uint8 frames with Discrete actions (RewardStepSource stores "
                            "float32 rows)")
        require_device(ring.device)
        plan = frame_reward_plan(reward_net)
        if plan is None:
            raise NotImplementedError("the frame path's reward launch covers modules.CnnRewardNet(hwc_format=False) with "
                                      "normalize_images, plain or under GAIL's softplus; any other net takes the host path")
        self.ring, self.net = ring, reward_net
        self.cnn_net, self.softplus = plan
        self.device = ring.device
        self.n, self.od = ring.n_envs, ring.obs_dim
        self.shape = tuple(ring.observation_space.shape)          # (C, H, W)
        self.n_actions = int(ring.action_space.n)
        c = self.cnn_net
        self.S = int(c.use_state) + int(c.use_next_state)
        self.n_out = (self.n_actions if c.use_action else 1) * (2 if c.use_done else 1)
        self.lut = ops._byte_lut(self.device)
        C_, H, W = self.shape
        self.X = th.empty(self.n, H, W, C_ * self.S, device=self.device)
        n, od = self.n, self.od
        pin = lambda *shape, dtype=th.float32: th.zeros(*shape, dtype=dtype).pin_memory()
        self.slots = []
        for _ in range(int(slots or self.SLOTS)):
            rec = dict(obs=pin(n, od, dtype=th.uint8), next_obs=pin(n, od, dtype=th.uint8), dones=pin(n, dtype=th.uint8),
                       ring_done=pin(n), act=pin(n, dtype=th.int64))
            rec["np"] = {k: v.numpy() for k, v in rec.items()}
            self.slots.append(rec)
        self.events: List[Optional[th.cuda.Event]] = [None] * len(self.slots)
        self.launches = 0          # `ia_offpolicy_frames_step` calls so far (tests count them)
        self.reward_launches = 0   # `ia_offpolicy_frames_reward` calls so far
        self._slot_checked = -1
        self._staged = -1
        self.event_waits = 0
        self.tile_step = 0
        self._alloc_tile(int(tile_steps))
        self._args: List[Any] = [None] * len(self.slots)

    def _alloc_tile(self, steps: int) -> None:
        n, od, dev = self.n, self.od, self.device
        old = getattr(self, "tile_obs", None)
        olds = (self.tile_obs, self.tile_next, self.tile_act, self.tile_dones, self.rewards_host) if old is not None else None
        self.tile_cap = steps
        self.tile_obs = th.zeros(steps * n, od, dtype=th.uint8, device=dev)
        self.tile_next = th.zeros(steps * n, od, dtype=th.uint8, device=dev)
        self.tile_act = th.zeros(steps * n, dtype=th.int64, device=dev)
        self.tile_dones = th.zeros(steps * n, dtype=th.uint8, device=dev)
        self.rewards_host = th.zeros(steps, n).pin_memory()
        self.rewards_np = self.rewards_host.numpy()
        if olds is not None:   # a longer round than any before: the written rows move over (rare; one synchronisation)
            th.cuda.current_stream().synchronize()
            for new, o in zip((self.tile_obs, self.tile_next, self.tile_act, self.tile_dones, self.rewards_host), olds):
                m = min(len(o), len(new))
                new[:m].copy_(o[:m])
            th.cuda.current_stream().synchronize()

    def reward_row(self) -> np.ndarray:
        """The row of the pinned reward tile the NEXT stored step fills (valid once its reward launch has completed)."""
        if self.tile_step == self.tile_cap:
            self._alloc_tile(2 * self.tile_cap)
        return self.rewards_np[self.tile_step]

    def _slot(self):
        k = self.launches % len(self.slots)
        if self._slot_checked != self.launches:   # (once per step: `stage` and `store_step` fill the same record)
            self._slot_checked = self.launches
            ev = self.events[k]
            if ev is not None and not ev.query():
                self.event_waits += 1
                ev.synchronize()
        return k, self.slots[k]["np"]

    def stage(self, actions, dones) -> None:
        """The action the environment executed and the raw dones of the step."""
        _, rec = self._slot()
        rec["act"][...] = np.asarray(actions).reshape(rec["act"].shape)
        rec["dones"][...] = np.asarray(dones).reshape(-1)
        self._staged = self.launches

    def require_staged(self) -> None:
        if self._staged != self.launches:
            raise RuntimeError("ReplayBuffer.add on a ring with a reward source needs the step staged by the "
                               "RewardVecEnvWrapper the trainer built (stage() was not called for this step)")

    def store_step(self, ring_row: int, obs, next_obs, ring_action, ring_done) -> None:
        self.require_staged()
        k, rec = self._slot()
        n = self.n
        obs, next_obs = np.asarray(obs), np.asarray(next_obs)
        if obs.dtype != np.uint8 or next_obs.dtype != np.uint8:
            raise ValueError("a frame table stores uint8 frames as they come: the observations must be uint8 arrays")
        rec["obs"][...] = obs.reshape(n, -1)
        rec["next_obs"][...] = next_obs.reshape(n, -1)
        rec["ring_done"][...] = ring_done
        if self.tile_step == self.tile_cap:
            self._alloc_tile(2 * self.tile_cap)
        a = self._slot_args(k)
        a.ring_row, a.tile_row = int(ring_row), self.tile_step * n
        a.rewards_host = self.rewards_host.data_ptr() + 4 * self.tile_step * n
        lib, st = L.load(), L.stream()
        L.check(lib.ia_offpolicy_frames_step(C.byref(a), st), "ia_offpolicy_frames_step")
        with th.no_grad():
            out = self.cnn_net.cnn.forward_nhwc(self.X).contiguous()
        c = self.cnn_net
        L.check(lib.ia_offpolicy_frames_reward(C.byref(a), out.data_ptr(), self.n_out, None, self.n_actions,
                                               int(c.use_action), int(c.use_done), int(self.softplus), st),
                "ia_offpolicy_frames_reward")
        if self.events[k] is None:
            self.events[k] = th.cuda.Event()
        self.events[k].record()
        self.last_event = self.events[k]
        self.launches += 1
        self.reward_launches += 1
        self.tile_step += 1

    def _slot_args(self, k: int):
        """The argument record of pinned record `k`; refilled when the round tile has moved."""
        key = self.tile_obs.data_ptr()
        if self._args[k] is not None and self._args[k][0] == key:
            return self._args[k][1]
        slot, t, a = self.slots[k], self.ring.table, L.OffpolicyFramesArgs()
        a.obs, a.next_obs, a.act = slot["obs"].data_ptr(), slot["next_obs"].data_ptr(), slot["act"].data_ptr()
        a.dones, a.ring_done = slot["dones"].data_ptr(), slot["ring_done"].data_ptr()
        a.n, (a.C, a.H, a.W) = self.n, self.shape
        a.use_state, a.use_next_state = int(self.cnn_net.use_state), int(self.cnn_net.use_next_state)
        a.lut, a.X = self.lut.data_ptr(), self.X.data_ptr()
        a.ring_obs, a.ring_next_obs, a.ring_action = t.obs.data_ptr(), t.next_obs.data_ptr(), t.action.data_ptr()
        a.ring_reward, a.ring_done_out, a.ring_rows = t.reward.data_ptr(), t.done.data_ptr(), t.rows
        a.tile_obs, a.tile_next_obs = self.tile_obs.data_ptr(), self.tile_next.data_ptr()
        a.tile_act, a.tile_dones, a.tile_rows = self.tile_act.data_ptr(), self.tile_dones.data_ptr(), self.tile_cap * self.n
        self._args[k] = (key, a)
        return a

    def wait(self) -> None:
        """Until the latest reward launch has completed (its rewards are then in the pinned tile)."""
        if self.launches:
            self.last_event.synchronize()

    def rollout_view(self):
        """The round tile with the fields `buffer.FrameReplayBuffer.store_from_rollout` reads."""
        T, n = self.tile_step, self.n
        return _RoundTile(self.tile_obs[:T * n], self.tile_next[:T * n], self.tile_act[:T * n], self.tile_dones[:T * n], T, n)

    def reset_tile(self) -> None:
        self.tile_step = 0


class QNetwork:
    """[SB3 dqn.policies.QNetwork]: `create_mlp(features_dim, n_actions, net_arch, activation_fn)` over the flattened
    observation; parameters as one flat device vector in torch's `parameters()` order."""

    def __init__(self, observation_space, action_space, net_arch: List[int], activation_fn=nn.ReLU):
        if not isinstance(action_space, spaces.Discrete):
            raise NotImplementedError("DQN needs a Discrete action space")
        if not isinstance(observation_space, spaces.Box):
            raise NotImplementedError("the Q-network takes flat Box observations")
        if activation_fn not in (nn.ReLU, nn.Tanh):
            raise NotImplementedError(f"activation {activation_fn} is not implemented on the HIP path")
        self.observation_space, self.action_space = observation_space, action_space
        self.obs_dim, self.n_actions = int(np.prod(observation_space.shape)), int(action_space.n)
        self.net_arch, self.activation_fn = [int(h) for h in net_arch], activation_fn
        self.act = L.ACT_RELU if activation_fn is nn.ReLU else L.ACT_TANH
        self.dims = [self.obs_dim] + self.net_arch + [self.n_actions]
        if len(self.dims) - 1 > L.IA_MAX_LAYERS:
            raise NotImplementedError(f"at most {L.IA_MAX_LAYERS} layers")
        # CPU modules give torch's default initialisation AND its consumption of the global generator
        layers: List[nn.Module] = []
        for i in range(len(self.dims) - 1):
            layers.append(nn.Linear(self.dims[i], self.dims[i + 1]))
            if i < len(self.dims) - 2:
                layers.append(activation_fn())
        seq = nn.Sequential(*layers)
        self._names = [(k, tuple(v.shape)) for k, v in seq.state_dict().items()]
        self._flat = th.cat([p.detach().reshape(-1) for p in seq.parameters()]).contiguous()
        self.desc = L.mlp_desc(self.dims, self.act)

    @property
    def device(self) -> th.device:
        return self._flat.device

    def to(self, device):
        self._flat = self._flat.to(device).contiguous()
        return self

    def fused_shape(self) -> bool:
        return (len(self.net_arch) == 2 and self.net_arch[0] == self.net_arch[1] and self.net_arch[0] in (32, 64)
                and self.act == L.ACT_RELU and self.obs_dim <= 64 and self.n_actions <= 16)

    def parameters(self):
        off = 0
        for _, shape in self._names:
            n = int(np.prod(shape))
            yield self._flat[off:off + n].view(shape)
            off += n

    def state_dict(self) -> Dict[str, th.Tensor]:
        return {f"q_net.{k}": p for (k, _), p in zip(self._names, self.parameters())}

    def load_state_dict(self, sd) -> None:
        for (k, shape), p in zip(self._names, self.parameters()):
            p.copy_(th.as_tensor(sd[f"q_net.{k}"]).reshape(shape))

    def q_values(self, obs_dev: th.Tensor) -> Tuple[th.Tensor, Optional[th.Tensor]]:
        """Q [n, A] on device rows `obs_dev[n, D]`; with it the first arg-max per row where the act kernel covers the net
        (None otherwise: the caller takes it from Q)."""
        require_device(self.device)
        n = obs_dev.shape[0]
        q = th.empty(n, self.n_actions, device=self.device)
        if self.fused_shape() and fused_enabled():
            am = th.empty(n, dtype=th.int64, device=self.device)
            L.call("ia_dqn_q_values", self.obs_dim, self.net_arch[0], self.n_actions, L.ptr(self._flat), L.ptr(obs_dev), n,
                   L.ptr(q), L.ptr(am), L.stream())
            return q, am
        hidden = th.empty(max(1, n * sum(self.net_arch)), device=self.device)
        L.call("ia_mlp_forward", C.byref(self.desc), L.ptr(self._flat), L.ptr(obs_dev), self.obs_dim, n, L.ptr(hidden),
               L.ptr(q), L.ACT_NONE, L.stream())
        return q, None


class CnnQNetwork(NatureCnnTrunk):
    """[SB3 dqn.policies.QNetwork] over `NatureCNN(features_dim)` with SB3's default `net_arch=[]` behind it: `q_net` is
    one `Linear(features_dim, n_actions)`. Torch's default initialisation (DQN does no orthogonal re-init), modules built
    on the host in SB3's order (conv 0 / 2 / 4, linear.0, the head). Parameters: one flat fp32 buffer in the trunk's device
    layout (`cnn_policy.NatureCnnTrunk`); `state_dict` / `load_state_dict` permute to and from torch's layouts."""

    def __init__(self, observation_space, action_space, features_dim: int = 512):
        if not isinstance(action_space, spaces.Discrete):
            raise NotImplementedError("DQN needs a Discrete action space")
        if not _is_image_space(observation_space):
            raise ValueError("the CNN Q-network is for uint8 image spaces [C, H, W] with bounds 0 / 255")
        self.action_space = action_space
        self.n_actions = int(action_space.n)
        self.net_arch: List[int] = []
        self._init_trunk(observation_space, features_dim)
        cnn, linear = self._host_trunk()
        head = nn.Linear(self.features_dim, self.n_actions)
        self._set_flat(["features_extractor.cnn.0", "features_extractor.cnn.2", "features_extractor.cnn.4",
                        "features_extractor.linear.0", "q_net.0"], [cnn[0], cnn[2], cnn[4], linear[0], head], [])

    def to(self, device):
        self.device = th.device(device)
        self._flat = self._flat.to(self.device).contiguous()
        self._bufs, self._dgrad_idx = {}, {}
        if self.device.type == "cuda":
            self._resolve_conv1()
        return self

    def fused_shape(self) -> bool:
        return False

    def named_parameters(self):
        for i, name in enumerate(self._names):
            yield f"{name}.weight", self._to_torch_layout(i, self.w(i)).reshape(self._shapes[i])
            yield f"{name}.bias", self.b(i)

    def parameters(self):
        for _, p in self.named_parameters():
            yield p

    def state_dict(self) -> Dict[str, th.Tensor]:
        return dict(self.named_parameters())

    def load_state_dict(self, sd) -> None:
        for i, name in enumerate(self._names):
            w = th.as_tensor(sd[f"{name}.weight"]).to(self.device).float().reshape(self._shapes[i])
            self.w(i).copy_(self._to_device_layout(i, w).reshape(-1))
            self.b(i).copy_(th.as_tensor(sd[f"{name}.bias"]).to(self.device).float().reshape(-1))

    def grad_to_torch(self, grad: th.Tensor) -> Dict[str, th.Tensor]:
        """A flat vector in the parameters' device layout (a gradient, an Adam moment) under `state_dict`'s keys and
        layouts."""
        out = {}
        for i, name in enumerate(self._names):
            ow, nw, ob, nb = self._offsets[i]
            out[f"{name}.weight"] = self._to_torch_layout(i, grad[ow:ow + nw]).reshape(self._shapes[i])
            out[f"{name}.bias"] = grad[ob:ob + nb]
        return out

    def _head_buffers(self, B: int, d: Dict[str, th.Tensor]) -> None:
        d["q"] = th.empty(B, self.n_actions, device=self.device)
        d["dq"] = th.empty(B, self.n_actions, device=self.device)

    def forward(self, obs_u8: th.Tensor) -> Dict[str, th.Tensor]:
        """The batch buffers with `q` [B, A] = Q(obs, .) of device frames `obs_u8` uint8 [B, C, H, W] (and the activations
        `backward` needs)."""
        d = self._forward_trunk(obs_u8)
        F_, A = self.features_dim, self.n_actions
        self._gemm(0, d["feat"], F_, self.w(4), F_, d["q"], A, obs_u8.shape[0], A, F_, bias=self.b(4))
        return d

    def backward(self, B: int, grad: th.Tensor) -> None:
        """Adds to `grad` (flat, device layout) the parameter gradient of the loss whose gradient w.r.t. Q the caller left
        in the batch-`B` buffers' `dq`."""
        d = self._bufs[B]
        F_, A = self.features_dim, self.n_actions
        self._wgrad(4, d["dq"], B, A, d["feat"], F_, grad)
        self._gemm(1, d["dq"], A, self.w(4), F_, d["dfeat"], F_, B, F_, A, act=1, P=d["feat"], ldp=F_)
        self._backward_trunk(B, d, grad)


class DQNPolicy:
    """[SB3 dqn.policies.DQNPolicy]: `q_net`, then a separately initialised `q_net_target` that loads the online
    net's state, then Adam over the online parameters."""

    def __init__(self, observation_space, action_space, lr_schedule, net_arch: Optional[List[int]] = None,
                 activation_fn=nn.ReLU, features_extractor_class=FlattenExtractor, features_extractor_kwargs=None,
                 normalize_images: bool = True, optimizer_class=th.optim.Adam, optimizer_kwargs=None):
        if features_extractor_class not in (FlattenExtractor, NatureCNN):
            raise NotImplementedError("only the flatten extractor (MlpPolicy) and NatureCNN (CnnPolicy) are implemented")
        if optimizer_class is not th.optim.Adam:
            raise NotImplementedError("only torch.optim.Adam is implemented")
        self.observation_space, self.action_space = observation_space, action_space
        # image policy: NatureCNN over uint8 frames, the update's third route (`update_frames`)
        self.frames = features_extractor_class is NatureCNN
        if self.frames:
            if not _is_image_space(observation_space):
                raise ValueError("CnnPolicy is for uint8 image spaces [C, H, W] with bounds 0 / 255")
            if int(np.argmin(observation_space.shape)) != 0:
                raise NotImplementedError("channel-last image spaces are not implemented (there is no VecTransposeImage "
                                          "here): pass frames as [C, H, W]")
            if not normalize_images:
                raise NotImplementedError("normalize_images=False is not implemented: the first layer scales by 1 / 255")
            if net_arch not in (None, []):
                raise NotImplementedError("hidden layers behind NatureCNN are not implemented (SB3's CnnPolicy has none)")
            unknown = set(features_extractor_kwargs or {}) - {"features_dim"}
            if unknown:
                raise NotImplementedError(f"features_extractor_kwargs {sorted(unknown)} are not implemented")
        self.net_arch = [] if self.frames else [64, 64] if net_arch is None else list(net_arch)
        self.activation_fn = activation_fn
        self.optimizer_kwargs = dict(optimizer_kwargs or {})
        unknown = set(self.optimizer_kwargs) - {"betas", "eps", "weight_decay"}
        if unknown:
            raise NotImplementedError(f"optimizer_kwargs {sorted(unknown)} are not implemented")
        if self.frames:
            features_dim = int((features_extractor_kwargs or {}).get("features_dim", 512))
            self.q_net = CnnQNetwork(observation_space, action_space, features_dim)
            self.q_net_target = CnnQNetwork(observation_space, action_space, features_dim)
        else:
            self.q_net = QNetwork(observation_space, action_space, self.net_arch, activation_fn)
            self.q_net_target = QNetwork(observation_space, action_space, self.net_arch, activation_fn)
        self.q_net_target._flat.copy_(self.q_net._flat)
        self.lr = float(lr_schedule(1))
        self.betas = tuple(self.optimizer_kwargs.get("betas", (0.9, 0.999)))
        self.eps = float(self.optimizer_kwargs.get("eps", 1e-8))
        self.weight_decay = float(self.optimizer_kwargs.get("weight_decay", 0.0))
        self.exp_avg = th.zeros_like(self.q_net._flat)
        self.exp_avg_sq = th.zeros_like(self.q_net._flat)
        self.adam_steps = 0
        self.training = True
        self._ws: Dict[Any, Any] = {}

    @property
    def device(self) -> th.device:
        return self.q_net.device

    def to(self, device):
        self.q_net.to(device)
        self.q_net_target.to(device)
        self.exp_avg, self.exp_avg_sq = self.exp_avg.to(device), self.exp_avg_sq.to(device)
        self._ws = {}
        return self

    def set_training_mode(self, mode: bool) -> None:
        self.training = mode

    def parameters(self):
        yield from self.q_net.parameters()
        yield from self.q_net_target.parameters()

    def state_dict(self) -> Dict[str, th.Tensor]:
        out = {f"q_net.{k}": v for k, v in self.q_net.state_dict().items()}
        out.update({f"q_net_target.{k}": v for k, v in self.q_net_target.state_dict().items()})
        return out

    def load_state_dict(self, sd) -> None:
        self.q_net.load_state_dict({k[len("q_net."):]: v for k, v in sd.items() if k.startswith("q_net.")})
        self.q_net_target.load_state_dict(
            {k[len("q_net_target."):]: v for k, v in sd.items() if k.startswith("q_net_target.")})

    def q_values(self, observation: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Q and the greedy action of host observations (one upload, one read-back)."""
        if self.frames:   # the uint8 frames go up as they are; the arg-max is the first maximum, taken on the host
            frames = np.ascontiguousarray(observation)
            if frames.dtype != np.uint8:
                raise TypeError("image observations must be uint8 (the policy applies [SB3 preprocess_obs]: x / 255)")
            frames = frames.reshape((-1,) + tuple(self.observation_space.shape))
            qh = self.q_net.forward(th.from_numpy(frames).to(self.device))["q"].cpu().numpy()
            return qh, qh.argmax(axis=1).astype(np.int64)
        obs = np.ascontiguousarray(observation, np.float32).reshape(-1, self.q_net.obs_dim)
        q, am = self.q_net.q_values(th.from_numpy(obs).to(self.device))
        if am is None:
            qh = q.cpu().numpy()
            return qh, qh.argmax(axis=1).astype(np.int64)
        both = th.cat([q.reshape(-1), am.to(th.float32)]).cpu().numpy()   # (action indices < 2^24: exact as floats)
        n = len(obs)
        return both[:n * self.q_net.n_actions].reshape(n, -1), both[n * self.q_net.n_actions:].astype(np.int64)

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """[SB3 BasePolicy.predict]: the greedy action (`_predict` is the arg-max whatever `deterministic` says)."""
        self.set_training_mode(False)
        observation = np.asarray(observation)
        vectorized = observation.shape != tuple(self.observation_space.shape)
        _, actions = self.q_values(observation)
        if not vectorized:
            return actions[0], state
        return actions, state

    def polyak_update(self, tau: float) -> None:
        """[SB3 utils.polyak_update] of the target from the online parameters."""
        L.call("ia_polyak_update", L.ptr(self.q_net._flat), L.ptr(self.q_net_target._flat), self.q_net._flat.numel(),
               float(tau), L.stream())

    # ---- the update -------------------------------------------------------------------------------------------------
    # Routing by measured cost (tools/sqil_step_bench.py --sweep, H = 64, microseconds per gradient step inside a 16-step
    # call): the one-workgroup kernel walks the batch in 16-row groups, 27 + 15.6 per group at D = 4 and 35 + 25.3 per group
    # at D = 64 (taken as linear in D in between); the general path's launches cost 104 - 113 whatever the batch. A shape
    # whose estimate exceeds the limit takes the general path (D = 4: batches above 64; D = 64: above 32 -- the largest
    # batches at which the kernel was measured ahead; at the next group the two paths tie).
    FUSED_COST_LIMIT_US = 100.0

    def fused_cost_us(self, batch_size: int) -> float:
        D = self.q_net.obs_dim
        return 26.5 + D / 8.0 + -(-int(batch_size) // 16) * (15.0 + 0.16 * D)

    def fused_ok(self, batch_size: int) -> bool:
        q = self.q_net
        return (fused_enabled() and q.fused_shape() and self.weight_decay == 0.0 and
                self.fused_cost_us(batch_size) <= self.FUSED_COST_LIMIT_US and
                bool(L.load().ia_dqn_update_ok(q.obs_dim, q.net_arch[0], q.n_actions, int(batch_size))))

    def _adam_scalars(self, lr: float, n_steps: int) -> np.ndarray:
        b1, b2 = self.betas
        out = np.empty((n_steps, 2), np.float32)
        for s in range(n_steps):
            t = self.adam_steps + s + 1
            out[s, 0] = lr / (1.0 - b1 ** t)
            out[s, 1] = (1.0 - b2 ** t) ** 0.5
        return out

    def update_fused(self, ring: _Table, expert: Optional[_Table], idx_dev: th.Tensor, n_new: int, n_steps: int,
                     batch_size: int, gamma: float, max_grad_norm: float, lr: float, stats: th.Tensor,
                     grad_out: Optional[th.Tensor] = None) -> None:
        """`n_steps` gradient steps in one launch (`ia_dqn_update`); `idx_dev` int64 [n_steps, batch_size]."""
        q = self.q_net
        scal = np.ascontiguousarray(self._adam_scalars(lr, n_steps))
        e = expert
        rc = L.load().ia_dqn_update(
            q.obs_dim, q.net_arch[0], q.n_actions, int(batch_size), int(n_new), int(n_steps), L.ptr(q._flat),
            L.ptr(self.q_net_target._flat), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), L.ptr(ring.obs),
            L.ptr(ring.next_obs), L.ptr(ring.action), L.ptr(ring.reward), L.ptr(ring.done),
            None if e is None else L.ptr(e.obs), None if e is None else L.ptr(e.next_obs),
            None if e is None else L.ptr(e.action), None if e is None else L.ptr(e.reward),
            None if e is None else L.ptr(e.done), L.ptr(idx_dev), float(gamma), float(max_grad_norm), float(self.betas[0]),
            float(self.betas[1]), self.eps, scal.ctypes.data, L.ptr(stats), L.ptr(grad_out), L.stream())
        L.check(rc, "ia_dqn_update")
        self.adam_steps += n_steps

    def _general_ws(self, B: int):
        key = ("general", B)
        if key not in self._ws:
            q, dev = self.q_net, self.device
            hid = max(1, B * sum(q.net_arch))
            n = q._flat.numel()
            splits = max(1, min(64, B // 256))
            self._ws[key] = dict(
                obs=th.empty(B, q.obs_dim, device=dev), nxt=th.empty(B, q.obs_dim, device=dev),
                act=th.empty(B, dtype=th.int64, device=dev), rew=th.empty(B, device=dev), done=th.empty(B, device=dev),
                hidden=th.empty(hid, device=dev), hidden_t=th.empty(hid, device=dev), dhidden=th.empty(hid, device=dev),
                q=th.empty(B, q.n_actions, device=dev), qt=th.empty(B, q.n_actions, device=dev),
                dq=th.empty(B, q.n_actions, device=dev), terms=th.empty(B, device=dev), splits=splits,
                partials=th.empty(splits, n, device=dev), grads=th.empty(n, device=dev))
        return self._ws[key]

    def update_general(self, ring: _Table, expert: Optional[_Table], idx_dev: th.Tensor, n_new: int, n_steps: int,
                       batch_size: int, gamma: float, max_grad_norm: float, lr: float, stats: th.Tensor,
                       grad_out: Optional[th.Tensor] = None) -> None:
        """The same steps from the general kernels, one launch sequence per step."""
        q, B, st = self.q_net, int(batch_size), L.stream()
        w = self._general_ws(B)
        scal = self._adam_scalars(lr, n_steps)
        n = q._flat.numel()
        D = q.obs_dim
        idx_ptr, stats_ptr = idx_dev.data_ptr(), stats.data_ptr()
        for s in range(n_steps):
            for table, lo, cnt in ((ring, 0, n_new), (expert, n_new, B - n_new)):
                if cnt == 0:
                    continue
                ip = idx_ptr + 8 * (s * B + lo)
                L.call("ia_gather_rows", L.ptr(table.obs), ip, cnt, D, w["obs"].data_ptr() + 4 * lo * D, st)
                L.call("ia_gather_rows", L.ptr(table.next_obs), ip, cnt, D, w["nxt"].data_ptr() + 4 * lo * D, st)
                # (int64 actions travel as pairs of 32-bit words: the gather moves bits)
                L.call("ia_gather_rows", L.ptr(table.action), ip, cnt, 2, w["act"].data_ptr() + 8 * lo, st)
                L.call("ia_gather_rows", L.ptr(table.reward), ip, cnt, 1, w["rew"].data_ptr() + 4 * lo, st)
                L.call("ia_gather_rows", L.ptr(table.done), ip, cnt, 1, w["done"].data_ptr() + 4 * lo, st)
            L.call("ia_mlp_forward", C.byref(q.desc), L.ptr(q._flat), L.ptr(w["obs"]), D, B, L.ptr(w["hidden"]),
                   L.ptr(w["q"]), L.ACT_NONE, st)
            L.call("ia_mlp_forward", C.byref(q.desc), L.ptr(self.q_net_target._flat), L.ptr(w["nxt"]), D, B,
                   L.ptr(w["hidden_t"]), L.ptr(w["qt"]), L.ACT_NONE, st)
            L.call("ia_dqn_td_loss", L.ptr(w["q"]), L.ptr(w["qt"]), L.ptr(w["act"]), L.ptr(w["rew"]), L.ptr(w["done"]), B,
                   q.n_actions, float(gamma), L.ptr(w["dq"]), L.ptr(w["terms"]), stats_ptr + 8 * s, st)
            L.call("ia_mlp_backward", C.byref(q.desc), L.ptr(q._flat), L.ptr(w["obs"]), D, B, L.ptr(w["hidden"]),
                   L.ptr(w["dq"]), L.ptr(w["dhidden"]), L.ptr(w["partials"]), w["splits"], None, st)
            L.call("ia_reduce_partials", L.ptr(w["partials"]), w["splits"], n, 1.0, 0, L.ptr(w["grads"]), st)
            L.call("ia_clip_grad_norm", L.ptr(w["grads"]), n, float(max_grad_norm), stats_ptr + 8 * s + 4, None, st)
            L.call("ia_dqn_adam_step", L.ptr(q._flat), L.ptr(w["grads"]), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), n,
                   float(self.betas[0]), float(self.betas[1]), self.eps, self.weight_decay, float(scal[s, 0]),
                   float(scal[s, 1]), st)
        if grad_out is not None:
            grad_out.copy_(w["grads"])
        self.adam_steps += n_steps

    def _frames_ws(self, B: int):
        key = ("frames", B)
        if key not in self._ws:
            q, dev = self.q_net, self.device
            n = q._flat.numel()
            self._ws[key] = dict(
                obs=th.empty(B, q.obs_dim, dtype=th.uint8, device=dev), nxt=th.empty(B, q.obs_dim, dtype=th.uint8, device=dev),
                act=th.empty(B, dtype=th.int64, device=dev), rew=th.empty(B, device=dev), done=th.empty(B, device=dev),
                terms=th.empty(B, device=dev), grads=th.empty(n, device=dev),
                clip_ws=th.empty(int(L.load().ia_clip_grad_norm_ws_floats()), device=dev))
        return self._ws[key]

    @staticmethod
    def check_rows(rows: np.ndarray, n_new: int, ring: _Table, expert: Optional[_Table]) -> None:
        """Every sampled row of a `train` call against its table's row count, on the host, before anything is launched
        (`ia_dqn_assemble_u8` moves whole frames by these indices)."""
        rows = np.asarray(rows).reshape(len(rows), -1)
        for part, table, what in ((rows[:, :n_new], ring, "learner ring"), (rows[:, n_new:], expert, "expert table")):
            if part.size == 0:
                continue
            if table is None:
                raise ValueError(f"rows are drawn from the {what}, which does not exist")
            if int(part.min()) < 0 or int(part.max()) >= table.rows:
                raise IndexError(f"a sampled row lies outside the {what} ({table.rows} rows)")

    def update_frames(self, ring: _Table, expert: Optional[_Table], idx_dev: th.Tensor, n_new: int, n_steps: int,
                      batch_size: int, gamma: float, max_grad_norm: float, lr: float, stats: th.Tensor,
                      grad_out: Optional[th.Tensor] = None) -> None:
        """The steps of an image policy, per step: one `ia_dqn_assemble_u8` launch (the minibatch from the two uint8 frame
        tables), the online trunk's forward on `obs`, the target trunk's on `next_obs`, `ia_dqn_td_loss`, the trunk's
        backward seeded with `dq` into a flat gradient, `ia_clip_grad_norm`, `ia_dqn_adam_step`. The caller has checked the
        rows against the tables (`check_rows`)."""
        require_device(self.device)
        if not (ring.frames and (expert is None or expert.frames)):
            raise TypeError("update_frames reads uint8 frame tables")
        q, qt, B, st = self.q_net, self.q_net_target, int(batch_size), L.stream()
        w = self._frames_ws(B)
        scal = self._adam_scalars(lr, n_steps)
        n, D, e = q._flat.numel(), q.obs_dim, expert
        shape = (B,) + tuple(self.observation_space.shape)
        obs, nxt = w["obs"].view(shape), w["nxt"].view(shape)
        idx_ptr, stats_ptr = idx_dev.data_ptr(), stats.data_ptr()
        for s in range(n_steps):
            L.call("ia_dqn_assemble_u8", L.ptr(ring.obs), L.ptr(ring.next_obs), L.ptr(ring.action), L.ptr(ring.reward),
                   L.ptr(ring.done), ring.rows, None if e is None else L.ptr(e.obs), None if e is None else L.ptr(e.next_obs),
                   None if e is None else L.ptr(e.action), None if e is None else L.ptr(e.reward),
                   None if e is None else L.ptr(e.done), 0 if e is None else e.rows, idx_ptr + 8 * s * B, B, int(n_new), D,
                   L.ptr(w["obs"]), L.ptr(w["nxt"]), L.ptr(w["act"]), L.ptr(w["rew"]), L.ptr(w["done"]), st)
            d = q.forward(obs)
            dt = qt.forward(nxt)
            L.call("ia_dqn_td_loss", L.ptr(d["q"]), L.ptr(dt["q"]), L.ptr(w["act"]), L.ptr(w["rew"]), L.ptr(w["done"]), B,
                   q.n_actions, float(gamma), L.ptr(d["dq"]), L.ptr(w["terms"]), stats_ptr + 8 * s, st)
            w["grads"].zero_()
            q.backward(B, w["grads"])
            L.call("ia_clip_grad_norm", L.ptr(w["grads"]), n, float(max_grad_norm), stats_ptr + 8 * s + 4, L.ptr(w["clip_ws"]),
                   st)
            L.call("ia_dqn_adam_step", L.ptr(q._flat), L.ptr(w["grads"]), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), n,
                   float(self.betas[0]), float(self.betas[1]), self.eps, self.weight_decay, float(scal[s, 0]),
                   float(scal[s, 1]), st)
        if grad_out is not None:
            grad_out.copy_(w["grads"])
        self.adam_steps += n_steps

    def update(self, ring: _Table, expert: Optional[_Table], idx_dev: th.Tensor, n_new: int, n_steps: int,
               batch_size: int, gamma: float, max_grad_norm: float, lr: float, stats: th.Tensor,
               grad_out: Optional[th.Tensor] = None) -> None:
        """`update_frames` for an image policy; else the fused launch where `fused_ok(batch_size)`, else the general
        path."""
        if self.frames:
            return self.update_frames(ring, expert, idx_dev, n_new, n_steps, batch_size, gamma, max_grad_norm, lr, stats,
                                      grad_out)
        if getattr(ring, "frames", False):
            raise NotImplementedError("MlpPolicy on a uint8 frame ring is not implemented: use 'CnnPolicy'")
        fn = self.update_fused if self.fused_ok(batch_size) else self.update_general
        fn(ring, expert, idx_dev, n_new, n_steps, batch_size, gamma, max_grad_norm, lr, stats, grad_out)


MlpPolicy = DQNPolicy


class CnnPolicy(DQNPolicy):
    """[SB3 dqn.policies.CnnPolicy]: `DQNPolicy` with `NatureCNN` as the features extractor, on uint8 [C, H, W] frames."""

    def __init__(self, observation_space, action_space, lr_schedule, net_arch: Optional[List[int]] = None,
                 activation_fn=nn.ReLU, features_extractor_class=NatureCNN, features_extractor_kwargs=None,
                 normalize_images: bool = True, optimizer_class=th.optim.Adam, optimizer_kwargs=None):
        if features_extractor_class is FlattenExtractor:
            raise NotImplementedError("CnnPolicy runs NatureCNN; the flatten extractor is MlpPolicy's")
        super().__init__(observation_space, action_space, lr_schedule, net_arch, activation_fn, features_extractor_class,
                         features_extractor_kwargs, normalize_images, optimizer_class, optimizer_kwargs)


class OffPolicyAlgorithm:
    """What [SB3 common/off_policy_algorithm.py] gives DQN and TD3 alike: the `BaseAlgorithm` surface, `learn`,
    `collect_rollouts`, `_store_transition` and `_dump_logs`. A subclass supplies `_sample_action`, `_on_step`, `train`."""

    # ---- SB3 BaseAlgorithm surface ----------------------------------------------------------------------------------
    @property
    def logger(self):
        return self._logger

    def set_logger(self, logger) -> None:
        self._logger = logger
        self._custom_logger = True

    def get_env(self):
        return self.env

    def set_env(self, env, force_reset: bool = True) -> None:
        """[SB3 BaseAlgorithm.set_env]: the spaces and the number of environments must be the model's; with `force_reset`
        the next `_setup_learn` resets the environment."""
        if env.num_envs != self.n_envs:
            raise ValueError("The number of environments to be set is different from the number of environments in "
                             f"the model: ({env.num_envs} != {self.n_envs})")
        if env.observation_space != self.observation_space:
            raise ValueError(f"Observation spaces do not match: {self.observation_space} != {env.observation_space}")
        if env.action_space != self.action_space:
            raise ValueError(f"Action spaces do not match: {self.action_space} != {env.action_space}")
        if force_reset:
            self._last_obs = None
        self.n_envs = env.num_envs
        self.env = env

    def _init_callback(self, callback):
        if callback is None:
            callback = _NullCallback()
        elif isinstance(callback, (list, tuple)):
            callback = _CallbackList(callback)
        callback.init_callback(self)
        return callback

    def _setup_learn(self, total_timesteps: int, callback, reset_num_timesteps: bool):
        self.start_time = time.time_ns()
        if self.ep_info_buffer is None or reset_num_timesteps:
            self.ep_info_buffer = collections.deque(maxlen=self._stats_window_size)
        if reset_num_timesteps:
            self.num_timesteps = 0
            self._episode_num = 0
        else:
            total_timesteps += self.num_timesteps
        self._total_timesteps = total_timesteps
        self._num_timesteps_at_start = self.num_timesteps
        if reset_num_timesteps or self._last_obs is None:
            self._last_obs = self.env.reset()
            self._last_episode_starts = np.ones((self.env.num_envs,), dtype=bool)
        if not self._custom_logger and self._logger is None:
            self._logger = imit_logger.Logger(None, [])
        return total_timesteps, self._init_callback(callback)

    def _store_transition(self, buffer_action, new_obs, reward, dones, infos) -> None:
        next_obs = copy.deepcopy(new_obs)
        for i, done in enumerate(dones):
            if done and infos[i].get("terminal_observation") is not None:
                next_obs[i] = infos[i]["terminal_observation"]
        self.replay_buffer.add(self._last_obs, next_obs, buffer_action, reward, dones, infos)
        self._last_obs = new_obs

    def _on_step(self) -> None:
        pass

    def _run_updates(self, rows: np.ndarray, idx_dev: th.Tensor, run) -> None:
        """The gradient steps of one `train` call, `run(lo, hi)` being steps [lo, hi) of it, behind the sample-time reward
        relabelling of a `ReplayBufferRewardWrapper` (imitation_amd/replay_buffer_wrapper.py): every sampled row of the
        call relabelled on the device, then one `run` over all steps; or, for a `reward_fn` only the host can call, per
        step its rows relabelled and that one step run. Any other buffer: `run(0, G)` as it stands."""
        G = len(rows)
        relabel = getattr(self.replay_buffer, "relabel_for_train", None)
        if relabel is None or relabel(idx_dev):
            run(0, G)
            return
        for s in range(G):
            self.replay_buffer.relabel_step(rows[s], idx_dev[s])
            run(s, s + 1)

    def _on_episode_end(self, env_index: int, n_envs: int) -> None:
        """[SB3 collect_rollouts]: where an episode's end resets the action noise."""

    def _dump_logs(self) -> None:
        elapsed = max((time.time_ns() - self.start_time) / 1e9, sys.float_info.epsilon)
        fps = int((self.num_timesteps - self._num_timesteps_at_start) / elapsed)
        self.logger.record("time/episodes", self._episode_num, exclude="tensorboard")
        if len(self.ep_info_buffer) > 0 and len(self.ep_info_buffer[0]) > 0:
            self.logger.record("rollout/ep_rew_mean", float(np.mean([e["r"] for e in self.ep_info_buffer])))
            self.logger.record("rollout/ep_len_mean", float(np.mean([e["l"] for e in self.ep_info_buffer])))
        self.logger.record("time/fps", fps)
        self.logger.record("time/time_elapsed", int(elapsed), exclude="tensorboard")
        self.logger.record("time/total_timesteps", self.num_timesteps, exclude="tensorboard")
        self.logger.dump(step=self.num_timesteps)

    def collect_rollouts(self, env, callback, train_freq, learning_starts: int, log_interval) -> Tuple[int, bool]:
        """[SB3 OffPolicyAlgorithm.collect_rollouts] -> (timesteps collected, continue training). `train_freq`: a number of
        steps, or SB3's pair (n, "step" | "episode"); episodes need one environment, as there."""
        self.policy.set_training_mode(False)
        steps, episodes = 0, 0
        freq, unit = train_freq if isinstance(train_freq, tuple) else (train_freq, "step")
        assert freq > 0, "Should at least collect one step or episode."
        if env.num_envs > 1:
            assert unit == "step", "You must use only one env when doing episodic training."
        callback.on_rollout_start()
        # [SB3 utils.should_collect_more_steps]
        while (steps < freq) if unit == "step" else (episodes < freq):
            actions = self._sample_action(learning_starts, env.num_envs)
            # (a learner with continuous actions returns the pair (env action, buffer action))
            actions, buffer_actions = actions if isinstance(actions, tuple) else (actions, actions)
            new_obs, rewards, dones, infos = env.step(actions)
            self.num_timesteps += env.num_envs
            steps += 1
            callback.update_locals(locals())
            if not callback.on_step():
                return steps * env.num_envs, False
            for info in infos:
                if info.get("episode") is not None:
                    self.ep_info_buffer.extend([info["episode"]])
            self._store_transition(buffer_actions, new_obs, rewards, dones, infos)
            self._current_progress_remaining = 1.0 - float(self.num_timesteps) / float(self._total_timesteps)
            self._on_step()
            for i, done in enumerate(dones):
                if done:
                    episodes += 1
                    self._episode_num += 1
                    self._on_episode_end(i, env.num_envs)
                    if log_interval is not None and self._episode_num % log_interval == 0:
                        self._dump_logs()
        callback.on_rollout_end()
        return steps * env.num_envs, True

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "DQN",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        if progress_bar:
            raise NotImplementedError("the progress bar is not implemented")
        require_device(self.device)
        total_timesteps, callback = self._setup_learn(total_timesteps, callback, reset_num_timesteps)
        callback.on_training_start(locals(), globals())
        while self.num_timesteps < total_timesteps:
            collected, go_on = self.collect_rollouts(self.env, callback, self.train_freq, self.learning_starts, log_interval)
            if not go_on:
                break
            if self.num_timesteps > 0 and self.num_timesteps > self.learning_starts:
                gradient_steps = self.gradient_steps if self.gradient_steps >= 0 else collected
                if gradient_steps > 0:
                    self.train(batch_size=self.batch_size, gradient_steps=gradient_steps)
        callback.on_training_end()
        return self




class DQN(OffPolicyAlgorithm):
    """[SB3 dqn.DQN] with `train_freq` in steps."""

    policy_aliases = {"MlpPolicy": DQNPolicy, "CnnPolicy": CnnPolicy}

    def __init__(self, policy, env, learning_rate=1e-4, buffer_size: int = 1_000_000, learning_starts: int = 50_000,
                 batch_size: int = 32, tau: float = 1.0, gamma: float = 0.99, train_freq=4, gradient_steps: int = 1,
                 replay_buffer_class=None, replay_buffer_kwargs: Optional[Dict[str, Any]] = None,
                 optimize_memory_usage: bool = False, target_update_interval: int = 10_000,
                 exploration_fraction: float = 0.1, exploration_initial_eps: float = 1.0,
                 exploration_final_eps: float = 0.05, max_grad_norm: float = 10, stats_window_size: int = 100,
                 tensorboard_log=None, policy_kwargs: Optional[Dict[str, Any]] = None, verbose: int = 0,
                 seed: Optional[int] = None, device="auto", _init_setup_model: bool = True):
        if isinstance(policy, str):
            if policy not in self.policy_aliases:
                raise NotImplementedError(f"policy {policy!r}: only 'MlpPolicy' and 'CnnPolicy' are implemented for DQN")
            policy = self.policy_aliases[policy]
        if isinstance(train_freq, tuple):
            if len(train_freq) != 2 or train_freq[1] != "step":
                raise NotImplementedError("train_freq is counted in steps")
            train_freq = train_freq[0]
        if tensorboard_log is not None:
            raise NotImplementedError("tensorboard logging is not implemented")
        self.policy_class = policy
        self.policy_kwargs = dict(policy_kwargs or {})
        self.device = _device(device)
        self.learning_rate, self.buffer_size, self.learning_starts = learning_rate, buffer_size, learning_starts
        self.batch_size, self.tau, self.gamma = batch_size, tau, gamma
        self.train_freq, self.gradient_steps = int(train_freq), gradient_steps
        self.replay_buffer_class = replay_buffer_class
        self.replay_buffer_kwargs = dict(replay_buffer_kwargs or {})
        self.optimize_memory_usage = optimize_memory_usage
        self.target_update_interval = target_update_interval
        self.exploration_initial_eps, self.exploration_final_eps = exploration_initial_eps, exploration_final_eps
        self.exploration_fraction = exploration_fraction
        self.max_grad_norm, self.seed, self.verbose = max_grad_norm, seed, verbose
        self._n_calls = 0
        self.exploration_rate = 0.0   # [SB3 dqn.py]: zero until the first `_on_step`
        self.num_timesteps = 0
        self._total_timesteps = 0
        self._num_timesteps_at_start = 0
        self._n_updates = 0
        self._episode_num = 0
        self._current_progress_remaining = 1.0
        self._last_obs = None
        self._last_episode_starts = None
        self._stats_window_size = stats_window_size
        self.ep_info_buffer = None
        self._logger: Optional[imit_logger.Logger] = None
        self._custom_logger = False
        self.start_time = 0
        self.env = env
        self.policy: Optional[DQNPolicy] = None
        self.replay_buffer: Optional[ReplayBuffer] = None
        self.last_action_branch: Optional[str] = None   # "warmup" / "explore" / "greedy" of the latest `_sample_action`
        if env is not None:
            self.observation_space, self.action_space, self.n_envs = env.observation_space, env.action_space, env.num_envs
        if _init_setup_model:
            self._setup_model()

    def _setup_model(self) -> None:
        self.lr_schedule = _schedule(self.learning_rate)
        if self.seed is not None:
            set_random_seed(self.seed)
            self.action_space.seed(self.seed)
            if self.env is not None:
                self.env.seed(self.seed)
        if self.replay_buffer_class is None:
            self.replay_buffer_class = ReplayBuffer
        if self.replay_buffer is None:
            self.replay_buffer = self.replay_buffer_class(
                self.buffer_size, self.observation_space, self.action_space, device=self.device, n_envs=self.n_envs,
                optimize_memory_usage=self.optimize_memory_usage, **self.replay_buffer_kwargs)
        self.policy = self.policy_class(self.observation_space, self.action_space, self.lr_schedule,
                                        **self.policy_kwargs).to(self.device)
        self.q_net, self.q_net_target = self.policy.q_net, self.policy.q_net_target
        self.exploration_schedule = get_linear_fn(self.exploration_initial_eps, self.exploration_final_eps,
                                                  self.exploration_fraction)
        if self.n_envs > 1 and self.n_envs > self.target_update_interval:
            warnings.warn("The number of environments used is greater than the target network update interval "
                          f"({self.n_envs} > {self.target_update_interval}), therefore the target network will be updated "
                          "after each call to env.step() which corresponds to "
                          f"{self.n_envs} steps.")

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """[SB3 DQN.predict]: ONE `np.random.rand()` per call decides for the whole batch."""
        if not deterministic and np.random.rand() < self.exploration_rate:
            self.last_action_branch = "explore"
            observation = np.asarray(observation)
            if observation.shape != tuple(self.observation_space.shape):
                action = np.array([self.action_space.sample() for _ in range(observation.shape[0])])
            else:
                action = np.array(self.action_space.sample())
            return action, state
        self.last_action_branch = "greedy"
        return self.policy.predict(observation, state, episode_start, deterministic)

    def _sample_action(self, learning_starts: int, n_envs: int) -> np.ndarray:
        if self.num_timesteps < learning_starts:
            self.last_action_branch = "warmup"
            return np.array([self.action_space.sample() for _ in range(n_envs)])
        action, _ = self.predict(self._last_obs, deterministic=False)
        return action

    def _on_step(self) -> None:
        self._n_calls += 1
        if self._n_calls % max(self.target_update_interval // self.n_envs, 1) == 0:
            self.policy.polyak_update(self.tau)
        self.exploration_rate = self.exploration_schedule(self._current_progress_remaining)
        self.logger.record("rollout/exploration_rate", self.exploration_rate)

    def train(self, gradient_steps: int, batch_size: int = 100) -> None:
        """[SB3 DQN.train]: the index draws of all `gradient_steps` minibatches first (the same global-stream draws in
        the same order: nothing else draws in between), one upload, the update, one read-back."""
        self.policy.set_training_mode(True)
        lr = self.lr_schedule(self._current_progress_remaining)
        self.logger.record("train/learning_rate", lr)
        rows = np.empty((gradient_steps, batch_size), np.int64)
        n_new = batch_size
        for s in range(gradient_steps):
            rows[s], n_new = self.replay_buffer.sample_rows(batch_size)
        self.last_sample_rows, self.last_n_new = rows, n_new
        if self.policy.frames:   # (the assemble kernel moves whole frames by these indices: checked before any launch)
            self.policy.check_rows(rows, n_new, self.replay_buffer.table, self.replay_buffer.expert_table())
        idx_dev = th.from_numpy(rows).to(self.device)
        stats = th.empty(gradient_steps, 2, device=self.device)
        self._run_updates(rows, idx_dev, lambda lo, hi: self.policy.update(
            self.replay_buffer.table, self.replay_buffer.expert_table(), idx_dev[lo:hi], n_new, hi - lo, batch_size,
            self.gamma, self.max_grad_norm, lr, stats[lo:hi]))
        self.last_train_stats = stats.cpu().numpy()
        self._n_updates += gradient_steps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/loss", np.mean(self.last_train_stats[:, 0].astype(np.float64)))
