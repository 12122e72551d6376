"""The per-step reward sources of a learner ring under a learned reward (DESIGN sections 4.11 and 4.18): `AdversarialTrainer`
installs one on `off_policy.ReplayBuffer.reward_source`, and every environment step is then relabelled and stored by the
source's own launches instead of a reward prediction with its read-back followed by five small copies.

`StepSource` is what the two sources share: the step's rows go in through a ring of `SLOTS` pinned host records; a record is
rewritten only after the launch that read it has completed (one event per record, waited on only when the ring of records
wraps). `RewardVecEnvWrapper` stages the action the environment saw and the raw dones (`stage`); `ReplayBuffer.add` passes
the learner's view of the step (`store_step`), which writes the rows to the ring, to a per-round device tile (what the
trainer's own replay ring is filled from) and the rewards to a pinned host tile (the wrapper's episode bookkeeping).
`RewardStepSource` does so for float32 rows (csrc/offpolicy.hip), `FrameRewardStepSource` for uint8 frames under a
`modules.CnnRewardNet` (csrc/offpolicy_frames.hip).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, List, NamedTuple, Optional

import numpy as np
import torch as th

from imitation_amd import _lib as L
from imitation_amd.networks import require_device


class _RoundTile(NamedTuple):
    obs: th.Tensor
    next_fixed: th.Tensor
    clipped: th.Tensor
    dones: th.Tensor
    buffer_size: int
    n_envs: int


def _pin(*shape, dtype=th.float32) -> th.Tensor:
    return th.zeros(*shape, dtype=dtype).pin_memory()


class StepSource:
    """The ring of pinned records, the round tile and the body of a stored step. A subclass supplies its record layout
    (`_record`), its tile tensors (`_tile`), its argument record (`_args_key`, `_fill_args`), the record fill of a step
    (`_fill`), its launches (`_launch`) and `rollout_view`."""

    SLOTS = 8

    def __init__(self, ring, reward_net, slots: Optional[int] = None, tile_steps: int = 64):
        self.ring, self.net = ring, reward_net
        self.device = ring.device
        self.n, self.od = ring.n_envs, ring.obs_dim
        self.slots = []
        for _ in range(int(slots or self.SLOTS)):
            rec = self._record()
            rec["np"] = {k: v.numpy() for k, v in rec.items() if v is not None}
            self.slots.append(rec)
        self.events: List[Optional[th.cuda.Event]] = [None] * len(self.slots)
        self.launches = 0          # step launches so far (tests count them)
        self._slot_checked = -1
        self._staged = -1          # the `launches` count at the latest `stage`
        self.event_waits = 0       # records found still in flight when the ring of records wrapped
        self.tile_step = 0         # steps in the round tile
        self.tile_obs = None
        self._alloc_tile(int(tile_steps))
        self._args: List[Any] = [None] * len(self.slots)   # per record: (key, argument record with its pointers filled in)

    def _alloc_tile(self, steps: int) -> None:
        olds = None if self.tile_obs is None else (self.tile_obs, self.tile_next, self.tile_act, self.tile_dones,
                                                   self.rewards_host)
        self.tile_cap = steps
        self.tile_obs, self.tile_next, self.tile_act, self.tile_dones = self._tile(steps)
        self.rewards_host = th.zeros(steps, self.n).pin_memory()
        self.rewards_np = self.rewards_host.numpy()
        if olds is not None:   # a longer round than any before: the written rows move over (rare; one synchronisation)
            th.cuda.current_stream().synchronize()
            for new, o in zip((self.tile_obs, self.tile_next, self.tile_act, self.tile_dones, self.rewards_host), olds):
                m = min(len(o), len(new))
                new[:m].copy_(o[:m])
            th.cuda.current_stream().synchronize()

    def reward_row(self) -> np.ndarray:
        """The row of the pinned reward tile the NEXT stored step fills (valid once that step's launches have completed)."""
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
        self._fill(rec, obs, next_obs, ring_action, ring_done)
        if self.tile_step == self.tile_cap:
            self._alloc_tile(2 * self.tile_cap)
        # the argument record of pinned record `k`; refilled when a buffer it points to has moved
        key, cached = self._args_key(), self._args[k]
        if cached is not None and cached[0] == key:
            a = cached[1]
        else:
            a = self._fill_args(self.slots[k], self.ring.table)
            self._args[k] = (key, a)
        a.ring_row, a.tile_row = int(ring_row), self.tile_step * self.n
        a.rewards_host = self.rewards_host.data_ptr() + 4 * self.tile_step * self.n
        self._launch(a, rec)
        if self.events[k] is None:
            self.events[k] = th.cuda.Event()
        self.events[k].record()
        self.last_event = self.events[k]
        self.launches += 1
        self.tile_step += 1

    def wait(self) -> None:
        """Until the latest step's launches have completed (its rewards are then in the pinned tile)."""
        if self.launches:
            self.last_event.synchronize()

    def reset_tile(self) -> None:
        self.tile_step = 0


class RewardStepSource(StepSource):
    """The source of a float32 ring: one `ia_offpolicy_step` launch per environment step (csrc/offpolicy.hip). With a net
    whose `forward_plan` the kernel covers the reward is computed in the launch; any other net's `predict_th` stays on the
    device and the launch reads it from there."""

    def __init__(self, ring, reward_net, slots: Optional[int] = None, tile_steps: int = 64):
        if ring.frames:
            raise NotImplementedError("a learned reward on a uint8 frame ring is not implemented (ia_offpolicy_step reads "
                                      "and writes float32 rows)")
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
        super().__init__(ring, reward_net, slots, tile_steps)

    def _record(self):
        n, od, A = self.n, self.od, self.A
        return dict(obs=_pin(n, od), next_obs=_pin(n, od), dones=_pin(n, dtype=th.uint8), ring_done=_pin(n),
                    act=_pin(n, dtype=th.int64) if self.discrete else _pin(n, A),
                    ring_act=None if self.discrete else _pin(n, A))

    def _tile(self, steps: int):
        n, od, dev = self.n, self.od, self.device
        return (th.zeros((steps + 1) * n, od, device=dev),   # (one spare row block: `store_from_rollout`'s view)
                th.zeros(steps * n, od, device=dev),
                th.zeros(steps * n, dtype=th.int64, device=dev) if self.discrete else th.zeros(steps * n, self.A, device=dev),
                th.zeros(steps * n, dtype=th.uint8, device=dev))

    def _fill(self, rec, obs, next_obs, ring_action, ring_done) -> None:
        n = self.n
        rec["obs"][...] = np.asarray(obs).reshape(n, -1)
        rec["next_obs"][...] = np.asarray(next_obs).reshape(n, -1)
        rec["ring_done"][...] = ring_done
        if not self.discrete:
            rec["ring_act"][...] = np.asarray(ring_action).reshape(n, -1)

    def _args_key(self):
        """(a longer round tile, a reward net moved to another device)"""
        b = self.base
        nrm = None if b is None else b.mlp.norm
        return (self.tile_obs.data_ptr(), None if b is None else b.mlp.flat.data_ptr(),
                None if nrm is None else nrm.running_mean.data_ptr())

    def _fill_args(self, slot, t):
        b, n, a = self.base, self.n, L.OffpolicyStepArgs()
        nrm = None if b is None else b.mlp.norm
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
        return a

    def _launch(self, a, rec) -> None:
        if self.base is None:   # any other net: its prediction stays on the device
            n = self.n
            so, sa = tuple(self.ring.observation_space.shape), tuple(self.ring.action_space.shape)
            rewards_in = self.net.predict_th(rec["obs"].reshape((n,) + so), rec["act"].reshape((n,) + sa),
                                             rec["next_obs"].reshape((n,) + so), rec["dones"].astype(bool)).contiguous()
            a.rewards_in = rewards_in.data_ptr()
        L.check(L.load().ia_offpolicy_step(C.byref(a), L.stream()), "ia_offpolicy_step")

    def rollout_view(self):
        """The round tile with the fields `buffer.ReplayBuffer.store_from_rollout` reads."""
        T, n = self.tile_step, self.n
        return _RoundTile(self.tile_obs[:(T + 1) * n], self.tile_next[:T * n], self.tile_act[:T * n].reshape(T * n, -1),
                          self.tile_dones[:T * n], T, n)


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


class FrameRewardStepSource(StepSource):
    """The source of a uint8 frame ring under a `modules.CnnRewardNet` (csrc/offpolicy_frames.hip): per environment step ONE
    `ia_offpolicy_frames_step` launch reads the step's frames once from a pinned host record and writes them to the
    learner's ring, to the uint8 round tile and, as channel-last fp32 through the byte table, to the reward CNN's input;
    the CNN runs under `no_grad` (`forward_nhwc`, the convolution ops); ONE `ia_offpolicy_frames_reward` launch selects
    the action's (and done's) output, applies GAIL's softplus and writes the rewards to the ring and to the pinned host
    reward tile."""

    def __init__(self, ring, reward_net, slots: Optional[int] = None, tile_steps: int = 64):
        from imitation_amd import ops
        if not ring.frames or ring.act_dim is not None:
            raise TypeError("FrameRewardStepSource stores uint8 frames with Discrete actions (RewardStepSource stores "
                            "float32 rows)")
        require_device(ring.device)
        plan = frame_reward_plan(reward_net)
        if plan is None:
            raise NotImplementedError("the frame path's reward launch covers modules.CnnRewardNet(hwc_format=False) with "
                                      "normalize_images, plain or under GAIL's softplus; any other net takes the host path")
        self.cnn_net, self.softplus = plan
        self.shape = tuple(ring.observation_space.shape)          # (C, H, W)
        self.n_actions = int(ring.action_space.n)
        c = self.cnn_net
        self.S = int(c.use_state) + int(c.use_next_state)
        self.n_out = (self.n_actions if c.use_action else 1) * (2 if c.use_done else 1)
        self.lut = ops._byte_lut(ring.device)
        C_, H, W = self.shape
        self.X = th.empty(ring.n_envs, H, W, C_ * self.S, device=ring.device)
        self.reward_launches = 0   # `ia_offpolicy_frames_reward` calls so far
        super().__init__(ring, reward_net, slots, tile_steps)

    def _record(self):
        n, od = self.n, self.od
        return dict(obs=_pin(n, od, dtype=th.uint8), next_obs=_pin(n, od, dtype=th.uint8), dones=_pin(n, dtype=th.uint8),
                    ring_done=_pin(n), act=_pin(n, dtype=th.int64))

    def _tile(self, steps: int):
        n, od, dev = self.n, self.od, self.device
        return (th.zeros(steps * n, od, dtype=th.uint8, device=dev), th.zeros(steps * n, od, dtype=th.uint8, device=dev),
                th.zeros(steps * n, dtype=th.int64, device=dev), th.zeros(steps * n, dtype=th.uint8, device=dev))

    def _fill(self, rec, obs, next_obs, ring_action, ring_done) -> None:
        n = self.n
        obs, next_obs = np.asarray(obs), np.asarray(next_obs)
        if obs.dtype != np.uint8 or next_obs.dtype != np.uint8:
            raise ValueError("a frame table stores uint8 frames as they come: the observations must be uint8 arrays")
        rec["obs"][...] = obs.reshape(n, -1)
        rec["next_obs"][...] = next_obs.reshape(n, -1)
        rec["ring_done"][...] = ring_done

    def _args_key(self):
        """(a longer round tile)"""
        return self.tile_obs.data_ptr()

    def _fill_args(self, slot, t):
        a = L.OffpolicyFramesArgs()
        a.obs, a.next_obs, a.act = slot["obs"].data_ptr(), slot["next_obs"].data_ptr(), slot["act"].data_ptr()
        a.dones, a.ring_done = slot["dones"].data_ptr(), slot["ring_done"].data_ptr()
        a.n, (a.C, a.H, a.W) = self.n, self.shape
        a.use_state, a.use_next_state = int(self.cnn_net.use_state), int(self.cnn_net.use_next_state)
        a.lut, a.X = self.lut.data_ptr(), self.X.data_ptr()
        a.ring_obs, a.ring_next_obs, a.ring_action = t.obs.data_ptr(), t.next_obs.data_ptr(), t.action.data_ptr()
        a.ring_reward, a.ring_done_out, a.ring_rows = t.reward.data_ptr(), t.done.data_ptr(), t.rows
        a.tile_obs, a.tile_next_obs = self.tile_obs.data_ptr(), self.tile_next.data_ptr()
        a.tile_act, a.tile_dones, a.tile_rows = self.tile_act.data_ptr(), self.tile_dones.data_ptr(), self.tile_cap * self.n
        return a

    def _launch(self, a, rec) -> None:
        lib, st, c = L.load(), L.stream(), self.cnn_net
        L.check(lib.ia_offpolicy_frames_step(C.byref(a), st), "ia_offpolicy_frames_step")
        with th.no_grad():
            out = c.cnn.forward_nhwc(self.X).contiguous()
        L.check(lib.ia_offpolicy_frames_reward(C.byref(a), out.data_ptr(), self.n_out, None, self.n_actions,
                                               int(c.use_action), int(c.use_done), int(self.softplus), st),
                "ia_offpolicy_frames_reward")
        self.reward_launches += 1

    def rollout_view(self):
        """The round tile with the fields `buffer.FrameReplayBuffer.store_from_rollout` reads."""
        T, n = self.tile_step, self.n
        return _RoundTile(self.tile_obs[:T * n], self.tile_next[:T * n], self.tile_act[:T * n], self.tile_dones[:T * n], T, n)
