"""What SQIL needs of stable-baselines3's DQN (`algorithms/sqil.py:12-19,77-83`): `DQN`, `DQNPolicy` ("MlpPolicy",
"CnnPolicy") and `QNetwork` -- a restatement of stable-baselines3 2.2.x from its documented behaviour ([SB3 dqn/dqn.py,
dqn/policies.py]). SB3's `ReplayBuffer` and the off-policy loop are `imitation_amd/off_policy.py`, the per-step reward
sources of a learner ring under a learned reward `imitation_amd/step_source.py`; their names stay importable from here.

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

import ctypes as C
import os
import warnings
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch as th
from torch import nn

from imitation_amd import _lib as L
from imitation_amd import spaces
from imitation_amd.cnn_policy import NatureCNN, NatureCnnTrunk, _is_image_space
from imitation_amd.networks import require_device
from imitation_amd.off_policy import (OffPolicyAlgorithm, ReplayBuffer, ReplayBufferSamples, ReplayIndex,  # noqa: F401
                                      _device, _Table, adam_kwargs, table_pointers)
from imitation_amd.policies import FlattenExtractor
from imitation_amd.step_source import (FrameRewardStepSource, RewardStepSource, StepSource, _RoundTile,  # noqa: F401
                                       frame_reward_plan)


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
        self.optimizer_kwargs, self.betas, self.eps, self.weight_decay = adam_kwargs(optimizer_kwargs)
        if self.frames:
            features_dim = int((features_extractor_kwargs or {}).get("features_dim", 512))
            self.q_net = CnnQNetwork(observation_space, action_space, features_dim)
            self.q_net_target = CnnQNetwork(observation_space, action_space, features_dim)
        else:
            self.q_net = QNetwork(observation_space, action_space, self.net_arch, activation_fn)
            self.q_net_target = QNetwork(observation_space, action_space, self.net_arch, activation_fn)
        self.q_net_target._flat.copy_(self.q_net._flat)
        self.lr = float(lr_schedule(1))
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
        rc = L.load().ia_dqn_update(   # (the kernel takes no row counts: the five columns of each table)
            q.obs_dim, q.net_arch[0], q.n_actions, int(batch_size), int(n_new), int(n_steps), L.ptr(q._flat),
            L.ptr(self.q_net_target._flat), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), *ring.pointers()[:5],
            *table_pointers(expert)[:5], L.ptr(idx_dev), float(gamma), float(max_grad_norm), float(self.betas[0]),
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
        n, D = q._flat.numel(), q.obs_dim
        shape = (B,) + tuple(self.observation_space.shape)
        obs, nxt = w["obs"].view(shape), w["nxt"].view(shape)
        idx_ptr, stats_ptr = idx_dev.data_ptr(), stats.data_ptr()
        tables = ring.pointers() + table_pointers(expert)
        for s in range(n_steps):
            L.call("ia_dqn_assemble_u8", *tables, idx_ptr + 8 * s * B, B, int(n_new), D,
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
        if isinstance(policy, str) and policy not in self.policy_aliases:
            raise NotImplementedError(f"policy {policy!r}: only 'MlpPolicy' and 'CnnPolicy' are implemented for DQN")
        if isinstance(train_freq, tuple):
            if len(train_freq) != 2 or train_freq[1] != "step":
                raise NotImplementedError("train_freq is counted in steps")
            train_freq = train_freq[0]
        if tensorboard_log is not None:
            raise NotImplementedError("tensorboard logging is not implemented")
        super().__init__(policy=policy, env=env, learning_rate=learning_rate, buffer_size=buffer_size,
                         learning_starts=learning_starts, batch_size=batch_size, tau=tau, gamma=gamma,
                         train_freq=int(train_freq), gradient_steps=gradient_steps, replay_buffer_class=replay_buffer_class,
                         replay_buffer_kwargs=replay_buffer_kwargs, optimize_memory_usage=optimize_memory_usage,
                         stats_window_size=stats_window_size, policy_kwargs=policy_kwargs, verbose=verbose, seed=seed,
                         device=device)
        self.target_update_interval, self.max_grad_norm = target_update_interval, max_grad_norm
        self.exploration_initial_eps, self.exploration_final_eps = exploration_initial_eps, exploration_final_eps
        self.exploration_fraction = exploration_fraction
        self._n_calls = 0
        self.exploration_rate = 0.0   # [SB3 dqn.py]: zero until the first `_on_step`
        if _init_setup_model:
            self._setup_model()

    def _bind_policy(self) -> None:
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

    def _check_rows(self, rows: np.ndarray, n_new: int) -> None:
        if self.policy.frames:   # (the assemble kernel moves whole frames by these indices: checked before any launch)
            self.policy.check_rows(rows, n_new, self.replay_buffer.table, self.replay_buffer.expert_table())

    def train(self, gradient_steps: int, batch_size: int = 100) -> None:
        """[SB3 DQN.train]: the index draws of all `gradient_steps` minibatches first (the same global-stream draws in
        the same order: nothing else draws in between), one upload, the update, one read-back."""
        lr, rows, n_new, idx_dev = self._begin_train(gradient_steps, batch_size)
        stats = th.empty(gradient_steps, 2, device=self.device)
        self._run_updates(rows, idx_dev, lambda lo, hi: self.policy.update(
            self.replay_buffer.table, self.replay_buffer.expert_table(), idx_dev[lo:hi], n_new, hi - lo, batch_size,
            self.gamma, self.max_grad_norm, lr, stats[lo:hi]))
        self.last_train_stats = stats.cpu().numpy()
        self._n_updates += gradient_steps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        self.logger.record("train/loss", np.mean(self.last_train_stats[:, 0].astype(np.float64)))
