"""TD3 and DDPG, the continuous-action learners SQIL can run on (`algorithms/sqil.py:42,77-83` takes any off-policy learner
through `rl_algo_class`; the reference's tests run it on Pendulum with both): `TD3`, `DDPG`, `TD3Policy` ("MlpPolicy"),
`Actor`, `ContinuousCritic` and `NormalActionNoise` -- a restatement of stable-baselines3 2.2.x from its documented behaviour
([SB3 td3/td3.py, td3/policies.py, ddpg/ddpg.py, common/off_policy_algorithm.py, common/noise.py, common/policies.py]).
SAC (a stochastic actor and a learned entropy coefficient) builds on these classes in `imitation_amd/sac.py`.

Layout, as for `dqn.py`: the host makes every index decision with SB3's draw sequence from NumPy's GLOBAL
stream and draws the target-policy noise from torch's GLOBAL CPU generator with SB3's own call and shape per step; a `train`
call draws the rows of all its gradient steps, then the noise of all its steps, uploads both once, enqueues every step
(`TD3Policy.update`: no host synchronisation and no ATen operator inside the step loop) and reads back one block
{critic_loss, actor_loss or NaN} per step. The networks run on the fp32 MFMA stacks (`ia_mlp_forward` / `ia_mlp_backward`);
the step around them is csrc/td3.hip. The ring stores the SCALED action in [-1, 1]; the environment receives the unscaled
one. Demonstrations enter the expert table as given (the reference does not scale them, `sqil.py:196-204`).
"""
from __future__ import annotations

import copy
import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch as th
from torch import nn

from imitation_amd import _lib as L
from imitation_amd import spaces
from imitation_amd.networks import require_device
from imitation_amd.off_policy import OffPolicyAlgorithm, _Table, adam_kwargs, table_pointers
from imitation_amd.policies import FlattenExtractor


class ActionNoise:
    """[SB3 common/noise.py ActionNoise]: anything with `__call__` and `reset` serves."""

    def reset(self) -> None:
        pass

    def __call__(self) -> np.ndarray:
        raise NotImplementedError


class NormalActionNoise(ActionNoise):
    """[SB3 NormalActionNoise]: `np.random.normal(mean, sigma)` from NumPy's global stream, cast to `dtype`."""

    def __init__(self, mean: np.ndarray, sigma: np.ndarray, dtype=np.float32):
        self._mu, self._sigma, self._dtype = mean, sigma, dtype

    def __call__(self) -> np.ndarray:
        return np.random.normal(self._mu, self._sigma).astype(self._dtype)

    def __repr__(self) -> str:
        return f"NormalActionNoise(mu={self._mu}, sigma={self._sigma})"


class VectorizedActionNoise(ActionNoise):
    """[SB3 VectorizedActionNoise]: `n_envs` deep copies of a base noise, called in order and stacked."""

    def __init__(self, base_noise, n_envs: int):
        self.n_envs = int(n_envs)
        self.base_noise = base_noise
        self.noises = [copy.deepcopy(base_noise) for _ in range(self.n_envs)]

    def reset(self, indices=None) -> None:
        for i in (range(len(self.noises)) if indices is None else indices):
            self.noises[i].reset()

    def __call__(self) -> np.ndarray:
        return np.stack([noise() for noise in self.noises])


def create_mlp(input_dim: int, output_dim: int, net_arch: List[int], activation_fn=nn.ReLU,
               squash_output: bool = False) -> nn.Sequential:
    """[SB3 torch_layers.create_mlp] as CPU modules: torch's default initialisation AND its consumption of the generator."""
    mods: List[nn.Module] = []
    if len(net_arch) > 0:
        mods += [nn.Linear(input_dim, net_arch[0]), activation_fn()]
    for i in range(len(net_arch) - 1):
        mods += [nn.Linear(net_arch[i], net_arch[i + 1]), activation_fn()]
    if output_dim > 0:
        mods.append(nn.Linear(net_arch[-1] if len(net_arch) > 0 else input_dim, output_dim))
    if squash_output:
        mods.append(nn.Tanh())
    return nn.Sequential(*mods)


def get_actor_critic_arch(net_arch) -> Tuple[List[int], List[int]]:
    """[SB3 torch_layers.get_actor_critic_arch]: a list serves both; a dict names `pi` and `qf`."""
    if isinstance(net_arch, list):
        return list(net_arch), list(net_arch)
    assert isinstance(net_arch, dict), "Error: the net_arch can only contain be a list of ints or a dict"
    assert "pi" in net_arch, "Error: no key 'pi' was provided in net_arch for the actor network"
    assert "qf" in net_arch, "Error: no key 'qf' was provided in net_arch for the critic network"
    return list(net_arch["pi"]), list(net_arch["qf"])


def _check_spaces(observation_space, action_space, activation_fn) -> None:
    if not isinstance(action_space, spaces.Box) or len(action_space.shape) != 1:
        raise NotImplementedError("TD3 / DDPG need a flat Box action space")
    if not isinstance(observation_space, spaces.Box) or len(observation_space.shape) != 1:
        raise NotImplementedError("only flat Box observations are implemented")
    if activation_fn not in (nn.ReLU, nn.Tanh):
        raise NotImplementedError(f"activation {activation_fn} is not implemented on the HIP path")


class _Stack:
    """One MLP's names, sizes and descriptor; its parameters are a view `_flat` into the policy's flat buffers."""

    def __init__(self, seq: nn.Sequential, prefix: str, dims: List[int], act: int):
        if len(dims) - 1 > L.IA_MAX_LAYERS:
            raise NotImplementedError(f"at most {L.IA_MAX_LAYERS} layers")
        self.names = [(prefix + k, tuple(v.shape)) for k, v in seq.state_dict().items()]
        self.init = th.cat([p.detach().reshape(-1) for p in seq.parameters()]).contiguous()
        self.numel = self.init.numel()
        self.dims, self.desc = dims, L.mlp_desc(dims, act)
        self.hidden_per_row = sum(dims[1:-1])


class _Holder:
    """State holder over `stacks` whose parameters lie back to back in `_flat` (torch's `parameters()` order)."""

    stacks: List[_Stack]
    _flat: th.Tensor

    @property
    def device(self) -> th.device:
        return self._flat.device

    def numel(self) -> int:
        return sum(s.numel for s in self.stacks)

    def _init_flat(self) -> th.Tensor:
        return th.cat([s.init for s in self.stacks])

    def parameters(self):
        off = 0
        for s in self.stacks:
            for _, shape in s.names:
                n = int(np.prod(shape))
                yield self._flat[off:off + n].view(shape)
                off += n

    def state_dict(self) -> Dict[str, th.Tensor]:
        names = [k for s in self.stacks for k, _ in s.names]
        return dict(zip(names, self.parameters()))

    def load_state_dict(self, sd) -> None:
        for (k, p) in self.state_dict().items():
            p.copy_(th.as_tensor(sd[k]).reshape(p.shape))


class Actor(_Holder):
    """[SB3 td3.policies.Actor]: `mu = create_mlp(features_dim, action_dim, net_arch, activation_fn, squash_output=True)`."""

    def __init__(self, observation_space, action_space, net_arch: List[int], activation_fn=nn.ReLU):
        _check_spaces(observation_space, action_space, activation_fn)
        self.observation_space, self.action_space = observation_space, action_space
        self.obs_dim, self.act_dim = int(observation_space.shape[0]), int(action_space.shape[0])
        self.net_arch, self.activation_fn = [int(h) for h in net_arch], activation_fn
        act = L.ACT_RELU if activation_fn is nn.ReLU else L.ACT_TANH
        seq = create_mlp(self.obs_dim, self.act_dim, self.net_arch, activation_fn, squash_output=True)
        self.stacks = [_Stack(seq, "mu.", [self.obs_dim] + self.net_arch + [self.act_dim], act)]
        self._flat = self._init_flat()

    def forward(self, obs_dev: th.Tensor, hidden: Optional[th.Tensor] = None, out: Optional[th.Tensor] = None) -> th.Tensor:
        """mu [n, A] in [-1, 1] of device rows `obs_dev[n, D]`."""
        require_device(self.device)
        n, s = obs_dev.shape[0], self.stacks[0]
        out = th.empty(n, self.act_dim, device=self.device) if out is None else out
        hidden = th.empty(max(1, n * s.hidden_per_row), device=self.device) if hidden is None else hidden
        L.call("ia_mlp_forward", C.byref(s.desc), L.ptr(self._flat), L.ptr(obs_dev), self.obs_dim, n, L.ptr(hidden),
               L.ptr(out), L.ACT_TANH, L.stream())
        return out


class ContinuousCritic(_Holder):
    """[SB3 common/policies.ContinuousCritic]: `n_critics` stacks `qf{i} = create_mlp(features_dim + action_dim, 1, ...)`
    over the same input [obs | action]."""

    def __init__(self, observation_space, action_space, net_arch: List[int], activation_fn=nn.ReLU, n_critics: int = 2):
        _check_spaces(observation_space, action_space, activation_fn)
        if n_critics not in (1, 2):
            raise NotImplementedError("1 or 2 critics are implemented")
        self.observation_space, self.action_space = observation_space, action_space
        self.obs_dim, self.act_dim = int(observation_space.shape[0]), int(action_space.shape[0])
        self.net_arch, self.activation_fn, self.n_critics = [int(h) for h in net_arch], activation_fn, int(n_critics)
        act = L.ACT_RELU if activation_fn is nn.ReLU else L.ACT_TANH
        dims = [self.obs_dim + self.act_dim] + self.net_arch + [1]
        self.stacks = [_Stack(create_mlp(dims[0], 1, self.net_arch, activation_fn), f"qf{i}.", dims, act)
                       for i in range(self.n_critics)]
        self.q_networks = self.stacks
        self._flat = self._init_flat()


class ContinuousPolicy:
    """What `TD3Policy` and `sac.SACPolicy` share: an actor and critics (with the targets a subclass names) whose parameters
    lie in ONE flat online buffer [actor | critic] and one flat target buffer, one pair of Adam moment buffers over the
    online one, SB3's action scaling and `predict`, the workspace of a batch size and the launch sequences both `update`
    loops contain. A subclass supplies `holders`, `_build`, `actor_output`, `_extra_workspace` and `update`."""

    holders: Tuple[str, ...] = ()   # the networks in SB3's order; "<name>_target" starts as a copy of "<name>"

    def __init__(self, observation_space, action_space, lr_schedule, net_arch, activation_fn, features_extractor_class,
                 optimizer_class, optimizer_kwargs, n_critics, share_features_extractor):
        if features_extractor_class is not FlattenExtractor:
            raise NotImplementedError("only the flatten extractor (MlpPolicy) is implemented: no CNN extractor")
        if share_features_extractor:
            raise NotImplementedError("share_features_extractor=True is not implemented")
        if optimizer_class is not th.optim.Adam:
            raise NotImplementedError("only torch.optim.Adam is implemented")
        self.observation_space, self.action_space = observation_space, action_space
        self.net_arch = net_arch
        actor_arch, critic_arch = get_actor_critic_arch(self.net_arch)
        self.activation_fn, self.n_critics = activation_fn, n_critics
        self.optimizer_kwargs, self.betas, self.eps, self.weight_decay = adam_kwargs(optimizer_kwargs)
        self._build(actor_arch, critic_arch)   # (the draw order of torch's global generator)
        # online parameters as ONE flat buffer [actor | critic] (one pair of moment buffers), the targets as another in
        # the order of `holders`: one polyak launch covers all of them
        self._online = th.cat([self.actor._init_flat(), self.critic._init_flat()]).contiguous()
        self._target = th.cat([getattr(self, name[:-len("_target")])._init_flat() for name in self._targets()]).contiguous()
        self.exp_avg, self.exp_avg_sq = th.zeros_like(self._online), th.zeros_like(self._online)
        self.lr = float(lr_schedule(1))
        self.actor_adam_steps = self.critic_adam_steps = 0
        self.training = True
        self.squash_output = True
        self._ws: Dict[Any, Any] = {}
        self._bind()

    def _build(self, actor_arch: List[int], critic_arch: List[int]) -> None:
        """The networks named in `holders`, made in SB3's order."""
        raise NotImplementedError

    def _targets(self) -> List[str]:
        return [name for name in self.holders if name.endswith("_target")]

    def _bind(self) -> None:
        na = self.actor.numel()
        self.actor._flat, self.critic._flat = self._online[:na], self._online[na:]
        off = 0
        for name in self._targets():
            h = getattr(self, name)
            h._flat = self._target[off:off + h.numel()]
            off += h.numel()

    @property
    def device(self) -> th.device:
        return self._online.device

    def to(self, device):
        self._online, self._target = self._online.to(device).contiguous(), self._target.to(device).contiguous()
        self.exp_avg, self.exp_avg_sq = self.exp_avg.to(device), self.exp_avg_sq.to(device)
        self._ws = {}
        self._bind()
        return self

    def set_training_mode(self, mode: bool) -> None:
        self.training = mode

    def parameters(self):
        for name in self.holders:
            yield from getattr(self, name).parameters()

    def state_dict(self) -> Dict[str, th.Tensor]:
        out: Dict[str, th.Tensor] = {}
        for name in self.holders:
            out.update({f"{name}.{k}": v for k, v in getattr(self, name).state_dict().items()})
        return out

    def load_state_dict(self, sd) -> None:
        for name in self.holders:
            getattr(self, name).load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")})

    # ---- [SB3 BasePolicy] actions ------------------------------------------------------------------------------------
    def scale_action(self, action: np.ndarray) -> np.ndarray:
        """[SB3 BasePolicy.scale_action]: from [low, high] to [-1, 1]."""
        low, high = self.action_space.low, self.action_space.high
        return 2.0 * ((action - low) / (high - low)) - 1.0

    def unscale_action(self, scaled_action: np.ndarray) -> np.ndarray:
        """[SB3 BasePolicy.unscale_action]: from [-1, 1] to [low, high]."""
        low, high = self.action_space.low, self.action_space.high
        return low + (0.5 * (scaled_action + 1.0) * (high - low))

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """[SB3 BasePolicy.predict] of a squashing policy: the actor's action, unscaled to the action bounds."""
        self.set_training_mode(False)
        observation = np.asarray(observation)
        vectorized = observation.shape != tuple(self.observation_space.shape)
        actions = self.actor_output(observation, deterministic).reshape((-1, *self.action_space.shape))
        actions = self.unscale_action(actions)
        if not vectorized:
            actions = actions.squeeze(axis=0)
        return actions, state

    # ---- the update --------------------------------------------------------------------------------------------------
    def _adam_scalars(self, lr: float, t: int) -> Tuple[float, float]:
        b1, b2 = self.betas
        pair = np.array([lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5], np.float32)
        return float(pair[0]), float(pair[1])

    def _workspace(self, B: int):
        if B not in self._ws:
            a, c, dev = self.actor, self.critic, self.device
            D, A, nc = a.obs_dim, a.act_dim, c.n_critics
            ld = D + A
            sa, sc = a.stacks[0], c.stacks[0]
            splits = max(1, min(64, B // 256))
            e = lambda *shape: th.empty(*shape, device=dev)
            hid = lambda s: e(max(1, B * s.hidden_per_row))
            w = dict(ld=ld, splits=splits, X=e(B, ld), S=e(B, D), S2=e(B, D), rew=e(B), done=e(B), X2=e(B, ld), q=e(nc, B),
                     qt=e(nc, B), dq=e(nc, B), hid_a=hid(sa), hid_c=[hid(sc) for _ in range(nc)], dhid_a=hid(sa),
                     dhid_c=hid(sc), grads_a=e(sa.numel), grads_c=e(nc * sc.numel), scratch_c=e(splits, sc.numel))
            w.update(self._extra_workspace(B, e, hid))
            # one K split (batches below 512 rows): the backward's slab IS the gradient, no reduction launch
            w["part_a"] = w["grads_a"].view(1, -1) if splits == 1 else e(splits, sa.numel)
            w["part_c"] = [w["grads_c"][i * sc.numel:(i + 1) * sc.numel].view(1, -1) if splits == 1 else e(splits, sc.numel)
                           for i in range(nc)]
            self._ws[B] = w
        return self._ws[B]

    def _extra_workspace(self, B: int, e, hid) -> Dict[str, Any]:
        """The learner's own buffers of a batch of `B` rows (`e(*shape)`: an fp32 device buffer; `hid(stack)`: a stack's
        hidden activations)."""
        raise NotImplementedError

    def _begin_update(self, ring: Optional[_Table], expert: Optional[_Table], B: int, lr: float, st):
        """What both `update` loops start from -> (P, tables, critics_forward, critic_step, actor_step): the workspace of
        `B` rows as raw pointers (`hid_c` and `part_c` as lists of them), the pointers and row counts of the two tables
        (a table no row of the batch comes from may be absent) and the launch sequences the two steps share, bound to
        these buffers and to stream `st` so that a step pays one call for each:
          critics_forward(params, x, out)  the critics at `params` (n_critics blocks back to back) on input `x` -> `out`
          critic_step()                    critics' backward from `dq`, the K-split reduction if any, their Adam step
          actor_step(seed)                 the actor's backward from `seed`, the reduction if any, its Adam step"""
        require_device(self.device)
        w = self._workspace(B)
        sa, sc = self.actor.stacks[0], self.critic.stacks[0]
        D, nc, ld, splits, na, ncrit = self.actor.obs_dim, self.critic.n_critics, w["ld"], w["splits"], sa.numel, sc.numel
        call, ref = L.call, C.byref
        P = {k: (v.data_ptr() if isinstance(v, th.Tensor) else v) for k, v in w.items()}
        hid_c = P["hid_c"] = [t.data_ptr() for t in w["hid_c"]]
        part_c = P["part_c"] = [t.data_ptr() for t in w["part_c"]]
        on_a, on_c = self._online.data_ptr(), self._online.data_ptr() + 4 * na
        m, v = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        b1, b2 = float(self.betas[0]), float(self.betas[1])

        def critics_forward(params, x, out):   # the twin critics: two parameter blocks over ONE input tile
            for i in range(nc):
                call("ia_mlp_forward", ref(sc.desc), params + 4 * i * ncrit, x, ld, B, hid_c[i], out + 4 * i * B, L.ACT_NONE,
                     st)

        def critic_step():
            for i in range(nc):
                call("ia_mlp_backward", ref(sc.desc), on_c + 4 * i * ncrit, P["X"], ld, B, hid_c[i], P["dq"] + 4 * i * B,
                     P["dhid_c"], part_c[i], splits, None, st)
                if splits > 1:
                    call("ia_reduce_partials", part_c[i], splits, ncrit, 1.0, 0, P["grads_c"] + 4 * i * ncrit, st)
            self.critic_adam_steps += 1
            step_size, bc2 = self._adam_scalars(lr, self.critic_adam_steps)
            call("ia_dqn_adam_step", on_c, P["grads_c"], m + 4 * na, v + 4 * na, nc * ncrit, b1, b2, self.eps,
                 self.weight_decay, step_size, bc2, st)

        def actor_step(seed):
            call("ia_mlp_backward", ref(sa.desc), on_a, P["S"], D, B, P["hid_a"], seed, P["dhid_a"], P["part_a"], splits, None,
                 st)
            if splits > 1:
                call("ia_reduce_partials", P["part_a"], splits, na, 1.0, 0, P["grads_a"], st)
            self.actor_adam_steps += 1
            step_size, bc2 = self._adam_scalars(lr, self.actor_adam_steps)
            call("ia_dqn_adam_step", on_a, P["grads_a"], m, v, na, b1, b2, self.eps, self.weight_decay, step_size, bc2, st)

        return P, table_pointers(ring) + table_pointers(expert), critics_forward, critic_step, actor_step


class TD3Policy(ContinuousPolicy):
    """[SB3 td3.policies.TD3Policy]: `_build` makes the actor, the actor target (which loads the actor's state), the critic
    and the critic target (likewise), in that order; one Adam over the actor and one over the critic."""

    holders = ("actor", "actor_target", "critic", "critic_target")

    def __init__(self, observation_space, action_space, lr_schedule, net_arch=None, activation_fn=nn.ReLU,
                 features_extractor_class=FlattenExtractor, features_extractor_kwargs=None, normalize_images: bool = True,
                 optimizer_class=th.optim.Adam, optimizer_kwargs=None, n_critics: int = 2,
                 share_features_extractor: bool = False):
        super().__init__(observation_space, action_space, lr_schedule, [400, 300] if net_arch is None else net_arch,
                         activation_fn, features_extractor_class, optimizer_class, optimizer_kwargs, n_critics,
                         share_features_extractor)

    def _build(self, actor_arch: List[int], critic_arch: List[int]) -> None:
        # [SB3 TD3Policy._build]
        space, fn = (self.observation_space, self.action_space), self.activation_fn
        self.actor = Actor(*space, actor_arch, fn)
        self.actor_target = Actor(*space, actor_arch, fn)
        self.critic = ContinuousCritic(*space, critic_arch, fn, self.n_critics)
        self.critic_target = ContinuousCritic(*space, critic_arch, fn, self.n_critics)

    def optimizer_state(self) -> Dict[str, th.Tensor]:
        """Adam's moments per optimiser, in the layout of the parameters."""
        na = self.actor.numel()
        return {"actor.exp_avg": self.exp_avg[:na], "actor.exp_avg_sq": self.exp_avg_sq[:na],
                "critic.exp_avg": self.exp_avg[na:], "critic.exp_avg_sq": self.exp_avg_sq[na:]}

    def actor_output(self, observation: np.ndarray, deterministic: bool = False) -> np.ndarray:
        """mu of host observations (one upload, one read-back); the policy is deterministic either way."""
        obs = np.ascontiguousarray(observation, np.float32).reshape(-1, self.actor.obs_dim)
        return self.actor.forward(th.from_numpy(obs).to(self.device)).cpu().numpy()

    def _extra_workspace(self, B: int, e, hid) -> Dict[str, Any]:
        A, ld = self.actor.act_dim, self.actor.obs_dim + self.actor.act_dim
        return dict(mu_t=e(B, A), mu=e(B, A), dmu=e(B, A), q1=e(1, B), ones=th.ones(B, device=self.device), dX=e(B, ld))

    def update(self, ring: Optional[_Table], expert: Optional[_Table], idx_dev: th.Tensor, noise_dev: th.Tensor, n_new: int,
               n_steps: int, batch_size: int, gamma: float, tau: float, policy_delay: int, noise_clip: float,
               n_updates: int, lr: float, stats: th.Tensor) -> List[bool]:
        """`n_steps` gradient steps of [SB3 TD3.train]. `idx_dev` int64 [n_steps, B], `noise_dev` float32 [n_steps, B, A]
        (unclipped), `n_updates` the learner's count BEFORE this call, `stats` float32 [n_steps, 2] with NaN in column 1.
        Returns which steps updated the actor. Nothing in the loop synchronises with the device or calls ATen."""
        a, c, B, st = self.actor, self.critic, int(batch_size), L.stream()
        P, tables, critics_forward, critic_step, actor_step = self._begin_update(ring, expert, B, lr, st)
        D, A, nc, ld, splits = a.obs_dim, a.act_dim, c.n_critics, P["ld"], P["splits"]
        sa, sc = a.stacks[0], c.stacks[0]
        na, ncrit = sa.numel, sc.numel
        call, ref = L.call, C.byref
        on_a, on_c = self._online.data_ptr(), self._online.data_ptr() + 4 * na
        tg_a, tg_c = self._target.data_ptr(), self._target.data_ptr() + 4 * na
        idx_ptr, noise_ptr, stats_ptr = idx_dev.data_ptr(), noise_dev.data_ptr(), stats.data_ptr()
        actor_steps: List[bool] = []
        for s in range(n_steps):
            n_updates += 1
            call("ia_td3_assemble", *tables, idx_ptr + 8 * s * B, B, int(n_new), D, A, ld, P["X"], P["S"], P["S2"], P["rew"],
                 P["done"], st)
            # target: y = r + (1 - d) gamma min_i Qt_i(s', clamp(mu_t(s') + clamp(noise)))
            call("ia_mlp_forward", ref(sa.desc), tg_a, P["S2"], D, B, P["hid_a"], P["mu_t"], L.ACT_TANH, st)
            call("ia_td3_target_input", P["S2"], P["mu_t"], noise_ptr + 4 * s * B * A, B, D, A, ld, float(noise_clip), P["X2"],
                 st)
            critics_forward(tg_c, P["X2"], P["qt"])
            critics_forward(on_c, P["X"], P["q"])
            call("ia_td3_critic_loss", P["q"], P["qt"], P["rew"], P["done"], B, nc, float(gamma), P["dq"], None,
                 stats_ptr + 8 * s, st)
            critic_step()
            actor_steps.append(n_updates % policy_delay == 0)
            if not actor_steps[-1]:
                continue
            # actor: loss = -mean Q_1(s, mu(s)); its gradient enters the actor through the critic's dX
            call("ia_mlp_forward", ref(sa.desc), on_a, P["S"], D, B, P["hid_a"], P["mu"], L.ACT_TANH, st)
            call("ia_td3_actor_input", P["mu"], B, D, A, ld, P["X"], st)
            call("ia_mlp_forward", ref(sc.desc), on_c, P["X"], ld, B, P["hid_c"][0], P["q1"], L.ACT_NONE, st)
            call("ia_mlp_backward", ref(sc.desc), on_c, P["X"], ld, B, P["hid_c"][0], P["ones"], P["dhid_c"], P["scratch_c"],
                 splits, P["dX"], st)
            call("ia_td3_actor_seed", P["q1"], P["dX"], P["mu"], B, D, A, ld, P["dmu"], stats_ptr + 8 * s + 4, st)
            actor_step(P["dmu"])
            # [SB3 utils.polyak_update] of critic and actor: one launch over [actor | critic]
            call("ia_polyak_update", on_a, tg_a, na + nc * ncrit, float(tau), st)
        return actor_steps


MlpPolicy = TD3Policy


class ContinuousOffPolicyAlgorithm(OffPolicyAlgorithm):
    """What `TD3` and `sac.SAC` share of [SB3 OffPolicyAlgorithm] for Box actions: `train_freq` in steps or episodes, the
    action noise, action scaling around the ring (it stores the SCALED action) and the collection branches."""

    def __init__(self, *, policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq,
                 gradient_steps, action_noise, replay_buffer_class, replay_buffer_kwargs, optimize_memory_usage,
                 stats_window_size, tensorboard_log, policy_kwargs, verbose, seed, device):
        if tensorboard_log is not None:
            raise NotImplementedError("tensorboard logging is not implemented")
        # [SB3 OffPolicyAlgorithm._convert_train_freq]
        if not isinstance(train_freq, tuple):
            train_freq = (train_freq, "step")
        if len(train_freq) != 2 or train_freq[1] not in ("step", "episode"):
            raise ValueError(f"The unit of the `train_freq` must be either 'step' or 'episode' not {train_freq!r}!")
        if not isinstance(train_freq[0], int):
            raise ValueError(f"The frequency of `train_freq` must be an integer and not {train_freq[0]}")
        if action_noise is not None and not (callable(action_noise) and hasattr(action_noise, "reset")):
            raise TypeError("action_noise must be None or an object with __call__ and reset")
        if (policy_kwargs or {}).get("use_sde") or "sde_sample_freq" in (policy_kwargs or {}):
            raise NotImplementedError("gSDE is not implemented")
        super().__init__(policy=policy, env=env, learning_rate=learning_rate, buffer_size=buffer_size,
                         learning_starts=learning_starts, batch_size=batch_size, tau=tau, gamma=gamma,
                         train_freq=(int(train_freq[0]), train_freq[1]), gradient_steps=gradient_steps,
                         replay_buffer_class=replay_buffer_class, replay_buffer_kwargs=replay_buffer_kwargs,
                         optimize_memory_usage=optimize_memory_usage, stats_window_size=stats_window_size,
                         policy_kwargs=policy_kwargs, verbose=verbose, seed=seed, device=device)
        self.action_noise = action_noise
        if env is not None and isinstance(self.action_space, spaces.Box):
            assert np.all(np.isfinite(np.array([self.action_space.low, self.action_space.high]))), \
                "Continuous action space must have a finite lower and upper bound"

    def _setup_learn(self, total_timesteps: int, callback, reset_num_timesteps: bool):
        # [SB3 OffPolicyAlgorithm._setup_learn]: one noise object per environment
        if (self.action_noise is not None and self.env.num_envs > 1 and
                not isinstance(self.action_noise, VectorizedActionNoise)):
            self.action_noise = VectorizedActionNoise(self.action_noise, self.env.num_envs)
        return super()._setup_learn(total_timesteps, callback, reset_num_timesteps)

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        return self.policy.predict(observation, state, episode_start, deterministic)

    def _sample_action(self, learning_starts: int, n_envs: int) -> Tuple[np.ndarray, np.ndarray]:
        """[SB3 OffPolicyAlgorithm._sample_action] for Box actions -> (action for the environment, scaled action for the
        ring)."""
        if self.num_timesteps < learning_starts:
            self.last_action_branch = "warmup"
            unscaled_action = np.array([self.action_space.sample() for _ in range(n_envs)])
        else:
            self.last_action_branch = "policy"
            unscaled_action, _ = self.predict(self._last_obs, deterministic=False)
        scaled_action = self.policy.scale_action(unscaled_action)
        if self.action_noise is not None:
            scaled_action = np.clip(scaled_action + self.action_noise(), -1, 1)
        return self.policy.unscale_action(scaled_action), scaled_action

    def _on_episode_end(self, env_index: int, n_envs: int) -> None:
        if self.action_noise is not None:
            kwargs = dict(indices=[env_index]) if n_envs > 1 else {}
            self.action_noise.reset(**kwargs)


class TD3(ContinuousOffPolicyAlgorithm):
    """[SB3 td3.TD3]."""

    policy_aliases = {"MlpPolicy": TD3Policy}

    def __init__(self, policy, env, learning_rate=1e-3, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 100, tau: float = 0.005, gamma: float = 0.99, train_freq=(1, "episode"),
                 gradient_steps: int = -1, action_noise=None, replay_buffer_class=None,
                 replay_buffer_kwargs: Optional[Dict[str, Any]] = None, optimize_memory_usage: bool = False,
                 policy_delay: int = 2, target_policy_noise: float = 0.2, target_noise_clip: float = 0.5,
                 stats_window_size: int = 100, tensorboard_log=None, policy_kwargs: Optional[Dict[str, Any]] = None,
                 verbose: int = 0, seed: Optional[int] = None, device="auto", _init_setup_model: bool = True):
        if isinstance(policy, str) and policy not in self.policy_aliases:
            raise NotImplementedError(f"policy {policy!r}: only 'MlpPolicy' is implemented for TD3 / DDPG "
                                      "(no CNN or multi-input extractor)")
        super().__init__(policy=policy, env=env, learning_rate=learning_rate, buffer_size=buffer_size,
                         learning_starts=learning_starts, batch_size=batch_size, tau=tau, gamma=gamma, train_freq=train_freq,
                         gradient_steps=gradient_steps, action_noise=action_noise, replay_buffer_class=replay_buffer_class,
                         replay_buffer_kwargs=replay_buffer_kwargs, optimize_memory_usage=optimize_memory_usage,
                         stats_window_size=stats_window_size, tensorboard_log=tensorboard_log, policy_kwargs=policy_kwargs,
                         verbose=verbose, seed=seed, device=device)
        self.policy_delay, self.target_policy_noise = policy_delay, target_policy_noise
        self.target_noise_clip = target_noise_clip
        if _init_setup_model:
            self._setup_model()

    def _bind_policy(self) -> None:
        self.actor, self.actor_target = self.policy.actor, self.policy.actor_target
        self.critic, self.critic_target = self.policy.critic, self.policy.critic_target

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "TD3",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return super().learn(total_timesteps, callback, log_interval, tb_log_name, reset_num_timesteps, progress_bar)

    def draw_target_noise(self, gradient_steps: int, batch_size: int) -> th.Tensor:
        """The target-policy noise of `gradient_steps` steps, UNCLIPPED, float32 [steps, B, A], from torch's global CPU
        generator: per step SB3's own call on a [B, A] float32 tensor (`actions.clone().data.normal_(0, sigma)`), so the
        generator ends where SB3's does."""
        out = th.empty(gradient_steps, batch_size, self.policy.actor.act_dim)
        for s in range(gradient_steps):
            out[s] = th.zeros(batch_size, self.policy.actor.act_dim).clone().data.normal_(0, self.target_policy_noise)
        return out

    def train(self, gradient_steps: int, batch_size: int = 100) -> None:
        """[SB3 TD3.train]: the index draws of all `gradient_steps` minibatches (NumPy's global stream), then the noise of
        all of them (torch's global generator) -- the two streams are independent, so each ends where SB3's interleaved
        draws leave it -- one upload of each, the steps, one read-back."""
        lr, rows, n_new, idx_dev = self._begin_train(gradient_steps, batch_size)
        self.last_target_noise = noise = self.draw_target_noise(gradient_steps, batch_size)
        noise_dev = noise.to(self.device)
        stats = th.full((gradient_steps, 2), float("nan"), device=self.device)
        self.last_actor_steps = []
        self._run_updates(rows, idx_dev, lambda lo, hi: self.last_actor_steps.extend(self.policy.update(
            self.replay_buffer.table, self.replay_buffer.expert_table(), idx_dev[lo:hi], noise_dev[lo:hi], n_new, hi - lo,
            batch_size, self.gamma, self.tau, self.policy_delay, self.target_noise_clip, self._n_updates + lo, lr,
            stats[lo:hi])))
        self.last_train_stats = stats.cpu().numpy()
        self._n_updates += gradient_steps
        self.logger.record("train/n_updates", self._n_updates, exclude="tensorboard")
        if any(self.last_actor_steps):
            actor_losses = self.last_train_stats[np.array(self.last_actor_steps), 1]
            self.logger.record("train/actor_loss", np.mean(actor_losses.astype(np.float64)))
        self.logger.record("train/critic_loss", np.mean(self.last_train_stats[:, 0].astype(np.float64)))


class DDPG(TD3):
    """[SB3 ddpg.DDPG]: TD3 with one critic, `policy_delay=1` and no target-policy noise. SB3 passes
    `target_policy_noise=0.1` with `target_noise_clip=0.0` ("we still need to specify target_policy_noise > 0 to avoid
    errors"): the noise is drawn, so torch's generator advances, and clipped to zero."""

    def __init__(self, policy, env, learning_rate=1e-3, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 100, tau: float = 0.005, gamma: float = 0.99, train_freq=(1, "episode"),
                 gradient_steps: int = -1, action_noise=None, replay_buffer_class=None,
                 replay_buffer_kwargs: Optional[Dict[str, Any]] = None, optimize_memory_usage: bool = False,
                 tensorboard_log=None, policy_kwargs: Optional[Dict[str, Any]] = None, verbose: int = 0,
                 seed: Optional[int] = None, device="auto", _init_setup_model: bool = True):
        super().__init__(policy=policy, env=env, learning_rate=learning_rate, buffer_size=buffer_size,
                         learning_starts=learning_starts, batch_size=batch_size, tau=tau, gamma=gamma, train_freq=train_freq,
                         gradient_steps=gradient_steps, action_noise=action_noise, replay_buffer_class=replay_buffer_class,
                         replay_buffer_kwargs=replay_buffer_kwargs, optimize_memory_usage=optimize_memory_usage,
                         policy_delay=1, target_noise_clip=0.0, target_policy_noise=0.1, tensorboard_log=tensorboard_log,
                         policy_kwargs=policy_kwargs, verbose=verbose, seed=seed, device=device, _init_setup_model=False)
        if "n_critics" not in self.policy_kwargs:
            self.policy_kwargs["n_critics"] = 1
        if _init_setup_model:
            self._setup_model()

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str = "DDPG",
              reset_num_timesteps: bool = True, progress_bar: bool = False):
        return super().learn(total_timesteps, callback, log_interval, tb_log_name, reset_num_timesteps, progress_bar)
