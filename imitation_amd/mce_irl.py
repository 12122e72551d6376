"""Finite-horizon tabular Maximum Causal Entropy IRL (`algorithms/mce_irl.py`), planned on the device.

Same surface as the reference module: `mce_partition_fh`, `mce_occupancy_measures`, `squeeze_r`, `TabularPolicy` and
`MCEIRL` with its constructor, `set_demonstrations`, `train` and `policy`. The environment is any object with the
arrays of a tabular model (`TabularEnv` is a plain container of them; `seals` is not a dependency here).

The soft Bellman backup and the occupancy pass run in float64 on `ia_mce_backup` / `ia_mce_forward` (`csrc/mce.hip`);
`MCEIRL.train` keeps the transition tensor, the tables and the reward net on the device and reads back one row of three
statistics per iteration. There is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import itertools
import warnings
from typing import Any, Dict, Iterable, List, Mapping, Optional, Tuple, Type, Union

import numpy as np
import torch as th

from imitation_amd import _lib as L
from imitation_amd import data_types as dt
from imitation_amd import logger as imit_logger
from imitation_amd import networks, reward_nets, spaces
from imitation_amd.networks import HipAdam, require_device


@dataclasses.dataclass
class TabularEnv:
    """The arrays of a tabular, known-dynamics POMDP (what `seals.base_envs.TabularModelPOMDP` exposes to MCE IRL)."""

    transition_matrix: np.ndarray     # [S, A, S], transition_matrix[s, a, s'] = P(s' | s, a)
    observation_matrix: np.ndarray    # [S, obs_dim]
    reward_matrix: np.ndarray         # [S]
    horizon: Optional[int]
    initial_state_dist: np.ndarray    # [S]

    @property
    def state_dim(self) -> int:
        return int(self.transition_matrix.shape[0])

    @property
    def action_dim(self) -> int:
        return int(self.transition_matrix.shape[1])

    @property
    def obs_dim(self) -> int:
        return int(self.observation_matrix.shape[1])

    @property
    def state_space(self) -> spaces.Discrete:
        return spaces.Discrete(self.state_dim)

    @property
    def action_space(self) -> spaces.Discrete:
        return spaces.Discrete(self.action_dim)

    @property
    def observation_space(self) -> spaces.Box:
        return spaces.Box(-np.inf, np.inf, (self.obs_dim,), np.float32)


def _device() -> th.device:
    dev = th.device("cuda" if th.cuda.is_available() else "cpu")
    require_device(dev)
    return dev


def _reward_f32(reward: np.ndarray, n_states: int) -> np.ndarray:
    reward = np.asarray(reward)
    assert reward.shape == (n_states,), f"expected a reward of shape ({n_states},), got {reward.shape}"
    r32 = np.ascontiguousarray(reward, dtype=np.float32)
    if not np.array_equal(r32.astype(np.float64), reward.astype(np.float64), equal_nan=True):
        warnings.warn("the reward is rounded to float32, the planning kernels' input dtype (a reward net's output dtype)")
    return r32


class _Planner:
    """Device tables of one environment and the kernel calls over them."""

    def __init__(self, env, device: th.device):
        horizon = env.horizon
        if horizon is None:
            raise ValueError("Only finite-horizon environments are supported.")
        self.S, self.A, self.H = int(env.state_dim), int(env.action_dim), int(horizon)
        S, A, H = self.S, self.A, self.H
        T = np.ascontiguousarray(env.transition_matrix, dtype=np.float64)
        assert T.shape == (S, A, S), f"expected a transition matrix of shape {(S, A, S)}, got {T.shape}"
        f64 = dict(dtype=th.float64, device=device)
        self.T = th.as_tensor(T).to(device)
        self.init = th.as_tensor(np.ascontiguousarray(env.initial_state_dist, dtype=np.float64).reshape(S)).to(device)
        self.V = th.empty(H, S, **f64)
        self.Q = th.empty(H, S, A, **f64)
        self.pi = th.empty(H, S, A, **f64)
        self.D = th.empty(H + 1, S, **f64)
        self.Dcum = th.empty(S, **f64)
        self.ws = th.empty(max(1, int(L.load().ia_mce_forward_ws_doubles(S, A))), **f64)

    def backup(self, reward: th.Tensor, discount: float) -> None:
        assert reward.dtype == th.float32 and reward.numel() == self.S
        L.call("ia_mce_backup", L.ptr(self.T), L.ptr(reward), self.S, self.A, self.H, float(discount), L.ptr(self.V),
               L.ptr(self.Q), L.ptr(self.pi), L.stream())

    def forward(self, pi: th.Tensor, discount: float) -> None:
        L.call("ia_mce_forward", L.ptr(self.T), L.ptr(pi), L.ptr(self.init), self.S, self.A, self.H, float(discount),
               L.ptr(self.D), L.ptr(self.Dcum), L.ptr(self.ws), L.stream())


def mce_partition_fh(env, *, reward: Optional[np.ndarray] = None,
                     discount: float = 1.0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    r"""Performs the soft Bellman backup for a finite-horizon MDP (`mce_irl.py:38-93`).

    Returns `(V, Q, \pi)`, float64: `V[t, s]`, `Q[t, s, a]` and `\pi[t, s, a]`.

    Raises:
        ValueError: if ``env.horizon`` is None (infinite horizon).
    """
    if env.horizon is None:
        raise ValueError("Only finite-horizon environments are supported.")
    if reward is None:
        reward = env.reward_matrix
    dev = _device()
    p = _Planner(env, dev)
    p.backup(th.as_tensor(_reward_f32(reward, p.S)).to(dev), discount)
    return p.V.cpu().numpy(), p.Q.cpu().numpy(), p.pi.cpu().numpy()


def mce_occupancy_measures(env, *, reward: Optional[np.ndarray] = None, pi: Optional[np.ndarray] = None,
                           discount: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """State visitation frequencies under a policy (`mce_irl.py:96-144`): `D[t, s]` of shape `(horizon + 1, n_states)` and
    the discounted sum `Dcum[s]`.

    `pi` defaults to the soft-optimal policy of `reward`; like the reference, that default policy is planned WITHOUT the
    discount (`:133` calls `mce_partition_fh(env, reward=reward)`), `discount` weighs the sum over time only.

    Raises:
        ValueError: if ``env.horizon`` is None (infinite horizon).
    """
    if env.horizon is None:
        raise ValueError("Only finite-horizon environments are supported.")
    if reward is None:
        reward = env.reward_matrix
    dev = _device()
    p = _Planner(env, dev)
    if pi is None:
        p.backup(th.as_tensor(_reward_f32(reward, p.S)).to(dev), 1.0)
        pi_d = p.pi
    else:
        pi = np.ascontiguousarray(pi, dtype=np.float64)
        assert pi.shape == (p.H, p.S, p.A), f"expected a policy of shape {(p.H, p.S, p.A)}, got {pi.shape}"
        pi_d = th.as_tensor(pi).to(dev)
    p.forward(pi_d, discount)
    return p.D.cpu().numpy(), p.Dcum.cpu().numpy()


def squeeze_r(r_output: th.Tensor) -> th.Tensor:
    """Squeeze a reward output tensor down to one dimension, if necessary (`[n_states]` or `[n_states, 1]`)."""
    if r_output.ndim == 2:
        return th.squeeze(r_output, 1)
    assert r_output.ndim == 1
    return r_output


class TabularPolicy:
    """A tabular policy. Cannot be trained -- prediction only. Host only: `predict` walks the rows in order."""

    pi: np.ndarray
    rng: np.random.Generator

    def __init__(self, state_space, action_space, pi: np.ndarray, rng: np.random.Generator) -> None:
        assert isinstance(state_space, spaces.Discrete), "state not tabular"
        assert isinstance(action_space, spaces.Discrete), "action not tabular"
        # What we call state space here is observation space in SB3 nomenclature.
        self.observation_space, self.action_space = state_space, action_space
        self.rng = rng
        self.set_pi(pi)

    def set_pi(self, pi: np.ndarray) -> None:
        """Sets tabular policy to `pi`."""
        assert pi.ndim == 3, "expected three-dimensional policy"
        assert np.allclose(pi.sum(axis=2), 1), "policy not normalized"
        assert np.all(pi >= 0), "policy has negative probabilities"
        self.pi = pi

    def _predict(self, observation, deterministic: bool = False):
        raise NotImplementedError("Should never be called as predict overridden.")

    def forward(self, observation, deterministic: bool = False):
        raise NotImplementedError("Should never be called.")

    def predict(self, observation, state: Optional[Tuple[np.ndarray, ...]] = None,
                episode_start: Optional[np.ndarray] = None,
                deterministic: bool = False) -> Tuple[np.ndarray, Optional[Tuple[np.ndarray, ...]]]:
        """Actions for the states `observation` of the underlying MDP; `state` carries the timesteps (`:210-258`)."""
        if state is None:
            timesteps = np.zeros(len(observation), dtype=int)
        else:
            assert len(state) == 1
            timesteps = state[0]
        assert len(timesteps) == len(observation), "timestep and obs batch size differ"

        if episode_start is not None:
            timesteps[episode_start] = 0

        actions: List[int] = []
        for obs, t in zip(observation, timesteps):
            assert self.observation_space.contains(obs), "illegal state"
            dist = self.pi[t, obs, :]
            if deterministic:
                actions.append(int(dist.argmax()))
            else:
                actions.append(self.rng.choice(len(dist), p=dist))

        timesteps += 1  # increment timestep
        state = (timesteps,)
        return np.array(actions), state


def _is_trajectory(x) -> bool:
    return isinstance(x, dt.TrajectoryWithRew) or all(hasattr(x, k) for k in ("obs", "acts", "terminal"))


def _is_transitions(x) -> bool:
    return isinstance(x, dt.Transitions) or (hasattr(x, "obs") and hasattr(x, "acts") and not hasattr(x, "terminal"))


_ADAM_OPTIONS = {"lr", "betas", "eps", "weight_decay", "amsgrad"}


def _supported_stack(reward_net) -> reward_nets.BasicRewardNet:
    """The product `BasicRewardNet` on the state alone whose `DenseStack` the loop drives, or `NotImplementedError`."""
    if type(reward_net) is not reward_nets.BasicRewardNet:
        raise NotImplementedError(
            f"reward net {type(reward_net).__name__} is not implemented for MCE IRL on the HIP path "
            "(imitation_amd.reward_nets.BasicRewardNet with use_action=False)")
    used = [n for n, f in (("actions", reward_net.use_action), ("next states", reward_net.use_next_state),
                           ("dones", reward_net.use_done)) if f]
    if used or not reward_net.use_state:
        raise NotImplementedError(
            f"MCE IRL learns a reward of the state alone: a reward net that uses {', '.join(used) or 'no state'} "
            "is not implemented (BasicRewardNet(..., use_action=False))")
    if reward_net.mlp.norm is not None:
        raise NotImplementedError("a reward net with an input normalisation layer is not implemented for MCE IRL")
    return reward_net


class MCEIRL:
    """Tabular MCE IRL (`mce_irl.py:264-560`).

    Reward is a function of observations, but policy is a function of states: planning gives the policy, the reward net
    is trained on `E_pi[r(S)] - E_D[r(S)]`."""

    demo_state_om: Optional[np.ndarray]

    def __init__(self, demonstrations, env, reward_net, rng: np.random.Generator,
                 optimizer_cls: Type[th.optim.Optimizer] = th.optim.Adam,
                 optimizer_kwargs: Optional[Mapping[str, Any]] = None, discount: float = 1.0, linf_eps: float = 1e-3,
                 grad_l2_eps: float = 1e-4, log_interval: Optional[int] = 100, *,
                 custom_logger: Optional[imit_logger.HierarchicalLogger] = None) -> None:
        self.discount = discount
        self.env = env
        self.demo_state_om = None
        self._logger = custom_logger or imit_logger.configure()
        if demonstrations is not None:
            self.set_demonstrations(demonstrations)

        self._basic = _supported_stack(reward_net)
        self.reward_net = reward_net
        if optimizer_cls is not th.optim.Adam:
            raise NotImplementedError("the fused reward-net step implements Adam (the reference's default)")
        self._optimizer_kwargs = dict(optimizer_kwargs or {"lr": 1e-2})
        unknown = set(self._optimizer_kwargs) - _ADAM_OPTIONS
        if unknown:
            raise NotImplementedError(f"Adam options {sorted(unknown)} are not implemented on the HIP path")
        self._optimizer: Optional[HipAdam] = None
        self._ensure_optimizer()

        self.linf_eps = linf_eps
        self.grad_l2_eps = grad_l2_eps
        self.log_interval = log_interval
        self.rng = rng

        # Uniform random until trained: something to return at all times from `policy`.
        if self.env.horizon is None:
            raise ValueError("Only finite-horizon environments are supported.")
        ones = np.ones((self.env.horizon, self.env.state_dim, self.env.action_dim))
        uniform_pi = ones / self.env.action_dim
        self._policy = TabularPolicy(state_space=self.env.state_space, action_space=self.env.action_space,
                                     pi=uniform_pi, rng=self.rng)
        self._dev: Dict[str, Any] = {}
        self._predicted_r_np: Optional[np.ndarray] = None

    @property
    def logger(self) -> imit_logger.HierarchicalLogger:
        return self._logger

    @logger.setter
    def logger(self, value: imit_logger.HierarchicalLogger) -> None:
        self._logger = value

    def _ensure_optimizer(self) -> HipAdam:
        """`HipAdam` over the net's flat buffer; rebuilt when the net has moved (`to(device)` re-materialises the buffer)
        before any step was taken."""
        store = self._basic._store
        opt = self._optimizer
        if opt is None or opt.flat is not store.flat:
            if opt is not None and opt.step_count > 0:
                raise RuntimeError("the reward net was moved after optimiser steps were taken")
            self._optimizer = HipAdam(store.flat, store.grad, **self._optimizer_kwargs)
        return self._optimizer

    @property
    def optimizer(self) -> HipAdam:
        return self._ensure_optimizer()

    # ---- demonstrations -> state occupancy measure (host, `:357-465`)
    def _set_demo_from_trajectories(self, trajs: Iterable) -> None:
        self.demo_state_om = np.zeros((self.env.state_dim,))
        num_demos = 0
        for traj in trajs:
            cum_discount = 1.0
            for obs in traj.obs:
                self.demo_state_om[obs] += cum_discount
                cum_discount *= self.discount
            num_demos += 1
        self.demo_state_om /= num_demos

    def _set_demo_from_obs(self, obses, dones, next_obses) -> None:
        self.demo_state_om = np.zeros((self.env.state_dim,))

        for obs in obses:
            if isinstance(obs, th.Tensor):
                obs = obs.item()  # must be scalar
            self.demo_state_om[obs] += 1.0

        # Transitions flattened from trajectories, possibly shuffled: terminal next observations appear nowhere else.
        if dones is not None and next_obses is not None:
            for done, obs in zip(dones, next_obses):
                if isinstance(done, th.Tensor):
                    done = done.item()  # must be scalar
                    obs = obs.item()  # must be scalar
                if done:
                    self.demo_state_om[obs] += 1.0
        else:
            warnings.warn(
                "Training MCEIRL with transitions that lack next observation."
                "This will result in systematically wrong occupancy measure estimates.",
            )

        # Normalize occupancy measure estimates
        assert self.env.horizon is not None
        self.demo_state_om *= (self.env.horizon + 1) / self.demo_state_om.sum()

    def set_demonstrations(self, demonstrations) -> None:
        self._dev_demo = None
        if isinstance(demonstrations, np.ndarray):
            # Demonstrations are an occupancy measure
            assert demonstrations.ndim == 1
            self.demo_state_om = demonstrations
            return

        # Trajectories or transitions: compute the occupancy measure from them.
        if isinstance(demonstrations, Iterable) and not _is_transitions(demonstrations):
            it = iter(demonstrations)
            try:
                first_item = next(it)
            except StopIteration:
                raise ValueError(f"iterable {demonstrations} had no elements")
            demonstrations = itertools.chain([first_item], it)
            if _is_trajectory(first_item):
                self._set_demo_from_trajectories(demonstrations)
                return

        # Transitions carry no timesteps, so the occupancy measure can only be computed undiscounted.
        if self.discount != 1.0:
            raise ValueError(
                "Cannot compute discounted OM from timeless Transitions.",
            )

        if _is_transitions(demonstrations):
            self._set_demo_from_obs(demonstrations.obs, getattr(demonstrations, "dones", None),
                                    getattr(demonstrations, "next_obs", None))
        elif isinstance(demonstrations, Iterable):
            # An iterable of batch mappings (a data loader): collect them into one array.
            collated_list: Dict[str, List[Any]] = collections.defaultdict(list)
            for batch in demonstrations:
                assert isinstance(batch, Mapping)
                for k in ("obs", "dones", "next_obs"):
                    x = batch.get(k)
                    if x is not None:
                        assert isinstance(x, (np.ndarray, th.Tensor))
                        collated_list[k].append(x)
            collated = {k: np.concatenate(v) for k, v in collated_list.items()}

            assert "obs" in collated
            for k, v in collated.items():
                assert len(v) == len(collated["obs"]), k
            self._set_demo_from_obs(collated["obs"], collated.get("dones"), collated.get("next_obs"))
        else:
            raise TypeError(
                f"Unsupported demonstration type {type(demonstrations)}",
            )

    # ---- training
    def _device_state(self) -> Dict[str, Any]:
        """Uploads made once per (algorithm, device): the planner's tables and the float32 observation matrix."""
        dev = self.reward_net.device
        require_device(dev)
        d = self._dev
        if d.get("device") != dev:
            obs = np.ascontiguousarray(self.env.observation_matrix, dtype=np.float32)
            assert obs.ndim == 2 and obs.shape[1] == self._basic.mlp.dims[0], \
                f"observation matrix {obs.shape} does not match the reward net's input ({self._basic.mlp.dims[0]})"
            d = self._dev = {"device": dev, "planner": _Planner(self.env, dev), "obs": th.as_tensor(obs).to(dev),
                             "w": th.empty(obs.shape[0], device=dev),
                             "stats": th.zeros(3, dtype=th.float64, device=dev)}
            self._dev_demo = None
        if getattr(self, "_dev_demo", None) is None:
            self._dev_demo = th.as_tensor(np.ascontiguousarray(self.demo_state_om, dtype=np.float64)).to(dev)
        return d

    def train(self, max_iter: int = 1000) -> np.ndarray:
        """Runs MCE IRL for at most `max_iter` iterations; stops early on `linf_eps` or `grad_l2_eps` (`:500-556`).

        Returns:
            State occupancy measure for the final reward function. `self.reward_net` and `self.optimizer` are updated
            in place.
        """
        obs_mat = self.env.observation_matrix
        assert self.demo_state_om is not None
        assert self.demo_state_om.shape == (len(obs_mat),)
        d = self._device_state()
        p: _Planner = d["planner"]
        optim = self._ensure_optimizer()
        mlp = self._basic.mlp
        S, stats, w = p.S, d["stats"], d["w"]
        ws = mlp.train_workspace(S, "mce")
        ws["X"][:, :mlp.dims[0]].copy_(d["obs"])
        ws["_in"] = ws["X"]
        reward = ws["out"].reshape(S)
        fuse = optim.flat.numel() == mlp.n_params
        if max_iter <= 0:
            raise ValueError("max_iter must be positive")   # (the reference fails on its unset `predicted_r_np`)

        with networks.training(self.reward_net):
            for t in range(max_iter):
                # reward predicted for each state by the current model, then the expected number of visits to each
                # state under the soft-optimal policy of that reward (planned undiscounted, see `mce_occupancy_measures`)
                L.call("ia_mlp_forward", C.byref(mlp.desc), L.ptr(mlp.flat), L.ptr(ws["X"]), mlp.ldx, S,
                       L.ptr(ws["hidden"]), L.ptr(ws["out"]), L.ACT_NONE, L.stream())
                p.backup(reward, 1.0)
                p.forward(p.pi, self.discount)
                # dOut = visitations - demo_state_om: the gradient of E_pi[r(S)] - E_D[r(S)]
                L.call("ia_mce_weights", L.ptr(p.Dcum), L.ptr(self._dev_demo), S, L.ptr(w), L.ptr(stats), L.stream())
                mlp.backward_rows(ws, S, w, False, adam=optim if fuse else None)
                if not fuse:
                    optim.step()
                L.call("ia_mce_norms", L.ptr(mlp.grad), L.ptr(mlp.flat), mlp.n_params, L.ptr(stats), L.stream())
                linf_delta, grad_norm, weight_norm = stats.cpu().tolist()   # the iteration's one read-back

                if self.log_interval is not None and 0 == (t % self.log_interval):
                    self.logger.record("iteration", t)
                    self.logger.record("linf_delta", linf_delta)
                    self.logger.record("weight_norm", weight_norm)
                    self.logger.record("grad_norm", grad_norm)
                    self.logger.dump(t)

                if linf_delta <= self.linf_eps or grad_norm <= self.grad_l2_eps:
                    break

        visitations = p.Dcum.cpu().numpy()
        self._predicted_r_np = reward.cpu().numpy()
        p.backup(reward, self.discount)
        self._policy.set_pi(p.pi.cpu().numpy())
        return visitations

    @property
    def policy(self) -> TabularPolicy:
        return self._policy
