"""Density-based reward baseline (`algorithms/density.py:24-423`) on the fused HIP kernel density estimate.

`DensityAlgorithm` keeps the reference's constructor, `set_demonstrations`, `train`, `__call__`, `train_policy`,
`test_policy` and `policy`, and its errors. What changes is the mechanism of the density model:

* the reference fits a `sklearn.neighbors.KernelDensity` tree per timestep and scores a batch one row at a time
  (`density.py:295-360`); here every demonstration group is uploaded once at `train()` (standardised, fp32, with its
  squared norms) and a whole batch of queries -- any mix of timesteps -- is scored by ONE call of
  `ia_kde_log_density` (`imitation_amd/csrc/kde.hip`): an all-pairs fp32 MFMA product with an online log-sum-exp,
  the query rows standardised inside the kernel exactly as `StandardScaler.transform` does on float32 rows;
* the scaler is restated in NumPy (`StandardScaler.fit`'s float64 two-pass moments, its near-constant-feature rule);
* flattening follows `gymnasium.spaces.utils.flatten` for the spaces of `imitation_amd.spaces` (Box: ravel; Discrete:
  one-hot in the space's dtype).

A row's reward does not depend on the batch it is scored in (the kernel's slab rule), so `PPO.collect_rollouts` relabels
a stationary model's whole rollout tile in one call after the last step, with the same bits the per-step calls give.
"""
from __future__ import annotations

import enum
import itertools
import math
from collections.abc import Mapping
from typing import Any, Dict, Iterable, List, Optional

import numpy as np
import torch as th

from imitation_amd import _lib as L
from imitation_amd import data_types as dt
from imitation_amd import rollout, spaces
from imitation_amd.logger import HierarchicalLogger, configure as configure_logger
from imitation_amd.networks import require_device
from imitation_amd.wrappers import BufferingWrapper, RewardVecEnvWrapper

KERNELS = ("gaussian", "tophat", "epanechnikov", "exponential", "linear", "cosine")   # codes of `ia_kde_log_density`


class DensityType(enum.Enum):
    """Input type the density model should use."""

    STATE_DENSITY = enum.auto()
    STATE_ACTION_DENSITY = enum.auto()
    STATE_STATE_DENSITY = enum.auto()


def flatten(space: spaces.Space, x) -> np.ndarray:
    """`gymnasium.spaces.utils.flatten` of one element: Box -> ravel in the space's dtype, Discrete -> one-hot."""
    if isinstance(space, spaces.Box):
        return np.asarray(x, dtype=space.dtype).flatten()
    if isinstance(space, spaces.Discrete):
        onehot = np.zeros(space.n, dtype=space.dtype)
        onehot[int(x)] = 1
        return onehot
    raise NotImplementedError(f"density features of {space!r}: only Box and Discrete spaces are supported")


def flatten_batch(space: spaces.Space, x) -> np.ndarray:
    """`flatten` of every row of a batch, as one array (the same values and dtype, row by row)."""
    x = np.asarray(x)
    if isinstance(space, spaces.Box):
        return np.asarray(x, dtype=space.dtype).reshape(len(x), -1)
    if isinstance(space, spaces.Discrete):
        onehot = np.zeros((len(x), space.n), dtype=space.dtype)
        onehot[np.arange(len(x)), x.reshape(len(x)).astype(np.int64)] = 1
        return onehot
    raise NotImplementedError(f"density features of {space!r}: only Box and Discrete spaces are supported")


class StandardScaler:
    """`sklearn.preprocessing.StandardScaler(with_mean=s, with_std=s).fit` restated: float64 accumulators, the corrected
    two-pass variance, scale 1 for near-constant features. `standardise=False` is the identity (mean 0, scale 1)."""

    def __init__(self, standardise: bool = True):
        self.standardise = standardise
        self.mean_: Optional[np.ndarray] = None
        self.scale_: Optional[np.ndarray] = None

    def fit(self, X: np.ndarray) -> "StandardScaler":
        X = np.asarray(X)
        n, d = X.shape
        if not self.standardise:
            self.mean_, self.scale_ = np.zeros(d), np.ones(d)
            return self
        acc = dict(dtype=np.float64) if (np.issubdtype(X.dtype, np.floating) and X.dtype.itemsize < 8) else {}
        new_sum = np.sum(X, axis=0, **acc)
        mean = new_sum / n
        temp = X - mean
        correction = np.sum(temp, axis=0, **acc)
        temp **= 2
        var = (np.sum(temp, axis=0, **acc) - correction ** 2 / n) / n
        eps = np.finfo(np.float64).eps
        constant = var <= n * eps * var + (n * mean * eps) ** 2
        scale = np.sqrt(var)
        scale[constant] = 1.0
        self.mean_, self.scale_ = mean.astype(np.float64), scale.astype(np.float64)
        return self

    def transform(self, X: np.ndarray) -> np.ndarray:
        """`StandardScaler.transform`: in place in the rows' own dtype, subtraction then division (float32 rows: each step
        in double, rounded to float32 -- what the kernel does to the query rows)."""
        X = np.array(X, copy=True)
        if not np.issubdtype(X.dtype, np.floating):
            X = X.astype(np.float64)
        if self.standardise:
            X -= self.mean_
            X /= self.scale_
        return X


def log_kernel_norm(h: float, d: int, kernel: str) -> float:
    """log of the normaliser of the kernel on R^d with bandwidth h (sklearn's `_log_kernel_norm`), in float64."""
    log_pi, log_2pi = math.log(math.pi), math.log(2 * math.pi)

    def log_vn(n):   # log volume of the unit n-ball
        return 0.5 * n * log_pi - math.lgamma(0.5 * n + 1)

    def log_sn(n):   # log surface of the unit n-sphere (in R^(n+1))
        return log_2pi + log_vn(n - 1)

    if kernel == "gaussian":
        factor = 0.5 * d * log_2pi
    elif kernel == "tophat":
        factor = log_vn(d)
    elif kernel == "epanechnikov":
        factor = log_vn(d) + math.log(2.0 / (d + 2.0))
    elif kernel == "exponential":
        factor = log_sn(d - 1) + math.lgamma(d)
    elif kernel == "linear":
        factor = log_vn(d) - math.log(d + 1.0)
    elif kernel == "cosine":   # integral of cos(pi r / 2) r^(d-1) over [0, 1], by parts
        factor, tmp = 0.0, 2.0 / math.pi
        for k in range(1, d + 1, 2):
            factor += tmp
            tmp *= -(d - k) * (d - k - 1) * (2.0 / math.pi) ** 2
        # (the alternating sum goes negative for some d -- 4 and 23 among them -- where sklearn's C `log` gives NaN and
        #  so does the reference's density: kept, not repaired)
        factor = (math.log(factor) if factor > 0 else -math.inf if factor == 0 else math.nan) + log_sn(d - 1)
    else:
        raise ValueError(f"kernel {kernel!r} not recognized")
    return -factor - d * math.log(h)


class KdeModel:
    """Device-resident kernel density model of one or more demonstration groups (one per timestep for non-stationary
    models) sharing a scaler: the state `ia_kde_log_density` reads."""

    def __init__(self, groups: List[np.ndarray], scaler: StandardScaler, kernel: str, bandwidth: float, device):
        if kernel not in KERNELS:
            raise ValueError(f"kernel {kernel!r} not recognized")
        self.kernel, self.code, self.h = kernel, KERNELS.index(kernel), float(bandwidth)
        self.device = th.device(device)
        require_device(self.device)
        self.d = int(groups[0].shape[1])
        self.tile_rows = L.load().ia_kde_tile_rows(self.d)
        if self.tile_rows < 0:
            raise ValueError(f"kernel density: feature width {self.d} not supported (code {self.tile_rows})")
        std = [scaler.transform(g).astype(np.float32) for g in groups]
        self.ldy = (self.d + 3) & ~3
        Y = np.zeros((sum(len(g) for g in std), self.ldy), np.float32)
        off = np.cumsum([0] + [len(g) for g in std])
        for g, o in zip(std, off):
            Y[o:o + len(g), :self.d] = g
        self.n = np.array([len(g) for g in std], np.int32)
        self.slabs = np.array([L.load().ia_kde_slabs(int(k), self.d) for k in self.n], np.int32)
        self.max_slabs = int(self.slabs.max())
        c = log_kernel_norm(self.h, self.d, kernel)
        dev = lambda a: th.as_tensor(a).to(self.device)
        self.Y = dev(Y)
        self.ynorm = dev(np.square(Y.astype(np.float64)).sum(axis=1).astype(np.float32))
        self.off, self.n_dev = dev(off[:-1].astype(np.int64)), dev(self.n)
        self.gconst = dev(np.array([c - math.log(k) for k in self.n], np.float64))
        self.mean, self.scale = dev(np.asarray(scaler.mean_, np.float64)), dev(np.asarray(scaler.scale_, np.float64))
        self._tiles: Dict[int, th.Tensor] = {}   # stationary tile tables by batch size

    def _tile_table(self, groups_sorted: np.ndarray) -> np.ndarray:
        """(first sorted row, rows, group) per tile: each group's run of the stably sorted rows cut into tiles."""
        bounds = np.flatnonzero(np.diff(groups_sorted)) + 1
        starts = np.concatenate([[0], bounds])
        ends = np.concatenate([bounds, [len(groups_sorted)]])
        out = []
        for s, e in zip(starts, ends):
            for t in range(s, e, self.tile_rows):
                out.append((t, min(self.tile_rows, e - t), groups_sorted[s]))
        return np.asarray(out, np.int32).reshape(-1, 3)

    def log_density_rows(self, rows: th.Tensor, out: th.Tensor, groups: Optional[np.ndarray] = None) -> th.Tensor:
        """out[i] = log p(rows[i]) of group groups[i] (None: group 0 for every row), on the current stream.
        rows: device float32 [B, d] in raw (unstandardised) features; out: device float32 [B]."""
        B = rows.shape[0]
        assert rows.dtype == th.float32 and rows.shape == (B, self.d) and rows.is_contiguous()
        assert out.dtype == th.float32 and out.numel() == B and out.is_contiguous()
        if B == 0:
            return out
        if groups is None:
            perm = None
            tiles = self._tiles.get(B)
            if tiles is None:
                tiles = self._tiles[B] = th.as_tensor(self._tile_table(np.zeros(B, np.int32))).to(self.device)
        else:
            order = np.argsort(groups, kind="stable")
            perm = th.as_tensor(order.astype(np.int32)).to(self.device)
            tiles = th.as_tensor(self._tile_table(np.asarray(groups)[order])).to(self.device)
        partials = th.empty(self.max_slabs, B, 2, dtype=th.float32, device=self.device)
        L.call("ia_kde_log_density", self.code, self.h, self.d, L.ptr(self.Y), self.ldy, L.ptr(self.ynorm),
               L.ptr(self.off), L.ptr(self.n_dev), L.ptr(self.gconst), self.max_slabs, L.ptr(rows), B, L.ptr(self.mean),
               L.ptr(self.scale), L.ptr(perm), L.ptr(tiles), int(tiles.shape[0]), L.ptr(partials), L.ptr(out), 3,
               L.stream())
        return out


class DensityAlgorithm:
    """`algorithms/density.py:37-413`: a reward `log p_hat(s)`, `log p_hat(s, a)` or `log p_hat(s, s')` from a kernel
    density estimate of the demonstrations (per timestep when `is_stationary` is False)."""

    def __init__(self, *, demonstrations, venv, rng: np.random.Generator,
                 density_type: DensityType = DensityType.STATE_ACTION_DENSITY, kernel: str = "gaussian",
                 kernel_bandwidth: float = 0.5, rl_algo=None, is_stationary: bool = True, standardise_inputs: bool = True,
                 custom_logger: Optional[HierarchicalLogger] = None, allow_variable_horizon: bool = False, device=None):
        self.is_stationary = is_stationary
        self.density_type = density_type
        self.venv = venv
        self.transitions: Dict[Optional[int], np.ndarray] = dict()
        self._logger = custom_logger or configure_logger()
        self.allow_variable_horizon = allow_variable_horizon
        self._horizon = None
        if demonstrations is not None:
            self.set_demonstrations(demonstrations)
        self.kernel = kernel
        self.kernel_bandwidth = kernel_bandwidth
        self.standardise = standardise_inputs
        self._scaler: Optional[StandardScaler] = None
        self._model: Optional[KdeModel] = None
        self._keys: List[Optional[int]] = []
        self.rng = rng
        self.rl_algo = rl_algo
        if device is None:
            device = rl_algo.device if rl_algo is not None else th.device("cuda", th.cuda.current_device()) \
                if th.cuda.is_available() else th.device("cpu")
        self.device = th.device(device)
        self.buffering_wrapper = BufferingWrapper(self.venv)
        self.venv_wrapped = RewardVecEnvWrapper(self.buffering_wrapper, self)
        self.wrapper_callback = self.venv_wrapped.make_log_callback()

    # ---- `algorithms/base.py` surface
    @property
    def logger(self) -> HierarchicalLogger:
        return self._logger

    @logger.setter
    def logger(self, value: HierarchicalLogger) -> None:
        self._logger = value

    def _check_fixed_horizon(self, horizons: Iterable[int]) -> None:
        """`algorithms/base.py:77-110`."""
        if self.allow_variable_horizon:
            return
        hs = set(int(h) for h in horizons)
        if self._horizon is not None:
            hs.add(self._horizon)
        if len(hs) > 1:
            raise ValueError(f"Episodes of different length detected: {hs}. Variable horizon environments are "
                             "discouraged -- termination conditions leak information about reward. If you are SURE "
                             "you want to run imitation on a variable horizon task, then please pass in the flag: "
                             "`allow_variable_horizon=True`.")
        if len(hs) == 1:
            self._horizon = hs.pop()

    # ---- demonstrations
    def _flat_batch(self, obs, act, next_obs) -> np.ndarray:
        """`_preprocess_transition` of every row of a batch (the same values and dtype, row by row)."""
        ob_space, ac_space = self.venv.observation_space, self.venv.action_space
        if isinstance(obs, Mapping):
            raise NotImplementedError("Dict observations: imitation_amd.spaces has no Dict space")
        flat_obs = flatten_batch(ob_space, obs)
        if self.density_type == DensityType.STATE_DENSITY:
            return flat_obs
        if self.density_type == DensityType.STATE_ACTION_DENSITY:
            return np.concatenate([flat_obs, flatten_batch(ac_space, act)], axis=1)
        if self.density_type == DensityType.STATE_STATE_DENSITY:
            assert next_obs is not None
            return np.concatenate([flat_obs, flatten_batch(ob_space, next_obs)], axis=1)
        raise ValueError(f"Unknown density type {self.density_type}")

    def _get_demo_from_batch(self, obs_b, act_b, next_obs_b) -> Dict[Optional[int], List[np.ndarray]]:
        if next_obs_b is None and self.density_type == DensityType.STATE_STATE_DENSITY:
            raise ValueError("STATE_STATE_DENSITY requires next_obs_b to be provided, but it was None")
        if isinstance(obs_b, Mapping):
            raise NotImplementedError("Dict observations: imitation_amd.spaces has no Dict space")
        obs_b, act_b = np.asarray(obs_b), np.asarray(act_b)
        assert act_b.shape[1:] == self.venv.action_space.shape
        assert obs_b.shape[1:] == self.venv.observation_space.shape
        assert len(act_b) == len(obs_b)
        if next_obs_b is not None:
            next_obs_b = np.asarray(next_obs_b)
            assert next_obs_b.shape == obs_b.shape
        return {None: list(self._flat_batch(obs_b, act_b, next_obs_b))}

    def set_demonstrations(self, demonstrations) -> None:
        """Trajectories (keyed by timestep), `Transitions` (under the `None` key) or an iterable of batch mappings."""
        transitions: Dict[Optional[int], List[np.ndarray]] = {}
        if isinstance(demonstrations, dt.Transitions) or (
                hasattr(demonstrations, "obs") and hasattr(demonstrations, "acts") and not hasattr(demonstrations, "terminal")):
            transitions.update(self._get_demo_from_batch(demonstrations.obs, demonstrations.acts,
                                                         getattr(demonstrations, "next_obs", None)))
        elif isinstance(demonstrations, Iterable):
            it = iter(demonstrations)
            try:
                first = next(it)
            except StopIteration:
                raise ValueError("No elements in demonstrations")   # (`util.get_first_iter_element`)
            demonstrations = itertools.chain([first], it)
            if hasattr(first, "obs") and hasattr(first, "acts") and hasattr(first, "terminal"):
                for traj in demonstrations:
                    rows = self._flat_batch(np.asarray(traj.obs[:-1]), np.asarray(traj.acts), np.asarray(traj.obs[1:]))
                    for i, row in enumerate(rows):
                        transitions.setdefault(i, []).append(row)
            elif isinstance(first, Mapping):
                for batch in demonstrations:
                    obs = _to_numpy(batch["obs"])
                    acts = _to_numpy(batch["acts"])
                    next_obs = batch.get("next_obs")
                    next_obs = None if next_obs is None else _to_numpy(next_obs)
                    transitions.update(self._get_demo_from_batch(obs, acts, next_obs))
            else:
                raise TypeError(f"Unsupported demonstration type {type(demonstrations)}")
        else:
            raise TypeError(f"Unsupported demonstration type {type(demonstrations)}")

        self.transitions = {k: np.stack(v, axis=0) for k, v in transitions.items()}
        if not self.is_stationary and None in self.transitions:
            raise ValueError("Non-stationary model incompatible with non-trajectory demonstrations.")
        if self.is_stationary:
            self.transitions = {None: np.concatenate(list(self.transitions.values()), axis=0)}

    # ---- the density model
    def train(self) -> None:
        """Fits the scaler on all demonstration rows (in the reference's key order) and uploads every group."""
        require_device(self.device)
        self._scaler = StandardScaler(self.standardise).fit(np.concatenate(list(self.transitions.values()), axis=0))
        self._keys = list(self.transitions.keys())
        self._model = KdeModel([self.transitions[k] for k in self._keys], self._scaler, self.kernel,
                               self.kernel_bandwidth, self.device)
        self._group_of = {k: g for g, k in enumerate(self._keys)}

    @property
    def model(self) -> KdeModel:
        assert self._model is not None, "call train() first"
        return self._model

    def __call__(self, state, action, next_state, done, steps: Optional[np.ndarray] = None) -> np.ndarray:
        """`r_t(s, a, s') = log p_hat_t(s, a, s')` of a batch, float32 [B], from one kernel call."""
        if not self.is_stationary and steps is None:
            raise ValueError("steps must be provided with non-stationary models")
        del done
        assert len(state) == len(action) and len(state) == len(next_state)
        assert self._scaler is not None and self._model is not None
        groups = None
        if not self.is_stationary:
            steps = np.asarray(steps)
            n_models = len(self._keys)
            for time in steps:
                if time >= n_models:
                    raise ValueError(f"Time {time} out of range (0, {n_models}], "
                                     "and absorbing states not currently supported")
            groups = np.array([self._group_of[int(t)] for t in steps], np.int32)
        flat = self._flat_batch(np.asarray(state), np.asarray(action), np.asarray(next_state))
        rows = th.as_tensor(np.ascontiguousarray(flat, dtype=np.float32)).to(self.device)
        out = th.empty(len(flat), dtype=th.float32, device=self.device)
        self._model.log_density_rows(rows, out, groups)
        return out.cpu().numpy()

    def relabel_rollout(self, obs: th.Tensor, acts: th.Tensor, next_obs: th.Tensor, out: th.Tensor,
                        discrete: bool) -> None:
        """Rewards of a rollout tile straight from device tensors (`PPO.collect_rollouts`' bulk relabelling of a stationary
        model): obs / next_obs [T, n, obs_dim], acts [T, n, act_width] (Discrete: the action index), out [T, n]. The rows
        are the ones `__call__` would build from the same steps, so the rewards are the same bits."""
        T, n = out.shape
        S = obs.reshape(T * n, -1)
        if self.density_type == DensityType.STATE_DENSITY:
            rows = S
        elif self.density_type == DensityType.STATE_ACTION_DENSITY:
            A = acts.reshape(T * n, -1)
            if discrete:
                A = th.nn.functional.one_hot(A[:, 0].long(), self.venv.action_space.n).to(th.float32)
            rows = th.cat([S, A], dim=1)
        else:
            rows = th.cat([S, next_obs.reshape(T * n, -1)], dim=1)
        self.model.log_density_rows(rows.contiguous(), out.view(-1))

    # ---- RL on the learned reward
    def train_policy(self, n_timesteps: int = int(1e6), **kwargs: Any) -> None:
        """`density.py:362-381`."""
        assert self.rl_algo is not None
        self.rl_algo.set_env(self.venv_wrapped)
        self.rl_algo.learn(n_timesteps, reset_num_timesteps=False, callback=self.wrapper_callback, **kwargs)
        trajs, ep_lens = self.buffering_wrapper.pop_trajectories()
        self._check_fixed_horizon(ep_lens)

    def test_policy(self, *, n_trajectories: int = 10, true_reward: bool = True):
        """`density.py:383-406`: rollout statistics of the current policy on the true or the imitation reward."""
        trajs = rollout.generate_trajectories(self.rl_algo, self.venv if true_reward else self.venv_wrapped,
                                              sample_until=rollout.make_min_episodes(n_trajectories), rng=self.rng)
        self.buffering_wrapper.pop_trajectories()
        self._check_fixed_horizon(len(traj) for traj in trajs)
        return rollout.rollout_stats(trajs)

    @property
    def policy(self):
        assert self.rl_algo is not None
        assert self.rl_algo.policy is not None
        return self.rl_algo.policy


def _to_numpy(x) -> np.ndarray:
    if isinstance(x, th.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)
