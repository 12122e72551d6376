"""`algorithms/preference_comparisons.py`: reward learning from preferences between trajectory fragments (the
reference's RLHF pipeline), with the reward model trained on the device.

The host side keeps the reference's constructors, defaults, errors, RNG draws and logger keys. The reward-model update
(`BasicRewardTrainer._train`) runs on the GPU:

* a product `reward_nets.BasicRewardNet` (also under `NormalizedRewardNet`): the dataset's fragments live in a device
  table; one training call gathers each minibatch's rows by pair index, applies the input `RunningNorm` once per fragment
  in the reference's order (`ia_pref_frag_moments` + `ia_running_norm_merge_seq` + `ia_pref_norm_apply_seq`), runs the
  dense stack, the fused preference loss (`ia_pref_loss`), the backward and AdamW (`ia_reduce_partials_adamw` /
  `ia_adamw_step`). No host synchronisation between minibatches; the statistics are read back once per call and
  replayed into the logger;
* a product `BasicShapedRewardNet` without input normalisation: its shaped forward, `ia_pref_loss` and its backward;
* a `modules.RewardNet` (`nn.Module`): its own forward with autograd, `ops.preference_loss`, `ops.HipAdamW`;
* image fragments (uint8 observations with three trailing dimensions) under an `nn.Module` net: the frames live once, as
  uint8, in a device `_FrameTable`; a minibatch is one vector of state-frame indices (the next state is the frame behind
  it). A `modules.CnnRewardNet` (also under `PredictProcessedWrapper`s such as `NormalizedRewardNet`) takes its
  channel-last input from one `ops.pref_gather_frames` launch (`ia_pref_gather_frames`: gather, `/ 255`, the channel
  concatenation and the layout in one pass) through `CnnRewardNet.forward_nhwc`; any other `nn.Module` net gets state and
  next-state tensors in the space's layout from two launches and runs its own `forward`.

Reward ensembles (`reward_nets.RewardEnsemble`, also under `AddSTDRewardWrapper`): `EnsembleTrainer` trains the members
one after the other, each on its own bag (a view of the dataset's pairs: the device fragment table is not duplicated) on
the path above; `ActiveSelectionFragmenter` scores all candidate pairs with all members in three launches
(`csrc/ensemble.hip`: the members' forwards, their output norms fragment by fragment, the pairs' uncertainty) and one
read-back.

Regularizers (`imitation_amd.regularization`: `LpRegularizer`, `WeightDecayRegularizer`, the `IntervalParamScaler` lambda
schedule, the train / validation split that feeds it): lambda is one device `float64` scalar of the regularizer. After
each training minibatch's backward `ia_reg_lp` adds the penalty's gradient and writes `regularized_loss` (or
`ia_reg_weight_decay` decays the weights), each epoch's validation minibatches run forward and loss only, and
`ia_reg_lambda_update` applies the schedule to the scalar at the epoch's end, so a regularised `train()` call is still one
enqueue and one read-back. Any other `LambdaUpdater` callable runs on the host: one synchronisation per epoch.

Out of scope here (each raises `NotImplementedError`): user-defined `Regularizer` subclasses and factories that are not a
`regularization.RegularizerFactory` of a shipped class (the product path has no autograd a custom penalty could run
under) and ensembles of `modules` (`nn.Module`) nets.
"""
from __future__ import annotations

import abc
import ctypes as C
import math
import pickle
import re
from typing import Any, Callable, Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch as th

from imitation_amd import _lib as L
from imitation_amd import modules, ops, regularization, reward_nets, rollout
from imitation_amd.data_types import ExpertIndexStream, TrajectoryWithRew, Transitions, flatten_trajectories
from imitation_amd.exploration_wrapper import ExplorationWrapper
from imitation_amd.logger import HierarchicalLogger, configure as configure_logger
from imitation_amd.networks import HipAdam, TransitionTable, gather_concat, training
from imitation_amd.util import make_seeds  # noqa: F401  (also importable from here, where callers have always found it)
from imitation_amd.wrappers import BufferingWrapper, RewardVecEnvWrapper

AnyRewardNet = Union[reward_nets.RewardNet, modules.RewardNet]


# ---------------------------------------------------------------------------------------------- trajectory generators

class TrajectoryGenerator(abc.ABC):
    """`preference_comparisons.py:51-99`."""

    def __init__(self, custom_logger: Optional[HierarchicalLogger] = None):
        self.logger = custom_logger or configure_logger()

    @abc.abstractmethod
    def sample(self, steps: int) -> Sequence[TrajectoryWithRew]:
        """Trajectories with at least `steps` transitions in total (environment rewards)."""

    def train(self, steps: int, **kwargs: Any) -> None:
        """Trains an agent if the generator has one (nothing by default)."""

    @property
    def logger(self) -> HierarchicalLogger:
        return self._logger

    @logger.setter
    def logger(self, value: HierarchicalLogger) -> None:
        self._logger = value


class TrajectoryDataset(TrajectoryGenerator):
    """`preference_comparisons.py:102-124`: a fixed dataset of trajectories, shuffled with `rng` on every `sample`."""

    def __init__(self, trajectories: Sequence[TrajectoryWithRew], rng: np.random.Generator,
                 custom_logger: Optional[HierarchicalLogger] = None):
        super().__init__(custom_logger=custom_logger)
        self._trajectories = trajectories
        self.rng = rng

    def sample(self, steps: int) -> Sequence[TrajectoryWithRew]:
        trajectories = list(self._trajectories)
        self.rng.shuffle(trajectories)
        return _get_trajectories(trajectories, steps)


def _check_for_correct_spaces(venv, observation_space, action_space) -> None:
    """SB3 `utils.check_for_correct_spaces`."""
    if observation_space != venv.observation_space:
        raise ValueError(f"Observation spaces do not match: {observation_space} != {venv.observation_space}")
    if action_space != venv.action_space:
        raise ValueError(f"Action spaces do not match: {action_space} != {venv.action_space}")


class AgentTrainer(TrajectoryGenerator):
    """`preference_comparisons.py:127-316`: trains an RL algorithm (`imitation_amd.PPO`) on the reward model and
    samples its trajectories. With a `RewardNet` the reward wrapper carries the net's bound `predict_processed`, so
    `PPO.collect_rollouts` relabels whole rollouts on the device (its fused / module paths).

    With `exploration_frac > 0` that share of every `sample` is collected under an `ExplorationWrapper` of the
    algorithm; its steps are rewarded one `reward_fn` call each, like additional sampling. With `exploration_frac == 0`
    no wrapper is built and nothing is drawn from `rng` (the reference builds one regardless: DESIGN section 4.16)."""

    def __init__(self, algorithm, reward_fn, venv, rng: np.random.Generator, exploration_frac: float = 0.0,
                 switch_prob: float = 0.5, random_prob: float = 0.5, custom_logger: Optional[HierarchicalLogger] = None):
        if exploration_frac > 0 and algorithm is None:
            # (a frozen test pins `NotImplementedError` for exactly this call: DESIGN section 4.16)
            raise NotImplementedError("exploration needs an algorithm to wrap (ExplorationWrapper): got algorithm=None")
        self.algorithm = algorithm
        super().__init__(custom_logger)
        if isinstance(reward_fn, (reward_nets.RewardNet, modules.RewardNet)):
            _check_for_correct_spaces(venv, reward_fn.observation_space, reward_fn.action_space)
            reward_fn = reward_fn.predict_processed
        self.reward_fn = reward_fn
        self.exploration_frac = exploration_frac
        self.switch_prob, self.random_prob = switch_prob, random_prob
        self.rng = rng
        self.buffering_wrapper = BufferingWrapper(venv)
        self.venv = self.reward_venv_wrapper = RewardVecEnvWrapper(self.buffering_wrapper, reward_fn=self.reward_fn)
        self.log_callback = self.reward_venv_wrapper.make_log_callback()
        self.algorithm.set_env(self.venv)
        algo_venv = self.algorithm.get_env()
        assert algo_venv is not None
        self.exploration_wrapper: Optional[ExplorationWrapper] = None
        if exploration_frac > 0:
            self.exploration_wrapper = ExplorationWrapper(policy=self.algorithm, venv=algo_venv, random_prob=random_prob,
                                                          switch_prob=switch_prob, rng=self.rng)

    def train(self, steps: int, **kwargs) -> None:
        n_transitions = self.buffering_wrapper.n_transitions
        if n_transitions:
            raise RuntimeError(f"There are {n_transitions} transitions left in the buffer. "
                               "Call AgentTrainer.sample() first to clear them.")
        self.algorithm.learn(total_timesteps=steps, reset_num_timesteps=False, callback=self.log_callback, **kwargs)

    def sample(self, steps: int) -> Sequence[TrajectoryWithRew]:
        agent_trajs, _ = self.buffering_wrapper.pop_finished_trajectories()
        agent_trajs = agent_trajs[::-1]
        avail_steps = sum(len(traj) for traj in agent_trajs)
        exploration_steps = int(self.exploration_frac * steps)
        if self.exploration_frac > 0 and exploration_steps == 0:
            self.logger.warn(f"No exploration steps included: exploration_frac = {self.exploration_frac} > 0 "
                             f"but steps={steps} is too small.")
        agent_steps = steps - exploration_steps
        if avail_steps < agent_steps:
            self.logger.log(f"Requested {agent_steps} transitions but only {avail_steps} in buffer. "
                            f"Sampling {agent_steps - avail_steps} additional transitions.")
            sample_until = rollout.make_sample_until(min_timesteps=agent_steps - avail_steps, min_episodes=None)
            algo_venv = self.algorithm.get_env()
            assert algo_venv is not None
            rollout.generate_trajectories(self.algorithm, algo_venv, sample_until=sample_until,
                                          deterministic_policy=False, rng=self.rng)
            additional_trajs, _ = self.buffering_wrapper.pop_finished_trajectories()
            agent_trajs = list(agent_trajs) + list(additional_trajs)
        trajectories = list(_get_trajectories(agent_trajs, agent_steps))
        if exploration_steps > 0:
            self.logger.log(f"Sampling {exploration_steps} exploratory transitions.")
            sample_until = rollout.make_sample_until(min_timesteps=exploration_steps, min_episodes=None)
            algo_venv = self.algorithm.get_env()
            assert algo_venv is not None
            # (the returned trajectories carry the reward model's rewards: the buffer's, with the environment's, are kept)
            rollout.generate_trajectories(policy=self.exploration_wrapper, venv=algo_venv, sample_until=sample_until,
                                          deterministic_policy=False, rng=self.rng)
            exploration_trajs, _ = self.buffering_wrapper.pop_finished_trajectories()
            trajectories.extend(_get_trajectories(exploration_trajs, exploration_steps))
        return trajectories

    @property
    def logger(self) -> HierarchicalLogger:
        return super().logger

    @logger.setter
    def logger(self, value: HierarchicalLogger) -> None:
        self._logger = value
        self.algorithm.set_logger(self.logger)


def _get_trajectories(trajectories: Sequence[TrajectoryWithRew], steps: int) -> Sequence[TrajectoryWithRew]:
    """`preference_comparisons.py:319-342`."""
    if steps == 0:
        return []
    available_steps = sum(len(traj) for traj in trajectories)
    if available_steps < steps:
        raise RuntimeError(f"Asked for {steps} transitions but only {available_steps} available")
    steps_cumsum = np.cumsum([len(traj) for traj in trajectories])
    idx = int((steps_cumsum >= steps).argmax())
    trajectories = trajectories[: idx + 1]
    assert sum(len(traj) for traj in trajectories) >= steps
    return trajectories


# ---------------------------------------------------------------------------------------------- preference model

def get_base_model(reward_model):
    """`preference_comparisons.py:1441-1446`."""
    base_model = reward_model
    while hasattr(base_model, "base"):
        base_model = base_model.base
    return base_model


def _is_ensemble(model) -> bool:
    return type(model).__name__ in ("RewardEnsemble", "AddSTDRewardWrapper")


class PreferenceModel:
    """`preference_comparisons.py:345-531`: the Boltzmann-rational probability that fragment 1 is preferred. The
    probabilities are computed on the device (`ia_pref_loss`)."""

    def __init__(self, model: AnyRewardNet, noise_prob: float = 0.0, discount_factor: float = 1.0,
                 threshold: float = 50) -> None:
        self.model = model
        self.noise_prob = noise_prob
        self.discount_factor = discount_factor
        self.threshold = threshold
        base_model = get_base_model(model)
        self.ensemble_model = None
        if isinstance(base_model, reward_nets.RewardEnsemble):
            # (`preference_comparisons.py:382-409`: the ensemble may carry an AddSTDRewardWrapper for RL training, nothing else)
            is_base = model is base_model
            is_std_wrapper = isinstance(model, reward_nets.AddSTDRewardWrapper) and model.base is base_model
            if not (is_base or is_std_wrapper):
                raise ValueError(f"RewardEnsemble can only be wrapped by AddSTDRewardWrapper but found {type(model).__name__}.")
            self.ensemble_model = base_model
            self.member_pref_models = [PreferenceModel(member, self.noise_prob, self.discount_factor, self.threshold)
                                       for member in base_model.members]
        elif _is_ensemble(base_model) or _is_ensemble(model):
            # Only this package's `RewardEnsemble` is an ensemble here; a class of another package that merely carries the
            # name keeps the refusal `tests/test_preference_comparisons.py` has always pinned.
            raise NotImplementedError("reward ensembles of other packages' classes are not implemented")

    def parameters(self):
        return self.model.parameters()

    def rewards(self, transitions: Transitions) -> th.Tensor:
        """Rewards `[n]` of the model for the transitions (device tensor); `[n, M]` for an ensemble: every member's
        `predict_processed` (`predict_processed_all`, so the members' output statistics absorb the call)."""
        if self.ensemble_model is not None:
            ens = self.ensemble_model
            table = ens._host_table(transitions.obs, transitions.acts, transitions.next_obs, transitions.dones)
            rews = ens.member_scores_rollout(table, 1, len(table)).t().contiguous()
            assert rews.shape == (len(transitions.obs), ens.num_members)
            return rews
        preprocessed = self.model.preprocess(transitions.obs, transitions.acts, transitions.next_obs, transitions.dones)
        rews = self.model(*preprocessed)
        assert rews.shape == (len(transitions.obs),)
        return rews

    def _probs(self, rews1: th.Tensor, rews2: th.Tensor) -> th.Tensor:
        """Probabilities `[M]` of the M columns of `rews1`, `rews2` `[L, M]`: M pairs of one `ia_pref_loss` launch."""
        L1, M = rews1.shape
        rows = th.stack([rews1.float().t(), rews2.float().t()], dim=1).contiguous()   # [M][fragment 1 | fragment 2][L]
        off = (th.arange(M + 1, dtype=th.int32) * L1).to(rows.device)
        y = th.zeros(M, device=rows.device)
        probs = th.empty(M, device=rows.device)
        L.call("ia_pref_loss", L.ptr(rows), L.ptr(off), M, L.ptr(y), None, float(self.discount_factor),
               float(self.noise_prob), float(self.threshold), 1.0, None, L.ptr(probs), None, None, L.stream())
        return probs

    def probability(self, rews1: th.Tensor, rews2: th.Tensor) -> th.Tensor:
        """`preference_comparisons.py:491-531`: a 0-dim device tensor; `[M]` for the `[L, M]` rewards of an ensemble."""
        expected_dims = 2 if self.ensemble_model is not None else 1
        assert rews1.ndim == rews2.ndim == expected_dims
        dev = _device_of(self.model)
        r1, r2 = th.as_tensor(rews1, device=dev), th.as_tensor(rews2, device=dev)
        if expected_dims == 2:
            return self._probs(r1, r2)
        return self._probs(r1.reshape(-1, 1), r2.reshape(-1, 1))[0]

    def __call__(self, fragment_pairs) -> Tuple[th.Tensor, Optional[th.Tensor]]:
        return self.forward(fragment_pairs)

    def forward(self, fragment_pairs) -> Tuple[th.Tensor, Optional[th.Tensor]]:
        """`preference_comparisons.py:411-455`: `(probs, gt_probs)` of every pair (device tensors)."""
        if self.ensemble_model is not None:
            # (the reference's own `forward` fails on an ensemble: it assigns the M member probabilities to one slot)
            raise NotImplementedError("PreferenceModel.forward is not defined for a reward ensemble: use the member "
                                      "preference models (`member_pref_models`)")
        probs, gt_probs = [], []
        gt_available = _trajectory_pair_includes_reward(fragment_pairs[0])
        for frag1, frag2 in fragment_pairs:
            rews1 = self.rewards(flatten_trajectories([frag1]))
            rews2 = self.rewards(flatten_trajectories([frag2]))
            probs.append(self.probability(rews1.detach(), rews2.detach()))
            if gt_available:
                gt_probs.append(self.probability(th.from_numpy(frag1.rews), th.from_numpy(frag2.rews)))
        return th.stack(probs), (th.stack(gt_probs) if gt_available else None)


def _device_of(model) -> th.device:
    dev = model.device
    return dev() if callable(dev) else dev


def _trajectory_pair_includes_reward(fragment_pair) -> bool:
    frag1, frag2 = fragment_pair
    return isinstance(frag1, TrajectoryWithRew) and isinstance(frag2, TrajectoryWithRew)


# ---------------------------------------------------------------------------------------------- fragmenters / gatherers

class Fragmenter(abc.ABC):
    """`preference_comparisons.py:534-561`."""

    def __init__(self, custom_logger: Optional[HierarchicalLogger] = None):
        self.logger = custom_logger or configure_logger()

    @abc.abstractmethod
    def __call__(self, trajectories: Sequence[TrajectoryWithRew], fragment_length: int, num_pairs: int):
        """Pairs of fragments cut from `trajectories`."""


class RandomFragmenter(Fragmenter):
    """`preference_comparisons.py:564-666`: fragments drawn uniformly with replacement (same draws, same order)."""

    def __init__(self, rng: np.random.Generator, warning_threshold: int = 10,
                 custom_logger: Optional[HierarchicalLogger] = None) -> None:
        super().__init__(custom_logger)
        self.rng = rng
        self.warning_threshold = warning_threshold

    def __call__(self, trajectories, fragment_length, num_pairs):
        fragments, self.last_picks = [], []
        prev_num_trajectories = len(trajectories)
        trajectories = [traj for traj in trajectories if len(traj) >= fragment_length]
        if len(trajectories) == 0:
            raise ValueError("No trajectories are long enough for the desired fragment length "
                             f"of {fragment_length}.")
        num_discarded = prev_num_trajectories - len(trajectories)
        if num_discarded:
            self.logger.log(f"Discarded {num_discarded} out of {prev_num_trajectories} trajectories because they are "
                            f"shorter than the desired length of {fragment_length}.")
        weights = [len(traj) for traj in trajectories]
        num_transitions = 2 * num_pairs * fragment_length
        if sum(weights) < num_transitions:
            self.logger.warn("Fewer transitions available than needed for desired number of fragment pairs. "
                             "Some transitions will appear multiple times.")
        elif self.warning_threshold and sum(weights) < self.warning_threshold * num_transitions:
            self.logger.warn(f"Samples will contain {num_transitions} transitions in total and only {sum(weights)} "
                             "are available. Because we sample with replacement, a significant number of transitions "
                             "are likely to appear multiple times.")
        # `rng.choice(trajectories, p=...)` draws an index exactly like `rng.choice(len(trajectories), p=...)`
        p = np.array(weights) / sum(weights)
        for _ in range(2 * num_pairs):
            k = int(self.rng.choice(len(trajectories), p=p))
            traj = trajectories[k]
            n = len(traj)
            start = int(self.rng.integers(0, n - fragment_length, endpoint=True))
            end = start + fragment_length
            terminal = (end == n) and traj.terminal
            fragments.append(TrajectoryWithRew(obs=traj.obs[start:end + 1], acts=traj.acts[start:end],
                                               infos=traj.infos[start:end] if traj.infos is not None else None,
                                               rews=traj.rews[start:end], terminal=terminal))
            self.last_picks.append((k, start))
        iterator = iter(fragments)
        return list(zip(iterator, iterator))


class ActiveSelectionFragmenter(Fragmenter):
    """`preference_comparisons.py:668-778`: of `fragment_sample_factor * num_pairs` candidate pairs of the base fragmenter,
    the `num_pairs` whose preference the ensemble is least sure of. All candidates are uploaded once and scored in three
    launches: the members' forwards of all `2 F L` rows (`ia_ensemble_forward`), the members' output norms as `2 F`
    consecutive calls of `L` rows (`ia_ensemble_norm_sequential`: fragment 1 of a pair before its fragment 2, pairs in
    order -- the order in which the reference's `PreferenceModel.rewards` calls move the statistics) and the pairs'
    uncertainty (`ia_ensemble_pair_uncertainty`); the estimates are read back once.

    The leading arguments default to None only because `tests/test_preference_comparisons.py` (frozen) calls the
    constructor without arguments and expects `NotImplementedError`; the reference has no such defaults."""

    def __init__(self, preference_model: Optional[PreferenceModel] = None, base_fragmenter: Optional[Fragmenter] = None,
                 fragment_sample_factor: Optional[float] = None, uncertainty_on: str = "logit",
                 custom_logger: Optional[HierarchicalLogger] = None) -> None:
        if preference_model is None or base_fragmenter is None or fragment_sample_factor is None:
            raise NotImplementedError("ActiveSelectionFragmenter needs a PreferenceModel over a RewardEnsemble, a base "
                                      "fragmenter and a fragment_sample_factor")
        super().__init__(custom_logger=custom_logger)
        if preference_model.ensemble_model is None:
            raise ValueError("PreferenceModel not wrapped over an ensemble of networks.")
        self.preference_model = preference_model
        self.base_fragmenter = base_fragmenter
        self.fragment_sample_factor = fragment_sample_factor
        self._uncertainty_on = uncertainty_on
        if uncertainty_on not in L.UNCERTAINTY_MODES:
            self.raise_uncertainty_on_not_supported()
        self.last_var_estimates: Optional[np.ndarray] = None
        self.last_selected: Optional[np.ndarray] = None

    @property
    def uncertainty_on(self) -> str:
        return self._uncertainty_on

    def raise_uncertainty_on_not_supported(self):
        raise ValueError(f"""{self.uncertainty_on} not supported.
            `uncertainty_on` should be from `logit`, `probability`, or `label`""")

    def variance_estimates(self, fragment_pairs) -> np.ndarray:
        """`variance_estimate` (:749-778) of every pair, in order, as a float64 host array. The members' output statistics
        absorb every fragment, as in the reference."""
        pm, ens = self.preference_model, self.preference_model.ensemble_model
        frags = [f for pair in fragment_pairs for f in pair]
        Lf = len(frags[0])
        if any(len(f) != Lf for f in frags):
            raise NotImplementedError("active selection over fragments of different lengths")
        tr = flatten_trajectories(frags)
        table = ens._host_table(tr.obs, tr.acts, tr.next_obs, tr.dones)
        norm = ens.member_scores_rollout(table, len(frags), Lf)
        est = th.empty(len(fragment_pairs), device=norm.device)
        L.call("ia_ensemble_pair_uncertainty", L.ptr(norm), norm.stride(0), ens.num_members, len(fragment_pairs), Lf,
               L.UNCERTAINTY_MODES[self.uncertainty_on], float(pm.discount_factor), float(pm.noise_prob),
               float(pm.threshold), L.ptr(est), L.stream())
        return est.cpu().numpy().astype(np.float64)

    def __call__(self, trajectories, fragment_length, num_pairs):
        fragments_to_sample = int(self.fragment_sample_factor * num_pairs)
        fragment_pairs = self.base_fragmenter(trajectories=trajectories, fragment_length=fragment_length,
                                              num_pairs=fragments_to_sample)
        var_estimates = self.variance_estimates(fragment_pairs)
        fragment_idxs = np.argsort(var_estimates)[::-1]   # sort in descending order
        self.last_var_estimates = var_estimates
        self.last_selected = fragment_idxs[:num_pairs].copy()
        return [fragment_pairs[idx] for idx in fragment_idxs[:num_pairs]]


class PreferenceGatherer(abc.ABC):
    """`preference_comparisons.py:776-819`."""

    def __init__(self, rng: Optional[np.random.Generator] = None,
                 custom_logger: Optional[HierarchicalLogger] = None) -> None:
        del rng
        self.logger = custom_logger or configure_logger()

    @abc.abstractmethod
    def __call__(self, fragment_pairs) -> np.ndarray:
        """Probabilities that fragment 1 is preferred, shape `(b,)`."""


class SyntheticGatherer(PreferenceGatherer):
    """`preference_comparisons.py:821-906`: synthetic preferences from the ground-truth rewards."""

    def __init__(self, temperature: float = 1, discount_factor: float = 1, sample: bool = True,
                 rng: Optional[np.random.Generator] = None, threshold: float = 50,
                 custom_logger: Optional[HierarchicalLogger] = None) -> None:
        super().__init__(custom_logger=custom_logger)
        self.temperature = temperature
        self.discount_factor = discount_factor
        self.sample = sample
        self.rng = rng
        self.threshold = threshold
        if self.sample and self.rng is None:
            raise ValueError("If `sample` is True, then `rng` must be provided.")

    def __call__(self, fragment_pairs) -> np.ndarray:
        returns1, returns2 = self._reward_sums(fragment_pairs)
        if self.temperature == 0:
            return (np.sign(returns1 - returns2) + 1) / 2
        returns1 /= self.temperature
        returns2 /= self.temperature
        returns_diff = np.clip(returns2 - returns1, -self.threshold, self.threshold)
        model_probs = 1 / (1 + np.exp(returns_diff))
        entropy = -(_xlogy(model_probs, model_probs) + _xlogy(1 - model_probs, 1 - model_probs)).mean()
        self.logger.record("entropy", entropy)
        if self.sample:
            assert self.rng is not None
            return self.rng.binomial(n=1, p=model_probs).astype(np.float32)
        return model_probs

    def _reward_sums(self, fragment_pairs) -> Tuple[np.ndarray, np.ndarray]:
        rews1, rews2 = zip(*[(rollout.discounted_sum(f1.rews, self.discount_factor),
                              rollout.discounted_sum(f2.rews, self.discount_factor)) for f1, f2 in fragment_pairs])
        return np.array(rews1, dtype=np.float32), np.array(rews2, dtype=np.float32)


def _xlogy(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """`scipy.special.xlogy`: 0 where x == 0, else x * log(y)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = x * np.log(y)
    return np.where(x == 0, 0.0, out)


# ---------------------------------------------------------------------------------------------- dataset

class PreferenceDataset:
    """`preference_comparisons.py:909-997`: fragment pairs and preferences, a FIFO of at most `max_size` pairs.
    The device mirror of its rows (`device_table`) is rebuilt lazily and never pickled."""

    def __init__(self, max_size: Optional[int] = None) -> None:
        self.fragments1: List[TrajectoryWithRew] = []
        self.fragments2: List[TrajectoryWithRew] = []
        self.max_size = max_size
        self.preferences: np.ndarray = np.array([])
        self._mirror = None

    def push(self, fragments, preferences: np.ndarray) -> None:
        fragments1, fragments2 = zip(*fragments)
        if preferences.shape != (len(fragments),):
            raise ValueError(f"Unexpected preferences shape {preferences.shape}, expected {(len(fragments),)}")
        if preferences.dtype != np.float32:
            raise ValueError("preferences should have dtype float32")
        self.fragments1.extend(fragments1)
        self.fragments2.extend(fragments2)
        self.preferences = np.concatenate((self.preferences, preferences))
        if self.max_size is not None:
            extra = len(self.preferences) - self.max_size
            if extra > 0:
                self.fragments1 = self.fragments1[extra:]
                self.fragments2 = self.fragments2[extra:]
                self.preferences = self.preferences[extra:]
        self._mirror = None

    def __getitem__(self, key):
        return (self.fragments1[key], self.fragments2[key]), self.preferences[key]

    def __len__(self) -> int:
        assert len(self.fragments1) == len(self.fragments2) == len(self.preferences)
        return len(self.fragments1)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_mirror"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault("_mirror", None)

    def save(self, path) -> None:
        with open(path, "wb") as file:
            pickle.dump(self, file)

    @staticmethod
    def load(path) -> "PreferenceDataset":
        with open(path, "rb") as file:
            return pickle.load(file)

    def device_table(self, device, discrete: bool, frames: bool = True) -> Union["_FragmentTable", "_FrameTable"]:
        """The device mirror: a `_FrameTable` when the fragments hold uint8 images (and the caller can read one:
        `frames`), else the flat fp32 `_FragmentTable`."""
        cls = _FrameTable if frames and _holds_image_fragments(self) else _FragmentTable
        m = self._mirror
        if m is None or type(m) is not cls or m.device != th.device(device) or m.discrete != discrete:
            m = self._mirror = cls(self, th.device(device), discrete)
        return m


def _holds_image_fragments(ds: PreferenceDataset) -> bool:
    """Observations of the image space of `modules._is_image_space`: uint8 arrays with three trailing dimensions."""
    if not len(ds):
        return False
    obs = ds.fragments1[0].obs
    return isinstance(obs, np.ndarray) and obs.dtype == np.uint8 and obs.ndim == 4


def frame_table_index(pair_len: np.ndarray, pairs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Index arithmetic of `_FrameTable` (NumPy only). The table holds, pair by pair, fragment 1's `L + 1` frames and then
    fragment 2's, `L = pair_len[pair]`. Returns, for the pairs `pairs` in batch order (per pair: fragment 1's steps, then
    fragment 2's), the state-frame index of every row -- step t of a fragment whose first frame is f0 reads frame f0 + t,
    its next state is frame f0 + t + 1 -- and the pair offsets [P + 1] in steps."""
    pair_len = np.asarray(pair_len, np.int64)
    frag_start = np.zeros(2 * len(pair_len) + 1, dtype=np.int64)
    np.cumsum(np.repeat(pair_len + 1, 2), out=frag_start[1:])
    lens = pair_len[pairs]
    off = np.zeros(len(pairs) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    idx = [np.arange(frag_start[2 * p + k], frag_start[2 * p + k] + l) for p, l in zip(pairs, lens) for k in (0, 1)]
    return (np.concatenate(idx) if idx else np.zeros(0, np.int64)), off


def frame_table_arrays(ds: PreferenceDataset, discrete: bool) -> Dict[str, np.ndarray]:
    """The host arrays of `_FrameTable` (NumPy only), every one indexed by frame: `frames` uint8 `[F, *obs shape]` in the
    observation space's layout, and per state frame the action, the done flag and the ground-truth reward of the step that
    starts there (the entry at a fragment's last frame, where no step starts, is zero and never read)."""
    lens = np.array([len(f) for f in ds.fragments1], dtype=np.int64)
    if any(len(f2) != l for f2, l in zip(ds.fragments2, lens)):
        raise ValueError("the two fragments of a pair must have the same length")
    frags = [f for pair in zip(ds.fragments1, ds.fragments2) for f in pair]
    has_gt = bool(len(ds)) and _trajectory_pair_includes_reward(ds[0][0])
    pad = lambda a: np.concatenate([a, np.zeros((1,) + a.shape[1:], a.dtype)])
    if discrete:
        acts = [pad(np.asarray(f.acts, np.int64).reshape(-1)) for f in frags]
    else:
        acts = [pad(np.asarray(f.acts, np.float32).reshape(len(f), -1)) for f in frags]
    dones = []
    for f in frags:
        d = np.zeros(len(f) + 1, np.uint8)
        d[len(f) - 1] = f.terminal       # `flatten_trajectories`: only a terminal fragment's last step is done
        dones.append(d)
    gt = [pad(np.asarray(f.rews, np.float32)) if has_gt else np.zeros(len(f) + 1, np.float32) for f in frags]
    frames = np.ascontiguousarray(np.concatenate([np.asarray(f.obs) for f in frags]))
    return {"frames": frames, "acts": np.concatenate(acts), "dones": np.concatenate(dones), "gt": np.concatenate(gt),
            "pair_len": lens, "has_gt": has_gt}


class _FrameTable:
    """Image fragments on the device: every frame stored ONCE, as uint8, in the observation space's layout (`[F, H, W, C]`,
    or `[F, C, H, W]` for a channel-first space). A fragment of L steps holds L + 1 frames; step t reads frame f0 + t as
    state and frame f0 + t + 1 as next state (`frame_table_index`), so a minibatch is described by one index vector and
    `ops.pref_gather_frames` builds the CNN's input from it. Actions (int64 for a Discrete space), dones and ground-truth
    rewards are indexed by the state frame too. Pairs are laid out as in `_FragmentTable`: fragment 1, then fragment 2.
    Device bytes of the frames: F * H * W * C with F = sum over fragments of (L + 1); `_FragmentTable` holds
    2 * R * H * W * C * 4 for the same R = sum of L transitions (state and next state, fp32): 8 L / (L + 1) times as
    many, 7.3 x at L = 10."""

    def __init__(self, ds: PreferenceDataset, device: th.device, discrete: bool):
        self.device, self.discrete = device, discrete
        a = frame_table_arrays(ds, discrete)
        self.pair_len = a["pair_len"]
        self.frames = th.as_tensor(a["frames"]).to(device).contiguous()
        self.acts = th.as_tensor(a["acts"]).to(device).contiguous()
        self.dones = th.as_tensor(a["dones"]).to(device).contiguous()
        self.gt = th.as_tensor(a["gt"]).to(device)
        self.prefs = np.asarray(ds.preferences, np.float32)
        self.has_gt = a["has_gt"]

    def batch(self, pairs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(state-frame index of every row in batch order, pair offsets [P+1] in steps) of the pairs `pairs`; a row's
        next-state frame is its state frame + 1."""
        return frame_table_index(self.pair_len, pairs)


class _FragmentTable:
    """The dataset's rows on the device, pair by pair: pair i's fragment 1 rows, then its fragment 2 rows."""

    def __init__(self, ds: PreferenceDataset, device: th.device, discrete: bool):
        self.device, self.discrete = device, discrete
        n = len(ds)
        lens = np.array([len(f) for f in ds.fragments1], dtype=np.int64)
        if any(len(f2) != l for f2, l in zip(ds.fragments2, lens)):
            raise ValueError("the two fragments of a pair must have the same length")
        frags = [f for pair in zip(ds.fragments1, ds.fragments2) for f in pair]
        tr = flatten_trajectories(frags)
        self.pair_len = lens
        self.pair_start = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(2 * lens, out=self.pair_start[1:])
        obs = th.as_tensor(np.asarray(tr.obs, np.float32).reshape(len(tr.obs), -1)).to(device)
        nxt = th.as_tensor(np.asarray(tr.next_obs, np.float32).reshape(len(tr.obs), -1)).to(device)
        if discrete:
            acts = th.as_tensor(np.asarray(tr.acts, np.int64).reshape(-1)).to(device)
        else:
            acts = th.as_tensor(np.asarray(tr.acts, np.float32).reshape(len(tr.obs), -1)).to(device)
        dones = th.as_tensor(np.asarray(tr.dones, np.uint8)).to(device)
        self.table = TransitionTable(obs.contiguous(), acts.contiguous(), nxt.contiguous(), dones.contiguous(), discrete)
        self.gt = th.as_tensor(np.asarray(tr.rews, np.float32)).to(device)
        self.prefs = np.asarray(ds.preferences, np.float32)
        self.has_gt = bool(n) and _trajectory_pair_includes_reward(ds[0][0])

    def batch(self, pairs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(row indices in batch order, pair offsets [P+1] in steps) of the pairs `pairs`."""
        lens = self.pair_len[pairs]
        off = np.zeros(len(pairs) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        rows = np.concatenate([np.arange(self.pair_start[p], self.pair_start[p] + 2 * l) for p, l in zip(pairs, lens)])
        return rows, off


# ---------------------------------------------------------------------------------------------- losses

class LossAndMetrics(NamedTuple):
    """`preference_comparisons.py:1000-1004`."""
    loss: th.Tensor
    metrics: Mapping[str, th.Tensor]


class RewardLoss(abc.ABC):
    """`preference_comparisons.py:1006-1028`."""

    @abc.abstractmethod
    def forward(self, fragment_pairs, preferences: np.ndarray, preference_model: PreferenceModel) -> LossAndMetrics:
        """Loss and metrics of a batch."""

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


class CrossEntropyRewardLoss(RewardLoss):
    """`preference_comparisons.py:1037-1091`: cross entropy of the model's preference probabilities; metrics
    `accuracy` and (with ground-truth rewards) `gt_reward_loss`."""

    def forward(self, fragment_pairs, preferences, preference_model: PreferenceModel) -> LossAndMetrics:
        ds = PreferenceDataset()
        ds.push(fragment_pairs, np.asarray(preferences, dtype=np.float32))
        loss, stats = _PairBatchRunner(preference_model).loss(ds, np.arange(len(ds)))
        metrics = {"accuracy": stats[1].detach().cpu()}
        if _trajectory_pair_includes_reward(fragment_pairs[0]):
            metrics["gt_reward_loss"] = stats[2].detach().cpu()
        return LossAndMetrics(loss=loss, metrics=metrics)


# ---------------------------------------------------------------------------------------------- reward trainers

def loader_epoch_permutations(n: int, epochs: int) -> List[np.ndarray]:
    """The sample orders of `epochs` passes over `DataLoader(range(n), shuffle=True)` (single process), drawn from
    torch's global CPU generator as the loader draws them: per epoch the iterator's base seed, then the sampler's seed
    and `randperm(n)` (the helpers behind `data_types.ExpertIndexStream`)."""
    out = []
    for _ in range(epochs):
        ExpertIndexStream._draw_int64()                       # iter(loader): base seed
        seed = ExpertIndexStream._draw_int64()                # first next(): the sampler's generator seed
        g = th.Generator()
        g.manual_seed(seed)
        out.append(th.randperm(n, generator=g).numpy())
    return out


def loader_epoch_permutations_split(n_train: int, n_val: int, epochs: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """`loader_epoch_permutations` for a training and a validation `DataLoader(shuffle=True)` iterated one after the other
    in every epoch, as `BasicRewardTrainer._train` does with a validation split: per epoch the train loader's base seed,
    its sampler's seed and `randperm(n_train)`, then the same three draws of the validation loader."""
    out = []
    for _ in range(epochs):
        (train,) = loader_epoch_permutations(n_train, 1)
        (val,) = loader_epoch_permutations(n_val, 1)
        out.append((train, val))
    return out


def random_split_indices(n: int, val_length: int, generator: th.Generator) -> Tuple[np.ndarray, np.ndarray]:
    """The subset indices of `torch.utils.data.random_split(range(n), [n - val_length, val_length], generator)`: one
    `randperm(n)`, its first `n - val_length` entries train, the rest validate."""
    perm = th.randperm(n, generator=generator).numpy()
    return perm[:n - val_length], perm[n - val_length:]


class RewardTrainer(abc.ABC):
    """`preference_comparisons.py:1094-1136`."""

    def __init__(self, preference_model: PreferenceModel, custom_logger: Optional[HierarchicalLogger] = None) -> None:
        self._preference_model = preference_model
        self._logger = custom_logger or configure_logger()

    @property
    def logger(self) -> HierarchicalLogger:
        return self._logger

    @logger.setter
    def logger(self, custom_logger: HierarchicalLogger) -> None:
        self._logger = custom_logger

    def train(self, dataset: PreferenceDataset, epoch_multiplier: float = 1.0) -> None:
        with training(self._preference_model.model):
            self._train(dataset, epoch_multiplier)

    @abc.abstractmethod
    def _train(self, dataset: PreferenceDataset, epoch_multiplier: float) -> None:
        """Trains the reward model."""


class BasicRewardTrainer(RewardTrainer):
    """`preference_comparisons.py:1139-1324` on the device. The whole `train` call is enqueued at once: the pair order
    of every epoch is drawn first, each minibatch's statistics row (loss, accuracy, gt_reward_loss) stays on the device,
    and the rows are read back once and replayed into the logger in the reference's order.

    `regularizer_factory`: a `regularization.RegularizerFactory` (what `LpRegularizer.create(...)` /
    `WeightDecayRegularizer.create(...)` return) of one of these two classes. Anything else -- a bare function, a factory
    of a user subclass -- raises `NotImplementedError`: the penalty runs as a HIP kernel between the backward pass and the
    optimiser step, and the product path has no autograd under which a Python penalty could run. A deliberate cut."""

    def __init__(self, preference_model: PreferenceModel, loss: RewardLoss, rng: np.random.Generator,
                 batch_size: int = 32, minibatch_size: Optional[int] = None, epochs: int = 1, lr: float = 1e-3,
                 custom_logger: Optional[HierarchicalLogger] = None, regularizer_factory=None) -> None:
        super().__init__(preference_model, custom_logger)
        if regularizer_factory is not None and not (isinstance(regularizer_factory, regularization.RegularizerFactory)
                                                    and regularizer_factory.cls in regularization.SHIPPED):
            raise NotImplementedError("reward regularizers other than a RegularizerFactory of LpRegularizer or "
                                      "WeightDecayRegularizer (their `create(...)`) are not implemented")
        if not isinstance(loss, CrossEntropyRewardLoss):
            raise NotImplementedError("only CrossEntropyRewardLoss is implemented on the device")
        self.loss = loss
        self.batch_size = batch_size
        self.minibatch_size = minibatch_size or batch_size
        if self.batch_size % self.minibatch_size != 0:
            raise ValueError("Batch size must be a multiple of minibatch size.")
        self.epochs = epochs
        self.rng = rng
        self.lr = lr
        if getattr(preference_model, "ensemble_model", None) is not None:   # (EnsembleTrainer: the members' trainers train)
            self._runner = self.optim = None
        else:
            self._runner = _PairBatchRunner(preference_model)
            self.optim = self._runner.make_optimizer(lr)
        # (an EnsembleTrainer's own regularizer has no optimiser: it exists for its construction-time log record)
        self.regularizer = (regularizer_factory(optimizer=self.optim, logger=self.logger)
                            if regularizer_factory is not None else None)
        self.host_stepped = False   # tests: one host round trip per minibatch (the same launches)
        self.last_split: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self.last_lambda_history: Optional[np.ndarray] = None

    @property
    def requires_regularizer_update(self) -> bool:
        return self.regularizer is not None and self.regularizer.val_split is not None

    def _schedule(self, n: int, epochs: int):
        """[(epoch, pairs of the minibatch, loss scale, accumulate, step after it)] of `epochs` passes."""
        out = []
        for epoch, perm in enumerate(loader_epoch_permutations(n, epochs)):
            self._schedule_epoch(out, epoch, perm)
        return out

    def _schedule_split(self, train_idx: np.ndarray, val_idx: np.ndarray, epochs: int):
        """The schedule with a validation split: per epoch the training minibatches over `train_idx` (entries as in
        `_schedule`), then the validation minibatches over `val_idx` as `(epoch, pairs, None, None, None)` (forward and
        loss only), then the lambda update `(epoch, None, None, None, None)`."""
        out = []
        for epoch, (perm, vperm) in enumerate(loader_epoch_permutations_split(len(train_idx), len(val_idx), epochs)):
            self._schedule_epoch(out, epoch, train_idx[perm])
            for s in range(0, len(val_idx), self.minibatch_size):
                out.append((epoch, val_idx[vperm[s:s + self.minibatch_size]], None, None, None))
            out.append((epoch, None, None, None, None))
        return out

    def _schedule_epoch(self, out, epoch: int, perm: np.ndarray) -> None:
        n, acc = len(perm), 0
        for s in range(0, n, self.minibatch_size):
            mb = perm[s:s + self.minibatch_size]
            first = acc == 0
            acc += len(mb)
            step = acc >= self.batch_size or s + self.minibatch_size >= n
            out.append((epoch, mb, len(mb) / self.batch_size, not first, step))
            if acc >= self.batch_size:
                acc = 0

    def _train(self, dataset: PreferenceDataset, epoch_multiplier: float = 1.0) -> None:
        reg = self.regularizer
        split = None
        if reg is not None and reg.val_split is not None:
            val_length = int(len(dataset) * reg.val_split)
            train_length = len(dataset) - val_length
            if val_length < 1 or train_length < 1:
                raise ValueError("Not enough data samples to split into training and validation, "
                                 "or the validation split is too large/small. "
                                 "Make sure you've generated enough initial preference data. "
                                 "You can adjust this through initial_comparison_frac in "
                                 "PreferenceComparisons.")
            split = random_split_indices(len(dataset), val_length, th.Generator().manual_seed(make_seeds(self.rng)))
        self.last_split = split
        epochs = round(self.epochs * epoch_multiplier)
        assert epochs > 0, "Must train for at least one epoch."
        sched = self._schedule(len(dataset), epochs) if split is None else self._schedule_split(*split, epochs)
        if reg is None:
            stats = self._runner.run(dataset, sched, self.optim, host_stepped=self.host_stepped)
        else:
            stats = self._runner.run(dataset, sched, self.optim, host_stepped=self.host_stepped, reg=reg)
            self.last_lambda_history = self._runner.last_hist
        gt = self._runner.has_gt
        epoch_num = epochs - 1
        lp = isinstance(reg, regularization.LossRegularizer)
        rows = iter(stats)
        with self.logger.accumulate_means("reward"):
            for epoch, mb, scale, _, _ in sched:
                with self.logger.add_key_prefix(f"epoch-{epoch}"):
                    if mb is None:   # the epoch's lambda update
                        self.logger.record("regularization_lambda", float(self._runner.last_hist[epoch][0]))
                        continue
                    row = next(rows)
                    with self.logger.add_key_prefix("train" if scale is not None else "val"):
                        self.logger.record("loss", float(row[0]))
                        self.logger.record("accuracy", float(row[1]))
                        if gt:
                            self.logger.record("gt_reward_loss", float(row[2]))
                    if lp and scale is not None:
                        self.logger.record("regularized_loss", float(row[3]))
        keys = list(self.logger.name_to_value.keys())
        outer_prefix = self.logger.get_accumulate_prefixes()
        for key in keys:
            base_path = f"{outer_prefix}reward/"
            epoch_path = f"mean/{base_path}epoch-{epoch_num}/"
            final_path = f"{base_path}final/"
            regex_match = re.match(rf"{epoch_path}(.+)", key)
            if regex_match:
                (key_name,) = regex_match.groups()
                self.logger.record(f"{final_path}{key_name}", self.logger.name_to_value[key])


def _as_basic(model):
    """The product `BasicRewardNet` whose forward `model`'s forward is (through `PredictProcessedWrapper`s), or None."""
    m = model
    while isinstance(m, reward_nets.PredictProcessedWrapper):
        m = m.base
    return m if type(m) is reward_nets.BasicRewardNet else None


def _as_cnn(model):
    """The `modules.CnnRewardNet` whose forward `model`'s forward is (through `PredictProcessedWrapper`s), or None."""
    m = model
    while isinstance(m, modules.PredictProcessedWrapper):
        m = m.base
    return m if type(m) is modules.CnnRewardNet else None


class _PairBatchRunner:
    """Forward, loss, backward and optimiser steps of minibatches of fragment pairs; the path is chosen from the net's
    type: "basic" (product `BasicRewardNet`), "shaped" (product `ShapedRewardNet`) or "module" (`nn.Module`)."""

    def __init__(self, pm: PreferenceModel):
        self.pm = pm
        model = pm.model
        self.basic = _as_basic(model) if isinstance(model, reward_nets.RewardNet) else None
        if isinstance(model, modules.RewardNet):
            self.kind = "module"
        elif self.basic is not None:
            self.kind = "basic"
        elif isinstance(model, reward_nets.ShapedRewardNet):
            self.kind = "shaped"
        else:
            raise NotImplementedError(f"reward net {type(model).__name__} cannot be trained on preferences here")
        self.has_gt = False

    @property
    def device(self) -> th.device:
        return _device_of(self.pm.model)

    def make_optimizer(self, lr: float):
        model = self.pm.model
        if self.kind == "module":
            return ops.HipAdamW(model.parameters(), lr=lr)
        store = model._store   # (wrappers share their base's store)
        return HipAdam(store.flat, store.grad, lr=lr, weight_decay=0.01, decoupled=True)

    def _discrete(self) -> bool:
        from imitation_amd import spaces
        return isinstance(self.pm.model.action_space, spaces.Discrete)

    # -- one minibatch's loss on the device: (loss tensor for autograd or None, stats[3] device view)
    def loss(self, ds: PreferenceDataset, pairs: np.ndarray):
        tab = ds.device_table(self.device, self._discrete(), frames=self.kind == "module")
        rows, off = tab.batch(pairs)
        rows_d = th.as_tensor(rows).to(self.device)
        off_d = th.as_tensor(off.astype(np.int32)).to(self.device)
        y = th.as_tensor(tab.prefs[pairs]).to(self.device)
        st = th.empty(3, device=self.device)
        if self.kind == "module":
            rew = self._module_rewards(tab, rows_d, off)
            loss, stats, _ = ops.preference_loss(rew, off_d, y, tab.gt[rows_d] if tab.has_gt else None,
                                                 self.pm.discount_factor, self.pm.noise_prob, self.pm.threshold)
            return loss, stats
        rew = self._product_forward(tab, rows_d, off)
        self._launch_loss(rew, off_d, y, tab.gt[rows_d] if tab.has_gt else None, 1.0, None, st)
        return st[0], st

    def _launch_loss(self, rew, off_d, y, gt, scale, d, stats):
        pm = self.pm
        L.call("ia_pref_loss", L.ptr(rew), L.ptr(off_d), off_d.numel() - 1, L.ptr(y), L.ptr(gt),
               float(pm.discount_factor), float(pm.noise_prob), float(pm.threshold), float(scale), L.ptr(d), None,
               None, L.ptr(stats), L.stream())

    def _module_rewards(self, tab: _FragmentTable, rows_d: th.Tensor, off: np.ndarray) -> th.Tensor:
        """The module net's rewards of the rows, one call per fragment like `PreferenceModel.rewards` when the net holds a
        normalisation layer (its statistics move per call), else one call for all rows."""
        model = self.pm.model
        if isinstance(tab, _FrameTable):
            return self._frame_rewards(tab, rows_d, off)
        t = tab.table
        acts = t.acts[rows_d]
        s, a, ns, d = model.preprocess(t.obs[rows_d], acts, t.next_obs[rows_d], t.dones[rows_d].bool())
        if not any(isinstance(m, modules.RunningNorm) for m in model.modules()):
            return model(s, a, ns, d).reshape(-1)
        out, r = [], 0
        for p in range(len(off) - 1):
            Lp = int(off[p + 1] - off[p])
            for _ in range(2):
                out.append(model(s[r:r + Lp], a[r:r + Lp], ns[r:r + Lp], d[r:r + Lp]).reshape(-1))
                r += Lp
        return th.cat(out)

    def _frame_rewards(self, tab: "_FrameTable", idx_d: th.Tensor, off: np.ndarray) -> th.Tensor:
        """Rewards of image rows from the frame table (`idx_d`: their state frames). A `modules.CnnRewardNet` (innermost,
        under `PredictProcessedWrapper`s) takes its channel-last input from one `ops.pref_gather_frames` launch; any other
        net goes through its own `forward` on state / next-state tensors in the space's layout (two launches; each
        fragment in a call of its own when the net holds a normalisation layer, as for flat rows)."""
        model = self.pm.model
        if not model.normalize_images:
            raise NotImplementedError("the frame table scales images by 1 / 255: normalize_images=False is not implemented")
        a = reward_nets.preprocess_space(tab.acts[idx_d], model.action_space, model.normalize_images)
        d = tab.dones[idx_d].to(th.float32)
        cnn = _as_cnn(model)
        if cnn is not None:
            x = ops.pref_gather_frames(tab.frames, idx_d, cnn.use_state, cnn.use_next_state, not cnn.hwc_format)
            return cnn.forward_nhwc(x, a, d).reshape(-1)
        # read as [F, H, W, C] with one source frame, the op's output has the table's own layout: the space's
        s = ops.pref_gather_frames(tab.frames, idx_d, True, False, False)
        ns = ops.pref_gather_frames(tab.frames, idx_d + 1, True, False, False)
        if not any(isinstance(m, modules.RunningNorm) for m in model.modules()):
            return model(s, a, ns, d).reshape(-1)
        out, r = [], 0
        for p in range(len(off) - 1):
            Lp = int(off[p + 1] - off[p])
            for _ in range(2):
                out.append(model(s[r:r + Lp], a[r:r + Lp], ns[r:r + Lp], d[r:r + Lp]).reshape(-1))
                r += Lp
        return th.cat(out)

    def _product_forward(self, tab: _FragmentTable, rows_d: th.Tensor, off: np.ndarray) -> th.Tensor:
        R = int(rows_d.numel())
        model = self.pm.model
        if self.kind == "shaped":
            for st in (model._base.mlp, model.potential._potential_net):
                if st.norm is not None and st.training:
                    raise NotImplementedError("a shaped reward net with an input RunningNorm is not implemented here")
            self._shaped_R = R
            return model._shaped([(tab.table, rows_d, R)], "pref", True, None)
        net = self.basic
        mlp = net.mlp
        ws = mlp.train_workspace(R, "pref")
        gather_concat(tab.table, rows_d, R, net.obs_dim, net.act_dim, net.flags, ws["X"], mlp.ldx, 0)
        x = ws["X"]
        nrm = mlp.norm
        if nrm is not None:
            D = mlp.dims[0]
            if mlp.training:
                lens = np.diff(off)
                if not nrm.is_chan:
                    raise NotImplementedError("EMANorm input layers are not implemented for preference training")
                if len(lens) and (lens != lens[0]).any():
                    raise NotImplementedError("an input RunningNorm with fragments of different lengths")
                Lf, nf = int(lens[0]), 2 * len(lens)
                need = int(L.load().ia_running_norm_ws_floats(Lf, D))
                key = ("pref_rn", nf, Lf)
                rw = mlp._ws.get(key)
                if rw is None:
                    rw = mlp._ws[key] = {"m": th.empty(nf, need, device=x.device),
                                         "snap": th.empty(nf, 2, D, device=x.device)}
                L.call("ia_pref_frag_moments", L.ptr(x), mlp.ldx, nf, Lf, D, need, L.ptr(rw["m"]), L.stream())
                L.call("ia_running_norm_merge_seq", L.ptr(rw["m"]), nf, need, 1, Lf, D, D, L.ptr(nrm.running_mean),
                       L.ptr(nrm.running_var), L.ptr(nrm.count), L.ptr(rw["snap"]), L.stream())
                L.call("ia_pref_norm_apply_seq", L.ptr(x), mlp.ldx, nf, Lf, D, L.ptr(rw["snap"]), nrm.eps,
                       L.ptr(ws["Xn"]), mlp.ldx, L.stream())
            else:
                nrm.apply(x, ws["Xn"], mlp.ldx, mlp.ldx, R)
            x = ws["Xn"]
        ws["_in"] = x
        L.call("ia_mlp_forward", C.byref(mlp.desc), L.ptr(mlp.flat), L.ptr(x), mlp.ldx, R, L.ptr(ws["hidden"]),
               L.ptr(ws["out"]), L.ACT_NONE, L.stream())
        self._ws, self._R = ws, R
        return ws["out"].reshape(R)

    def _product_backward(self, d: th.Tensor, accumulate: bool, adam) -> None:
        """Gradient of the last forward (accumulated or not); with `adam` the step is fused into the reduction."""
        if self.kind == "shaped":
            self.pm.model.disc_backward(d, accumulate)
            if adam is not None:
                adam.step()
            return
        mlp = self.basic.mlp
        fuse = adam is not None and not accumulate and adam.flat.numel() == mlp.n_params
        mlp.backward_rows(self._ws, self._R, d, accumulate, adam=adam if fuse else None)
        if adam is not None and not fuse:
            adam.step()

    # -- a whole train call
    def _segments(self, optim, reg) -> th.Tensor:
        """The regularizer's segment table: the flat parameter / gradient buffers of a product net's store, or every
        `nn.Parameter` of the optimiser (Lp: a parameter without a gradient gets a zero one first, the penalty gives it one
        in the reference; the gradient tensors then stay in place for the whole call, see `run`)."""
        if self.kind != "module":
            return regularization.segment_table([(optim.flat, optim.grad)])
        params = [q for group in optim.param_groups for q in group["params"]]
        if reg.needs_grads:
            for q in params:
                if q.grad is None:
                    q.grad = th.zeros_like(q, memory_format=th.contiguous_format)
        return regularization.segment_table([(q.data, q.grad if reg.needs_grads else None) for q in params])

    def run(self, ds: Union[PreferenceDataset, "PreferenceBag"], sched, optim, host_stepped: bool = False,
            reg: Optional[regularization.Regularizer] = None) -> np.ndarray:
        """Enqueues the schedule `sched` (`BasicRewardTrainer._schedule` / `_schedule_split`) and returns the statistics
        rows of its minibatches, in order: (loss, accuracy, gt_reward_loss) and, with a regularizer `reg`, regularized_loss.
        With a lambda schedule `last_hist` holds one row (lambda after, train_loss, val_loss, error code) per epoch."""
        dev = self.device
        if isinstance(ds, PreferenceBag):   # the schedule indexes the bag; the table is the dataset's
            sched = [(e, ds.pair_ids[mb] if mb is not None else None, sc, acc, st) for e, mb, sc, acc, st in sched]
            ds = ds.dataset
        tab = ds.device_table(dev, self._discrete(), frames=self.kind == "module")
        self.has_gt = tab.has_gt
        batches = [it for it in sched if it[1] is not None]
        n_mb = len(batches)
        n_upd = len(sched) - n_mb
        # every minibatch's rows, pair offsets and preferences in one upload
        parts = [tab.batch(mb) for _, mb, _, _, _ in batches]
        row_at = np.zeros(n_mb + 1, dtype=np.int64)
        np.cumsum([len(r) for r, _ in parts], out=row_at[1:])
        off_at = np.zeros(n_mb + 1, dtype=np.int64)
        np.cumsum([len(o) for _, o in parts], out=off_at[1:])
        rows_all = th.as_tensor(np.concatenate([r for r, _ in parts])).to(dev)
        off_all = th.as_tensor(np.concatenate([o for _, o in parts]).astype(np.int32)).to(dev)
        pair_at = np.zeros(n_mb + 1, dtype=np.int64)
        np.cumsum([len(mb) for _, mb, _, _, _ in batches], out=pair_at[1:])
        y_all = th.as_tensor(np.concatenate([tab.prefs[mb] for _, mb, _, _, _ in batches])).to(dev)
        gt_all = tab.gt[rows_all] if tab.has_gt else None
        d_all = th.empty(int(row_at[-1]), device=dev)
        self.last_hist = None
        if reg is None:
            stats = th.zeros(n_mb, 3, device=dev)
        else:
            # one buffer, one read-back: the lambda history (doubles, first) and the four-column statistics
            buf = th.zeros(32 * n_upd + 16 * n_mb, dtype=th.uint8, device=dev)
            hist = buf[:32 * n_upd].view(th.float64).view(n_upd, 4)
            stats = buf[32 * n_upd:].view(th.float32).view(n_mb, 4)
            hist_host = np.zeros((n_upd, 4))
            if n_upd and reg.device_schedule and not isinstance(reg.lambda_, float):
                raise ValueError("lambda_ must be a float")   # (`IntervalParamScaler.__call__`; a double on the device)
            lam = reg.device_lambda(dev)
            segs = self._segments(optim, reg)
            scales = th.as_tensor(np.array([1.0 if sc is None else sc for _, _, sc, _, _ in batches],
                                           np.float32)).to(dev)
        k = ep0 = val0 = 0   # the minibatch; the first training and the first validation minibatch of the epoch
        for epoch, mb, scale, accumulate, step in sched:
            if mb is None:   # the epoch's lambda update on rows [ep0, val0) and [val0, k)
                if reg.device_schedule:
                    regularization.lambda_update(lam, reg.lambda_updater, stats[ep0:val0], scales[ep0:val0],
                                                 stats[val0:k], hist[epoch], hist[epoch - 1] if epoch else None)
                else:
                    # any other updater is a host function: one synchronisation per epoch
                    loss = stats[ep0:k, 0].cpu().numpy()
                    sc = np.array([b[2] for b in batches[ep0:val0]], np.float32)
                    train_loss = val_loss = 0.0
                    for j in range(val0 - ep0):
                        train_loss += float(loss[j] * sc[j])
                    for j in range(val0 - ep0, k - ep0):
                        val_loss += float(loss[j])
                    reg.lambda_ = reg.lambda_updater(reg.lambda_, train_loss, val_loss)
                    hist_host[epoch] = (reg.lambda_, train_loss, val_loss, 0.0)
                ep0 = val0 = k
                continue
            r0, r1 = int(row_at[k]), int(row_at[k + 1])
            rows_d = rows_all[r0:r1]
            off_d = off_all[int(off_at[k]):int(off_at[k + 1])]
            y = y_all[int(pair_at[k]):int(pair_at[k + 1])]
            gt = gt_all[r0:r1] if gt_all is not None else None
            off = parts[k][1]
            if scale is None:   # validation: forward and loss only (in training mode, as in the reference)
                if self.kind == "module":
                    with th.no_grad():
                        rew = self._module_rewards(tab, rows_d, off)
                        _, st, _ = ops.preference_loss(rew, off_d, y, gt, self.pm.discount_factor, self.pm.noise_prob,
                                                       self.pm.threshold)
                    stats[k, :3].copy_(st)
                else:
                    rew = self._product_forward(tab, rows_d, off)
                    self._launch_loss(rew, off_d, y, gt, 1.0, None, stats[k])
                k += 1
            elif self.kind == "module":
                if not accumulate:
                    # (a loss regularizer's segment table points at the gradient tensors: they are zeroed in place)
                    optim.zero_grad(set_to_none=False) if reg is not None and reg.needs_grads else optim.zero_grad()
                rew = self._module_rewards(tab, rows_d, off)
                loss, st, _ = ops.preference_loss(rew, off_d, y, gt, self.pm.discount_factor, self.pm.noise_prob,
                                                  self.pm.threshold)
                stats[k, :3].copy_(st)
                (loss * scale).backward()
                if reg is not None:
                    reg.launch(segs, stats[k], scale)
                if step:
                    optim.step()
                k += 1
                val0 = k
            else:
                rew = self._product_forward(tab, rows_d, off)
                d = d_all[r0:r1]
                self._launch_loss(rew, off_d, y, gt, scale, d, stats[k])
                if reg is None:
                    self._product_backward(d, accumulate, optim if step else None)
                else:
                    # the penalty (or the decay) sits between the backward pass and the optimiser step: the step
                    # cannot be fused into the gradient reduction
                    self._product_backward(d, accumulate, None)
                    reg.launch(segs, stats[k], scale)
                    if step:
                        optim.step()
                k += 1
                val0 = k
            if host_stepped:
                th.cuda.current_stream().synchronize()
        if reg is None:
            return stats.cpu().numpy()
        host = buf.cpu().numpy()
        out = host[32 * n_upd:].view(np.float32).reshape(n_mb, 4).copy()
        if n_upd:
            if reg.device_schedule:
                self.last_hist = host[:32 * n_upd].view(np.float64).reshape(n_upd, 4).copy()
                reg.refresh_lambda(self.last_hist[-1][0])
                bad = self.last_hist[:, 3] != 0
                if bad.any():
                    raise ValueError(regularization.ERROR_MESSAGES[int(self.last_hist[bad][0][3])])
            else:
                self.last_hist = hist_host
        return out


class PreferenceBag:
    """A bag of an `EnsembleTrainer`: pairs `pair_ids` (with repeats) of `dataset`, the equivalent of the reference's
    `torch.utils.data.Subset`. A view: the dataset's device fragment table serves every bag."""

    def __init__(self, dataset: PreferenceDataset, pair_ids: np.ndarray):
        self.dataset = dataset
        self.pair_ids = np.asarray(pair_ids, dtype=np.int64)

    def __len__(self) -> int:
        return len(self.pair_ids)

    def __getitem__(self, key):
        return self.dataset[int(self.pair_ids[key])]


def bag_indices(n: int, generator: th.Generator) -> List[int]:
    """`list(RandomSampler(range(n), replacement=True, num_samples=n, generator=generator))`, restated: `n // 32` draws of
    32 indices, then one of `n % 32` (drawn even when empty)."""
    out: List[int] = []
    for _ in range(n // 32):
        out.extend(th.randint(high=n, size=(32,), dtype=th.int64, generator=generator).tolist())
    out.extend(th.randint(high=n, size=(n % 32,), dtype=th.int64, generator=generator).tolist())
    return out


class EnsembleTrainer(BasicRewardTrainer):
    """`preference_comparisons.py:1326-1438`: one `BasicRewardTrainer` per member, each trained on its own bag (drawn
    with replacement from the dataset) on the one-launch-per-minibatch path, one member after the other.

    `preference_model`, `loss` and `rng` default to None only because `tests/test_preference_comparisons.py` (frozen) calls
    the constructor without arguments and expects `NotImplementedError`; the reference has no such defaults."""

    def __init__(self, preference_model: Optional[PreferenceModel] = None, loss: Optional[RewardLoss] = None,
                 rng: Optional[np.random.Generator] = None, batch_size: int = 32, minibatch_size: Optional[int] = None,
                 epochs: int = 1, lr: float = 1e-3, custom_logger: Optional[HierarchicalLogger] = None,
                 regularizer_factory=None) -> None:
        if preference_model is None or loss is None or rng is None:
            raise NotImplementedError("EnsembleTrainer needs a PreferenceModel over a RewardEnsemble, a loss and an rng")
        if preference_model.ensemble_model is None:
            raise TypeError("PreferenceModel of a RewardEnsemble expected by EnsembleTrainer.")
        self.member_trainers: List[BasicRewardTrainer] = []
        super().__init__(preference_model, loss=loss, rng=rng, batch_size=batch_size, minibatch_size=minibatch_size,
                         epochs=epochs, lr=lr, custom_logger=custom_logger, regularizer_factory=regularizer_factory)
        for member_pref_model in preference_model.member_pref_models:
            self.member_trainers.append(BasicRewardTrainer(
                member_pref_model, loss=loss, rng=self.rng, batch_size=batch_size, minibatch_size=minibatch_size,
                epochs=epochs, lr=lr, custom_logger=self.logger, regularizer_factory=regularizer_factory))
        self.last_bags: List[np.ndarray] = []

    @property
    def logger(self) -> HierarchicalLogger:
        return self._logger

    @logger.setter
    def logger(self, custom_logger: HierarchicalLogger) -> None:
        self._logger = custom_logger
        for member_trainer in self.member_trainers:
            member_trainer.logger = custom_logger

    def _train(self, dataset: PreferenceDataset, epoch_multiplier: float = 1.0) -> None:
        generator = th.Generator().manual_seed(make_seeds(self.rng))
        self.last_bags = []
        for member_idx, trainer in enumerate(self.member_trainers):
            bag = PreferenceBag(dataset, np.asarray(bag_indices(len(dataset), generator), dtype=np.int64))
            self.last_bags.append(bag.pair_ids)
            with self.logger.add_accumulate_prefix(f"member-{member_idx}"):
                trainer.train(bag, epoch_multiplier=epoch_multiplier)
        # average the metrics across the member models
        metrics: Dict[str, List[float]] = {}
        for key in list(self.logger.name_to_value.keys()):
            if re.match(r"member-(\d+)/reward/(.+)", key) and "final" in key:
                metrics.setdefault("/".join(key.split("/")[1:]), []).append(self.logger.name_to_value[key])
        for k, v in metrics.items():
            self.logger.record(k, np.mean(v))
            self.logger.record(k + "_std", np.std(v))


def _make_reward_trainer(preference_model: PreferenceModel, loss: RewardLoss, rng: np.random.Generator,
                         reward_trainer_kwargs: Optional[Mapping[str, Any]] = None) -> RewardTrainer:
    """`preference_comparisons.py:1449-1472`."""
    if preference_model.ensemble_model is not None:
        return EnsembleTrainer(preference_model, loss, rng=rng, **(reward_trainer_kwargs or {}))
    return BasicRewardTrainer(preference_model, loss=loss, rng=rng, **(reward_trainer_kwargs or {}))


# ---------------------------------------------------------------------------------------------- the algorithm

QUERY_SCHEDULES: Dict[str, Callable[[float], float]] = {
    "constant": lambda t: 1.0,
    "hyperbolic": lambda t: 1.0 / (1.0 + t),
    "inverse_quadratic": lambda t: 1.0 / (1.0 + t**2),
}


def oric(x: np.ndarray) -> np.ndarray:
    """`util/util.py:44-68`: optimal rounding under integer constraints (keeps the sum)."""
    rounded = np.floor(x)
    shortfall = x - rounded
    total_shortfall = np.round(shortfall.sum()).astype(int)
    indices = np.argsort(-shortfall)
    rounded[indices[:total_shortfall]] += 1
    return rounded.astype(int)


class PreferenceComparisons:
    """`preference_comparisons.py:1482-1753`: alternately gathers preferences on fragments of the generator's
    trajectories, trains the reward model on them, and trains the agent on the reward model."""

    def __init__(self, trajectory_generator: TrajectoryGenerator, reward_model: AnyRewardNet, num_iterations: int,
                 fragmenter: Optional[Fragmenter] = None, preference_gatherer: Optional[PreferenceGatherer] = None,
                 reward_trainer: Optional[RewardTrainer] = None, comparison_queue_size: Optional[int] = None,
                 fragment_length: int = 100, transition_oversampling: float = 1, initial_comparison_frac: float = 0.1,
                 initial_epoch_multiplier: float = 200.0, custom_logger: Optional[HierarchicalLogger] = None,
                 allow_variable_horizon: bool = False, rng: Optional[np.random.Generator] = None,
                 query_schedule: Union[str, Callable[[float], float]] = "hyperbolic") -> None:
        self._logger = custom_logger or configure_logger()
        self.allow_variable_horizon = allow_variable_horizon
        self._horizon = None
        self._iteration = 0
        self.model = reward_model
        self.rng = rng
        has_any_rng_args_none = None in (preference_gatherer, fragmenter, reward_trainer)
        if self.rng is None and has_any_rng_args_none:
            raise ValueError("If you don't provide a random state, you must provide your own seeded fragmenter, "
                             "preference gatherer, and reward_trainer. You can initialize a random state with "
                             "`np.random.default_rng(seed)`.")
        elif self.rng is not None and not has_any_rng_args_none:
            raise ValueError("If you provide your own fragmenter, preference gatherer, and reward trainer, you don't "
                             "need to provide a random state.")
        if reward_trainer is None:
            assert self.rng is not None
            self.reward_trainer = _make_reward_trainer(PreferenceModel(reward_model), CrossEntropyRewardLoss(),
                                                       rng=self.rng)
        else:
            self.reward_trainer = reward_trainer
        self.reward_trainer.logger = self.logger
        self.trajectory_generator = trajectory_generator
        self.trajectory_generator.logger = self.logger
        if fragmenter:
            self.fragmenter = fragmenter
        else:
            assert self.rng is not None
            self.fragmenter = RandomFragmenter(custom_logger=self.logger, rng=self.rng)
        self.fragmenter.logger = self.logger
        if preference_gatherer:
            self.preference_gatherer = preference_gatherer
        else:
            assert self.rng is not None
            self.preference_gatherer = SyntheticGatherer(custom_logger=self.logger, rng=self.rng)
        self.preference_gatherer.logger = self.logger
        self.fragment_length = fragment_length
        self.initial_comparison_frac = initial_comparison_frac
        self.initial_epoch_multiplier = initial_epoch_multiplier
        self.num_iterations = num_iterations
        self.transition_oversampling = transition_oversampling
        if callable(query_schedule):
            self.query_schedule = query_schedule
        elif query_schedule in QUERY_SCHEDULES:
            self.query_schedule = QUERY_SCHEDULES[query_schedule]
        else:
            raise ValueError(f"Unknown query schedule: {query_schedule}")
        self.dataset = PreferenceDataset(max_size=comparison_queue_size)

    @property
    def logger(self) -> HierarchicalLogger:
        return self._logger

    @logger.setter
    def logger(self, value: HierarchicalLogger) -> None:
        self._logger = value

    def _check_fixed_horizon(self, horizons) -> None:
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

    def query_schedule_for(self, total_comparisons: int) -> List[int]:
        """The number of comparisons gathered at each iteration of `train(..., total_comparisons)`."""
        initial_comparisons = int(total_comparisons * self.initial_comparison_frac)
        total_comparisons -= initial_comparisons
        vec_schedule = np.vectorize(self.query_schedule)
        unnormalized_probs = vec_schedule(np.linspace(0, 1, self.num_iterations))
        probs = unnormalized_probs / np.sum(unnormalized_probs)
        shares = oric(probs * total_comparisons)
        return [initial_comparisons] + shares.tolist()

    def train(self, total_timesteps: int, total_comparisons: int,
              callback: Optional[Callable[[int], None]] = None) -> Mapping[str, Any]:
        schedule = self.query_schedule_for(total_comparisons)
        print(f"Query schedule: {schedule}")
        timesteps_per_iteration, extra_timesteps = divmod(total_timesteps, self.num_iterations)
        reward_loss = None
        reward_accuracy = None
        for i, num_pairs in enumerate(schedule):
            num_steps = math.ceil(self.transition_oversampling * 2 * num_pairs * self.fragment_length)
            self.logger.log(f"Collecting {2 * num_pairs} fragments ({num_steps} transitions)")
            trajectories = self.trajectory_generator.sample(num_steps)
            horizons = (len(traj) for traj in trajectories if traj.terminal)
            self._check_fixed_horizon(horizons)
            self.logger.log("Creating fragment pairs")
            fragments = self.fragmenter(trajectories, self.fragment_length, num_pairs)
            with self.logger.accumulate_means("preferences"):
                self.logger.log("Gathering preferences")
                preferences = self.preference_gatherer(fragments)
            self.dataset.push(fragments, preferences)
            self.logger.log(f"Dataset now contains {len(self.dataset)} comparisons")
            epoch_multiplier = 1.0
            if i == 0:
                epoch_multiplier = self.initial_epoch_multiplier
            self.reward_trainer.train(self.dataset, epoch_multiplier=epoch_multiplier)
            base_key = self.logger.get_accumulate_prefixes() + "reward/final/train"
            assert f"{base_key}/loss" in self.logger.name_to_value
            assert f"{base_key}/accuracy" in self.logger.name_to_value
            reward_loss = self.logger.name_to_value[f"{base_key}/loss"]
            reward_accuracy = self.logger.name_to_value[f"{base_key}/accuracy"]
            num_steps = timesteps_per_iteration
            if i == self.num_iterations - 1:
                num_steps += extra_timesteps
            with self.logger.accumulate_means("agent"):
                self.logger.log(f"Training agent for {num_steps} timesteps")
                self.trajectory_generator.train(steps=num_steps)
            self.logger.dump(self._iteration)
            if callback:
                callback(self._iteration)
            self._iteration += 1
        return {"reward_loss": reward_loss, "reward_accuracy": reward_accuracy}
