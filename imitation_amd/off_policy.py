"""What the off-policy learners (`dqn.py`, `td3.py`, `sac.py`) share: SB3's `ReplayBuffer` with its rows in device memory
and the off-policy loop -- a restatement of stable-baselines3 2.2.x from its documented behaviour
([SB3 common/off_policy_algorithm.py, common/base_class.py, common/buffers.py]).

Layout, as everywhere in this package: every index decision (ring position, sampled rows) is made on the
host with SB3's own draw sequence from NumPy's GLOBAL stream; the learner ring and the expert table live in device memory
and rows never come back -- a step uploads its transition, a `train` call uploads ONE int64 index array for all its
gradient steps (`OffPolicyAlgorithm._begin_train`) and reads back one block of statistics.
"""
from __future__ import annotations

import collections
import copy
import sys
import time
from typing import Any, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch as th

from imitation_amd import _lib as L
from imitation_amd import logger as imit_logger
from imitation_amd import spaces
from imitation_amd.cnn_policy import _is_image_space
from imitation_amd.networks import require_device
from imitation_amd.ppo import _CallbackList, _NullCallback, _schedule, set_random_seed


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

    def pointers(self) -> tuple:
        """(obs, next_obs, action, reward, done, rows): the five columns as raw pointers and the row count, in the order
        the update kernels take a table."""
        return L.ptr(self.obs), L.ptr(self.next_obs), L.ptr(self.action), L.ptr(self.reward), L.ptr(self.done), self.rows


def table_pointers(table: Optional[_Table]) -> tuple:
    """`table.pointers()`, or five NULLs and 0 rows for an absent table (one no row of the batch comes from)."""
    return (None,) * 5 + (0,) if table is None else table.pointers()


def _device(device) -> th.device:
    return th.device("cuda" if device == "auto" else device)


def adam_kwargs(optimizer_kwargs) -> Tuple[Dict[str, Any], Tuple[float, float], float, float]:
    """(optimizer_kwargs as a dict, betas, eps, weight_decay) of a policy's `optimizer_kwargs` with Adam's defaults."""
    kwargs = dict(optimizer_kwargs or {})
    unknown = set(kwargs) - {"betas", "eps", "weight_decay"}
    if unknown:
        raise NotImplementedError(f"optimizer_kwargs {sorted(unknown)} are not implemented")
    return (kwargs, tuple(kwargs.get("betas", (0.9, 0.999))), float(kwargs.get("eps", 1e-8)),
            float(kwargs.get("weight_decay", 0.0)))


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
        # a `step_source.StepSource`: `add` then ignores its `reward` and stores the step with the source's launches
        self.reward_source: Optional["StepSource"] = None

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


class OffPolicyAlgorithm:
    """What [SB3 common/off_policy_algorithm.py] gives DQN, TD3 and SAC alike: the construction they share, the
    `BaseAlgorithm` surface, `learn`, `collect_rollouts`, `_store_transition` and `_dump_logs`. A subclass supplies
    `policy_aliases`, `_bind_policy`, `_sample_action`, `_on_step`, `train`."""

    policy_aliases: Dict[str, Any] = {}

    def __init__(self, *, policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq,
                 gradient_steps, replay_buffer_class, replay_buffer_kwargs, optimize_memory_usage, stats_window_size,
                 policy_kwargs, verbose, seed, device):
        """The hyper-parameters every learner has (`train_freq` as the subclass has converted it) and the bookkeeping of
        [SB3 BaseAlgorithm.__init__]; a subclass checks its arguments before and calls `_setup_model` after."""
        self.policy_class = self.policy_aliases[policy] if isinstance(policy, str) else policy
        self.policy_kwargs = dict(policy_kwargs or {})
        self.device = _device(device)
        self.learning_rate, self.buffer_size, self.learning_starts = learning_rate, buffer_size, learning_starts
        self.batch_size, self.tau, self.gamma = batch_size, tau, gamma
        self.train_freq, self.gradient_steps = train_freq, gradient_steps
        self.replay_buffer_class = replay_buffer_class
        self.replay_buffer_kwargs = dict(replay_buffer_kwargs or {})
        self.optimize_memory_usage = optimize_memory_usage
        self.seed, self.verbose = seed, verbose
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
        self.policy = None
        self.replay_buffer: Optional[ReplayBuffer] = None
        self.last_action_branch: Optional[str] = None   # which branch the latest `_sample_action` took
        if env is not None:
            self.observation_space, self.action_space, self.n_envs = env.observation_space, env.action_space, env.num_envs

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
        self._bind_policy()

    def _bind_policy(self) -> None:
        """The learner's aliases of the policy's networks and whatever else its `_setup_model` does behind the policy."""
        raise NotImplementedError

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

    def _check_rows(self, rows: np.ndarray, n_new: int) -> None:
        """Where a learner checks a `train` call's sampled rows on the host before anything is uploaded or launched."""

    def _begin_train(self, gradient_steps: int, batch_size: int) -> Tuple[float, np.ndarray, int, th.Tensor]:
        """How every `train` call opens -> (lr, rows, n_new, idx_dev): training mode, the learning rate of the schedule,
        the index draws of all `gradient_steps` minibatches (the same global-stream draws in the same order as SB3's:
        nothing else draws from NumPy in between) and their ONE upload, int64 [gradient_steps, batch_size]."""
        self.policy.set_training_mode(True)
        lr = self.lr_schedule(self._current_progress_remaining)
        self.logger.record("train/learning_rate", lr)
        rows = np.empty((gradient_steps, batch_size), np.int64)
        n_new = batch_size
        for s in range(gradient_steps):
            rows[s], n_new = self.replay_buffer.sample_rows(batch_size)
        self.last_sample_rows, self.last_n_new = rows, n_new
        self._check_rows(rows, n_new)
        return lr, rows, n_new, th.from_numpy(rows).to(self.device)

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
