"""Soft Q Imitation Learning (`algorithms/sqil.py`, https://arxiv.org/abs/1905.11108): DQN-style Q-learning on a replay
buffer whose minibatches are half learner transitions with reward 0 and half expert demonstrations with reward 1.

`SQIL` and `SQILReplayBuffer` keep the reference's surface; the learner is this package's `DQN` (`imitation_amd/dqn.py`)
or, on Box actions, its `TD3` / `DDPG` (`imitation_amd/td3.py`) or `SAC` (`imitation_amd/sac.py`), whose updates run on the
device from the learner ring and the expert table by index. Demonstrated actions enter the expert table as given: the reference does not scale them to
[-1, 1] either (`sqil.py:196-204`), while the learner ring holds scaled actions.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from imitation_amd import data_types as dt
from imitation_amd import dqn
from imitation_amd import logger as imit_logger
from imitation_amd import sac
from imitation_amd import td3
from imitation_amd.vec_env import VecEnv


def split_in_half(x: int) -> Tuple[int, int]:
    """`util/util.py:452-466`: two integers that differ by at most one and add up to `x`, the smaller first."""
    half = x // 2
    return half, x - half


class SQILReplayBuffer(dqn.ReplayBuffer):
    """`algorithms/sqil.py:104-251`: SB3's replay buffer plus an expert table; a sampled batch is
    `batch_size // 2` learner rows followed by `batch_size - batch_size // 2` expert rows."""

    def __init__(self, buffer_size: int, observation_space, action_space, demonstrations, device="auto", n_envs: int = 1,
                 optimize_memory_usage: bool = False):
        super().__init__(buffer_size=buffer_size, observation_space=observation_space, action_space=action_space,
                         device=device, n_envs=n_envs, optimize_memory_usage=optimize_memory_usage,
                         handle_timeout_termination=False)
        self.expert_index = dqn.ReplayIndex(0, 1)
        self.expert: Optional[dqn._Table] = None
        self.set_demonstrations(demonstrations)

    def set_demonstrations(self, demonstrations) -> None:
        """`sqil.py:156-204`: `Transitions`, or an iterable of trajectories that is flattened first. The reference
        flattens any `types.Trajectory`; this package's only trajectory class is `TrajectoryWithRew`, so that is what is
        recognised here (anything else raises `NotImplementedError`, as there)."""
        if not isinstance(demonstrations, dt.Transitions):
            try:
                seq = list(demonstrations)
                item = seq[0]
            except (TypeError, IndexError):
                raise NotImplementedError(f"Unsupported demonstrations type: {demonstrations}")
            if isinstance(item, dt.TrajectoryWithRew):
                demonstrations = dt.flatten_trajectories(seq)
        if not isinstance(demonstrations, dt.Transitions):
            raise NotImplementedError(f"Unsupported demonstrations type: {demonstrations}")
        n = len(demonstrations)
        if self.frames and not (np.asarray(demonstrations.obs).dtype == np.uint8
                                and np.asarray(demonstrations.next_obs).dtype == np.uint8):
            raise ValueError("demonstrations for an image space must hold uint8 frames (they are stored as they come)")
        # one `add` per demonstration into a ring of n positions with one env each: reward 1, the table is full afterwards
        self.expert_index = dqn.ReplayIndex(n, 1)
        self.expert_index.fill()
        self.expert = dqn._Table(n, self.obs_dim, self.device, self.act_dim, frames=self.frames)
        self.expert.write(0, demonstrations.obs, demonstrations.next_obs, demonstrations.acts, np.ones(n, np.float32),
                          demonstrations.dones)

    def add(self, obs, next_obs, action, reward, done, infos: List[Dict[str, Any]]) -> None:
        super().add(obs=obs, next_obs=next_obs, action=action, reward=np.array(0.0), done=done, infos=infos)

    def sample_rows(self, batch_size: int) -> Tuple[np.ndarray, int]:
        """Learner positions, learner envs, expert positions, expert envs: the four draws of `sqil.py:242-244`."""
        new_sample_size, expert_sample_size = split_in_half(batch_size)
        new_rows = self.index.rows(*self.index.sample(new_sample_size))
        expert_rows = self.expert_index.rows(*self.expert_index.sample(expert_sample_size))
        return np.concatenate([new_rows, expert_rows]), new_sample_size

    def expert_table(self) -> Optional[dqn._Table]:
        return self.expert

    def sample(self, batch_size: int, env=None) -> dqn.ReplayBufferSamples:
        if env is not None:
            raise NotImplementedError("VecNormalize is not implemented")
        import torch as th

        rows, n_new = self.sample_rows(batch_size)
        new, exp = self._gather(self.table, rows[:n_new]), self._gather(self.expert, rows[n_new:])
        return dqn.ReplayBufferSamples(*(th.cat((a, b)) for a, b in zip(new, exp)))


class SQIL:
    """`algorithms/sqil.py:26-101`."""

    def __init__(self, *, venv: VecEnv, demonstrations, policy, custom_logger: Optional[imit_logger.HierarchicalLogger] = None,
                 rl_algo_class=dqn.DQN, rl_kwargs: Optional[Dict[str, Any]] = None):
        self.venv = venv
        if rl_kwargs is None:
            rl_kwargs = {}
        if "replay_buffer_class" in rl_kwargs:
            raise ValueError("SQIL uses a custom replay buffer: 'replay_buffer_class' not allowed.")
        if "replay_buffer_kwargs" in rl_kwargs:
            raise ValueError("SQIL uses a custom replay buffer: 'replay_buffer_kwargs' not allowed.")
        if not (isinstance(rl_algo_class, type) and issubclass(rl_algo_class, (dqn.DQN, td3.TD3, sac.SAC))):
            # (the parenthesis is stale since `sac.SAC` exists; tests/test_td3.py pins the wording: DESIGN section 4.12)
            raise NotImplementedError(f"rl_algo_class {rl_algo_class}: only this package's DQN, TD3 and DDPG are implemented "
                                      "(SAC is out of scope, DESIGN section 1); this package's SAC is implemented too")
        self.rl_algo = rl_algo_class(policy=policy, env=venv, replay_buffer_class=SQILReplayBuffer,
                                     replay_buffer_kwargs={"demonstrations": demonstrations}, **rl_kwargs)
        # `algorithms/base.py:139-166` DemonstrationAlgorithm.__init__
        self._logger = custom_logger or imit_logger.configure()
        self.allow_variable_horizon = False
        if demonstrations is not None:
            self.set_demonstrations(demonstrations)

    @property
    def logger(self) -> imit_logger.HierarchicalLogger:
        return self._logger

    @logger.setter
    def logger(self, value: imit_logger.HierarchicalLogger) -> None:
        self._logger = value

    def set_demonstrations(self, demonstrations) -> None:
        assert isinstance(self.rl_algo.replay_buffer, SQILReplayBuffer)
        self.rl_algo.replay_buffer.set_demonstrations(demonstrations)

    def train(self, *, total_timesteps: int, tb_log_name: str = "SQIL", **kwargs: Any) -> None:
        self.rl_algo.learn(total_timesteps=total_timesteps, tb_log_name=tb_log_name, **kwargs)

    @property
    def policy(self):
        assert isinstance(self.rl_algo.policy, (dqn.DQNPolicy, td3.TD3Policy, sac.SACPolicy))
        return self.rl_algo.policy
