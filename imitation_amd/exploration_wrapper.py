"""`policies/exploration_wrapper.py`: a policy callable that alternates between a wrapped policy and uniformly random
actions, for the exploratory share of `preference_comparisons.AgentTrainer.sample`.

Everything here is host work (every random draw stays on the host). One policy acts for all
environments of a step; the only device work of an exploratory step is the wrapped learner's own `predict` launch.

The draws from `rng` and from the action space's generator are the reference's, in its order
(`tests/golden/exploration_*.npz`): construction draws one `make_seeds(rng)`, seeds `venv.action_space` with it and
draws one `rng.random()` for the first policy; every call draws one `rng.random()` after the policy has acted and, when
that asks for a switch, one more for the next policy.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from imitation_amd import rollout
from imitation_amd.util import make_seeds
from imitation_amd.vec_env import VecEnv

_STATEFUL = "Exploration wrapper does not support stateful policies."


class ExplorationWrapper:
    """`exploration_wrapper.py:12-95`. After every step the acting policy changes with probability `switch_prob`; the
    new one is the random policy with probability `random_prob`, whichever acted before."""

    def __init__(self, policy, venv: VecEnv, random_prob: float, switch_prob: float, rng: np.random.Generator,
                 deterministic_policy: bool = False):
        self.wrapped_policy = rollout.policy_to_callable(policy, venv, deterministic_policy)
        self.random_prob, self.switch_prob = random_prob, switch_prob
        self.venv = venv
        self.rng = rng
        self.venv.action_space.seed(make_seeds(self.rng))
        self.current_policy = self.wrapped_policy
        self._switch()

    def _random_policy(self, obs, state, episode_start) -> Tuple[np.ndarray, None]:
        return np.stack([self.venv.action_space.sample() for _ in range(len(obs))], axis=0), None

    def _switch(self) -> None:
        explore = self.rng.random() < self.random_prob
        self.current_policy = self._random_policy if explore else self.wrapped_policy

    def __call__(self, observation, input_state: Optional[tuple], episode_start) -> Tuple[np.ndarray, None]:
        if input_state is not None:
            raise ValueError(_STATEFUL)
        acts, output_state = self.current_policy(observation, None, None)
        if output_state is not None:
            raise ValueError(_STATEFUL)
        if self.rng.random() < self.switch_prob:
            self._switch()
        return acts, None
