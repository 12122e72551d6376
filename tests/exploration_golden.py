"""Shared by `tests/golden/make_golden_exploration.py` (which drives the reference's `ExplorationWrapper` and
`AgentTrainer`) and `tests/test_exploration.py` (which drives this package's): the case table, the stub algorithm, the
Discrete twin of `CountingVecEnv`, and `run_case`, which drives either implementation the same way and records what the
fixtures `tests/golden/exploration_*.npz` hold.

Nothing in a case rounds: environments count integers, the stub's action and the reward function are exactly
representable functions of the observation, and random actions are `Generator.uniform` / `Generator.integers` draws. The
host CPU therefore cannot move a bit, and the tests compare with exact equality.
"""
import json
import os
from types import SimpleNamespace

import numpy as np

from imitation_amd import spaces
from imitation_amd.vec_env import CountingVecEnv

HERE = os.path.dirname(os.path.abspath(__file__))
EPISODE_LENGTHS = [3, 5, 4]
N_ACTIONS = 3

CASES = {
    # the bare wrapper over the stub as a plain callable: `calls` calls on one observation batch
    "exploration_wrapper_box": dict(kind="wrapper", discrete=False, random_prob=0.5, switch_prob=0.3, calls=200, seed=0),
    "exploration_wrapper_discrete": dict(kind="wrapper", discrete=True, random_prob=0.5, switch_prob=0.3, calls=200,
                                         seed=1),
    # `AgentTrainer` over the stub; `ops` is the sequence of `train(steps)` / `sample(steps)` calls
    "exploration_trainer_box": dict(kind="trainer", discrete=False, exploration_frac=0.5, switch_prob=0.5,
                                    random_prob=0.5, seed=2,
                                    ops=[["train", 24], ["sample", 120], ["train", 24], ["sample", 120]]),
    # an empty buffer: the additional-sampling branch and the exploration branch run in the same call. One `sample(160)`
    # asks for 40 exploratory steps, 16 calls of the wrapper with three environments, which cannot hold 10 calls of each
    # policy: the call is made three times (no `train` in between, so the buffer is empty every time)
    "exploration_trainer_discrete_empty_buffer": dict(kind="trainer", discrete=True, exploration_frac=0.25,
                                                      switch_prob=0.2, random_prob=0.8, seed=6,
                                                      ops=[["sample", 160], ["sample", 160], ["sample", 160]]),
    # the agent's share is 0 steps: `_get_trajectories(..., 0)` returns []
    "exploration_trainer_all_exploration": dict(kind="trainer", discrete=False, exploration_frac=1.0, switch_prob=1.0,
                                                random_prob=0.5, seed=4, ops=[["train", 24], ["sample", 90]]),
    # int(0.01 * 20) == 0: a warning and no exploratory step
    "exploration_trainer_too_small": dict(kind="trainer", discrete=False, exploration_frac=0.01, switch_prob=0.5,
                                          random_prob=0.5, seed=5, ops=[["train", 24], ["sample", 20]]),
}
MIN_CALLS_EACH, MIN_CHANGES = 10, 4     # what the generator demands of every case that explores


def explores(cfg) -> bool:
    return cfg["kind"] == "wrapper" or any(op == "sample" and int(cfg["exploration_frac"] * steps) > 0
                                           for op, steps in cfg["ops"])


class DiscreteCountingVecEnv(CountingVecEnv):
    """`CountingVecEnv` with a `Discrete` action space (the actions do not move it either)."""

    def __init__(self, episode_lengths, n_actions: int = N_ACTIONS):
        super().__init__(episode_lengths)
        self.action_space = spaces.Discrete(n_actions)


def make_env(cfg):
    return DiscreteCountingVecEnv(EPISODE_LENGTHS) if cfg["discrete"] else CountingVecEnv(EPISODE_LENGTHS)


def stub_actions(obs, discrete: bool):
    if discrete:
        return (obs[:, 0].astype(np.int64) + 1) % N_ACTIONS
    return (obs[:, :1] * np.float32(0.5) - np.float32(1)).astype(np.float32)


class StubAlgorithm:
    """What `AgentTrainer` needs of an algorithm, and a plain callable for `policy_to_callable`. Like SB3's `learn` it
    resets the environment on its first call only and afterwards goes on from the observation it saw last."""

    def __init__(self, discrete: bool):
        self.discrete = discrete
        self.env = self.logger = self._last_obs = None
        self.calls = 0

    def set_env(self, env):
        self.env = env

    def get_env(self):
        return self.env

    def set_logger(self, logger):
        self.logger = logger

    def learn(self, total_timesteps, reset_num_timesteps=False, callback=None):
        if self._last_obs is None:
            self._last_obs = self.env.reset()
        for _ in range(-(-total_timesteps // self.env.num_envs)):
            self._last_obs = self.env.step(stub_actions(self._last_obs, self.discrete))[0]
        return self

    def __call__(self, obs, state, dones):
        self.calls += 1
        return stub_actions(obs, self.discrete), None


class CountingReward:
    """A reward function of the observation alone, counting its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self, obs, acts, next_obs, dones):
        self.calls += 1
        return (obs[:, 0] * np.float32(0.25) + np.float32(1)).astype(np.float32)


def generator_state(gen: np.random.Generator) -> np.ndarray:
    """A PCG64 state as decimal strings (its 128-bit words do not fit an integer array)."""
    st = gen.bit_generator.state
    assert st["bit_generator"] == "PCG64"
    return np.array([str(st["state"]["state"]), str(st["state"]["inc"]), str(st["has_uint32"]), str(st["uinteger"])])


def trace_wrapper(wrapper):
    """Notes, per call of `wrapper`, which policy acted (0 wrapped, 1 random) and its actions."""
    trace = SimpleNamespace(policy=[], acts=[])

    def noting(fn, which):
        def policy(obs, state, episode_start):
            acts, out_state = fn(obs, state, episode_start)
            trace.policy.append(which)
            trace.acts.append(np.array(acts))
            return acts, out_state
        return policy

    random_first = wrapper.current_policy == wrapper._random_policy
    wrapper.wrapped_policy = noting(wrapper.wrapped_policy, 0)
    wrapper._random_policy = noting(wrapper._random_policy, 1)
    wrapper.current_policy = wrapper._random_policy if random_first else wrapper.wrapped_policy
    return trace


def run_case(cfg, api, tmp):
    """Runs one case on `api` -- a namespace with `ExplorationWrapper`, `AgentTrainer` and `make_logger(folder)` of the
    implementation under test -- and returns the record as a dict of arrays."""
    venv = make_env(cfg)
    stub = StubAlgorithm(cfg["discrete"])
    rng = np.random.default_rng(cfg["seed"])
    out = {"cfg": json.dumps(cfg)}
    messages = []
    if cfg["kind"] == "wrapper":
        wrapper = api.ExplorationWrapper(stub, venv, cfg["random_prob"], cfg["switch_prob"], rng)
        trace = trace_wrapper(wrapper)
        obs = np.arange(len(EPISODE_LENGTHS), dtype=np.float32)[:, None]
        for _ in range(cfg["calls"]):
            acts, state = wrapper(obs, None, None)
            assert state is None
        out["rng_state0"] = generator_state(rng)
        out["space_state0"] = generator_state(venv.action_space._rng)
        n_samples = 1
    else:
        logger = api.make_logger(tmp)
        logger.log = lambda *a, **k: messages.append("log: " + " ".join(str(x) for x in a))
        logger.warn = lambda *a, **k: messages.append("warn: " + " ".join(str(x) for x in a))
        reward = CountingReward()
        trainer = api.AgentTrainer(stub, reward, venv, rng, exploration_frac=cfg["exploration_frac"],
                                   switch_prob=cfg["switch_prob"], random_prob=cfg["random_prob"], custom_logger=logger)
        trace = trace_wrapper(trainer.exploration_wrapper)
        n_samples = 0
        for op, steps in cfg["ops"]:
            if op == "train":
                trainer.train(steps)
                continue
            trajs = trainer.sample(steps)
            assert len(trajs) > 0 and all(len(t.obs) == len(t.acts) + 1 == len(t.rews) + 1 for t in trajs)
            pre = f"sample{n_samples}_"     # the trajectories in order, end to end (`lens`: their numbers of steps)
            out[pre + "lens"] = np.array([len(t.acts) for t in trajs], np.int64)
            out[pre + "terminal"] = np.array([t.terminal for t in trajs], np.bool_)
            for field in ("obs", "acts", "rews"):
                out[pre + field] = np.concatenate([getattr(t, field) for t in trajs])
            out[f"rng_state{n_samples}"] = generator_state(rng)
            out[f"space_state{n_samples}"] = generator_state(venv.action_space._rng)
            n_samples += 1
        out["reward_calls"] = np.int64(reward.calls)
    out["n_samples"] = np.int64(n_samples)
    out["messages"] = np.array(messages, dtype=str)
    out["stub_calls"] = np.int64(stub.calls)
    out["trace_policy"] = np.array(trace.policy, np.int64)
    act_shape = (len(EPISODE_LENGTHS),) + venv.action_space.shape
    out["trace_acts"] = (np.stack(trace.acts) if trace.acts else np.zeros((0,) + act_shape, venv.action_space.dtype))
    return out


def load(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    return z, json.loads(str(z["cfg"]))
