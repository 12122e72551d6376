"""Host side of GAIL over a DQN `CnnPolicy` generator: the fixtures' integrity, `buffer.FrameReplayBuffer` against
`buffer.ReplayBuffer` on the host device (same positions, same draws), and every refusal. Nothing here launches a kernel."""
import json
import os

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import buffer, dqn
from imitation_amd.buffer import FrameReplayBuffer
from imitation_amd.dqn import FrameRewardStepSource
from imitation_amd.vec_env import SyntheticImageVecEnv, SyntheticVecEnv
from tests import gail_dqn_cnn_golden as gg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, N_ACTIONS = (3, 44, 48), 4
CPU = dict(device="cpu", buffer_size=64, learning_starts=8, batch_size=8,
           policy_kwargs=dict(features_extractor_kwargs=dict(features_dim=32)))


def image_env(n_envs=4):
    return SyntheticImageVecEnv(num_envs=n_envs, shape=SHAPE, act_dim=2, horizon=8, seed=3, n_discrete=N_ACTIONS)


def demos(n=24):
    r = np.random.default_rng(1)
    obs, nxt = (r.integers(0, 256, size=(n,) + SHAPE, dtype=np.uint8) for _ in range(2))
    return p.Transitions(obs=obs, acts=r.integers(0, N_ACTIONS, size=n), next_obs=nxt, dones=r.uniform(size=n) < 0.2)


@pytest.mark.parametrize("name", list(gg.CASES))
def test_fixture_integrity(name):
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    assert os.path.getsize(path) <= 1 << 20
    g = np.load(path)
    cfg = json.loads(str(g["cfg"]))
    want = dict(gg.COMMON, **gg.CASES[name])
    assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in want.items()} == {k: cfg[k] for k in want}
    assert cfg["case"] == name and cfg["gap_margin"] == gg.GAP_MARGIN
    n, rounds = cfg["n_envs"], cfg["rounds"]
    steps = rounds * cfg["gen_train_timesteps"] // n
    # the demonstrations, regenerated from the seed
    obs, acts, nxt, dones = gg.make_demos(cfg, cfg["seed"])
    assert obs.dtype == np.uint8 and gg.demo_crc(cfg, cfg["seed"]) == int(g["demo_crc"])
    assert np.array_equal(acts, g["demo_acts"]) and np.array_equal(dones, g["demo_dones"])
    # no frame is stored, only CRCs
    assert not any(k in g.files for k in ("ring_obs", "ring_next_obs", "gen_obs", "gen_next_obs", "demo_obs"))
    for k in ("ring_obs_crc", "ring_next_obs_crc"):
        assert g[k].shape == (steps,), k
    for k in ("gen_obs_crc", "gen_next_obs_crc", "gen_idx", "gen_n_data"):
        assert g[k].shape == (rounds,), k
    assert g["ring_pos"].shape == (steps,) and g["actions"].shape[0] == steps and g["branches"].shape == (steps,)
    assert (g["branches"] == gg.BRANCH["greedy"]).sum() >= 10
    # counters
    assert int(g["counter/num_timesteps"]) == steps * n and int(g["counter/global_step"]) == rounds
    assert int(g["counter/disc_step"]) == rounds * cfg["n_disc"]
    assert int(g["counter/n_updates"]) == len(g["f64/loss"]) == len(g["train_at"]) == len(g["sample_rows"])
    assert g["sample_rows"].shape[1] == cfg["batch_size"]
    # the online net only; per float key both precisions' record of what a test needs
    assert not any("q_net_target" in k for k in g.files)
    finals = [k for k in g.files if k.startswith("f64/final/")]
    assert finals and all(k.startswith("f64/final/q_net.") for k in finals)
    assert {k[len("f64/final/"):] for k in finals} == {k[len("init_crc/"):] for k in g.files if k.startswith("init_crc/")}
    for k in g.files:
        if k.startswith("dref/"):
            assert "f64/" + k[len("dref/"):] in g.files and float(g[k]) >= 0.0, k
    assert {"dref/ring_reward", "dref/loss", "dref/greedy_q", "dref_first_round/ring_reward"} <= set(g.files)
    assert any(k.startswith("dref/disc_final/cnn.") for k in g.files)


class _Steps:
    def __init__(self, seed=0):
        self.r = np.random.default_rng(seed)

    def batch(self, n):
        obs, nxt = (self.r.integers(0, 256, size=(n,) + SHAPE, dtype=np.uint8) for _ in range(2))
        return p.Transitions(obs=obs, acts=self.r.integers(0, N_ACTIONS, size=n), next_obs=nxt,
                             dones=self.r.uniform(size=n) < 0.3)


def test_frame_replay_buffer_stores_and_draws_like_the_replay_buffer():
    env = image_env()
    frames, plain = FrameReplayBuffer(10, env, device="cpu"), buffer.ReplayBuffer(10, env, device="cpu")
    assert frames.capacity == 10 and frames.table.obs.dtype == th.uint8 and frames.table.next_obs.dtype == th.uint8
    assert plain.table.obs.dtype == th.float32 and frames.table.obs.numel() == plain.table.obs.numel()
    assert frames.table.acts.dtype == th.int64 and frames.table.dones.dtype == th.uint8 and frames.table.discrete
    with pytest.raises(ValueError, match="empty"):
        frames.sample_indices(3)
    steps = _Steps()
    for n in (4, 4, 4, 3, 13, 1):   # (wraps at the third store; 13 rows exceed the capacity: the last 10 are kept)
        t = steps.batch(n)
        frames.store(t)
        plain.store(t)
        assert frames.size() == plain.size() and frames._idx == plain._idx
        a, b = frames._arrays, plain._arrays
        for k in ("obs", "acts", "next_obs", "dones"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        np.random.seed(5)
        rows = frames.sample_indices(7)
        state = np.random.get_state()[1].copy()
        np.random.seed(5)
        assert np.array_equal(rows, plain.sample_indices(7)) and np.array_equal(state, np.random.get_state()[1])
    with pytest.raises(ValueError, match="Not enough capacity"):
        frames.store(steps.batch(11), truncate_ok=False)
    with pytest.raises(ValueError, match="uint8"):
        t = steps.batch(2)
        frames.store(p.Transitions(obs=t.obs.astype(np.float32), acts=t.acts, next_obs=t.next_obs.astype(np.float32),
                                   dones=t.dones))
    assert type(frames).sample_indices is buffer.ReplayBuffer.sample_indices   # (the trainer's pre-draws ask for this)
    flat = SyntheticVecEnv(num_envs=4, obs_dim=5, act_dim=2, horizon=8, seed=3, n_discrete=3)
    with pytest.raises(TypeError, match="uint8 frames"):
        FrameReplayBuffer(10, flat, device="cpu")


def make_gail(env=None, gen_kwargs=None, net=None, cls=None, **kw):
    env = env or image_env()
    model = p.DQN("CnnPolicy", env, **dict(CPU, **(gen_kwargs or {})))
    net = net or p.modules.CnnRewardNet(env.observation_space, env.action_space, hwc_format=False)
    return (cls or p.GAIL)(demonstrations=demos(), demo_batch_size=8, venv=env, gen_algo=model, reward_net=net,
                           custom_logger=p.configure_logger(None, []), **kw)


def test_a_generator_off_the_gpu_is_refused_by_name():
    """The frame path has no host implementation: the constructor says so, naming CnnPolicy, before the generic device
    check (whose message would be `no CPU fallback`)."""
    with pytest.raises(NotImplementedError, match="CnnPolicy.*no host implementation.*GPU only"):
        make_gail()


def test_new_refusals():
    class _World:   # (a data-parallel context: refused before anything reads it)
        world, rank = 2, 0

    with pytest.raises(NotImplementedError, match="data_parallel is not implemented for a DQN generator with a CnnPolicy"):
        make_gail(data_parallel=_World())
    with pytest.raises(NotImplementedError, match="disc_grad_penalty_coef > 0 is not implemented for a DQN generator"):
        make_gail(disc_grad_penalty_coef=1.0)
    env = image_env()
    with pytest.raises(TypeError, match="AIRL needs a stochastic policy"):
        make_gail(env, cls=p.AIRL, net=p.modules.CnnRewardNet(env.observation_space, env.action_space, hwc_format=False))
    # the refusals that stay: the float32 step source on a frame ring, the relabelling wrapper over an image space
    model = p.DQN("CnnPolicy", env, **CPU)
    with pytest.raises(NotImplementedError, match="uint8 frame ring"):
        dqn.RewardStepSource(model.replay_buffer, None)
    with pytest.raises(NotImplementedError, match="image space"):
        p.replay_buffer_wrapper.ReplayBufferRewardWrapper(16, env.observation_space, env.action_space,
                                                          replay_buffer_class=dqn.ReplayBuffer,
                                                          reward_fn=lambda *a: np.zeros(1), device="cpu", n_envs=4)


def test_frame_step_source_refusals():
    env = image_env()
    model = p.DQN("CnnPolicy", env, **CPU)
    net = p.modules.CnnRewardNet(env.observation_space, env.action_space, hwc_format=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FrameRewardStepSource(model.replay_buffer, net)
    flat = SyntheticVecEnv(num_envs=4, obs_dim=5, act_dim=2, horizon=8, seed=3, n_discrete=3)
    mlp = p.DQN("MlpPolicy", flat, device="cpu", buffer_size=64, learning_starts=8, batch_size=8)
    with pytest.raises(TypeError, match="uint8 frames"):
        FrameRewardStepSource(mlp.replay_buffer, net)
    # what the reward launch covers: CnnRewardNet over channel-first frames, plain or under GAIL's softplus
    assert dqn.frame_reward_plan(net) == (net, False)
    assert dqn.frame_reward_plan(p.modules.RewardNetFromDiscriminatorLogit(net)) == (net, True)
    hwc = SyntheticImageVecEnv(num_envs=4, shape=(44, 48, 3), act_dim=2, horizon=8, seed=3, n_discrete=N_ACTIONS)
    assert dqn.frame_reward_plan(p.modules.CnnRewardNet(hwc.observation_space, hwc.action_space, hwc_format=True)) is None
    assert dqn.frame_reward_plan(p.modules.BasicRewardNet(flat.observation_space, flat.action_space)) is None
