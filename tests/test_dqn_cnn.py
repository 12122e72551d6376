"""Host side of DQN's `CnnPolicy` (`imitation_amd/dqn.py`): construction parity with the torch restatement
(`tests/dqn_cnn_ref.py`), the state-dict permutations, the uint8 ring on the host device, every refusal, and the CPU
guards. Nothing here launches a kernel."""
import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import dqn, spaces
from imitation_amd.vec_env import SyntheticImageVecEnv, SyntheticVecEnv
from tests import dqn_cnn_ref

SHAPE = (3, 44, 48)   # maps 10 x 11, 4 x 4, 2 x 2: a final map with H != W, so a wrong (h, w, c) permutation shows
N_ACTIONS, FEATURES = 4, 32
CPU = dict(device="cpu", buffer_size=64, learning_starts=8, batch_size=8)
KEYS = {"features_extractor.cnn.0": ((32, 3, 8, 8), (32,)), "features_extractor.cnn.2": ((64, 32, 4, 4), (64,)),
        "features_extractor.cnn.4": ((64, 64, 3, 3), (64,)), "features_extractor.linear.0": ((FEATURES, 256), (FEATURES,)),
        "q_net.0": ((N_ACTIONS, FEATURES), (N_ACTIONS,))}


def image_env(shape=SHAPE, n_actions=N_ACTIONS, n_envs=4):
    return SyntheticImageVecEnv(num_envs=n_envs, shape=shape, act_dim=2, horizon=8, seed=3, n_discrete=n_actions)


def flat_env():
    return SyntheticVecEnv(num_envs=4, obs_dim=5, act_dim=2, horizon=8, seed=3, n_discrete=3)


def make_dqn(env=None, **kw):
    kw = dict(CPU, policy_kwargs=dict(features_extractor_kwargs=dict(features_dim=FEATURES)), **kw)
    return p.DQN("CnnPolicy", env or image_env(), **kw)


def restatement(env):
    return dqn_cnn_ref.CnnPolicy(env.observation_space, env.action_space, lambda _: 1e-4,
                                 features_extractor_kwargs=dict(features_dim=FEATURES))


def test_construction_matches_the_torch_restatement():
    env = image_env()
    th.manual_seed(11)
    ref = restatement(env)
    ref_state_after = th.get_rng_state()
    np_before = np.random.get_state()
    th.manual_seed(11)
    model = make_dqn(env)
    assert th.equal(th.get_rng_state(), ref_state_after)
    after = np.random.get_state()
    assert np_before[0] == after[0] and np.array_equal(np_before[1], after[1]) and np_before[2:] == after[2:]
    assert isinstance(model.policy, p.CnnPolicy) and isinstance(model.policy, p.DQNPolicy)
    assert isinstance(model.q_net, p.CnnQNetwork) and model.q_net is model.policy.q_net
    sd, want = model.policy.state_dict(), ref.state_dict()
    assert set(sd) == set(want) == {f"{net}.{k}.{part}" for net in ("q_net", "q_net_target") for k in KEYS
                                    for part in ("weight", "bias")}
    for k, (w_shape, b_shape) in KEYS.items():
        assert tuple(sd[f"q_net.{k}.weight"].shape) == w_shape and tuple(sd[f"q_net.{k}.bias"].shape) == b_shape
    for k in want:
        assert sd[k].dtype == th.float32 and th.equal(sd[k], want[k]), k
        assert th.equal(sd["q_net_target." + k.split(".", 1)[1]], sd["q_net." + k.split(".", 1)[1]])
    # Adam runs over the online parameters, trunk included
    assert model.policy.exp_avg.numel() == sum(v.numel() for k, v in want.items() if k.startswith("q_net."))


def test_state_dict_round_trips_are_the_identity():
    env = image_env()
    model = make_dqn(env)
    sd = {k: v.clone() for k, v in model.policy.state_dict().items()}
    flat = model.q_net._flat.clone()
    model.policy.load_state_dict(sd)
    assert th.equal(model.q_net._flat, flat)
    for k, v in model.policy.state_dict().items():
        assert th.equal(v, sd[k]), k
    # the permutation check: another net's torch-layout state in and out again, online and target distinct
    th.manual_seed(5)
    ref = restatement(env)
    with th.no_grad():
        for q in ref.q_net_target.parameters():
            q.mul_(-0.5)
    want = ref.state_dict()
    model.policy.load_state_dict(want)
    got = model.policy.state_dict()
    for k in want:
        assert th.equal(got[k], want[k]), k
    assert not th.equal(got["q_net.q_net.0.weight"], got["q_net_target.q_net.0.weight"])
    # the device layout is NOT torch's for the permuted tensors (else the check above would show nothing)
    q = model.q_net
    o, n, _, _ = q._offsets[3]
    assert not th.equal(q._flat[o:o + n], want["q_net.features_extractor.linear.0.weight"].reshape(-1))
    # ... and is channel-last: linear.0's column (h, w, c) holds torch's column (c, h, w)
    w_dev = q._flat[o:o + n].view(FEATURES, 2, 2, 64)
    w_torch = want["q_net.features_extractor.linear.0.weight"].view(FEATURES, 64, 2, 2)
    assert th.equal(w_dev[5, 1, 0, 7], w_torch[5, 7, 1, 0])
    mapped = q.grad_to_torch(q._flat)
    for k, v in mapped.items():
        assert th.equal(v, want["q_net." + k]), k


def test_features_dim_default_and_kwarg():
    env = image_env(shape=(4, 36, 36), n_actions=3)
    pol = p.CnnPolicy(env.observation_space, env.action_space, lambda _: 1e-4)
    assert pol.q_net.features_dim == 512 and pol.net_arch == [] and pol.frames
    assert tuple(pol.state_dict()["q_net.features_extractor.linear.0.weight"].shape) == (512, 64)
    pol = p.DQNPolicy(env.observation_space, env.action_space, lambda _: 1e-4, features_extractor_class=p.cnn_policy.NatureCNN,
                      features_extractor_kwargs=dict(features_dim=64))
    assert pol.q_net.features_dim == 64 and pol.frames


def test_image_ring_is_uint8_and_returns_the_stored_bytes():
    env = image_env()
    rb = dqn.ReplayBuffer(16, env.observation_space, env.action_space, device="cpu", n_envs=4)
    assert rb.frames and rb.table.obs.dtype == th.uint8 and rb.table.next_obs.dtype == th.uint8
    assert tuple(rb.table.obs.shape) == (16, int(np.prod(SHAPE)))
    r = np.random.default_rng(0)
    written = []
    for _ in range(5):   # (wraps: 4 positions of 4 rows)
        obs, nxt = (r.integers(0, 256, size=(4,) + SHAPE, dtype=np.uint8) for _ in range(2))
        act, done = r.integers(0, N_ACTIONS, size=4), r.uniform(size=4) < 0.3
        pos = rb.pos
        rb.add(obs, nxt, act, np.ones(4, np.float32), done, [{} for _ in range(4)])
        written.append((pos, obs, nxt, act, done))
    ring = {}
    for pos, obs, nxt, act, done in written:
        for e in range(4):
            ring[pos * 4 + e] = (obs[e], nxt[e], act[e], float(done[e]))
    np.random.seed(2)
    rows, n_new = rb.sample_rows(32)
    np.random.seed(2)
    s = rb.sample(32)
    assert n_new == 32 and s.observations.dtype == th.uint8 and s.next_observations.dtype == th.uint8
    assert tuple(s.observations.shape) == (32,) + SHAPE
    for i, row in enumerate(rows):
        obs, nxt, act, done = ring[int(row)]
        assert np.array_equal(s.observations[i].numpy(), obs) and np.array_equal(s.next_observations[i].numpy(), nxt)
        assert int(s.actions[i]) == act and float(s.dones[i]) == done and float(s.rewards[i]) == 1.0
    with pytest.raises(ValueError, match="uint8"):
        rb.add(np.zeros((4,) + SHAPE, np.float32), np.zeros((4,) + SHAPE, np.float32), act, np.ones(4), done, [{}] * 4)
    # a flat space keeps its float32 tables
    fe = flat_env()
    flat = dqn.ReplayBuffer(16, fe.observation_space, fe.action_space, device="cpu", n_envs=4)
    assert not flat.frames and flat.table.obs.dtype == th.float32


def _demos(n=24, dtype=np.uint8):
    r = np.random.default_rng(1)
    obs, nxt = (r.integers(0, 256, size=(n,) + SHAPE).astype(dtype) for _ in range(2))
    return p.Transitions(obs=obs, acts=r.integers(0, N_ACTIONS, size=n), next_obs=nxt, dones=r.uniform(size=n) < 0.2)


def test_sqil_buffer_over_uint8_demonstrations():
    env, demos = image_env(), _demos()
    rb = p.sqil.SQILReplayBuffer(16, env.observation_space, env.action_space, demos, device="cpu", n_envs=4)
    assert rb.expert.frames and rb.expert.obs.dtype == th.uint8 and rb.expert.rows == 24
    assert np.array_equal(rb.expert.obs.numpy(), demos.obs.reshape(24, -1))
    assert np.array_equal(rb.expert.next_obs.numpy(), demos.next_obs.reshape(24, -1))
    r = np.random.default_rng(4)
    obs, nxt = (r.integers(0, 256, size=(4,) + SHAPE, dtype=np.uint8) for _ in range(2))
    rb.add(obs, nxt, np.arange(4) % N_ACTIONS, np.full(4, 7.0), np.zeros(4, bool), [{} for _ in range(4)])
    np.random.seed(9)
    rows, n_new = rb.sample_rows(7)
    np.random.seed(9)
    s = rb.sample(7)
    assert n_new == 3 and s.observations.dtype == th.uint8 and tuple(s.observations.shape) == (7,) + SHAPE
    assert s.rewards.reshape(-1).tolist() == [0.0] * 3 + [1.0] * 4
    for i in range(3):
        assert np.array_equal(s.observations[i].numpy(), obs[rows[i]])
    for i in range(3, 7):
        assert np.array_equal(s.observations[i].numpy(), demos.obs[rows[i]])
        assert np.array_equal(s.next_observations[i].numpy(), demos.next_obs[rows[i]])
    with pytest.raises(ValueError, match="uint8"):
        rb.set_demonstrations(_demos(dtype=np.float32))
    algo = p.SQIL(venv=env, demonstrations=demos, policy="CnnPolicy",
                  rl_kwargs=dict(CPU, policy_kwargs=dict(features_extractor_kwargs=dict(features_dim=FEATURES))))
    assert isinstance(algo.policy, p.CnnPolicy) and algo.rl_algo.replay_buffer.expert.obs.dtype == th.uint8


def test_check_rows_refuses_an_index_outside_its_table():
    env = image_env()
    rb = p.sqil.SQILReplayBuffer(16, env.observation_space, env.action_space, _demos(), device="cpu", n_envs=4)
    check = p.DQNPolicy.check_rows
    check(np.array([[0, 15, 3, 0, 23, 23, 1]]), 3, rb.table, rb.expert)
    check(np.array([[0, 15, 3]]), 3, rb.table, None)
    for rows, n_new in (([[0, 16, 3, 0, 1, 2, 3]], 3), ([[0, 1, 2, 24, 1, 2, 3]], 3), ([[-1, 1, 2, 3, 1, 2, 3]], 3)):
        with pytest.raises(IndexError):
            check(np.array(rows), n_new, rb.table, rb.expert)
    with pytest.raises(ValueError, match="expert table"):
        check(np.array([[0, 1, 2, 3]]), 2, rb.table, None)


def test_refusals():
    env = image_env()
    osp, asp = env.observation_space, env.action_space
    mk = lambda space=osp, **kw: p.CnnPolicy(space, asp, lambda _: 1e-4, **kw)
    with pytest.raises(NotImplementedError, match="hidden layers"):
        mk(net_arch=[64])
    with pytest.raises(NotImplementedError, match="normalize_images"):
        mk(normalize_images=False)
    with pytest.raises(NotImplementedError, match="channel-last"):
        mk(spaces.Box(0, 255, (44, 48, 3), np.uint8))
    with pytest.raises(NotImplementedError, match="extractor"):
        mk(features_extractor_class=th.nn.Flatten)
    with pytest.raises(NotImplementedError, match="extractor"):
        p.DQNPolicy(osp, asp, lambda _: 1e-4, features_extractor_class=th.nn.Flatten)
    for bad in (spaces.Box(-1.0, 1.0, (5,), np.float32), spaces.Box(0.0, 1.0, SHAPE, np.float32),
                spaces.Box(0, 200, SHAPE, np.uint8)):
        with pytest.raises(ValueError, match="uint8 image"):
            mk(bad)
    with pytest.raises(ValueError, match="uint8 image"):
        p.DQN("CnnPolicy", flat_env(), **CPU)
    with pytest.raises(NotImplementedError, match="MlpPolicy"):
        p.TD3("CnnPolicy", SyntheticVecEnv(num_envs=4, obs_dim=5, act_dim=2, horizon=8, seed=3), **CPU)
    with pytest.raises(NotImplementedError, match="MlpPolicy"):
        p.SAC("CnnPolicy", SyntheticVecEnv(num_envs=4, obs_dim=5, act_dim=2, horizon=8, seed=3), **CPU)
    with pytest.raises(NotImplementedError, match="optimize_memory_usage"):
        dqn.ReplayBuffer(16, osp, asp, device="cpu", n_envs=4, optimize_memory_usage=True)
    with pytest.raises(NotImplementedError, match="image space"):
        p.replay_buffer_wrapper.ReplayBufferRewardWrapper(16, osp, asp, replay_buffer_class=dqn.ReplayBuffer,
                                                          reward_fn=lambda *a: np.zeros(1), device="cpu", n_envs=4)
    model = make_dqn(env)
    with pytest.raises(NotImplementedError, match="uint8 frame ring"):
        dqn.RewardStepSource(model.replay_buffer, None)
    demos = _demos()
    with pytest.raises(NotImplementedError, match="CnnPolicy"):
        p.GAIL(demonstrations=demos, demo_batch_size=8, venv=env, gen_algo=model,
               reward_net=p.modules.CnnRewardNet(osp, asp, hwc_format=False), custom_logger=p.configure_logger(None, []))
    # an MlpPolicy cannot read the uint8 ring an image space gets
    mlp = p.DQN("MlpPolicy", env, **CPU)
    with pytest.raises(NotImplementedError, match="CnnPolicy"):
        mlp.policy.update(mlp.replay_buffer.table, None, None, 8, 1, 8, 0.99, 10.0, 1e-4, None)


def test_cpu_device_has_no_fallback():
    env = image_env()
    model = make_dqn(env)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.learn(total_timesteps=64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.policy.q_values(env.reset())
    with pytest.raises(TypeError, match="uint8"):
        model.policy.q_values(env.reset().astype(np.float32))
