"""Host logic of the TD3 / DDPG learners (`imitation_amd/td3.py`) and of SQIL on them, with `device="cpu"` up to the point
where the device is needed: constructor surface and refusals, action scaling, the episode-unit collection loop, the
initialisation order and the noise drawn ahead -- against the torch restatement `tests/td3_ref.py`."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import dqn, sqil, td3
from imitation_amd.vec_env import SyntheticVecEnv
from oracle import ref_shim
from tests import sqil_ref, td3_golden, td3_ref

D, A = 3, 2
CPU = dict(device="cpu")


def _venv(n_envs=1, low=-1.0, high=1.0, horizon=8, seed=3):
    cfg = dict(n_envs=n_envs, obs_dim=D, act_dim=A, horizon=horizon, low=low, high=high)
    return td3_golden.make_env(cfg, seed)


def _demos(n=12, seed=0):
    r = np.random.default_rng(seed)
    return p.Transitions(obs=r.normal(size=(n, D)).astype(np.float32), acts=r.uniform(-1, 1, (n, A)).astype(np.float32),
                         next_obs=r.normal(size=(n, D)).astype(np.float32), dones=r.uniform(size=n) < 0.3)


def test_defaults_are_sb3s():
    d = {k: v.default for k, v in inspect.signature(p.TD3.__init__).parameters.items()}
    want = dict(learning_rate=1e-3, buffer_size=1_000_000, learning_starts=100, batch_size=100, tau=0.005, gamma=0.99,
                train_freq=(1, "episode"), gradient_steps=-1, action_noise=None, policy_delay=2, target_policy_noise=0.2,
                target_noise_clip=0.5)
    assert {k: d[k] for k in want} == want
    dd = {k: v.default for k, v in inspect.signature(p.DDPG.__init__).parameters.items()}
    assert {k: dd[k] for k in want if k in dd} == {k: v for k, v in want.items() if k in dd}
    assert not {"policy_delay", "target_policy_noise", "target_noise_clip"} & set(dd)
    venv = _venv()
    pol = p.TD3Policy(venv.observation_space, venv.action_space, lambda _: 1e-3)
    assert pol.net_arch == [400, 300] and pol.activation_fn is th.nn.ReLU and pol.n_critics == 2
    assert pol.betas == (0.9, 0.999) and pol.eps == 1e-8
    ddpg = p.DDPG("MlpPolicy", venv, **CPU)
    assert ddpg.policy.n_critics == 1 and ddpg.policy_delay == 1 and ddpg.target_noise_clip == 0.0
    assert ddpg.target_policy_noise == 0.1   # [SB3 ddpg.py]: drawn, then clipped to zero
    assert p.TD3("MlpPolicy", venv, **CPU).train_freq == (1, "episode")
    assert p.TD3("MlpPolicy", venv, train_freq=3, **CPU).train_freq == (3, "step")


def test_sqil_takes_td3_and_ddpg_with_default_arguments_and_refuses_the_rest():
    venv = _venv()
    for cls in (p.TD3, p.DDPG, type("MyTD3", (p.TD3,), {})):
        algo = p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_algo_class=cls, rl_kwargs=CPU)
        assert isinstance(algo.rl_algo, cls) and isinstance(algo.rl_algo.replay_buffer, sqil.SQILReplayBuffer)
        assert algo.policy is algo.rl_algo.policy
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            algo.train(total_timesteps=8)
    with pytest.raises(NotImplementedError, match="only this package's DQN, TD3 and DDPG are implemented .SAC is out of scope"):
        p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_algo_class=p.PPO)
    with pytest.raises(NotImplementedError, match="Discrete"):   # DQN on a Box action space
        p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_kwargs=CPU)


def test_constructor_errors_and_refusals():
    venv = _venv()
    mk = lambda **kw: p.TD3("MlpPolicy", venv, **dict(CPU, **kw))
    with pytest.raises(NotImplementedError, match="MlpPolicy"):
        p.TD3("CnnPolicy", venv, **CPU)
    with pytest.raises(NotImplementedError, match="tensorboard"):
        mk(tensorboard_log="x")
    with pytest.raises(NotImplementedError, match="optimize_memory_usage"):
        mk(optimize_memory_usage=True)
    with pytest.raises(NotImplementedError, match="share_features_extractor"):
        mk(policy_kwargs=dict(share_features_extractor=True))
    with pytest.raises(NotImplementedError, match="extractor"):
        mk(policy_kwargs=dict(features_extractor_class=object))
    with pytest.raises(NotImplementedError, match="gSDE"):
        mk(policy_kwargs=dict(use_sde=True))
    with pytest.raises(NotImplementedError, match="1 or 2 critics"):
        mk(policy_kwargs=dict(n_critics=3))
    with pytest.raises(ValueError, match="train_freq"):
        mk(train_freq=(1, "rollout"))
    with pytest.raises(TypeError, match="action_noise"):
        mk(action_noise=0.1)
    with pytest.raises(NotImplementedError, match="Box action"):
        p.TD3("MlpPolicy", SyntheticVecEnv(num_envs=1, obs_dim=D, n_discrete=3, prefetch_noise=False), **CPU)
    with pytest.raises(NotImplementedError, match="counted in steps"):   # DQN keeps refusing the pair
        p.DQN("MlpPolicy", SyntheticVecEnv(num_envs=1, obs_dim=D, n_discrete=3, prefetch_noise=False),
              train_freq=(1, "episode"), **CPU)
    algo = mk()
    with pytest.raises(NotImplementedError, match="progress bar"):
        algo.learn(8, progress_bar=True)
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        algo.replay_buffer.sample(4, env=object())
    with pytest.raises(AssertionError, match="only one env"):
        many = p.TD3("MlpPolicy", _venv(2), **CPU)
        many.set_logger(p.logger.Logger(None, []))
        _, cb = many._setup_learn(8, None, True)
        many.collect_rollouts(many.env, cb, many.train_freq, 100, None)
    for arch in ([], [5], [7, 6, 5, 4], dict(pi=[8], qf=[9, 3])):   # no shape of net_arch raises
        pol = mk(policy_kwargs=dict(net_arch=arch)).policy
        assert pol.actor.stacks[0].dims[0] == D and pol.critic.stacks[0].dims[0] == D + A


@pytest.mark.parametrize("low,high", [(-1.0, 1.0), (-2.0, 3.0)])
def test_scale_and_unscale_are_sb3s_round_trip(low, high):
    venv = _venv(low=low, high=high)
    ours = p.TD3("MlpPolicy", venv, **CPU).policy
    ref = td3_ref.TD3("MlpPolicy", venv).policy
    a = np.random.default_rng(0).uniform(low, high, size=(50, A)).astype(np.float32)
    s = ours.scale_action(a)
    assert s.dtype == np.float32 and np.array_equal(s, ref.scale_action(a)) and np.abs(s).max() <= 1 + 1e-6
    assert np.array_equal(ours.unscale_action(s), ref.unscale_action(s))
    assert np.allclose(ours.unscale_action(s), a, atol=1e-6)
    assert np.array_equal(ours.unscale_action(np.array([[-1.0, 1.0]], np.float32)), np.array([[low, high]], np.float32))


def _collect(algo, n_calls, learning_starts, total=10_000):
    """`n_calls` collection calls of a learner that stays in its warm-up (no device needed)."""
    logger = (p.logger if isinstance(algo, p.TD3) else td3_ref.sb).Logger(None, [])
    algo.set_logger(logger)
    _, cb = algo._setup_learn(total, None, True)
    out = []
    for _ in range(n_calls):
        if isinstance(algo, p.TD3):
            out.append(algo.collect_rollouts(algo.env, cb, algo.train_freq, learning_starts, None))
        else:
            out.append(algo.collect_rollouts(algo.env, cb, algo.train_freq, algo.replay_buffer, learning_starts, None))
    return out


@pytest.mark.parametrize("train_freq,n_envs,noise", [((1, "episode"), 1, False), ((2, "episode"), 1, True), (3, 4, True),
                                                      ((5, "step"), 1, False)])
@pytest.mark.parametrize("low,high", [(-1.0, 1.0), (-2.0, 3.0)])
def test_collection_loop_against_the_restatement(train_freq, n_envs, noise, low, high):
    """Steps per call, warm-up draws (one `action_space.sample()` per environment), action noise and its resets, scaled
    actions in the ring, unscaled ones to the environment, and NumPy's generator afterwards."""
    runs = []
    for mod, cls in ((td3, p.TD3), (td3_ref, td3_ref.TD3)):
        venv = _venv(n_envs, low, high, horizon=5)
        kw = dict(train_freq=train_freq, buffer_size=64, policy_kwargs=dict(net_arch=[8]))
        if noise:
            kw["action_noise"] = mod.NormalActionNoise(np.zeros(A, np.float32), np.full(A, 0.7, np.float32))
        np.random.seed(4)
        venv.action_space.seed(5)
        algo = cls("MlpPolicy", venv, **kw) if cls is td3_ref.TD3 else cls("MlpPolicy", venv, **dict(kw, **CPU))
        seen = []
        step = venv.step
        venv.step = lambda a, _s=step, _seen=seen: (_seen.append(np.array(a)), _s(a))[1]
        if isinstance(venv, td3_golden.BoundsWrapper):
            pass
        got = _collect(algo, 4, learning_starts=10_000)
        rb = algo.replay_buffer
        if cls is p.TD3:
            n = rb.pos * n_envs
            ring = rb.table.action[:n].numpy().reshape(rb.pos, n_envs, A)
            obs = rb.table.obs[:n].numpy().reshape(rb.pos, n_envs, D)
        else:
            ring, obs = rb.actions[:rb.pos], rb.observations[:rb.pos]
        runs.append(dict(got=got, pos=rb.pos, ring=ring.copy(), obs=obs.copy(), env_actions=np.stack(seen),
                         state=np.random.get_state()[1].copy(), t=algo.num_timesteps, ep=algo._episode_num,
                         vec=type(algo.action_noise).__name__))
    ours, ref = runs
    assert ours["got"] == [tuple(g) for g in ref["got"]] and ours["pos"] == ref["pos"] > 0
    assert (ours["t"], ours["ep"], ours["vec"]) == (ref["t"], ref["ep"], ref["vec"])
    for k in ("ring", "obs", "env_actions", "state"):
        assert np.array_equal(ours[k], ref[k]), k
    assert np.abs(ours["ring"]).max() <= 1 and ours["env_actions"].min() >= low and ours["env_actions"].max() <= high
    if isinstance(train_freq, tuple) and train_freq[1] == "episode":
        assert ours["ep"] == 4 * train_freq[0]   # a call runs until that many episodes have ended
    if noise:
        assert (np.abs(ours["ring"]) == 1).any()   # the clip after the noise binds


@pytest.mark.parametrize("cls_name,net_arch", [("TD3", [400, 300]), ("TD3", [8]), ("DDPG", [6, 5]), ("TD3", dict(pi=[4], qf=[3, 3]))])
def test_initialisation_consumes_the_generator_like_sb3_and_keys_match(cls_name, net_arch):
    venv = _venv()
    kw = dict(policy_kwargs=dict(net_arch=net_arch))
    th.manual_seed(5)
    ref = getattr(td3_ref, cls_name)("MlpPolicy", venv, **kw)
    want = th.get_rng_state()
    th.manual_seed(5)
    algo = p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_algo_class=getattr(p, cls_name),
                  rl_kwargs=dict(kw, **CPU)).rl_algo
    assert th.equal(th.get_rng_state(), want)
    ours, theirs = algo.policy.state_dict(), ref.policy.state_dict()
    assert list(ours) == list(theirs) and "actor.mu.0.weight" in ours and "critic.qf0.0.weight" in ours
    assert ("critic.qf1.0.weight" in ours) == (cls_name == "TD3")
    assert any(k.startswith("actor_target.") for k in ours) and any(k.startswith("critic_target.") for k in ours)
    for k in ours:
        assert th.equal(ours[k], theirs[k]), k
    pol = algo.policy
    assert th.equal(pol._online, pol._target) and pol.actor._flat.data_ptr() == pol._online.data_ptr()
    sd = {k: v + 1 for k, v in ours.items()}
    pol.load_state_dict(sd)
    assert all(th.equal(v, sd[k]) for k, v in pol.state_dict().items())


@pytest.mark.parametrize("cls_name,B", [("TD3", 100), ("TD3", 7), ("DDPG", 32), ("TD3", 1)])
def test_noise_drawn_ahead_equals_sb3s_draws_step_by_step(cls_name, B):
    venv = _venv()
    algo = getattr(p, cls_name)("MlpPolicy", venv, **dict(CPU, policy_kwargs=dict(net_arch=[4])))
    th.manual_seed(9)
    ahead = algo.draw_target_noise(5, B)
    state = th.get_rng_state()
    th.manual_seed(9)
    actions = th.zeros(B, A)   # what [SB3 TD3.train] draws on: the sampled float32 [B, A] actions
    for s in range(5):
        assert th.equal(ahead[s], actions.clone().data.normal_(0, algo.target_policy_noise))
    assert th.equal(th.get_rng_state(), state) and ahead.dtype == th.float32 and ahead.shape == (5, B, A)
    assert ahead.abs().max() > 0


@pytest.mark.parametrize("n_envs", [1, 4])
def test_box_replay_buffer_against_the_restatement(n_envs):
    venv = _venv(n_envs)
    ref = sqil_ref.ReplayBuffer(24, venv.observation_space, venv.action_space, n_envs=n_envs)
    ours = dqn.ReplayBuffer(24, venv.observation_space, venv.action_space, device="cpu", n_envs=n_envs)
    assert ours.table.action.shape == (ours.buffer_size * n_envs, A) and ours.table.action.dtype == th.float32
    r = np.random.default_rng(1)
    for step in range(2 * ref.buffer_size + 3):
        o, o2 = r.normal(size=(2, n_envs, D)).astype(np.float32)
        a = r.uniform(-1, 1, size=(n_envs, A)).astype(np.float32)
        done = r.uniform(size=n_envs) < 0.3
        infos = [{"TimeLimit.truncated": bool(r.uniform() < 0.5)} for _ in range(n_envs)]
        assert ours.pos == ref.pos
        for b in (ours, ref):
            b.add(o, o2, a, r.normal(size=n_envs).astype(np.float32) * 0 + step, done, infos)
    np.random.seed(2)
    want = ref.sample(9)
    state = np.random.get_state()[1].copy()
    np.random.seed(2)
    got = ours.sample(9)
    assert np.array_equal(np.random.get_state()[1], state)
    for k in want._fields:
        assert getattr(got, k).shape == getattr(want, k).shape, k
        assert np.array_equal(getattr(got, k).numpy(), getattr(want, k).numpy()), k
    # the Discrete column is what it was
    disc = dqn.ReplayBuffer(8, venv.observation_space, p.Discrete(3), device="cpu")
    assert disc.table.action.dtype == th.int64 and disc.table.action.shape == (8,) and disc.act_dim is None


def test_td3_kernels_keep_every_value_in_registers():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("llvm-readelf / c++filt not available")
    from tools.kernel_resources import kernel_notes

    ks = [k for k in kernel_notes() if "td3_" in k["name"]]
    for sub in ("td3_assemble_kernel", "td3_target_input_kernel", "td3_actor_input_kernel", "td3_actor_seed_kernel"):
        assert any(sub in k["name"] for k in ks), (sub, ks)
    assert sorted(int(re.search(r"<(\d+)>", k["name"]).group(1)) for k in ks if "td3_critic_loss_kernel<" in k["name"]) == [1, 2]
    for k in ks:
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k


@pytest.mark.reference
def test_reference_sqil_buffer_on_box_demonstrations():
    """The reference's own `SQILReplayBuffer` (over the SB3 restatement) against this package's on Box actions: the same
    expert table (actions as given, not scaled), the same sampled rows, rewards and generator state."""
    if not ref_shim.reference_available():
        pytest.skip("reference sources not present")
    ref_shim.install()
    td3_ref.install_sb3_modules()
    from imitation.algorithms import sqil as ref_sqil
    from imitation.data import types as ref_types

    venv = _venv(4, low=-2.0, high=3.0)
    demos = _demos(12)
    demos = p.Transitions(obs=demos.obs, acts=demos.acts * 2.5, next_obs=demos.next_obs, dones=demos.dones)
    ref_demos = ref_types.Transitions(obs=demos.obs, acts=demos.acts, next_obs=demos.next_obs, dones=demos.dones,
                                      infos=np.array([{}] * 12))
    theirs = ref_sqil.SQILReplayBuffer(24, venv.observation_space, venv.action_space, ref_demos, n_envs=4)
    ours = sqil.SQILReplayBuffer(24, venv.observation_space, venv.action_space, demos, device="cpu", n_envs=4)
    assert np.array_equal(ours.expert.action.numpy(), theirs.expert_buffer.actions.reshape(12, A))
    assert np.array_equal(ours.expert.action.numpy(), demos.acts) and np.abs(demos.acts).max() > 1
    r = np.random.default_rng(3)
    for step in range(4):
        o = r.normal(size=(4, D)).astype(np.float32)
        a = r.uniform(-1, 1, size=(4, A)).astype(np.float32)
        for b in (ours, theirs):
            b.add(o, o + 1, a, np.ones(4), np.zeros(4, bool), [{}] * 4)
    np.random.seed(7)
    want = theirs.sample(9)
    state = np.random.get_state()[1].copy()
    np.random.seed(7)
    got = ours.sample(9)
    assert np.array_equal(np.random.get_state()[1], state)
    for k in want._fields:
        assert np.array_equal(getattr(got, k).numpy(), getattr(want, k).numpy()), k
    assert got.rewards.reshape(-1).tolist() == [0.0] * 4 + [1.0] * 5
