"""Host logic of the SAC learner (`imitation_amd/sac.py`) and of SQIL on it, with `device="cpu"` up to the point where the
device is needed: constructor surface and refusals, the initialisation order and the fused head's SB3 view, the `eps` drawn
ahead, the collection loop -- against the torch restatement `tests/sac_ref.py` (SB3 itself is installed nowhere: parity
unpinned) -- and the register budget of the built `sac_` kernels."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

import imitation_amd as p
from imitation_amd import sac, sqil
from tests import sac_ref, td3_golden

D, A = 3, 2
CPU = dict(device="cpu")


def _venv(n_envs=1, low=-1.0, high=1.0, horizon=8, seed=3):
    return td3_golden.make_env(dict(n_envs=n_envs, obs_dim=D, act_dim=A, horizon=horizon, low=low, high=high), seed)


def _demos(n=12, seed=0):
    r = np.random.default_rng(seed)
    return p.Transitions(obs=r.normal(size=(n, D)).astype(np.float32), acts=r.uniform(-1, 1, (n, A)).astype(np.float32),
                         next_obs=r.normal(size=(n, D)).astype(np.float32), dones=r.uniform(size=n) < 0.3)


def test_defaults_are_sb3s():
    d = {k: v.default for k, v in inspect.signature(p.SAC.__init__).parameters.items()}
    want = dict(learning_rate=3e-4, buffer_size=1_000_000, learning_starts=100, batch_size=256, tau=0.005, gamma=0.99,
                train_freq=1, gradient_steps=1, ent_coef="auto", target_update_interval=1, target_entropy="auto",
                action_noise=None)
    assert {k: d[k] for k in want} == want
    ref = {k: v.default for k, v in inspect.signature(sac_ref.SAC.__init__).parameters.items()}
    assert {k: ref[k] for k in want} == want
    venv = _venv()
    pol = p.SACPolicy(venv.observation_space, venv.action_space, lambda _: 3e-4)
    assert pol.net_arch == [256, 256] and pol.activation_fn is th.nn.ReLU and pol.n_critics == 2
    assert pol.betas == (0.9, 0.999) and pol.eps == 1e-8 and not hasattr(pol, "actor_target")
    algo = p.SAC("MlpPolicy", venv, **CPU)
    assert algo.train_freq == (1, "step") and algo.target_entropy == -float(A) and isinstance(algo.target_entropy, float)
    assert algo.policy.ent_learned and float(algo.log_ent_coef) == 0.0 and float(algo.policy.ent_state[3]) == 1.0
    assert not hasattr(algo, "policy_delay")
    half = p.SAC("MlpPolicy", venv, ent_coef="auto_0.5", target_entropy=-0.25, **CPU)
    assert float(half.log_ent_coef) == float(th.log(th.ones(1) * 0.5)) and half.target_entropy == -0.25
    const = p.SAC("MlpPolicy", venv, ent_coef=0.2, **CPU)
    assert const.log_ent_coef is None and float(const.policy.ent_state[3]) == float(np.float32(0.2))
    assert "ent_coef.exp_avg" in algo.policy.optimizer_state() and "ent_coef.exp_avg" not in const.policy.optimizer_state()
    assert p.sac is sac and p.SACPolicy is sac.MlpPolicy


def test_constructor_errors_and_refusals():
    venv = _venv()
    mk = lambda **kw: p.SAC("MlpPolicy", venv, **dict(CPU, **kw))
    for name in ("CnnPolicy", "MultiInputPolicy"):
        with pytest.raises(NotImplementedError, match="MlpPolicy"):
            p.SAC(name, venv, **CPU)
    for kw in (dict(use_sde=True), dict(sde_sample_freq=4), dict(use_sde_at_warmup=True), dict(policy_kwargs=dict(use_sde=True))):
        with pytest.raises(NotImplementedError, match="gSDE"):
            mk(**kw)
    with pytest.raises(NotImplementedError, match="tensorboard"):
        mk(tensorboard_log="x")
    with pytest.raises(NotImplementedError, match="optimize_memory_usage"):
        mk(optimize_memory_usage=True)
    with pytest.raises(NotImplementedError, match="share_features_extractor"):
        mk(policy_kwargs=dict(share_features_extractor=True))
    with pytest.raises(NotImplementedError, match="extractor"):
        mk(policy_kwargs=dict(features_extractor_class=object))
    with pytest.raises(NotImplementedError, match="Adam"):
        mk(policy_kwargs=dict(optimizer_class=th.optim.SGD))
    with pytest.raises(NotImplementedError, match="1 or 2 critics"):
        mk(policy_kwargs=dict(n_critics=3))
    with pytest.raises(ValueError, match="ent_coef"):
        mk(ent_coef="fixed")
    with pytest.raises(NotImplementedError, match="Box action"):
        p.SAC("MlpPolicy", p.SyntheticVecEnv(num_envs=1, obs_dim=D, n_discrete=3, prefetch_noise=False), **CPU)
    for arch in ([], [5], [7, 6, 5, 4], dict(pi=[8], qf=[9, 3])):   # no shape of net_arch raises
        pol = mk(policy_kwargs=dict(net_arch=arch)).policy
        assert pol.actor.stacks[0].dims[0] == D and pol.actor.stacks[0].dims[-1] == 2 * A
        assert pol.critic.stacks[0].dims[0] == D + A


def test_sqil_takes_sac_and_a_subclass_and_gail_refuses_it():
    venv = _venv()
    for cls in (p.SAC, type("MySAC", (p.SAC,), {})):
        algo = p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_algo_class=cls, rl_kwargs=CPU)
        assert isinstance(algo.rl_algo, cls) and isinstance(algo.rl_algo.replay_buffer, sqil.SQILReplayBuffer)
        assert algo.policy is algo.rl_algo.policy and isinstance(algo.policy, p.SACPolicy)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            algo.train(total_timesteps=8)
    with pytest.raises(NotImplementedError, match="this package's SAC"):
        p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_algo_class=p.PPO)
    gen = p.SAC("MlpPolicy", venv, **CPU)
    with pytest.raises(NotImplementedError, match="SAC generator"):
        p.GAIL(demonstrations=_demos(), demo_batch_size=4, venv=venv, gen_algo=gen,
               reward_net=p.BasicRewardNet(venv.observation_space, venv.action_space))


def test_train_and_predict_on_cpu_raise_no_cpu_fallback():
    algo = p.SAC("MlpPolicy", _venv(), learning_starts=0, **CPU)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.learn(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.predict(np.zeros(D, np.float32))


@pytest.mark.parametrize("net_arch", [[256, 256], [8], [], dict(pi=[8], qf=[16, 8])])
@pytest.mark.parametrize("n_critics", [1, 2])
def test_initialisation_consumes_the_generator_like_the_restatement_and_keys_match(net_arch, n_critics):
    venv = _venv()
    kw = dict(policy_kwargs=dict(net_arch=net_arch, n_critics=n_critics))
    th.manual_seed(5)
    ref = sac_ref.SAC("MlpPolicy", venv, **kw)
    want = th.get_rng_state()
    th.manual_seed(5)
    algo = p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_algo_class=p.SAC, rl_kwargs=dict(kw, **CPU)).rl_algo
    assert th.equal(th.get_rng_state(), want)
    ours, theirs = algo.policy.state_dict(), ref.policy.state_dict()
    assert list(ours) == list(theirs) and "actor.mu.weight" in ours and "actor.log_std.bias" in ours
    assert ("actor.latent_pi.0.weight" in ours) == (net_arch != []) and "critic.qf0.0.weight" in ours
    assert ("critic.qf1.0.weight" in ours) == (n_critics == 2)
    assert not any(k.startswith("actor_target.") for k in ours) and any(k.startswith("critic_target.") for k in ours)
    for k in ours:
        assert ours[k].shape == theirs[k].shape and th.equal(ours[k], theirs[k]), k
    assert [tuple(q.shape) for q in algo.policy.parameters()] == [tuple(q.shape) for q in ref.policy.parameters()]
    pol = algo.policy
    na = pol.actor.numel()
    assert th.equal(pol._online[na:], pol._target) and pol.actor._flat.data_ptr() == pol._online.data_ptr()
    # the two heads are ONE [2A, H] layer of the flat buffer: [mu.weight; log_std.weight], then [mu.bias; log_std.bias]
    H = pol.actor.stacks[0].dims[-2]
    head = pol.actor._flat[na - 2 * A * H - 2 * A:]
    assert th.equal(head[:2 * A * H].view(2 * A, H), th.cat([ours["actor.mu.weight"], ours["actor.log_std.weight"]]))
    assert th.equal(head[2 * A * H:], th.cat([ours["actor.mu.bias"], ours["actor.log_std.bias"]]))
    order = pol.actor.sb3_order()
    assert sorted(order.tolist()) == list(range(na))
    assert th.equal(pol.actor._flat[order], th.cat([q.reshape(-1) for q in ref.policy.actor.parameters()]))
    sd = {k: v + 1 for k, v in ours.items()}
    pol.load_state_dict(sd)
    assert all(th.equal(v, sd[k]) for k, v in pol.state_dict().items())


@pytest.mark.parametrize("net_arch", [[256, 256], dict(pi=[8], qf=[16, 8])])
@pytest.mark.parametrize("B", [1, 7, 256])
def test_eps_drawn_ahead_equals_the_restatements_draws_step_by_step(net_arch, B):
    venv = _venv()
    kw = dict(policy_kwargs=dict(net_arch=net_arch))
    algo = p.SAC("MlpPolicy", venv, **dict(CPU, **kw))
    ref = sac_ref.SAC("MlpPolicy", venv, **kw)
    n = 5
    th.manual_seed(9)
    ahead = algo.draw_eps(n, B)
    state = th.get_rng_state()
    th.manual_seed(9)
    obs = th.zeros(B, D)
    for s in range(n):   # what [SB3 SAC.train] draws per step: action_log_prob(obs), then action_log_prob(next_obs)
        for k in range(2):
            with th.no_grad():
                ref.actor.action_log_prob(obs)
            assert th.equal(ahead[s, k], ref.actor.action_dist.last_eps), (s, k)
    assert th.equal(th.get_rng_state(), state) and ahead.dtype == th.float32 and ahead.shape == (n, 2, B, A)
    assert ahead.abs().max() > 0
    # the draw of the restatement IS Normal.rsample's
    th.manual_seed(9)
    d = th.distributions.Normal(th.zeros(B, A), th.ones(B, A))
    assert th.equal(d.rsample(), ahead[0, 0])


def _torch_actor(pol):
    """The actor of `pol` in torch on the CPU (the collection test's stand-in for the device call)."""
    def action_log_prob(obs, eps):
        sd = pol.actor.state_dict()
        x = obs
        for i in range(len(pol.actor.net_arch)):
            x = F.relu(F.linear(x, sd[f"latent_pi.{2 * i}.weight"], sd[f"latent_pi.{2 * i}.bias"]))
        mu = F.linear(x, sd["mu.weight"], sd["mu.bias"])
        ls = F.linear(x, sd["log_std.weight"], sd["log_std.bias"]).clamp(sac.LOG_STD_MIN, sac.LOG_STD_MAX)
        return th.tanh(mu if eps is None else mu + eps * ls.exp()), th.zeros(len(obs))
    return action_log_prob


@pytest.mark.parametrize("n_envs", [1, 4])
@pytest.mark.parametrize("low,high,noise", [(-1.0, 1.0, False), (-2.0, 3.0, True)])
def test_collection_loop_against_the_restatement(n_envs, low, high, noise, monkeypatch):
    """Warm-up and policy branches, one [n_envs, A] `eps` draw per policy step, action noise, ring positions, and both
    generators afterwards. The device call of the policy branch is replaced by the same actor in torch."""
    monkeypatch.setattr(sac, "require_device", lambda device: None)
    runs = []
    for cls in (p.SAC, sac_ref.SAC):
        ours = cls is p.SAC
        venv = _venv(n_envs, low, high, horizon=5)
        kw = dict(train_freq=3, buffer_size=64, learning_starts=6 * n_envs, policy_kwargs=dict(net_arch=[8]))
        if noise:
            mod = p if ours else sac_ref
            kw["action_noise"] = mod.NormalActionNoise(np.zeros(A, np.float32), np.full(A, 0.7, np.float32))
        th.manual_seed(2)
        np.random.seed(4)
        venv.action_space.seed(5)
        algo = cls("MlpPolicy", venv, **(dict(kw, **CPU) if ours else kw))
        algo.set_logger((p.logger if ours else sac_ref.sb).Logger(None, []))
        branches, eps = [], []
        if ours:
            algo.policy.actor.action_log_prob = _torch_actor(algo.policy)
            orig = algo._sample_action

            def sample(*a, _o=orig, _algo=algo, **k):
                out = _o(*a, **k)
                branches.append(_algo.last_action_branch)
                if _algo.last_action_branch == "policy":
                    eps.append(_algo.policy.last_eps.numpy().copy())
                return out
            algo._sample_action = sample
        _, cb = algo._setup_learn(10_000, None, True)
        got = []
        for _ in range(4):
            args = (algo.env, cb, algo.train_freq) + (() if ours else (algo.replay_buffer,)) + (algo.learning_starts, None)
            got.append(tuple(algo.collect_rollouts(*args)))
        rb = algo.replay_buffer
        if ours:
            ring = rb.table.action[:rb.pos * n_envs].numpy().reshape(rb.pos, n_envs, A)
        else:
            ring, branches, eps = rb.actions[:rb.pos], [a[0] for a in algo.action_log], algo.act_eps_log
        runs.append(dict(got=got, pos=rb.pos, ring=ring.copy(), branches=branches, eps=np.stack(eps),
                         np_state=np.random.get_state()[1].copy(), th_state=th.get_rng_state().numpy().copy(),
                         t=algo.num_timesteps))
    ours, ref = runs
    assert ours["got"] == ref["got"] and ours["pos"] == ref["pos"] == 12 and ours["t"] == ref["t"]
    assert ours["branches"] == ref["branches"] and set(ours["branches"]) == {"warmup", "policy"}
    assert ours["eps"].shape == (6, n_envs, A) and np.array_equal(ours["eps"], ref["eps"])
    assert np.array_equal(ours["np_state"], ref["np_state"]) and np.array_equal(ours["th_state"], ref["th_state"])
    assert np.allclose(ours["ring"], ref["ring"], atol=1e-6) and np.abs(ours["ring"]).max() <= 1


def test_sac_kernels_keep_every_value_in_registers():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("llvm-readelf / c++filt not available")
    from tools.kernel_resources import kernel_notes

    ks = [k for k in kernel_notes() if "sac_" in k["name"]]
    for sub in ("sac_sample_kernel", "sac_alpha_step_kernel", "sac_min_seed_kernel", "sac_actor_seed_kernel"):
        assert any(sub in k["name"] for k in ks), (sub, ks)
    assert sorted(int(re.search(r"<(\d+)>", k["name"]).group(1)) for k in ks if "sac_critic_loss_kernel<" in k["name"]) == [1, 2]
    for k in ks:
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k
