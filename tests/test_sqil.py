"""SQIL / DQN host logic (no GPU): the reference's constructor surface, the replay index class against the SB3
restatement in `tests/sqil_ref.py`, schedules and counters, the init draw order, and the resource notes of dqn.hip."""
import os
import re
import shutil

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import dqn, sqil
from oracle import ref_shim
from tests import sqil_ref

D, A = 4, 2


def _venv(n_envs=4, obs_dim=D, n_actions=A):
    return p.SyntheticVecEnv(num_envs=n_envs, obs_dim=obs_dim, act_dim=2, horizon=8, n_discrete=n_actions,
                             prefetch_noise=False)


def _demos(n=12, obs_dim=D, n_actions=A, seed=0):
    r = np.random.default_rng(seed)
    return p.Transitions(obs=r.normal(size=(n, obs_dim)).astype(np.float32), acts=r.integers(0, n_actions, n),
                         next_obs=r.normal(size=(n, obs_dim)).astype(np.float32), dones=r.uniform(size=n) < 0.3)


def _trajs(obs_dim=D, n_actions=A):
    r = np.random.default_rng(3)
    return [p.TrajectoryWithRew(obs=r.normal(size=(L + 1, obs_dim)).astype(np.float32), acts=r.integers(0, n_actions, L),
                                rews=np.zeros(L, np.float32), infos=None, terminal=t) for L, t in ((5, True), (3, False))]


CPU = dict(device="cpu", buffer_size=64)


def test_constructor_errors_carry_the_reference_messages():
    venv = _venv()
    with pytest.raises(ValueError, match="SQIL uses a custom replay buffer: 'replay_buffer_class' not allowed."):
        p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_kwargs=dict(replay_buffer_class=dqn.ReplayBuffer))
    with pytest.raises(ValueError, match="SQIL uses a custom replay buffer: 'replay_buffer_kwargs' not allowed."):
        p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_kwargs=dict(replay_buffer_kwargs={}))
    with pytest.raises(NotImplementedError, match="only this package's DQN"):
        p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_algo_class=p.PPO)
    with pytest.raises(NotImplementedError):
        sqil.SQILReplayBuffer(64, venv.observation_space, venv.action_space, _demos(), device="cpu",
                              optimize_memory_usage=True)
    algo = p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_kwargs=CPU)
    assert algo.policy is algo.rl_algo.policy and isinstance(algo.policy, p.DQNPolicy)
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        algo.rl_algo.replay_buffer.sample(4, env=object())
    with pytest.raises(NotImplementedError, match="progress bar"):
        algo.train(total_timesteps=8, progress_bar=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.train(total_timesteps=8)


def test_dqn_defaults_are_sb3s():
    import inspect
    d = {k: v.default for k, v in inspect.signature(p.DQN.__init__).parameters.items()}
    want = dict(learning_rate=1e-4, buffer_size=1_000_000, learning_starts=50_000, batch_size=32, tau=1.0, gamma=0.99,
                train_freq=4, gradient_steps=1, target_update_interval=10_000, exploration_fraction=0.1,
                exploration_initial_eps=1.0, exploration_final_eps=0.05, max_grad_norm=10)
    assert {k: d[k] for k in want} == want
    pol = p.DQNPolicy(_venv().observation_space, _venv().action_space, lambda _: 1e-4)
    assert pol.net_arch == [64, 64] and pol.activation_fn is th.nn.ReLU and pol.betas == (0.9, 0.999) and pol.eps == 1e-8


def test_set_demonstrations_accepts_transitions_and_trajectories():
    venv = _venv()
    algo = p.SQIL(venv=venv, demonstrations=_demos(12), policy="MlpPolicy", rl_kwargs=CPU)
    rb = algo.rl_algo.replay_buffer
    assert rb.expert.rows == 12 and rb.expert_index.size() == 12 and rb.expert_index.n_envs == 1
    assert th.equal(rb.expert.reward, th.ones(12))
    demos = _demos(12)
    assert np.array_equal(rb.expert.obs.numpy(), demos.obs) and np.array_equal(rb.expert.action.numpy(), demos.acts)
    assert np.array_equal(rb.expert.done.numpy(), demos.dones.astype(np.float32))
    algo.set_demonstrations(_trajs())
    flat = p.flatten_trajectories(_trajs())
    assert rb.expert.rows == 8 and rb.expert_index.size() == 8
    assert np.array_equal(rb.expert.obs.numpy(), flat.obs) and np.array_equal(rb.expert.next_obs.numpy(), flat.next_obs)
    assert rb.expert.done.numpy().tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    for bad in (7, [1, 2, 3], "abc", [], {"obs": 1}):
        with pytest.raises(NotImplementedError, match="Unsupported demonstrations type"):
            algo.set_demonstrations(bad)


def test_add_stores_reward_zero_and_every_done_cuts_the_bootstrap():
    venv = _venv()
    rb = sqil.SQILReplayBuffer(64, venv.observation_space, venv.action_space, _demos(), device="cpu", n_envs=4)
    obs = np.arange(16, dtype=np.float32).reshape(4, 4)
    infos = [{}, {"TimeLimit.truncated": True}, {}, {}]
    rb.add(obs, obs + 1, np.array([1, 0, 1, 0]), np.full(4, 5.0), np.array([False, True, True, False]), infos)
    assert rb.pos == 1 and rb.table.reward[:4].tolist() == [0, 0, 0, 0]
    assert rb.table.done[:4].tolist() == [0, 1, 1, 0]   # (handle_timeout_termination=False: the truncation counts)
    assert rb.table.action[:4].tolist() == [1, 0, 1, 0] and np.array_equal(rb.table.next_obs[:4].numpy(), obs + 1)
    plain = dqn.ReplayBuffer(64, venv.observation_space, venv.action_space, device="cpu", n_envs=4)
    plain.add(obs, obs + 1, np.array([1, 0, 1, 0]), np.full(4, 5.0), np.array([False, True, True, False]), infos)
    assert plain.table.reward[:4].tolist() == [5, 5, 5, 5] and plain.table.done[:4].tolist() == [0, 0, 1, 0]


@pytest.mark.parametrize("batch", [1, 2, 7, 32])
def test_sample_is_split_in_half_learner_rows_first(batch):
    assert sqil.split_in_half(batch) == (batch // 2, batch - batch // 2)
    venv = _venv()
    rb = sqil.SQILReplayBuffer(64, venv.observation_space, venv.action_space, _demos(12), device="cpu", n_envs=4)
    for t in range(3):
        o = np.full((4, 4), 100.0 + t, np.float32)
        rb.add(o, o, np.zeros(4, np.int64), np.zeros(4), np.zeros(4, bool), [{}] * 4)
    np.random.seed(batch)
    rows, n_new = rb.sample_rows(batch)
    assert n_new == batch // 2 and len(rows) == batch
    assert (rows[:n_new] < 12).all() and (rows[n_new:] < 12).all()
    np.random.seed(batch)
    s = rb.sample(batch)
    assert s.rewards.reshape(-1).tolist() == [0.0] * n_new + [1.0] * (batch - n_new)
    assert (s.observations[:n_new] >= 100).all() and (s.observations[n_new:] < 50).all()
    assert np.array_equal(s.observations[n_new:].numpy(), _demos(12).obs[rows[n_new:]])
    assert s.actions.shape == (batch, 1) and s.dones.shape == (batch, 1)


@pytest.mark.parametrize("n_envs", [1, 4])
def test_replay_index_matches_the_sb3_restatement(n_envs):
    """Positions, env indices and the post-state of NumPy's global generator, over a ring that wraps."""
    venv = _venv(n_envs)
    ref = sqil_ref.ReplayBuffer(24, venv.observation_space, venv.action_space, n_envs=n_envs,
                                handle_timeout_termination=False)
    ref_exp = sqil_ref.ReplayBuffer(10, venv.observation_space, venv.action_space, handle_timeout_termination=False)
    for _ in range(10):
        ref_exp.add(np.zeros((1, D)), np.zeros((1, D)), np.zeros(1), np.array(1.0), np.zeros(1), [{}])
    ours, ours_exp = dqn.ReplayIndex(24, n_envs), dqn.ReplayIndex(10, 1)
    ours_exp.fill()
    assert ours.buffer_size == ref.buffer_size == 24 // n_envs and (ours_exp.pos, ours_exp.full) == (ref_exp.pos, ref_exp.full)
    z = np.zeros((n_envs, D), np.float32)
    for step in range(2 * ref.buffer_size + 3):
        at = ours.add()
        assert at == ref.pos
        ref.add(z, z, np.zeros(n_envs), np.zeros(n_envs), np.zeros(n_envs), [{}] * n_envs)
        assert (ours.pos, ours.full, ours.size()) == (ref.pos, ref.full, ref.size())
        for batch in (1, 7, 8):
            new_n, exp_n = batch // 2, batch - batch // 2
            np.random.seed(1000 + step)
            ref.sample(new_n)
            ref_exp.sample(exp_n)
            want_state = np.random.get_state()
            np.random.seed(1000 + step)
            a = ours.sample(new_n)
            b = ours_exp.sample(exp_n)
            got_state = np.random.get_state()
            assert np.array_equal(a[0], ref.sample_log[-1][0]) and np.array_equal(a[1], ref.sample_log[-1][1])
            assert np.array_equal(b[0], ref_exp.sample_log[-1][0]) and np.array_equal(b[1], ref_exp.sample_log[-1][1])
            assert got_state[2] == want_state[2] and np.array_equal(got_state[1], want_state[1])
            assert np.array_equal(ours.rows(*a), a[0] * n_envs + a[1]) and ours.rows(*a).dtype == np.int64
            # the row of (position, env) is where the restatement keeps that transition
            assert (ours.rows(*a) < ref.observations.shape[0] * n_envs).all()


def test_buffer_size_smaller_than_n_envs_keeps_one_position():
    assert dqn.ReplayIndex(3, 4).buffer_size == 1 and dqn.ReplayIndex(0, 1).buffer_size == 1


@pytest.mark.parametrize("interval,n_envs", [(2, 4), (4, 4), (10, 4), (16, 4), (1, 1)])
def test_exploration_schedule_and_target_update_counter(interval, n_envs, monkeypatch):
    venv = _venv(n_envs)
    kw = dict(CPU, target_update_interval=interval, exploration_fraction=0.3, exploration_initial_eps=0.9,
              exploration_final_eps=0.1)
    with pytest.warns(UserWarning) if n_envs > interval else _no_warning():
        algo = p.DQN("MlpPolicy", venv, **kw)
    th.manual_seed(0)
    ref = sqil_ref.DQN("MlpPolicy", venv, **kw)
    ref._logger = algo._logger = p.logger.Logger(None, [])
    assert algo.exploration_rate == 0.0 == ref.exploration_rate
    updates = []
    monkeypatch.setattr(algo.policy, "polyak_update", lambda tau: updates.append(algo._n_calls))
    total = 40 * n_envs
    for step in range(1, 41):
        for a in (algo, ref):
            a.num_timesteps = step * n_envs
            a._current_progress_remaining = 1.0 - float(a.num_timesteps) / float(total)
            a._on_step()
        assert algo.exploration_rate == ref.exploration_rate == ref.eps_log[-1]
    assert updates == ref.target_update_log and len(updates) == 40 // max(interval // n_envs, 1)
    assert algo.exploration_rate == 0.1 and abs(ref.eps_log[0] - (0.9 - 0.8 / 40 / 0.3)) < 1e-12


class _no_warning:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("net_arch", [[64, 64], [32, 32], [48]])
def test_init_draws_from_torchs_generator_like_the_restatement(net_arch):
    """q_net, then a separately initialised q_net_target (which then loads q_net's state): same parameters, same
    generator state afterwards."""
    venv = _venv()
    kw = dict(CPU, policy_kwargs=dict(net_arch=net_arch))
    th.manual_seed(5)
    ref = sqil_ref.DQN("MlpPolicy", venv, **kw)
    want = th.get_rng_state()
    th.manual_seed(5)
    algo = p.SQIL(venv=venv, demonstrations=_demos(), policy="MlpPolicy", rl_kwargs=kw).rl_algo
    assert th.equal(th.get_rng_state(), want)
    ours, theirs = algo.policy.state_dict(), ref.policy.state_dict()
    assert list(ours) == list(theirs)
    for k in ours:
        assert th.equal(ours[k], theirs[k]), k
    assert th.equal(algo.policy.q_net._flat, algo.policy.q_net_target._flat)
    assert algo.policy.q_net.fused_shape() == (len(net_arch) == 2)


def test_fused_shape_limits_and_the_switch(monkeypatch):
    mk = lambda d, a, arch, act=th.nn.ReLU: dqn.QNetwork(p.Box(-1, 1, (d,)), p.Discrete(a), arch, act)
    assert mk(64, 16, [64, 64]).fused_shape() and mk(1, 2, [32, 32]).fused_shape()
    for q in (mk(65, 2, [64, 64]), mk(4, 17, [64, 64]), mk(4, 2, [48, 48]), mk(4, 2, [64]), mk(4, 2, [64, 32]),
              mk(4, 2, [64, 64, 64]), mk(4, 2, [64, 64], th.nn.Tanh)):
        assert not q.fused_shape()
    monkeypatch.setenv("IA_DQN_FUSED", "0")
    assert not dqn.fused_enabled()
    monkeypatch.delenv("IA_DQN_FUSED")
    assert dqn.fused_enabled()


def test_dqn_kernels_keep_every_value_in_registers():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("llvm-readelf / c++filt not available")
    from tools.kernel_resources import kernel_notes

    ks = [k for k in kernel_notes() if "dqn_" in k["name"]]
    for sub in ("dqn_update_kernel<", "dqn_q_kernel<"):
        got = sorted(int(re.search(r"<(\d+)>", k["name"]).group(1)) for k in ks if sub in k["name"])
        assert got == [32, 64], (sub, ks)
    assert any("dqn_td_loss_kernel" in k["name"] for k in ks) and any("dqn_polyak_kernel" in k["name"] for k in ks)
    for k in ks:
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k


@pytest.mark.reference
def test_reference_sqil_buffer_samples_like_the_index_class():
    """The reference's own `SQILReplayBuffer` (over the SB3 restatement) against this package's buffer on the same seeds:
    the same rows in the same order, the same rewards, the same generator state afterwards."""
    if not ref_shim.reference_available():
        pytest.skip("reference sources not present")
    ref_shim.install()
    sqil_ref.install_sb3_modules()
    from imitation.algorithms import sqil as ref_sqil
    from imitation.data import types as ref_types

    venv = _venv()
    demos = _demos(12)
    ref_demos = ref_types.Transitions(obs=demos.obs, acts=demos.acts, next_obs=demos.next_obs, dones=demos.dones,
                                      infos=np.array([{}] * 12))
    theirs = ref_sqil.SQILReplayBuffer(24, venv.observation_space, venv.action_space, ref_demos, n_envs=4)
    ours = sqil.SQILReplayBuffer(24, venv.observation_space, venv.action_space, demos, device="cpu", n_envs=4)
    r = np.random.default_rng(0)
    for t in range(9):   # the ring of 6 positions wraps
        o, o2 = r.normal(size=(4, D)).astype(np.float32), r.normal(size=(4, D)).astype(np.float32)
        a, d = r.integers(0, A, 4), r.uniform(size=4) < 0.3
        for rb in (theirs, ours):
            rb.add(o, o2, a, np.ones(4, np.float32), d, [{}] * 4)
        for batch in (1, 2, 7, 32):
            np.random.seed(t * 100 + batch)
            want = theirs.sample(batch)
            want_state = np.random.get_state()
            np.random.seed(t * 100 + batch)
            got = ours.sample(batch)
            got_state = np.random.get_state()
            assert np.array_equal(got_state[1], want_state[1]) and got_state[2] == want_state[2]
            for name in want._fields:
                w, g = getattr(want, name).numpy(), getattr(got, name).numpy()
                assert w.shape == g.shape and np.array_equal(w.astype(np.float64), g.astype(np.float64)), (name, batch)
