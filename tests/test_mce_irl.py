"""Host logic of `imitation_amd.mce_irl` (no GPU): the five demonstration forms of `MCEIRL.set_demonstrations` against the
occupancy measures the reference computed from the same data (`tests/golden/mce_*.npz`, `make_golden_mce.py`), its
errors and warning, `TabularPolicy.predict`, the finite-horizon check, the nets and optimisers the device loop refuses,
and the register use of the new kernels."""
import os
import shutil
import types
import warnings

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import data_types as dt
from imitation_amd import mce_irl, reward_nets, spaces
from imitation_amd.networks import RunningNorm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def env_of(g, horizon="golden"):
    return mce_irl.TabularEnv(transition_matrix=g["transition_matrix"], observation_matrix=g["observation_matrix"],
                              reward_matrix=g["reward_matrix"], horizon=int(g["horizon"]) if horizon == "golden" else horizon,
                              initial_state_dist=g["initial_state_dist"])


def net_of(env, **kw):
    return reward_nets.BasicRewardNet(env.observation_space, env.action_space, **{"use_action": False, "hid_sizes": [], **kw})


def algo_of(demos, env, discount=1.0, **kw):
    return mce_irl.MCEIRL(demos, env, net_of(env), np.random.default_rng(0), discount=discount,
                          custom_logger=p.configure_logger(None, []), **kw)


def test_exports_and_container():
    assert p.MCEIRL is mce_irl.MCEIRL and p.TabularPolicy is mce_irl.TabularPolicy and p.mce_irl is mce_irl
    env = env_of(golden("mce_linear"))
    assert (env.state_dim, env.action_dim, env.obs_dim, env.horizon) == (24, 3, 6, 8)
    assert env.state_space == spaces.Discrete(24) and env.action_space == spaces.Discrete(3)
    assert env.observation_space.shape == (6,)


def _trajectories(g):
    return [dt.TrajectoryWithRew(obs=s, acts=a, rews=np.zeros(len(a), np.float32), infos=None, terminal=True)
            for s, a in zip(g["traj_states"], g["traj_acts"])]


def _transitions(g):
    states, acts = g["traj_states"], g["traj_acts"]
    H = acts.shape[1]
    return dt.Transitions(obs=states[:, :-1].reshape(-1), acts=acts.reshape(-1), next_obs=states[:, 1:].reshape(-1),
                          dones=np.tile(np.arange(H) == H - 1, len(states)))


def test_set_demonstrations_occupancy_vector():
    g = golden("mce_linear")
    om = g["demo_state_om"]
    algo = algo_of(om, env_of(g))
    assert algo.demo_state_om is om


def test_set_demonstrations_trajectories_discounted():
    g = golden("mce_mlp_discount")
    algo = algo_of(_trajectories(g), env_of(g), discount=0.9)
    assert np.array_equal(algo.demo_state_om, g["demo_state_om"])
    algo = algo_of(iter(_trajectories(g)), env_of(g))            # any iterable, undiscounted
    assert np.array_equal(algo.demo_state_om, g["form_om/trajectories_undiscounted"])


def test_set_demonstrations_transitions():
    g = golden("mce_mlp_discount")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        algo = algo_of(_transitions(g), env_of(g))
    assert np.array_equal(algo.demo_state_om, g["form_om/transitions"])
    assert algo.demo_state_om.sum() == pytest.approx(int(g["horizon"]) + 1)


def test_set_demonstrations_transitions_without_next_obs_warns():
    g = golden("mce_mlp_discount")
    tr = _transitions(g)
    minimal = types.SimpleNamespace(obs=tr.obs, acts=tr.acts)
    with pytest.warns(UserWarning, match="Training MCEIRL with transitions that lack next observation."):
        algo = algo_of(minimal, env_of(g))
    assert np.array_equal(algo.demo_state_om, g["form_om/minimal"])


def test_set_demonstrations_mappings():
    g = golden("mce_mlp_discount")
    tr = _transitions(g)
    batches = [{"obs": tr.obs[i:i + 50], "acts": tr.acts[i:i + 50], "next_obs": th.as_tensor(tr.next_obs[i:i + 50]),
                "dones": tr.dones[i:i + 50]} for i in range(0, len(tr), 50)]
    algo = algo_of(batches, env_of(g))
    assert np.array_equal(algo.demo_state_om, g["form_om/mappings"])
    assert np.array_equal(g["form_om/mappings"], g["form_om/transitions"])


def test_set_demonstrations_errors():
    g = golden("mce_mlp_discount")
    env = env_of(g)
    with pytest.raises(ValueError, match="Cannot compute discounted OM from timeless Transitions."):
        algo_of(_transitions(g), env, discount=0.9)
    with pytest.raises(ValueError, match="Cannot compute discounted OM from timeless Transitions."):
        algo_of([{"obs": np.zeros(3, np.int64)}], env, discount=0.9)
    with pytest.raises(TypeError, match="Unsupported demonstration type <class 'int'>"):
        algo_of(5, env)
    with pytest.raises(AssertionError):
        algo_of(np.zeros((3, 3)), env)      # an occupancy measure is one-dimensional


class RecordingRng:
    """`choice` returns the last index of positive probability and records what it was asked."""

    def __init__(self):
        self.calls = []

    def choice(self, n, p=None):
        self.calls.append((n, np.array(p)))
        return int(np.nonzero(p)[0][-1])


def _pi(H=3, S=4, A=3, seed=0):
    r = np.random.default_rng(seed)
    pi = r.uniform(0.1, 1, size=(H, S, A))
    pi[:, :, 2][r.uniform(size=(H, S)) < 0.5] = 0.0
    return pi / pi.sum(axis=2, keepdims=True)


def test_tabular_policy_predict():
    pi = _pi()
    rng = RecordingRng()
    pol = mce_irl.TabularPolicy(spaces.Discrete(4), spaces.Discrete(3), pi, rng)
    obs = np.array([2, 0, 3])
    acts, state = pol.predict(obs)
    assert [c[0] for c in rng.calls] == [3, 3, 3]
    for (_, pr), s in zip(rng.calls, obs):                      # one draw per row, in row order, from pi[0, s]
        assert np.array_equal(pr, pi[0, s])
    assert np.array_equal(acts, [np.nonzero(pi[0, s])[0][-1] for s in obs])
    assert len(state) == 1 and np.array_equal(state[0], [1, 1, 1])

    rng.calls.clear()
    acts, state = pol.predict(obs, state=state, episode_start=np.array([False, True, False]))
    for (_, pr), s, t in zip(rng.calls, obs, [1, 0, 1]):        # the timesteps travel in `state`; a new episode restarts
        assert np.array_equal(pr, pi[t, s])
    assert np.array_equal(state[0], [2, 1, 2])

    rng.calls.clear()
    acts, state = pol.predict(obs, state=state, deterministic=True)
    assert rng.calls == []
    assert np.array_equal(acts, [pi[2, 2].argmax(), pi[1, 0].argmax(), pi[2, 3].argmax()])
    assert np.array_equal(state[0], [3, 2, 3])

    with pytest.raises(AssertionError, match="illegal state"):
        pol.predict(np.array([4]))
    with pytest.raises(AssertionError, match="timestep and obs batch size differ"):
        pol.predict(obs, state=(np.zeros(2, dtype=int),))
    with pytest.raises(NotImplementedError):
        pol.forward(obs)
    with pytest.raises(NotImplementedError):
        pol._predict(obs)


def test_tabular_policy_set_pi_assertions():
    pi = _pi()
    pol = mce_irl.TabularPolicy(spaces.Discrete(4), spaces.Discrete(3), pi, np.random.default_rng(0))
    with pytest.raises(AssertionError, match="expected three-dimensional policy"):
        pol.set_pi(pi[0])
    with pytest.raises(AssertionError, match="policy not normalized"):
        pol.set_pi(pi * 0.5)
    bad = pi.copy()
    bad[0, 0] = [1.5, -0.5, 0.0]
    with pytest.raises(AssertionError, match="policy has negative probabilities"):
        pol.set_pi(bad)
    assert pol.pi is pi
    with pytest.raises(AssertionError, match="state not tabular"):
        mce_irl.TabularPolicy(spaces.Box(-1, 1, (2,)), spaces.Discrete(3), pi, np.random.default_rng(0))
    with pytest.raises(AssertionError, match="action not tabular"):
        mce_irl.TabularPolicy(spaces.Discrete(4), spaces.Box(-1, 1, (2,)), pi, np.random.default_rng(0))


def test_policy_is_uniform_before_training():
    g = golden("mce_early_stop")
    algo = algo_of(g["demo_state_om"], env_of(g))
    assert algo.policy.pi.shape == (5, 12, 2) and (algo.policy.pi == 0.5).all()
    assert algo.optimizer.param_groups[0]["lr"] == 1e-2


def test_infinite_horizon_is_refused():
    g = golden("mce_early_stop")
    env = env_of(g, horizon=None)
    for fn in (mce_irl.mce_partition_fh, mce_irl.mce_occupancy_measures):
        with pytest.raises(ValueError, match="Only finite-horizon environments are supported."):
            fn(env)
    with pytest.raises(ValueError, match="Only finite-horizon environments are supported."):
        algo_of(g["demo_state_om"], env)


def test_unsupported_nets_and_optimisers_are_named():
    g = golden("mce_early_stop")
    env = env_of(g)
    om, rng = g["demo_state_om"], np.random.default_rng(0)
    with pytest.raises(NotImplementedError, match="uses actions"):
        mce_irl.MCEIRL(om, env, net_of(env, use_action=True), rng)
    with pytest.raises(NotImplementedError, match="uses next states, dones"):
        mce_irl.MCEIRL(om, env, net_of(env, use_next_state=True, use_done=True), rng)
    with pytest.raises(NotImplementedError, match="input normalisation layer"):
        mce_irl.MCEIRL(om, env, net_of(env, normalize_input_layer=RunningNorm), rng)
    shaped = reward_nets.BasicShapedRewardNet(env.observation_space, env.action_space)
    with pytest.raises(NotImplementedError, match="BasicShapedRewardNet"):
        mce_irl.MCEIRL(om, env, shaped, rng)
    with pytest.raises(NotImplementedError, match="implements Adam"):
        mce_irl.MCEIRL(om, env, net_of(env), rng, optimizer_cls=th.optim.SGD)
    with pytest.raises(NotImplementedError, match=r"Adam options \['foreach'\]"):
        mce_irl.MCEIRL(om, env, net_of(env), rng, optimizer_kwargs={"lr": 1e-3, "foreach": True})
    with pytest.raises(NotImplementedError, match="amsgrad"):
        mce_irl.MCEIRL(om, env, net_of(env), rng, optimizer_kwargs={"amsgrad": True})


def test_training_refuses_the_cpu():
    g = golden("mce_early_stop")
    algo = algo_of(g["demo_state_om"], env_of(g))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        algo.train(max_iter=1)


def test_squeeze_r():
    assert mce_irl.squeeze_r(th.zeros(5, 1)).shape == (5,)
    assert mce_irl.squeeze_r(th.zeros(5)).shape == (5,)
    with pytest.raises(AssertionError):
        mce_irl.squeeze_r(th.zeros(5, 1, 1))


def test_mce_kernels_keep_every_value_in_registers():
    from imitation_amd import _lib
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("llvm-readelf / c++filt not available")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libimitation_hip.so is not built")
    from tools.kernel_resources import kernel_notes

    ks = [k for k in kernel_notes() if "mce_" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    for want in ("mce_backup_kernel<true>", "mce_backup_kernel<false>", "mce_forward_slab_kernel", "mce_forward_sum_kernel",
                 "mce_discounted_sum_kernel", "mce_weights_kernel", "mce_norms_kernel"):
        assert want in names, (want, names)
    for k in ks:
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k
