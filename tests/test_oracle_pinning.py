"""Pins the oracle (CPU restatement) against (1) the committed golden vectors produced by
the reference's own code, (2) the reference itself when /root/reference is present, and
(3) the reference's known-answer tests for this path."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch as th

from oracle import imitation_restated as o
from oracle import ref_shim
from oracle import sb3_restated as sb
from tests import harness

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _compare(a, b, rtol, atol, exact_keys=harness.EXACT_KEYS):
    assert set(a) == set(b), set(a) ^ set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if k in exact_keys or x.dtype.kind in "biu":
            assert np.array_equal(x, y), k
        else:
            np.testing.assert_allclose(x, y, rtol=rtol, atol=atol, equal_nan=True, err_msg=k)


@pytest.mark.parametrize("case", list(harness.CASES))
def test_oracle_matches_golden(case, tmp_path):
    gold = dict(np.load(os.path.join(GOLDEN, f"{case}.npz")))
    got = harness.run_case("oracle", case, str(tmp_path))
    # Same torch-CPU ops in the same order: tight tolerance (exact on the generating host).
    _compare(got, gold, rtol=2e-4, atol=2e-5)


@pytest.mark.reference
@pytest.mark.skipif(not ref_shim.reference_available(), reason="/root/reference not present")
@pytest.mark.parametrize("case", ["gail_box", "airl_box"])
def test_oracle_bit_identical_to_live_reference(case, tmp_path):
    ref = harness.run_case("reference", case, str(tmp_path / "r"))
    got = harness.run_case("oracle", case, str(tmp_path / "o"))
    assert set(ref) == set(got)
    for k in ref:
        assert np.array_equal(ref[k], got[k], equal_nan=True), k


def test_sb3_fixture_layout():
    """The only offline-verifiable SB3 facts: key layout + Adam eps=1e-5."""
    lay = json.load(open(os.path.join(GOLDEN, "sb3_fixture_layout.json")))
    from imitation_amd import spaces
    pol = sb.ActorCriticPolicy(spaces.Box(-1, 1, (4,)), spaces.Discrete(2), lambda _: 1e-3)
    sd = {k: list(v.shape) for k, v in pol.state_dict().items()}
    assert sd == lay["state_dict"]
    pg = pol.optimizer.param_groups[0]
    assert pg["eps"] == lay["optimizer"]["eps"] == 1e-5
    assert list(pg["betas"]) == lay["optimizer"]["betas"]
    assert len(pg["params"]) == lay["optimizer"]["n_params"]
    ppo_fields = set(lay["hyperparameter_fields"])
    algo = sb.PPO(sb.ActorCriticPolicy, None, _init_setup_model=False)
    assert ppo_fields <= set(vars(algo))


# ---- known-answer tests restated from the reference's test-suite -------------------------


def test_shaped_reward_net_known_answer():
    """tests/rewards/test_reward_nets.py:753-768: 0 + 0.9*10 - 10 = -1."""
    from imitation_amd import spaces
    os_, as_ = spaces.Box(-1, 1, (2,)), spaces.Box(-1, 1, (1,))

    class Zero(o.RewardNet):
        def forward(self, s, a, ns, d):
            return th.zeros(s.shape[0])

    net = o.ShapedRewardNet(Zero(os_, as_), lambda x: th.full((x.shape[0],), 10.0), 0.9)
    n = 8
    out = net(th.zeros(n, 2), th.zeros(n, 1), th.zeros(n, 2), th.zeros(n))
    assert th.allclose(out, th.full((n,), -1.0))
    out_done = net(th.zeros(n, 2), th.zeros(n, 1), th.zeros(n, 2), th.ones(n))
    assert th.allclose(out_done, th.full((n,), -10.0))


def test_running_norm_matches_empirical_moments():
    """tests/util/test_networks.py:145-177: running stats == moments of all data; count exact."""
    th.manual_seed(3)
    rn = o.RunningNorm(5)
    chunks = [th.randn(n, 5) * 3 + 2 for n in (7, 64, 1, 200)]
    for c in chunks:
        rn.train()
        rn(c)
    allx = th.cat(chunks)
    assert int(rn.count) == len(allx)
    assert th.allclose(rn.running_mean, allx.mean(0), atol=1e-5)
    assert th.allclose(rn.running_var, allx.var(0, unbiased=False), atol=1e-4)
    rn.eval()
    before = rn.running_mean.clone()
    rn(th.randn(10, 5))
    assert th.equal(before, rn.running_mean)  # eval mode freezes (test_networks.py:112-142)


def test_replay_ring_semantics():
    """tests/data/test_buffer.py:54-77,117-173: FIFO wrap, _idx, truncation keeps the tail."""
    from imitation_amd.vec_env import SyntheticVecEnv
    venv = SyntheticVecEnv(num_envs=2, obs_dim=3, act_dim=2, horizon=5)
    buf = o.ReplayBuffer(10, venv)

    def mk(lo, hi):
        n = hi - lo
        base = np.arange(lo, hi, dtype=np.float32)
        return o.Transitions(obs=np.repeat(base[:, None], 3, 1), acts=np.repeat(base[:, None], 2, 1),
                             next_obs=np.repeat(base[:, None] + 0.5, 3, 1), dones=np.zeros(n, bool))

    buf.store(mk(0, 7))
    assert (buf._idx, buf.size()) == (7, 7)
    buf.store(mk(7, 13))  # wraps
    assert (buf._idx, buf.size()) == (3, 10)
    assert np.array_equal(buf._arrays["obs"][:, 0], [10, 11, 12, 3, 4, 5, 6, 7, 8, 9])
    buf.store(mk(100, 125))  # > capacity: keeps the last 10, written from _idx=3
    assert np.array_equal(buf._arrays["obs"][:, 0], [122, 123, 124, 115, 116, 117, 118, 119, 120, 121])
    np.random.seed(0)
    s = buf.sample(50)
    assert np.array_equal(s.obs[:, 0], s.acts[:, 0])  # in-order correspondence across keys
    assert np.array_equal(s.next_obs[:, 0], s.obs[:, 0] + 0.5)


@pytest.mark.parametrize("lens,n_steps", [((1,), 20), ((6, 5, 1, 2), 21), ((2, 2), 2), ((6, 5, 1, 2), 1)])
def test_buffering_wrapper_counting_env(lens, n_steps):
    """tests/data/test_wrappers.py:119-227: multiset of popped (obs, next_obs, rew) tuples."""
    from imitation_amd.vec_env import CountingVecEnv
    venv = o.BufferingWrapper(CountingVecEnv(lens))
    venv.reset()
    expect = []
    t = np.zeros(len(lens), int)
    for _ in range(n_steps):
        venv.step(np.zeros((len(lens), 1), np.float32))
        for i, L in enumerate(lens):
            expect.append((float(t[i]), float(t[i] + 1), 10.0 * (t[i] + 1)))
            t[i] = 0 if t[i] + 1 >= L else t[i] + 1
    assert venv.n_transitions == n_steps * len(lens)
    trajs, ep_lens = venv.pop_trajectories()
    trans = o.flatten_trajectories(trajs)
    got = sorted(zip(trans.obs[:, 0].tolist(), trans.next_obs[:, 0].tolist(), trans.rews.tolist()))
    assert got == sorted(expect)
    assert sorted(ep_lens) == sorted(L for L in lens for _ in range(n_steps // L))
    assert venv.n_transitions == 0


def test_fixed_horizon_check_and_stats_contract():
    """tests/algorithms/test_base.py:11-40; test_adversarial.py:421-435."""
    tr = o.AdversarialTrainer.__new__(o.AdversarialTrainer)
    tr.allow_variable_horizon, tr._horizon = False, None
    tr._check_fixed_horizon([5, 5])
    tr._check_fixed_horizon([])
    with pytest.raises(ValueError, match="different length"):
        tr._check_fixed_horizon([5, 6])
    stats = o.compute_train_stats(th.tensor([1.0, -2.0, 0.5, -0.1]), th.tensor([1, 0, 0, 1]), th.tensor(0.7))
    assert all(isinstance(v, float) for v in stats.values())
    assert stats["n_expert"] == 2 and stats["n_generated"] == 2
    assert stats["disc_acc"] == 0.5 and stats["disc_acc_expert"] == 0.5 and stats["disc_acc_gen"] == 0.5
    only_gen = o.compute_train_stats(th.tensor([1.0, -2.0]), th.tensor([0, 0]), th.tensor(0.7))
    assert np.isnan(only_gen["disc_acc_expert"])


def test_grad_accumulation_equivalence(tmp_path):
    """tests/algorithms/test_adversarial.py:285-343: minibatch 3 vs batch 6 over 8 steps."""
    cfg = dict(harness.CASES["gail_box"], demo_batch=6, demo_minibatch=None, capacity=None, norm_disc=False)
    a, _ = harness.build_trainer("oracle", cfg, str(tmp_path / "a"))
    b, _ = harness.build_trainer("oracle", dict(cfg, demo_minibatch=3), str(tmp_path / "b"))
    b._reward_net.load_state_dict(a._reward_net.state_dict())
    rng = np.random.default_rng(0)
    for step in range(8):
        mk = lambda: dict(obs=rng.standard_normal((6, 17)).astype(np.float32),
                          acts=rng.uniform(-1, 1, (6, 6)).astype(np.float32),
                          next_obs=rng.standard_normal((6, 17)).astype(np.float32), dones=np.zeros(6, bool))
        e, g = mk(), mk()
        a.train_disc(expert_samples=e, gen_samples=g)
        b.train_disc(expert_samples=e, gen_samples=g)
        for pa, pb in zip(a._reward_net.parameters(), b._reward_net.parameters()):
            assert th.allclose(pa, pb, atol=(1 + step) * 2e-4, rtol=(1 + step) * 1e-5)


def test_disc_loss_decreases(tmp_path):
    """tests/algorithms/test_adversarial.py:256-282."""
    tr, _ = harness.build_trainer("oracle", harness.CASES["gail_box"], str(tmp_path))
    tr.train_gen()
    rng = np.random.default_rng(0)
    mk = lambda: dict(obs=rng.standard_normal((64, 17)).astype(np.float32),
                      acts=rng.uniform(-1, 1, (64, 6)).astype(np.float32),
                      next_obs=rng.standard_normal((64, 17)).astype(np.float32), dones=np.zeros(64, bool))
    e, g = mk(), mk()
    losses = [tr.train_disc(expert_samples=e, gen_samples=g)["disc_loss"] for _ in range(4)]
    assert losses[-1] < losses[0]


def test_trainer_error_contract(tmp_path):
    """common.py:193-194, 548-551, 555-562, 447-452; airl.py:114-117."""
    cfg = harness.CASES["gail_box"]
    with pytest.raises(ValueError, match="multiple of minibatch"):
        harness.build_trainer("oracle", dict(cfg, demo_minibatch=5), str(tmp_path / "a"))
    tr, _ = harness.build_trainer("oracle", cfg, str(tmp_path / "b"))
    with pytest.raises(RuntimeError, match="No generator samples"):
        tr.train_disc()
    with pytest.raises(AssertionError):
        tr.train(1)
    tr.train_gen()
    with pytest.raises(ValueError, match="exactly `demo_batch_size`"):
        bad = dict(obs=np.zeros((3, 17), np.float32), acts=np.zeros((3, 6), np.float32),
                   next_obs=np.zeros((3, 17), np.float32), dones=np.zeros(3, bool))
        tr.train_disc(gen_samples=bad)
    at, _ = harness.build_trainer("oracle", harness.CASES["airl_box"], str(tmp_path / "c"))
    with pytest.raises(TypeError):
        at.logits_expert_is_high(th.zeros(2, 11), th.zeros(2, 3), th.zeros(2, 11), th.zeros(2), None)


CNN_REWARD_NET_KWS = [dict(), dict(use_next_state=True, use_done=True), dict(use_action=False),
                      dict(use_action=False, use_done=True, hwc_format=False, hid_channels=(8,))]


def cnn_reward_net_inputs(kw):
    """Spaces and seeded `predict_processed` arguments (7 uint8 frames) for one `CnnRewardNet` variant."""
    from imitation_amd import spaces

    shape = (12, 10, 3) if kw.get("hwc_format", True) else (3, 12, 10)
    rng = np.random.default_rng(0)
    obs = rng.integers(0, 256, (7, *shape), dtype=np.uint8)
    nxt = rng.integers(0, 256, (7, *shape), dtype=np.uint8)
    acts, dones = rng.integers(0, 5, 7), rng.random(7) < 0.5
    return spaces.Box(0, 255, shape, np.uint8), spaces.Discrete(5), (obs, acts, nxt, dones)


@pytest.mark.parametrize("kw", CNN_REWARD_NET_KWS)
def test_cnn_reward_net_bit_identical_to_live_reference(kw):
    """`CnnRewardNet` / `build_cnn` (rewards/reward_nets.py:460-610, util/networks.py:286-357): same parameters
    from the same seed, same forward values, same `predict_processed` on uint8 frames, same errors. Against the
    reference's own net where it is present; elsewhere against what it produced (tests/golden/
    cnn_reward_net_variants.json: parameter digests, bit for bit; predictions within the golden tolerance)."""
    from imitation_amd import spaces
    from oracle import imitation_restated as o

    osp, asp, args = cnn_reward_net_inputs(kw)
    th.manual_seed(3)
    b = o.CnnRewardNet(osp, asp, **kw)
    sb_ = b.state_dict()
    nets = [o.CnnRewardNet]
    if ref_shim.reference_available():
        ref_shim.install()
        from imitation.rewards import reward_nets as rrn

        th.manual_seed(3)
        a = rrn.CnnRewardNet(osp, asp, **kw)
        sa = a.state_dict()
        assert list(sa) == list(sb_) and all(th.equal(sa[k], sb_[k]) for k in sa)
        assert np.array_equal(a.predict_processed(*args), b.predict_processed(*args))
        nets.insert(0, rrn.CnnRewardNet)
    else:
        with open(os.path.join(GOLDEN, "cnn_reward_net_variants.json")) as f:
            gold = json.load(f)[CNN_REWARD_NET_KWS.index(kw)]
        assert gold["kw"] == {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}
        assert {k: harness.array_digest(v.numpy()) for k, v in sb_.items()} == gold["state_dict"]
        assert list(sb_) == list(gold["state_dict"])
        got = np.asarray(b.predict_processed(*args))
        assert got.dtype.str == gold["rews_dtype"]
        np.testing.assert_allclose(got, np.asarray(gold["rews"], dtype=got.dtype), rtol=1e-5, atol=1e-6)
    for net in nets:
        with pytest.raises(ValueError, match="current or next state"):
            net(osp, asp, use_state=False, use_next_state=False)
        with pytest.raises(ValueError, match="to be images"):
            net(spaces.Box(-1, 1, (4,), np.float32), asp)
        with pytest.raises(ValueError, match="Discrete action"):
            net(osp, spaces.Box(-1, 1, (2,), np.float32))


def test_cnn_reward_net_matches_golden():
    """The oracle's `CnnRewardNet` with the reference's parameters reproduces the reference's predictions
    (tests/golden/cnn_reward_net.npz, generated by the reference itself)."""
    from imitation_amd import spaces

    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "cnn_reward_net.npz")))
    net = o.CnnRewardNet(spaces.Box(0, 255, (12, 10, 3), np.uint8), spaces.Discrete(5), use_next_state=True,
                         use_done=True)
    net.load_state_dict({k[3:]: th.as_tensor(v) for k, v in g.items() if k.startswith("sd/")})
    got = net.predict_processed(g["obs"], g["acts"], g["next_obs"], g["dones"])
    np.testing.assert_allclose(got, g["rews"], rtol=1e-5, atol=1e-6)


def _linear_schedule(initial: float):
    """`imitation.util.util` / rl-zoo style linear schedule: lr = progress_remaining * initial."""
    return lambda progress: progress * initial


def test_sb3_bookkeeping_matches_the_fixture_zip():
    """[SB3 OnPolicyAlgorithm.learn / PPO.train] bookkeeping, pinned to what SB3 2.2.0a3 ITSELF stored in
    `/root/reference/tests/testdata/expert_models/cartpole_0/policies/final/model.zip` (`data`,
    `policy.optimizer.pth`; extracted by `tests/golden/make_golden.py:dump_sb3_fixture_layout`): after
    `learn(100_000)` with `n_steps 32 x n_envs 8`, `batch_size 256`, `n_epochs 20` and a linear learning rate of
    1e-3 the file holds `num_timesteps 100096` (the loop runs whole rollouts past the budget), `_n_updates 7820`
    (+1 per EPOCH), Adam `step 7820` (one per MINIBATCH: 391 rollouts x 20 epochs x 1), progress
    `-0.00096...` (taken after the last rollout, BEFORE `train()`) and a param-group `lr` of `-9.6e-07` (the
    schedule applied through `_update_learning_rate` at the head of `train()`, negative in the overshoot)."""
    from imitation_amd.vec_env import SyntheticVecEnv
    lay = json.load(open(os.path.join(GOLDEN, "sb3_fixture_layout.json")))
    hp, bk = lay["hyperparameter_fields"], lay["bookkeeping"]
    th.manual_seed(0)
    np.random.seed(0)
    threads = th.get_num_threads()
    th.set_num_threads(1)   # 12 512 eight-row forwards + 7 820 256-row steps: thread hand-offs dominate otherwise
    venv = SyntheticVecEnv(num_envs=bk["n_envs"], obs_dim=4, act_dim=1, horizon=50, n_discrete=2, seed=3)
    algo = sb.PPO(sb.ActorCriticPolicy, venv, learning_rate=_linear_schedule(1e-3), n_steps=hp["n_steps"],
                  batch_size=hp["batch_size"], n_epochs=hp["n_epochs"], gamma=hp["gamma"],
                  gae_lambda=hp["gae_lambda"], ent_coef=hp["ent_coef"], vf_coef=hp["vf_coef"],
                  max_grad_norm=hp["max_grad_norm"], seed=0)
    try:
        algo.learn(bk["_total_timesteps"])
    finally:
        th.set_num_threads(threads)
    assert algo.num_timesteps == bk["num_timesteps"] == 100096
    assert algo._total_timesteps == bk["_total_timesteps"]
    assert algo._n_updates == bk["_n_updates"] == 7820
    assert algo._current_progress_remaining == bk["_current_progress_remaining"]   # same float64 expression
    opt = algo.policy.optimizer
    assert sorted({float(s["step"]) for s in opt.state.values()}) == bk["adam_step"] == [7820.0]
    assert opt.param_groups[0]["lr"] == bk["param_group_lr"]
    assert len(opt.state) == lay["optimizer"]["n_params"]
