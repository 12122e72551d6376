"""Reward ensembles and active selection, host side: constructor errors, trainer dispatch, the bag restatement against
torch's own `RandomSampler`, and the NumPy restatements of the moment / uncertainty kernels (`tests/ensemble_ref.py`)
against `np.mean` / `np.var` and against torch on the CPU. What needs a device is in `tests/test_ensemble_kernels_gpu.py`
and `tests/test_preference_ensemble_gpu.py`."""
import numpy as np
import pytest
import torch as th
from torch.utils.data import RandomSampler

import imitation_amd as p
from imitation_amd import preference_comparisons as pc
from tests import ensemble_ref as ref


def _spaces():
    return p.Box(-np.inf, np.inf, (5,), np.float32), p.Box(-1.0, 1.0, (2,), np.float32)


def _member(normalized=True, **kw):
    o, a = _spaces()
    base = p.BasicRewardNet(o, a, **kw)
    return p.NormalizedRewardNet(base, p.RunningNorm) if normalized else base


def _ensemble(M=3, **kw):
    o, a = _spaces()
    return p.RewardEnsemble(o, a, [_member(**kw) for _ in range(M)])


def test_reward_ensemble_constructor_and_plumbing():
    o, a = _spaces()
    with pytest.raises(ValueError, match="Must be at least 2 member in the ensemble."):
        p.RewardEnsemble(o, a, [_member()])
    with pytest.raises(ValueError, match="Must be at least 2 member"):
        p.RewardEnsemble(o, a, [])
    ens = _ensemble(3)
    assert isinstance(ens, p.RewardNetWithVariance) and isinstance(ens, p.RewardNet)
    assert ens.num_members == 3 and len(ens.members) == 3
    with pytest.raises(NotImplementedError):
        ens.forward(None, None, None, None)
    # the reference's state keys: members.{i}.<member key>
    keys = set(ens.state_dict())
    member_keys = set(ens.members[0].state_dict())
    assert "_base.mlp.dense0.weight" in member_keys and "normalize_output_layer.count" in member_keys
    assert keys == {f"members.{i}.{k}" for i in range(3) for k in member_keys}
    assert [k for k, _ in ens.named_parameters()] == [f"members.{i}.{k}" for i in range(3)
                                                      for k, _ in ens.members[i].named_parameters()]
    assert len(list(ens.parameters())) == 3 * 6
    # train / eval recurse
    ens.eval()
    assert not any(m.training or m.base.training or m.base.mlp.training for m in ens.members)
    ens.train()
    assert all(m.training and m.base.training and m.base.mlp.training for m in ens.members)
    # load_state_dict recurses
    other = _ensemble(3)
    other.load_state_dict(ens.state_dict())
    for (k1, v1), (k2, v2) in zip(sorted(ens.state_dict().items()), sorted(other.state_dict().items())):
        assert k1 == k2 and th.equal(v1, v2)


def test_add_std_wrapper_constructor():
    with pytest.raises(TypeError, match="not an instance of RewardNetWithVariance"):
        p.AddSTDRewardWrapper(_member())
    ens = _ensemble(2)
    w = p.AddSTDRewardWrapper(ens, default_alpha=0.5)
    assert w.base is ens and w.default_alpha == 0.5
    assert p.AddSTDRewardWrapper(ens).default_alpha == 0.0
    assert set(w.state_dict()) == {f"_base.{k}" for k in ens.state_dict()}
    assert w.rollout_tail_plan() is None and ens.rollout_tail_plan() is None


def test_preference_model_over_an_ensemble():
    ens = _ensemble(3)
    pm = pc.PreferenceModel(ens, noise_prob=0.1, discount_factor=0.9, threshold=7)
    assert pm.ensemble_model is ens and len(pm.member_pref_models) == 3
    for m, mp in zip(ens.members, pm.member_pref_models):
        assert mp.model is m and mp.ensemble_model is None
        assert (mp.noise_prob, mp.discount_factor, mp.threshold) == (0.1, 0.9, 7)
    w = p.AddSTDRewardWrapper(ens)
    assert pc.PreferenceModel(w).ensemble_model is ens
    with pytest.raises(ValueError, match="RewardEnsemble can only be wrapped by AddSTDRewardWrapper but found "
                                         "NormalizedRewardNet"):
        pc.PreferenceModel(p.NormalizedRewardNet(ens, p.RunningNorm))
    with pytest.raises(ValueError, match="can only be wrapped by AddSTDRewardWrapper"):
        pc.PreferenceModel(p.AddSTDRewardWrapper(p_wrapped_twice(ens)))
    assert pc.PreferenceModel(_member()).ensemble_model is None
    with pytest.raises(NotImplementedError, match="not defined for a reward ensemble"):
        pm.forward([])


class _Variance(p.PredictProcessedWrapper, p.RewardNetWithVariance):
    """A RewardNetWithVariance that is not the ensemble itself (AddSTDRewardWrapper accepts it)."""

    def predict_reward_moments(self, *args, **kwargs):
        return self.base.predict_reward_moments(*args, **kwargs)


def p_wrapped_twice(ens):
    return _Variance(ens)


def test_ensemble_trainer_constructor_and_dispatch():
    rng = np.random.default_rng(0)
    loss = pc.CrossEntropyRewardLoss()
    with pytest.raises(NotImplementedError, match="EnsembleTrainer"):
        pc.EnsembleTrainer()
    with pytest.raises(TypeError, match="PreferenceModel of a RewardEnsemble expected by EnsembleTrainer."):
        pc.EnsembleTrainer(pc.PreferenceModel(_member()), loss, rng)
    pm = pc.PreferenceModel(p.AddSTDRewardWrapper(_ensemble(3)))
    tr = pc._make_reward_trainer(pm, loss, rng, dict(batch_size=6, minibatch_size=3, epochs=2, lr=2e-3))
    assert type(tr) is pc.EnsembleTrainer and len(tr.member_trainers) == 3
    for t, mp in zip(tr.member_trainers, pm.member_pref_models):
        assert type(t) is pc.BasicRewardTrainer and t._preference_model is mp and t.logger is tr.logger
        assert (t.batch_size, t.minibatch_size, t.epochs, t.rng) == (6, 3, 2, rng)
    new_logger = pc.configure_logger()
    tr.logger = new_logger
    assert tr.logger is new_logger and all(t.logger is new_logger for t in tr.member_trainers)
    assert type(pc._make_reward_trainer(pc.PreferenceModel(_member()), loss, rng)) is pc.BasicRewardTrainer
    with pytest.raises(ValueError, match="multiple of minibatch size"):
        pc.EnsembleTrainer(pm, loss, rng, batch_size=8, minibatch_size=3)
    with pytest.raises(NotImplementedError, match="regularizers"):
        pc.EnsembleTrainer(pm, loss, rng, regularizer_factory=lambda **k: None)


def test_active_selection_fragmenter_constructor():
    rng = np.random.default_rng(0)
    base = pc.RandomFragmenter(rng)
    with pytest.raises(NotImplementedError, match="ActiveSelectionFragmenter"):
        pc.ActiveSelectionFragmenter()
    with pytest.raises(ValueError, match="PreferenceModel not wrapped over an ensemble of networks."):
        pc.ActiveSelectionFragmenter(pc.PreferenceModel(_member()), base, 2.0)
    pm = pc.PreferenceModel(_ensemble(2))
    with pytest.raises(ValueError, match="`uncertainty_on` should be from `logit`, `probability`, or `label`"):
        pc.ActiveSelectionFragmenter(pm, base, 2.0, uncertainty_on="entropy")
    for mode in ("logit", "probability", "label"):
        f = pc.ActiveSelectionFragmenter(pm, base, 2.0, uncertainty_on=mode)
        assert f.uncertainty_on == mode and f.base_fragmenter is base and f.fragment_sample_factor == 2.0
        assert f.last_var_estimates is None and f.last_selected is None


def test_foreign_classes_with_the_names_keep_the_refusal():
    class AddSTDRewardWrapper:
        def __init__(self, base):
            self.base = base

    class RewardEnsemble:
        pass

    with pytest.raises(NotImplementedError, match="ensembles of other packages' classes"):
        pc.PreferenceModel(RewardEnsemble())
    with pytest.raises(NotImplementedError, match="ensembles of other packages' classes"):
        pc.PreferenceModel(AddSTDRewardWrapper(RewardEnsemble()))


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("N", [5, 32, 33, 70])
def test_bag_indices_are_the_random_samplers(N, seed):
    s1 = pc.make_seeds(np.random.default_rng(seed))
    s2 = int(np.random.default_rng(seed).integers(0, (1 << 31) - 1, (1,))[0])
    assert s1 == s2 and 0 <= s1 < (1 << 31) - 1
    sampler = RandomSampler(range(N), replacement=True, num_samples=N, generator=th.Generator().manual_seed(s1))
    g = th.Generator().manual_seed(s1)
    for _ in range(3):   # one bag per member, from one generator
        want = list(sampler)
        got = pc.bag_indices(N, g)
        assert got == [int(i) for i in want] and len(got) == N


def test_preference_bag_is_a_view():
    ds = pc.PreferenceDataset()
    frag = lambda v: pc.TrajectoryWithRew(obs=np.full((3, 5), v, np.float32), acts=np.zeros((2, 2), np.float32), infos=None,
                                          terminal=False, rews=np.zeros(2, np.float32))
    ds.push([(frag(i), frag(-i)) for i in range(4)], np.array([0, 1, 0.5, 1], np.float32))
    bag = pc.PreferenceBag(ds, np.array([3, 3, 0]))
    assert len(bag) == 3 and bag.dataset is ds
    (f1, f2), y = bag[1]
    assert f1 is ds.fragments1[3] and f2 is ds.fragments2[3] and y == 1


@pytest.mark.parametrize("M", [2, 3, 5, 7])
@pytest.mark.parametrize("alpha", [0.0, -1.5, 2.0])
def test_moments_restatement_is_numpys_below_8_members(M, alpha):
    r = np.random.default_rng(M)
    x = (r.normal(size=(M, 333)) * 3 + 1).astype(np.float32)
    mean, var, bound = ref.moments_f32(x, alpha)
    xt = np.ascontiguousarray(x.T)                      # predict_processed_all's [batch, M]
    np.testing.assert_array_equal(mean, xt.mean(-1))
    np.testing.assert_array_equal(var, xt.var(-1, ddof=1))
    np.testing.assert_array_equal(bound, xt.mean(-1) + alpha * np.sqrt(xt.var(-1, ddof=1)))
    assert mean.dtype == var.dtype == bound.dtype == np.float32
    t = th.from_numpy(xt)
    np.testing.assert_allclose(mean, t.mean(-1).numpy(), rtol=0, atol=4e-7 * np.abs(x).max())
    np.testing.assert_allclose(var, t.var(-1, unbiased=True).numpy(), rtol=2e-5)


def test_moments_restatement_at_8_members_is_within_4_ulp_of_numpys():
    """From 8 members on NumPy's reduction over the last axis is unrolled eight wide: another order, a few ulp apart."""
    r = np.random.default_rng(8)
    for M in (8, 16):
        x = (r.normal(size=(M, 500)) + 2).astype(np.float32)
        mean, var, _ = ref.moments_f32(x, 0.0)
        xt = np.ascontiguousarray(x.T)
        assert ref.ulp_distance(mean, xt.mean(-1)).max() <= 4
        np.testing.assert_allclose(var, xt.var(-1, ddof=1), rtol=1e-5)


def _torch_estimate(x, P, L, mode, gamma, noise, threshold):
    """`ActiveSelectionFragmenter.variance_estimate` with the reference's torch / NumPy operations, float32 on the CPU."""
    M = x.shape[0]
    out = np.zeros(P)
    for pi in range(P):
        rews1 = th.from_numpy(x[:, 2 * pi * L:2 * pi * L + L].T.copy())
        rews2 = th.from_numpy(x[:, 2 * pi * L + L:2 * pi * L + 2 * L].T.copy())
        if mode == "logit":
            out[pi] = (rews1.sum(0) - rews2.sum(0)).var().item()
            continue
        if gamma == 1:
            diff = (rews2 - rews1).sum(axis=0)
        else:
            diff = ((gamma ** th.arange(L)).reshape(-1, 1) * (rews2 - rews1)).sum(axis=0)
        diff = th.clip(diff, -threshold, threshold)
        probs = (noise * 0.5 + (1 - noise) * (1 / (1 + diff.exp()))).numpy()
        assert probs.shape == (M,)
        if mode == "probability":
            out[pi] = probs.var()
        else:
            pe = (probs > 0.5).astype(np.float32).mean()
            out[pi] = pe * (1 - pe)
    return out


@pytest.mark.parametrize("gamma,noise", [(1.0, 0.0), (0.9, 0.1)])
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("P,L,M", [(1, 1, 2), (7, 5, 3), (24, 100, 5)])
def test_uncertainty_restatement_against_torch_and_float64(P, L, M, mode, gamma, noise):
    r = np.random.default_rng(1000 * P + M)
    x = (r.normal(size=(M, 2 * P * L)) * (3.0 / np.sqrt(L))).astype(np.float32)
    f32 = ref.pair_uncertainty_f32(x, P, L, mode, gamma, noise, 2.0)
    f64 = ref.pair_uncertainty_f64(x, P, L, mode, gamma, noise, 2.0)
    tor = _torch_estimate(x, P, L, mode, gamma, noise, 2.0)
    assert f32.dtype == np.float32 and f32.shape == (P,)
    if mode == "label":
        probs = ref.member_probabilities_f64(x, P, L, gamma, noise, 2.0)
        decisive = np.abs(probs - 0.5).min(1) > 1e-4
        assert decisive.any()
        np.testing.assert_array_equal(f32[decisive], f64[decisive].astype(np.float32))
        np.testing.assert_array_equal(f32[decisive], tor[decisive].astype(np.float32))
    else:
        assert ref.rel(f32, f64) < 2e-5 and ref.rel(tor, f64) < 2e-5
    if P > 1 and mode != "label":   # the clip is hit somewhere, and not everywhere
        w = gamma ** np.arange(L)
        d = ((x.reshape(M, P, 2, L)[:, :, 1] - x.reshape(M, P, 2, L)[:, :, 0]) * w).sum(-1)
        assert (np.abs(d) > 2.0).any() and (np.abs(d) < 2.0).any()


def test_norm_sequential_restatement_is_the_per_step_formula():
    r = np.random.default_rng(3)
    raw = r.normal(size=3 * 7)
    out, mean, var, count = ref.norm_sequential(np.float64, raw, 3, 7, 1e-5, True, 0.0, 1.0, 0)
    np.testing.assert_allclose(out[:7], raw[:7] / np.sqrt(1 + 1e-5))
    assert count == 21
    np.testing.assert_allclose(mean, raw.mean())
    np.testing.assert_allclose(var, raw.var())
    out2, m2, v2, c2 = ref.norm_sequential(np.float64, raw, 3, 7, 1e-5, False, 0.5, 2.0, 9)
    np.testing.assert_allclose(out2, (raw - 0.5) / np.sqrt(2 + 1e-5))
    assert (m2, v2, c2) == (0.5, 2.0, 9)


@pytest.mark.parametrize("name", ["preference_ensemble_logit", "preference_ensemble_label"])
def test_active_selection_restatement_reproduces_the_references_goldens(name):
    """`ensemble_ref.active_selection_f64` from the reference's member states before each fragmenter call gives the
    reference's float64 estimates, selections and statistics: the device tests propagate parameter deviations with it."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    trajs = [(z[f"traj{k}_obs"], z[f"traj{k}_acts"]) for k in range(cfg["n_traj"])]
    for i in range(int(z["n_iters"])):
        prefix = f"it{i - 1}_param/" if i else "init/"
        state = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
        est, stats, counts = ref.active_selection_f64(state, trajs, z[f"it{i}_picks"], cfg["members"], cfg["frag"],
                                                      cfg["uncertainty_on"], cfg["gamma"], cfg["noise"],
                                                      n_onehot=cfg["act_dim"] if cfg["discrete"] else 0)
        np.testing.assert_allclose(est, z[f"it{i}_estimates"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(stats, z[f"it{i}_frag_stats"], rtol=1e-9, atol=1e-12)
        assert np.array_equal(counts, z[f"it{i}_frag_counts"])
        assert np.array_equal(np.argsort(est)[::-1][:int(z["schedule"][i])], z[f"it{i}_selected"])
