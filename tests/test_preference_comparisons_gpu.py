"""Preference comparisons on the MI355X: the fused preference loss (`ia_pref_loss`) against a float64 autograd
restatement, AdamW against torch's, `PreferenceComparisons.train` against the reference's goldens
(`tests/golden/preference_*.npz`) on the product and the `nn.Module` paths, the one-call and the host-stepped reward
training, and the agent's rollout relabelling through PPO's device path."""
import json
import os

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import data_types as dt
from imitation_amd import modules
from imitation_amd import preference_comparisons as pc
from imitation_amd.vec_env import SyntheticVecEnv

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["preference_basic_rn", "preference_plain_disc_noise_accum", "preference_normalized_queue",
         "preference_discrete", "preference_default_sizes"]


# ---------------------------------------------------------------------------------------------- kernel (a)

def _ref_loss(r, off, y, gt, gamma, noise, thr):
    """Restatement of PreferenceModel.probability + CrossEntropyRewardLoss (torch autograd, on the CPU) in the dtype of
    `r`: float64 for the gradients, float32 -- the reference's own precision -- for values that saturate (a
    probability that rounds to 0 or 1 in float32 meets the -100 log clamp, in float64 it does not)."""
    r = r.detach().cpu().clone().requires_grad_(True)
    gt = gt.detach().cpu() if gt is not None else None
    y = y.detach().cpu()
    probs, gt_probs = [], []
    for k in range(len(off) - 1):
        L = off[k + 1] - off[k]
        a, b = 2 * off[k], 2 * off[k] + L
        for src, out in ((r, probs), (gt, gt_probs)):
            if src is None:
                continue
            r1, r2 = src[a:a + L], src[b:b + L]
            if gamma == 1:
                diff = (r2 - r1).sum()
            else:
                diff = ((gamma ** th.arange(L, dtype=r.dtype)) * (r2 - r1)).sum()
            diff = th.clip(diff, -thr, thr)
            out.append(noise * 0.5 + (1 - noise) * (1 / (1 + diff.exp())))
    probs = th.stack(probs)
    yy = y.to(r.dtype)
    loss = th.nn.functional.binary_cross_entropy(probs, yy)
    loss.backward()
    acc = ((probs > 0.5) == (yy > 0.5)).double().mean()
    gtl = th.nn.functional.binary_cross_entropy(th.stack(gt_probs), yy) if gt is not None else None
    return loss.item(), acc.item(), (gtl.item() if gtl is not None else 0.0), r.grad, probs.detach()


@pytest.mark.parametrize("lens", [[1, 1, 1], [5] * 4, [100] * 8, [257, 257], [1, 5, 100, 257, 3]])
@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("noise", [0.0, 0.1])
def test_pref_loss_kernel_matches_autograd(lens, gamma, noise):
    g = th.Generator().manual_seed(len(lens) * 7 + int(gamma * 100) + int(noise * 10))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    R = 2 * int(off[-1])
    r = (th.randn(R, generator=g) * 0.3).cuda()
    gt = th.randn(R, generator=g).cuda()
    y = th.tensor(([0.0, 0.5, 1.0] * 4)[:len(lens)]).cuda()
    off_d = th.as_tensor(off.astype(np.int32)).cuda()
    st, d, pr = th.ops.imitation_amd.preference_loss(r, off_d, y, gt, gamma, noise, 50.0)
    rl, ra, rg, _, rprobs = _ref_loss(r, off, y, gt, gamma, noise, 50.0)
    _, _, _, rgrad, _ = _ref_loss(r.double(), off, y.double(), gt.double(), gamma, noise, 50.0)
    s = st.cpu().numpy()
    np.testing.assert_allclose(s[0], rl, rtol=2e-5, atol=1e-6)
    assert s[1] == ra
    np.testing.assert_allclose(s[2], rg, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(pr.cpu().numpy(), rprobs.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(d.cpu().numpy(), rgrad.numpy(), rtol=1e-4, atol=1e-8)


def test_pref_loss_clip_and_log_clamp():
    # pair 0: returns difference 200 beyond threshold 50 (zero gradient); pair 1: -200 (zero gradient);
    # threshold 1e4 on pair 2 -> p rounds to exactly 0 / 1 in float32: the -100 log clamp
    r = th.zeros(8).cuda()
    r[1] = 200.0    # pair 0 fragment 2 row (L = 1): diff = +200
    r[2] = 200.0    # pair 1 fragment 1 row: diff = -200
    off = th.tensor([0, 1, 2], dtype=th.int32).cuda()
    y = th.tensor([1.0, 0.0]).cuda()
    st, d, pr = th.ops.imitation_amd.preference_loss(r[:4].contiguous(), off, y, None, 1.0, 0.0, 50.0)
    assert th.all(d == 0)
    rl, ra, _, _, _ = _ref_loss(r[:4], [0, 1, 2], y, None, 1.0, 0.0, 50.0)
    np.testing.assert_allclose(st[0].item(), rl, rtol=1e-5)
    st, d, pr = th.ops.imitation_amd.preference_loss(r[:4].contiguous(), off, y, None, 1.0, 0.0, 1e4)
    assert pr[0].item() == 0.0 and pr[1].item() == 1.0
    np.testing.assert_allclose(st[0].item(), 100.0, rtol=1e-6)   # both pairs hit log(0) -> clamp at -100
    assert st[1].item() == 0.0
    # exp(200) overflows float32: torch's backward gives 0 * inf = NaN there, and so does the kernel
    _, _, _, rgrad, _ = _ref_loss(r[:4], [0, 1, 2], y, None, 1.0, 0.0, 1e4)
    np.testing.assert_array_equal(th.isnan(d).cpu().numpy(), th.isnan(rgrad).numpy())


def test_adamw_matches_torch():
    g = th.Generator().manual_seed(0)
    p0 = th.randn(1000, generator=g)
    grads = [th.randn(1000, generator=g) for _ in range(5)]
    ref = p0.clone().requires_grad_(True)
    opt = th.optim.AdamW([ref], lr=1e-3)
    flat, grad = p0.clone().cuda(), th.zeros(1000).cuda()
    mine = p.networks.HipAdam(flat, grad, lr=1e-3, weight_decay=0.01, decoupled=True)
    for gr in grads:
        ref.grad = gr.clone()
        opt.step()
        grad.copy_(gr)
        mine.step()
    np.testing.assert_allclose(flat.cpu().numpy(), ref.detach().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(mine.exp_avg_sq.cpu().numpy(), opt.state[ref]["exp_avg_sq"].numpy(), rtol=1e-4)
    # the default Adam (L2-coupled decay) is untouched by the new flag
    assert p.networks.HipAdam(flat, grad).decoupled is False


# ---------------------------------------------------------------------------------------------- end to end

def _load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    trajs = [dt.TrajectoryWithRew(obs=z[f"traj{k}_obs"], acts=z[f"traj{k}_acts"], rews=z[f"traj{k}_rews"], infos=None,
                                  terminal=True) for k in range(cfg["n_traj"])]
    return z, cfg, trajs


def _run(name, module_net=False, host_stepped=False):
    z, cfg, trajs = _load(name)
    obs_space = p.Box(-np.inf, np.inf, (cfg["obs_dim"],), np.float32)
    act_space = p.Discrete(cfg["act_dim"]) if cfg["discrete"] else p.Box(-1.0, 1.0, (cfg["act_dim"],), np.float32)
    th.manual_seed(cfg["seed"])
    if module_net:
        kw = dict(normalize_input_layer=modules.RunningNorm) if cfg["norm"] else {}
        net = modules.BasicRewardNet(obs_space, act_space, **kw).cuda()
        model = modules.NormalizedRewardNet(net, modules.RunningNorm).cuda() if cfg["wrap"] else net
    else:
        kw = dict(normalize_input_layer=p.RunningNorm) if cfg["norm"] else {}
        net = p.BasicRewardNet(obs_space, act_space, **kw).to("cuda")
        model = p.NormalizedRewardNet(net, p.RunningNorm).to("cuda") if cfg["wrap"] else net
    rng = np.random.default_rng(cfg["seed"])
    logger = p.configure_logger(format_strs=[])
    gen = pc.TrajectoryDataset(trajs, rng=rng, custom_logger=logger)
    pm = pc.PreferenceModel(model, noise_prob=cfg["noise"], discount_factor=cfg["gamma"])
    trainer = pc.BasicRewardTrainer(pm, pc.CrossEntropyRewardLoss(), rng=rng, batch_size=cfg["batch"],
                                    minibatch_size=cfg["mb"], epochs=cfg["epochs"], custom_logger=logger)
    trainer.host_stepped = host_stepped
    got = {"params": [], "adam": [], "dumps": []}
    orig_train, orig_dump = trainer.train, logger.dump

    def train_call(dataset, epoch_multiplier=1.0):
        orig_train(dataset, epoch_multiplier)
        got["params"].append({k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()})
        if module_net:
            ps = list(trainer.optim.param_groups[0]["params"])
            st = trainer.optim.state
            got["adam"].append({"step": st[ps[0]]["step"],
                                "exp_avg": th.cat([st[q]["exp_avg"].reshape(-1) for q in ps]).cpu().numpy(),
                                "exp_avg_sq": th.cat([st[q]["exp_avg_sq"].reshape(-1) for q in ps]).cpu().numpy()})
        else:
            o = trainer.optim
            got["adam"].append({"step": o.step_count, "exp_avg": o.exp_avg.cpu().numpy().copy(),
                                "exp_avg_sq": o.exp_avg_sq.cpu().numpy().copy()})

    def dump(step=0):
        got["dumps"].append({k: float(v) for k, v in logger.default_logger.name_to_value.items()})
        orig_dump(step)

    trainer.train, logger.dump = train_call, dump
    algo = pc.PreferenceComparisons(gen, model, num_iterations=cfg["iters"],
                                    fragmenter=pc.RandomFragmenter(rng=rng, custom_logger=logger),
                                    preference_gatherer=pc.SyntheticGatherer(rng=rng, discount_factor=cfg["gamma"],
                                                                             custom_logger=logger),
                                    reward_trainer=trainer, comparison_queue_size=cfg["queue"],
                                    fragment_length=cfg["frag"], initial_epoch_multiplier=cfg["init_mult"],
                                    custom_logger=logger)
    result = algo.train(total_timesteps=0, total_comparisons=cfg["comparisons"])
    return z, got, result


ATOL, RTOL = 5e-5, 2e-4
LR = 1e-3


def _close(x, y, what, worst, steps=None, atol=ATOL, rtol=RTOL, frac=0.15):
    """x within atol + rtol |y| of y. `steps` (parameters after that many AdamW steps): at most 10 % of the entries of an
    array may miss, by no more than 2 * steps * lr. Adam moves a weight by about lr * g / |g| per step whatever |g| is,
    so an entry whose gradient is at rounding level takes its steps in a direction set by rounding. Bias gradients
    nearly cancel between a pair's two fragments (the final bias at discount 1 cancels exactly). Observed: 4 of the 32
    second-layer biases off by 3e-4 after 6 steps, the same entries on the product and the module path. After the first
    reward training those steps reach every later gradient: `frac=1` keeps only the bound."""
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    assert x.shape == y.shape, what
    err = np.abs(x - y)
    miss = err > atol + rtol * np.abs(y)
    worst[what] = float(err.max()) if x.size else 0.0
    if steps is None or not miss.any():
        assert not miss.any(), (what, float(err.max()))
        return
    assert miss.mean() <= frac or miss.sum() <= 1, (what, int(miss.sum()), x.size)
    assert err.max() <= 2 * steps * LR, (what, float(err.max()), steps)


def _check(z, got, result):
    worst = {}
    n = int(z["n_iters"])
    assert len(got["params"]) == n and len(got["dumps"]) == n
    for i in range(n):
        steps = int(z[f"it{i}_adam/step"])
        for key in [k for k in z.files if k.startswith(f"it{i}_param/")]:
            name = key.split("/", 1)[1]
            gold = z[key]
            x = got["params"][i][name]
            if gold.dtype.kind in "iu":
                assert np.array_equal(np.asarray(x), gold), (i, name)   # RunningNorm count: exact
            elif "normalize_" in name:
                _close(x, gold, f"it{i} {name}", worst)   # statistics: no optimiser in between
            else:
                _close(x, gold, f"it{i} {name}", worst, steps=steps, frac=0.15 if i == 0 else 1.0)
        a = got["adam"][i]
        assert int(a["step"]) == steps
        if i == 0:
            _close(a["exp_avg"], z[f"it{i}_adam/exp_avg"], f"it{i} exp_avg", worst, steps=steps)
        else:
            # later gradients are taken at parameters that carry the rounding-directed steps above: the first moment
            # follows them within a few percent of its scale
            gold = z[f"it{i}_adam/exp_avg"]
            err = np.abs(a["exp_avg"] - gold).max()
            worst[f"it{i} exp_avg"] = float(err)
            assert err <= 0.05 * np.abs(gold).max() + 1e-5, (i, float(err), float(np.abs(gold).max()))
        keys = list(z[f"it{i}_log_keys"])
        assert sorted(got["dumps"][i]) == keys, i
        _close([got["dumps"][i][k] for k in keys], z[f"it{i}_log_vals"], f"it{i} log", worst, atol=1e-4, rtol=1e-3)
    _close([result["reward_loss"], result["reward_accuracy"]], z["result"], "result", worst, atol=1e-4, rtol=1e-3)
    print("worst |deviation|:", max(worst.values()), max(worst, key=worst.get))


@pytest.mark.parametrize("name", CASES)
def test_preference_comparisons_matches_reference(name):
    _check(*_run(name))


@pytest.mark.parametrize("name", ["preference_basic_rn", "preference_plain_disc_noise_accum",
                                  "preference_default_sizes"])
def test_module_net_path_matches_reference(name):
    _check(*_run(name, module_net=True))


def test_one_call_and_host_stepped_are_bit_identical():
    _, a, ra = _run("preference_plain_disc_noise_accum")
    _, b, rb = _run("preference_plain_disc_noise_accum", host_stepped=True)
    assert ra == rb
    for pa, pb in zip(a["params"], b["params"]):
        for k in pa:
            assert np.array_equal(pa[k], pb[k]), k
    assert a["dumps"] == b["dumps"]


def test_product_and_module_paths_agree():
    za, a, _ = _run("preference_basic_rn")
    zb, b, _ = _run("preference_basic_rn", module_net=True)
    worst = {}
    steps = int(za["it0_adam/step"])
    for k, v in a["params"][0].items():
        if v.dtype.kind in "iu":
            assert np.array_equal(v, b["params"][0][k])
        else:
            _close(v, b["params"][0][k], k, worst, steps=steps)
    print("worst |deviation| after the first reward training:", max(worst.values()), max(worst, key=worst.get))


def test_shaped_net_trains_and_norm_variants_rejected():
    z, cfg, trajs = _load("preference_plain_disc_noise_accum")
    obs_space = p.Box(-np.inf, np.inf, (cfg["obs_dim"],), np.float32)
    act_space = p.Box(-1.0, 1.0, (cfg["act_dim"],), np.float32)
    th.manual_seed(0)
    net = p.BasicShapedRewardNet(obs_space, act_space).to("cuda")
    rng = np.random.default_rng(0)
    algo = pc.PreferenceComparisons(pc.TrajectoryDataset(trajs, rng), net, num_iterations=1, fragment_length=5, rng=rng,
                                    initial_epoch_multiplier=2, custom_logger=p.configure_logger(format_strs=[]))
    before = net._store.flat.clone()
    out = algo.train(total_timesteps=0, total_comparisons=10)
    assert np.isfinite(out["reward_loss"]) and not th.equal(before, net._store.flat)
    ema = p.BasicRewardNet(obs_space, act_space, normalize_input_layer=p.EMANorm).to("cuda")
    algo = pc.PreferenceComparisons(pc.TrajectoryDataset(trajs, rng), ema, num_iterations=1, fragment_length=5, rng=rng,
                                    custom_logger=p.configure_logger(format_strs=[]))
    with pytest.raises(NotImplementedError, match="EMANorm"):
        algo.train(total_timesteps=0, total_comparisons=10)


def test_agent_trainer_relabels_on_device(monkeypatch):
    th.manual_seed(0)
    venv = SyntheticVecEnv(num_envs=8, obs_dim=6, act_dim=2, horizon=20, seed=0)
    algo = p.PPO(p.FeedForward32Policy, venv, n_steps=16, batch_size=64, n_epochs=1, seed=0, device="cuda")
    net = p.BasicRewardNet(venv.observation_space, venv.action_space).to("cuda")
    calls = {"n": 0}
    orig = p.BasicRewardNet.predict

    def counting(self, *a, **k):
        calls["n"] += 1
        return orig(self, *a, **k)

    monkeypatch.setattr(p.BasicRewardNet, "predict", counting)
    gen = pc.AgentTrainer(algo, net, venv, rng=np.random.default_rng(0),
                          custom_logger=p.configure_logger(format_strs=[]))
    assert gen.reward_venv_wrapper.reward_fn.__self__ is net
    gen.train(steps=8 * 16 * 2)
    assert calls["n"] == 0   # two rollouts of 16 steps relabelled without a per-step predict call
    trajs = gen.sample(100)
    assert sum(len(t) for t in trajs) >= 100
