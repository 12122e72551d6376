"""Reward ensembles and active selection on the MI355X against the reference's own classes
(`tests/golden/make_golden_preference_ensemble.py`: `ensemble_moments.npz`, `preference_ensemble_*.npz`), the rollout
(bulk) path against the per-step device calls bit for bit, and an `AgentTrainer` + `PPO` run under `AddSTDRewardWrapper`.

`ensemble_moments`: relative L2 against the float64 run within 8 x the float32 run's own deviation (`dref/`), counts exact.
Training runs: picks, bags, selected indices, counts and key lists exact; floats by the rules of
`tests/test_preference_comparisons_gpu.py` (`_close`). What those rules mean for this feature's quantities:

* Parameters carry `_close`'s `steps` allowance: an entry whose gradient cancels to rounding level is stepped by AdamW in a
  direction set by rounding, up to `2 * steps * lr`. Measured here after the first training (2 steps): every weight within
  1e-7, 1 - 3 of the 32 second-layer biases off by up to 8e-4, the final bias (whose gradient cancels exactly between a
  pair's fragments at any discount) by up to 1.6e-3; after 8 steps the final bias by up to 5.1e-3.
* A member's output statistics and the estimates are functions of its parameters, so after the first training a
  free-running run's values carry the run's own parameter deviation: the running mean of a member's outputs moves one for
  one with its final bias, and a `logit` estimate -- a variance over members of sums of outputs divided by the outputs'
  standard deviation (0.06 - 0.08 here) -- moves with the second-layer biases. That deviation is not allowed for by a wider
  tolerance but PROPAGATED: `ensemble_ref.active_selection_f64` (float64, NumPy; `tests/test_reward_ensemble.py` shows that
  from the reference's states it reproduces the goldens to 1e-9) scores the call once from this run's member states before
  the call and once from the reference's, and the difference of the two is taken off the device's value before the plain
  rule is applied: estimates atol 1e-4 + rtol 1e-3 (the log values' rule), statistics atol 5e-5 + rtol 2e-4 (`_check`'s rule
  for `normalize_` keys), in every iteration, for every pair and member. An estimate wrong by more than 0.1 %, or a
  statistics update wrong by more than 2e-4, beyond what the run's own parameters explain, fails (measured rest: 1.2e-5 on
  the estimates). Directly against the
  goldens the estimates are also held to `_check`'s rule for quantities downstream of earlier trainings (`exp_avg`):
  5 % of the array's scale, 2.3 - 2.4 here -- loose (the measured deviation is 0.06 on values of 0.5 - 47, 1.9 %; the
  smallest gaps between neighbouring estimates are 0.026 and 0.047), which is why the propagated rule is the one that
  constrains. Before any training both plain rules hold directly (measured: estimates 1.4e-5 on values up to 38,
  statistics 5e-9). The selected indices are exact in every iteration.
* Every iteration is ALSO scored on the device from the reference's own member states (`_teacher_forced`), where the plain
  rules hold for every pair against the goldens directly. `label` estimates are exact throughout."""
import json
import os

import numpy as np
import pytest
import torch as th

import imitation_amd as p
from imitation_amd import data_types as dt
from imitation_amd import preference_comparisons as pc
from imitation_amd.networks import TransitionTable
from imitation_amd.vec_env import SyntheticVecEnv
from tests.ensemble_ref import active_selection_f64, rel
from tests.preference_ensemble_golden import MOMENTS, MOMENTS_CASES, PROBABILITY_CASE, RUNS, moments_inputs
from tests.test_preference_comparisons_gpu import _close

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS32 = float(np.finfo(np.float32).eps)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def make_ensemble(obs_space, act_space, n_members, seed):
    """The reference's `reward_ensemble` members, drawn in the reference's order from `seed`."""
    th.manual_seed(seed)
    members = [p.NormalizedRewardNet(p.BasicRewardNet(obs_space, act_space), p.RunningNorm) for _ in range(n_members)]
    return p.RewardEnsemble(obs_space, act_space, members).to("cuda")


def check_init(ens, z, prefix):
    sd = ens.state_dict()
    keys = [k[len(prefix):] for k in z.files if k.startswith(prefix)]
    assert sorted(sd) == sorted(keys)                       # the reference's own keys
    for k in keys:
        assert np.array_equal(sd[k].cpu().numpy(), z[prefix + k]), k


def output_stats(ens):
    norms = [m.normalize_output_layer for m in ens.members]
    return (np.array([[n.running_mean.item(), n.running_var.item()] for n in norms], np.float32),
            np.array([int(n.count.item()) for n in norms], np.int64))


def table_of(inputs, discrete):
    s, a, ns, d = (np.concatenate([c[k] for c in inputs]) for k in range(4))
    acts = th.as_tensor(a.astype(np.int64) if discrete else a.astype(np.float32)).cuda()
    return TransitionTable(th.as_tensor(s).cuda(), acts, th.as_tensor(ns).cuda(), th.as_tensor(d.astype(np.uint8)).cuda(),
                           discrete)


def within(got, z, case, key, worst):
    f64, dref = z[f"{case}/f64/{key}"], float(z[f"{case}/dref/{key}"])
    d = rel(got, f64)
    worst[key] = (d, dref)
    assert np.shape(got) == f64.shape and d <= (8 * dref if dref > 0 else EPS32), (key, d, dref)


# ---------------------------------------------------------------------------------------------- the reward nets alone

def _moments_spaces(discrete):
    cfg = MOMENTS
    return (p.Box(-np.inf, np.inf, (cfg["obs_dim"],), np.float32),
            p.Discrete(cfg["n_discrete"]) if discrete else p.Box(-1.0, 1.0, (cfg["act_dim"],), np.float32))


@pytest.mark.parametrize("case", MOMENTS_CASES)
def test_ensemble_moments_match_the_reference_and_the_rollout_path_matches_the_calls(case):
    z = np.load(os.path.join(GOLDEN, "ensemble_moments.npz"))
    cfg, discrete = MOMENTS, case == "discrete"
    assert json.loads(str(z["cfg"])) == cfg
    ens = make_ensemble(*_moments_spaces(discrete), cfg["members"], cfg["seed"])
    check_init(ens, z, f"{case}/init/")
    net = p.AddSTDRewardWrapper(ens, default_alpha=cfg["alpha"])
    inputs = moments_inputs(discrete)
    worst, bounds = {}, []
    for c in range(cfg["calls"]):
        bounds.append(net.predict_processed(*inputs[c]))
        assert bounds[-1].dtype == np.float32 and bounds[-1].shape == (cfg["rows"],)
        within(bounds[-1], z, case, f"call{c}/bound", worst)
        stats, counts = output_stats(ens)
        within(stats, z, case, f"call{c}/stats", worst)
        assert np.array_equal(counts, z[f"{case}/call{c}/counts"])
    allm = ens.predict_processed_all(*inputs[-1], update_stats=False)
    assert allm.shape == (cfg["rows"], cfg["members"]) and allm.dtype == np.float32
    within(allm, z, case, "all", worst)
    mean, var = ens.predict_reward_moments(*inputs[-1], update_stats=False)
    within(mean, z, case, "all_mean", worst)
    within(var, z, case, "all_var", worst)
    # NumPy's arithmetic on the members' matrix, bit for bit
    assert np.array_equal(bits(mean), bits(allm.mean(-1))) and np.array_equal(bits(var), bits(allm.var(-1, ddof=1)))
    assert np.array_equal(bits(ens.predict(*inputs[-1], update_stats=False)), bits(mean))
    assert np.array_equal(bits(ens.predict_processed(*inputs[-1], update_stats=False)), bits(mean))
    stats, counts = output_stats(ens)                       # update_stats=False moved nothing
    within(stats, z, case, "final/stats", worst)
    assert np.array_equal(counts, z[f"{case}/final/counts"]) and np.array_equal(counts, z[f"{case}/call2/counts"])
    print(case, {k: f"{d:.2e} (dref {r:.2e})" for k, (d, r) in worst.items()})
    # the same calls as ONE rollout tile: T = 3 steps of n = 7 rows
    twin = make_ensemble(*_moments_spaces(discrete), cfg["members"], cfg["seed"])
    tile = p.AddSTDRewardWrapper(twin, default_alpha=cfg["alpha"]).predict_processed_rollout(
        table_of(inputs[:cfg["calls"]], discrete), cfg["calls"], cfg["rows"])
    assert np.array_equal(bits(tile.cpu().numpy()), bits(np.concatenate(bounds)))
    s2, c2 = output_stats(twin)
    s1, c1 = output_stats(ens)
    assert np.array_equal(bits(s1), bits(s2)) and np.array_equal(c1, c2)
    assert twin.rollout_calls == 1 and twin.host_calls == 0 and ens.rollout_calls == 0


@pytest.mark.parametrize("fused", [True, False], ids=["member-batched", "per-member"])
def test_rollout_tile_equals_per_step_calls_16x64(fused, monkeypatch):
    """T = 16, n = 64, M = 5 with next state and done in the input. Member-batched forward: the tile is the per-step calls
    bit for bit (a row's forward depends on the row and the parameters alone; the statistics are replayed step by step).
    `IA_ENSEMBLE_FUSED=0`: the members' own forward launches, whose bits are not pinned across batch sizes -- the two ways
    agree to float32 rounding, and with the member-batched result."""
    monkeypatch.setenv("IA_ENSEMBLE_FUSED", "1" if fused else "0")
    T, n, M = 16, 64, 5
    o_space, a_space = p.Box(-np.inf, np.inf, (6,), np.float32), p.Box(-1.0, 1.0, (3,), np.float32)

    def build():
        th.manual_seed(5)
        members = [p.NormalizedRewardNet(p.BasicRewardNet(o_space, a_space, use_next_state=True, use_done=True),
                                         p.RunningNorm) for _ in range(M - 1)]
        members.append(p.BasicRewardNet(o_space, a_space, use_next_state=True, use_done=True))   # one without a norm
        return p.RewardEnsemble(o_space, a_space, members).to("cuda")

    r = np.random.default_rng(0)
    steps = [(r.normal(size=(n, 6)).astype(np.float32), r.uniform(-1, 1, (n, 3)).astype(np.float32),
              r.normal(size=(n, 6)).astype(np.float32), r.uniform(size=n) < 0.2) for _ in range(T)]
    a, b = build(), build()
    assert (a._fused_plan() is not None)
    per_step = np.concatenate([p.AddSTDRewardWrapper(a, 0.5).predict_processed(*s) for s in steps])
    tile = p.AddSTDRewardWrapper(b, 0.5).predict_processed_rollout(table_of(steps, False), T, n).cpu().numpy()
    sa, ca = output_stats(type("E", (), {"members": a.members[:-1]}))
    sb, cb = output_stats(type("E", (), {"members": b.members[:-1]}))
    assert np.array_equal(ca, cb) and (ca == T * n).all()
    if fused:
        assert np.array_equal(bits(tile), bits(per_step)) and np.array_equal(bits(sa), bits(sb))
    else:
        np.testing.assert_allclose(tile, per_step, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(sa, sb, rtol=1e-5)
        monkeypatch.setenv("IA_ENSEMBLE_FUSED", "1")
        ref_tile = p.AddSTDRewardWrapper(build(), 0.5).predict_processed_rollout(table_of(steps, False), T, n).cpu().numpy()
        np.testing.assert_allclose(tile, ref_tile, rtol=1e-4, atol=1e-5)
    assert np.isfinite(tile).all()


def test_mixed_members_take_their_own_forwards():
    """Members of different shapes (one outside the one-launch forward): no member-batched plan, same semantics."""
    o_space, a_space = p.Box(-np.inf, np.inf, (4,), np.float32), p.Discrete(3)
    th.manual_seed(1)
    members = [p.NormalizedRewardNet(p.BasicRewardNet(o_space, a_space), p.RunningNorm),
               p.NormalizedRewardNet(p.BasicRewardNet(o_space, a_space, hid_sizes=(16,)), p.RunningNorm),
               p.BasicRewardNet(o_space, a_space, hid_sizes=(64, 64))]
    ens = p.RewardEnsemble(o_space, a_space, members).to("cuda")
    assert ens._fused_plan() is None
    r = np.random.default_rng(2)
    args = (r.normal(size=(9, 4)).astype(np.float32), r.integers(0, 3, 9), r.normal(size=(9, 4)).astype(np.float32),
            np.zeros(9, bool))
    want = np.stack([m.predict_processed(*args, update_stats=False) for m in members], axis=-1)
    got = ens.predict_processed_all(*args, update_stats=False)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    mean, var = ens.predict_reward_moments(*args)
    assert np.array_equal(bits(mean), bits(got.mean(-1))) and np.array_equal(bits(var), bits(got.var(-1, ddof=1)))
    assert [int(m.normalize_output_layer.count.item()) for m in members[:2]] == [9, 9]
    bound = p.AddSTDRewardWrapper(ens, 0.5).predict_processed(*args, alpha=-1.0, update_stats=False)   # (kwargs not used)
    assert [int(m.normalize_output_layer.count.item()) for m in members[:2]] == [18, 18] and bound.shape == (9,)


def test_adversarial_trainers_refuse_an_ensemble():
    venv = SyntheticVecEnv(num_envs=2, obs_dim=4, act_dim=2, horizon=8, seed=0)
    ens = make_ensemble(venv.observation_space, venv.action_space, 2, 0)
    algo = p.PPO(p.FeedForward32Policy, venv, n_steps=8, batch_size=16, n_epochs=1, seed=0, device="cuda")
    for net in (ens, p.AddSTDRewardWrapper(ens)):
        with pytest.raises(NotImplementedError, match="reward ensembles"):
            p.GAIL(demonstrations=None, demo_batch_size=4, venv=venv, gen_algo=algo, reward_net=net,
                   custom_logger=p.configure_logger(format_strs=[]))
        with pytest.raises(NotImplementedError, match="reward ensembles"):
            p.AIRL(demonstrations=None, demo_batch_size=4, venv=venv, gen_algo=algo, reward_net=net,
                   custom_logger=p.configure_logger(format_strs=[]))


# ---------------------------------------------------------------------------------------------- the training runs

def _load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    assert {k: v for k, v in cfg.items() if k != "seed"} == RUNS[name]
    trajs = [dt.TrajectoryWithRew(obs=z[f"traj{k}_obs"], acts=z[f"traj{k}_acts"], rews=z[f"traj{k}_rews"], infos=None,
                                  terminal=True) for k in range(cfg["n_traj"])]
    return z, cfg, trajs


def _spaces(cfg):
    return (p.Box(-np.inf, np.inf, (cfg["obs_dim"],), np.float32),
            p.Discrete(cfg["act_dim"]) if cfg["discrete"] else p.Box(-1.0, 1.0, (cfg["act_dim"],), np.float32))


class _Recording(pc.ActiveSelectionFragmenter):
    def __init__(self, *args, ens, trajs, **kwargs):
        super().__init__(*args, **kwargs)
        self.ens, self.calls = ens, []
        self.number = {id(t): k for k, t in enumerate(trajs)}   # the goldens number the trajectories as the dataset does

    def __call__(self, trajectories, fragment_length, num_pairs):
        out = super().__call__(trajectories, fragment_length, num_pairs)
        stats, counts = output_stats(self.ens)
        assert all(len(t) >= fragment_length for t in trajectories)   # (the base fragmenter's indices are into this list)
        picks = [(self.number[id(trajectories[k])], start) for k, start in self.base_fragmenter.last_picks]
        self.calls.append(dict(picks=np.array(picks, np.int64), estimates=self.last_var_estimates,
                               selected=self.last_selected, stats=stats, counts=counts, n_out=len(out)))
        return out


def _run(name):
    z, cfg, trajs = _load(name)
    ens = make_ensemble(*_spaces(cfg), cfg["members"], cfg["seed"])
    check_init(ens, z, "init/")
    model = p.AddSTDRewardWrapper(ens, default_alpha=cfg["alpha"]) if cfg["std_wrapper"] else ens
    rng = np.random.default_rng(cfg["seed"])
    logger = p.configure_logger(format_strs=[])
    gen = pc.TrajectoryDataset(trajs, rng=rng, custom_logger=logger)
    pm = pc.PreferenceModel(model, noise_prob=cfg["noise"], discount_factor=cfg["gamma"])
    trainer = pc._make_reward_trainer(pm, pc.CrossEntropyRewardLoss(), rng,
                                      dict(batch_size=cfg["batch"], minibatch_size=cfg["mb"], epochs=cfg["epochs"],
                                           custom_logger=logger))
    assert type(trainer) is pc.EnsembleTrainer
    fragmenter = _Recording(pm, pc.RandomFragmenter(rng=rng, custom_logger=logger), cfg["factor"],
                            uncertainty_on=cfg["uncertainty_on"], custom_logger=logger, ens=ens, trajs=trajs)
    got = {"params": [], "adam": [], "dumps": [], "bags": [], "frag": fragmenter.calls}
    orig_train, orig_dump = trainer.train, logger.dump

    def train_call(dataset, epoch_multiplier=1.0):
        orig_train(dataset, epoch_multiplier)
        got["bags"].append(np.stack(trainer.last_bags))
        got["params"].append({k: v.detach().cpu().numpy().copy() for k, v in ens.state_dict().items()})
        got["adam"].append([{"step": t.optim.step_count, "exp_avg": t.optim.exp_avg.cpu().numpy().copy(),
                             "exp_avg_sq": t.optim.exp_avg_sq.cpu().numpy().copy()} for t in trainer.member_trainers])

    def dump(step=0):
        got["dumps"].append({k: float(v) for k, v in logger.default_logger.name_to_value.items()})
        orig_dump(step)

    trainer.train, logger.dump = train_call, dump
    algo = pc.PreferenceComparisons(gen, model, num_iterations=cfg["iters"], fragmenter=fragmenter,
                                    preference_gatherer=pc.SyntheticGatherer(rng=rng, discount_factor=cfg["gamma"],
                                                                             custom_logger=logger),
                                    reward_trainer=trainer, comparison_queue_size=cfg["queue"],
                                    fragment_length=cfg["frag"], initial_epoch_multiplier=cfg["init_mult"],
                                    custom_logger=logger)
    result = algo.train(total_timesteps=0, total_comparisons=cfg["comparisons"])
    return z, cfg, trajs, ens, got, result


def _propagated(z, cfg, trajs, got, i):
    """(estimates, statistics) by which fragmenter call i >= 1 of THIS run differs from the reference's because its member
    states before the call do: `active_selection_f64` from this run's states minus the same from the golden's."""
    gold_state = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"it{i - 1}_param/")}
    host = [(t.obs, t.acts) for t in trajs]
    args = (host, z[f"it{i}_picks"], cfg["members"], cfg["frag"], cfg["uncertainty_on"], cfg["gamma"], cfg["noise"])
    kw = dict(n_onehot=cfg["act_dim"] if cfg["discrete"] else 0)
    est_d, stats_d, _ = active_selection_f64(got["params"][i - 1], *args, **kw)
    est_g, stats_g, _ = active_selection_f64(gold_state, *args, **kw)
    np.testing.assert_allclose(est_g, z[f"it{i}_estimates"], rtol=1e-9, atol=1e-12)   # (the restatement is the reference's)
    np.testing.assert_allclose(stats_g, z[f"it{i}_frag_stats"], rtol=1e-9, atol=1e-12)
    return est_d - est_g, stats_d - stats_g


def _fragment(traj, start, L_):
    end = start + L_
    return dt.TrajectoryWithRew(obs=traj.obs[start:end + 1], acts=traj.acts[start:end], infos=None,
                                rews=traj.rews[start:end], terminal=(end == len(traj)) and traj.terminal)


def _teacher_forced(z, cfg, trajs):
    """Every fragmenter call of the run scored from the REFERENCE's member states before that call (the initial ones, then
    the golden's states after each training) on the reference's candidate pairs: estimates by the plain rule (`label`:
    exact), selected indices and counts exact, statistics after the call by the plain rule -- every iteration, every pair."""
    worst = {}
    logger = p.configure_logger(format_strs=[])
    for i in range(int(z["n_iters"])):
        ens = make_ensemble(*_spaces(cfg), cfg["members"], cfg["seed"])
        if i:
            ens.load_state_dict({k.split("/", 1)[1]: th.from_numpy(np.asarray(z[k])) for k in z.files
                                 if k.startswith(f"it{i - 1}_param/")})
        pm = pc.PreferenceModel(ens, noise_prob=cfg["noise"], discount_factor=cfg["gamma"])
        f = pc.ActiveSelectionFragmenter(pm, pc.RandomFragmenter(np.random.default_rng(0), custom_logger=logger),
                                         cfg["factor"], uncertainty_on=cfg["uncertainty_on"], custom_logger=logger)
        frags = iter([_fragment(trajs[k], start, cfg["frag"]) for k, start in z[f"it{i}_picks"]])
        est = f.variance_estimates(list(zip(frags, frags)))
        gold = z[f"it{i}_estimates"]
        if cfg["uncertainty_on"] == "label":
            assert np.array_equal(est, gold), i
        else:
            _close(est, gold, f"it{i} estimates from the reference's states", worst, atol=1e-4, rtol=1e-3)
        num_pairs = int(z["schedule"][i])
        assert np.array_equal(np.argsort(est)[::-1][:num_pairs], z[f"it{i}_selected"]), i
        stats, counts = output_stats(ens)
        assert np.array_equal(counts, z[f"it{i}_frag_counts"]), i
        _close(stats, z[f"it{i}_frag_stats"], f"it{i} statistics from the reference's states", worst)
    print("from the reference's states, worst |deviation|:", worst)


def _check_run(z, cfg, trajs, got, result):
    worst = {}
    n = int(z["n_iters"])
    assert len(got["params"]) == len(got["dumps"]) == len(got["frag"]) == len(got["bags"]) == n
    for i in range(n):                                    # every iteration, every pair
        f = got["frag"][i]
        assert np.array_equal(f["picks"], z[f"it{i}_picks"]), i
        assert f["estimates"].dtype == np.float64 and f["estimates"].shape == z[f"it{i}_estimates"].shape
        gold = z[f"it{i}_estimates"]
        d_est, d_stats = _propagated(z, cfg, trajs, got, i) if i else (0.0, 0.0)
        err = np.abs(f["estimates"] - gold)
        print(f"it{i} estimates: largest deviation {float(err.max()):.3e} on values up to {float(gold.max()):.3g}; with this "
              f"run's parameter deviation taken off {float(np.abs(f['estimates'] - d_est - gold).max()):.3e}")
        if cfg["uncertainty_on"] == "label":
            assert np.array_equal(f["estimates"], gold), i
        else:
            _close(f["estimates"] - d_est, gold, f"it{i} estimates", worst, atol=1e-4, rtol=1e-3)
            assert err.max() <= 0.05 * np.abs(gold).max() + 1e-5, (i, float(err.max()), float(np.abs(gold).max()))
        assert np.array_equal(f["selected"], z[f"it{i}_selected"]), (i, f["selected"], z[f"it{i}_selected"])
        assert f["n_out"] == int(z["schedule"][i])
        assert np.array_equal(f["counts"], z[f"it{i}_frag_counts"]), i
        print(f"it{i} statistics after the fragmenter: largest deviation "
              f"{float(np.abs(f['stats'] - z[f'it{i}_frag_stats']).max()):.3e}")
        _close(f["stats"] - d_stats, z[f"it{i}_frag_stats"], f"it{i} statistics after the fragmenter", worst)
        assert np.array_equal(got["bags"][i], z[f"it{i}_bags"]), i
        for key in [k for k in z.files if k.startswith(f"it{i}_param/")]:
            name = key.split("/", 1)[1]
            gold, x = z[key], got["params"][i][name]
            steps = int(z[f"it{i}_adam{name.split('.')[1]}/step"])
            if gold.dtype.kind in "iu":
                assert np.array_equal(np.asarray(x), gold), (i, name)
            elif "normalize_" in name:
                # reward training does not touch the output statistics: they are the ones checked after the fragmenter call
                m, col = int(name.split(".")[1]), 0 if "running_mean" in name else 1
                assert np.asarray(x).item() == f["stats"][m, col] and gold.item() == z[f"it{i}_frag_stats"][m, col], (i, name)
            else:
                _close(x, gold, f"it{i} {name}", worst, steps=steps, frac=0.15 if i == 0 else 1.0)
        for m, a in enumerate(got["adam"][i]):
            steps = int(z[f"it{i}_adam{m}/step"])
            assert int(a["step"]) == steps
            gold = z[f"it{i}_adam{m}/exp_avg"]
            if i == 0:
                _close(a["exp_avg"], gold, f"it{i} member {m} exp_avg", worst, steps=steps)
            else:
                err = np.abs(a["exp_avg"] - gold).max()
                worst[f"it{i} member {m} exp_avg"] = float(err)
                assert err <= 0.05 * np.abs(gold).max() + 1e-5, (i, m, float(err), float(np.abs(gold).max()))
        keys = list(z[f"it{i}_log_keys"])
        assert sorted(got["dumps"][i]) == keys, i
        assert any(k.startswith("member-0/") for k in keys) and any(k.endswith("_std") for k in keys)
        _close([got["dumps"][i][k] for k in keys], z[f"it{i}_log_vals"], f"it{i} log", worst, atol=1e-4, rtol=1e-3)
    _close([result["reward_loss"], result["reward_accuracy"]], z["result"], "result", worst, atol=1e-4, rtol=1e-3)
    print("worst |deviation|:", max(worst.values()), max(worst, key=worst.get))


def test_logit_run_matches_reference_and_probability_call_on_its_final_states():
    z, cfg, trajs, ens, got, result = _run("preference_ensemble_logit")
    _check_run(z, cfg, trajs, got, result)
    _teacher_forced(z, cfg, trajs)
    # one `probability` fragmenter call on the golden's final member states
    last = int(z["n_iters"]) - 1
    fresh = make_ensemble(*_spaces(cfg), cfg["members"], cfg["seed"])
    fresh.load_state_dict({k.split("/", 1)[1]: th.from_numpy(np.asarray(z[k])) for k in z.files
                           if k.startswith(f"it{last}_param/")})
    pm = pc.PreferenceModel(fresh, noise_prob=cfg["noise"], discount_factor=cfg["gamma"])
    logger = p.configure_logger(format_strs=[])
    base = pc.RandomFragmenter(rng=np.random.default_rng(PROBABILITY_CASE["rng_seed"]), custom_logger=logger)
    f = _Recording(pm, base, cfg["factor"], uncertainty_on="probability", custom_logger=logger, ens=fresh,
                   trajs=trajs)
    out = f(trajs, cfg["frag"], PROBABILITY_CASE["num_pairs"])
    c, worst = f.calls[0], {}
    assert len(out) == PROBABILITY_CASE["num_pairs"] and np.array_equal(c["picks"], z["prob_picks"])
    _close(c["estimates"], z["prob_estimates"], "probability estimates", worst)
    assert np.array_equal(c["selected"], z["prob_selected"]) and np.array_equal(c["counts"], z["prob_counts"])
    _close(c["stats"], z["prob_stats"], "statistics after the probability call", worst)
    print("probability case, worst |deviation|:", worst)


def test_label_run_matches_reference():
    z, cfg, trajs, ens, got, result = _run("preference_ensemble_label")
    _check_run(z, cfg, trajs, got, result)
    _teacher_forced(z, cfg, trajs)


def test_preference_model_rewards_and_probability_of_an_ensemble():
    """`rewards()` is `predict_processed_all` as a device tensor `[n, M]` (statistics move); `probability()` on `[L, M]`
    rewards is, column by column, the members' own `probability`."""
    o, a = p.Box(-np.inf, np.inf, (4,), np.float32), p.Box(-1.0, 1.0, (2,), np.float32)
    ens, twin = make_ensemble(o, a, 3, 9), make_ensemble(o, a, 3, 9)
    pm = pc.PreferenceModel(p.AddSTDRewardWrapper(ens), noise_prob=0.1, discount_factor=0.9, threshold=2.0)
    r = np.random.default_rng(4)
    frag = dt.TrajectoryWithRew(obs=r.normal(size=(8, 4)).astype(np.float32), acts=r.uniform(-1, 1, (7, 2)).astype(np.float32),
                                infos=None, terminal=True, rews=np.zeros(7, np.float32))
    tr = dt.flatten_trajectories([frag])
    for _ in range(2):   # the second call is normalised with the statistics the first one left
        rews = pm.rewards(tr)
        assert rews.shape == (7, 3) and rews.is_cuda and rews.dtype == th.float32
        want = twin.predict_processed_all(tr.obs, tr.acts, tr.next_obs, tr.dones)
        assert np.array_equal(bits(rews.cpu().numpy()), bits(want))
    assert np.array_equal(output_stats(ens)[1], [14, 14, 14])
    r1 = th.as_tensor((r.normal(size=(7, 3)) * 0.8).astype(np.float32)).cuda()
    r2 = th.as_tensor((r.normal(size=(7, 3)) * 0.8).astype(np.float32)).cuda()
    r2[:, 2] += 3.0                                              # member 2: beyond the clip
    probs = pm.probability(r1, r2)
    assert probs.shape == (3,)
    member = th.stack([mp.probability(r1[:, m].contiguous(), r2[:, m].contiguous())
                       for m, mp in enumerate(pm.member_pref_models)])
    assert th.equal(probs, member)
    w = 0.9 ** np.arange(7)
    diff = np.clip(((r2 - r1).cpu().numpy().astype(np.float64) * w[:, None]).sum(0), -2.0, 2.0)
    assert abs(diff[2]) == 2.0
    np.testing.assert_allclose(probs.cpu().numpy(), 0.05 + 0.9 / (1 + np.exp(diff)), rtol=1e-5)
    with pytest.raises(AssertionError):
        pm.probability(r1[:, 0], r2[:, 0])                       # the reference's own shape assertion


def test_fragments_of_unequal_length_are_refused():
    o, a = p.Box(-np.inf, np.inf, (3,), np.float32), p.Box(-1.0, 1.0, (2,), np.float32)
    pm = pc.PreferenceModel(make_ensemble(o, a, 2, 0))
    frag = lambda L_: dt.TrajectoryWithRew(obs=np.zeros((L_ + 1, 3), np.float32), acts=np.zeros((L_, 2), np.float32),
                                           infos=None, terminal=False, rews=np.zeros(L_, np.float32))

    class Base(pc.Fragmenter):
        def __call__(self, trajectories, fragment_length, num_pairs):
            return [(frag(3), frag(4))] * num_pairs

    f = pc.ActiveSelectionFragmenter(pm, Base(), 2.0)
    with pytest.raises(NotImplementedError, match="different lengths"):
        f([], 3, 2)


# ---------------------------------------------------------------------------------------------- the agent's rollouts

def _agent_run(bulk: bool):
    th.manual_seed(0)
    venv = SyntheticVecEnv(num_envs=8, obs_dim=6, act_dim=2, horizon=20, seed=0)
    algo = p.PPO(p.FeedForward32Policy, venv, n_steps=16, batch_size=64, n_epochs=1, seed=0, device="cuda")
    ens = make_ensemble(venv.observation_space, venv.action_space, 3, 3)
    net = p.AddSTDRewardWrapper(ens, default_alpha=0.5)
    tiles, steps = [], []
    if bulk:
        orig = net.predict_processed_rollout

        def rollout(table, T, n):
            out = orig(table, T, n)
            tiles.append(out.detach().cpu().numpy().reshape(T, n).copy())
            return out

        net.predict_processed_rollout = rollout
        reward_fn = net
    else:
        def reward_fn(state, action, next_state, done):   # a plain function: the collector calls it once per step
            steps.append(net.predict_processed(state, action, next_state, done))
            return steps[-1]

    gen = pc.AgentTrainer(algo, reward_fn, venv, rng=np.random.default_rng(0),
                          custom_logger=p.configure_logger(format_strs=[]))
    if bulk:
        assert gen.reward_venv_wrapper.reward_fn.__self__ is net
    gen.train(steps=8 * 16 * 2)
    if not bulk:
        tiles = [np.stack(steps[k:k + 16]) for k in range(0, len(steps), 16)]
    return ens, tiles, output_stats(ens)


def test_agent_trainer_relabels_tiles_in_bulk_with_the_per_step_bits():
    ens, tiles, (stats, counts) = _agent_run(bulk=True)
    assert ens.rollout_calls == 2 and ens.host_calls == 0        # two rollouts, no per-step host call
    assert len(tiles) == 2 and tiles[0].shape == (16, 8) and (counts == 2 * 16 * 8).all()
    twin, steps, (stats2, counts2) = _agent_run(bulk=False)
    assert twin.rollout_calls == 0 and twin.host_calls == 2 * 16
    assert len(steps) == 2
    for a, b in zip(tiles, steps):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(stats), bits(stats2)) and np.array_equal(counts, counts2)
