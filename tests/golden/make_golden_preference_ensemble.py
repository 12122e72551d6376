"""Generates `tests/golden/ensemble_moments.npz` and `tests/golden/preference_ensemble_*.npz` by running the REFERENCE's own
`RewardEnsemble`, `AddSTDRewardWrapper`, `EnsembleTrainer` and `ActiveSelectionFragmenter` (imported unmodified under
`oracle.ref_shim`, as `make_golden_preferences.py` does). Runs only where the reference sources are present.
Usage: `python tests/golden/make_golden_preference_ensemble.py [moments] [CASE ...]` (nothing: everything).

Every run is made twice: in float32, the reference as it stands, and in float64: the same classes with the members
converted to double, a `BasicRewardNet` subclass whose `preprocess` widens the reference's float32 tensors, and -- for the
training runs -- the algorithm module's `th.float32` read as `th.float64` (the module allocates its probability vectors
and casts the preferences with that name). Floating values stored are the float64 run's; per float key of
`ensemble_moments.npz`, `dref/` = the relative L2 deviation of the float32 run from it (the device is allowed 8 x).

A seed of a training run is kept only if
* the float32 and the float64 run select the same candidate pairs in the same order in every fragmenter call;
* `logit` / `probability`: in every fragmenter call every adjacent gap of the sorted float64 estimates is at least
  `DIFFER_FACTOR` (100) x that call's largest float32-to-float64 deviation of an estimate;
* `label`: the two runs' estimates are equal (so exact ties are broken identically) and no member probability of either
  run lies within 1e-4 of 0.5, nor within `DIFFER_FACTOR` x the largest float32-to-float64 deviation of a probability.
Seeds are searched from 0 upwards, at most `SEARCH_BOUND` = 200 of them. Kept: `preference_ensemble_logit` seed 1 (seed 0
fails the gap condition; the `probability` component case is part of the conditions), `preference_ensemble_label` seed 0
-- `main` prints the seed it keeps and stores it in the file's `cfg`.
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from imitation_amd import spaces as sp  # noqa: E402
from oracle import ref_shim  # noqa: E402
from tests.preference_ensemble_golden import (DECISIVE, DIFFER_FACTOR, MOMENTS, MOMENTS_CASES, PROBABILITY_CASE,  # noqa: E402
                                              RUNS, make_trajectories, moments_inputs)

SEARCH_BOUND = 200


def install():
    ref_shim.install()
    import types as _types

    from oracle import sb3_restated as sb
    ta = _types.ModuleType("stable_baselines3.common.type_aliases")
    ta.Schedule = object
    sys.modules["stable_baselines3.common.type_aliases"] = ta
    sys.modules["stable_baselines3.common"].type_aliases = ta
    if not hasattr(sb.Logger, "warn"):
        sb.Logger.warn = lambda self, *args, **kwargs: None
    from imitation.algorithms import preference_comparisons as pc
    from imitation.data import types
    from imitation.rewards import reward_nets
    from imitation.util import logger as imit_logger
    from imitation.util import networks
    return dict(pc=pc, types=types, rn=reward_nets, nets=networks, log=imit_logger)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


class _ThDouble:
    """`torch` for the algorithm module of a float64 run: `float32` reads as `float64`, everything else is torch's."""

    def __init__(self, th):
        self._th = th
        self.float32 = th.float64

    def __getattr__(self, name):
        return getattr(self._th, name)


@contextlib.contextmanager
def algorithm_in_double(m, double):
    import torch as th
    if double:
        m["pc"].th = _ThDouble(th)
    try:
        yield
    finally:
        m["pc"].th = th


def make_ensemble(m, obs_space, act_space, n_members, seed, double):
    """`RewardEnsemble` of `NormalizedRewardNet(BasicRewardNet(32, 32), RunningNorm)` members (the reference's
    `reward_ensemble` named config), initial parameters drawn in float32 from `seed` in both precisions."""
    import torch as th
    rn, nets = m["rn"], m["nets"]

    class DoubleBasicRewardNet(rn.BasicRewardNet):
        def preprocess(self, state, action, next_state, done):
            return tuple(t.double() for t in super().preprocess(state, action, next_state, done))

    th.manual_seed(seed)
    cls = DoubleBasicRewardNet if double else rn.BasicRewardNet
    members = [rn.NormalizedRewardNet(cls(obs_space, act_space), nets.RunningNorm) for _ in range(n_members)]
    ens = rn.RewardEnsemble(obs_space, act_space, members)
    return ens.double() if double else ens


def state_of(net):
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


def output_stats(ens):
    """([M, 2] running (mean, var) of the members' output norms -- one array, so that its relative deviation is not that of
    a single scalar --, [M] counts)."""
    norms = [mem.normalize_output_layer for mem in ens.members]
    stats = np.array([[float(n.running_mean), float(n.running_var)] for n in norms], np.float64)
    return stats, np.array([int(n.count) for n in norms], np.int64)


# ------------------------------------------------------------------------------------------------------- the reward nets alone

def moments_run(m, discrete, double):
    cfg = MOMENTS
    obs_space = sp.Box(-np.inf, np.inf, (cfg["obs_dim"],), np.float32)
    act_space = sp.Discrete(cfg["n_discrete"]) if discrete else sp.Box(-1.0, 1.0, (cfg["act_dim"],), np.float32)
    ens = make_ensemble(m, obs_space, act_space, cfg["members"], cfg["seed"], double)
    net = m["rn"].AddSTDRewardWrapper(ens, default_alpha=cfg["alpha"])
    out = {"init": state_of(ens)}
    inputs = moments_inputs(discrete)
    for c in range(cfg["calls"]):
        out[f"call{c}/bound"] = np.asarray(net.predict_processed(*inputs[c]), np.float64)
        out[f"call{c}/stats"], out[f"call{c}/counts"] = output_stats(ens)
    out["all"] = np.asarray(ens.predict_processed_all(*inputs[-1], update_stats=False), np.float64)
    mean, var = ens.predict_reward_moments(*inputs[-1], update_stats=False)
    out["all_mean"], out["all_var"] = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    out["final/stats"], out["final/counts"] = output_stats(ens)
    return out


def make_moments(m):
    out = {"cfg": json.dumps(MOMENTS)}
    for name in MOMENTS_CASES:
        r32, r64 = moments_run(m, name == "discrete", False), moments_run(m, name == "discrete", True)
        for k, v in r32["init"].items():
            out[f"{name}/init/{k}"] = v
            assert np.array_equal(np.asarray(v, np.float64), np.asarray(r64["init"][k], np.float64)), k
        for k in (k for k in r64 if k != "init"):
            v64, v32 = np.asarray(r64[k]), np.asarray(r32[k])
            if v64.dtype.kind in "iu":
                assert np.array_equal(v64, v32), k
                out[f"{name}/{k}"] = v64
            else:
                out[f"{name}/f64/{k}"] = v64.astype(np.float64)
                out[f"{name}/dref/{k}"] = np.float64(rel_l2(v32, v64))
        print(name, {k[len(name) + 6:]: float(f"{float(v):.2e}") for k, v in out.items() if k.startswith(f"{name}/dref/")})
    path = os.path.join(HERE, "ensemble_moments.npz")
    np.savez_compressed(path, **out)
    print("ensemble_moments.npz bytes", os.path.getsize(path))


# ------------------------------------------------------------------------------------------------------- the training runs

class Recorder:
    """Wraps the reference's objects of one run and records what the fixture stores."""

    def __init__(self, m, trajs):
        self.m, self.trajs = m, trajs
        self.by_id = {id(t.obs): k for k, t in enumerate(trajs)}
        self.picks, self.estimates, self.probs, self.frag_stats = [], [], [], []
        self.bags, self.params, self.adam, self.dumps, self.gathered = [], [], [], [], []

    def picks_of(self, pairs):
        picks = []
        for f in (f for p in pairs for f in p):
            k = self.by_id[id(f.obs.base)]
            start = (f.obs.__array_interface__["data"][0] - self.trajs[k].obs.__array_interface__["data"][0]) \
                // self.trajs[k].obs.strides[0]
            picks.append((k, int(start)))
        return np.array(picks, np.int64)

    def base_fragmenter(self, rng, logger):
        pc, rec = self.m["pc"], self
        inner = pc.RandomFragmenter(rng=rng, custom_logger=logger)

        class Base(pc.Fragmenter):
            def __call__(self, trajectories, fragment_length, num_pairs):
                pairs = inner(trajectories, fragment_length, num_pairs)
                rec.picks.append(rec.picks_of(pairs))
                return pairs

        return Base(custom_logger=logger)

    def active_fragmenter(self, pm, base, factor, mode, logger, ens):
        pc, rec = self.m["pc"], self

        class Active(pc.ActiveSelectionFragmenter):
            def __call__(self, trajectories, fragment_length, num_pairs):
                rec.estimates.append([])
                rec.probs.append([])
                out = super().__call__(trajectories, fragment_length, num_pairs)
                rec.frag_stats.append(output_stats(ens))
                return out

            def variance_estimate(self, rews1, rews2):
                v = super().variance_estimate(rews1, rews2)
                rec.estimates[-1].append(float(v))
                if self.uncertainty_on != "logit":
                    rec.probs[-1].append(self.preference_model.probability(rews1, rews2).detach().numpy().astype(np.float64))
                return v

        return Active(pm, base, factor, uncertainty_on=mode, custom_logger=logger)


def training_run(m, cfg, seed, double):
    import torch as th
    pc, types, rn, log = m["pc"], m["types"], m["rn"], m["log"]
    raw = make_trajectories(cfg, seed)
    trajs = [types.TrajectoryWithRew(obs=o, acts=a, rews=w, infos=None, terminal=True) for o, a, w in raw]
    obs_space = sp.Box(-np.inf, np.inf, (cfg["obs_dim"],), np.float32)
    act_space = sp.Discrete(cfg["act_dim"]) if cfg["discrete"] else sp.Box(-1.0, 1.0, (cfg["act_dim"],), np.float32)
    ens = make_ensemble(m, obs_space, act_space, cfg["members"], seed, double)
    model = rn.AddSTDRewardWrapper(ens, default_alpha=cfg["alpha"]) if cfg["std_wrapper"] else ens
    init = state_of(ens)
    rng = np.random.default_rng(seed)
    logger = log.configure(os.path.join(tempfile.mkdtemp(), "run"), ["log"])
    rec = Recorder(m, trajs)
    gen = pc.TrajectoryDataset(trajs, rng=rng, custom_logger=logger)
    pm = pc.PreferenceModel(model, noise_prob=cfg["noise"], discount_factor=cfg["gamma"])
    trainer = pc._make_reward_trainer(pm, pc.CrossEntropyRewardLoss(), rng,
                                      dict(batch_size=cfg["batch"], minibatch_size=cfg["mb"], epochs=cfg["epochs"],
                                           custom_logger=logger))
    assert type(trainer) is pc.EnsembleTrainer
    fragmenter = rec.active_fragmenter(pm, rec.base_fragmenter(rng, logger), cfg["factor"], cfg["uncertainty_on"], logger, ens)
    inner_gather = pc.SyntheticGatherer(rng=rng, discount_factor=cfg["gamma"], custom_logger=logger)

    class Gatherer(pc.PreferenceGatherer):
        def __call__(self, pairs):
            p = inner_gather(pairs)
            rec.gathered.append(np.asarray(p, np.float32))
            return p

    for i, t in enumerate(trainer.member_trainers):
        def member_train(dataset, epoch_multiplier=1.0, _orig=t.train):
            rec.bags[-1].append(np.asarray(dataset.indices, np.int64))
            _orig(dataset, epoch_multiplier)
        t.train = member_train
    orig_train = trainer.train

    def train_call(dataset, epoch_multiplier=1.0):
        rec.bags.append([])
        orig_train(dataset, epoch_multiplier)
        rec.params.append(state_of(ens))
        adam = []
        for t in trainer.member_trainers:
            st, ps = t.optim.state, list(t.optim.param_groups[0]["params"])
            adam.append({"step": int(st[ps[0]]["step"]),
                         "exp_avg": np.concatenate([st[q]["exp_avg"].reshape(-1).numpy() for q in ps]),
                         "exp_avg_sq": np.concatenate([st[q]["exp_avg_sq"].reshape(-1).numpy() for q in ps])})
        rec.adam.append(adam)

    trainer.train = train_call
    orig_dump = logger.dump

    def dump(step=0):
        rec.dumps.append({k: float(v) for k, v in logger.default_logger.name_to_value.items()})
        orig_dump(step)

    logger.dump = dump
    algo = pc.PreferenceComparisons(gen, model, num_iterations=cfg["iters"], fragmenter=fragmenter,
                                    preference_gatherer=Gatherer(custom_logger=logger), reward_trainer=trainer,
                                    comparison_queue_size=cfg["queue"], fragment_length=cfg["frag"],
                                    initial_epoch_multiplier=cfg["init_mult"], custom_logger=logger)
    fragmenter.logger = logger
    trainer.train, logger.dump = train_call, dump
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), algorithm_in_double(m, double):
        result = algo.train(total_timesteps=0, total_comparisons=cfg["comparisons"])
        schedule = json.loads(buf.getvalue().split("Query schedule: ")[1].split("\n")[0])
        extra = None
        if cfg["probability_case"]:   # one more fragmenter call, `probability`, on the final member states
            prng = np.random.default_rng(PROBABILITY_CASE["rng_seed"])
            n_before = len(rec.picks)
            # (over the bare ensemble: the reference's `probability` asserts on `model.num_members`, which the
            #  AddSTDRewardWrapper of this run does not have)
            pm2 = pc.PreferenceModel(ens, noise_prob=cfg["noise"], discount_factor=cfg["gamma"])
            f2 = rec.active_fragmenter(pm2, rec.base_fragmenter(prng, logger), cfg["factor"], "probability", logger, ens)
            f2(trajs, cfg["frag"], PROBABILITY_CASE["num_pairs"])
            extra = dict(picks=rec.picks.pop(), estimates=np.array(rec.estimates.pop()), probs=np.array(rec.probs.pop()),
                         stats=rec.frag_stats.pop())
            assert len(rec.picks) == n_before
    return dict(raw=raw, init=init, schedule=schedule, result=result, rec=rec, extra=extra)


def selection(estimates, num_pairs):
    return np.argsort(np.asarray(estimates, np.float64))[::-1][:num_pairs]


def call_ok(mode, e32, e64, p32, p64, num_pairs):
    """The conditions on one fragmenter call (module docstring)."""
    e32, e64 = np.asarray(e32, np.float64), np.asarray(e64, np.float64)
    if not np.array_equal(selection(e32, num_pairs), selection(e64, num_pairs)):
        return False
    if mode == "label":
        p32, p64 = np.asarray(p32), np.asarray(p64)
        margin = min(np.abs(p32 - 0.5).min(), np.abs(p64 - 0.5).min())
        return bool(np.array_equal(e32, e64) and margin > max(DECISIVE, DIFFER_FACTOR * np.abs(p32 - p64).max()))
    gaps = np.diff(np.sort(e64))
    return bool(gaps.min() >= DIFFER_FACTOR * np.abs(e32 - e64).max())


def make_run(m, name):
    cfg = RUNS[name]
    for seed in range(SEARCH_BOUND):
        r32, r64 = training_run(m, cfg, seed, False), training_run(m, cfg, seed, True)
        a, b = r32["rec"], r64["rec"]
        ok = r32["schedule"] == r64["schedule"] and all(np.array_equal(x, y) for x, y in zip(a.picks, b.picks))
        ok = ok and all(np.array_equal(np.stack(x), np.stack(y)) for x, y in zip(a.bags, b.bags))
        ok = ok and all(np.array_equal(x, y) for x, y in zip(a.gathered, b.gathered))
        for i, num_pairs in enumerate(r32["schedule"]):
            ok = ok and call_ok(cfg["uncertainty_on"], a.estimates[i], b.estimates[i], a.probs[i], b.probs[i], num_pairs)
        if ok and cfg["probability_case"]:
            x, y = r32["extra"], r64["extra"]
            ok = np.array_equal(x["picks"], y["picks"]) and call_ok("probability", x["estimates"], y["estimates"], None, None,
                                                                    PROBABILITY_CASE["num_pairs"])
        print(name, "seed", seed, "kept" if ok else "dropped")
        if ok:
            break
    else:
        raise SystemExit(f"{name}: no seed below {SEARCH_BOUND} satisfies the conditions")
    rec = r64["rec"]
    out = {"cfg": json.dumps(dict(cfg, seed=seed)), "schedule": np.array(r64["schedule"], np.int64),
           "n_iters": np.int64(len(r64["schedule"])),
           "result": np.array([r64["result"]["reward_loss"], r64["result"]["reward_accuracy"]], np.float64)}
    for k, (o, ac, w) in enumerate(r64["raw"]):
        out[f"traj{k}_obs"], out[f"traj{k}_acts"], out[f"traj{k}_rews"] = o, ac, w
    for k, v in r32["init"].items():
        out[f"init/{k}"] = v
    for i, num_pairs in enumerate(r64["schedule"]):
        out[f"it{i}_picks"] = rec.picks[i]
        out[f"it{i}_estimates"] = np.array(rec.estimates[i], np.float64)
        out[f"it{i}_est_dev32"] = np.float64(np.abs(np.array(a.estimates[i]) - np.array(rec.estimates[i])).max())
        out[f"it{i}_selected"] = selection(rec.estimates[i], num_pairs).astype(np.int64)
        out[f"it{i}_prefs"] = rec.gathered[i]
        out[f"it{i}_bags"] = np.stack(rec.bags[i])
        out[f"it{i}_frag_stats"], out[f"it{i}_frag_counts"] = rec.frag_stats[i]
        for k, v in rec.params[i].items():
            out[f"it{i}_param/{k}"] = v
        for mi, ad in enumerate(rec.adam[i]):
            for k, v in ad.items():
                out[f"it{i}_adam{mi}/{k}"] = np.asarray(v)
        d = rec.dumps[i]
        keys = sorted(d)
        out[f"it{i}_log_keys"] = np.array(keys)
        out[f"it{i}_log_vals"] = np.array([d[k] for k in keys], np.float64)
    if cfg["probability_case"]:
        x = r64["extra"]
        out["prob_picks"], out["prob_estimates"] = x["picks"], np.asarray(x["estimates"], np.float64)
        out["prob_est_dev32"] = np.float64(np.abs(np.asarray(r32["extra"]["estimates"]) - x["estimates"]).max())
        out["prob_selected"] = selection(x["estimates"], PROBABILITY_CASE["num_pairs"]).astype(np.int64)
        out["prob_stats"], out["prob_counts"] = x["stats"]
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "seed", seed, "schedule", r64["schedule"], "result", r64["result"], "bytes", os.path.getsize(path))


def main():
    names = sys.argv[1:] or ["moments", *RUNS]
    unknown = [n for n in names if n != "moments" and n not in RUNS]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {['moments', *RUNS]}")
    m = install()
    for name in names:
        if name == "moments":
            make_moments(m)
        else:
            make_run(m, name)


if __name__ == "__main__":
    main()
