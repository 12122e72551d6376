"""Reward-ensemble scoring on the GPU (`imitation_amd/reward_nets.py` `RewardEnsemble` / `AddSTDRewardWrapper`,
`imitation_amd/preference_comparisons.py` `ActiveSelectionFragmenter`, `csrc/ensemble.hip`). Two workloads, each measured
two ways that take turns sample by sample (drift of the machine lands on both alike); one JSON line per workload and way:

  (a) rollout_tile    the reward step of a 16 x 1024 rollout tile: D = 23 (obs 17, act 6), M = 5 members
                      `NormalizedRewardNet(BasicRewardNet(32, 32), RunningNorm)`, `AddSTDRewardWrapper(alpha = 0.5)`:
                      `predict_processed_rollout` on a resident table (forward, the members' output norms step by step,
                      the moments over the members);
  (b) active_selection one `ActiveSelectionFragmenter` call at the reference's defaults: fragments of 100 steps, 2 x 50
                      candidate pairs for 50 (`fragment_sample_factor` 2), M = 5, `logit`; `score_us` = upload, the
                      three launches and the read-back of the estimates for pairs drawn ahead, `call_us` = the whole call
                      (the base fragmenter's host draws included).

  member-batched   `ia_ensemble_forward`: the M members' forwards in ONE launch                    (IA_ENSEMBLE_FUSED=1)
  per-member       the M members' own forward launches as before this module existed              (IA_ENSEMBLE_FUSED=0)

Both ways share the norm, moment and uncertainty kernels. Times are the host clock around work that ends in a device
synchronise (or a read-back); warm-up first, then `--samples` samples each; median and the 10th / 90th percentile. The run
ends itself after `--limit` seconds.

  python tools/ensemble_bench.py [--samples 200] [--warmup 20]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAYS = (("member-batched", "1"), ("per-member", "0"))


def _stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)))


def make_ensemble(p, th, obs_space, act_space, M):
    th.manual_seed(0)
    members = [p.NormalizedRewardNet(p.BasicRewardNet(obs_space, act_space), p.RunningNorm) for _ in range(M)]
    return p.RewardEnsemble(obs_space, act_space, members).to("cuda")


def bench(args):
    import torch as th

    import imitation_amd as p
    from imitation_amd import preference_comparisons as pc
    from imitation_amd.data_types import TrajectoryWithRew
    from imitation_amd.networks import TransitionTable
    assert th.cuda.is_available(), "ensemble_bench needs a GPU"
    M, od, ad = 5, 17, 6
    obs_space, act_space = p.Box(-np.inf, np.inf, (od,), np.float32), p.Box(-1.0, 1.0, (ad,), np.float32)
    sync = th.cuda.synchronize

    # ---- (a) the reward step of a rollout tile
    T, n = 16, 1024
    g = th.Generator(device="cuda").manual_seed(0)
    table = TransitionTable(th.randn(T * n, od, device="cuda", generator=g),
                            th.rand(T * n, ad, device="cuda", generator=g) * 2 - 1,
                            th.randn(T * n, od, device="cuda", generator=g),
                            th.zeros(T * n, dtype=th.uint8, device="cuda"), False)
    nets = {}
    for way, flag in WAYS:
        os.environ["IA_ENSEMBLE_FUSED"] = flag
        nets[way] = p.AddSTDRewardWrapper(make_ensemble(p, th, obs_space, act_space, M), default_alpha=0.5)
        assert (nets[way].base._fused_plan() is not None)

    def tile(way, flag):
        os.environ["IA_ENSEMBLE_FUSED"] = flag
        sync()
        t0 = time.perf_counter()
        out = nets[way].predict_processed_rollout(table, T, n)
        sync()
        return 1e6 * (time.perf_counter() - t0), out

    outs = {way: tile(way, flag)[1].clone() for way, flag in WAYS}
    dev = float((outs["member-batched"] - outs["per-member"]).abs().max())
    times = {way: [] for way, _ in WAYS}
    for k in range(args.warmup + args.samples):
        for way, flag in WAYS:
            us, _ = tile(way, flag)
            if k >= args.warmup:
                times[way].append(us)
    for way, _ in WAYS:
        print(json.dumps(dict(bench="ensemble", workload="rollout_tile", way=way, T=T, n=n, D=od + ad, members=M, alpha=0.5,
                              launches=3 if way == "member-batched" else "2 + the members' forwards", samples=args.samples,
                              tile_us=_stats(times[way]), max_abs_difference_between_ways=dev)), flush=True)

    # ---- (b) one active-selection call
    L_, num_pairs, factor = 100, 50, 2.0
    r = np.random.default_rng(0)
    trajs = [TrajectoryWithRew(obs=r.normal(size=(501, od)).astype(np.float32),
                               acts=r.uniform(-1, 1, (500, ad)).astype(np.float32), infos=None, terminal=True,
                               rews=r.normal(size=500).astype(np.float32)) for _ in range(40)]
    logger = p.configure_logger(format_strs=[])
    frs = {}
    for way, flag in WAYS:
        os.environ["IA_ENSEMBLE_FUSED"] = flag
        pm = pc.PreferenceModel(make_ensemble(p, th, obs_space, act_space, M))
        frs[way] = pc.ActiveSelectionFragmenter(pm, pc.RandomFragmenter(np.random.default_rng(1), custom_logger=logger),
                                                factor, uncertainty_on="logit", custom_logger=logger)
    pairs = pc.RandomFragmenter(np.random.default_rng(2), custom_logger=logger)(trajs, L_, int(factor * num_pairs))

    def select(way, flag, whole):
        os.environ["IA_ENSEMBLE_FUSED"] = flag
        sync()
        t0 = time.perf_counter()
        if whole:
            frs[way](trajs, L_, num_pairs)
        else:
            frs[way].variance_estimates(pairs)      # (ends in the read-back of the estimates)
        return 1e6 * (time.perf_counter() - t0)

    times = {(way, whole): [] for way, _ in WAYS for whole in (False, True)}
    for k in range(args.warmup + args.samples):
        for whole in (False, True):
            for way, flag in WAYS:
                us = select(way, flag, whole)
                if k >= args.warmup:
                    times[(way, whole)].append(us)
    for way, _ in WAYS:
        print(json.dumps(dict(bench="ensemble", workload="active_selection", way=way, fragment_length=L_,
                              candidate_pairs=int(factor * num_pairs), num_pairs=num_pairs, members=M, uncertainty_on="logit",
                              samples=args.samples, score_us=_stats(times[(way, False)]),
                              call_us=_stats(times[(way, True)]))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the run ends itself")
    args = ap.parse_args()
    signal.alarm(args.limit)
    bench(args)


if __name__ == "__main__":
    main()
