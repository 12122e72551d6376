"""Kernel density reward (`imitation_amd/density.py`, `csrc/kde.hip`): kernel timing, a config-P `train_policy` round, and
the reference's per-row scoring time on the CPU. One JSON line per measurement on stdout.

  python tools/kde_bench.py kernel   # slab kernel and merge alone, device events: ms, pairs/s, fraction of the MFMA bound
  python tools/kde_bench.py round    # train_policy rounds at config P geometry, bulk vs forced per-step, alternating
  python tools/kde_bench.py reference   # CPU only: the reference DensityAlgorithm (sklearn) scoring 256 rows

The bound of the slab kernel is its fp32 MFMA work, N_q * N_d * 2 * 4 ceil(d / 4) FLOP at 157.3 TFLOP/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12


def _demos(n_demo=64000):
    import bench
    cfg = dict(bench.CFG_P)
    cfg["horizon"] = n_demo // 64
    return bench.make_demos(cfg)


def kernel(args):
    import torch as th
    from imitation_amd import _lib as L
    from imitation_amd import density as D
    dev = th.device("cuda")
    g = np.random.default_rng(0)
    for d in (4, 23, 34):
        y = g.standard_normal((64000, d)).astype(np.float32)
        sc = D.StandardScaler().fit(y)
        for kern in ("gaussian", "epanechnikov"):
            model = D.KdeModel([y], sc, kern, 0.5, dev)
            for nq in (1024, 16384):
                q = th.as_tensor(y[g.integers(0, 64000, nq)] + 0.1 * g.standard_normal((nq, d)).astype(np.float32)).to(dev)
                out = th.empty(nq, dtype=th.float32, device=dev)
                tiles = th.as_tensor(model._tile_table(np.zeros(nq, np.int32))).to(dev)
                part = th.empty(model.max_slabs, nq, 2, dtype=th.float32, device=dev)

                def run(stages):
                    L.call("ia_kde_log_density", model.code, model.h, d, L.ptr(model.Y), model.ldy, L.ptr(model.ynorm),
                           L.ptr(model.off), L.ptr(model.n_dev), L.ptr(model.gconst), model.max_slabs, L.ptr(q), nq,
                           L.ptr(model.mean), L.ptr(model.scale), None, L.ptr(tiles), int(tiles.shape[0]), L.ptr(part),
                           L.ptr(out), stages, L.stream())

                res = {}
                for stages, name in ((1, "slab_kernel"), (2, "merge"), (3, "both")):
                    for _ in range(args.warmup):
                        run(stages)
                    times = []
                    for _ in range(args.reps):
                        a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                        a.record()
                        run(stages)
                        b.record()
                        b.synchronize()
                        times.append(a.elapsed_time(b))
                    res[name] = float(np.median(times))
                bound_ms = 1e3 * nq * 64000 * 2 * 4 * ((d + 3) // 4) / PEAK_F32_MFMA
                print(json.dumps(dict(what="kde_kernel", d=d, kernel=kern, n_q=nq, n_d=64000, slabs=model.max_slabs,
                                      tile_rows=model.tile_rows, slab_kernel_ms=round(res["slab_kernel"], 4),
                                      merge_ms=round(res["merge"], 4), both_ms=round(res["both"], 4),
                                      pairs_per_s=nq * 64000 / (res["slab_kernel"] * 1e-3), bound_ms=round(bound_ms, 4),
                                      fraction_of_bound=round(bound_ms / res["slab_kernel"], 3))), flush=True)


def round_(args):
    import torch as th
    import bench
    import imitation_amd as p
    from imitation_amd import density as D
    from imitation_amd.vec_env import SyntheticVecEnv
    cfg = dict(bench.CFG_P)
    demos = p.Transitions(**_demos())
    th.manual_seed(0)
    np.random.seed(0)
    venv = SyntheticVecEnv(num_envs=cfg["n_envs"], obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], horizon=cfg["horizon"],
                           seed=0)
    pk = dict(features_extractor_class=p.NormalizeFeaturesExtractor, features_extractor_kwargs=dict(normalize_class=p.RunningNorm))
    algo = p.PPO(p.FeedForward32Policy, venv, n_steps=cfg["n_steps"], batch_size=cfg["ppo_batch"], n_epochs=cfg["n_epochs"],
                 ent_coef=cfg["ent_coef"], learning_rate=cfg["lr"], seed=0, policy_kwargs=pk, device="cuda")
    dens = D.DensityAlgorithm(demonstrations=demos, venv=venv, rng=np.random.default_rng(0), rl_algo=algo,
                              density_type=D.DensityType.STATE_ACTION_DENSITY, kernel_bandwidth=0.5)
    dens.train()
    host_s = [0.0]

    def per_step(*a, **k):
        t0 = time.perf_counter()
        r = dens(*a, **k)
        host_s[0] += time.perf_counter() - t0
        return r

    round_steps = cfg["n_envs"] * cfg["n_steps"]
    rates = {"bulk": [], "per_step": []}
    relabel_ms = {"bulk": [], "per_step": []}
    for i in range(args.warmup + 2 * args.rounds):
        mode = "bulk" if i % 2 == 0 else "per_step"
        dens.venv_wrapped.reward_fn = dens if mode == "bulk" else per_step
        host_s[0] = 0.0
        th.cuda.synchronize()
        t0 = time.perf_counter()
        dens.train_policy(n_timesteps=round_steps)
        th.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        if mode == "bulk":   # the relabelling call alone, on the rollout just collected (device events)
            rb = algo.rollout_buffer
            a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            scratch = th.empty_like(rb.rew)
            a.record()
            dens.relabel_rollout(rb.obs[:rb.buffer_size], rb.clipped, rb.next_fixed, scratch, algo.policy.discrete)
            b.record()
            b.synchronize()
            rel = a.elapsed_time(b)
        else:
            rel = 1e3 * host_s[0]
        if i >= args.warmup:
            rates[mode].append(round_steps / dt_s)
            relabel_ms[mode].append(rel)
    for mode in rates:
        r = np.asarray(rates[mode])
        print(json.dumps(dict(what="kde_round", mode=mode, n_envs=cfg["n_envs"], n_steps=cfg["n_steps"], n_demo=len(demos.obs),
                              rounds=len(r), env_steps_per_s_p10=float(np.percentile(r, 10)),
                              env_steps_per_s_median=float(np.median(r)), env_steps_per_s_p90=float(np.percentile(r, 90)),
                              relabel_ms_median=float(np.median(relabel_ms[mode])))), flush=True)


def reference(args):
    from imitation_amd.vec_env import SyntheticVecEnv
    from tests.golden import make_golden_density as mk
    density, types = mk.install()
    d = _demos()
    n = len(d["obs"])
    demos = types.Transitions(obs=d["obs"], acts=d["acts"], next_obs=d["next_obs"], dones=d["dones"],
                              infos=np.array([{}] * n))
    venv = SyntheticVecEnv(num_envs=1, obs_dim=17, act_dim=6, horizon=1000)
    algo = density.DensityAlgorithm(demonstrations=demos, venv=venv, rng=np.random.default_rng(0),
                                    density_type=density.DensityType.STATE_ACTION_DENSITY, kernel_bandwidth=0.5)
    algo.train()
    idx = np.random.default_rng(0).integers(0, n, 256)
    t0 = time.perf_counter()
    algo(d["obs"][idx], d["acts"][idx], d["next_obs"][idx], np.zeros(256, bool))
    dt_s = time.perf_counter() - t0
    print(json.dumps(dict(what="kde_reference_cpu", device="CPU", n_demo=n, rows=256, seconds=dt_s,
                          ms_per_row=1e3 * dt_s / 256, config_p_round_s_estimate=dt_s / 256 * 16384)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "round", "reference"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    {"kernel": kernel, "round": round_, "reference": reference}[a.mode](a)
