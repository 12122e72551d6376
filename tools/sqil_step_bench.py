"""One `DQN.train` call of SQIL on the GPU (`imitation_amd/dqn.py`, `csrc/dqn.hip`): the fused one-launch update against
the general path (the same steps from `ia_gather_rows` / `ia_mlp_forward` / `ia_dqn_td_loss` / `ia_mlp_backward` / ...),
alternating in one process. One JSON line per configuration:

  python tools/sqil_step_bench.py      # CartPole shape (D = 4, A = 2, H = 64, batch 32) and D = 64, A = 16, batch 256,
                                       # each with gradient_steps 1 and 16

A timed sample is one whole `train` call -- its index draws, the one index upload, the launches, the read-back of the
statistics (which is the call's only synchronisation) -- after a synchronise, so nothing earlier is counted. Warm-up calls
first, then `--samples` samples per side, interleaved; median and the 10th / 90th percentile of the microseconds per
gradient step are reported, and the ratio of the medians. The whole run ends itself after `--limit` seconds.
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


def _stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)))


def make(D, A, H, n_envs=8, n_demo=1024, ring=4096):
    import torch as th

    import imitation_amd as p
    venv = p.SyntheticVecEnv(num_envs=n_envs, obs_dim=D, act_dim=2, horizon=50, n_discrete=A, prefetch_noise=False)
    r = np.random.default_rng(0)
    demos = p.Transitions(obs=r.normal(size=(n_demo, D)).astype(np.float32), acts=r.integers(0, A, n_demo),
                          next_obs=r.normal(size=(n_demo, D)).astype(np.float32), dones=r.uniform(size=n_demo) < 0.05)
    th.manual_seed(0)
    algo = p.SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy",
                  rl_kwargs=dict(buffer_size=ring, policy_kwargs=dict(net_arch=[H, H])))
    rl = algo.rl_algo
    rl._logger = p.logger.Logger(None, [])
    for _ in range(ring // n_envs):
        o = r.normal(size=(n_envs, D)).astype(np.float32)
        rl.replay_buffer.add(o, (0.9 * o).astype(np.float32), r.integers(0, A, n_envs), np.zeros(n_envs, np.float32),
                             r.uniform(size=n_envs) < 0.05, [{}] * n_envs)
    return rl


def bench(args):
    import torch as th
    np.random.seed(0)
    configs = [(4, 2, 64, 32), (64, 16, 64, 256)]
    if args.sweep:   # where the routing rule (`DQNPolicy.fused_cost_us`) comes from
        configs = [(D, A, 64, B) for D, A in ((4, 2), (64, 16)) for B in (16, 32, 48, 64, 96, 128)]
    for D, A, H, B in configs:
        rl = make(D, A, H)
        default_path = "fused" if rl.policy.fused_ok(B) else "general"
        rl.policy.FUSED_COST_LIMIT_US = float("inf")   # the "fused" side is the kernel itself, whatever the routing says
        for gs in (1, 16):
            def call(fused):
                os.environ["IA_DQN_FUSED"] = "1" if fused else "0"
                assert rl.policy.fused_ok(B) == fused
                th.cuda.synchronize()
                t0 = time.perf_counter()
                rl.train(gradient_steps=gs, batch_size=B)
                return 1e6 * (time.perf_counter() - t0) / gs

            for _ in range(args.warmup):
                call(True), call(False)
            t = {True: [], False: []}
            for i in range(args.samples):
                for fused in ((True, False) if i % 2 == 0 else (False, True)):
                    t[fused].append(call(fused))
            print(json.dumps(dict(bench="sqil_train_call", obs_dim=D, n_actions=A, hidden=H, batch_size=B,
                                  gradient_steps=gs, samples=args.samples, default_path=default_path,
                                  fused_us_per_step=_stats(t[True]),
                                  general_us_per_step=_stats(t[False]),
                                  general_over_fused=float(np.median(t[False]) / np.median(t[True])))), flush=True)
    os.environ.pop("IA_DQN_FUSED", None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="batch sizes 16 .. 128 at both widths instead of the two shapes")
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    signal.alarm(a.limit)
    bench(a)
