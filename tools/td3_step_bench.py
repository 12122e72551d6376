"""Whole `TD3.train` calls of SQIL on the GPU (`imitation_amd/td3.py`, `csrc/td3.hip`): microseconds per gradient step,
including the index and noise draws, the two uploads, the launches and the read-back of the statistics (the call's only
synchronisation). One JSON line per configuration:

  python tools/td3_step_bench.py       # the Pendulum shape (D = 3, A = 1) and config P's shape (D = 17, A = 6), net
                                       # [400, 300], batch 100, each with gradient_steps 1 and 64

The four configurations take turns, sample by sample, so that drift of the machine lands on all of them alike; warm-up calls
first, then `--samples` samples each; median and the 10th / 90th percentile are reported. `launches` is counted from the
code, not measured: the C-ABI calls of one step as `TD3Policy.update` makes them, each weighted with the launches
`ia_mlp_forward` / `ia_mlp_backward` make for that stack (csrc/mlp.hip: one per layer forwards; backwards two per layer --
weight gradient and input gradient -- but one for a single-output head and one for the first layer when no dX is asked).
The whole run ends itself after `--limit` seconds.
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


def make(D, A, arch, n_demo=1024, ring=4096):
    import torch as th

    import imitation_amd as p
    venv = p.SyntheticVecEnv(num_envs=1, obs_dim=D, act_dim=A, horizon=50, prefetch_noise=False)
    r = np.random.default_rng(0)
    demos = p.Transitions(obs=r.normal(size=(n_demo, D)).astype(np.float32),
                          acts=r.uniform(-1, 1, (n_demo, A)).astype(np.float32),
                          next_obs=r.normal(size=(n_demo, D)).astype(np.float32), dones=r.uniform(size=n_demo) < 0.05)
    th.manual_seed(0)
    algo = p.SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_algo_class=p.TD3,
                  rl_kwargs=dict(buffer_size=ring, policy_kwargs=dict(net_arch=list(arch))))
    rl = algo.rl_algo
    rl._logger = p.logger.Logger(None, [])
    for _ in range(ring):
        o = r.normal(size=(1, D)).astype(np.float32)
        rl.replay_buffer.add(o, (0.9 * o).astype(np.float32), r.uniform(-1, 1, (1, A)).astype(np.float32),
                             np.zeros(1, np.float32), r.uniform(size=1) < 0.05, [{}])
    return rl


def count_launches(rl, batch_size):
    """Launches of a step without and with the actor update, from the calls `TD3Policy.update` makes in a two-step call."""
    from imitation_amd import _lib as L

    def mlp_launches(name, args):
        desc = args[0]._obj   # (the structure behind `ctypes.byref`)
        n = desc.n_layers
        if name == "ia_mlp_forward":
            return n
        dX = args[10]
        total = 0
        for layer in range(n):
            if desc.dims[layer + 1] == 1 and layer > 0:
                total += 1
            else:
                total += 2 if (layer > 0 or dX is not None) else 1
        return total

    per_step, orig = [], L.call

    def counting(name, *args):
        if name == "ia_td3_assemble":
            per_step.append(0)
        per_step[-1] += mlp_launches(name, args) if name in ("ia_mlp_forward", "ia_mlp_backward") else 1
        return orig(name, *args)

    L.call = counting
    try:
        before = rl._n_updates
        rl.train(gradient_steps=2, batch_size=batch_size)
    finally:
        L.call = orig
    flags = rl.last_actor_steps
    assert len(per_step) == 2 and sorted(flags) == [False, True] and rl._n_updates == before + 2
    return dict(critic_only=per_step[flags.index(False)], with_actor=per_step[flags.index(True)])


def bench(args):
    import torch as th
    np.random.seed(0)
    th.manual_seed(0)
    configs = [(D, A, gs) for D, A in ((3, 1), (17, 6)) for gs in (1, 64)]
    learners = {(D, A): make(D, A, args.arch) for D, A in ((3, 1), (17, 6))}
    launches = {k: count_launches(rl, args.batch) for k, rl in learners.items()}

    def call(D, A, gs):
        rl = learners[(D, A)]
        th.cuda.synchronize()
        t0 = time.perf_counter()
        rl.train(gradient_steps=gs, batch_size=args.batch)
        return 1e6 * (time.perf_counter() - t0) / gs

    for _ in range(args.warmup):
        for c in configs:
            call(*c)
    t = {c: [] for c in configs}
    for i in range(args.samples):
        for c in (configs if i % 2 == 0 else configs[::-1]):
            t[c].append(call(*c))
    for D, A, gs in configs:
        print(json.dumps(dict(bench="td3_train_call", obs_dim=D, act_dim=A, net_arch=list(args.arch), batch_size=args.batch,
                              gradient_steps=gs, policy_delay=2, samples=args.samples, launches=launches[(D, A)],
                              us_per_step=_stats(t[(D, A, gs)]))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--arch", type=int, nargs="*", default=[400, 300])
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    signal.alarm(a.limit)
    bench(a)
