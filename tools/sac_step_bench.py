"""Whole `SAC.train` calls of SQIL on the GPU (`imitation_amd/sac.py`, `csrc/sac.hip`) with `TD3.train` at the same shapes
beside them for scale: microseconds per gradient step, including the index and `eps` draws, the two uploads, the launches and
the read-back of the statistics (the call's only synchronisation). One JSON line per configuration:

  python tools/sac_step_bench.py       # SAC's defaults (D = 17, A = 6) and the SQIL tutorial's Pendulum shape (D = 3, A = 1),
                                       # net [256, 256], batch 256, gradient_steps 64, SAC and TD3

`us_per_step` is host wall-clock around the call, `event_us_per_step` the time between two events recorded on the stream
around it. The configurations take turns, sample by sample, so that drift of the machine lands on all of them alike; warm-up
calls first, then `--samples` samples each; median and the 10th / 90th percentile are reported. `launches` is counted from the
code as in `tools/td3_step_bench.py` (SAC updates the actor in every step; TD3's figure is the step with the actor update).
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

from tools.td3_step_bench import _stats, count_launches  # noqa: E402


def make(cls_name, D, A, arch, n_demo=1024, ring=4096):
    import torch as th

    import imitation_amd as p
    venv = p.SyntheticVecEnv(num_envs=1, obs_dim=D, act_dim=A, horizon=50, prefetch_noise=False)
    r = np.random.default_rng(0)
    demos = p.Transitions(obs=r.normal(size=(n_demo, D)).astype(np.float32),
                          acts=r.uniform(-1, 1, (n_demo, A)).astype(np.float32),
                          next_obs=r.normal(size=(n_demo, D)).astype(np.float32), dones=r.uniform(size=n_demo) < 0.05)
    th.manual_seed(0)
    algo = p.SQIL(venv=venv, demonstrations=demos, policy="MlpPolicy", rl_algo_class=getattr(p, cls_name),
                  rl_kwargs=dict(buffer_size=ring, policy_kwargs=dict(net_arch=list(arch))))
    rl = algo.rl_algo
    rl._logger = p.logger.Logger(None, [])
    for _ in range(ring):
        o = r.normal(size=(1, D)).astype(np.float32)
        rl.replay_buffer.add(o, (0.9 * o).astype(np.float32), r.uniform(-1, 1, (1, A)).astype(np.float32),
                             np.zeros(1, np.float32), r.uniform(size=1) < 0.05, [{}])
    return rl


def sac_launches(rl, batch_size):
    """Launches of one SAC step, from the calls `SACPolicy.update` makes (every step is the same)."""
    from imitation_amd import _lib as L

    counts, orig = [], L.call

    def counting(name, *args):
        if name == "ia_td3_assemble":
            counts.append(0)
        if name in ("ia_mlp_forward", "ia_mlp_backward"):
            desc, n = args[0]._obj, args[0]._obj.n_layers
            if name == "ia_mlp_forward":
                counts[-1] += n
            else:
                dX = args[10]
                counts[-1] += sum(1 if (desc.dims[k + 1] == 1 and k > 0) else (2 if (k > 0 or dX is not None) else 1)
                                  for k in range(n))
        else:
            counts[-1] += 1
        return orig(name, *args)

    L.call = counting
    try:
        rl.train(gradient_steps=2, batch_size=batch_size)
    finally:
        L.call = orig
    assert len(counts) == 2 and counts[0] == counts[1]
    return counts[0]


def bench(args):
    import torch as th
    np.random.seed(0)
    th.manual_seed(0)
    shapes = ((17, 6), (3, 1))
    configs = [(cls, D, A) for D, A in shapes for cls in ("SAC", "TD3")]
    learners = {c: make(*c, args.arch) for c in configs}
    launches = {c: (sac_launches(rl, args.batch) if c[0] == "SAC" else count_launches(rl, args.batch)["with_actor"])
                for c, rl in learners.items()}
    gs = args.steps

    def call(c):
        rl = learners[c]
        th.cuda.synchronize()
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        rl.train(gradient_steps=gs, batch_size=args.batch)
        e1.record()
        wall = 1e6 * (time.perf_counter() - t0) / gs
        e1.synchronize()
        return wall, 1e3 * e0.elapsed_time(e1) / gs

    for _ in range(args.warmup):
        for c in configs:
            call(c)
    t = {c: [] for c in configs}
    for i in range(args.samples):
        for c in (configs if i % 2 == 0 else configs[::-1]):
            t[c].append(call(c))
    for c in configs:
        cls, D, A = c
        print(json.dumps(dict(bench="sac_train_call", learner=cls, obs_dim=D, act_dim=A, net_arch=list(args.arch),
                              batch_size=args.batch, gradient_steps=gs, samples=args.samples, launches=launches[c],
                              us_per_step=_stats([x[0] for x in t[c]]), event_us_per_step=_stats([x[1] for x in t[c]]))),
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--arch", type=int, nargs="*", default=[256, 256])
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    signal.alarm(a.limit)
    bench(a)
