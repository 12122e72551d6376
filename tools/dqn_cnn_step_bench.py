"""`DQN.train` with a `CnnPolicy` on the GPU (`DQNPolicy.update_frames`, `csrc/dqn_frames.hip`): the time per gradient step
at SB3's Atari shape -- frames (4, 84, 84), 6 actions, batch 32, NatureCNN(512) -- from the uint8 device ring. One JSON line:

  python tools/dqn_cnn_step_bench.py                    # one warm-up call, then 20 timed `train` calls of 64 steps
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/dqn_cnn_step_bench.py --samples 3   # the kernels' device times

A timed sample is one whole `train(gradient_steps=64)` call -- its index draws, the host check of the rows, the one index
upload, 64 launch sequences, the read-back of the statistics (the call's only synchronisation) -- after a synchronise, so
nothing earlier is counted; reported are the median and the 10th / 90th percentile of the microseconds per gradient step
(call time / 64), and the bytes `ia_dqn_assemble_u8` moves per step (2 B frame_bytes read and as many written). The run ends
itself after `--limit` seconds.
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


def make(shape, A, n_envs=8, ring=1024):
    import torch as th

    import imitation_amd as p
    from imitation_amd.vec_env import SyntheticImageVecEnv
    venv = SyntheticImageVecEnv(num_envs=n_envs, shape=shape, act_dim=2, horizon=50, n_discrete=A)
    th.manual_seed(0)
    rl = p.DQN("CnnPolicy", venv, buffer_size=ring, learning_rate=1e-4)
    rl._logger = p.logger.Logger(None, [])
    r = np.random.default_rng(0)
    for _ in range(ring // n_envs):
        o, o2 = (r.integers(0, 256, size=(n_envs,) + shape, dtype=np.uint8) for _ in range(2))
        rl.replay_buffer.add(o, o2, r.integers(0, A, n_envs), r.normal(size=n_envs).astype(np.float32),
                             r.uniform(size=n_envs) < 0.05, [{}] * n_envs)
    return rl


def bench(args):
    import torch as th
    np.random.seed(0)
    shape, A, B, G = (4, 84, 84), 6, args.batch, args.steps
    rl = make(shape, A)

    def call():
        th.cuda.synchronize()
        t0 = time.perf_counter()
        rl.train(gradient_steps=G, batch_size=B)
        return 1e6 * (time.perf_counter() - t0) / G

    for _ in range(args.warmup):
        call()
    t = np.asarray([call() for _ in range(args.samples)])
    fb = int(np.prod(shape))
    assert np.isfinite(rl.last_train_stats).all()
    print(json.dumps(dict(bench="dqn_cnn_train_call", frames=list(shape), n_actions=A, batch_size=B, gradient_steps=G,
                          samples=args.samples, us_per_step=dict(median=float(np.median(t)), p10=float(np.percentile(t, 10)),
                                                                 p90=float(np.percentile(t, 90))),
                          assemble_bytes_per_step=2 * 2 * B * fb, parameters=int(rl.policy.q_net._flat.numel()))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    signal.alarm(a.limit)
    bench(a)
