"""Sample-time reward relabelling of a `ReplayBufferRewardWrapper` on the GPU (`imitation_amd/replay_buffer_wrapper.py`,
`csrc/relabel.hip`): one `train` call's relabelling -- all `gradient_steps x batch_size` sampled rows -- in the one
`ia_replay_relabel` launch (fp32 MFMA) against the general kernel `ia_replay_relabel_general` (`IA_RELABEL_FUSED=0`: any
stack, one thread per row in float64), and what share of the whole `train` call it is. One JSON line per configuration:

  python tools/relabel_bench.py     # SAC's defaults (D = 17, A = 6, batch 256) at gradient_steps 1 and 64; TD3's (batch 256,
                                    # one 200-step episode's gradient steps); DQN's (CartPole shape, batch 32, 1 step)

The reward net is the scripts' `NormalizedRewardNet(BasicRewardNet(hid_sizes=(32, 32), normalize_input_layer=RunningNorm),
RunningNorm)` behind `functools.partial(predict_processed, update_stats=False)`. `relabel_us` is the host clock around the
relabelling of one call's (already uploaded) indices, ended by a device synchronise; `train_us` around a whole `train` call
(index draws, uploads, relabelling, update, the read-back of the statistics). The two paths and the configurations take
turns, sample by sample, so that drift of the machine lands on all alike; warm-up first, then `--samples` samples each;
median and the 10th / 90th percentile. The whole run ends itself after `--limit` seconds.
"""
import argparse
import functools
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [   # (name, learner, obs_dim, act_dim / n_actions, batch, gradient_steps)
    ("sac_default_g1", "SAC", 17, 6, 256, 1),
    ("sac_default_g64", "SAC", 17, 6, 256, 64),
    ("td3_episode_g200", "TD3", 17, 6, 256, 200),
    ("dqn_default_g1", "DQN", 4, 2, 32, 1),
]


def _stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)))


def make(kind, D, A, ring=16384):
    import torch as th

    import imitation_amd as p
    from imitation_amd import dqn
    discrete = kind == "DQN"
    venv = p.SyntheticVecEnv(num_envs=1, obs_dim=D, act_dim=2 if discrete else A, horizon=50, prefetch_noise=False,
                             n_discrete=A if discrete else None)
    th.manual_seed(0)
    base = p.BasicRewardNet(venv.observation_space, venv.action_space, normalize_input_layer=p.RunningNorm)
    net = p.NormalizedRewardNet(base, p.RunningNorm).to("cuda")
    rl = getattr(p, kind)("MlpPolicy", venv, buffer_size=ring, replay_buffer_class=p.ReplayBufferRewardWrapper,
                          replay_buffer_kwargs=dict(replay_buffer_class=dqn.ReplayBuffer,
                                                    reward_fn=functools.partial(net.predict_processed, update_stats=False)))
    rl._logger = p.logger.Logger(None, [])
    buf = rl.replay_buffer
    t = buf.replay_buffer.table   # a full ring of random rows
    t.obs.normal_()
    t.next_obs.normal_()
    if discrete:
        t.action.copy_(th.randint(0, A, (t.rows,)))
    else:
        t.action.uniform_(-1, 1)
    t.done.copy_((th.rand(t.rows) < 0.05).float())
    buf.pos, buf.full = 0, True
    return rl


def bench(args):
    import torch as th
    np.random.seed(0)
    th.manual_seed(0)
    learners = {(k, D, A): make(k, D, A) for _, k, D, A, _, _ in CONFIGS}

    def relabel(cfg, fused):
        _, k, D, A, B, G = cfg
        buf = learners[(k, D, A)].replay_buffer
        os.environ["IA_RELABEL_FUSED"] = "1" if fused else "0"
        idx = th.randint(0, buf.relabelled.numel(), (G, B), device="cuda")
        th.cuda.synchronize()
        t0 = time.perf_counter()
        assert buf.relabel_for_train(idx)
        th.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0)

    def train(cfg, fused):
        _, k, D, A, B, G = cfg
        os.environ["IA_RELABEL_FUSED"] = "1" if fused else "0"
        th.cuda.synchronize()
        t0 = time.perf_counter()
        learners[(k, D, A)].train(gradient_steps=G, batch_size=B)
        return 1e6 * (time.perf_counter() - t0)

    runs = [(fn, cfg, fused) for cfg in CONFIGS for fn in (relabel, train) for fused in (True, False)]
    for _ in range(args.warmup):
        for fn, cfg, fused in runs:
            fn(cfg, fused)
    t = {(fn.__name__, cfg[0], fused): [] for fn, cfg, fused in runs}
    for i in range(args.samples):
        for fn, cfg, fused in (runs if i % 2 == 0 else runs[::-1]):
            t[(fn.__name__, cfg[0], fused)].append(fn(cfg, fused))
    for cfg in CONFIGS:
        name, k, D, A, B, G = cfg
        buf = learners[(k, D, A)].replay_buffer
        os.environ["IA_RELABEL_FUSED"] = "1"
        base, out_norm = buf.plan()
        r = {f: _stats(t[("relabel", name, f)]) for f in (True, False)}
        c = {f: _stats(t[("train", name, f)]) for f in (True, False)}
        print(json.dumps(dict(bench="replay_relabel", config=name, learner=k, obs_dim=D, act_dim=A, batch_size=B,
                              gradient_steps=G, rows=G * B, kernel_covers=bool(buf.fused_ok(base, out_norm)),
                              samples=args.samples, relabel_us=dict(fused=r[True], general=r[False]),
                              train_us=dict(fused=c[True], general=c[False]),
                              relabel_share_of_train=dict(fused=r[True]["median"] / c[True]["median"],
                                                          general=r[False]["median"] / c[False]["median"]))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300)
    a = ap.parse_args()
    signal.alarm(a.limit)
    bench(a)
