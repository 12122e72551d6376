"""Reward-model training on preference comparisons (`imitation_amd/preference_comparisons.py`, `csrc/pref.hip`):
`BasicRewardTrainer.train` at the training script's defaults -- `BasicRewardNet` (32, 32) + `RunningNorm`, 17 + 6
inputs, fragments of 100 steps, batch 32 -- timed with device events. One JSON line per configuration on stdout.

  python tools/pref_reward_bench.py            # 500 comparisons x 600 epochs, and 5 000 comparisons x 3 epochs
  python tools/pref_reward_bench.py --quick    # 500 comparisons x 20 epochs (under rocprofv3 --kernel-trace)

FLOPs per optimiser step (32 pairs = 6 400 rows, D = 23): forward 2 * (23*32 + 32*32 + 32) per row, backward twice that
(input gradient of layer 0 skipped), about 69 MFLOP in all.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _dataset(n_pairs, L=100, obs_dim=17, act_dim=6, seed=0):
    from imitation_amd import data_types as dt
    from imitation_amd import preference_comparisons as pc
    g = np.random.default_rng(seed)

    def frag():
        return dt.TrajectoryWithRew(obs=g.standard_normal((L + 1, obs_dim)).astype(np.float32),
                                    acts=g.uniform(-1, 1, (L, act_dim)).astype(np.float32),
                                    rews=g.standard_normal(L).astype(np.float32), infos=None, terminal=False)

    ds = pc.PreferenceDataset()
    ds.push([(frag(), frag()) for _ in range(n_pairs)], g.integers(0, 2, n_pairs).astype(np.float32))
    return ds


def run(n_pairs, epochs, launches_per_step):
    import torch as th

    import imitation_amd as p
    from imitation_amd import preference_comparisons as pc
    th.manual_seed(0)
    obs, act = p.Box(-np.inf, np.inf, (17,), np.float32), p.Box(-1.0, 1.0, (6,), np.float32)
    net = p.BasicRewardNet(obs, act, normalize_input_layer=p.RunningNorm).to("cuda")
    ds = _dataset(n_pairs)
    trainer = pc.BasicRewardTrainer(pc.PreferenceModel(net), pc.CrossEntropyRewardLoss(), np.random.default_rng(0),
                                    batch_size=32, epochs=1, custom_logger=p.configure_logger(format_strs=[]))
    trainer.train(ds, epoch_multiplier=1)   # warm-up: device table, workspaces
    th.cuda.synchronize()
    steps = epochs * -(-n_pairs // 32)
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    trainer.train(ds, epoch_multiplier=epochs)
    e1.record()
    th.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev_ms = e0.elapsed_time(e1)
    out = {"comparisons": n_pairs, "epochs": epochs, "optimiser_steps": steps, "call_wall_ms": round(wall * 1e3, 2),
           "call_device_ms": round(dev_ms, 2), "us_per_step_device": round(dev_ms * 1e3 / steps, 2),
           "us_per_step_wall": round(wall * 1e6 / steps, 2), "launches_per_step": launches_per_step}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    # per minibatch of the default net with RunningNorm: gather, fragment moments, sequential merge, count, apply,
    # forward (3), loss, backward (4), reduction + AdamW -- counted in the kernel trace of the --quick run
    # (profiles/preference_reward.md)
    launches = 14
    if a.quick:
        run(500, 20, launches)
        return
    run(500, 600, launches)
    run(5000, 3, launches)


if __name__ == "__main__":
    main()
