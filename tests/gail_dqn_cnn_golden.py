"""What the fixtures of GAIL over a DQN `CnnPolicy` generator (`tests/golden/make_golden_gail_dqn_cnn.py`) and their tests
share: the cases, the environment, the uint8 demonstrations, the seeding of a run, and `run_case`, which runs THIS package's
`GAIL(gen_algo=DQN("CnnPolicy"), reward_net=modules.CnnRewardNet(hwc_format=False))` on a case and records what the
fixtures record. Frames are never stored: every learner-ring write, the trainer's replay ring after every round and the
demonstrations are `zlib.crc32` values (`frames_to_crc`). `python -m tests.gail_dqn_cnn_golden CASE SEED OUT.npz` writes one
record (the tests use it to run a case in a fresh process with `IA_OFFPOLICY_FUSED=0`)."""
import sys
import zlib

import numpy as np

from tests import gail_offpolicy_golden as go
from tests import sqil_cnn_golden as sc
from tests import sqil_golden as sq

GAP_MARGIN = go.GAP_MARGIN
BRANCH = go.BRANCH
NOT_COMPARED_PREFIX = go.NOT_COMPARED_PREFIX

# `gail_offpolicy_golden.COMMON` (without its MLP tower) plus the keys of `sqil_golden.COMMON` the image learner is built from
IMAGE_KEYS = ("tau", "max_grad_norm", "gradient_steps", "exploration_fraction", "exploration_initial_eps",
              "exploration_final_eps")
COMMON = dict({k: sq.COMMON[k] for k in IMAGE_KEYS}, **{k: v for k, v in go.COMMON.items() if k != "net_arch"}, algo="DQN")
CASES = {
    # the smallest valid NatureCNN input, two 4 KB chunks per frame, 16-byte aligned rows
    "gail_dqn_cnn_min": dict(frames=(4, 36, 36), n_actions=3, features_dim=64, flags=[True, True, False, False]),
    # three channels, H != W, an odd batch; the CNN reads state and next state, its output has 2 * n_actions entries
    "gail_dqn_cnn_next_done": dict(frames=(3, 44, 48), n_actions=4, batch_size=7, features_dim=32,
                                   flags=[True, True, True, True]),
}

crc = sc.crc
make_env = sc.make_env
make_demos = sc.make_demos
demo_crc = sc.demo_crc
rl_kwargs_of = sc.rl_kwargs_of
seed_everything = go.seed_everything


def tensor_crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a, np.float32).tobytes())


def frames_to_crc(rec):
    """A record with its frame arrays replaced by CRCs: `ring_obs` / `ring_next_obs` one per ring write, `gen_obs` /
    `gen_next_obs` one per round (the whole ring in its space's dtype); the learner's initial online parameters as one
    CRC per tensor; the target net dropped (initially equal to the online net, finally the online net at the last target
    update)."""
    out = {}
    for k, v in rec.items():
        if k in ("ring_obs", "ring_next_obs", "gen_obs", "gen_next_obs"):
            out[k + "_crc"] = np.array([crc(np.asarray(a).astype(np.uint8)) for a in v], np.int64)
        elif k.startswith(("init/q_net_target.", "final/q_net_target.")):
            continue
        elif k.startswith("init/"):
            out["init_crc/" + k[len("init/"):]] = np.int64(tensor_crc(v))
        else:
            out[k] = v
    return out


class CnnRecorder(go.Recorder):
    """`gail_offpolicy_golden.Recorder` plus the frame path's launch counters."""

    def record(self):
        out = super().record()
        tr = self.trainer
        src = tr._step_source
        out["reward_launches"] = np.int64(-1 if src is None else getattr(src, "reward_launches", -1))
        out["gather_launches"] = np.int64(tr.frame_gather_launches)
        out["frame_path"] = np.int64(bool(tr._frame_path))
        return out


def build(cfg, seed, device="cuda"):
    """This package's GAIL on a case, seeded as the fixture's run was; returns (trainer, recorder)."""
    import tempfile

    import imitation_amd as p

    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = p.Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones)
    seed_everything(venv, seed)
    rl = p.DQN("CnnPolicy", venv, device=device, **rl_kwargs_of(cfg))
    f = cfg["flags"]
    net = p.modules.CnnRewardNet(venv.observation_space, venv.action_space, use_state=f[0], use_action=f[1],
                                 use_next_state=f[2], use_done=f[3], hwc_format=False)
    trainer = p.GAIL(demonstrations=demos, demo_batch_size=cfg["demo_batch_size"], venv=venv, gen_algo=rl, reward_net=net,
                     n_disc_updates_per_round=cfg["n_disc"], gen_train_timesteps=cfg["gen_train_timesteps"],
                     custom_logger=p.configure_logger(tempfile.mkdtemp(), []), allow_variable_horizon=False)
    return trainer, CnnRecorder(trainer, cfg)


def run_case(name, seed, device="cuda"):
    cfg = dict(COMMON, **CASES[name])
    trainer, rec = build(cfg, seed, device)
    init = {f"init/{k}": v.cpu().numpy() for k, v in trainer.gen_algo.policy.state_dict().items()}
    init.update({f"disc_init/{k}": v.cpu().numpy() for k, v in trainer._reward_net.state_dict().items()})
    trainer.train(cfg["rounds"] * cfg["gen_train_timesteps"], callback=rec.end_of_round)
    return frames_to_crc(dict(rec.record(), **init))


if __name__ == "__main__":
    np.savez(sys.argv[3], **run_case(sys.argv[1], int(sys.argv[2])))
