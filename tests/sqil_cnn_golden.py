"""What the image-SQIL fixtures' generator (`tests/golden/make_golden_sqil_cnn.py`) and their tests share: the cases, the
environment, the uint8 demonstrations and the seeding of a run, and `run_case`, which runs THIS package's
`SQIL(policy="CnnPolicy")` on a case and records what the fixtures record. Frames are never stored: every ring write is
recorded as `zlib.crc32` of its `obs` rows and of its `next_obs` rows (read back from the device ring here), the
demonstrations as one CRC (the tests regenerate them from the seed)."""
import zlib

import numpy as np

from imitation_amd.vec_env import SyntheticImageVecEnv
from tests.sqil_golden import COMMON, GAP_MARGIN, Recorder, seed_everything  # noqa: F401

CASES = {
    # the smallest valid NatureCNN input (a 1 x 1 final map), the implicit first layer on a 4-frame stack
    "sqil_cnn_min": dict(frames=(4, 36, 36), n_actions=3, batch_size=8, gradient_steps=1, features_dim=64),
    # three channels (whatever path the policy takes outside the 4-frame stack); maps 10 x 11, 4 x 4, 2 x 2: a column no
    # window of the second convolution reaches, a final map with H != W (the (h, w, c) / (c, h, w) permutations)
    "sqil_cnn_wide_map": dict(frames=(3, 44, 48), n_actions=4, batch_size=7, gradient_steps=2, features_dim=32),
}


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a, np.uint8).tobytes())


def make_env(cfg, seed):
    return SyntheticImageVecEnv(num_envs=cfg["n_envs"], shape=tuple(cfg["frames"]), act_dim=2, horizon=cfg["horizon"],
                                seed=100 + seed, n_discrete=cfg["n_actions"])


def make_demos(cfg, seed):
    """Plain arrays (the caller wraps them in its own `Transitions`): uint8 obs, acts, uint8 next_obs, dones."""
    r = np.random.default_rng(500 + seed)
    n, shape = cfg["n_demo"], tuple(cfg["frames"])
    obs = r.integers(0, 256, size=(n,) + shape, dtype=np.uint8)
    nxt = r.integers(0, 256, size=(n,) + shape, dtype=np.uint8)
    acts = r.integers(0, cfg["n_actions"], size=n).astype(np.int64)
    dones = r.uniform(size=n) < 0.2
    return obs, acts, nxt, dones


def demo_crc(cfg, seed) -> int:
    obs, _, nxt, _ = make_demos(cfg, seed)
    return crc(np.concatenate([obs.reshape(-1), nxt.reshape(-1)]))


def rl_kwargs_of(cfg):
    return dict(learning_rate=cfg["learning_rate"], buffer_size=cfg["buffer_size"], learning_starts=cfg["learning_starts"],
                batch_size=cfg["batch_size"], tau=cfg["tau"], gamma=cfg["gamma"], train_freq=cfg["train_freq"],
                gradient_steps=cfg["gradient_steps"], target_update_interval=cfg["target_update_interval"],
                exploration_fraction=cfg["exploration_fraction"], exploration_initial_eps=cfg["exploration_initial_eps"],
                exploration_final_eps=cfg["exploration_final_eps"], max_grad_norm=cfg["max_grad_norm"],
                policy_kwargs=dict(features_extractor_kwargs=dict(features_dim=cfg["features_dim"])))


class CnnRecorder(Recorder):
    """`sqil_golden.Recorder` plus: the `update_frames` counter, the CRCs of every ring write as the DEVICE ring holds it,
    and the online parameters as they stood at the latest target update."""

    def __init__(self, algo):
        super().__init__(algo)
        rl = algo.rl_algo
        rb, pol = rl.replay_buffer, rl.policy
        self.path_calls["frames"] = 0
        self.crc_obs, self.crc_next = [], []
        self.target_snapshot = None
        frames_fn, add_fn, polyak_fn = pol.update_frames, rb.add, pol.polyak_update

        def update_frames(*a, **k):
            self.path_calls["frames"] += 1
            return frames_fn(*a, **k)

        def add(obs, next_obs, action, reward, done, infos):
            pos, n = rb.pos, rb.n_envs
            add_fn(obs, next_obs, action, reward, done, infos)
            self.crc_obs.append(crc(rb.table.obs[pos * n:(pos + 1) * n].cpu().numpy()))
            self.crc_next.append(crc(rb.table.next_obs[pos * n:(pos + 1) * n].cpu().numpy()))

        def polyak(tau):
            self.target_snapshot = {k: v.clone() for k, v in pol.q_net.state_dict().items()}
            return polyak_fn(tau)

        pol.update_frames, rb.add, pol.polyak_update = update_frames, add, polyak

    def record(self):
        out = super().record()
        for k in ("ring_obs", "ring_next_obs", "table_obs", "table_next_obs"):
            out.pop(k)
        out["ring_obs_crc"] = np.array(self.crc_obs, np.int64)
        out["ring_next_obs_crc"] = np.array(self.crc_next, np.int64)
        out["frames_calls"] = np.int64(self.path_calls["frames"])
        for k, v in (self.target_snapshot or {}).items():
            out[f"target_snapshot/{k}"] = v.cpu().numpy()
        return out


def build(cfg, seed, device="cuda"):
    """This package's SQIL on a case, seeded as the fixture's run was; returns (algo, recorder)."""
    import imitation_amd as p

    venv = make_env(cfg, seed)
    obs, acts, nxt, dones = make_demos(cfg, seed)
    demos = p.Transitions(obs=obs, acts=acts, next_obs=nxt, dones=dones)
    seed_everything(venv, seed)
    algo = p.SQIL(venv=venv, demonstrations=demos, policy="CnnPolicy", rl_kwargs=dict(rl_kwargs_of(cfg), device=device))
    return algo, CnnRecorder(algo)


def run_case(name, seed, device="cuda"):
    cfg = dict(COMMON, **CASES[name])
    algo, rec = build(cfg, seed, device)
    init = {f"init/{k}": v.cpu().numpy() for k, v in algo.policy.state_dict().items()}
    algo.train(total_timesteps=cfg["total_timesteps"], log_interval=cfg["log_interval"])
    return dict(rec.record(), **init)
