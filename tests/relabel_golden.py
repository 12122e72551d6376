"""What the relabel fixtures' generator (`tests/golden/make_golden_relabel.py`) and their tests share: the settings of the
buffer cases and of the two-phase SAC run. The environment, the seeding, the SAC settings' translation and the thinning rule
are `tests/sac_golden.py`'s (and through it `tests/td3_golden.py`'s)."""
import numpy as np

from tests.sac_golden import COMMON

# ---- `relabel_buffer.npz`: the buffer alone
BUFFER = dict(n_envs=2, obs_dim=5, act_dim=2, n_discrete=3, buffer_size=64, n_adds=40, terminal_at=(12, 0), truncated_at=(19, 1),
              batch=7, n_samples=3, np_seed=31, flags=(True, True, True, True))
BUFFER_CASES = ("box", "discrete")

# ---- `relabel_sac_two_phase.npz`: SAC under the wrapper, the reward net's parameters replaced between two `learn` calls
TWO_PHASE = dict(COMMON, n_envs=2, obs_dim=5, act_dim=2, horizon=8, train_freq=2, gradient_steps=2, net_arch=[32, 32],
                 batch_size=7, learning_starts=8, buffer_size=256, target_update_interval=2, phase_timesteps=40,
                 flags=(True, True, True, True))
DIFFER_FACTOR = 100.0   # phase-2 rewards of phase-1 rows: the two parameter sets differ by more than this x the f32 deviation


def reward_net_kwargs(flags):
    return dict(use_state=flags[0], use_action=flags[1], use_next_state=flags[2], use_done=flags[3])


def buffer_adds(discrete: bool, cfg=BUFFER):
    """The adds of a buffer case: per add (obs, next_obs, action, env reward, done, infos)."""
    r = np.random.default_rng(17 + int(discrete))
    n, out = cfg["n_envs"], []
    for i in range(cfg["n_adds"]):
        done = np.zeros(n, bool)
        infos = [{} for _ in range(n)]
        for (at, env), truncated in ((cfg["terminal_at"], False), (cfg["truncated_at"], True)):
            if i == at:
                done[env] = True
                infos[env] = {"TimeLimit.truncated": truncated}
        act = r.integers(0, cfg["n_discrete"], n) if discrete else r.uniform(-1, 1, (n, cfg["act_dim"])).astype(np.float32)
        out.append((r.normal(size=(n, cfg["obs_dim"])).astype(np.float32), r.normal(size=(n, cfg["obs_dim"])).astype(np.float32),
                    act, r.normal(size=n).astype(np.float32), done, infos))
    return out
