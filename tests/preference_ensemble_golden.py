"""What the ensemble fixtures' generator (`tests/golden/make_golden_preference_ensemble.py`) and their test
(`tests/test_preference_ensemble_gpu.py`) share: the settings of the cases and the fixed trajectories. NumPy only."""
import numpy as np

DIFFER_FACTOR = 100.0   # adjacent estimates of a fragmenter call lie further apart than this x the call's f32 deviation
DECISIVE = 1e-4         # `label`: no member probability this close to 0.5

# ---- `ensemble_moments.npz`: the reward nets alone
MOMENTS = dict(obs_dim=5, act_dim=2, n_discrete=3, members=3, alpha=0.5, rows=7, calls=3, seed=11)
MOMENTS_CASES = ("box", "discrete")

# ---- `preference_ensemble_*.npz`: PreferenceComparisons over a TrajectoryDataset, sized like `preference_normalized_queue`
RUNS = {
    "preference_ensemble_logit": dict(obs_dim=5, act_dim=2, discrete=False, members=3, uncertainty_on="logit", factor=2.0,
                                      std_wrapper=True, alpha=0.5, n_traj=10, horizon=25, frag=5, iters=2, comparisons=40,
                                      batch=6, mb=3, epochs=1, init_mult=2.0, gamma=1.0, noise=0.0, queue=14,
                                      probability_case=True),
    "preference_ensemble_label": dict(obs_dim=5, act_dim=3, discrete=True, members=5, uncertainty_on="label", factor=2.0,
                                      std_wrapper=False, alpha=0.0, n_traj=10, horizon=25, frag=5, iters=2, comparisons=40,
                                      batch=6, mb=3, epochs=1, init_mult=2.0, gamma=0.9, noise=0.1, queue=14,
                                      probability_case=False),
}
PROBABILITY_CASE = dict(num_pairs=6, rng_seed=77)   # one more fragmenter call on the final member states of the logit run


def make_trajectories(cfg, seed):
    """Fixed trajectories: (obs, acts, rews) drawn from their own generator (rewards correlate with the first observation
    column, so the preferences carry signal)."""
    r = np.random.default_rng(1000 + seed)
    out = []
    for _ in range(cfg["n_traj"]):
        T = cfg["horizon"]
        obs = r.normal(size=(T + 1, cfg["obs_dim"])).astype(np.float32)
        if cfg["discrete"]:
            acts = r.integers(cfg["act_dim"], size=T).astype(np.int64)
        else:
            acts = r.uniform(-1, 1, size=(T, cfg["act_dim"])).astype(np.float32)
        rews = (obs[:-1, 0] + 0.3 * r.normal(size=T)).astype(np.float32)
        out.append((obs, acts, rews))
    return out


def moments_inputs(discrete: bool, cfg=MOMENTS):
    """Per call (state, action, next_state, done) of `rows` rows; one more set for the final `predict_processed_all`."""
    r = np.random.default_rng(cfg["seed"] + int(discrete))
    out = []
    for _ in range(cfg["calls"] + 1):
        n = cfg["rows"]
        act = r.integers(0, cfg["n_discrete"], n) if discrete else r.uniform(-1, 1, (n, cfg["act_dim"])).astype(np.float32)
        out.append((r.normal(size=(n, cfg["obs_dim"])).astype(np.float32) * 2, act,
                    r.normal(size=(n, cfg["obs_dim"])).astype(np.float32), r.uniform(size=n) < 0.3))
    return out
