"""NumPy restatements of the ensemble kernels (`imitation_amd/csrc/ensemble.hip`), shared by the host tests
(`tests/test_reward_ensemble.py`) and the device tests (`tests/test_ensemble_kernels_gpu.py`). NumPy only.

* `np_forward`: a member's forward (gather, input norm, dense stack) at a chosen precision;
* `norm_sequential`: `NormalizedRewardNet.predict_processed` once per step (normalise with the statistics so far, then the
  Chan update of `util/networks.py:111-134`) at a chosen precision;
* `moments_f32`: kernel C, float32, in the kernel's order -- which is NumPy's own order of `mean(-1)` / `var(-1, ddof=1)` on
  a C-contiguous `[R, M]` array below 8 members (from 8 on NumPy's reduction is unrolled eight wide);
* `pair_uncertainty_f32`: kernel D, float32, in the kernel's order (lane-strided partial sums of a 64-lane wave, then the
  xor butterfly); `pair_uncertainty_f64`: `ActiveSelectionFragmenter.variance_estimate` in float64, plain formulas.
"""
import numpy as np

MODES = ("logit", "probability", "label")
F32 = np.float32


def rel(x, ref):
    x, ref = np.asarray(x, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


def ulp_distance(a, b):
    """Distance in float32 units in the last place (finite inputs)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def np_forward(dtype, cols, idx, flags, n_onehot, layers, relu, in_norm):
    """Raw reward of table rows `idx` at `dtype`. `cols` = (obs, action, next_obs, done) host arrays; `layers` =
    [(W, b), ...]; `in_norm` = (mean, var, eps) or None; `relu`: ReLU, else Tanh."""
    obs, action, next_obs, done = cols
    parts = []
    if flags[0]:
        parts.append(obs[idx])
    if flags[1]:
        parts.append(np.eye(n_onehot)[action[idx]] if n_onehot else action[idx])
    if flags[2]:
        parts.append(next_obs[idx])
    if flags[3]:
        parts.append(done[idx][:, None])
    x = np.concatenate(parts, axis=1).astype(dtype)
    if in_norm is not None:
        x = (x - in_norm[0].astype(dtype)) / np.sqrt(in_norm[1].astype(dtype) + dtype(in_norm[2]))
    for k, (W, b) in enumerate(layers):
        x = x @ W.astype(dtype).T + b.astype(dtype)
        if k < len(layers) - 1:
            x = np.maximum(x, dtype(0)) if relu else np.tanh(x)
    return x[:, 0]


def norm_sequential(dtype, raw, T, n, eps, update, mean, var, count):
    """(out [T * n], mean, var, count) after T per-step calls on `raw` (time-major)."""
    raw = np.asarray(raw, dtype).reshape(T, n)
    mean, var, count = dtype(mean), dtype(var), int(count)
    out = np.empty_like(raw)
    for t in range(T):
        out[t] = (raw[t] - mean) / np.sqrt(var + dtype(eps))
        if update:
            b_mean, b_var = raw[t].mean(dtype=dtype), raw[t].var(dtype=dtype)
            tot = dtype(count + n)
            delta = b_mean - mean
            new_mean = mean + delta * dtype(n) / tot
            rv = var * dtype(count) + b_var * dtype(n) + delta * delta * dtype(count) * dtype(n) / tot
            mean, var, count = dtype(new_mean), dtype(rv / tot), count + n
    return out.reshape(-1), mean, var, count


def moments_f32(x, alpha):
    """Kernel C on `x` float32 `[M, R]`: (mean, var, bound), members in index order."""
    x = np.asarray(x, F32)
    M = x.shape[0]
    s = np.zeros(x.shape[1], F32)
    for m in range(M):
        s = s + x[m]
    mu = s / F32(M)
    q = np.zeros(x.shape[1], F32)
    for m in range(M):
        d = x[m] - mu
        q = q + d * d
    var = q / F32(M - 1)
    return mu, var, mu + F32(alpha) * np.sqrt(var)


def _wave_sum_f32(vals):
    """Sum of `vals` as a 64-lane wave forms it: lane l adds elements l, l + 64, ... in order, then the xor butterfly."""
    lanes = np.zeros(64, F32)
    for t, v in enumerate(np.asarray(vals, F32)):
        lanes[t % 64] = lanes[t % 64] + v
    ids = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[ids ^ o]
    return lanes[0]


def _probability(dtype, diff, noise, threshold):
    c = np.minimum(np.maximum(diff, dtype(-threshold)), dtype(threshold))
    mp = dtype(1) / (dtype(1) + np.exp(c))
    return dtype(noise) * dtype(0.5) + (dtype(1) - dtype(noise)) * mp


def member_probabilities_f64(x, P, L, gamma, noise, threshold):
    """`PreferenceModel.probability` of every (pair, member) in float64: `[P, M]`."""
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    r = x.reshape(M, P, 2, L)
    w = np.float64(gamma) ** np.arange(L)
    diff = ((r[:, :, 1] - r[:, :, 0]) * w).sum(-1)
    return _probability(np.float64, diff, noise, threshold).T


def pair_uncertainty_f64(x, P, L, mode, gamma, noise, threshold):
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    r = x.reshape(M, P, 2, L)
    if mode == "logit":
        return (r[:, :, 0].sum(-1) - r[:, :, 1].sum(-1)).var(0, ddof=1)
    probs = member_probabilities_f64(x, P, L, gamma, noise, threshold)
    if mode == "probability":
        return probs.var(1)
    # (the reference forms the estimate of the labels in float32 -- `preds.astype(np.float32).mean()` -- whatever the
    #  precision of the probabilities: on decisive inputs this value is exact)
    p = (probs > 0.5).astype(np.float32).mean(1)
    return p * (F32(1) - p)


def pair_uncertainty_f32(x, P, L, mode, gamma, noise, threshold):
    """Kernel D on `x` float32 `[M, 2 P L]`, in the kernel's order."""
    x = np.asarray(x, F32)
    M = x.shape[0]
    est = np.empty(P, F32)
    w = np.ones(L, F32) if gamma == 1.0 else np.power(F32(gamma), np.arange(L).astype(F32)).astype(F32)
    for p in range(P):
        v = np.zeros(M, F32)
        for m in range(M):
            r1, r2 = x[m, 2 * p * L:2 * p * L + L], x[m, 2 * p * L + L:2 * p * L + 2 * L]
            if mode == "logit":
                v[m] = _wave_sum_f32(r1) - _wave_sum_f32(r2)
            else:
                pr = _probability(F32, _wave_sum_f32(w * (r2 - r1)), noise, threshold)
                v[m] = (F32(1) if pr > F32(0.5) else F32(0)) if mode == "label" else pr
        s = F32(0)
        for m in range(M):
            s = s + v[m]
        mu = s / F32(M)
        if mode == "label":
            est[p] = mu * (F32(1) - mu)
            continue
        q = F32(0)
        for m in range(M):
            d = v[m] - mu
            q = q + d * d
        est[p] = q / F32(M - 1 if mode == "logit" else M)
    return est


def active_selection_f64(state, trajs, picks, n_members, frag_len, mode, gamma, noise, threshold=50.0, n_onehot=0,
                         eps=1e-5):
    """One `ActiveSelectionFragmenter` scoring in float64 from member states `state` (the ensemble's `state_dict` as host
    arrays: the reference's default member, `NormalizedRewardNet(BasicRewardNet(32, 32), RunningNorm)`, state and action in,
    ReLU) on the candidate fragments `picks` `[2 F, 2]` = (trajectory, start) of `trajs` = [(obs, acts), ...]: every member
    scores fragment after fragment (normalise with its output statistics so far, then absorb the fragment).
    Returns (estimates [F], the members' (mean, var) afterwards [M, 2], their counts [M])."""
    obs = np.concatenate([trajs[k][0][s:s + frag_len] for k, s in picks])
    nxt = np.concatenate([trajs[k][0][s + 1:s + frag_len + 1] for k, s in picks])
    act = np.concatenate([trajs[k][1][s:s + frag_len] for k, s in picks])
    rows = np.arange(len(obs))
    cols = (obs, act, nxt, np.zeros(len(obs), np.float32))
    F = len(picks) // 2
    x, stats, counts = np.empty((n_members, len(obs))), np.empty((n_members, 2)), np.empty(n_members, np.int64)
    for m in range(n_members):
        pre = f"members.{m}."
        layers = [(np.asarray(state[f"{pre}_base.mlp.{l}.weight"]), np.asarray(state[f"{pre}_base.mlp.{l}.bias"]))
                  for l in ("dense0", "dense1", "dense_final")]
        raw = np_forward(np.float64, cols, rows, (1, 1, 0, 0), n_onehot, layers, True, None)
        nl = pre + "normalize_output_layer."
        x[m], mean, var, counts[m] = norm_sequential(np.float64, raw, 2 * F, frag_len, eps, True,
                                                     np.asarray(state[nl + "running_mean"]).item(),
                                                     np.asarray(state[nl + "running_var"]).item(),
                                                     np.asarray(state[nl + "count"]).item())
        stats[m] = mean, var
    return pair_uncertainty_f64(x, F, frag_len, mode, gamma, noise, threshold), stats, counts
