"""The ensemble kernels (`imitation_amd/csrc/ensemble.hip`) through the raw C ABI. Every output buffer is NaN-filled and
carries guard elements that must come back untouched.

A  `ia_ensemble_forward`: every member's row bit-equal to `ia_replay_relabel` (no output norm) with that member's
   parameters, and within 8 x the float32 NumPy forward's own deviation of the float64 forward (relative L2; the allowance
   every device test of this package gives a kernel that sums the same float32 terms in another order);
B  `ia_ensemble_norm_sequential`: bit-equal to M runs of `ia_reward_norm_sequential`, counts exact;
C  `ia_ensemble_moments`: bit-equal to the index-order float32 restatement (`tests/ensemble_ref.py`), which is NumPy's own
   result below 8 members;
D  `ia_ensemble_pair_uncertainty`: against float64 within 8 x the float32 restatement's deviation; `label` exact."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from tests import ensemble_ref as ref

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)
GUARD = 5


def dev(a):
    return th.from_numpy(np.ascontiguousarray(a)).to("cuda")


def nan_buffer(n):
    return th.full((n + GUARD,), float("nan"), device="cuda")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- kernel A

def make_params(r, dims):
    layers = []
    for i, o in zip(dims[:-1], dims[1:]):
        k = 1.0 / np.sqrt(i)
        layers.append((r.uniform(-k, k, (o, i)).astype(np.float32), r.uniform(-k, k, o).astype(np.float32)))
    return layers


def flat(layers):
    return np.concatenate([t.reshape(-1) for W, b in layers for t in (W, b)])


class ForwardCase:
    def __init__(self, seed, od, ad, discrete, flags, hid, relu, M, n, N, idx, normed):
        r = np.random.default_rng(seed)
        self.od, self.ad, self.discrete, self.flags, self.relu, self.M, self.n, self.N = od, ad, discrete, flags, relu, M, n, N
        self.D = (od if flags[0] else 0) + (ad if flags[1] else 0) + (od if flags[2] else 0) + (1 if flags[3] else 0)
        self.dims = [self.D, *hid, 1]
        self.cols = (r.normal(size=(N, od)).astype(np.float32),
                     r.integers(0, ad, N) if discrete else r.uniform(-1, 1, (N, ad)).astype(np.float32),
                     r.normal(size=(N, od)).astype(np.float32), (r.uniform(size=N) < 0.3).astype(np.float32))
        self.layers = [make_params(r, self.dims) for _ in range(M)]
        self.norms = [(r.normal(size=self.D).astype(np.float32), r.uniform(0.5, 2.0, self.D).astype(np.float32))
                      if m in normed else None for m in range(M)]
        self.eps = 1e-5
        self.idx = idx
        self.d_cols = [dev(c) for c in self.cols]
        self.d_params = [dev(flat(l)) for l in self.layers]
        self.d_norms = [None if s is None else (dev(s[0]), dev(s[1])) for s in self.norms]
        self.d_idx = None if idx is None else dev(idx.astype(np.int64))
        self.descs = [L.mlp_desc(self.dims, L.ACT_RELU if relu else L.ACT_TANH) for _ in range(M)]

    def rows(self):
        """(positions i, table rows) of the valid indices."""
        idx = np.arange(self.n) if self.idx is None else self.idx
        ok = (idx >= 0) & (idx < self.N)
        return np.nonzero(ok)[0], idx[ok]

    def args(self, raw, ld, M=None):
        a = L.EnsembleForwardArgs()
        obs, act, nxt, done = self.d_cols
        a.obs, a.next_obs, a.done, a.rows = L.ptr(obs), L.ptr(nxt), L.ptr(done), self.N
        a.act_f32, a.act_i64 = (None, L.ptr(act)) if self.discrete else (L.ptr(act), None)
        a.idx, a.n = L.ptr(self.d_idx), self.n
        a.obs_dim, a.act_dim = self.od, self.ad
        a.use_state, a.use_action, a.use_next_state, a.use_done = self.flags
        a.n_members = self.M if M is None else M
        for m in range(min(a.n_members, self.M)):
            a.desc[m] = C.pointer(self.descs[m])
            a.params[m] = L.ptr(self.d_params[m])
            if self.d_norms[m] is not None:
                a.norm_mean[m], a.norm_var[m] = L.ptr(self.d_norms[m][0]), L.ptr(self.d_norms[m][1])
        a.norm_eps = self.eps
        a.raw, a.ld = L.ptr(raw), ld
        return a

    def relabel(self, m):
        """`ia_replay_relabel` with member m's parameters and no output norm: reward [N] (NaN where not written)."""
        reward = nan_buffer(self.N)
        a = L.ReplayRelabelArgs()
        obs, act, nxt, done = self.d_cols
        a.obs, a.next_obs, a.done, a.ring_rows = L.ptr(obs), L.ptr(nxt), L.ptr(done), self.N
        a.act_f32, a.act_i64 = (None, L.ptr(act)) if self.discrete else (L.ptr(act), None)
        idx = self.d_idx if self.d_idx is not None else th.arange(self.n, device="cuda")
        a.idx, a.n = L.ptr(idx), self.n
        a.obs_dim, a.act_dim = self.od, self.ad
        a.use_state, a.use_action, a.use_next_state, a.use_done = self.flags
        a.desc, a.params = C.pointer(self.descs[m]), L.ptr(self.d_params[m])
        if self.d_norms[m] is not None:
            a.norm_mean, a.norm_var, a.norm_eps = L.ptr(self.d_norms[m][0]), L.ptr(self.d_norms[m][1]), self.eps
        a.reward = L.ptr(reward)
        L.check(L.load().ia_replay_relabel(C.byref(a), L.stream()), "ia_replay_relabel")
        return reward.cpu().numpy()


def _idx_with_duplicates(seed, n, N):
    r = np.random.default_rng(seed)
    idx = r.integers(0, N, n).astype(np.int64)
    idx[1] = idx[0]
    idx[n // 2] = N - 1
    idx[-1] = N - 1
    idx[7] = N            # one past the table: skipped
    return idx


FORWARD_CASES = {
    # a second tile with one row; rows 0 .. n - 1 (no index vector); input norms on members 0, 2, 4
    "box17x6_32x32_M5_n65": lambda: ForwardCase(1, 17, 6, False, (1, 1, 0, 0), (32, 32), True, 5, 65, 65, None, {0, 2, 4}),
    # D = 5 padded to 8; one row
    "box3x2_64x64_M2_n1": lambda: ForwardCase(2, 3, 2, False, (1, 1, 0, 0), (64, 64), False, 2, 1, 9, np.array([8]), set()),
    # D = 63 with next state and done; duplicates and one out-of-range index; an input norm on member 1 only
    "box27x8_all_32x64_M3_n130": lambda: ForwardCase(3, 27, 8, False, (1, 1, 1, 1), (32, 64), True, 3, 130, 97,
                                                     _idx_with_duplicates(3, 130, 97), {1}),
    # one-hot actions, the member cap
    "disc4x3_64x32_M16_n64": lambda: ForwardCase(4, 4, 3, True, (1, 1, 0, 0), (64, 32), False, 16, 64, 70,
                                                 np.random.default_rng(4).integers(0, 70, 64), set(range(0, 16, 3))),
}


@pytest.mark.parametrize("name", list(FORWARD_CASES))
def test_forward_rows_are_the_relabel_kernels_bits_and_close_to_float64(name):
    c = FORWARD_CASES[name]()
    lib = L.load()
    descs = (C.POINTER(L.MlpDesc) * c.M)(*[C.pointer(d) for d in c.descs])
    assert lib.ia_ensemble_forward_ok(descs, c.M, c.od, c.ad, *c.flags) == 1
    ld = c.n + 3
    raw = nan_buffer(c.M * ld)
    L.check(lib.ia_ensemble_forward(C.byref(c.args(raw, ld)), L.stream()), "ia_ensemble_forward")
    got = raw.cpu().numpy()
    assert np.isnan(got[c.M * ld:]).all()                       # guard
    got = got[:c.M * ld].reshape(c.M, ld)
    pos, rows = c.rows()
    written = np.zeros(ld, bool)
    written[pos] = True
    assert np.isnan(got[:, ~written]).all() and np.isfinite(got[:, written]).all()   # row tails, skipped indices
    f64, f32 = [], []
    for m in range(c.M):
        np.testing.assert_array_equal(bits(got[m, pos]), bits(c.relabel(m)[rows]), err_msg=f"member {m}")
        norm = None if c.norms[m] is None else (*c.norms[m], c.eps)
        n_onehot = c.ad if c.discrete else 0
        f64.append(ref.np_forward(np.float64, c.cols, rows, c.flags, n_onehot, c.layers[m], c.relu, norm))
        f32.append(ref.np_forward(np.float32, c.cols, rows, c.flags, n_onehot, c.layers[m], c.relu, norm))
    dref = ref.rel(np.stack(f32), np.stack(f64))
    bound = 8 * dref if dref > 0 else EPS32
    d = ref.rel(got[:, pos], np.stack(f64))
    print(f"{name}: dref {dref:.3e}, device {d:.3e}")
    assert d <= bound, (d, bound)


def test_forward_refuses_what_it_does_not_cover_and_writes_nothing():
    lib = L.load()
    c = FORWARD_CASES["box17x6_32x32_M5_n65"]()
    ld = c.n
    for what, mutate in (("M = 1", lambda a: setattr(a, "n_members", 1)),
                         ("M = 17", lambda a: setattr(a, "n_members", 17)),
                         ("ld < n", lambda a: setattr(a, "ld", c.n - 1)),
                         ("both kinds of action", lambda a: setattr(a, "act_i64", a.act_f32)),
                         ("no parameters", lambda a: a.params.__setitem__(2, None)),
                         ("half a norm", lambda a: a.norm_var.__setitem__(0, None))):
        raw = nan_buffer(c.M * ld)
        a = c.args(raw, ld)
        mutate(a)
        assert lib.ia_ensemble_forward(C.byref(a), L.stream()) in (L.ERR_ARG, L.ERR_UNSUPPORTED), what
        th.cuda.synchronize()
        assert bool(th.isnan(raw).all()), what
    # members with differing descriptors
    other = L.mlp_desc([c.D, 64, 32, 1], L.ACT_RELU)
    raw = nan_buffer(c.M * ld)
    a = c.args(raw, ld)
    a.desc[1] = C.pointer(other)
    assert lib.ia_ensemble_forward(C.byref(a), L.stream()) == L.ERR_UNSUPPORTED
    descs = (C.POINTER(L.MlpDesc) * c.M)(*[C.pointer(d) for d in c.descs])
    descs[1] = C.pointer(other)
    assert lib.ia_ensemble_forward_ok(descs, c.M, c.od, c.ad, *c.flags) == 0
    tanh = L.mlp_desc(c.dims, L.ACT_TANH)
    descs[1] = C.pointer(tanh)
    assert lib.ia_ensemble_forward_ok(descs, c.M, c.od, c.ad, *c.flags) == 0
    # D = 65
    wide = ForwardCase(5, 30, 4, False, (1, 1, 1, 1), (32, 32), True, 2, 4, 8, None, set())
    assert wide.D == 65
    raw2 = nan_buffer(2 * 4)
    assert lib.ia_ensemble_forward(C.byref(wide.args(raw2, 4)), L.stream()) == L.ERR_UNSUPPORTED
    descs2 = (C.POINTER(L.MlpDesc) * 2)(*[C.pointer(d) for d in wide.descs])
    assert lib.ia_ensemble_forward_ok(descs2, 2, 30, 4, 1, 1, 1, 1) == 0
    assert lib.ia_ensemble_forward_ok(descs2, 1, 30, 4, 1, 1, 1, 1) == 0
    th.cuda.synchronize()
    assert bool(th.isnan(raw).all()) and bool(th.isnan(raw2).all())


# ---------------------------------------------------------------------------------------------------------------- kernel B

MTN = [(2, 1, 1), (5, 3, 7), (3, 17, 100), (8, 2, 64)]


def _norm_states(M, warm, r):
    """Per member (mean, var, count) host values; the LAST member has no norm."""
    out = []
    for m in range(M - 1):
        out.append((np.float32(r.normal()), np.float32(r.uniform(0.5, 2.0)), int(r.integers(1, 5000))) if warm
                   else (np.float32(0), np.float32(1), 0))
    return out + [None]


@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("update", [0, 1])
@pytest.mark.parametrize("M,T,n", MTN)
def test_norm_sequential_is_m_runs_of_the_single_kernel(M, T, n, update, warm):
    lib = L.load()
    r = np.random.default_rng(100 * M + T)
    R, ld = T * n, T * n + 2
    raw_h = np.full((M, ld), np.nan, np.float32)
    raw_h[:, :R] = (r.normal(size=(M, R)) * 2 + 0.5).astype(np.float32)
    raw = dev(raw_h.reshape(-1))
    states = _norm_states(M, warm, r)
    eps = [1e-5 if m % 2 == 0 else 1e-3 for m in range(M)]
    mk = lambda s: None if s is None else (th.tensor([s[0]], device="cuda"), th.tensor([s[1]], device="cuda"),
                                           th.tensor([s[2]], dtype=th.int32, device="cuda"))
    # the single kernel, member by member
    want = []
    for m in range(M):
        if states[m] is None:
            want.append((raw_h[m, :R], None))
            continue
        mean, var, cnt = mk(states[m])
        out = nan_buffer(R)
        L.call("ia_reward_norm_sequential", raw.data_ptr() + 4 * m * ld, T, n, eps[m], update, L.ptr(mean), L.ptr(var),
               L.ptr(cnt), L.ptr(out), L.stream())
        want.append((out.cpu().numpy()[:R], (mean.item(), var.item(), cnt.item())))
    # the ensemble kernel
    bufs = [mk(s) for s in states]
    out = nan_buffer(M * ld)
    a = L.EnsembleNormArgs()
    a.raw, a.out, a.ld = L.ptr(raw), L.ptr(out), ld
    a.T, a.n, a.n_members, a.update_stats = T, n, M, update
    for m in range(M):
        a.eps[m] = eps[m]
        if bufs[m] is not None:
            a.mean[m], a.var[m], a.count[m] = (L.ptr(t) for t in bufs[m])
    L.check(lib.ia_ensemble_norm_sequential(C.byref(a), L.stream()), "ia_ensemble_norm_sequential")
    got = out.cpu().numpy()
    assert np.isnan(got[M * ld:]).all()
    got = got[:M * ld].reshape(M, ld)
    assert np.isnan(got[:, R:]).all()
    for m in range(M):
        np.testing.assert_array_equal(bits(got[m, :R]), bits(want[m][0]), err_msg=f"member {m}")
        if bufs[m] is None:
            continue
        mean, var, cnt = (t.item() for t in bufs[m])
        assert bits(np.float32(mean)) == bits(np.float32(want[m][1][0])) and bits(np.float32(var)) == bits(np.float32(want[m][1][1]))
        assert cnt == want[m][1][2] == states[m][2] + (R if update else 0)
        if not update:
            assert (np.float32(mean), np.float32(var)) == (states[m][0], states[m][1])
    # against the per-step formula in float64 (a member with a norm), as a sanity check of what both kernels compute
    s0 = states[0]
    f64 = ref.norm_sequential(np.float64, raw_h[0, :R], T, n, eps[0], bool(update), s0[0], s0[1], s0[2])
    np.testing.assert_allclose(got[0, :R], f64[0], rtol=2e-4, atol=2e-5)


def test_norm_sequential_refuses_bad_records():
    lib = L.load()
    raw, out = nan_buffer(8), nan_buffer(8)
    a = L.EnsembleNormArgs()
    a.raw, a.out, a.ld, a.T, a.n, a.n_members = L.ptr(raw), L.ptr(out), 3, 2, 2, 2    # ld < T * n
    assert lib.ia_ensemble_norm_sequential(C.byref(a), L.stream()) == L.ERR_ARG
    a.ld, a.n_members = 4, 17
    assert lib.ia_ensemble_norm_sequential(C.byref(a), L.stream()) == L.ERR_ARG
    a.n_members = 2
    mean = th.zeros(1, device="cuda")
    a.mean[0] = L.ptr(mean)                                                                # mean without var / count
    assert lib.ia_ensemble_norm_sequential(C.byref(a), L.stream()) == L.ERR_ARG
    th.cuda.synchronize()
    assert bool(th.isnan(out).all())


# ---------------------------------------------------------------------------------------------------------------- kernel C

@pytest.mark.parametrize("alpha", [0.0, -1.5, 2.0])
@pytest.mark.parametrize("M,T,n", MTN)
def test_moments_are_numpys_float32_moments(M, T, n, alpha):
    r = np.random.default_rng(10 * M + T)
    R, ld = T * n, T * n + 3
    x_h = np.full((M, ld), np.nan, np.float32)
    # (8 members: positive inputs, so that the mean has no cancellation and a distance in ulp of it means something)
    x_h[:, :R] = (r.normal(size=(M, R)) if M < 8 else r.uniform(0.5, 1.5, size=(M, R))).astype(np.float32)
    x = dev(x_h.reshape(-1))
    mean, var, bound = nan_buffer(R), nan_buffer(R), nan_buffer(R)
    L.call("ia_ensemble_moments", L.ptr(x), ld, M, R, alpha, L.ptr(mean), L.ptr(var), L.ptr(bound), L.stream())
    mean, var, bound = (t.cpu().numpy() for t in (mean, var, bound))
    for t in (mean, var, bound):
        assert np.isnan(t[R:]).all() and np.isfinite(t[:R]).all()
    w_mean, w_var, w_bound = ref.moments_f32(x_h[:, :R], alpha)
    np.testing.assert_array_equal(bits(mean[:R]), bits(w_mean))
    np.testing.assert_array_equal(bits(var[:R]), bits(w_var))
    assert ref.ulp_distance(bound[:R], w_bound).max() <= 1
    xt = np.ascontiguousarray(x_h[:, :R].T)              # what `predict_processed_all` returns: [batch, M]
    if M < 8:
        np.testing.assert_array_equal(bits(mean[:R]), bits(xt.mean(-1)))
        np.testing.assert_array_equal(bits(var[:R]), bits(xt.var(-1, ddof=1)))
    else:
        # At 8 members NumPy's own reduction over the last axis changes its order (eight partial sums side by side); the
        # kernel keeps the index order, so the two may differ by a few units in the last place.
        assert ref.ulp_distance(mean[:R], xt.mean(-1)).max() <= 4
        assert ref.ulp_distance(var[:R], xt.var(-1, ddof=1)).max() <= 4
    # every output is nullable
    only = nan_buffer(R)
    L.call("ia_ensemble_moments", L.ptr(x), ld, M, R, alpha, None, None, L.ptr(only), L.stream())
    np.testing.assert_array_equal(bits(only.cpu().numpy()[:R]), bits(bound[:R]))
    assert L.load().ia_ensemble_moments(L.ptr(x), R - 1, M, R, alpha, None, None, L.ptr(only), L.stream()) == L.ERR_ARG
    assert L.load().ia_ensemble_moments(L.ptr(x), ld, 1, R, alpha, None, None, L.ptr(only), L.stream()) == L.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- kernel D

PLM = [(1, 1, 2), (7, 5, 3), (24, 100, 5)]
THRESHOLD = 2.0


def uncertainty_input(P, L_, M, gamma, noise):
    """Member rewards `[M, 2 P L]` whose returns differences straddle the clip, from the first seed (searched on the CPU,
    in float64) at which no member probability lies within 1e-4 of 0.5: the labels are then decisive."""
    for seed in range(100):
        r = np.random.default_rng(7000 + 97 * P + seed)
        x = (r.normal(size=(M, 2 * P * L_)) * (3.0 / np.sqrt(L_))).astype(np.float32)
        probs = ref.member_probabilities_f64(x, P, L_, gamma, noise, THRESHOLD)
        if np.abs(probs - 0.5).min() > 1e-4:
            return x, probs
    raise AssertionError("no decisive seed")


def run_uncertainty(x, P, L_, M, mode, gamma, noise, ld):
    buf = np.full((M, ld), np.nan, np.float32)
    buf[:, :2 * P * L_] = x
    est = nan_buffer(P)
    L.call("ia_ensemble_pair_uncertainty", L.ptr(dev(buf.reshape(-1))), ld, M, P, L_, L.UNCERTAINTY_MODES[mode], gamma, noise,
           THRESHOLD, L.ptr(est), L.stream())
    got = est.cpu().numpy()
    assert np.isnan(got[P:]).all() and np.isfinite(got[:P]).all()
    return got[:P]


@pytest.mark.parametrize("noise", [0.0, 0.1])
@pytest.mark.parametrize("gamma", [1.0, 0.9])
@pytest.mark.parametrize("P,L_,M", PLM)
def test_pair_uncertainty(P, L_, M, gamma, noise):
    x, probs = uncertainty_input(P, L_, M, gamma, noise)
    assert np.abs(probs - 0.5).min() > 1e-4
    if P > 1:   # the clip is hit, and not everywhere
        w = gamma ** np.arange(L_)
        d = ((x.reshape(M, P, 2, L_)[:, :, 1].astype(np.float64) - x.reshape(M, P, 2, L_)[:, :, 0]) * w).sum(-1)
        assert (np.abs(d) > THRESHOLD).any() and (np.abs(d) < THRESHOLD).any()
    ld = 2 * P * L_ + 1
    for mode in ref.MODES:
        got = run_uncertainty(x, P, L_, M, mode, gamma, noise, ld)
        again = run_uncertainty(x, P, L_, M, mode, gamma, noise, ld)
        np.testing.assert_array_equal(bits(got), bits(again))            # fixed order, no atomics
        f64 = ref.pair_uncertainty_f64(x, P, L_, mode, gamma, noise, THRESHOLD)
        if mode == "label":
            np.testing.assert_array_equal(got, f64.astype(np.float32))
            continue
        dref = ref.rel(ref.pair_uncertainty_f32(x, P, L_, mode, gamma, noise, THRESHOLD), f64)
        bound = 8 * dref if dref > 0 else EPS32
        d = ref.rel(got, f64)
        print(f"P {P} L {L_} M {M} {mode} gamma {gamma} noise {noise}: dref {dref:.3e}, device {d:.3e}")
        assert d <= bound, (mode, d, bound)


def test_pair_uncertainty_refuses_bad_arguments():
    lib = L.load()
    x, est = th.zeros(64, device="cuda"), nan_buffer(4)
    call = lambda ld, M, P, L_, mode: lib.ia_ensemble_pair_uncertainty(L.ptr(x), ld, M, P, L_, mode, 1.0, 0.0, 50.0,
                                                                       L.ptr(est), L.stream())
    assert call(15, 2, 2, 4, 0) == L.ERR_ARG        # ld < 2 P L
    assert call(16, 1, 2, 4, 0) == L.ERR_ARG and call(16, 17, 2, 4, 0) == L.ERR_ARG
    assert call(16, 2, 2, 4, 3) == L.ERR_ARG
    th.cuda.synchronize()
    assert bool(th.isnan(est).all())
