"""Kernel-level parity of the tabular MCE planning entries (`csrc/mce.hip`): `ia_mce_backup`, `ia_mce_forward`,
`ia_mce_weights` and `ia_mce_norms` against a float64 NumPy restatement of `mce_irl.py:38-144` written here, at the
smallest shapes that cross the kernels' constants: one state; S not a multiple of the wave (67, odd: the 8-byte loads);
S even (the 16-byte loads) with more than one block of four waves, more than one forward slab of 32 rows and more than one
block of 256 s' (300); A past the chunk of 8 actions by one (9) and by several chunks (33); H = 1 (the base case alone).

Tolerance: the restatement is also evaluated in `np.longdouble`; a kernel table may differ from the float64 NumPy table
by 4 x the largest difference NumPy-float64 itself shows from the longdouble table on that input (a different but
equally long summation order), with a floor of 1e-13 relative to the table's largest finite magnitude; the row sums of pi
are held to 1 by the same rule. Output buffers are
NaN-prefilled between guard elements that must come back untouched; two runs must agree bit for bit."""
import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from tests.test_preference_kernels_gpu import DEV, GUARD, _KEEP, Guarded, _release_temporaries, dev  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


class Guarded64(Guarded):
    """`Guarded` for float64 outputs (the guard zone is 512 bytes, so the payload keeps the allocation's alignment)."""

    def __init__(self, n, init=None):
        self.n, self.dtype = int(n), th.float64
        self.buf = th.full((self.n + 2 * GUARD,), float("nan"), dtype=th.float64, device=DEV)
        self.v = self.buf[GUARD:GUARD + self.n]
        if init is not None:
            self.v.copy_(th.as_tensor(np.ascontiguousarray(init, dtype=np.float64)).reshape(-1))
        _KEEP.append(self.buf)

    def guards_ok(self):
        g = th.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]]).cpu().numpy()
        return bool(np.isnan(g).all())


def make_problem(S, A, seed, big_negative=True):
    r = np.random.default_rng(seed)
    T = r.uniform(0.05, 1.0, size=(S, A, S))
    T[r.uniform(size=T.shape) < 1.0 / 3.0] = 0.0
    T[np.arange(S)[:, None], np.arange(A)[None, :], r.integers(S, size=(S, A))] += 0.5
    T /= T.sum(axis=2, keepdims=True)
    reward = r.normal(size=S).astype(np.float32)
    if big_negative and S > 2:
        reward[r.choice(S, size=max(1, S // 7), replace=False)] = -1e4   # log-sum-exp stability
    init = r.uniform(0.1, 1.0, size=S)
    if S > 2:
        init[r.choice(S, size=S // 3, replace=False)] = 0.0               # zero initial mass
    init /= init.sum()
    return T, reward, init


def _lse(x):
    m = x.max(axis=1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=1))


def restate_backup(T, reward, H, discount, dtype):
    T, r, g = T.astype(dtype), reward.astype(dtype), dtype(discount)
    S, A = T.shape[:2]
    V, Q = np.zeros((H, S), dtype), np.zeros((H, S, A), dtype)
    Q[H - 1] = r[:, None]
    V[H - 1] = _lse(Q[H - 1])
    for t in reversed(range(H - 1)):
        Q[t] = r[:, None] + g * (T @ V[t + 1])
        V[t] = _lse(Q[t])
    return V, Q, np.exp(Q - V[:, :, None])


def restate_forward(T, pi, init, H, discount, dtype):
    T, pi, g = T.astype(dtype), pi.astype(dtype), dtype(discount)
    S, A = T.shape[:2]
    D = np.zeros((H + 1, S), dtype)
    D[0] = init.astype(dtype)
    for t in range(H):
        for a in range(A):
            D[t + 1] += (D[t] * pi[t, :, a]) @ T[:, a, :]
    Dcum = np.zeros(S, dtype)
    for t in reversed(range(H + 1)):
        Dcum = D[t] + g * Dcum
    return D, Dcum


def bound(f64, ld):
    """Allowed |kernel - f64|: see the module docstring."""
    own = float(np.max(np.abs(f64.astype(np.longdouble) - ld))) if f64.size else 0.0
    fin = np.abs(f64[np.isfinite(f64)])
    return max(4.0 * own, 1e-13 * (float(fin.max()) if fin.size else 1.0))


def run_backup(T_d, r_d, S, A, H, discount):
    V, Q, pi = Guarded64(H * S), Guarded64(H * S * A), Guarded64(H * S * A)
    L.call("ia_mce_backup", L.ptr(T_d), L.ptr(r_d), S, A, H, float(discount), V.ptr, Q.ptr, pi.ptr, L.stream())
    th.cuda.synchronize()
    assert V.guards_ok() and Q.guards_ok() and pi.guards_ok()
    return V.np().reshape(H, S), Q.np().reshape(H, S, A), pi.np().reshape(H, S, A)


def run_forward(T_d, pi_d, init_d, S, A, H, discount):
    n_ws = int(L.load().ia_mce_forward_ws_doubles(S, A))
    assert n_ws >= S
    D, Dcum, ws = Guarded64((H + 1) * S), Guarded64(S), Guarded64(n_ws)
    L.call("ia_mce_forward", L.ptr(T_d), L.ptr(pi_d), L.ptr(init_d), S, A, H, float(discount), D.ptr, Dcum.ptr, ws.ptr,
           L.stream())
    th.cuda.synchronize()
    assert D.guards_ok() and Dcum.guards_ok() and ws.guards_ok()
    return D.np().reshape(H + 1, S), Dcum.np()


SHAPES = [(1, 1, 1), (67, 3, 5), (300, 5, 4), (128, 9, 2), (130, 33, 3), (67, 3, 1)]


@pytest.mark.parametrize("discount", [1.0, 0.9])
@pytest.mark.parametrize("S,A,H", SHAPES)
def test_backup_and_forward_match_numpy(S, A, H, discount):
    T, reward, init = make_problem(S, A, seed=S * 1000 + A * 10 + H)
    ref = restate_backup(T, reward, H, discount, np.float64)
    ref_ld = restate_backup(T, reward, H, discount, np.longdouble)
    T_d, r_d = dev(T, th.float64), dev(reward)
    got = run_backup(T_d, r_d, S, A, H, discount)
    for name, x, y, z in zip(("V", "Q", "pi"), got, ref, ref_ld):
        assert np.isfinite(x).all(), name
        tol = bound(y, z)
        err = float(np.max(np.abs(x - y)))
        print(f"backup {name} S={S} A={A} H={H} g={discount}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, err, tol)
    # rows of pi sum to 1 under the same rule, applied to the table of row sums (where V is near -1e4 its own rounding
    # moves a whole row by ~1e-12: NumPy's rows show that too, an entry-wise bound divided among A entries would not)
    rows_tol = bound(ref[2].sum(axis=2), ref_ld[2].sum(axis=2))
    rows_err = float(np.max(np.abs(got[2].sum(axis=2) - 1.0)))
    print(f"backup pi rows S={S} A={A} H={H} g={discount}: err {rows_err:.3e} bound {rows_tol:.3e}")
    assert rows_err <= rows_tol, (rows_err, rows_tol)
    assert (got[2] >= 0).all()
    again = run_backup(T_d, r_d, S, A, H, discount)
    for x, y in zip(got, again):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))

    # the occupancy pass on NumPy's own float64 policy, so both sides start from the same input
    pi = ref[2]
    refD = restate_forward(T, pi, init, H, discount, np.float64)
    refD_ld = restate_forward(T, pi, init, H, discount, np.longdouble)
    pi_d, init_d = dev(pi, th.float64), dev(init, th.float64)
    gotD = run_forward(T_d, pi_d, init_d, S, A, H, discount)
    for name, x, y, z in zip(("D", "Dcum"), gotD, refD, refD_ld):
        assert np.isfinite(x).all(), name
        tol = bound(y, z)
        err = float(np.max(np.abs(x - y)))
        print(f"forward {name} S={S} A={A} H={H} g={discount}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (name, err, tol)
    assert np.array_equal(gotD[0][0], init)                       # D[0] is the initial distribution itself
    assert (gotD[0][:, init == 0][0] == 0).all()
    againD = run_forward(T_d, pi_d, init_d, S, A, H, discount)
    for x, y in zip(gotD, againD):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))


@pytest.mark.parametrize("S", [1, 67, 300, 1031])
def test_weights_and_norms(S):
    r = np.random.default_rng(S)
    Dcum, demo = r.uniform(0, 3, size=S), r.uniform(0, 3, size=S)
    w, stats = Guarded(S), Guarded64(3)
    L.call("ia_mce_weights", L.ptr(dev(Dcum, th.float64)), L.ptr(dev(demo, th.float64)), S, w.ptr, stats.ptr, L.stream())
    th.cuda.synchronize()
    assert w.guards_ok() and stats.guards_ok()
    assert np.array_equal(w.np(), (Dcum - demo).astype(np.float32))         # th.as_tensor(..., dtype=float32)
    st = stats.np()
    assert st[0] == np.max(np.abs(demo - Dcum)) and np.isnan(st[1:]).all()  # exact: a max; the norms' slots untouched

    n = 3 * S + 5
    g, p = r.normal(size=n).astype(np.float32), r.normal(size=n).astype(np.float32)
    L.call("ia_mce_norms", L.ptr(dev(g)), L.ptr(dev(p)), n, stats.ptr, L.stream())
    th.cuda.synchronize()
    assert stats.guards_ok()
    st2 = stats.np()
    assert st2[0] == st[0]
    # float32 sums of n squares, any order: relative error of the sum <= n * 2^-24, half of it after the root
    for got, x in zip(st2[1:], (g, p)):
        exact = np.sqrt(np.sum(x.astype(np.float64) ** 2))
        assert got == np.float32(got)
        assert abs(got - exact) <= exact * (n * 2.0 ** -24 + 2.0 ** -23), (got, exact)


def test_weights_propagate_nan():
    Dcum, demo = np.array([1.0, np.nan, 2.0]), np.array([0.5, 0.5, 0.5])
    w, stats = Guarded(3), Guarded64(3)
    L.call("ia_mce_weights", L.ptr(dev(Dcum, th.float64)), L.ptr(dev(demo, th.float64)), 3, w.ptr, stats.ptr, L.stream())
    th.cuda.synchronize()
    assert np.isnan(stats.np()[0])     # np.max(np.abs(...)) is NaN: the loop must not read it as "converged" or go on blindly


def test_argument_checks():
    lib = L.load()
    assert lib.ia_mce_backup(None, None, 4, 2, 3, 1.0, None, None, None, None) == L.ERR_ARG
    assert lib.ia_mce_forward(None, None, None, 4, 2, 3, 1.0, None, None, None, None) == L.ERR_ARG
    assert lib.ia_mce_forward_ws_doubles(0, 3) == 0
    t = dev(np.zeros(8), th.float64)
    assert lib.ia_mce_backup(L.ptr(t), L.ptr(dev(np.zeros(1))), 1, 2000, 1, 1.0, L.ptr(t), L.ptr(t), L.ptr(t),
                             None) == L.ERR_UNSUPPORTED   # more actions than the LDS row holds: refused before any launch
