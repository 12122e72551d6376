"""The NumPy reference of the implicit first-layer convolution (`tests/conv1_ref.py`) against torch on the CPU, at the
frame shapes the GPU tests run: `forward` is `relu(F.conv2d(...))` and `wgrad` its autograd, in float64 on
`(float32(x) * float32(scale)).double()`; the int64 forms are the float64 forms on integer operands. So the oracle of
`tests/test_conv1_implicit_gpu.py` is checked before a GPU is involved. One test shows that the GPU tests' comparisons reject
a reference that is subtly wrong (no kernel is mutated), one that an honest float32 evaluation sits two orders of magnitude
inside their tolerances, and one lists the shapes the documented predicate accepts."""
import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

from tests import conv1_ref as R

CPU_B = 3


def gid(s):
    return "x".join(map(str, s))


def _torch64(x, Wt, bias, dout, scale):
    """relu(conv2d) and the autograd of sum(dout * (conv2d + bias)) -- `dout` is the gradient w.r.t. the pre-activation."""
    B, _, H, W = x.shape
    OH, OW = R.out_size(H, 8, 4), R.out_size(W, 8, 4)
    xs = (th.from_numpy(x).float() * th.tensor(scale, dtype=th.float32)).double()       # the same single float32 multiply
    w = th.from_numpy(Wt.astype(np.float64)).reshape(32, 4, 8, 8).requires_grad_()       # torch's weights are (co, c, i, j)
    b = th.from_numpy(bias.astype(np.float64)).requires_grad_()
    z = F.conv2d(xs, w, b, stride=4)                                                     # [B, 32, OH, OW]
    assert z.shape == (B, 32, OH, OW)
    z.backward(th.from_numpy(dout.astype(np.float64)).reshape(B, OH, OW, 32).permute(0, 3, 1, 2))
    out = th.relu(z).detach().permute(0, 2, 3, 1).reshape(B * OH * OW, 32).numpy()
    return out, w.grad.reshape(32, 256).numpy(), b.grad.numpy()


@pytest.mark.parametrize("scale", R.SCALES + (1.0,), ids=lambda s: f"scale{s:.4g}")
@pytest.mark.parametrize("shape", R.SHAPES, ids=gid)
def test_reference_is_torch_conv2d_and_its_autograd(shape, scale):
    H, W = shape
    x, Wt, bias, dout = R.float_inputs(CPU_B, H, W) if scale != 1.0 else R.int_inputs(CPU_B, H, W)
    rows = CPU_B * R.npix(H, W)
    out, dW, db = _torch64(x, Wt, bias, dout, scale)
    got = R.forward(x, Wt, bias, scale)
    gW, gb = R.wgrad(x, dout, scale)
    assert got.shape == (rows, 32) and got.dtype == np.float64 and gW.shape == (32, 256) and gb.shape == (32,)
    # relative to the magnitude of the sums (256 terms per output, `rows` terms per gradient element)
    np.testing.assert_allclose(got, out, rtol=1e-13, atol=1e-13 * max(1.0, np.abs(out).max()))
    np.testing.assert_allclose(gW, dW, rtol=1e-13, atol=1e-13 * max(1.0, np.abs(dW).max()))
    np.testing.assert_allclose(gb, db, rtol=1e-13, atol=1e-13 * max(1.0, np.abs(db).max()))
    if scale == 1.0:    # the integer twins are these very numbers
        assert R.int_bound(CPU_B, H, W) < 2 ** 24
        fi, (wi, bi) = R.forward_int(x, Wt, bias), R.wgrad_int(x, dout)
        assert fi.dtype == wi.dtype == bi.dtype == np.int64
        assert np.array_equal(fi, out) and np.array_equal(wi, dW) and np.array_equal(bi, db)
        assert max(np.abs(fi).max(), np.abs(wi).max(), np.abs(bi).max()) <= R.int_bound(CPU_B, H, W)


def test_inputs_are_what_the_cases_claim():
    for H, W in R.SHAPES:
        x, Wt, bias, dout = R.int_inputs(CPU_B, H, W)
        assert x.dtype == np.uint8 and np.all(x[:, :, 0, 0] == 0) and np.all(x[:, :, -1, -1] == 255)
        for a in (Wt, bias, dout):
            assert a.dtype == np.float32 and np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 2
        x, Wt, bias, dout = R.float_inputs(CPU_B, H, W)
        assert all(a.dtype == np.float32 for a in (Wt, bias, dout))
        if dout.size >= 1024:
            assert 0.4 < np.mean(dout == 0) < 0.6
    # the looped exact cases stay exact, whatever the device's CU count up to 1 024
    fwd, wg = R.looped_batches(1024)
    assert max(R.int_bound(B, H, W) for B in fwd + wg for H, W in R.LOOP_SHAPES) < 2 ** 24
    assert max(R.int_bound(B, H, W) for B in R.BATCHES for H, W in R.SHAPES) < 2 ** 24
    assert [R.npix(H, W) for H, W in R.SHAPES] == [2, 2, 8, 32, 64, 80, 140, 400, 400]


# ---- sharpness: wrong references miss the GPU tests' comparisons ----
def _mutations(x, scale, integer):
    """{name: (column matrix, rows kept)} of subtly wrong evaluations: `rows kept` marks the rows the wrong kernel would
    have processed (the others contribute nothing to the gradient and are not produced by the forward)."""
    B, _, H, W = x.shape
    n = R.npix(H, W)
    col = R.columns_int(x) if integer else R.columns(x, scale)
    every = np.ones(col.shape[0], dtype=bool)
    out = {}
    out["columns (i, j, c)"] = (np.ascontiguousarray(col.reshape(-1, 4, 8, 8).transpose(0, 2, 3, 1)).reshape(col.shape), every)
    shifted = col.copy()
    k = 1 * 64 + 3 * 8 + 2                                  # tap (c, i, j) = (1, 3, 2) reads the pixel to its right
    shifted[:, k] = col[:, k + 1]
    out["one tap shifted"] = (shifted, every)
    if not integer:
        out["scale 1/256"] = (R.columns(x, 1.0 / 256.0), every)
    if B > 1:
        keep = every.copy()
        keep[(B - 1) * n:] = False
        out["last image dropped"] = (col, keep)
    keep = every.copy()
    keep[n - 1::n] = False
    out["last pixel of each image dropped"] = (col, keep)
    return out


@pytest.mark.parametrize("shape", R.SHAPES, ids=gid)
def test_comparisons_reject_a_subtly_wrong_reference(shape):
    H, W = shape
    rows = CPU_B * R.npix(H, W)
    # float form, scale 1/255: every mutation misses the float cases' tolerances (a forward row that was not produced is
    # the NaN it was filled with: counted as missed outright)
    x, Wt, bias, dout = R.float_inputs(CPU_B, H, W)
    scale = R.SCALES[0]
    ref, (rW, rb) = R.forward(x, Wt, bias, scale), R.wgrad(x, dout, scale)
    for name, (col, keep) in _mutations(x, scale, False).items():
        f = R.forward(x, Wt, bias, scale, col=col)
        f_ratio = np.inf if not keep.all() else R.tol_ratio(f, ref, R.FWD_RTOL, R.fwd_atol())
        mW, mb = R.wgrad(x, dout * keep[:, None], scale, col=col)
        w_ratio = R.tol_ratio(mW, rW, R.WGRAD_RTOL, R.wgrad_atol(rows))
        b_ratio = R.tol_ratio(mb, rb, R.WGRAD_RTOL, R.wgrad_atol(rows))
        print(f"{gid(shape)} {name}: forward {f_ratio:.3g}, dW {w_ratio:.3g}, db {b_ratio:.3g} x tolerance")
        assert f_ratio > 1 and w_ratio > 1, (shape, name)
        if not keep.all():
            assert b_ratio > 1, (shape, name)
    # integer form: each changes at least one element (the scale is no operand of the integer form)
    x, Wt, bias, dout = R.int_inputs(CPU_B, H, W)
    ref, (rW, rb) = R.forward_int(x, Wt, bias), R.wgrad_int(x, dout)
    for name, (col, keep) in _mutations(x, 1.0, True).items():
        mW, mb = R.wgrad_int(x, dout * keep[:, None], col=col)
        assert not np.array_equal(mW, rW), (shape, name)
        if keep.all():
            assert not np.array_equal(R.forward_int(x, Wt, bias, col=col), ref), (shape, name)
        else:
            assert not np.array_equal(mb, rb), (shape, name)


# ---- an honest float32 evaluation sits far inside the tolerances ----
def _fp32_forward(x, Wt, bias, scale):
    """Products rounded to float32 and summed in column order in float32, then bias and ReLU."""
    col = R.columns(x, scale)
    acc = np.zeros((col.shape[0], 32), dtype=np.float32)
    for k in range(256):
        acc += col[:, k:k + 1] * Wt[None, :, k]
    return np.maximum(acc + bias[None, :], np.float32(0))


def _fp32_wgrad(x, dout, scale):
    """Products rounded to float32 and summed in row order in float32."""
    col = R.columns(x, scale)
    dW, db = np.zeros((32, 256), dtype=np.float32), np.zeros(32, dtype=np.float32)
    for m in range(col.shape[0]):
        dW += dout[m, :, None] * col[m, None, :]
        db += dout[m]
    return dW, db


@pytest.mark.parametrize("case", [(3, 8, 12), (5, 44, 36), (1030, 8, 12), (2, 84, 84)], ids=gid)
def test_float32_evaluation_stays_far_inside_the_tolerances(case):
    """Measured on these inputs: forward at most 0.0083 of its tolerance (0.0042 at scale 1/255), weight gradient at most
    0.041 (0.029) -- sequential float32 summation, the least favourable order, leaves the bounds of the GPU tests between one
    and two orders of magnitude of headroom, so a kernel that misses them is wrong, not unlucky."""
    B, H, W = case
    rows = B * R.npix(H, W)
    x, Wt, bias, dout = R.float_inputs(B, H, W)
    for scale in R.SCALES:
        f = R.tol_ratio(_fp32_forward(x, Wt, bias, scale), R.forward(x, Wt, bias, scale), R.FWD_RTOL, R.fwd_atol())
        gW, gb = _fp32_wgrad(x, dout, scale)
        rW, rb = R.wgrad(x, dout, scale)
        w = max(R.tol_ratio(gW, rW, R.WGRAD_RTOL, R.wgrad_atol(rows)), R.tol_ratio(gb, rb, R.WGRAD_RTOL, R.wgrad_atol(rows)))
        print(f"{gid(case)} scale {scale:.4g}: forward {f:.4f}, weight gradient {w:.4f} x tolerance")
        assert f < 1 and w < 1


# ---- the predicate ----
# accepted: W = 12, 20, ..., 100 (W % 4 == 0 with OW = (W - 8) / 4 + 1 even) and 8 <= H <= this (the LDS budgets)
LARGEST_H = {12: 100, 20: 100, 28: 100, 36: 100, 44: 100, 52: 100, 60: 100, 68: 100, 76: 95, 84: 87, 92: 79, 100: 74}


def test_predicate_table():
    t = R.ok_table()
    assert t.shape == (93, 93) and t.dtype == bool and int(t.sum()) == 1051
    for wi, W in enumerate(R.SCAN):
        accepted = [H for hi, H in enumerate(R.SCAN) if t[hi, wi]]
        assert accepted == (list(range(8, LARGEST_H[W] + 1)) if W in LARGEST_H else []), W
    assert all(t[H - 8, W - 8] for H, W in R.SHAPES)
    assert R.largest_ok_H(84) == 87 and R.SHAPES[-1] == (87, 84) and not t[88 - 8, 84 - 8]
    # at 87 x 84 the weight gradient's budget binds (29 232 + 51 200 of 81 920 bytes; 88 rows make 21 output rows: 83 328)
    assert 4 * 87 * 84 + 400 * 128 <= 80 * 1024 < 4 * 88 * 84 + 420 * 128 and 2 * 4 * 88 * 84 <= 64 * 1024
    for H, W in [(8, 16), (8, 10), (7, 12), (8, 8), (100, 84)]:       # OW odd; W % 4; H < 8; OW = 1; too large
        assert not R.shape_ok(4, H, W, 8, 8, 4, 32)
    for other in [(3, 84, 84, 8, 8, 4, 32), (4, 84, 84, 4, 8, 4, 32), (4, 84, 84, 8, 4, 4, 32), (4, 84, 84, 8, 8, 2, 32),
                  (4, 84, 84, 8, 8, 4, 64)]:
        assert not R.shape_ok(*other)
