"""The NumPy references of the convolution data-movement kernels (`tests/conv_ref.py`) against torch on the CPU, at the
geometries the GPU tests run: `im2col` is `torch.nn.functional.unfold` with the columns in the documented order (exact),
`col2im` is `F.fold` and conv autograd's input gradient in float64 (up to the float32 accumulation of the reference, bounded
from the terms themselves), the Categorical head is `torch.distributions.Categorical` and its autograd in float64. So
the oracle of `tests/test_conv_kernels_gpu.py` is checked before a GPU is involved, and one test shows that these
comparisons reject a reference that is off by one tap or one pixel."""
import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

from tests import conv_ref as R

EPS = 2.0 ** -24   # unit roundoff of float32


def gid(g):
    return "x".join(map(str, g))


def _randn32(*shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _pad_geoms():
    """Every float32 geometry as (B, H, W, C, KH, KW, S, P)."""
    return [g + (0,) for g in R.F32_GEOMS + R.COL2IM_GAP_GEOMS] + [(B, H, W, C, K, K, S, P) for B, H, W, C, K, S, P in R.F32_PAD_GEOMS]


# ---- im2col: pure data movement, compared exactly ----
@pytest.mark.parametrize("scale", [1 / 255, 1.0])
@pytest.mark.parametrize("geom", R.U8_KW8_GEOMS + R.U8_GENERIC_GEOMS, ids=gid)
def test_im2col_u8_is_unfold(geom, scale):
    B, C, H, W, KH, KW, S = geom
    x = np.random.default_rng(3).integers(0, 256, size=(B, C, H, W), dtype=np.uint8)
    x[0, 0, 0, :2] = (0, 255)
    got = R.im2col_u8_nchw(x, KH, KW, S, scale)
    OH, OW = R.out_size(H, KH, S), R.out_size(W, KW, S)
    assert got.shape == (B * OH * OW, C * KH * KW) and got.dtype == np.float32
    xs = th.from_numpy(x).float() * th.tensor(scale, dtype=th.float32)           # the same single float32 multiply
    want = F.unfold(xs, (KH, KW), stride=S).permute(0, 2, 1).reshape(B * OH * OW, -1)   # unfold's columns are (c, i, j)
    assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32))


@pytest.mark.parametrize("geom", _pad_geoms(), ids=gid)
def test_im2col_f32_is_unfold(geom):
    B, H, W, C, KH, KW, S, P = geom
    x = _randn32(B, H, W, C, seed=1)
    got = R.im2col_f32_nhwc(x, KH, KW, S, P)
    OH, OW = R.out_size(H, KH, S, P), R.out_size(W, KW, S, P)
    assert got.shape == (B * OH * OW, KH * KW * C) and got.dtype == np.float32
    u = F.unfold(th.from_numpy(x).permute(0, 3, 1, 2), (KH, KW), stride=S, padding=P)        # [B, (c, i, j), OH*OW]
    want = u.reshape(B, C, KH, KW, OH * OW).permute(0, 4, 2, 3, 1).reshape(B * OH * OW, -1)  # -> rows, (i, j, c)
    assert np.array_equal(got.view(np.int32), want.contiguous().numpy().view(np.int32))
    if P == 0:
        assert np.array_equal(got, R.im2col_f32_nhwc(x, KH, KW, S))


# ---- col2im: float32 sums of at most ceil(KH/S) ceil(KW/S) terms per pixel against float64 ----
def _fold64(dcol, geom):
    """F.fold of dcol (columns (i, j, c)) in float64 -> [B, H, W, C]."""
    B, H, W, C, KH, KW, S, P = geom
    L = dcol.shape[0] // B
    u = th.from_numpy(dcol.astype(np.float64)).reshape(B, L, KH, KW, C).permute(0, 4, 2, 3, 1).reshape(B, C * KH * KW, L)
    return F.fold(u, (H, W), (KH, KW), stride=S, padding=P).permute(0, 2, 3, 1).numpy()


def _fold_error(got, dcol, geom):
    """max over the pixels of |got - fold64| / (T 2^-24 fold64(|dcol|)), T = the most terms a pixel sums: at most 1 if
    `got` is a float32 sum of the right terms in any order; pixels without terms must be exactly 0."""
    B, H, W, C, KH, KW, S, P = geom
    want, mag = _fold64(dcol, geom), _fold64(np.abs(dcol), geom)
    T = -(-KH // S) * -(-KW // S)
    err = np.abs(got.astype(np.float64) - want)
    empty = mag == 0
    if np.any(err[empty] != 0):
        return np.inf
    return float(np.max(err[~empty] / (T * EPS * mag[~empty]))) if np.any(~empty) else 0.0


def _dcol(geom, seed=2):
    B, H, W, C, KH, KW, S, P = geom
    return _randn32(B * R.out_size(H, KH, S, P) * R.out_size(W, KW, S, P), KH * KW * C, seed=seed)


@pytest.mark.parametrize("geom", _pad_geoms(), ids=gid)
def test_col2im_is_fold(geom):
    B, H, W, C, KH, KW, S, P = geom
    dcol = _dcol(geom)
    got = R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S, P)
    assert got.shape == (B, H, W, C) and got.dtype == np.float32
    assert _fold_error(got, dcol, geom) <= 1.0
    # a pixel that no window covers is exactly zero, and the geometries named for that have such pixels
    covered = _fold64(np.ones_like(dcol), geom) > 0
    assert np.all(got[~covered] == 0.0)
    if geom[:7] in R.COL2IM_GAP_GEOMS:
        assert not covered.all()
    # the mask rule: kept where mask > 0, zero at 0.0, -0.0 and negative values
    mask = _randn32(B, H, W, C, seed=5)
    mask.reshape(-1)[::5] = 0.0
    mask.reshape(-1)[1::7] = -0.0
    masked = R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S, P, mask=mask)
    keep = mask > 0
    assert np.array_equal(masked[keep].view(np.int32), got[keep].view(np.int32)) and np.all(masked[~keep] == 0.0)
    assert masked.dtype == np.float32


@pytest.mark.parametrize("geom", _pad_geoms(), ids=gid)
def test_col2im_is_conv_input_gradient(geom):
    """With one-hot weights (output channel (i, j, c) reads tap (i, j) of channel c) a convolution's output IS the column
    matrix, so autograd's input gradient for the output gradient `dcol` is col2im(dcol)."""
    B, H, W, C, KH, KW, S, P = geom
    K = KH * KW * C
    dcol = _dcol(geom)
    OH, OW = R.out_size(H, KH, S, P), R.out_size(W, KW, S, P)
    w = th.eye(K, dtype=th.float64).reshape(K, KH, KW, C).permute(0, 3, 1, 2).contiguous()
    x = th.zeros(B, C, H, W, dtype=th.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=S, padding=P)
    y.backward(th.from_numpy(dcol.astype(np.float64)).reshape(B, OH, OW, K).permute(0, 3, 1, 2))
    want = x.grad.permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(want, _fold64(dcol, geom), rtol=1e-13, atol=1e-13)
    got = R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S, P).astype(np.float64)
    T = -(-KH // S) * -(-KW // S)
    assert np.all(np.abs(got - want) <= T * EPS * _fold64(np.abs(dcol), geom))


def test_fold_comparison_rejects_a_reference_that_is_off_by_one():
    """The sharpness of the comparisons above, shown on perturbed forms of the reference itself (no kernel is mutated):
    windows whose origin is one pixel off, and taps read in (j, i) for (i, j), miss the fold comparison by orders of
    magnitude. Visiting the right taps in another ORDER is still a float32 sum of the right terms -- the fold comparison
    accepts it, as it must -- but changes bits, which is what the bit comparison of the GPU tests pins."""
    for geom in [(3, 7, 9, 64, 3, 3, 1, 0), (2, 8, 8, 32, 4, 4, 2, 0), (2, 5, 7, 4, 3, 3, 1, 1), (2, 6, 5, 8, 5, 5, 1, 2)]:
        B, H, W, C, KH, KW, S, P = geom
        assert geom in _pad_geoms() and KH == KW
        dcol = _dcol(geom)
        good = R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S, P)
        assert _fold_error(good, dcol, geom) <= 1.0
        for origin in (-1, 1):
            assert _fold_error(R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S, P, origin=origin), dcol, geom) > 1e4, (geom, origin)
        swapped = np.ascontiguousarray(dcol.reshape(-1, KH, KW, C).transpose(0, 2, 1, 3)).reshape(dcol.shape)
        assert _fold_error(R.col2im_nhwc(swapped, B, H, W, C, KH, KW, S, P), dcol, geom) > 1e4, geom
        backwards = [(i, j) for i in reversed(range(KH)) for j in reversed(range(KW))]
        other = R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S, P, taps=backwards)
        assert _fold_error(other, dcol, geom) <= 1.0
        assert not np.array_equal(other.view(np.int32), good.view(np.int32)), geom


# ---- pool and ReLU ----
@pytest.mark.parametrize("HW,C", [(35, 8), (7, 3), (64, 32)])
def test_pool_and_relu_references_are_torch_autograd(HW, C):
    B = 3
    assert HW in R.BACKWARD_HW and C in R.BACKWARD_C
    y = _randn32(B, HW, C, seed=HW)
    y.reshape(-1)[::5] = 0.0
    y.reshape(-1)[1::7] = -0.0
    dout = _randn32(B, C, seed=C)
    yt = th.from_numpy(y.astype(np.float64)).requires_grad_()
    pooled = th.relu(yt).mean(dim=1)
    pooled.backward(th.from_numpy(dout.astype(np.float64)))
    np.testing.assert_allclose(R.avgpool_float64(np.maximum(y, 0)), pooled.detach().numpy(), rtol=1e-13, atol=1e-13)
    dy = R.avgpool_backward(dout, HW)
    assert dy.shape == (B, HW, C) and dy.dtype == np.float32
    assert np.array_equal(dy, th.from_numpy(dout)[:, None, :].div(th.tensor(float(HW))).expand(B, HW, C).numpy())
    dz = R.relu_backward(dy, y)
    assert dz.dtype == np.float32 and np.all(dz[y <= 0] == 0.0) and np.array_equal(dz[y > 0], dy[y > 0])
    # relu'(0) = 0 in torch as well; one float32 division against the float64 gradient
    np.testing.assert_allclose(dz, yt.grad.numpy(), rtol=2 * EPS, atol=0)


def test_avgpool_chain_lengths():
    assert R.avgpool_chain(7056, 32) == 56 + 3 + 32 and R.avgpool_chain(1, 32) == 1 + 3 + 32
    assert R.avgpool_chain(341, 12) == 2 + 3 + 85 and R.avgpool_chain(5, 1024) == 2 + 3 + 1
    assert R.avgpool_chain(3, 1028) == 3 and R.avgpool_chain(10, 6) == 10


# ---- Categorical head ----
@pytest.mark.parametrize("scale", R.CAT_SCALES)
@pytest.mark.parametrize("A", R.CAT_A)
@pytest.mark.parametrize("B", R.CAT_B)
def test_categorical_reference_is_torch_categorical(B, A, scale):
    logits, act = R.cat_inputs(B, A, scale)
    assert logits.dtype == np.float32 and act.min() >= 0 and act.max() < A
    for c_lp, c_ent in R.cat_coefs(B):
        x = th.from_numpy(logits.astype(np.float64)).requires_grad_()
        dist = th.distributions.Categorical(logits=x)
        logp, ent = dist.log_prob(th.from_numpy(act).long()), dist.entropy()
        (c_lp * logp + c_ent * ent).sum().backward()
        got = R.categorical_float64(logits, act, c_lp, c_ent)
        for g, w in zip(got, (logp.detach(), ent.detach(), x.grad)):
            assert np.all(np.isfinite(g))
            np.testing.assert_allclose(g, w.numpy(), rtol=1e-12, atol=1e-12 * max(abs(c_lp), abs(c_ent), 1.0))


def test_categorical_bound_is_four_times_torch_float32_error():
    """`conv_ref.CAT_TORCH_F32_ERROR` records what torch's own float32 `Categorical` and autograd lose against float64 on
    the GPU test's inputs; re-measured here (another libm may move it a little: within a factor of two of the record)."""
    worst = {}
    for scale in R.CAT_SCALES:
        for B in R.CAT_B:
            for A in R.CAT_A:
                logits, act = R.cat_inputs(B, A, scale)
                for c_lp, c_ent in R.cat_coefs(B):
                    ref = R.categorical_float64(logits, act, c_lp, c_ent)
                    x = th.from_numpy(logits).requires_grad_()
                    dist = th.distributions.Categorical(logits=x)
                    logp, ent = dist.log_prob(th.from_numpy(act).long()), dist.entropy()
                    (np.float32(c_lp) * logp + np.float32(c_ent) * ent).sum().backward()
                    got = (logp.detach().numpy(), ent.detach().numpy(), x.grad.numpy())
                    for name, g, r, u in zip(("logp", "entropy", "dlogits"), got, ref, (1.0, 1.0, max(abs(c_lp), abs(c_ent)))):
                        worst[name, scale] = max(worst.get((name, scale), 0.0), R.cat_error(g, r, u))
    assert set(worst) == set(R.CAT_TORCH_F32_ERROR)
    for k, recorded in R.CAT_TORCH_F32_ERROR.items():
        assert recorded / 2 <= worst[k] <= 2 * recorded, (k, worst[k], recorded)
        assert R.CAT_BOUND[k] == min(4 * recorded, 2e-5) and worst[k] < R.CAT_BOUND[k]
