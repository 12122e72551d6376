"""The float64 reference of the GEMM's implicit-convolution forms (`tests/gemm_view_ref.py`) against torch on the CPU:
`view` + `nt` is `torch.nn.functional.conv2d`, and the scattered transposed form is autograd's input gradient of a strided
`conv2d`. Everything in float64 at rtol 1e-12, so the oracle of `tests/test_gemm_views_gpu.py` is checked before a GPU
is involved."""
import numpy as np
import pytest
import torch as th
from torch.nn import functional as F

from tests import gemm_view_ref as R

RTOL = 1e-12   # also the absolute floor: sums of O(1) products that cancel to ~0 keep float64 rounding of ~1e-14


def _rand(*shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


@pytest.mark.parametrize("geom", R.NT_GEOMS + R.PAD_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_view_then_nt_is_conv2d(geom):
    B, H, W, Cin, KH, KW, S, P, Cout = geom
    x, Wt, bias = _rand(B, H, W, Cin, seed=1), _rand(Cout, KH, KW, Cin, seed=2), _rand(Cout, seed=3)
    OH, OW = R.out_size(H, KH, S, P), R.out_size(W, KW, S, P)
    V = R.view(x, KH, KW, S, P)
    assert V.shape == (B * OH * OW, KH * KW * Cin) and V.dtype == np.float64
    xt, wt = th.from_numpy(x).permute(0, 3, 1, 2), th.from_numpy(Wt).permute(0, 3, 1, 2)
    for b, act, f in [(bias, R.ACT_NONE, lambda z: z), (None, R.ACT_RELU, th.relu), (bias, R.ACT_RELU, th.relu)]:
        ref = f(F.conv2d(xt, wt, None if b is None else th.from_numpy(b), stride=S, padding=P))
        ref = ref.permute(0, 2, 3, 1).reshape(B * OH * OW, Cout).numpy()
        got = R.nt(x, Wt.reshape(Cout, -1), b, act, KH, KW, S, P)
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=RTOL)


@pytest.mark.parametrize("geom", R.NT_GEOMS[:3] + R.PAD_GEOMS[:1] + R.PAD_GEOMS[3:4], ids=lambda g: "x".join(map(str, g)))
def test_tn_is_conv2d_weight_gradient(geom):
    B, H, W, Cin, KH, KW, S, P, Cout = geom
    x, Wt = _rand(B, H, W, Cin, seed=1), _rand(Cout, KH, KW, Cin, seed=2)
    OH, OW = R.out_size(H, KH, S, P), R.out_size(W, KW, S, P)
    dout = _rand(B * OH * OW, Cout, seed=4)
    wt = th.from_numpy(Wt).permute(0, 3, 1, 2).contiguous().requires_grad_()
    bt = th.zeros(Cout, dtype=th.float64, requires_grad=True)
    y = F.conv2d(th.from_numpy(x).permute(0, 3, 1, 2), wt, bt, stride=S, padding=P)
    y.backward(th.from_numpy(dout).reshape(B, OH, OW, Cout).permute(0, 3, 1, 2))
    dW, db = R.tn(dout, x, 3, KH, KW, S, P)
    np.testing.assert_allclose(dW, wt.grad.permute(0, 2, 3, 1).reshape(Cout, -1).numpy(), rtol=RTOL, atol=RTOL)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=RTOL, atol=RTOL)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("geom", R.SCATTER_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_scattered_transposed_form_is_conv2d_input_gradient(geom, with_mask, form):
    """The input gradient of a stride-S convolution as one padded stride-1 product over `dout` per sub-pixel class, its rows
    scattered onto the input grid. With (h - k) % S != 0 the pixels no window reaches are in no class: absent from the
    written set (NaN in the reference), and their true gradient is zero."""
    k, S, h, w, Cin, Cout = geom
    B, kt = 2, k // S
    W_ = _rand(Cout, k, k, Cin, seed=2)
    x = th.from_numpy(_rand(B, h, w, Cin, seed=1)).permute(0, 3, 1, 2).contiguous().requires_grad_()
    y = F.conv2d(x, th.from_numpy(W_).permute(0, 3, 1, 2), stride=S)
    OH, OW = y.shape[2], y.shape[3]
    dout = _rand(B, OH, OW, Cout, seed=4)
    y.backward(th.from_numpy(dout).permute(0, 3, 1, 2))
    dx = x.grad.permute(0, 2, 3, 1).numpy()                                   # [B, h, w, Cin]
    mask = np.maximum(_rand(B, h, w, Cin, seed=5), 0.0) if with_mask else None
    want = dx if mask is None else np.where(mask > 0, dx, 0.0)
    gh, gw = OH + kt - 1, OW + kt - 1

    if form == 2:
        Wd_all = np.concatenate([R.dgrad_weights(W_, S, py, px) for py in range(S) for px in range(S)])
        rows = R.nt(dout, Wd_all, None, R.ACT_NONE, kt, kt, 1, kt - 1)
        got = R.scatter(rows, (S, -1, -1, h, w), (B, gh, gw), mask)
    else:
        got = np.full((B, h, w, Cin), np.nan)
        for py in range(S):
            for px in range(S):
                rows = R.nt(dout, R.dgrad_weights(W_, S, py, px), None, R.ACT_NONE, kt, kt, 1, kt - 1)
                one = R.scatter(rows, (S, py, px, h, w), (B, gh, gw), mask)
                new = ~np.isnan(one)
                assert not (new & ~np.isnan(got)).any(), "two classes write one pixel"
                got[new] = one[new]
    written = ~np.isnan(got)
    # the written set is exactly the pixels below S*gh x S*gw; the rest of the grid is reached by no window
    inside = np.zeros((B, h, w, Cin), dtype=bool)
    inside[:, :S * gh, :S * gw] = True
    assert np.array_equal(written, inside)
    if (h - k) % S or (w - k) % S:
        assert not written.all()
    np.testing.assert_allclose(got[written], want[written], rtol=RTOL, atol=RTOL)
    assert np.all(dx[~written] == 0.0)
    if with_mask:
        assert np.all(got[written & (mask <= 0)] == 0.0)
