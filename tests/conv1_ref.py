"""NumPy reference of the implicit first-layer convolution of `csrc/conv1_implicit.hip` (`ia_conv1_u8_forward`,
`ia_conv1_u8_wgrad`, `ia_conv1_u8_implicit_ok`): Conv2d(4, 32, 8, stride 4) on uint8 `[B, 4, H, W]` frames with `x * scale`
folded in, written from the definition as a product with the column matrix of `tests.conv_ref.im2col_u8_nchw` (which forms
`float32(x) * float32(scale)` with the kernel's single float32 multiply, columns `(c, i, j)`, rows `(b, oh, ow)`) -- numpy
only, no torch, no GPU, no project kernel. `tests/test_conv1_ref.py` checks it against torch float64 on the CPU before
`tests/test_conv1_implicit_gpu.py` uses it as the oracle of the kernels.

Every function comes twice: in float64 (the oracle of the float cases) and in int64 on integer operands with `scale = 1`
(the oracle of the exact cases: every partial sum is an integer below 2^24, so float32 accumulation in ANY order gives these
very integers). The inputs of both kinds of case are generated here, so the CPU and the GPU tests see the same arrays."""
import math

import numpy as np

from tests.conv_ref import im2col_u8_nchw, out_size

C1, K1, S1, CO1 = 4, 8, 4, 32          # channels, kernel extent, stride, output channels
KTOT = C1 * K1 * K1                    # 256 columns


def npix(H, W):
    """Output pixels per image."""
    return out_size(H, K1, S1) * out_size(W, K1, S1)


def columns(x, scale):
    """x[B, 4, H, W] uint8 -> col[B*OH*OW, 256] float32 = float32(x) * float32(scale) at column (c, i, j)."""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[1] == C1
    return im2col_u8_nchw(x, K1, K1, S1, scale)


def forward(x, W, bias, scale, *, col=None):
    """out[B*OH*OW, 32] = max(col . W^T + bias, 0) in float64. `col` (another column matrix in place of `columns(x, scale)`)
    exists for `test_conv1_ref`'s sharpness test alone."""
    col = columns(x, scale) if col is None else col
    W, bias = np.asarray(W, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    assert W.shape == (CO1, KTOT) and bias.shape == (CO1,)
    return np.maximum(col.astype(np.float64) @ W.T + bias, 0.0)


def wgrad(x, dout, scale, *, col=None):
    """(dW[32, 256] = dout^T . col, db[32] = the column sums of dout), float64. `col` as in `forward`."""
    col = columns(x, scale) if col is None else col
    dout = np.asarray(dout, dtype=np.float64)
    assert dout.shape == (col.shape[0], CO1)
    return dout.T @ col.astype(np.float64), dout.sum(axis=0)


def _int(a):
    a = np.asarray(a)
    i = np.rint(a).astype(np.int64)
    assert np.array_equal(i, a), "the integer forms take integer-valued operands"
    return i


def columns_int(x):
    """`columns(x, 1.0)` as int64: the bytes themselves."""
    return _int(columns(x, 1.0))


def forward_int(x, W, bias, *, col=None):
    """`forward` at scale 1 on integer-valued W and bias, in int64."""
    col = columns_int(x) if col is None else col
    return np.maximum(col @ _int(W).T + _int(bias), 0)


def wgrad_int(x, dout, *, col=None):
    """`wgrad` at scale 1 on integer-valued dout, in int64."""
    col = columns_int(x) if col is None else col
    d = _int(dout)
    return d.T @ col, d.sum(axis=0)


def shape_ok(C, H, W, KH, KW, S, Cout):
    """The documented predicate of `ia_conv1_u8_implicit_ok`: 4 channels, 8 x 8 kernel, stride 4, 32 output channels;
    H, W >= 8; W % 4 == 0 (a window's row is two aligned dwords); OW even and >= 2 (the weight gradient steps through an
    output row in pixel pairs); two images as bytes within 64 KiB of LDS (forward); one image as bytes and its
    [OH*OW, 32] float32 dout within 80 KiB (weight gradient)."""
    if (C, KH, KW, S, Cout) != (C1, K1, K1, S1, CO1):
        return False
    if H < K1 or W < K1 or W % 4 != 0:
        return False
    OH, OW = out_size(H, K1, S1), out_size(W, K1, S1)
    if OW < 2 or OW % 2 != 0:
        return False
    return 2 * C1 * H * W <= 64 * 1024 and C1 * H * W + OH * OW * CO1 * 4 <= 80 * 1024


SCAN = range(8, 101)                   # the H and W of the predicate table


def ok_table():
    """bool [93, 93]: `shape_ok(4, H, W, 8, 8, 4, 32)` at [H - 8, W - 8] for 8 <= H, W <= 100."""
    return np.array([[shape_ok(C1, H, W, K1, K1, S1, CO1) for W in SCAN] for H in SCAN])


def largest_ok_H(W):
    """The largest accepted H <= 100 at width W."""
    return max(H for H in SCAN if shape_ok(C1, H, W, K1, K1, S1, CO1))


# ---- the cases both test files run ----
# (H, W): what the frame shape exercises in the kernels (npix output pixels per image in 32-pixel tiles for the forward,
# half = OW / 2 steps per output row in groups of 5 for the weight gradient)
SHAPES = [
    (8, 12),                           # npix = 2, half = 1: remainder loop only
    (11, 12),                          # the same, with three rows of H that no window reads
    (12, 20),                          # npix = 8
    (36, 20),                          # npix = 32: exactly one full tile
    (36, 36),                          # npix = 64
    (44, 36),                          # npix = 80: three tiles, the last partial; with two images the pairs u / u + 4 straddle them
    (44, 60),                          # npix = 140, half = 7: one group of 5 plus a remainder of 2
    (84, 84),                          # npix = 400, half = 10, 13 tiles: the benchmark's frame
    (largest_ok_H(84), 84),            # the LDS budget at its limit
]
BATCHES = (1, 2, 3, 7)
LOOP_SHAPES = SHAPES[0], SHAPES[2]     # 384 and 960 bytes per frame: the shapes of the batch sizes beyond the grid


def looped_batches(cus):
    """(forward, weight gradient) batch sizes at which the persistent grids (2 * cus workgroups; two images per forward
    workgroup, one per weight-gradient workgroup) loop: the forward's second sweep holds a full pair and a lone image."""
    return (4 * cus + 3,), (2 * cus + 3, 4 * cus + 1)


def frames(B, H, W, seed):
    """Seeded random bytes [B, 4, H, W] with 0 in the first and 255 in the last pixel of every channel."""
    x = np.random.default_rng(seed).integers(0, 256, size=(B, C1, H, W), dtype=np.uint8)
    x[:, :, 0, 0] = 0
    x[:, :, -1, -1] = 255
    return x


def _seed(B, H, W):
    return 100003 * B + 101 * H + W


def int_inputs(B, H, W):
    """(x, W, bias, dout) of an exact case: weights, bias and dout integers in [-2, 2] (as float32), about half of dout 0."""
    rng = np.random.default_rng(_seed(B, H, W) + 1)
    rows = B * npix(H, W)
    Wt = rng.integers(-2, 3, size=(CO1, KTOT)).astype(np.float32)
    bias = rng.integers(-2, 3, size=CO1).astype(np.float32)
    dout = (rng.integers(-2, 3, size=(rows, CO1)) * (rng.random((rows, CO1)) < 0.5)).astype(np.float32)
    return frames(B, H, W, _seed(B, H, W)), Wt, bias, dout


def int_bound(B, H, W):
    """The largest magnitude any partial sum of an exact case can reach: 256 products of 255 * 2 and the bias in the forward,
    one product of 255 * 2 per row in the weight gradient."""
    return max(KTOT * 255 * 2 + 2, B * npix(H, W) * 255 * 2)


def float_inputs(B, H, W):
    """(x, W, bias, dout) of a float case: weights unit normals / sqrt(256), bias unit normals, dout unit normals with a
    random half zeroed (as behind a ReLU mask); all float32."""
    rng = np.random.default_rng(_seed(B, H, W) + 2)
    rows = B * npix(H, W)
    Wt = (rng.standard_normal((CO1, KTOT)) / math.sqrt(KTOT)).astype(np.float32)
    bias = rng.standard_normal(CO1).astype(np.float32)
    dout = (rng.standard_normal((rows, CO1)) * (rng.random((rows, CO1)) < 0.5)).astype(np.float32)
    return frames(B, H, W, _seed(B, H, W)), Wt, bias, dout


SCALES = (1.0 / 255.0, 1.0 / 128.0)
# the project's tolerances for fp32 MFMA accumulation (tests/test_gemm_views_gpu.py): a 256-term product per forward output,
# a `rows`-term reduction per gradient element
FWD_RTOL, WGRAD_RTOL = 2e-5, 3e-5


def fwd_atol():
    return FWD_RTOL * math.sqrt(KTOT)


def wgrad_atol(rows):
    return WGRAD_RTOL * math.sqrt(rows)


def tol_ratio(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): at most 1 exactly when `assert_allclose(got, ref, rtol, atol)` passes."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref)))) if ref.size else 0.0
