"""NumPy references of the convolution data-movement kernels of `csrc/conv.hip` (both `im2col` forms, both `col2im`
forms and their padded variants, the average pool and its backward, `relu_backward`, the Categorical head) and of
`ia_avgpool_relu_backward` (`csrc/conv3x3.hip`): each function restates one kernel's documented contract with plain
index arithmetic -- numpy only, no torch, no GPU, no project kernel. `tests/test_conv_ref.py` checks them against
torch float64 on the CPU before `tests/test_conv_kernels_gpu.py` uses them as the oracle of the kernels.

Data movement and the fixed-order float32 sums are reproduced to the bit (float32 arithmetic, the kernel's order); the
two operations with real rounding -- the pool's sum and the Categorical head -- get a float64 reference.

Column orders: the uint8 channel-first form has columns `(c, i, j)` (torch's `[Cout, Cin, KH, KW]` weights flattened), the
float32 channel-last forms have columns `(i, j, c)` (weights kept as `[Cout, KH, KW, Cin]`); rows are `(b, oh, ow)`."""
import numpy as np


def out_size(n, k, S, P=0):
    """Number of window positions along one axis of extent `n`."""
    return (n + 2 * P - k) // S + 1


def im2col_u8_nchw(x, KH, KW, S, scale):
    """x[B, C, H, W] uint8 -> col[B*OH*OW, C*KH*KW] float32, col[(b, oh, ow)][(c, i, j)] = float(x[b, c, oh*S+i, ow*S+j]) *
    scale: one IEEE float32 multiply per element."""
    x = np.asarray(x)
    assert x.dtype == np.uint8
    B, C, H, W = x.shape
    OH, OW = out_size(H, KH, S), out_size(W, KW, S)
    ys = np.arange(OH)[:, None] * S + np.arange(KH)[None, :]          # [OH, KH]
    xs = np.arange(OW)[:, None] * S + np.arange(KW)[None, :]          # [OW, KW]
    V = x[:, :, ys[:, None, :, None], xs[None, :, None, :]]           # [B, C, OH, OW, KH, KW]
    V = V.transpose(0, 2, 3, 1, 4, 5).reshape(B * OH * OW, C * KH * KW)
    return V.astype(np.float32) * np.float32(scale)


def im2col_f32_nhwc(x, KH, KW, S, P=0):
    """x[B, H, W, C] float32 -> col[B*OH*OW, KH*KW*C] float32, col[(b, oh, ow)][(i, j, c)] = x[b, oh*S+i-P, ow*S+j-P, c], zero
    where that tap lies outside the image."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    B, H, W, C = x.shape
    OH, OW = out_size(H, KH, S, P), out_size(W, KW, S, P)
    xp = np.zeros((B, H + 2 * P, W + 2 * P, C), dtype=np.float32)
    xp[:, P:P + H, P:P + W] = x
    ys = np.arange(OH)[:, None] * S + np.arange(KH)[None, :]
    xs = np.arange(OW)[:, None] * S + np.arange(KW)[None, :]
    V = xp[:, ys[:, None, :, None], xs[None, :, None, :], :]          # [B, OH, OW, KH, KW, C]
    return V.reshape(B * OH * OW, KH * KW * C)


def _axis_range(n, k, S, P, n_out):
    """Windows o in [0, n_out) whose tap k lands inside [0, n): (first o, last o) or None."""
    lo = max(0, -((k - P) // S))                 # ceil((P - k) / S)
    hi = min(n_out - 1, (n - 1 + P - k) // S)
    return (lo, hi) if lo <= hi else None


def col2im_nhwc(dcol, B, H, W, C, KH, KW, S, P=0, mask=None, *, taps=None, origin=0):
    """dcol[B*OH*OW, KH*KW*C] float32 -> dx[B, H, W, C] float32: dx[b, h, w, c] = the sum of dcol[(b, oh, ow)][(i, j, c)] over
    the windows with oh*S+i-P == h and ow*S+j-P == w, accumulated in float32 in increasing (i, j) order starting from zero
    (a pixel receives at most one term per (i, j), so whole-array updates per tap give every pixel its terms in that
    order). Pixels no window covers stay exactly 0. `mask` (like dx): the value is kept where mask > 0 and is 0 elsewhere.

    `taps` (another visiting order of the (i, j) pairs) and `origin` (the windows' origin moved by that many pixels) exist
    for `test_conv_ref`'s sharpness test alone."""
    dcol = np.asarray(dcol)
    assert dcol.dtype == np.float32
    OH, OW = out_size(H, KH, S, P), out_size(W, KW, S, P)
    d = dcol.reshape(B, OH, OW, KH, KW, C)
    dx = np.zeros((B, H, W, C), dtype=np.float32)
    if taps is None:
        taps = [(i, j) for i in range(KH) for j in range(KW)]
    Po = P - origin
    for i, j in taps:
        rh, rw = _axis_range(H, i, S, Po, OH), _axis_range(W, j, S, Po, OW)
        if rh is None or rw is None:
            continue
        h0, h1 = rh[0] * S + i - Po, rh[1] * S + i - Po
        w0, w1 = rw[0] * S + j - Po, rw[1] * S + j - Po
        dx[:, h0:h1 + 1:S, w0:w1 + 1:S, :] += d[:, rh[0]:rh[1] + 1, rw[0]:rw[1] + 1, i, j, :]
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.shape == dx.shape
        dx = np.where(mask > 0, dx, np.float32(0))
    return dx


def avgpool_backward(dout, HW):
    """dout[B, C] float32 -> dy[B, HW, C] float32 = dout / float32(HW) at every position: one IEEE division."""
    dout = np.asarray(dout)
    assert dout.dtype == np.float32
    q = dout / np.float32(HW)
    return np.broadcast_to(q[:, None, :], (dout.shape[0], HW, dout.shape[1])).copy()


def relu_backward(dy, y):
    """dy where y > 0, 0 elsewhere (also at y = -0.0)."""
    dy = np.asarray(dy)
    return np.where(np.asarray(y) > 0, dy, dy.dtype.type(0))


def avgpool_float64(y):
    """y[B, HW, C] -> the float64 mean over the positions, [B, C]."""
    return np.asarray(y, dtype=np.float64).mean(axis=1)


def avgpool_chain(HW, C):
    """Length of the longest chain of float32 additions behind one output of `ia_avgpool_nhwc`. Channel counts that are
    a multiple of 4 up to 1024: the positions are dealt over G = 256 // (C/4) groups, a group sums its positions in four
    interleaved chains (at most ceil(HW / 4G) + 1 terms each), folds the four (2 more) and the groups are added in order
    (G - 1 more): at most ceil(HW / 4G) + 3 + G. Every other channel count: one chain over the HW positions."""
    if C % 4 == 0 and C <= 1024:
        G = 256 // (C // 4)
        return -(-HW // (4 * G)) + 3 + G
    return HW


def categorical_float64(logits, act, c_lp, c_ent):
    """logits[B, A], act[B] -> (logp[B], entropy[B], dlogits[B, A]) in float64, from a log-sum-exp: z = log_softmax(logits),
    p = exp(z), logp = z[act], entropy H = -sum_k p_k z_k, dlogits = d(c_lp * logp + c_ent * H) / dlogits
    = c_lp * (onehot(act) - p) - c_ent * p * (z + H)."""
    x = np.asarray(logits, dtype=np.float64)
    a = np.asarray(act).astype(np.int64)
    B, A = x.shape
    mx = x.max(axis=1, keepdims=True)
    z = x - (mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True)))
    p = np.exp(z)
    Hn = -(p * z).sum(axis=1)
    onehot = np.zeros((B, A))
    onehot[np.arange(B), a] = 1.0
    d = float(c_lp) * (onehot - p) - float(c_ent) * p * (z + Hn[:, None])
    return z[np.arange(B), a], Hn, d


# ---- the geometries both test files run ----
# ia_im2col_u8_nchw: (B, C, H, W, KH, KW, S)
U8_KW8_GEOMS = [
    (2, 4, 36, 36, 8, 8, 4),       # NatureCNN's first layer (smaller frame): C*KH = 32, 8 rows per pass
    (3, 3, 20, 24, 8, 8, 4),       # C*KH = 24 does not divide 256: 10 rows per pass, 16 idle threads; M = 60, one partial block
    (1, 1, 8, 8, 8, 8, 4),         # M = 1
    (2, 16, 12, 16, 8, 8, 8),      # K = 1024, the limit; stride 8
    (5, 4, 44, 60, 8, 8, 4),       # H != W; M = 700 is no multiple of the block's 128 rows
]
U8_GENERIC_GEOMS = [
    (2, 4, 36, 37, 8, 8, 4),       # W % 4 != 0
    (2, 3, 12, 12, 8, 8, 2),       # S % 4 != 0
    (2, 4, 9, 11, 3, 5, 2),        # KW != 8, KH != KW, K = 60 < 256: three of a thread's four columns are idle
    (1, 4, 16, 16, 16, 16, 1),     # K = 1024: four columns per thread
]
U8_REJECTED = (1, 17, 8, 8, 8, 8, 4)   # K = 1088 > 1024
# ia_im2col_f32_nhwc / ia_col2im_nhwc: (B, H, W, C, KH, KW, S)
# (col2im: C % 4 == 0 with 16-byte aligned buffers takes the four-channel vector kernel, every other C the scalar one)
F32_GEOMS = [
    (2, 8, 8, 32, 4, 4, 2),        # NatureCNN's second layer (smaller image); col2im: vector kernel
    (3, 7, 9, 64, 3, 3, 1),        # 3 x 3, stride 1: nine terms per interior pixel; col2im: vector kernel
    (1, 5, 6, 3, 2, 3, 2),         # odd sizes, KH != KW; col2im: C = 3, scalar kernel
    (2, 4, 4, 64, 4, 4, 1),        # K = 1024, four columns per thread; col2im: vector kernel
    (1, 3, 3, 5, 3, 3, 1),         # M = 1; col2im: C = 5, scalar kernel
]
F32_REJECTED = (1, 4, 4, 65, 4, 4, 1)   # K = 1040 > 1024
# ia_im2col_f32_nhwc_pad / ia_col2im_nhwc_pad: (B, H, W, C, K, S, P), square K x K kernels
F32_PAD_GEOMS = [
    (2, 5, 7, 4, 3, 1, 1),         # the ordinary "same" 3 x 3
    (1, 4, 4, 3, 3, 2, 1),         # stride 2 with padding
    (2, 6, 5, 8, 5, 1, 2),         # 5 x 5, P = 2
    (1, 3, 3, 2, 3, 1, 2),         # P = K - 1: the corner windows hold one pixel of the image, the rest is border
    (1, 3, 3, 2, 3, 1, 3),         # P = K: the outer ring of windows lies wholly in the border, rows that are exactly zero
    (1, 1, 1, 32, 3, 1, 1),        # a single pixel
    (1, 4, 4, 128, 3, 1, 1),       # K = 1152: the padded form has no column limit
]
# ia_col2im_nhwc only: (B, H, W, C, KH, KW, S)
COL2IM_GAP_GEOMS = [
    (2, 7, 8, 4, 2, 2, 3),         # S > K: the pixels between the windows are covered by none; C = 4, vector kernel
    (2, 10, 11, 8, 4, 4, 3),       # (H - KH) % S != 0: the tail rows and columns are covered by none; C = 8, vector kernel
]
# ia_avgpool_nhwc: (HW, C); every one with B in AVGPOOL_BATCHES
AVGPOOL_SHAPES = (
    [(hw, 32) for hw in (1, 31, 32, 33, 127, 128, 129, 7056)] +   # 8 quads, G = 32 groups: HW below, at and above G and 4G
    [(hw, 12) for hw in (9, 85, 86, 341)] +                       # 3 quads, G = 85 groups and one idle thread
    [(hw, 4) for hw in (255, 257, 1025)] +                        # 1 quad, G = 256
    [(5, 1024)] +                                                 # 256 quads, one group
    [(3, 1028)] +                                                 # more than 256 quads: a thread per channel, loop past 256
    [(10, c) for c in (1, 3, 6)]                                  # C % 4 != 0: a thread per channel
)
AVGPOOL_BATCHES = (1, 3)
# backward of the pool / ReLU: HW x C
BACKWARD_HW = (1, 7, 35, 64)
BACKWARD_C = (3, 8, 32)
# ia_categorical_loss
CAT_B = (1, 128, 129, 300)
CAT_A = (1, 2, 6, 18)
CAT_SCALES = (1.0, 40.0)


# Error of torch-CPU float32 `Categorical` (log_prob, entropy, autograd of c_lp * logp + c_ent * H) against
# `categorical_float64`, as `cat_error` (gradients with unit = max(|c_lp|, |c_ent|)), the largest over every B, A and
# coefficient pair above at one logit scale: {(output, scale): error}. With 40 * randn logits the row maximum is ~100, so
# one float32 rounding of the log-sum-exp (ulp(128) / 2 = 3.8e-6) is most of the error of a log-prob near 0.
CAT_TORCH_F32_ERROR = {
    ("logp", 1.0): 1.28e-7, ("entropy", 1.0): 1.70e-7, ("dlogits", 1.0): 2.13e-7,
    ("logp", 40.0): 3.41e-6, ("entropy", 40.0): 3.78e-6, ("dlogits", 40.0): 3.72e-6,
}
# The kernel's bound: 4 x that error (device expf / logf differ from the host's libm by a few ulp, and the sums run in
# another order), never looser than the rtol = atol = 2e-5 the policy-level test grants the same quantities.
CAT_BOUND = {k: min(4.0 * v, 2e-5) for k, v in CAT_TORCH_F32_ERROR.items()}


def cat_coefs(B):
    """The (c_lp, c_ent) pairs: BC's loss coefficients at batch B, log-prob alone, entropy alone."""
    return [(-0.7 / B, -0.01 / B), (1.0, 0.0), (0.0, 1.0)]


def cat_inputs(B, A, scale):
    """Seeded float32 logits[B, A] (unit normals times `scale`) and actions[B] in [0, A)."""
    rng = np.random.default_rng(1000 * B + 10 * A + int(scale))
    logits = (rng.standard_normal((B, A)) * scale).astype(np.float32)
    act = rng.integers(0, A, size=B).astype(np.float32)
    return logits, act


def cat_error(got, ref, unit=1.0):
    """The largest |got - ref| / (unit + |ref|): the left side of an `rtol == atol` comparison, in units of that tolerance,
    with the absolute part scaled by `unit` (the coefficient scale for gradients)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / (unit + np.abs(ref)))) if ref.size else 0.0
