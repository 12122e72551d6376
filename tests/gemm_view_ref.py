"""Float64 reference of the GEMM's implicit-convolution forms (`ia_gemm_f32_im2col`, `ia_gemm_f32_im2col_pad`),
written from the definition of the operation with explicit index arithmetic: numpy only, no GPU, no project
kernel. `tests/test_gemm_view_ref.py` checks it against `torch.nn.functional.conv2d` and autograd before
`tests/test_gemm_views_gpu.py` uses it as the oracle of the kernels.

Activations are channel-last `[B, H, W, C]`; the column index of the view is `(i, j, c)` (kernel row, kernel column,
channel), i.e. weights are kept as `[Cout, KH, KW, Cin]`."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SOFTPLUS = 0, 1, 2, 3


def out_size(n, k, S, P):
    """Number of window positions along one axis of extent `n`."""
    return (n + 2 * P - k) // S + 1


def view(x, KH, KW, S=1, P=0):
    """x[B, H, W, Cin] -> V[B*OH*OW, KH*KW*Cin] (float64): row (b, oh, ow), column (i, j, c) holds
    x[b, oh*S - P + i, ow*S - P + j, c], or zero where that tap lies outside the image."""
    x = np.asarray(x, dtype=np.float64)
    B, H, W, C = x.shape
    OH, OW = out_size(H, KH, S, P), out_size(W, KW, S, P)
    xp = np.zeros((B, H + 2 * P, W + 2 * P, C))
    xp[:, P:P + H, P:P + W] = x
    ys = np.arange(OH)[:, None] * S + np.arange(KH)[None, :]      # [OH, KH]: row of tap i of window oh (padded frame)
    xs = np.arange(OW)[:, None] * S + np.arange(KW)[None, :]      # [OW, KW]
    V = xp[:, ys[:, None, :, None], xs[None, :, None, :], :]      # [B, OH, OW, KH, KW, C]
    return V.reshape(B * OH * OW, KH * KW * C)


def apply_act(z, act):
    if act == ACT_NONE:
        return z
    if act == ACT_RELU:
        return np.maximum(z, 0.0)
    if act == ACT_TANH:
        return np.tanh(z)
    if act == ACT_SOFTPLUS:
        return np.logaddexp(z, 0.0)
    raise ValueError(act)


def nt(x, Wt, bias, act, KH, KW, S=1, P=0):
    """act(V . Wt^T + bias): Wt[N, KH*KW*Cin], bias[N] or None -> [B*OH*OW, N]."""
    z = view(x, KH, KW, S, P) @ np.asarray(Wt, dtype=np.float64).T
    if bias is not None:
        z = z + np.asarray(bias, dtype=np.float64)
    return apply_act(z, act)


def tn(dout, x, splits, KH, KW, S=1, P=0):
    """(dout^T . V, column sums of dout): dout[rows, Cout] -> ([Cout, KH*KW*Cin], [Cout]). These are the SUMS over the
    `splits` slabs of the split product: however the rows are divided among the slabs, every row is in exactly one."""
    assert splits >= 1
    dout = np.asarray(dout, dtype=np.float64)
    V = view(x, KH, KW, S, P)
    assert dout.shape[0] == V.shape[0]
    return dout.T @ V, dout.sum(0)


def scatter(rows, cmap, grid, mask=None):
    """Places the rows of a `[B*gh*gw, N]` product on a `[B, H_out, W_out, C]` grid; `grid = (B, gh, gw)`, `cmap =
    (S_out, py, px, H_out, W_out)`: row (b, y', x') of class (py, px) goes to pixel (b, y'*S_out + py, x'*S_out + px).
    Form 1 (py, px >= 0): one class, C = N. Form 2 (py < 0): all S_out^2 classes side by side along the columns,
    C = N / S_out^2, class = column // C, py = class // S_out, px = class % S_out. `mask` (like the output): the
    output is zero where mask <= 0. Pixels that no row reaches are NaN in the result."""
    rows = np.asarray(rows, dtype=np.float64)
    S_out, py0, px0, H_out, W_out = (int(v) for v in cmap)
    B, gh, gw = grid
    M, N = rows.shape
    assert M == B * gh * gw
    if py0 >= 0:
        classes, C = [(py0, px0, 0)], N
    else:
        assert N % (S_out * S_out) == 0
        C = N // (S_out * S_out)
        classes = [(cls // S_out, cls % S_out, cls * C) for cls in range(S_out * S_out)]
    out = np.full((B, H_out, W_out, C), np.nan)
    hits = np.zeros((B, H_out, W_out), dtype=np.int64)
    r = rows.reshape(B, gh, gw, N)
    for py, px, c0 in classes:
        for b in range(B):
            for yy in range(gh):
                for xx in range(gw):
                    y, x_ = yy * S_out + py, xx * S_out + px
                    assert y < H_out and x_ < W_out, "row outside the output grid"
                    out[b, y, x_] = r[b, yy, xx, c0:c0 + C]
                    hits[b, y, x_] += 1
    assert hits.max() <= 1, "two rows of the product land on one pixel"
    if mask is not None:
        mask = np.asarray(mask, dtype=np.float64)
        assert mask.shape == out.shape
        out = np.where(np.isnan(out), out, np.where(mask > 0, out, 0.0))
    return out


def dgrad_weights(W, S, py, px):
    """The `kt x kt` (kt = k / S) stride-1 kernel of sub-pixel class (py, px) of the input gradient of a stride-S
    convolution with weights W[Cout, k, k, Cin]: Wd[c, ti, tj, co] = W[co, py + S (kt-1-ti), px + S (kt-1-tj), c],
    returned as the GEMM operand [Cin, kt*kt*Cout]."""
    W = np.asarray(W)
    cout, k, k2, cin = W.shape
    assert k == k2 and k % S == 0
    kt = k // S
    Wd = np.empty((cin, kt, kt, cout), dtype=W.dtype)
    for ti in range(kt):
        for tj in range(kt):
            Wd[:, ti, tj, :] = W[:, py + S * (kt - 1 - ti), px + S * (kt - 1 - tj), :].T
    return Wd.reshape(cin, kt * kt * cout)


# ---- the geometries both test files run: (B, H, W, Cin, KH, KW, S, P, Cout) ----
NT_GEOMS = [
    (1, 20, 20, 32, 4, 4, 2, 0, 64),     # M = 81: one interior 64-row tile and a guarded tail
    (3, 20, 20, 32, 4, 4, 2, 0, 64),     # M = 243
    (5, 9, 9, 64, 3, 3, 1, 0, 64),       # M = 245
    (3, 20, 20, 32, 4, 4, 2, 0, 32),     # N == 32 and M >= 128: an interior 128 x 32 tile
    (4, 10, 13, 8, 2, 4, 3, 0, 20),      # non-square image and kernel; N <= 32 takes the 128 x 32 tile
    (4, 10, 13, 8, 2, 4, 3, 0, 70),      # N tail
    (7, 5, 4, 8, 3, 4, 1, 0, 33),        # W == KW: OW == 1
    (130, 3, 4, 8, 3, 4, 1, 0, 64),      # OH*OW == 1: every row its own image
]
PAD_GEOMS = [
    (3, 5, 7, 32, 3, 3, 1, 1, 64),       # reward-CNN form ("same" 3 x 3)
    (2, 9, 11, 64, 3, 3, 1, 2, 32),      # whole kernel rows outside the image
    (3, 6, 5, 16, 2, 2, 1, 1, 32),       # P = k - 1: the "full" form of the input gradients
    (4, 8, 9, 32, 4, 4, 2, 1, 32),       # strided and padded
    (70, 1, 1, 32, 3, 3, 1, 1, 32),      # clamp against H - 1 == W - 1 == 0
]
# input gradients of a stride-S convolution: (k, S, h, w, Cin, Cout); kt = k / S, (kt * Cout) % 32 == 0
SCATTER_GEOMS = [
    (4, 2, 20, 20, 24, 16),              # the classes cover the whole grid; 4 * 24 = 96 fused columns (N tail of a 64-wide tile)
    (4, 2, 21, 23, 8, 16),               # row 20 and column 22 belong to no class
    (3, 3, 9, 12, 8, 32),                # kt = 1, P = 0
]
