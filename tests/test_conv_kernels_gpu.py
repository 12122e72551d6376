"""Kernel-level parity (`-m gpu`) of the convolution data-movement kernels: every C entry point of `csrc/conv.hip` --
`ia_im2col_u8_nchw`, `ia_im2col_f32_nhwc`, `ia_col2im_nhwc`, their `_pad` forms, `ia_avgpool_nhwc` and its backward,
`ia_relu_backward`, `ia_categorical_loss` -- and `ia_avgpool_relu_backward` (`csrc/conv3x3.hip`), called directly through
the C ABI against the NumPy references of `tests/conv_ref.py` (themselves checked on the CPU by `tests/test_conv_ref.py`).

The library is built with `-ffp-contract=off` and without fast-math, and all of this but two operations is data movement or
float32 addition in a documented order: those results are defined to the bit and compared as bits. The two tolerances are
the forward bound of a float32 sum for the pool (from the length of its addition chain, `conv_ref.avgpool_chain`) and
`conv_ref.CAT_BOUND` for the Categorical head (4 x the error of torch's own float32 `Categorical` on the same inputs).

Every output lies inside a larger NaN-filled buffer with a guard of at least one row on either side: the guard must come
back all NaN (no write out of bounds), every defined element finite, and two launches into fresh buffers bit-identical.
Each entry point dispatches between kernel variants by shape and pointer alignment; the dispatch condition is restated
here and asserted per case, so every variant is reached by a case that says so."""
import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from tests import conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
EPS = 2.0 ** -24   # unit roundoff of float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


_KEEP = []


@pytest.fixture(autouse=True)
def _release_temporaries():
    yield
    if th.cuda.is_available():
        th.cuda.synchronize()
    _KEEP.clear()


def gid(g):
    return "x".join(map(str, g))


def dev(x, shift=0):
    """Uploads a numpy array (dtype kept) and returns the flat device tensor, `shift` ELEMENTS into its allocation (the
    allocator's blocks are 256-byte aligned, so shift = 0 is aligned for every vector access and shift = 1 for none). The
    tensor stays alive until the test ends: raw pointers carry no ownership."""
    src = th.from_numpy(np.array(x, order="C").reshape(-1))
    buf = th.empty(src.numel() + shift, dtype=src.dtype, device=DEV)
    t = buf[shift:]
    t.copy_(src)
    assert buf.data_ptr() % 256 == 0 and t.data_ptr() == buf.data_ptr() + shift * src.element_size()
    _KEEP.append(buf)
    return t


class Guarded:
    """`n` float32 outputs, all NaN, inside a larger NaN-filled buffer: a guard of at least `rowlen` elements (a multiple of
    64, so the body keeps the buffer's 256-byte alignment) before and after; `shift` moves the body that many floats."""

    def __init__(self, n, rowlen, shift=0):
        self.n, self.lo = n, (max(rowlen, 1) + 63) // 64 * 64 + shift
        self.buf = th.full((self.lo + n + (max(rowlen, 1) + 63) // 64 * 64,), NAN, device=DEV)
        self.body = self.buf[self.lo:self.lo + n]
        _KEEP.append(self.buf)

    def guard_intact(self):
        return bool(th.isnan(self.buf[:self.lo]).all()) and bool(th.isnan(self.buf[self.lo + self.n:]).all())


def bits_equal(a, b):
    return th.equal(a.view(th.int32), b.view(th.int32))


def call(name, *args):
    """The entry point's return code (`L.call` would raise on the rejections that some cases expect)."""
    return int(getattr(L.load(), name)(*args))


def launch_twice(what, n, rowlen, launch, shift=0, rc=0):
    """`launch(out)` -> return code, into two fresh guarded NaN buffers: both return `rc`, both guards stay NaN, the two bodies
    are bit-identical. Returns the first body (a device tensor)."""
    outs = []
    for _ in range(2):
        o = Guarded(n, rowlen, shift)
        got_rc = launch(o.body)
        th.cuda.synchronize()
        assert got_rc == rc, f"{what}: returned {got_rc}, expected {rc}"
        assert o.guard_intact(), f"{what}: wrote outside its output"
        outs.append(o)
    assert bits_equal(outs[0].body, outs[1].body), f"{what}: two launches differ"
    return outs[0].body


def assert_bits(what, got, ref):
    """`got` (device) equals `ref` (numpy float32) bit for bit, and every element is finite."""
    got = got.cpu().numpy().reshape(ref.shape)
    assert np.all(np.isfinite(got)), f"{what}: {np.sum(~np.isfinite(got))} defined elements not finite"
    same = got.view(np.int32) == np.ascontiguousarray(ref).view(np.int32)
    assert same.all(), f"{what}: {np.sum(~same)} of {same.size} elements differ, first at {np.argwhere(~same)[0]}"


def randn32(*shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def relu_like(*shape, seed):
    """Unit normals with exact +0.0 and -0.0 sprinkled in: what a mask / ReLU output must be tested with."""
    y = randn32(*shape, seed=seed)
    flat = y.reshape(-1)
    flat[::5] = 0.0
    flat[1::7] = -0.0
    assert (flat > 0).any() and (flat < 0).any() and np.signbit(flat[flat == 0]).any() and not np.signbit(flat[flat == 0]).all()
    return y


# ------------------------------------------------------------------------------------------------------------------
# a. ia_im2col_u8_nchw
# ------------------------------------------------------------------------------------------------------------------
def frames(B, C, H, W):
    x = np.random.default_rng(3).integers(0, 256, size=(B, C, H, W), dtype=np.uint8)
    x.reshape(-1)[:2] = (0, 255)
    return x


def takes_kw8(geom, x):
    """The dispatch of `ia_im2col_u8_nchw`, restated: the vectorised KW == 8 kernel reads a window row as two aligned dwords."""
    B, C, H, W, KH, KW, S = geom
    return KW == 8 and S % 4 == 0 and W % 4 == 0 and C * KH <= 256 and x.data_ptr() % 4 == 0


def im2col_u8(geom, scale, shift=0):
    B, C, H, W, KH, KW, S = geom
    x = frames(B, C, H, W)
    xd = dev(x, shift)
    M, K = B * R.out_size(H, KH, S) * R.out_size(W, KW, S), C * KH * KW
    what = f"im2col_u8 {gid(geom)} scale={scale:.4g} shift={shift}"
    got = launch_twice(what, M * K, K, lambda out: call("ia_im2col_u8_nchw", L.ptr(xd), B, C, H, W, KH, KW, S, scale, L.ptr(out),
                                                        L.stream()))
    assert_bits(what, got, R.im2col_u8_nchw(x, KH, KW, S, scale))
    return got, takes_kw8(geom, xd)


@pytest.mark.parametrize("scale", [1 / 255, 1.0], ids=["1/255", "1"])
@pytest.mark.parametrize("geom", R.U8_KW8_GEOMS, ids=gid)
def test_im2col_u8_vectorised_kw8_kernel(geom, scale):
    """KW == 8, S % 4 == 0, W % 4 == 0, C*KH <= 256 and aligned frames: the (c, i)-pair-per-thread kernel (see each case's
    comment in `conv_ref.U8_KW8_GEOMS` for what it reaches there)."""
    _, kw8 = im2col_u8(geom, scale)
    assert kw8


@pytest.mark.parametrize("scale", [1 / 255, 1.0], ids=["1/255", "1"])
@pytest.mark.parametrize("geom", R.U8_GENERIC_GEOMS, ids=gid)
def test_im2col_u8_generic_kernel(geom, scale):
    """One of the KW == 8 path's conditions fails (which one: the case's comment in `conv_ref.U8_GENERIC_GEOMS`): the
    column-per-thread kernel."""
    _, kw8 = im2col_u8(geom, scale)
    assert not kw8


def test_im2col_u8_both_kernels_agree_bit_for_bit():
    """The first KW == 8 geometry with its frames one byte into their allocation is not dword aligned and takes the generic
    kernel: the same bits as the aligned call through the vectorised one."""
    for scale in (1 / 255, 1.0):
        a, kw8_a = im2col_u8(R.U8_KW8_GEOMS[0], scale)
        b, kw8_b = im2col_u8(R.U8_KW8_GEOMS[0], scale, shift=1)
        assert kw8_a and not kw8_b
        assert bits_equal(a, b)


def test_im2col_u8_rejects_more_than_1024_columns():
    B, C, H, W, KH, KW, S = R.U8_REJECTED
    assert C * KH * KW == 1088
    xd = dev(frames(B, C, H, W))
    out = launch_twice("im2col_u8 K=1088", 1088, 1088, lambda o: call("ia_im2col_u8_nchw", L.ptr(xd), B, C, H, W, KH, KW, S, 1.0,
                                                                     L.ptr(o), L.stream()), rc=L.ERR_ARG)
    assert bool(th.isnan(out).all()), "a rejected call wrote its output"


# ------------------------------------------------------------------------------------------------------------------
# b. ia_im2col_f32_nhwc, ia_im2col_f32_nhwc_pad
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", R.F32_GEOMS, ids=gid)
def test_im2col_f32(geom):
    """The unpadded entry (one kernel: a block walks 16 rows, a thread owns up to four columns), and the padded entry at
    P = 0 (another kernel: an element per thread), which must produce the same bits."""
    B, H, W, C, KH, KW, S = geom
    x = randn32(B, H, W, C, seed=1)
    xd = dev(x)
    M, K = B * R.out_size(H, KH, S) * R.out_size(W, KW, S), KH * KW * C
    ref = R.im2col_f32_nhwc(x, KH, KW, S)
    what = f"im2col_f32 {gid(geom)}"
    got = launch_twice(what, M * K, K, lambda o: call("ia_im2col_f32_nhwc", L.ptr(xd), B, H, W, C, KH, KW, S, L.ptr(o), L.stream()))
    assert_bits(what, got, ref)
    pad0 = launch_twice(what + " pad entry P=0", M * K, K,
                        lambda o: call("ia_im2col_f32_nhwc_pad", L.ptr(xd), B, H, W, C, KH, KW, S, 0, L.ptr(o), L.stream()))
    assert bits_equal(got, pad0), f"{what}: the padded entry at P = 0 differs from the unpadded entry"


def test_im2col_f32_rejects_more_than_1024_columns():
    B, H, W, C, KH, KW, S = R.F32_REJECTED
    assert KH * KW * C == 1040
    xd = dev(randn32(B, H, W, C, seed=1))
    out = launch_twice("im2col_f32 K=1040", 1040, 1040, lambda o: call("ia_im2col_f32_nhwc", L.ptr(xd), B, H, W, C, KH, KW, S, L.ptr(o),
                                                                       L.stream()), rc=L.ERR_ARG)
    assert bool(th.isnan(out).all()), "a rejected call wrote its output"


@pytest.mark.parametrize("geom", R.F32_PAD_GEOMS, ids=gid)
def test_im2col_f32_pad(geom):
    B, H, W, C, Kk, S, P = geom
    x = randn32(B, H, W, C, seed=1)
    x[x == 0] = 1.0                                   # so that a zero in the result can only be a border tap
    xd = dev(x)
    M, K = B * R.out_size(H, Kk, S, P) * R.out_size(W, Kk, S, P), Kk * Kk * C
    ref = R.im2col_f32_nhwc(x, Kk, Kk, S, P)
    if geom == (1, 3, 3, 2, 3, 1, 3):                 # windows wholly in the border: whole rows of zeros
        assert np.sum(~ref.any(axis=1)) == 7 * 7 - 5 * 5   # the outer ring of the 7 x 7 windows
    what = f"im2col_f32_pad {gid(geom)}"
    got = launch_twice(what, M * K, K, lambda o: call("ia_im2col_f32_nhwc_pad", L.ptr(xd), B, H, W, C, Kk, Kk, S, P, L.ptr(o), L.stream()))
    assert_bits(what, got, ref)


# ------------------------------------------------------------------------------------------------------------------
# c. ia_col2im_nhwc, ia_col2im_nhwc_pad
# ------------------------------------------------------------------------------------------------------------------
def takes_v4(C, *tensors):
    """The dispatch of `ia_col2im_nhwc`, restated: four channels per thread with 16-byte accesses, when every pointer allows."""
    return C % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def col2im(geom, masked, shift_dx=0, shift_dcol=0, shift_mask=0):
    """One unpadded case: NaN-prefilled dx (so uncovered pixels must be WRITTEN as 0), bit-exact against the ordered float32
    reference. Returns (dx, whether the vector kernel ran)."""
    B, H, W, C, KH, KW, S = geom
    M, K = B * R.out_size(H, KH, S) * R.out_size(W, KW, S), KH * KW * C
    dcol = randn32(M, K, seed=2)
    mask = relu_like(B, H, W, C, seed=5) if masked else None
    dd, md = dev(dcol, shift_dcol), (dev(mask, shift_mask) if masked else None)
    what = f"col2im {gid(geom)} mask={masked} shifts={shift_dx, shift_dcol, shift_mask}"
    v4 = []

    def launch(o):
        v4.append(takes_v4(C, dd, md, o))
        return call("ia_col2im_nhwc", L.ptr(dd), B, H, W, C, KH, KW, S, L.ptr(md), L.ptr(o), L.stream())

    got = launch_twice(what, B * H * W * C, W * C, launch, shift=shift_dx)
    ref = R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S, 0, mask)
    assert_bits(what, got, ref)
    if geom in R.COL2IM_GAP_GEOMS:                    # pixels that no window covers, written as exact zeros
        covered = R.col2im_nhwc(np.ones_like(dcol), B, H, W, C, KH, KW, S) > 0
        assert not covered.all() and np.all(got.cpu().numpy().reshape(B, H, W, C)[~covered] == 0.0), what
    assert v4[0] == v4[1]
    return got, v4[0]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("geom", R.F32_GEOMS + R.COL2IM_GAP_GEOMS, ids=gid)
def test_col2im(geom, masked):
    """C in {4, 8, 32, 64} with aligned buffers: the four-channel vector kernel; C in {3, 5}: the scalar kernel."""
    C = geom[3]
    assert C in (3, 4, 5, 8, 32, 64)
    _, v4 = col2im(geom, masked)
    assert v4 == (C in (4, 8, 32, 64))


def test_col2im_both_kernels_agree_bit_for_bit():
    """A C % 4 == 0 geometry with dx, then dcol, then the mask one float (4 bytes) into its allocation takes the scalar
    kernel: each time the same bits as the aligned call through the vector kernel."""
    geom = R.F32_GEOMS[0]
    a, v4 = col2im(geom, True)
    assert v4
    for shifts in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        b, v4 = col2im(geom, True, *shifts)
        assert not v4, shifts
        assert bits_equal(a, b), shifts
    a, v4 = col2im(geom, False)                       # and without a mask: a NULL mask counts as aligned
    b, v4_b = col2im(geom, False, shift_dcol=1)
    assert v4 and not v4_b and bits_equal(a, b)


@pytest.mark.parametrize("geom", [g + (0,) for g in R.F32_GEOMS if g[4] == g[5]] + [(B, H, W, C, K, K, S, P) for B, H, W, C, K, S, P in
                                                                                   R.F32_PAD_GEOMS], ids=gid)
def test_col2im_pad(geom):
    """The padded entry (one scalar kernel), at every padded geometry and at P = 0 at the unpadded ones."""
    B, H, W, C, KH, KW, S, P = geom
    M, K = B * R.out_size(H, KH, S, P) * R.out_size(W, KW, S, P), KH * KW * C
    dcol = randn32(M, K, seed=2)
    dd = dev(dcol)
    what = f"col2im_pad {gid(geom)}"
    got = launch_twice(what, B * H * W * C, W * C, lambda o: call("ia_col2im_nhwc_pad", L.ptr(dd), B, H, W, C, KH, KW, S, P, L.ptr(o),
                                                                 L.stream()))
    assert_bits(what, got, R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S, P))


@pytest.mark.parametrize("geom", [g for g in R.F32_GEOMS if g[4] != g[5]] + R.COL2IM_GAP_GEOMS, ids=gid)
def test_col2im_pad_entry_without_padding(geom):
    """The remaining unpadded geometries (KH != KW, gaps, uncovered tails) through the padded entry at P = 0."""
    B, H, W, C, KH, KW, S = geom
    M, K = B * R.out_size(H, KH, S) * R.out_size(W, KW, S), KH * KW * C
    dcol = randn32(M, K, seed=2)
    dd = dev(dcol)
    what = f"col2im_pad P=0 {gid(geom)}"
    got = launch_twice(what, B * H * W * C, W * C, lambda o: call("ia_col2im_nhwc_pad", L.ptr(dd), B, H, W, C, KH, KW, S, 0, L.ptr(o),
                                                                 L.stream()))
    assert_bits(what, got, R.col2im_nhwc(dcol, B, H, W, C, KH, KW, S))


# ------------------------------------------------------------------------------------------------------------------
# d. ia_avgpool_nhwc
# ------------------------------------------------------------------------------------------------------------------
def avgpool(y):
    B, HW, C = y.shape
    yd = dev(y)
    return launch_twice(f"avgpool {B}x{HW}x{C}", B * C, C, lambda o: call("ia_avgpool_nhwc", L.ptr(yd), B, HW, C, L.ptr(o), L.stream()))


@pytest.mark.parametrize("B", R.AVGPOOL_BATCHES)
@pytest.mark.parametrize("HW,C", R.AVGPOOL_SHAPES, ids=lambda v: str(v))
def test_avgpool_matches_the_float64_mean(HW, C, B):
    """C % 4 == 0 and C <= 1024: the channel-quad kernel (G = 256 // (C/4) position groups); otherwise a thread per channel.
    |got - mean64| <= (n + 2) 2^-24 mean_p |y|: a float32 sum whose longest chain has n additions is within n 2^-24 sum |y|
    of the exact sum (to first order), the quotient rounds once more; the + 2 covers both that and the higher-order terms.
    With y = 1 + 0.5 randn a dropped or doubled position moves the mean by ~1 / HW, at every shape here more than 25 times
    the bound (HW = 7056, C = 32: 1.4e-4 against 5.5e-6)."""
    quad = C % 4 == 0 and C // 4 <= 256
    n = (-(-HW // (4 * (256 // (C // 4)))) + 3 + 256 // (C // 4)) if quad else HW
    assert n == R.avgpool_chain(HW, C)
    y = (1 + 0.5 * np.random.default_rng(HW * 10007 + C + B).standard_normal((B, HW, C))).astype(np.float32)
    got = avgpool(y).cpu().numpy().reshape(B, C).astype(np.float64)
    assert np.all(np.isfinite(got))
    ref = R.avgpool_float64(y)
    bound = (n + 2) * EPS * np.abs(y.astype(np.float64)).mean(axis=1)
    err = np.abs(got - ref)
    print(f"avgpool B={B} HW={HW} C={C} quad={quad} n={n}: max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"HW={HW} C={C}: {np.max(err / bound):.3f} x the bound"


@pytest.mark.parametrize("HW,C", [(64, 32), (1024, 4), (8, 6)], ids=lambda v: str(v))
def test_avgpool_of_a_constant_is_that_constant(HW, C):
    """y constant per channel over HW = 2^k positions. The constants are multiples of 1/8 below 16 (7 significant bits),
    so every partial sum m * c, m <= HW <= 2^10, is a float32 (17 bits at most) whatever the order: no addition rounds, and
    the quotient by 2^k is exact. Quad kernel at G = 32 and G = 256, and the thread-per-channel kernel."""
    assert HW & (HW - 1) == 0
    B = 2
    c = (np.random.default_rng(C).integers(-127, 128, size=(B, 1, C)) / 8).astype(np.float32)
    c[0, 0, 0] = 15.875
    y = np.ascontiguousarray(np.broadcast_to(c, (B, HW, C)))
    assert_bits(f"avgpool const {HW}x{C}", avgpool(y), c.reshape(B, C))


# ------------------------------------------------------------------------------------------------------------------
# e. ia_avgpool_nhwc_backward, ia_relu_backward, ia_avgpool_relu_backward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.BACKWARD_C)
@pytest.mark.parametrize("HW", R.BACKWARD_HW)
def test_pool_and_relu_backward(HW, C):
    B = 3
    dout, y = randn32(B, C, seed=HW + C), relu_like(B, HW, C, seed=HW * C)
    n = B * HW * C
    dd, yd = dev(dout), dev(y)
    what = f"HW={HW} C={C}"
    dy_ref = R.avgpool_backward(dout, HW)
    dy = launch_twice("avgpool_backward " + what, n, C, lambda o: call("ia_avgpool_nhwc_backward", L.ptr(dd), B, HW, C, L.ptr(o), L.stream()))
    assert_bits("avgpool_backward " + what, dy, dy_ref)
    dz_ref = R.relu_backward(dy_ref, y)
    dyd = dev(dy_ref)
    dz = launch_twice("relu_backward " + what, n, C, lambda o: call("ia_relu_backward", L.ptr(dyd), L.ptr(yd), n, L.ptr(o), L.stream()))
    assert_bits("relu_backward " + what, dz, dz_ref)
    if C % 4 == 0:
        fused = launch_twice("avgpool_relu_backward " + what, n, C,
                             lambda o: call("ia_avgpool_relu_backward", L.ptr(dd), L.ptr(yd), B, HW, C, L.ptr(o), L.stream()))
        assert_bits("avgpool_relu_backward " + what, fused, dz_ref)
    else:                                             # the fused kernel owns channel quads: unsupported, nothing written
        out = launch_twice("avgpool_relu_backward " + what, n, C,
                           lambda o: call("ia_avgpool_relu_backward", L.ptr(dd), L.ptr(yd), B, HW, C, L.ptr(o), L.stream()),
                           rc=L.ERR_UNSUPPORTED)
        assert bool(th.isnan(out).all()), "a rejected call wrote its output"


@pytest.mark.parametrize("n", [1, 257])
def test_relu_backward_small_and_in_place(n):
    """One element, one element past a block, and the in-place form `out == dy` that `ops.py` uses."""
    dy = randn32(n, seed=n)
    dyd = dev(dy)
    ys = [relu_like(320, seed=n + 1)[:n]] if n > 1 else [np.array([v], dtype=np.float32) for v in (-0.0, 0.0, 2.0, -1.0)]
    for yy in ys:
        yd = dev(yy)
        ref = R.relu_backward(dy, yy)
        got = launch_twice(f"relu_backward n={n}", n, n, lambda o: call("ia_relu_backward", L.ptr(dyd), L.ptr(yd), n, L.ptr(o), L.stream()))
        assert_bits(f"relu_backward n={n}", got, ref)

        def in_place(o):
            o.copy_(dyd)
            return call("ia_relu_backward", L.ptr(o), L.ptr(yd), n, L.ptr(o), L.stream())

        assert_bits(f"relu_backward in place n={n}", launch_twice(f"relu_backward in place n={n}", n, n, in_place), ref)


BIG = 2 ** 26 + 257   # threads of the largest grid (262 144 blocks of 256) + 257: the grid-stride loops take a second trip


def test_relu_backward_grid_stride_second_trip():
    """An element per thread: BIG elements. Expectation and comparison on the device."""
    g = th.Generator(device=DEV).manual_seed(1)
    dy, y = th.randn(BIG, device=DEV, generator=g), th.randn(BIG, device=DEV, generator=g)
    y[::5] = 0.0
    y[1::7] = -0.0
    want = th.where(y > 0, dy, th.zeros((), device=DEV))
    got = launch_twice("relu_backward BIG", BIG, 64, lambda o: call("ia_relu_backward", L.ptr(dy), L.ptr(y), BIG, L.ptr(o), L.stream()))
    assert bool(th.isfinite(got).all()) and th.equal(got, want)
    assert not th.equal(got[-257:], th.zeros(257, device=DEV))   # the second trip's elements are not all masked
    del dy, y, want, got
    _KEEP.clear()
    th.cuda.empty_cache()


def test_avgpool_relu_backward_grid_stride_second_trip():
    """A channel QUAD per thread, so the second trip needs BIG quads: B = 3 images of HW = 22 369 707 positions of C = 4
    channels (3 * 22 369 707 = BIG), 1 GiB per buffer. The quotient dout / float(HW) is the reference's single IEEE
    division, computed on the host for the 12 values of dout (torch's division by a scalar multiplies by its reciprocal);
    the broadcast, the mask and the comparison run on the device."""
    B, HW, C = 3, 22369707, 4
    assert B * HW == BIG
    g = th.Generator(device=DEV).manual_seed(2)
    y = th.randn(B, HW, C, device=DEV, generator=g)
    y.view(-1)[::5] = 0.0
    y.view(-1)[1::7] = -0.0
    dout = randn32(B, C, seed=9)
    dd = dev(dout)
    quot = th.from_numpy(dout / np.float32(HW)).to(DEV)
    want = th.where(y > 0, quot[:, None, :], th.zeros((), device=DEV))
    got = launch_twice("avgpool_relu_backward BIG", B * HW * C, 64,
                       lambda o: call("ia_avgpool_relu_backward", L.ptr(dd), L.ptr(y), B, HW, C, L.ptr(o), L.stream()))
    assert bool(th.isfinite(got).all()) and th.equal(got.view(B, HW, C), want)
    assert bool((got[-4 * 257:] != 0).any())                     # the second trip's quads are not all masked
    del y, want, got
    _KEEP.clear()
    th.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------
# f. ia_categorical_loss
# ------------------------------------------------------------------------------------------------------------------
def categorical(logits, act, ldl, c_lp, c_ent, want_grad=True):
    """One row per lane in blocks of 128. logits[B, A] are laid out with row stride `ldl`, the padding columns NaN; the
    padding columns of dlogits must stay NaN. Returns (logp, entropy, dlogits[B, A] or None) as numpy arrays."""
    B, A = logits.shape
    padded = np.full((B, ldl), np.nan, dtype=np.float32)
    padded[:, :A] = logits
    ld, ad = dev(padded), dev(act)
    what = f"categorical B={B} A={A} ldl={ldl} c=({c_lp:.3g}, {c_ent:.3g}) grad={want_grad}"
    outs = []
    for _ in range(2):
        lp, en, dl = Guarded(B, B), Guarded(B, B), Guarded(B * ldl, ldl)
        rc = call("ia_categorical_loss", L.ptr(ld), ldl, L.ptr(ad), B, A, c_lp, c_ent, L.ptr(lp.body), L.ptr(en.body),
                  L.ptr(dl.body) if want_grad else None, L.stream())
        th.cuda.synchronize()
        assert rc == 0, what
        assert lp.guard_intact() and en.guard_intact() and dl.guard_intact(), f"{what}: wrote outside its outputs"
        outs.append((lp.body, en.body, dl.body))
    assert all(bits_equal(a, b) for a, b in zip(*outs)), f"{what}: two launches differ"
    lp, en, dl = (t.cpu().numpy() for t in outs[0])
    dl = dl.reshape(B, ldl)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(en)), f"{what}: inf or nan"
    if not want_grad:
        return lp, en, None
    assert np.all(np.isfinite(dl[:, :A])), f"{what}: inf or nan in dlogits"
    assert np.all(np.isnan(dl[:, A:])), f"{what}: padding columns of dlogits written"
    return lp, en, dl[:, :A]


_cat_worst = {}


@pytest.mark.parametrize("A", R.CAT_A)
@pytest.mark.parametrize("B", R.CAT_B)
def test_categorical_loss_matches_float64(B, A):
    for scale in R.CAT_SCALES:                        # 40 * randn: the maximum must be subtracted before expf
        logits, act = R.cat_inputs(B, A, scale)
        for ldl in (A, A + 3):
            for c_lp, c_ent in R.cat_coefs(B):
                ref = R.categorical_float64(logits, act, c_lp, c_ent)
                got = categorical(logits, act, ldl, c_lp, c_ent)
                if A == 1:                            # one action: logp = 0, H = 0, no gradient -- exactly
                    assert all(np.all(g == 0.0) for g in got)
                    continue
                unit = max(abs(c_lp), abs(c_ent))
                for name, g, r, u in zip(("logp", "entropy", "dlogits"), got, ref, (1.0, 1.0, unit)):
                    err = R.cat_error(g, r, u)
                    _cat_worst[name, scale] = max(_cat_worst.get((name, scale), 0.0), err)
                    # Error as |got - float64| / (unit + |float64|), the largest over every case of this test, logits
                    # randn | 40 randn:
                    #   torch-CPU float32 Categorical + autograd   logp 1.28e-7 | 3.41e-6   entropy 1.70e-7 | 3.78e-6   dlogits 2.13e-7 | 3.72e-6
                    #   this kernel on the MI355X                  logp 1.68e-7 | 3.41e-6   entropy 2.43e-7 | 3.77e-6   dlogits 3.36e-7 | 3.41e-6
                    #   bound = 4 x torch's (CAT_BOUND, <= 2e-5)   logp 5.12e-7 | 1.36e-5   entropy 6.80e-7 | 1.51e-5   dlogits 8.52e-7 | 1.49e-5
                    assert err <= R.CAT_BOUND[name, scale], f"{name} B={B} A={A} scale={scale} ldl={ldl}: {err:.3e} > {R.CAT_BOUND[name, scale]:.3e}"
        # without a gradient buffer the other two outputs are the same bits
        c_lp, c_ent = R.cat_coefs(B)[0]
        with_grad = categorical(logits, act, A + 3, c_lp, c_ent)
        lp, en, _ = categorical(logits, act, A + 3, c_lp, c_ent, want_grad=False)
        assert np.array_equal(lp.view(np.int32), with_grad[0].view(np.int32)) and np.array_equal(en.view(np.int32), with_grad[1].view(np.int32))
    print("categorical worst errors so far:", {k: f"{v:.3e}" for k, v in sorted(_cat_worst.items())})
