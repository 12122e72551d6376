"""Kernel-level parity (`-m gpu`) of the implicit first-layer convolution, `ia_conv1_u8_forward`, `ia_conv1_u8_wgrad`,
`ia_conv1_u8_wgrad_ws_floats` and `ia_conv1_u8_implicit_ok` (csrc/conv1_implicit.hip), against the reference of
`tests/conv1_ref.py` (itself checked on the CPU by `tests/test_conv1_ref.py`).

Exact cases: with `scale = 1` and integer weights, bias and dout in [-2, 2] every partial sum is an integer below 2^24, so
float32 MFMA accumulation is exact in any order and the forward, dW and db must equal the int64 reference bit for bit -- at
every frame shape (each chosen for one path of the kernels, `conv1_ref.SHAPES`), at B = 1, 2, 3, 7 and at batch sizes
derived from the device's CU count at which the persistent grids loop (where the weight gradient's accumulators carry
across a workgroup's images). Float cases: seeded normals against the float64 reference at the project's tolerances for fp32
MFMA accumulation (rtol 2e-5, atol 2e-5 sqrt(256) forward; 3e-5 and sqrt(rows) for dW and db); the worst error over tolerance
is printed per case.

Every output and workspace is filled with NaN before the launch, with guard floats behind it: each element the operation
defines must come back finite, the guards must still be NaN. Each case is launched twice and the two results must be
bit-equal. The refusal tests launch nothing."""
import functools

import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from tests import conv1_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
FWD_WS = 128 * 64                      # the forward's workspace: the weight fragments
PER_WG = 32 * 256 + 32                 # the weight gradient's workspace per workgroup: one dW and one db partial
GUARD = 64


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


def dev(x):
    """Uploads `x` in its own type (uint8 frames, float32 everything else); the tensor stays alive until the test ends
    (raw pointers carry no ownership)."""
    t = th.tensor(np.ascontiguousarray(x)).to(DEV).contiguous()
    assert t.dtype in (th.uint8, th.float32) and t.data_ptr() % 16 == 0
    _KEEP.append(t)
    return t


def nans(n):
    t = th.full((int(n),), NAN, device=DEV)
    _KEEP.append(t)
    return t


def bits_equal(a, b):
    return th.equal(a.view(th.int32), b.view(th.int32))


def gid(s):
    return "x".join(map(str, s))


def cus():
    return th.cuda.get_device_properties(0).multi_processor_count


def ws_floats(B):
    return int(L.load().ia_conv1_u8_wgrad_ws_floats(B))


def run_forward(dx, B, H, W, dW, dbias, scale):
    """One forward launch into NaN-filled buffers -> out[rows, 32] (a view); the workspace's defined part must be finite,
    the guards behind the workspace and behind `out` still NaN."""
    rows = B * R.npix(H, W)
    ws, out = nans(FWD_WS + GUARD), nans(rows * 32 + 32)
    L.call("ia_conv1_u8_forward", L.ptr(dx), B, H, W, L.ptr(dW), L.ptr(dbias), scale, L.ptr(ws), L.ptr(out), L.stream())
    th.cuda.synchronize()
    assert bool(th.isfinite(ws[:FWD_WS]).all()), "forward workspace not fully written"
    assert bool(th.isnan(ws[FWD_WS:]).all()), "written behind the forward workspace"
    assert bool(th.isnan(out[rows * 32:]).all()), "written behind the forward output"
    return out[:rows * 32].view(rows, 32)


def run_wgrad(dx, B, H, W, ddout, scale, accumulate=0, dW=None, db=None):
    """One weight-gradient launch -> (dW[32, 256], db[32]) (views); NaN-filled buffers unless `dW` / `db` (8192 + 32 and
    32 + 32 floats, guards NaN) are given; the workspace's defined part must be finite, every guard still NaN."""
    n = ws_floats(B)
    assert n == min(B, 2 * cus()) * PER_WG
    ws = nans(n + GUARD)
    dW = nans(32 * 256 + 32) if dW is None else dW
    db = nans(32 + 32) if db is None else db
    L.call("ia_conv1_u8_wgrad", L.ptr(dx), B, H, W, L.ptr(ddout), scale, L.ptr(ws), accumulate, L.ptr(dW), L.ptr(db),
           L.stream())
    th.cuda.synchronize()
    assert bool(th.isfinite(ws[:n]).all()), "weight-gradient workspace not fully written"
    assert bool(th.isnan(ws[n:]).all()), "written behind the weight-gradient workspace"
    assert bool(th.isnan(dW[32 * 256:]).all()) and bool(th.isnan(db[32:]).all()), "written behind dW or db"
    return dW[:32 * 256].view(32, 256), db[:32]


def batches_of(shape):
    """(forward batch sizes, weight-gradient batch sizes) of a frame shape: the looped ones at the two smallest frames."""
    fwd, wg = R.looped_batches(cus()) if shape in R.LOOP_SHAPES else ((), ())
    return R.BATCHES + fwd, R.BATCHES + wg


def test_looped_batch_sizes_do_loop():
    """The sizes the cases below call looped exceed the grids of this device (2 * CUs workgroups; the forward takes two
    images per workgroup), and the workspace size says so."""
    n = cus()
    fwd, wg = R.looped_batches(n)
    print(f"cus = {n}: forward B = {fwd}, weight gradient B = {wg}")
    assert all((B + 1) // 2 > 2 * n for B in fwd) and all(B > 2 * n for B in wg)
    for B in (1, 2, 2 * n - 1, 2 * n, 2 * n + 1) + fwd + wg:
        assert ws_floats(B) == min(B, 2 * n) * PER_WG, B
    assert ws_floats(0) == 0


# ------------------------------------------------------------------------------------------------------------------
# a. exact cases: integers, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=gid)
def test_exact_integer_cases(shape):
    H, W = shape
    fwd_B, wg_B = batches_of(shape)
    for B in sorted(set(fwd_B + wg_B)):
        what = f"{gid(shape)} B={B}"
        assert R.int_bound(B, H, W) < 2 ** 24, what                  # every partial sum is an exact float32
        x, Wt, bias, dout = R.int_inputs(B, H, W)
        col = R.columns_int(x)
        dx = dev(x)
        if B in fwd_B:
            ref = R.forward_int(x, Wt, bias, col=col)
            dWt, dbias = dev(Wt), dev(bias)
            outs = [run_forward(dx, B, H, W, dWt, dbias, 1.0) for _ in range(2)]
            got = outs[0].cpu().numpy()
            assert np.all(np.isfinite(got)), f"{what}: {np.sum(~np.isfinite(got))} forward outputs not finite"
            bad = np.argwhere(got != ref)
            assert bad.size == 0, f"{what}: {len(bad)} forward outputs differ, first at (row, channel) {bad[0]}"
            assert ref.max() > 0 and np.mean(ref == 0) > 0.1, what   # both sides of the ReLU are there
            assert bits_equal(outs[0], outs[1]), f"{what}: two forward launches differ"
        if B in wg_B:
            rW, rb = R.wgrad_int(x, dout, col=col)
            ddout = dev(dout)
            outs = [run_wgrad(dx, B, H, W, ddout, 1.0) for _ in range(2)]
            gW, gb = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
            assert np.all(np.isfinite(gW)) and np.all(np.isfinite(gb)), f"{what}: gradient not finite"
            bad = np.argwhere(gW != rW)
            assert bad.size == 0, f"{what}: {len(bad)} elements of dW differ, first at (channel, column) {bad[0]}"
            assert np.array_equal(gb, rb), f"{what}: db differs"
            assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1]), f"{what}: two launches differ"
        print(f"{what}: exact (largest possible partial sum {R.int_bound(B, H, W)})")


# ------------------------------------------------------------------------------------------------------------------
# b. float cases against float64
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_case(B, H, W, scale):
    """Inputs and float64 references of one float case, computed once and shared (nobody writes to them)."""
    x, Wt, bias, dout = R.float_inputs(B, H, W)
    col = R.columns(x, scale)
    arrays = (x, Wt, bias, dout, R.forward(x, Wt, bias, scale, col=col)) + R.wgrad(x, dout, scale, col=col)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def check_forward(got, ref, what):
    got = got.cpu().numpy()
    assert np.all(np.isfinite(got)), f"{what}: {np.sum(~np.isfinite(got))} forward outputs not finite"
    ratio = R.tol_ratio(got, ref, R.FWD_RTOL, R.fwd_atol())
    print(f"{what}: forward max abs err {np.abs(got - ref).max():.3e} (atol {R.fwd_atol():.3e}), {ratio:.4f} x tolerance")
    np.testing.assert_allclose(got, ref, rtol=R.FWD_RTOL, atol=R.fwd_atol(), err_msg=what)
    return ratio


def check_wgrad(gW, gb, rW, rb, rows, what):
    gW, gb = gW.cpu().numpy(), gb.cpu().numpy()
    assert np.all(np.isfinite(gW)) and np.all(np.isfinite(gb)), f"{what}: gradient not finite"
    atol = R.wgrad_atol(rows)
    ratio = max(R.tol_ratio(gW, rW, R.WGRAD_RTOL, atol), R.tol_ratio(gb, rb, R.WGRAD_RTOL, atol))
    print(f"{what}: dW max abs err {np.abs(gW - rW).max():.3e}, db {np.abs(gb - rb).max():.3e} (atol {atol:.3e}), "
          f"{ratio:.4f} x tolerance")
    np.testing.assert_allclose(gW, rW, rtol=R.WGRAD_RTOL, atol=atol, err_msg=what + " dW")
    np.testing.assert_allclose(gb, rb, rtol=R.WGRAD_RTOL, atol=atol, err_msg=what + " db")
    return ratio


@pytest.mark.parametrize("scale", R.SCALES, ids=["scale1/255", "scale1/128"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=gid)
def test_float_cases(shape, scale):
    H, W = shape
    fwd_loop, wg_loop = R.looped_batches(cus()) if shape in R.LOOP_SHAPES else ((), ())
    worst_f = worst_w = 0.0
    for B in sorted(set((3,) + fwd_loop + wg_loop)):
        what = f"{gid(shape)} B={B} scale={scale:.4g}"
        rows = B * R.npix(H, W)
        x, Wt, bias, dout, ref, rW, rb = float_case(B, H, W, scale)
        dx = dev(x)
        if B == 3 or B in fwd_loop:
            dWt, dbias = dev(Wt), dev(bias)
            outs = [run_forward(dx, B, H, W, dWt, dbias, scale) for _ in range(2)]
            worst_f = max(worst_f, check_forward(outs[0], ref, what))
            assert bits_equal(outs[0], outs[1]), f"{what}: two forward launches differ"
        if B == 3 or B in wg_loop:
            ddout = dev(dout)
            outs = [run_wgrad(dx, B, H, W, ddout, scale) for _ in range(2)]
            worst_w = max(worst_w, check_wgrad(*outs[0], rW, rb, rows, what))
            assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1]), f"{what}: two launches differ"
    print(f"WORST {gid(shape)} scale={scale:.4g}: forward {worst_f:.4f}, weight gradient {worst_w:.4f} x tolerance")


# ------------------------------------------------------------------------------------------------------------------
# c. the contract around the arithmetic
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 44, 36), (7, 8, 12), ("looped", 12, 20)], ids=gid)
def test_accumulate_adds_the_same_total_once(case):
    """`accumulate = 0` overwrites NaN-filled dW / db (finite and in tolerance); `accumulate = 1` over seeded dW0 / db0 gives
    float32(dW0 + the accumulate = 0 result) bit for bit: the reduction adds the same total with one float32 addition."""
    B, H, W = case
    if B == "looped":
        B = R.looped_batches(cus())[1][0]
    scale = R.SCALES[0]
    what = f"accumulate {B}x{H}x{W}"
    x, _, _, dout, _, rW, rb = float_case(B, H, W, scale)
    dx, ddout = dev(x), dev(dout)
    gW, gb = run_wgrad(dx, B, H, W, ddout, scale, accumulate=0)
    check_wgrad(gW, gb, rW, rb, B * R.npix(H, W), what)
    rng = np.random.default_rng(11)
    W0, b0 = rng.standard_normal((32, 256)).astype(np.float32), rng.standard_normal(32).astype(np.float32)
    bufW, bufb = nans(32 * 256 + 32), nans(32 + 32)
    bufW[:32 * 256] = dev(W0).reshape(-1)
    bufb[:32] = dev(b0)
    aW, ab = run_wgrad(dx, B, H, W, ddout, scale, accumulate=1, dW=bufW, db=bufb)
    wantW, wantb = W0 + gW.cpu().numpy(), b0 + gb.cpu().numpy()              # float32 + float32: one rounding
    assert wantW.dtype == np.float32 and wantb.dtype == np.float32
    assert np.array_equal(aW.cpu().numpy().view(np.int32), wantW.view(np.int32)), f"{what}: dW"
    assert np.array_equal(ab.cpu().numpy().view(np.int32), wantb.view(np.int32)), f"{what}: db"


# ------------------------------------------------------------------------------------------------------------------
# d. predicate and refusals: nothing is launched
# ------------------------------------------------------------------------------------------------------------------
def test_predicate_equals_the_documented_table():
    ok = L.load().ia_conv1_u8_implicit_ok
    got = np.array([[bool(ok(4, H, W, 8, 8, 4, 32)) for W in R.SCAN] for H in R.SCAN])
    want = R.ok_table()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} shapes differ, first (H, W) = {bad[0] + 8}: library says {got[tuple(bad[0])]}"
    assert ok(4, 84, 84, 8, 8, 4, 32) == 1
    for args in [(3, 84, 84, 8, 8, 4, 32), (4, 84, 84, 4, 8, 4, 32), (4, 84, 84, 8, 8, 2, 32), (4, 84, 84, 8, 8, 4, 64)]:
        assert ok(*args) == 0 and not R.shape_ok(*args), args


def test_entries_refuse_what_the_predicate_rejects():
    """Each violated precondition returns IA_ERR_ARG (-1) before anything is launched: NaN-filled outputs and workspaces
    keep their fill. The buffers are large enough for every variant, should one of them be launched after all."""
    assert L.ERR_ARG == -1
    rejected_H = min(H for H in R.SCAN if not R.shape_ok(4, H, 84, 8, 8, 4, 32))
    assert rejected_H == 88 and R.shape_ok(4, rejected_H - 1, 84, 8, 8, 4, 32)
    B = 2
    xbuf = dev(R.frames(4, 128, 128, seed=5).reshape(-1))                   # 256 KiB of frame bytes
    rng = np.random.default_rng(6)
    Wt, bias = dev(rng.standard_normal((32, 256)).astype(np.float32)), dev(rng.standard_normal(32).astype(np.float32))
    dout = dev(rng.standard_normal(B * 32 * 32 * 32 + 4).astype(np.float32))
    out, ws_f = nans(B * 32 * 32 * 32), nans(FWD_WS)
    ws_w, dW, db = nans(4 * PER_WG), nans(32 * 256), nans(32)

    def refused(what, B, H, W, x_off=0, dout_off=0):
        with pytest.raises(RuntimeError, match=r"code -1$"):
            L.call("ia_conv1_u8_forward", xbuf.data_ptr() + x_off, B, H, W, L.ptr(Wt), L.ptr(bias), 1.0 / 255.0, L.ptr(ws_f),
                   L.ptr(out), L.stream())
        with pytest.raises(RuntimeError, match=r"code -1$"):
            L.call("ia_conv1_u8_wgrad", xbuf.data_ptr() + x_off, B, H, W, dout.data_ptr() + dout_off, 1.0 / 255.0,
                   L.ptr(ws_w), 0, L.ptr(dW), L.ptr(db), L.stream())
        th.cuda.synchronize()
        for name, t in (("out", out), ("forward workspace", ws_f), ("gradient workspace", ws_w), ("dW", dW), ("db", db)):
            assert bool(th.isnan(t).all()), f"{what}: {name} was written"

    refused("OW odd", B, 8, 16)
    refused("W % 4 != 0", B, 8, 10)
    refused("H < 8", B, 7, 12)
    refused("beyond the LDS budget", B, rejected_H, 84)
    refused("B = 0", 0, 84, 84)
    refused("frames 4 bytes off a 16-byte boundary", B, 84, 84, x_off=4)
    # an unaligned dout concerns the weight gradient alone
    with pytest.raises(RuntimeError, match=r"code -1$"):
        L.call("ia_conv1_u8_wgrad", L.ptr(xbuf), B, 84, 84, dout.data_ptr() + 4, 1.0 / 255.0, L.ptr(ws_w), 0, L.ptr(dW),
               L.ptr(db), L.stream())
    th.cuda.synchronize()
    assert bool(th.isnan(ws_w).all()) and bool(th.isnan(dW).all()) and bool(th.isnan(db).all()), "unaligned dout: written"
    # and the unchanged arguments are accepted (the refusals above are not an artefact of this test's harness)
    L.call("ia_conv1_u8_forward", L.ptr(xbuf), B, 84, 84, L.ptr(Wt), L.ptr(bias), 1.0 / 255.0, L.ptr(ws_f), L.ptr(out),
           L.stream())
    L.call("ia_conv1_u8_wgrad", L.ptr(xbuf), B, 84, 84, L.ptr(dout), 1.0 / 255.0, L.ptr(ws_w), 0, L.ptr(dW), L.ptr(db),
           L.stream())
    th.cuda.synchronize()
    n = B * 400 * 32
    assert bool(th.isfinite(out[:n]).all()) and bool(th.isnan(out[n:]).all()) and bool(th.isfinite(ws_f).all())
    assert bool(th.isfinite(dW).all()) and bool(th.isfinite(db).all())
    assert bool(th.isfinite(ws_w[:B * PER_WG]).all()) and bool(th.isnan(ws_w[B * PER_WG:]).all())
