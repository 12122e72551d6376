"""Kernel-level parity (`-m gpu`) of the GEMM's implicit-convolution forms, `ia_gemm_f32_im2col` and
`ia_gemm_f32_im2col_pad` (csrc/gemm.hip), against the float64 reference of `tests/gemm_view_ref.py` (itself checked on
the CPU by `tests/test_gemm_view_ref.py`).

Every output buffer -- `ldc` padding columns and slab storage included -- is filled with NaN before the launch: each
element the operation defines must come back finite and within tolerance, every other element must still be NaN.
Each case is launched twice and the two results must be bit-equal. Inputs are seeded unit normals, weights are
scaled by 1/sqrt(K). Tolerances are those of the float64 GEMM tests of `tests/test_kernels_gpu.py` (fp32 MFMA
accumulation): rtol 2e-5, atol 2e-5 sqrt(K) for NT with K = KH*KW*Cin; 3e-5 and sqrt(rows) for the TN slab and
`dbias` sums. Masked zeros, empty slabs, untouched sentinels and repeated launches are compared exactly."""
import ctypes as C
import math

import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from tests import gemm_view_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


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
    """Uploads `x` as fp32; the tensor stays alive until the test ends (raw pointers carry no ownership)."""
    t = th.as_tensor(np.ascontiguousarray(x)).to(DEV, th.float32).contiguous()
    _KEEP.append(t)
    return t


def rnd(*shape, seed, scale=1.0):
    """Seeded unit normals, rounded to fp32 (what the kernel sees), as a numpy array."""
    g = th.Generator().manual_seed(seed)
    return (th.randn(*shape, generator=g) * scale).numpy()


def nans(*shape):
    return th.full(shape, NAN, device=DEV)


def bits_equal(a, b):
    return th.equal(a.view(th.int32), b.view(th.int32))


def gid(g):
    return "x".join(map(str, g))


def launch(entry, mode, A, lda, Bm, ldb, Cbuf, ldc, M, N, K, bias, act, splits, db, H, W, Cin, KH, KW, S, P=0,
           cmap=None, mask=None):
    """One launch through the C ABI; `entry` = "im2col" (no padding argument) or "pad"."""
    if entry == "im2col":
        assert P == 0 and cmap is None and mask is None
        L.call("ia_gemm_f32_im2col", mode, L.ptr(A), lda, L.ptr(Bm), ldb, L.ptr(Cbuf), ldc, M, N, K, L.ptr(bias), act,
               splits, L.ptr(db), H, W, Cin, KH, KW, S, L.stream())
    else:
        cm = None if cmap is None else (C.c_int * 5)(*cmap)
        L.call("ia_gemm_f32_im2col_pad", mode, L.ptr(A), lda, L.ptr(Bm), ldb, L.ptr(Cbuf), ldc, M, N, K, L.ptr(bias), act,
               splits, L.ptr(db), H, W, Cin, KH, KW, S, P, cm, L.ptr(mask), L.stream())
    th.cuda.synchronize()


def check_defined(got, ref, K, rtol=2e-5, what=""):
    """got[..., :n] (n = ref's last extent) finite and close to ref; the `ld` padding behind it still NaN."""
    got = got.cpu().numpy()
    n = ref.shape[-1]
    body, padding = got[..., :n], got[..., n:]
    assert np.all(np.isfinite(body)), f"{what}: {np.sum(~np.isfinite(body))} defined elements not finite"
    err = np.abs(body - ref)
    print(f"{what}: max abs err {err.max():.3e} (atol {rtol * math.sqrt(K):.3e})")
    np.testing.assert_allclose(body, ref, rtol=rtol, atol=rtol * math.sqrt(K), err_msg=what)
    assert np.all(np.isnan(padding)), f"{what}: ld padding overwritten"


# ------------------------------------------------------------------------------------------------------------------
# NT: C = act(view(x) . Wt^T + bias)
# ------------------------------------------------------------------------------------------------------------------
def _nt_case(entry, geom, masked=False):
    B, H, W, Cin, KH, KW, S, P, Cout = geom
    K = KH * KW * Cin
    M = B * R.out_size(H, KH, S, P) * R.out_size(W, KW, S, P)
    x, Wt, bias = rnd(B, H, W, Cin, seed=1), rnd(Cout, K, seed=2, scale=1 / math.sqrt(K)), rnd(Cout, seed=3)
    dx, dW, db = dev(x), dev(Wt), dev(bias)
    for act in (R.ACT_NONE, R.ACT_RELU):
        for b_np, b_dev in ((bias, db), (None, None)):
            ref = R.nt(x, Wt, b_np, act, KH, KW, S, P)
            for ldc in (Cout, Cout + 3):
                what = f"{entry} {gid(geom)} act={act} bias={b_np is not None} ldc={ldc}"
                mask_np = mask_dev = None
                want = ref
                if masked:   # laid out like C (same ld); about half the entries exact zeros
                    mask_np = np.maximum(rnd(M, ldc, seed=7), 0.0)
                    mask_dev = dev(mask_np)
                    want = np.where(mask_np[:, :Cout] > 0, ref, 0.0)
                outs = []
                for _ in range(2):
                    out = nans(M, ldc)
                    launch(entry, 0, dx, K, dW, K, out, ldc, M, Cout, K, b_dev, act, 1, None, H, W, Cin, KH, KW, S, P,
                           None, mask_dev)
                    outs.append(out)
                check_defined(outs[0], want, K, what=what)
                assert bits_equal(outs[0], outs[1]), f"{what}: two launches differ"
                if masked:
                    zeros = outs[0].cpu().numpy()[:, :Cout][mask_np[:, :Cout] <= 0]
                    assert zeros.size > M * Cout // 4 and np.all(zeros == 0.0), f"{what}: masked outputs not exactly 0"


@pytest.mark.parametrize("geom", R.NT_GEOMS, ids=gid)
def test_im2col_nt(geom):
    _nt_case("im2col", geom)


@pytest.mark.parametrize("geom", R.PAD_GEOMS, ids=gid)
def test_im2col_pad_nt(geom):
    _nt_case("pad", geom)


def test_im2col_pad_nt_with_relu_mask():
    _nt_case("pad", R.PAD_GEOMS[0], masked=True)


def test_im2col_pad_entry_without_padding_matches_plain_entry():
    """P = 0 through the padded entry is the same launch as the plain entry: the same bits."""
    B, H, W, Cin, KH, KW, S, P, Cout = geom = R.NT_GEOMS[1]
    K, M = KH * KW * Cin, B * R.out_size(H, KH, S, 0) * R.out_size(W, KW, S, 0)
    dx, dW = dev(rnd(B, H, W, Cin, seed=1)), dev(rnd(Cout, K, seed=2, scale=1 / math.sqrt(K)))
    a, b = nans(M, Cout), nans(M, Cout)
    launch("im2col", 0, dx, K, dW, K, a, Cout, M, Cout, K, None, 0, 1, None, H, W, Cin, KH, KW, S)
    launch("pad", 0, dx, K, dW, K, b, Cout, M, Cout, K, None, 0, 1, None, H, W, Cin, KH, KW, S, 0)
    assert bits_equal(a, b), gid(geom)


# ------------------------------------------------------------------------------------------------------------------
# TN: C_s = dout^T . view(x) per K split (+ dbias = column sums of dout)
# ------------------------------------------------------------------------------------------------------------------
TN_GEOMS = [(1, 20, 20, 32, 4, 4, 2, 0, 64), (5, 9, 9, 64, 3, 3, 1, 0, 64), (3, 5, 7, 32, 3, 3, 1, 1, 64),
            (130, 3, 4, 8, 3, 4, 1, 0, 64)]                                 # rows = 81, 245, 105, 130
assert all(g in R.NT_GEOMS + R.PAD_GEOMS for g in TN_GEOMS)


@pytest.mark.parametrize("geom", TN_GEOMS, ids=gid)
def test_im2col_tn_split_rows(geom):
    B, H, W, Cin, KH, KW, S, P, _ = geom
    N = KH * KW * Cin
    rows = B * R.out_size(H, KH, S, P) * R.out_size(W, KW, S, P)
    assert rows in (81, 245, 105, 130)
    chunks = (rows + 31) // 32                      # a non-empty slab holds at least one 32-row chunk of the reduction
    x = rnd(B, H, W, Cin, seed=1)
    dx = dev(x)
    entries = ("im2col", "pad") if P == 0 else ("pad",)
    for Cout in (20, 32, 64):
        dout = rnd(rows, Cout, seed=4)
        ddout = dev(dout)
        ref_w, ref_b = R.tn(dout, x, 1, KH, KW, S, P)
        for splits in (1, 3, chunks + 2):
            for want_db in (True, False):
                for entry in entries:
                    ldc = N + 3 if want_db else N
                    what = f"{entry} {gid(geom)} Cout={Cout} splits={splits} dbias={want_db}"
                    outs = []
                    for _ in range(2):
                        slabs = nans(splits, Cout, ldc)
                        db = nans(splits, Cout) if want_db else None
                        launch(entry, 2, ddout, Cout, dx, N, slabs, ldc, Cout, N, rows, None, 0, splits, db, H, W, Cin,
                               KH, KW, S, P)
                        outs.append((slabs, db))
                    slabs, db = outs[0]
                    got = slabs.cpu().numpy()
                    assert np.all(np.isfinite(got[..., :N])), f"{what}: slab elements not finite (empty slab left unwritten?)"
                    assert np.all(np.isnan(got[..., N:])), f"{what}: ld padding overwritten"
                    total = got[..., :N].astype(np.float64).sum(0)
                    print(f"{what}: max abs err {np.abs(total - ref_w).max():.3e} (atol {3e-5 * math.sqrt(rows):.3e})")
                    np.testing.assert_allclose(total, ref_w, rtol=3e-5, atol=3e-5 * math.sqrt(rows), err_msg=what)
                    if splits > chunks:
                        assert np.all(got[chunks:, :, :N] == 0.0), f"{what}: empty slabs not exactly zero"
                    assert bits_equal(slabs, outs[1][0]), f"{what}: two launches differ"
                    if want_db:
                        gdb = db.cpu().numpy()
                        assert np.all(np.isfinite(gdb)), f"{what}: dbias not finite"
                        np.testing.assert_allclose(gdb.astype(np.float64).sum(0), ref_b, rtol=3e-5,
                                                   atol=3e-5 * math.sqrt(rows), err_msg=what + " dbias")
                        if splits > chunks:
                            assert np.all(gdb[chunks:] == 0.0), f"{what}: dbias of empty slabs not exactly zero"
                        assert bits_equal(db, outs[1][1]), f"{what}: dbias of two launches differs"


# ------------------------------------------------------------------------------------------------------------------
# Scatter: the input gradient of a stride-S convolution, rows placed on the input grid by sub-pixel class
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("geom", R.SCATTER_GEOMS, ids=gid)
def test_im2col_pad_scatter(geom, B):
    k, S, h, w, Cin, Cout = geom
    kt = k // S
    OH, OW = R.out_size(h, k, S, 0), R.out_size(w, k, S, 0)
    gh, gw = OH + kt - 1, OW + kt - 1
    assert h >= S * gh and w >= S * gw              # no launch addresses a row outside its buffer
    Kd, M = kt * kt * Cout, B * gh * gw
    dout = rnd(B, OH, OW, Cout, seed=4)
    W_ = rnd(Cout, k, k, Cin, seed=2, scale=1 / math.sqrt(Kd))
    classes = [(py, px) for py in range(S) for px in range(S)]
    Wd = {c: R.dgrad_weights(W_, S, *c) for c in classes}
    Wd_all = np.concatenate([Wd[c] for c in classes])
    ddout, dWd_all = dev(dout), dev(Wd_all)
    dWd = {c: dev(Wd[c]) for c in classes}
    rows_all = R.nt(dout, Wd_all, None, R.ACT_NONE, kt, kt, 1, kt - 1)
    rows_cls = {c: rows_all[:, i * Cin:(i + 1) * Cin] for i, c in enumerate(classes)}

    def compare(got, want, what):
        """`want` [B, h, w, Cin] with NaN where nothing is written; `got` [B, h, w, ldc]."""
        got = got.cpu().numpy()
        body, padding = got[..., :Cin], got[..., Cin:]
        written = ~np.isnan(want)
        assert np.all(np.isfinite(body[written])), f"{what}: defined elements not finite"
        assert np.all(np.isnan(body[~written])), f"{what}: pixels of no class were written"
        assert np.all(np.isnan(padding)), f"{what}: ld padding overwritten"
        print(f"{what}: max abs err {np.abs(body[written] - want[written]).max():.3e} (atol {2e-5 * math.sqrt(Kd):.3e})")
        np.testing.assert_allclose(body[written], want[written], rtol=2e-5, atol=2e-5 * math.sqrt(Kd), err_msg=what)

    for with_mask in (False, True):
        # ---- form 2: every class in one launch (C has Cin columns)
        mask_np = np.maximum(rnd(B, h, w, Cin, seed=7), 0.0) if with_mask else None
        mask_dev = dev(mask_np) if with_mask else None
        what = f"form2 {gid(geom)} B={B} mask={with_mask}"
        cmap = (S, -1, -1, h, w)
        want = R.scatter(rows_all, cmap, (B, gh, gw), mask_np)
        outs = []
        for _ in range(2):
            out = nans(B, h, w, Cin)
            launch("pad", 0, ddout, Kd, dWd_all, Kd, out, Cin, M, S * S * Cin, Kd, None, 0, 1, None, OH, OW, Cout, kt, kt,
                   1, kt - 1, cmap, mask_dev)
            outs.append(out)
        compare(outs[0], want, what)
        assert bits_equal(outs[0], outs[1]), f"{what}: two launches differ"
        if with_mask:
            z = outs[0].cpu().numpy()[~np.isnan(want) & (mask_np <= 0)]
            assert z.size and np.all(z == 0.0), f"{what}: masked outputs not exactly 0"

        # ---- form 1: one launch per class into a re-filled buffer; every pixel written by exactly one launch
        ldc = Cin + 3
        mask1_np = np.maximum(rnd(B, h, w, ldc, seed=8), 0.0) if with_mask else None     # laid out like C: ld = ldc
        mask1_dev = dev(mask1_np) if with_mask else None
        union = np.full((B, h, w, ldc), np.nan, dtype=np.float32)
        hits = np.zeros((B, h, w), dtype=np.int64)
        want_union = np.full((B, h, w, Cin), np.nan)
        for c in classes:
            what = f"form1 {gid(geom)} B={B} class={c} mask={with_mask}"
            cmap = (S, c[0], c[1], h, w)
            want = R.scatter(rows_cls[c], cmap, (B, gh, gw), None if mask1_np is None else mask1_np[..., :Cin])
            outs = []
            for _ in range(2):
                out = nans(B, h, w, ldc)
                launch("pad", 0, ddout, Kd, dWd[c], Kd, out, ldc, M, Cin, Kd, None, 0, 1, None, OH, OW, Cout, kt, kt, 1,
                       kt - 1, cmap, mask1_dev)
                outs.append(out)
            compare(outs[0], want, what)
            assert bits_equal(outs[0], outs[1]), f"{what}: two launches differ"
            got = outs[0].cpu().numpy()
            new = ~np.isnan(got[..., :Cin]).all(-1)
            hits += new
            union[new] = got[new]
            want_union[~np.isnan(want)] = want[~np.isnan(want)]
        what = f"form1 {gid(geom)} B={B} union mask={with_mask}"
        inside = np.zeros((B, h, w), dtype=bool)
        inside[:, :S * gh, :S * gw] = True
        assert np.array_equal(hits, inside.astype(np.int64)), f"{what}: a pixel was written by {hits.max()} launches or by none"
        compare(th.from_numpy(union), want_union, what)
        if with_mask:
            z = union[..., :Cin][~np.isnan(want_union) & (mask1_np[..., :Cin] <= 0)]
            assert z.size and np.all(z == 0.0), f"{what}: masked outputs not exactly 0"


# ------------------------------------------------------------------------------------------------------------------
# Argument contract: IA_ERR_ARG and no launch
# ------------------------------------------------------------------------------------------------------------------
def test_im2col_argument_contract():
    """Each violated precondition returns IA_ERR_ARG (-1) before anything is launched: the outputs keep their NaN fill."""
    base = dict(B=2, H=16, W=16, Cin=8, KH=4, KW=4, S=2, P=0)
    Cout = 32
    # operands large enough for every variant below, should one of them be launched after all
    x, Wt, dout = dev(rnd(16384, seed=1)), dev(rnd(32768, seed=2)), dev(rnd(16384, seed=3))
    out, db = nans(65536), nans(1024)

    def rejected(what, entry, mode, cmap=None, rows_off=0, k_off=0, N_nt=Cout, **change):
        g = dict(base, **change)
        Kc = g["KH"] * g["KW"] * g["Cin"] + k_off
        rows = g["B"] * R.out_size(g["H"], g["KH"], g["S"], max(g["P"], 0)) * R.out_size(g["W"], g["KW"], g["S"], max(g["P"], 0))
        rows += rows_off
        geo = (g["H"], g["W"], g["Cin"], g["KH"], g["KW"], g["S"], g["P"])
        with pytest.raises(RuntimeError, match=r"code -1$"):
            if mode == 0:
                launch(entry, 0, x, Kc, Wt, Kc, out, N_nt, rows, N_nt, Kc, None, 0, 1, None, *geo, cmap, None)
            else:
                launch(entry, 2, dout, Cout, x, Kc, out, Kc, Cout, Kc, rows, None, 0, 2, db, *geo, cmap, None)
        th.cuda.synchronize()
        assert bool(th.isnan(out).all()) and bool(th.isnan(db).all()), f"{what}: something was launched"

    for entry in ("im2col", "pad"):
        for mode in (0, 2):
            tag = f"{entry} mode {mode}: "
            rejected(tag + "Cin % 4 != 0", entry, mode, Cin=6, KW=16)          # KW*Cin = 96 is a multiple of 32
            rejected(tag + "(KW*Cin) % 32 != 0", entry, mode, Cin=4)           # KW*Cin = 16
            rejected(tag + "rows % OHW != 0", entry, mode, rows_off=1)
            rejected(tag + "K != KH*KW*Cin", entry, mode, k_off=32)
    big = (64, 64)
    rejected("P < 0", "pad", 0, P=-1)
    rejected("P < 0 (TN)", "pad", 2, P=-1)
    rejected("cmap with mode TN", "pad", 2, cmap=(1, 0, 0, *big))
    rejected("cmap[0] == 0", "pad", 0, cmap=(0, 0, 0, *big))
    rejected("cmap[0] < 0", "pad", 0, cmap=(-2, 0, 0, *big))
    rejected("form 2 with N % S_out^2 != 0", "pad", 0, cmap=(2, -1, -1, *big), N_nt=30)
    # and the unchanged arguments are accepted (the rejections above are not an artefact of the harness of this test)
    for entry in ("im2col", "pad"):
        for mode in (0, 2):
            out.fill_(NAN)
            rows, Kc = 2 * 7 * 7, 128
            if mode == 0:
                launch(entry, 0, x, Kc, Wt, Kc, out, Cout, rows, Cout, Kc, None, 0, 1, None, 16, 16, 8, 4, 4, 2)
                assert bool(th.isfinite(out[:rows * Cout]).all()) and bool(th.isnan(out[rows * Cout:]).all())
            else:
                launch(entry, 2, dout, Cout, x, Kc, out, Kc, Cout, Kc, rows, None, 0, 2, db, 16, 16, 8, 4, 4, 2)
                assert bool(th.isfinite(out[:2 * Cout * Kc]).all()) and bool(th.isnan(out[2 * Cout * Kc:]).all())
                db.fill_(NAN)
