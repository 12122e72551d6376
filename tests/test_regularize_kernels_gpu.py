"""The three regularizer kernels (`csrc/regularize.hip`) on the MI355X against host restatements: `ia_reg_lp` (fp32 NumPy
in the kernel's operation order, float64 sums, float64 autograd of the reference's expression), `ia_reg_weight_decay`
(torch on the CPU, bit for bit) and `ia_reg_lambda_update` (the host `IntervalParamScaler`, bit for bit in float64)."""
import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from imitation_amd import regularization as rg
from tests.test_regularization import SCALER, SCALER_CASES, SCALER_ERRORS

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 63, 64, 65, 255, 257, 1025, 4099]
THREADS = 512          # the kernels' one workgroup
U = 2.0 ** -24         # fp32 unit roundoff
LAM = 0.0173           # not representable in fp32: the kernel must round it before use


def _layout(total, mode, seed, g_shift=0):
    """Weights and pre-filled gradients in two device buffers. "one": one segment at float offset 0 (16-byte aligned);
    "three": three segments whose starts are at float offsets 1, 2 and 3 mod 4, the middle one all zero. Weights hold exact
    zeros. `g_shift`: extra float offset of every gradient segment (1: g is aligned differently from w, the scalar path)."""
    r = np.random.default_rng(seed)
    if mode == "one":
        lens, starts = [total], [0]
    else:
        lens = [total // 3, total // 3, total - 2 * (total // 3)]
        starts, at = [], 0
        for k, n in enumerate(lens):
            at = (at + 3) // 4 * 4 + (1, 2, 3)[k]
            starts.append(at)
            at += n
    size = starts[-1] + lens[-1] + 8
    w = (r.normal(size=size) * 0.7).astype(np.float32)
    w[r.random(size) < 0.1] = 0.0
    if mode == "three":
        w[starts[1]:starts[1] + lens[1]] = 0.0
    g = r.normal(size=size).astype(np.float32)
    g[g == 0] = 1.0
    W, G = th.as_tensor(w).cuda(), th.as_tensor(np.concatenate([g, g[:8]])).cuda()
    assert W.data_ptr() % 16 == 0 and G.data_ptr() % 16 == 0
    segs = [(W[s:s + n], G[s + g_shift:s + g_shift + n]) for s, n in zip(starts, lens)]
    return W, G, segs, [(s, n) for s, n in zip(starts, lens)], w, np.concatenate([g, g[:8]])


def _chain(segs):
    """The longest chain of additions a term of S passes through, from the kernel's summation layout
    (`reg_lp_kernel`): per segment a thread adds at most one head element, four components of each of its
    ceil(nv / 512) vectors and one tail element (a segment whose g is aligned differently from w: ceil(n / 512) elements);
    then 6 butterfly levels and the 8 waves' sums (7 additions)."""
    chain = 6 + 7
    for w, g in segs:
        n = w.numel()
        if (w.data_ptr() ^ g.data_ptr()) & 15:
            chain += -(-n // THREADS)
            continue
        head = min(((16 - (w.data_ptr() & 15)) & 15) >> 2, n)
        nv = (n - head) // 4
        chain += (head > 0) + 4 * -(-nv // THREADS) + ((n - head - 4 * nv) > 0)
    return chain


def _lp_fp32(w, g, lam, p):
    """The kernel's operation order in NumPy fp32: c = float(lambda) * p; q = |w|^(p-1) as a left-to-right product;
    g + c * (sign(w) * q). Returns the new gradient."""
    lam_f = np.float32(lam)
    c = lam_f * np.float32(p)
    a = np.abs(w)
    q = np.ones_like(w)
    for _ in range(p - 1):
        q = q * a
    return g + c * (np.sign(w) * q)


def _run_lp(segs, p, stats=None, scale=1.0):
    table = rg.segment_table(segs)
    lam = th.full((1,), LAM, dtype=th.float64, device="cuda")
    s_out = th.zeros(1, device="cuda")
    rg.lp_penalty(table, p, lam, stats, scale, s_out)
    th.cuda.synchronize()
    return float(s_out.item())


@pytest.mark.parametrize("mode,g_shift", [("one", 0), ("three", 0), ("three", 1)])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_lp_kernel(mode, g_shift, p):
    lam_f = float(np.float32(LAM))
    for total in LENGTHS:
        W, G, segs, spans, w, g = _layout(total, mode, 100 * p + total, g_shift)
        chain = _chain(segs)
        stats = th.tensor([0.625, 0.0, 0.0, -1.0], device="cuda")
        S = _run_lp(segs, p, stats, 0.5)
        got_g, got_w = G.cpu().numpy(), W.cpu().numpy()
        assert np.array_equal(got_w, w)   # weights untouched, nothing outside the segments written
        want_g = g.copy()
        for s, n in spans:
            want_g[s + g_shift:s + g_shift + n] = _lp_fp32(w[s:s + n], g[s + g_shift:s + g_shift + n], LAM, p)
        inside = np.zeros(len(g), bool)
        for s, n in spans:
            inside[s + g_shift:s + g_shift + n] = True
        assert np.array_equal(got_g[~inside], g[~inside]), (total, "written outside the segments")
        # float64 values of the same quantities (lambda rounded to fp32 first, as the reference's fp32 product does)
        w64 = th.tensor(np.concatenate([w[s:s + n] for s, n in spans]).astype(np.float64), requires_grad=True)
        g0 = np.concatenate([g[s + g_shift:s + g_shift + n] for s, n in spans]).astype(np.float64)
        at, pen = 0, 0.0
        for _, n in spans:   # the reference's expression, parameter by parameter
            pen = pen + th.linalg.vector_norm(w64[at:at + n], ord=p).pow(p)
            at += n
        (lam_f * pen).backward()
        prod64 = w64.grad.numpy()
        want64 = g0 + prod64
        got = np.concatenate([got_g[s + g_shift:s + g_shift + n] for s, n in spans]).astype(np.float64)
        ref32 = np.concatenate([want_g[s + g_shift:s + g_shift + n] for s, n in spans])
        if p < 3:
            # c = lambda or 2 lambda, sign(w) q = sign(w) or w: one rounded product and one rounded sum in any order
            assert np.array_equal(got.astype(np.float32), ref32), (total, p)
        else:
            # kernel: c = fl(3 l), q = fl(a a), fl(c (s q)), fl(g + .): three roundings on the product, one on the sum. Any
            # other fp32 order of the same expression has three on the product too: the two differ by at most
            # 6 u |product| + 2 u |result|
            bound = (6 * np.abs(prod64) + 2 * np.abs(want64)) * U * (1 + 1e-3)
            assert (np.abs(got - ref32.astype(np.float64)) <= bound).all(), (total, p)
        # against float64 autograd: p + 1 roundings on the product (c, the p - 2 of q, the product; p = 1, 2: one), one sum
        bound = ((p + 1) * np.abs(prod64) + np.abs(want64)) * U * (1 + 1e-3)
        assert (np.abs(got - want64) <= bound).all(), (total, p, float(np.abs(got - want64).max()))
        # S: a term carries p - 1 roundings of the power and at most `chain` additions; all terms are non-negative
        S64 = float((np.abs(w64.detach().numpy()) ** p).sum())
        k = chain + p - 1
        assert abs(S - S64) <= k * U / (1 - k * U) * S64, (total, p, S, S64, chain)
        if mode == "three":   # the all-zero segment: sign(0) = 0, its gradients are untouched for every p
            s, n = spans[1]
            assert np.array_equal(got_g[s + g_shift:s + g_shift + n], g[s + g_shift:s + g_shift + n])
        # regularized_loss = fl(fl(loss * scale) + fl(float(lambda) * S))
        want_rl = np.float32(0.625) * np.float32(0.5) + np.float32(LAM) * np.float32(S)
        st = stats.cpu().numpy()
        assert st[3] == want_rl and st[0] == np.float32(0.625)


def test_lp_kernel_all_zero_weights_and_null_gradient():
    for p in (1, 2, 3):
        W, G = th.zeros(70, device="cuda"), th.full((70,), 0.5, device="cuda")
        assert _run_lp([(W[1:68], G[1:68])], p) == 0.0
        assert th.equal(G, th.full((70,), 0.5, device="cuda"))   # sign(0) = 0: nothing added for any p
    W = th.arange(9, device="cuda", dtype=th.float32)
    assert _run_lp([(W, None)], 2) == float((np.arange(9.0) ** 2).sum())   # a null gradient: S only


@pytest.mark.parametrize("mode", ["one", "three"])
def test_weight_decay_kernel(mode):
    lr = 1e-3
    for total in LENGTHS:
        W, G, segs, spans, w, g = _layout(total, mode, total)
        lam = th.full((1,), LAM, dtype=th.float64, device="cuda")
        rg.weight_decay(rg.segment_table([(a, None) for a, _ in segs]), lam, lr)
        want = w.copy()
        for s, n in spans:
            x = th.as_tensor(w[s:s + n])
            want[s:s + n] = (x + th.tensor(-LAM * lr).float() * x).numpy()
        assert np.array_equal(W.cpu().numpy(), want), total
        assert np.array_equal(G.cpu().numpy(), g)


def _update(lam, train, val, prev=None):
    """One `ia_reg_lambda_update` on losses given as (fp32 loss, fp32 scale) rows whose products are the wanted losses."""
    lam_d = th.full((1,), lam, dtype=th.float64, device="cuda")
    tr = th.tensor([[train, 9.0, 9.0, 9.0]], dtype=th.float32, device="cuda")
    va = th.tensor([[val, 9.0, 9.0, 9.0]], dtype=th.float32, device="cuda")
    row = th.full((4,), -7.0, dtype=th.float64, device="cuda")
    rg.lambda_update(lam_d, SCALER, tr, th.ones(1, device="cuda"), va, row, prev)
    return float(lam_d.item()), row.cpu().numpy(), row


@pytest.mark.parametrize("lam,train,val,want", SCALER_CASES)
def test_lambda_update_kernel_matches_the_host_scaler(lam, train, val, want):
    t32, v32 = float(np.float32(train)), float(np.float32(val))   # the losses the kernel sees are fp32
    host = SCALER(lam, t32, v32)
    got, row, _ = _update(lam, train, val)
    assert got == host and list(row) == [host, t32, v32, 0.0]
    if t32 == train and v32 == val:
        assert got == want


def test_lambda_update_kernel_ratio_exactly_at_the_bound():
    got, row, _ = _update(0.01, 1.0, 2.0)   # ratio 2.0 against the upper bound 2.0: strict comparison
    assert got == 0.01 and list(row) == [0.01, 1.0, 2.0, 0.0]
    got, _, _ = _update(0.01, 1.0, float(np.nextafter(np.float32(2.0), np.float32(3.0))))
    assert got == 0.01 * 1.5


def test_lambda_update_kernel_sums_in_order_with_fp32_scaled_products():
    r = np.random.default_rng(0)
    loss = r.uniform(0.3, 0.9, size=(7, 4)).astype(np.float32)
    scale = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.375], np.float32)
    vloss = r.uniform(0.3, 0.9, size=(3, 4)).astype(np.float32)
    train = val = 0.0
    for k in range(7):
        train += float(loss[k, 0] * scale[k])
    for k in range(3):
        val += float(vloss[k, 0])
    stats = th.as_tensor(np.concatenate([loss, vloss])).cuda()
    lam_d = th.full((1,), 0.02, dtype=th.float64, device="cuda")
    row = th.zeros(4, dtype=th.float64, device="cuda")
    rg.lambda_update(lam_d, SCALER, stats[:7], th.as_tensor(scale).cuda(), stats[7:], row)
    assert list(row.cpu().numpy()) == [SCALER(0.02, train, val), train, val, 0.0]


@pytest.mark.parametrize("lam,train,val,msg", SCALER_ERRORS)
def test_lambda_update_kernel_error_codes(lam, train, val, msg):
    got, row, row_d = _update(lam, train, val)
    assert got == lam   # lambda left alone
    code = int(row[3])
    assert code != 0 and msg in rg.ERROR_MESSAGES[code]
    assert list(row[:3]) == [lam, float(np.float32(train)), float(np.float32(val))]
    # ... and from then on: the next epoch carries the code over and leaves a (now valid) lambda alone
    got2, row2, _ = _update(0.01, 1.0, 2.5, prev=row_d)
    assert got2 == 0.01 and int(row2[3]) == code
    assert sorted(rg.ERROR_MESSAGES) == [L.REG_LAMBDA_ZERO, L.REG_LAMBDA_NEGATIVE, L.REG_LOSS_NEGATIVE]


def test_kernels_are_deterministic():
    outs = []
    for _ in range(2):
        W, G, segs, spans, w, g = _layout(4099, "three", 7)
        stats = th.tensor([0.625, 0.0, 0.0, 0.0], device="cuda")
        S = _run_lp(segs, 3, stats, 0.5)
        lam = th.full((1,), LAM, dtype=th.float64, device="cuda")
        rg.weight_decay(rg.segment_table([(a, None) for a, _ in segs]), lam, 1e-3)
        lam2, row, _ = _update(0.01, 0.7, 0.3)
        outs.append((S, G.cpu().numpy(), W.cpu().numpy(), stats.cpu().numpy(), lam2, row))
    for a, b in zip(*outs):
        assert np.array_equal(np.asarray(a), np.asarray(b))
