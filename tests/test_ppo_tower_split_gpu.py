"""The persistent PPO update with ONE TOWER PER GRADIENT WORKGROUP (`ia_ppo_update_tower_split(1)`,
`ppo_update_split_kernel`) against the form with one workgroup per row block: the same tile MFMA order, the same
slab-order sums and the same sum vector, so every output must be equal bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from imitation_amd import _lib as L
from tests.test_kernels_gpu import DEV, DevPolicy, _oracle_policy, dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


def _host_inputs(D, A, discrete, norm, T, n, H=32, seed=0):
    """Seeded policy and rollout on the host, built as `test_ppo_epochs_match_oracle` builds them (no oracle run, no
    device): time-major arrays and the two permutations `np.random.seed(123)` gives `RolloutBuffer.get`."""
    pol = _oracle_policy(D, A, H, discrete, norm, seed=3)
    rng = np.random.default_rng(seed)
    aw = 1 if discrete else A
    obs = rng.standard_normal((T, n, D)).astype(np.float32)
    act = (rng.integers(0, A, (T, n, 1)) if discrete else rng.standard_normal((T, n, A))).astype(np.float32)
    values = rng.standard_normal((T, n)).astype(np.float32)
    adv = rng.standard_normal((T, n)).astype(np.float32)
    ret = adv + values
    with th.no_grad():
        pol.set_training_mode(False)
        acts_t = th.as_tensor(act.reshape(T * n, aw))
        _, lp, _ = pol.evaluate_actions(th.as_tensor(obs.reshape(T * n, D)),
                                        acts_t.long().flatten() if discrete else acts_t)
    logp = (lp.numpy() + 0.1 * rng.standard_normal(T * n)).reshape(T, n).astype(np.float32)
    np.random.seed(123)
    perms = np.stack([np.random.permutation(T * n) for _ in range(2)])
    return pol, dict(obs=obs, act=act, lp=logp, adv=adv, ret=ret, perm=perms)


def _upload(host):
    """The host rollout of `_host_inputs` on the device."""
    obs, act, logp, adv, ret, perms = (host[k] for k in ("obs", "act", "lp", "adv", "ret", "perm"))
    T = obs.shape[0]
    # (one time slice more than T behind the observations, as the rollout tile has: rows are read in 16-byte pieces)
    d_obs = dev(np.concatenate([obs, np.zeros_like(obs[:1])]))[:T]
    return dict(obs=d_obs, act=dev(act), lp=dev(logp), adv=dev(adv), ret=dev(ret), perm=th.as_tensor(perms).to(DEV))


def _inputs(D, A, discrete, norm, T, n, H=32, seed=0):
    """`_host_inputs` with the rollout on the device."""
    pol, host = _host_inputs(D, A, discrete, norm, T, n, H, seed)
    return pol, _upload(host)


def _run(pol, rows, D, A, discrete, norm, T, n, bs, split, launches):
    """Two epochs through `ia_ppo_update` from a fresh copy of the state; `launches` = 1: one call of two epochs, 2: one
    call per epoch on the same workspace. Returns every output and the workspace's error word."""
    lib = L.load()
    dp = DevPolicy(pol, D, A, 32, discrete, norm)
    nws = int(lib.ia_ppo_update_ws_floats(C.byref(dp.d), bs))
    assert nws > 0
    uws = th.zeros(nws, device=DEV)
    n_mb = -(-T * n // bs)
    stats = th.zeros(2, n_mb, 8, device=DEV)
    lib.ia_ppo_update_tower_split(1 if split else 0)
    try:
        for k in range(launches):
            ne = 2 // launches
            L.call("ia_ppo_update", C.byref(dp.d), L.ptr(dp.P), L.ptr(dp.Pt), L.ptr(dp.nm), L.ptr(dp.nv), L.ptr(dp.nc),
                   int(norm), L.ptr(rows["obs"]), L.ptr(rows["act"]), L.ptr(rows["lp"]), L.ptr(rows["adv"]),
                   L.ptr(rows["ret"]), L.ptr(rows["perm"][k * ne:(k + 1) * ne].contiguous()), ne, T, n, bs, 1, 0.2, 0.05, 0.5,
                   0.5, L.ptr(dp.m), L.ptr(dp.v), 3e-4, 0.9, 0.999, 1e-5, k * ne * n_mb, L.ptr(uws),
                   L.ptr(stats[k * ne:(k + 1) * ne]), L.stream())
        th.cuda.synchronize()
    finally:
        lib.ia_ppo_update_tower_split(0)
    out = dict(P=dp.P, Pt=dp.Pt, m=dp.m, v=dp.v, stats=stats)
    if norm:
        out.update(nm=dp.nm, nv=dp.nv, nc=dp.nc)
    return out, int(uws[8:9].view(th.int32).item())


def _compare(D, A, discrete, norm, T, n, bs, launches=1, assume_cus=None):
    pol, rows = _inputs(D, A, discrete, norm, T, n)
    off, err_off = _run(pol, rows, D, A, discrete, norm, T, n, bs, False, launches)
    lib = L.load()
    if assume_cus is not None:
        lib.ia_ppo_update_assume_cus(assume_cus)
    try:
        on, err_on = _run(pol, rows, D, A, discrete, norm, T, n, bs, True, launches)
    finally:
        lib.ia_ppo_update_assume_cus(0)
    assert err_off == 0 and err_on == 0, (err_off, err_on)
    assert th.isfinite(on["P"]).all() and not th.equal(on["P"], DevPolicy(pol, D, A, 32, discrete, norm).P)
    for k in off:
        assert th.equal(off[k], on[k]), k


@pytest.mark.parametrize("D,A,discrete,norm,T,n,bs,launches", [
    # config P's kernel at nblk = 4: the narrow second K tile as dots, 8 parameters per thread
    (17, 6, False, True, 16, 64, 256, 1),
    # 9 parameters per thread; the second K tile holds 11 columns and runs as MFMA tiles
    (27, 8, False, True, 8, 64, 256, 1),
    # KS1 = 16, one action, nblk = 3 (odd; the last block has 12 rows), ONE step per epoch: two launches of one epoch on
    # the same workspace -- the sequence base and the buffer parity carry over an odd step count
    (33, 1, False, False, 2, 70, 140, 2),
    # 13 actions per quad; the short last minibatch (32 rows) leaves row block 1 without rows
    (20, 13, True, True, 4, 32, 96, 1),
    # 64 gradient workgroups, 4 statistics slices (two slicer workgroups each)
    (17, 6, False, True, 16, 256, 2048, 1)])
def test_tower_split_equals_the_two_tower_form(D, A, discrete, norm, T, n, bs, launches):
    _compare(D, A, discrete, norm, T, n, bs, launches)


def test_tower_split_falls_back_when_its_grid_does_not_fit():
    """Room for nblk + 1 + n_slices workgroups only: the split grid is not co-resident, the call succeeds on the form
    with one workgroup per row block (equal results again)."""
    nblk, n_slices = 4, 0   # 256-row minibatches: four row blocks, no statistics slices (the split grid needs 2 nblk + 1)
    _compare(17, 6, False, True, 16, 64, 256, 1, assume_cus=nblk + 1 + n_slices)
