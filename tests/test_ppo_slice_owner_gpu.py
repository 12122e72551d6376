"""The tower-split persistent PPO update with hop 1's slices dealt BY TOWER and summed by the value workgroups alone
(`ia_ppo_update_slice_owner(1)`) against today's ownership (mode 0, every gradient workgroup one contiguous slice), both
with `ia_ppo_update_tower_split(1)`: only WHO sums an element and WHEN changes -- every element's slab words are still
added in slab order 0 .. nblk - 1 -- so every output must be equal bit for bit and the workspace's error word stays 0."""
import ctypes as C

import pytest
import torch as th

from imitation_amd import _lib as L
from tests.test_kernels_gpu import DEV, DevPolicy
from tests.test_ppo_tower_split_gpu import _inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


def _run(pol, rows, D, A, discrete, norm, T, n, bs, mode, launches):
    """Two epochs through `ia_ppo_update` from a fresh copy of the state, tower split on, slice ownership `mode`;
    `launches` = 1: one call of two epochs, 2: one call per epoch on the same workspace (as the tower-split tests run)."""
    lib = L.load()
    dp = DevPolicy(pol, D, A, 32, discrete, norm)
    nws = int(lib.ia_ppo_update_ws_floats(C.byref(dp.d), bs))
    assert nws > 0
    uws = th.zeros(nws, device=DEV)
    n_mb = -(-T * n // bs)
    stats = th.zeros(2, n_mb, 8, device=DEV)
    lib.ia_ppo_update_tower_split(1)
    assert lib.ia_ppo_update_slice_owner(mode) == 0
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
        lib.ia_ppo_update_slice_owner(0)
        lib.ia_ppo_update_tower_split(0)
    out = dict(P=dp.P, Pt=dp.Pt, m=dp.m, v=dp.v, stats=stats)
    if norm:   # (the norm state exists with observation normalisation only)
        out.update(nm=dp.nm, nv=dp.nv, nc=dp.nc)
    return out, int(uws[8:9].view(th.int32).item())


def _compare(D, A, discrete, norm, T, n, bs, launches=1, assume_cus=None):
    pol, rows = _inputs(D, A, discrete, norm, T, n)
    lib = L.load()
    m0, err0 = _run(pol, rows, D, A, discrete, norm, T, n, bs, 0, launches)
    if assume_cus is not None:
        lib.ia_ppo_update_assume_cus(assume_cus)
    try:
        m1, err1 = _run(pol, rows, D, A, discrete, norm, T, n, bs, 1, launches)
    finally:
        lib.ia_ppo_update_assume_cus(0)
    assert err0 == 0 and err1 == 0, (err0, err1)
    assert th.isfinite(m1["P"]).all() and not th.equal(m1["P"], DevPolicy(pol, D, A, 32, discrete, norm).P)
    for k in m0:
        assert th.equal(m0[k], m1[k]), k


@pytest.mark.parametrize("D,A,discrete,norm,T,n,bs,launches", [
    # config P's kernel at nblk = 4
    (17, 6, False, True, 16, 64, 256, 1),
    # nine parameters per thread
    (27, 8, False, True, 8, 64, 256, 1),
    # nblk = 3, a 12-row last block, one step per launch: parity and sequence base carry across the launches; neither the
    # 2 178 + 5 policy elements nor the 2 177 value elements are a multiple of nblk
    (33, 1, False, False, 2, 70, 140, 2),
    # discrete: no log_std range at the head of the policy elements; a row block without rows
    (20, 13, True, True, 4, 32, 96, 1),
    # 64 gradient workgroups: 32 owners, two passes each
    (17, 6, False, True, 16, 256, 2048, 1)])
def test_value_tower_owners_equal_todays_ownership(D, A, discrete, norm, T, n, bs, launches):
    _compare(D, A, discrete, norm, T, n, bs, launches)


def test_value_tower_owners_fall_back_when_the_split_grid_does_not_fit():
    """Room for nblk + 1 + n_slices workgroups only in the mode-1 call: its split grid is not co-resident, it runs the form
    with one workgroup per row block (which has no tower to deal slices by) and equals mode 0 on the split grid."""
    nblk, n_slices = 4, 0
    _compare(17, 6, False, True, 16, 64, 256, 1, assume_cus=nblk + 1 + n_slices)


def test_slice_owner_rejects_an_unknown_mode():
    lib = L.load()
    assert lib.ia_ppo_update_slice_owner(2) != 0
    assert lib.ia_ppo_update_slice_owner(0) == 0
