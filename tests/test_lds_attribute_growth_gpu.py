"""A kernel's dynamic-LDS limit grows with the shape (`ensure_lds` in `policy.hip`): a launch that needs more dynamic LDS
than any earlier launch of the same kernel must raise the kernel's attribute again, not rely on the first call's.

Run in a FRESH process (this module's `__main__`), so that no earlier test has raised any attribute: three
`ia_ppo_update` calls with the tower split on -- a small policy, a larger one that selects the same kernel variant (two
gradient row blocks, observation width <= 32, 8 parameters per thread) and needs more LDS (155 216 against 144 072 bytes
by `upd_grad_lds_bytes`), and the larger one again -- then `ia_policy_logits` + `ia_policy_act` at hidden width 32 and 64
on 70 rows (two workgroups, the second partly empty), each repeated."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch as th

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _update_runs():
    from tests.test_ppo_tower_split_gpu import _inputs, _run
    small = (4, 3, True, True, 4, 32, 128)      # D, A, discrete, RunningNorm, T, n, batch
    large = (17, 6, False, True, 4, 32, 128)
    outs = []
    for shape in (small, large, large):
        pol, rows = _inputs(*shape[:6])
        out, err = _run(pol, rows, *shape, True, 1)   # (raises unless every call returns IA_OK)
        assert err == 0, (shape, err)               # workspace word 8
        assert all(th.isfinite(t.float()).all() for t in out.values()), shape
        outs.append(out)
    assert set(outs[1]) == {"P", "Pt", "m", "v", "stats", "nm", "nv", "nc"}
    for k in outs[1]:
        assert th.equal(outs[1][k], outs[2][k]), k


def _inference_runs():
    from imitation_amd import _lib as L
    from tests.test_kernels_gpu import DEV, DevPolicy, _oracle_policy, dev, rnd
    D, A, n = 4, 3, 70
    obs = dev(rnd(n, D, seed=4))
    noise = dev(th.rand(n, generator=th.Generator().manual_seed(5)))
    low, high = dev(-th.ones(A)), dev(th.ones(A))
    for H in (32, 64):
        dp = DevPolicy(_oracle_policy(D, A, H, True, True), D, A, H, True, True)
        got = []
        for _ in range(2):
            logits, lv = th.empty(n, A, device=DEV), th.empty(n, device=DEV)
            acts, clip = th.empty(n, 1, device=DEV), th.empty(n, 1, device=DEV)
            vals, logp = th.empty(n, device=DEV), th.empty(n, device=DEV)
            L.call("ia_policy_logits", C.byref(dp.d), L.ptr(dp.P), L.ptr(dp.Pt), L.ptr(dp.nm), L.ptr(dp.nv), L.ptr(obs), n,
                   L.ptr(logits), L.ptr(lv), L.stream())
            L.call("ia_policy_act", C.byref(dp.d), L.ptr(dp.P), L.ptr(dp.Pt), L.ptr(dp.nm), L.ptr(dp.nv), L.ptr(obs), n,
                   L.ptr(noise), L.ptr(low), L.ptr(high), L.ptr(acts), L.ptr(clip), L.ptr(vals), L.ptr(logp), L.stream())
            th.cuda.synchronize()
            got.append((logits, lv, acts, clip, vals, logp))
        for x, y in zip(*got):
            assert th.isfinite(x).all() and th.equal(x, y), H


def test_lds_attribute_grows_with_the_shape_in_a_fresh_process():
    if not th.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run([sys.executable, "-m", "tests.test_lds_attribute_growth_gpu"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "LDS_GROWTH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    from imitation_amd import _lib

    _lib.load()
    _update_runs()
    _inference_runs()
    print("LDS_GROWTH_OK")
