"""The built library's notes for `ppo_update_split_kernel` (one tower per gradient workgroup): like every production
instantiation of the persistent PPO update, it keeps every value in registers."""
import os
import re
import shutil

import pytest


def test_tower_split_kernels_do_not_spill():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("llvm-readelf / c++filt not available")
    from tools.kernel_resources import kernel_notes

    ks = [k for k in kernel_notes() if "ppo_update_split_kernel<" in k["name"]]
    assert len(ks) == 8, [k["name"] for k in ks]   # {8, 9 parameters per thread} x {production, phase clocks} x {KS1 8, 16}
    prod = [k for k in ks if not re.search(r"kernel<\d+, true,", k["name"])]
    assert len(prod) == 4, [k["name"] for k in prod]
    for k in prod:
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k
