"""What the compiler made of the posterior-band kernels (csrc/lf_bands.h; hipcc -Rpass-analysis=kernel-resource-usage, no GPU
needed): no scratch, the 32 KiB of keys DESIGN.md section 3.9 states (five workgroups per CU), and few enough VGPRs that the
LDS, not the registers, sets the occupancy."""
import pytest

import lf_isalib


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


@pytest.mark.parametrize("nrec", [3, 7])
def test_band_kernel_uses_no_scratch_and_the_stated_lds(remarks, nrec):
    hits = {k: v for k, v in remarks.items() if k.startswith("_ZN2lf8lf_bandsILi%dEEE" % nrec)}
    assert len(hits) == 1, sorted(remarks)
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 32 * 1024, (name, r)
        assert r["VGPRs"] <= 64, (name, r)            # 8 waves per SIMD by registers; LDS allows 5
