"""What the compiler made of the integrated-LF band kernels (lf_bands_integ in csrc/lf_bands.h, Gamma(a, x) of
csrc/lf_gammainc.h inlined; hipcc -Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, the 32 KiB
of keys of DESIGN.md section 3.9, and few enough VGPRs that the LDS (five workgroups per CU), not the registers, sets the
occupancy.  Measured: 70 VGPRs (<3, 0>, <7, 0>, <3, 1>), 72 (<7, 1>); 80 is the next occupancy step above (six waves
per SIMD)."""
import pytest

import lf_isalib


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


@pytest.mark.parametrize("nrec", [3, 7])
@pytest.mark.parametrize("kind", [0, 1])
def test_integral_band_kernel_uses_no_scratch_and_the_stated_lds(remarks, nrec, kind):
    hits = {k: v for k, v in remarks.items() if k.startswith("_ZN2lf14lf_bands_integILi%dELi%dEEE" % (nrec, kind))}
    assert len(hits) == 1, sorted(remarks)
    for name, r in hits.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 32 * 1024, (name, r)
        assert r["VGPRs"] <= 80, (name, r)            # 6 waves per SIMD by registers; LDS allows 5
