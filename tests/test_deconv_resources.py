"""What the compiler made of the kernels of the flux-error-convolved likelihood (csrc/lf_deconv.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, and the LDS DESIGN.md section 3.18 states - 544
bytes for lf_deconv_part (the node table of up to 32 nodes and the four waves' totals), none for lf_deconv_final - in each
of the three variants' instantiations."""
import os
import re

import pytest

import lf_isalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def test_deconv_part_uses_no_scratch_and_the_stated_lds(remarks):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_deconv_partILi[012]E", k)}
    assert len(hits) == 3, sorted(remarks)                       # FREE, FIXCOMP, ZEVOL
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 544, (name, r)
        assert r["VGPRs"] <= 128, (name, r)                      # four waves per SIMD at least
        print(name, r)


def test_deconv_final_uses_no_scratch_and_no_lds(remarks):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_deconv_final", k)}
    assert len(hits) == 1, sorted(remarks)
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (name, r)


def test_the_header_and_the_design_state_the_same_lds():
    lay = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_layout.h")).read()
    kmax = int(re.search(r"constexpr int DECONV_KMAX = (\d+)", lay).group(1))
    assert (2 * kmax + 4) * 8 == 544
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.18" in design and "544 bytes" in design[design.index("### 3.18"):]
