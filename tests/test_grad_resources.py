"""What the compiler made of the gradient kernels (csrc/lf_grad.h; hipcc -Rpass-analysis=kernel-resource-usage, no GPU needed):
no scratch, no spills, and the LDS DESIGN.md section 3.14 states - 256 bytes for lf_grad_part (the four waves' totals of its
8 slots), none for lf_grad_final - in each of the three variants' instantiations."""
import os
import re

import pytest

import lf_isalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = {"lf_grad_part": 256, "lf_grad_final": 0}


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_grad_kernel_uses_no_scratch_and_the_stated_lds(remarks, kernel):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+%sILi[012]E" % kernel, k)}
    assert len(hits) == 3, sorted(remarks)                       # FREE, FIXCOMP, ZEVOL
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == LDS[kernel], (name, r)
        assert r["VGPRs"] <= 128, (name, r)                      # four waves per SIMD at least


def test_the_header_and_the_design_state_the_same_lds():
    lay = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_layout.h")).read()
    slots = int(re.search(r"constexpr int GRAD_SLOTS = (\d+)", lay).group(1))
    assert 4 * slots * 8 == LDS["lf_grad_part"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.14" in design and "256 bytes" in design[design.index("### 3.14"):]
