"""What the compiler made of the chain-diagnostics kernels (csrc/lf_diag.h; hipcc -Rpass-analysis=kernel-resource-usage, no GPU
needed): no scratch, no spills, and the LDS DESIGN.md section 3.12 states - 39 456 bytes for lf_diag_acf, four workgroups per
CU by LDS, three waves per SIMD by registers."""
import os
import re

import pytest

import lf_isalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = {"lf_diag_moments": 2048, "lf_diag_acf": 39456, "lf_diag_norm": 0}


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_diag_kernel_uses_no_scratch_and_the_stated_lds(remarks, kernel):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+%sE" % kernel, k)}
    assert len(hits) == 1, sorted(remarks)
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == LDS[kernel], (name, r)
    if kernel == "lf_diag_acf":
        assert r["VGPRs"] <= 168, (name, r)                  # three waves per SIMD


def test_the_header_states_the_same_lds():
    src = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_diag.h")).read()
    dg, tb, lag = (int(re.search(r"constexpr int %s = (\d+)" % k, src).group(1)) for k in ("DIAG_DG", "DIAG_TB", "DIAG_LAGROW"))
    assert (dg * (tb + 8 + lag) + dg) * 8 == LDS["lf_diag_acf"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "39 456" in design
