"""What the compiler made of the kernels of the cut on the observed flux (csrc/lf_deconv_cut.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, 32 bytes of LDS (the four waves' totals) for
lf_deconv_cut_part in each of the three variants' instantiations, none for lf_deconv_cut_final, and the registers the build
gives (DESIGN.md section 3.31 states them)."""
import re

import pytest

import lf_isalib

PINNED = {0: (51, 72), 1: (42, 44), 2: (35, 72)}          # variant -> (VGPRs, SGPRs): what the build gives


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def test_cut_part_uses_no_scratch_and_the_stated_resources(remarks):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_deconv_cut_partILi[012]E", k)}
    assert len(hits) == 3, sorted(remarks)                       # FREE, FIXCOMP, ZEVOL
    for name, r in hits.items():
        v = int(re.search(r"ILi([012])E", name).group(1))
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 32, (name, r)
        assert (r["VGPRs"], r["TotalSGPRs"]) == PINNED[v], (name, r)


def test_cut_final_uses_no_scratch_and_no_lds(remarks):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_deconv_cut_final", k)}
    assert len(hits) == 1, sorted(remarks)
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (name, r)
