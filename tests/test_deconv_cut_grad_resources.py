"""What the compiler made of the kernels of the cut's gradient (csrc/lf_deconv_cut_grad.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills and 4 x (slots summed) x 8 bytes of LDS (the four
waves' totals) for lf_deconv_cut_grad_part in each of the three variants' instantiations, neither scratch nor LDS for
lf_deconv_cut_grad_final, and the registers the build gives (DESIGN.md section 3.33 states them)."""
import re

import pytest

import lf_isalib

SLOTS = {0: 5, 1: 3, 2: 7}                                # variant -> running sums: FREE, FIXCOMP, ZEVOL
PINNED_PART = {0: (90, 72), 1: (50, 44), 2: (52, 70)}      # variant -> (VGPRs, SGPRs): what the build gives
PINNED_FINAL = {0: (22, 41), 1: (16, 30), 2: (16, 30)}


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def _hits(remarks, kernel):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+%sILi[012]E" % kernel, k)}
    assert len(hits) == 3, sorted(remarks)                       # FREE, FIXCOMP, ZEVOL
    return {int(re.search(r"ILi([012])E", k).group(1)): (k, v) for k, v in hits.items()}


def test_cut_grad_part_uses_no_scratch_and_the_stated_resources(remarks):
    for v, (name, r) in sorted(_hits(remarks, "lf_deconv_cut_grad_part").items()):
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 4 * SLOTS[v] * 8, (name, r)
        assert (r["VGPRs"], r["TotalSGPRs"]) == PINNED_PART[v], (name, r)


def test_cut_grad_final_uses_no_scratch_and_no_lds(remarks):
    for v, (name, r) in sorted(_hits(remarks, "lf_deconv_cut_grad_final").items()):
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (name, r)
        assert (r["VGPRs"], r["TotalSGPRs"]) == PINNED_FINAL[v], (name, r)
