"""What the compiler made of the kernels of the convolved likelihood's gradient (csrc/lf_deconv_grad.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, the LDS DESIGN.md section 3.19 states - the node
table of up to 32 nodes (512 bytes) plus the four waves' slot totals, 640 bytes for FREE and ZEVOL (4 slots), 576 for FIXCOMP
(2 slots); none for lf_deconv_grad_final - and the registers and occupancy section 3.19 records, pinned at what the compile
gives in each of the three variants' instantiations."""
import os
import re

import pytest

import lf_isalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# variant (LF_FREE 0, LF_FIXCOMP 1, LF_ZEVOL 2): slots, VGPRs, SGPRs, occupancy (waves per SIMD)
PINNED = {0: (4, 82, 68, 5), 1: (2, 58, 64, 8), 2: (4, 72, 78, 7)}


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def test_deconv_grad_part_uses_no_scratch_and_the_stated_lds(remarks):
    hits = {int(re.match(r"_ZN2lf\d+lf_deconv_grad_partILi([012])E", k).group(1)): v for k, v in remarks.items()
            if re.match(r"_ZN2lf\d+lf_deconv_grad_partILi[012]E", k)}
    assert sorted(hits) == [0, 1, 2], sorted(remarks)               # FREE, FIXCOMP, ZEVOL
    for v, r in hits.items():
        slots, vgprs, sgprs, occ = PINNED[v]
        print(v, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (v, r)
        assert r["LDS Size"] == (2 * 32 + 4 * slots) * 8, (v, r)
        assert r["AGPRs"] == 0, (v, r)
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"]) == (vgprs, sgprs, occ), (v, r)


def test_deconv_grad_final_uses_no_scratch_and_no_lds(remarks):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_deconv_grad_finalILi[012]E", k)}
    assert len(hits) == 3, sorted(remarks)
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (name, r)


def test_the_header_and_the_design_state_the_same_resources():
    lay = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_layout.h")).read()
    assert int(re.search(r"constexpr int DECONV_KMAX = (\d+)", lay).group(1)) == 32
    hdr = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_deconv_grad.h")).read()
    assert "(2 * DECONV_KMAX + 4 * dgrad_slots<V>()) * 8" in hdr and "V == LF_FIXCOMP ? 2 : 4" in hdr
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.19" in design
    sec = design[design.index("### 3.19"):]
    assert "640 bytes" in sec and "576 bytes" in sec
    for slots, vgprs, sgprs, occ in PINNED.values():
        assert re.search(r"\| *%d *\| *%d *\| *%d *\|" % (vgprs, sgprs, occ), sec), (vgprs, sgprs, occ)
