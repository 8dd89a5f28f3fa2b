"""What the compiler made of the kernels of the per-source luminosity posterior (csrc/lf_lumpost.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, at most 128 vector registers, and the LDS DESIGN.md
section 3.22 states - the node table of the largest wide class, 144 nodes (2304 bytes), plus the LUMPOST_RT = 2 rows' constants
(176 bytes each): 2656 bytes for lf_lumpost_part in each of the three variants' instantiations, none for lf_lumpost_fold -
with the registers and occupancy that section records."""
import os
import re

import pytest

import lf_isalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX, ROW_BYTES = 144, 176
# variant (LF_FREE 0, LF_FIXCOMP 1, LF_ZEVOL 2): VGPRs, SGPRs, occupancy (waves per SIMD)
PINNED = {0: (56, 74, 8), 1: (56, 74, 8), 2: (64, 76, 8)}


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def _clean(r):
    return r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0 and r["VGPRs"] <= 128


def test_lumpost_part_uses_no_scratch_and_the_stated_lds(remarks):
    pat = r"_ZN2lf\d+lf_lumpost_partILi([012])E"
    hits = {int(re.match(pat, k).group(1)): v for k, v in remarks.items() if re.match(pat, k)}
    assert sorted(hits) == [0, 1, 2], sorted(remarks)               # FREE, FIXCOMP, ZEVOL
    lay = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_layout.h")).read()
    rt = int(re.search(r"constexpr int LUMPOST_RT = (\d+);", lay).group(1))
    for v, r in hits.items():
        print(v, r)
        assert _clean(r), (v, r)
        assert r["LDS Size"] == 2 * KMAX * 8 + rt * ROW_BYTES == 2656, (v, r)
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"]) == PINNED[v], (v, r)


def test_lumpost_fold_uses_no_scratch_and_no_lds(remarks):
    hits = [v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_lumpost_foldE", k)]
    assert len(hits) == 1, sorted(remarks)
    print(hits[0])
    assert _clean(hits[0]) and hits[0]["LDS Size"] == 0, hits[0]


def test_the_headers_and_the_design_state_the_same_resources():
    hdr = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_lumpost.h")).read()
    assert "DECONV_WIDE_TABLE_BYTES + LUMPOST_RT * (int)sizeof(DeconvRow)" in hdr
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.22" in design
    sec = design[design.index("### 3.22"):]
    assert "2656 bytes" in sec
    for vgprs, sgprs, occ in PINNED.values():
        assert re.search(r"\| *%d *\| *%d *\| *%d *\|" % (vgprs, sgprs, occ), sec), (vgprs, sgprs, occ)
