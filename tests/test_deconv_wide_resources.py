"""What the compiler made of the kernels of the wide rule (csrc/lf_deconv_wide.h; hipcc -Rpass-analysis=kernel-resource-usage,
no GPU needed): no scratch, no spills, the LDS DESIGN.md section 3.21 states - the table of the largest class, 144 nodes (2304
bytes), plus the four waves' totals: 2336 bytes for lf_deconv_wide_part, 2432 (FREE, ZEVOL: 4 slots) and 2368 (FIXCOMP: 2) for
lf_deconv_wide_grad_part - and the registers and occupancy section 3.21 records, pinned at what the compile gives in each of
the three variants' instantiations."""
import os
import re

import pytest

import lf_isalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = 144
# variant (LF_FREE 0, LF_FIXCOMP 1, LF_ZEVOL 2): VGPRs, SGPRs, occupancy (waves per SIMD)
PINNED_VALUE = {0: (51, 62, 8), 1: (51, 62, 8), 2: (55, 76, 8)}
# ... and the gradient's slots in front
PINNED_GRAD = {0: (4, 81, 62, 5), 1: (2, 57, 62, 8), 2: (4, 71, 76, 7)}


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def _hits(remarks, kernel):
    pat = r"_ZN2lf\d+%sILi([012])E" % kernel
    hits = {int(re.match(pat, k).group(1)): v for k, v in remarks.items() if re.match(pat, k)}
    assert sorted(hits) == [0, 1, 2], sorted(remarks)               # FREE, FIXCOMP, ZEVOL
    return hits


def test_deconv_wide_part_uses_no_scratch_and_the_stated_lds(remarks):
    for v, r in _hits(remarks, "lf_deconv_wide_part").items():
        print(v, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (v, r)
        assert r["LDS Size"] == (2 * KMAX + 4) * 8 == 2336, (v, r)
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"]) == PINNED_VALUE[v], (v, r)


def test_deconv_wide_grad_part_uses_no_scratch_and_the_stated_lds(remarks):
    for v, r in _hits(remarks, "lf_deconv_wide_grad_part").items():
        slots, vgprs, sgprs, occ = PINNED_GRAD[v]
        print(v, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (v, r)
        assert r["LDS Size"] == (2 * KMAX + 4 * slots) * 8, (v, r)
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"]) == (vgprs, sgprs, occ), (v, r)


def test_the_headers_and_the_design_state_the_same_resources():
    lay = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_layout.h")).read()
    panels = [int(p) for p in re.search(r"DECONV_WIDE_PANELS\[DECONV_WIDE_NCLASS\] = \{([^}]*)\}", lay).group(1).split(",")]
    npan = int(re.search(r"constexpr int DECONV_WIDE_NPAN = (\d+)", lay).group(1))
    assert max(panels) * npan == KMAX
    hdr = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_deconv_wide.h")).read()
    assert "2 * DECONV_WIDE_KMAX * 8" in hdr
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.21" in design
    sec = design[design.index("### 3.21"):]
    assert "2336 bytes" in sec and "2432 bytes" in sec and "2368 bytes" in sec
    for vgprs, sgprs, occ in list(PINNED_VALUE.values()) + [p[1:] for p in PINNED_GRAD.values()]:
        assert re.search(r"\| *%d *\| *%d *\| *%d *\|" % (vgprs, sgprs, occ), sec), (vgprs, sgprs, occ)
