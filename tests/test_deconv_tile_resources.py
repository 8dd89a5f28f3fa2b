"""What the compiler made of the row-tiled correction kernel (csrc/lf_deconv_tile.h; hipcc -Rpass-analysis=kernel-resource-usage,
no GPU needed): two instantiations (FIXCOMP, ZEVOL; none for FREE), no scratch, no spills, no AGPRs, the LDS DESIGN.md section
3.20 states - the node table, the rows' constants, the four waves' totals and the tile's sums - and the registers and
occupancy that section records.  lf_deconv_part keeps the figures of tests/test_deconv_resources.py."""
import os
import re

import pytest

import lf_isalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lumfuncmcmc_amd", "csrc")
DECONV_ROW_DOUBLES = 9 + 2 + 3 + 2 + 6        # DeconvRow of lf_deconv.h: GradRow, c1l Q, aC lF vs, aC_ln kc2, GradPiv
VGPRS, OCCUPANCY = 107, 4                      # as built; DESIGN.md section 3.20


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def tile_lds():
    lay = open(os.path.join(CSRC, "lf_layout.h")).read()
    kmax = int(re.search(r"constexpr int DECONV_KMAX = (\d+)", lay).group(1))
    rt = int(re.search(r"constexpr int DECONV_RT = (\d+)", open(os.path.join(CSRC, "lf_deconv_tile.h")).read()).group(1))
    return rt, 2 * kmax * 8 + rt * DECONV_ROW_DOUBLES * 8 + 4 * rt * 8 + rt * 8


def test_deconv_tile_resources(remarks):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_deconv_tileILi\dE", k)}
    assert sorted(re.search(r"ILi(\d)E", k).group(1) for k in hits) == ["1", "2"], sorted(remarks)      # FIXCOMP, ZEVOL; no FREE
    rt, lds = tile_lds()
    assert (rt, lds) == (8, 2240)
    for name, r in hits.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
        assert r["LDS Size"] == lds, (name, r)
        assert r["VGPRs"] == VGPRS and r["Occupancy"] == OCCUPANCY, (name, r)


def test_deconv_part_is_as_it_was(remarks):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_deconv_partILi[012]E", k)}
    assert len(hits) == 3
    assert sorted(r["VGPRs"] for r in hits.values()) == [51, 51, 55]
    for r in hits.values():
        assert r["LDS Size"] == 544 and r["ScratchSize"] == 0 and r["Occupancy"] == 8


def test_the_design_states_the_same_figures():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.20" in design
    sec = design[design.index("### 3.20"):]
    assert "2240 bytes" in sec and "%d VGPRs" % VGPRS in sec
