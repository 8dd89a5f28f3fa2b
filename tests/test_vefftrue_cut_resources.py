"""What the compiler made of the kernels of the deconvolved 1/Veff points under the cut (csrc/lf_vefftrue_cut.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, and the registers, LDS and occupancy that DESIGN.md
section 3.34 states - lf_vefftrue_part_cut, lf_vefftrue_part's statements with the nodes' factors, in the three variants'
instantiations (the same 2480 bytes of static LDS, the same five waves per SIMD: the extra load costs three vector registers);
lf_vefftrue_cutvol (static: the node offsets of the largest wide class and four counts, 1168 bytes; the cut model's image is
dynamic, vefft_cut_lds_bytes) and lf_cut_volume_points.  The plain kernel, lf_vefftrue_part, keeps the figures of
tests/test_vefftrue_resources.py."""
import os
import re

import pytest

import lf_isalib
from test_vefftrue_resources import LDS, PINNED as PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# variant (LF_FREE 0, LF_FIXCOMP 1, LF_ZEVOL 2): VGPRs, SGPRs, occupancy (waves per SIMD)
PINNED_CUT = {0: (87, 106, 5), 1: (87, 106, 5), 2: (87, 106, 5)}
CUTVOL = (30, 74, 8, 144 * 8 + 4 * 4)          # VGPRs, SGPRs, occupancy, static LDS
POINTS = (28, 46, 8, 0)


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def _clean(r):
    return r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0 and r["VGPRs"] <= 128


def test_part_cut_uses_no_scratch_and_keeps_the_occupancy(remarks):
    pat = r"_ZN2lf\d+lf_vefftrue_part_cutILi([012])E"
    hits = {int(re.match(pat, k).group(1)): v for k, v in remarks.items() if re.match(pat, k)}
    assert sorted(hits) == [0, 1, 2], sorted(remarks)
    for v, r in hits.items():
        print(v, r)
        assert _clean(r), (v, r)
        assert r["LDS Size"] == LDS == 2480, (v, r)
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"]) == PINNED_CUT[v], (v, r)
        assert r["Occupancy"] == PLAIN[v][2]


def test_the_plain_part_kernel_keeps_its_figures(remarks):
    pat = r"_ZN2lf\d+lf_vefftrue_partILi([012])E"
    hits = {int(re.match(pat, k).group(1)): v for k, v in remarks.items() if re.match(pat, k)}
    assert sorted(hits) == [0, 1, 2], sorted(remarks)
    for v, r in hits.items():
        assert _clean(r) and r["LDS Size"] == LDS, (v, r)
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"]) == PLAIN[v], (v, r)


@pytest.mark.parametrize("name,want", [("lf_vefftrue_cutvol", CUTVOL), ("lf_cut_volume_points", POINTS)])
def test_table_and_point_kernels(remarks, name, want):
    hits = [v for k, v in remarks.items() if re.match(r"_ZN2lf\d+%sE" % name, k)]
    assert len(hits) == 1, sorted(remarks)
    r = hits[0]
    print(name, r)
    assert _clean(r), r
    assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"], r["LDS Size"]) == want, r


def test_the_headers_use_no_atomics_and_no_inline_assembly_and_the_design_states_the_figures():
    for h in ("lf_vefftrue_cut.h", "lf_vefftrue_part_body.h"):
        src = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", h)).read()
        code = "\n".join(line.split("//")[0] for line in src.splitlines())
        assert "atomic" not in code.lower().replace("__atomic_acq_rel", "") and "asm" not in code, h
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.34" in design
    sec = design[design.index("### 3.34"):]
    for vgprs, sgprs, occ in list(PINNED_CUT.values()) + [CUTVOL[:3], POINTS[:3]]:
        assert re.search(r"\| *%d *\| *%d *\| *%d *\|" % (vgprs, sgprs, occ), sec), (vgprs, sgprs, occ)
    assert "1168" in sec and "256 MB" in sec
