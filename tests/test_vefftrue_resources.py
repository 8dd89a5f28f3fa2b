"""What the compiler made of the kernels of the deconvolved 1/Veff points (csrc/lf_vefftrue.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, and the LDS, registers and occupancy that DESIGN.md
section 3.26 states - static, the node table of the largest wide class (144 nodes) and the row's constants (176 bytes): 2480 bytes
for lf_vefftrue_part in each of the three variants' instantiations; the edges and the four histograms are dynamic, sized by the
call's nbin (vefft_dyn_lds_bytes: checked here by the header's own formula); none for lf_vefftrue_reduce."""
import os
import re

import pytest

import lf_isalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXBIN, KMAX, ROW_BYTES = 1024, 144, 176
LDS = 2 * KMAX * 8 + ROW_BYTES                                        # static
DYN = lambda nbin: (((nbin + 2) & ~1) + 4 * nbin) * 8                # noqa: E731  (dynamic: edges, padded to an even count, four histograms)
# variant (LF_FREE 0, LF_FIXCOMP 1, LF_ZEVOL 2): VGPRs, SGPRs, occupancy (waves per SIMD)
PINNED = {0: (84, 100, 5), 1: (84, 100, 5), 2: (82, 100, 5)}


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def _clean(r):
    return r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0 and r["VGPRs"] <= 128


def test_vefftrue_part_uses_no_scratch_and_the_stated_lds(remarks):
    pat = r"_ZN2lf\d+lf_vefftrue_partILi([012])E"
    hits = {int(re.match(pat, k).group(1)): v for k, v in remarks.items() if re.match(pat, k)}
    assert sorted(hits) == [0, 1, 2], sorted(remarks)               # FREE, FIXCOMP, ZEVOL
    for v, r in hits.items():
        print(v, r)
        assert _clean(r), (v, r)
        assert r["LDS Size"] == LDS == 2480, (v, r)
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"]) == PINNED[v], (v, r)


def test_vefftrue_reduce_uses_no_scratch_and_no_lds(remarks):
    hits = [v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_vefftrue_reduceE", k)]
    assert len(hits) == 1, sorted(remarks)
    print(hits[0])
    assert _clean(hits[0]) and hits[0]["LDS Size"] == 0 and hits[0]["Occupancy"] == 8, hits[0]


def test_the_kernels_use_no_atomics_and_no_inline_assembly():
    src = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_vefftrue.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.lower().replace("__atomic_acq_rel", "") and "asm" not in code


def test_the_header_and_the_design_state_the_same_resources():
    hdr = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_vefftrue.h")).read()
    assert "VEFFT_LDS_BYTES = DECONV_WIDE_TABLE_BYTES + (int)sizeof(DeconvRow)" in hdr
    assert "return (nbin + 2) & ~1;" in hdr and "return (vefft_edge_slots(nbin) + 4 * nbin) * 8;" in hdr
    # workgroups of a CU's 160 KiB: five (the registers' limit) up to 757 bins, three at the largest nbin
    kib160 = 160 * 1024
    assert kib160 // (LDS + DYN(757)) == 5 and kib160 // (LDS + DYN(758)) == 4 and kib160 // (LDS + DYN(MAXBIN)) == 3
    assert DYN(50) == 2016 and DYN(MAXBIN) == 40976
    assert "constexpr int VEFFT_MAXBIN = %d;" % MAXBIN in hdr
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.26" in design
    sec = design[design.index("### 3.26"):]
    assert "2480 bytes" in sec and "40976" in sec
    for vgprs, sgprs, occ in PINNED.values():
        assert re.search(r"\| *%d *\| *%d *\| *%d *\|" % (vgprs, sgprs, occ), sec), (vgprs, sgprs, occ)
