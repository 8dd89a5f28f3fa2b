"""What the compiler made of lf_mock_hist2<P> (csrc/lf_mock_hist2.h; hipcc -Rpass-analysis=kernel-resource-usage, no GPU needed):
the three instantiations compile for gfx950 with no scratch and no spills, their static LDS is what the header declares, and
their registers allow at least the occupancy DESIGN.md section 3.35 states (two workgroups of 256 threads per CU, that is two
waves per SIMD)."""
import os
import re

import pytest

import lf_isalib

HEADER = os.path.join(os.path.dirname(lf_isalib.SRC), "lf_mock_hist2.h")
STATED_WORKGROUPS_PER_CU = 2


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def _declared_lds():
    """bytes per process (plain, noisy, cut) from the header's constants: the tile, the two edge arrays, the error model's
    nodes and sigma row, the counter of kept candidates (8 bytes with its alignment)"""
    h = open(HEADER).read() + open(os.path.join(os.path.dirname(HEADER), "lf_mock.h")).read() + \
        open(os.path.join(os.path.dirname(HEADER), "lf_mock_noise.h")).read()
    const = lambda n: int(re.search(r"constexpr int %s = (\d+);" % n, h).group(1))      # noqa: E731
    plain = 4 * const("MOCK_HIST2_TILE_WORDS") + 2 * 8 * (const("MOCK_MAX_BINS") + 2)
    noisy = plain + 2 * 8 * const("MOCK_MAX_NODES")
    return {0: plain, 1: noisy, 2: noisy + 8}


def test_hist2_uses_no_scratch_the_declared_lds_and_registers_for_the_stated_occupancy(remarks):
    hits = {k: v for k, v in remarks.items() if re.match(r"_ZN2lf\d+lf_mock_hist2ILi[012]E", k)}
    assert len(hits) == 3, sorted(remarks)                       # plain, noisy, cut
    lds = _declared_lds()
    text = open(HEADER).read()
    for name, r in hits.items():
        p = int(re.search(r"ILi([012])E", name).group(1))
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == lds[p], (name, r, lds[p])
        assert "%d B" % lds[p] in text, lds[p]                   # the header's comment states the same bytes
        assert r["LDS Size"] < 64 * 1024 and STATED_WORKGROUPS_PER_CU * r["LDS Size"] <= 160 * 1024
        # 256 threads are one wave per SIMD: workgroups per CU = waves per SIMD; 512 registers per lane and SIMD
        assert 512 // (8 * -(-(r["VGPRs"] + r["AGPRs"]) // 8)) >= STATED_WORKGROUPS_PER_CU, (name, r)
        assert r["Occupancy"] >= STATED_WORKGROUPS_PER_CU, (name, r)


def test_design_states_that_occupancy():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "### 3.35" in design
    assert "two workgroups per CU" in design[design.index("### 3.35"):]
