"""What the compiler made of veffd_partial_zmax (csrc/lf_veffdraws.h; hipcc -Rpass-analysis=kernel-resource-usage, no GPU
needed): no scratch, no spills, and the LDS the header comment states - 2 x MAXF x 2 KiB (Flim and c, [MAXF fields][256
lanes]) + 2 x 2 KiB (flux, s) + 1 KiB (field) + 32 z pieces in rows of 9 doubles: 40192 bytes for the 8-field instantiation
(four workgroups per CU, so the registers must allow four waves per SIMD: 128 VGPRs) and 72960 bytes for the 16-field one
(two workgroups); 48 VGPRs each.  veffd_partial itself keeps its figures."""
import pytest

import lf_isalib


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def _one(remarks, prefix):
    hits = {k: v for k, v in remarks.items() if k.startswith(prefix)}
    assert len(hits) == 1, (prefix, sorted(remarks))
    (name, r), = hits.items()
    print(name, r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    return r


@pytest.mark.parametrize("fcmin", [0, 1])
@pytest.mark.parametrize("maxf,wg_per_cu", [(8, 4), (16, 2)])
def test_zmax_kernel_uses_no_scratch_and_the_stated_lds(remarks, fcmin, maxf, wg_per_cu):
    r = _one(remarks, "_ZN2lf18veffd_partial_zmaxILb%dELi%dEEE" % (fcmin, maxf))
    lds = 2 * maxf * 256 * 8 + 2 * 256 * 8 + 256 * 4 + 32 * 9 * 8
    assert r["LDS Size"] == lds == {8: 40192, 16: 72960}[maxf], r
    assert 160 * 1024 // lds == wg_per_cu
    assert r["VGPRs"] == 48, r                        # the header's figure; <= 128: never the registers that limit the occupancy
    assert r["Occupancy"] == wg_per_cu, r             # 256 threads = one wave per SIMD and workgroup


@pytest.mark.parametrize("fcmin,vgprs", [(0, 32), (1, 78)])
def test_veffd_partial_is_unchanged(remarks, fcmin, vgprs):
    r = _one(remarks, "_ZN2lf13veffd_partialILb%dEEE" % fcmin)
    assert r["LDS Size"] == 37 * 1024 and r["VGPRs"] == vgprs and r["Occupancy"] == 4, r
