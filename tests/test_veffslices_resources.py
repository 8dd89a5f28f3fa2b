"""What the compiler made of the kernels of lf_veff_slices (csrc/lf_veffslices.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, the LDS the header's constants declare and its
comment states - veffs_partial 4096 doubles = 32768 bytes in each of its three instantiations, veffs_reduce 4096 counters =
16384 bytes - below 64 KB, and registers that allow the occupancy DESIGN.md section 3.36 states: five workgroups of
veffs_partial per CU, set by the LDS (5 x 32 KiB = 160 KiB), i.e. 20, 10 or 5 waves per CU - at most 5 per SIMD."""
import os
import re

import pytest

import lf_isalib

HEADER = os.path.join(lf_isalib.ROOT, "lumfuncmcmc_amd", "csrc", "lf_veffslices.h")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


@pytest.fixture(scope="module")
def consts():
    """the header's integer constants, and the bytes its comment states"""
    src = open(HEADER).read()
    c = {}
    for name, expr in re.findall(r"constexpr (?:unsigned )?int (VEFFS_\w+) = ([^;]+);", src):
        c[name] = int(eval(expr.rstrip("u"), {}, dict(c)))
    m = re.search(r"VEFFS_LDS_DOUBLES = (\d+) doubles = (\d+) bytes", src)
    r = re.search(r"veffs_reduce (\d+)\s+(?://\s*)?counters of 4 bytes = (\d+) bytes", src)
    assert m and r, "the header's comment no longer states the LDS sizes"
    c["stated_partial"] = (int(m.group(1)), int(m.group(2)))
    c["stated_reduce"] = (int(r.group(1)), int(r.group(2)))
    return c


def _one(remarks, prefix):
    hits = {k: v for k, v in remarks.items() if k.startswith(prefix)}
    assert len(hits) == 1, (prefix, sorted(k for k in remarks if "veffs" in k))
    (name, r), = hits.items()
    print(name, r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    return r


def _waves_by_registers(r):
    alloc = -(-(r["VGPRs"] + r.get("AGPRs", 0)) // 8) * 8
    return min(8, 512 // max(alloc, 8))


@pytest.mark.parametrize("nb", [16, 32, 64])
def test_partial_sums_kernel_resources(remarks, consts, nb):
    r = _one(remarks, "_ZN2lf13veffs_partialILi%dEEE" % nb)
    assert consts["stated_partial"] == (consts["VEFFS_LDS_DOUBLES"], consts["VEFFS_LDS_BYTES"]) == (4096, 32768)
    assert r["LDS Size"] == consts["VEFFS_LDS_BYTES"] == consts["VEFFS_LDS_DOUBLES"] * 8 and r["LDS Size"] < 64 * 1024, r
    # the stated occupancy: VEFFS_WG_PER_CU workgroups per CU by the LDS, and registers that do not lower it
    lanes = consts["VEFFS_LDS_DOUBLES"] // nb
    assert consts["VEFFS_WG_PER_CU"] == LDS_PER_CU // r["LDS Size"] == 5
    waves_per_simd = -(-consts["VEFFS_WG_PER_CU"] * (lanes // 64) // 4)
    assert _waves_by_registers(r) >= waves_per_simd and r["VGPRs"] <= 64, (r, waves_per_simd)
    assert consts["VEFFS_CHUNK"] % (lanes * consts["VEFFS_UNROLL"]) == 0


def test_python_constants_are_the_headers(consts):
    from lumfuncmcmc_amd import veff
    assert veff.SLICES_CHUNK == consts["VEFFS_CHUNK"] and veff.SLICES_PURPOSE == consts["VEFFS_PURPOSE"]
    assert veff.SLICES_MAX == consts["VEFFS_MAXSLICE"] == consts["VEFFS_MAXBIN"]


def test_reduce_kernel_resources(remarks, consts):
    r = _one(remarks, "_ZN2lf12veffs_reduceE")
    assert consts["stated_reduce"] == (consts["VEFFS_MAXSLICE"] * consts["VEFFS_MAXBIN"], consts["VEFFS_REDUCE_LDS_BYTES"])
    assert r["LDS Size"] == consts["VEFFS_REDUCE_LDS_BYTES"] == 16384 and r["LDS Size"] < 64 * 1024, r
    assert _waves_by_registers(r) == 8, r


def test_pack_kernel_resources(remarks):
    r = _one(remarks, "_ZN2lf10veffs_packE")
    assert r["LDS Size"] == 0, r
