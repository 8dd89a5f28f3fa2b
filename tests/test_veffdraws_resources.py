"""What the compiler made of the kernels of lf_veff_draws (csrc/lf_veffdraws.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): no scratch, no spills, and the LDS the header comment states -
veffd_partial 32 KiB of Flim [16 fields][256 lanes] + 2 x 2 KiB (flux, 1 / (pref0 vol)) + 1 KiB (field) = 37 KiB, which
lets four workgroups share a CU, so the registers must allow four waves per SIMD too (128 VGPRs); veffd_reduce none;
veffd_quant the 32 KiB of keys of the band kernels."""
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
def test_partial_sums_kernel_uses_no_scratch_and_37_kib_of_lds(remarks, fcmin):
    r = _one(remarks, "_ZN2lf13veffd_partialILb%dEEE" % fcmin)
    assert r["LDS Size"] == 16 * 256 * 8 + 2 * 256 * 8 + 256 * 4 == 37 * 1024, r
    assert r["VGPRs"] <= 128, r                       # four waves per SIMD, as many as the LDS admits


def test_bin_sums_kernel_uses_no_scratch_and_no_lds(remarks):
    r = _one(remarks, "_ZN2lf12veffd_reduceE")
    assert r["LDS Size"] == 0, r


def test_quantile_kernel_uses_no_scratch_and_the_keys_of_the_bands(remarks):
    r = _one(remarks, "_ZN2lf11veffd_quantE")
    assert r["LDS Size"] == 32 * 1024, r
