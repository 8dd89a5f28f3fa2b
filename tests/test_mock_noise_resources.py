"""What the compiler made of the kernels of the mocks' observation step (csrc/lf_mock_noise.h; hipcc
-Rpass-analysis=kernel-resource-usage, no GPU needed): lf_mock_draw_err and lf_mock_hist_err use no scratch and spill nothing,
and lf_mock_hist_err's LDS is at most lf_mock_hist's plus 1 KiB (the nodes and one field's sigma row).  The register figures
are recorded in DESIGN.md section 3.23, not pinned here."""
import re

import pytest

import lf_isalib


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


def _one(remarks, name):
    hits = [v for k, v in remarks.items() if re.match(r"_ZN2lf\d+%sE" % name, k)]
    assert len(hits) == 1, (name, sorted(remarks))
    print(name, hits[0])
    return hits[0]


@pytest.mark.parametrize("name", ["lf_mock_draw_err", "lf_mock_hist_err"])
def test_no_scratch_and_no_spills(remarks, name):
    r = _one(remarks, name)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r


def test_the_histogram_kernel_adds_at_most_one_kib_of_lds(remarks):
    old, new = _one(remarks, "lf_mock_hist"), _one(remarks, "lf_mock_hist_err")
    assert old["LDS Size"] > 0
    assert new["LDS Size"] <= old["LDS Size"] + 1024, (old["LDS Size"], new["LDS Size"])
    assert _one(remarks, "lf_mock_draw_err")["LDS Size"] == 0
