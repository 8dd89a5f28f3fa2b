"""The kernel-argument side of the launch, read from the generated code object (hipcc --cuda-device-only -S, no GPU needed):
the one-launch lf_free takes one 64-byte line of arguments (its block pointer and the FreeLaunch: lf_free.h), and every
kernel that warms its arguments (lf_math.h: warm_kernarg) loads nothing past the end of its kernarg segment - a scalar load
beyond it can fault the GPU when the segment ends at the end of the runtime's kernarg pool."""
import re

import pytest

import lf_isalib


@pytest.fixture(scope="module")
def code():
    text = lf_isalib.asm()
    kern = {}
    for m in re.finditer(r"^(_ZN2lf\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        kern[m.group(1)] = {"body": m.group(2)}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        if m.group(1) in kern:
            kern[m.group(1)]["kernarg"] = int(re.search(r"\.amdhsa_kernarg_size (\d+)", m.group(2)).group(1))
    assert kern and all("kernarg" in v for v in kern.values())
    return kern


@pytest.mark.parametrize("st", [2, 4, 8])
def test_the_one_launch_free_kernel_takes_one_line_of_arguments(code, st):
    names = [k for k in code if k.startswith("_ZN2lf7lf_freeILi%dELb0ELb1EEE" % st)]
    assert len(names) == 1, names
    assert "FreeBlock" in names[0] and "FreeLaunch" in names[0], names
    assert code[names[0]]["kernarg"] <= 64, code[names[0]]["kernarg"]


def _warm_offsets(body):
    """the offsets of warm_kernarg's ladder: the inline-asm block whose loads take the kernarg segment pointer"""
    offs = []
    for blk in re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", body, re.S):
        for m in re.finditer(r"s_load_dword s\d+, s\[\d+:\d+\], (0x[0-9a-f]+) \+ (0x[0-9a-f]+)", blk):
            offs.append(int(m.group(1), 16) + int(m.group(2), 16))
    return offs


def test_the_argument_warm_up_stays_inside_the_segment(code):
    warmed = {}
    for name, k in code.items():
        offs = _warm_offsets(k["body"])
        if offs:
            warmed[name] = (max(offs), k["kernarg"])
            # one load per 64-byte line, every line that holds an argument
            assert sorted(offs) == list(range(0, 64 * len(offs), 64)), (name, offs)
            assert max(offs) + 4 <= k["kernarg"], (name, max(offs), k["kernarg"])
    # the kernels known to call it: lf_free (all instantiations), lf_free_step, lf_pers, lf_pers_step, lf_main, lf_prepare, lf_finalize
    for prefix in ("_ZN2lf7lf_freeILi8ELb0ELb0EEE", "_ZN2lf7lf_freeILi8ELb0ELb1EEE", "_ZN2lf12lf_free_stepILi8EEE",
                   "_ZN2lf12lf_pers_stepILi2EEE", "_ZN2lf7lf_persILi1ELb1EEE"):
        assert any(n.startswith(prefix) for n in warmed), prefix
