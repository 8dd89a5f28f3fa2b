"""What the compiler made of the library's device code, compiled ONCE per pytest process for every test that reads it
(test_*_resources.py, test_kernarg_bounds.py, test_mock_cpu.py, test_pt_cpu.py): the resource remarks per kernel
(hipcc -Rpass-analysis=kernel-resource-usage) and the assembly (-S) of csrc/lfmcmc.hip, from one run with the library's flags.
No GPU needed.  Test infrastructure only."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

from lumfuncmcmc_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lfmcmc.hip")


@functools.lru_cache(maxsize=None)
def _compile(src, emit):
    """One device-only hipcc run of `src`: (the remarks' text, what it wrote: the assembly text with emit "-S", else None).
    Cached on exactly these two arguments: the callers below always pass both."""
    hipcc = build.hipcc()
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "lf.s" if emit == "-S" else "lf.o")
        r = subprocess.run([hipcc] + build.CXXFLAGS + ["--cuda-device-only", emit, "-o", out, src,
                            "-Rpass-analysis=kernel-resource-usage"], stderr=subprocess.PIPE, stdout=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stderr.decode(), open(out).read() if emit == "-S" else None


def remarks(src=SRC, emit="-S"):
    """{mangled kernel name: {remark: int}}; emit "-c" assembles an object instead of writing the assembly (another unit's
    compile check)"""
    out = {}
    name = None
    for line in _compile(src, emit)[0].splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def asm(src=SRC):
    """the assembly text of the whole unit (the same run as remarks(src))"""
    return _compile(src, "-S")[1]
