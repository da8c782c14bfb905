"""Static guard on what the compiler makes of the kernels of range_check.hip (no GPU: hipcc -S cross-compiles gfx950;
bench/tools/isa_histogram.py reads the resource metadata): every kernel runs out of registers -- no scratch, no spill, no AGPR."""
import importlib.util
import os
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_histogram", os.path.join(ROOT, "bench", "tools", "isa_histogram.py"))
ih = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ih)


@pytest.fixture(scope="module")
def listing():
    if not os.path.exists(ih.HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        lines = ih.compile_s("range_check.hip", td)
    fn = ih.functions(lines)
    names = list(fn)
    return lines, fn, dict(zip(ih.demangle(names), names))


# 128 VGPRs of the 512-register file: four waves per SIMD.  Both kernels are one load, a barrel shift over eight registers and one
# multiplication; the shift indexes no register by a variable, which is what would send the element to scratch.
KERNELS = ["range_check_trace<0>", "range_check_trace<1>", "short_range_check_trace<0>", "short_range_check_trace<1>"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernels_run_out_of_registers(listing, kernel):
    lines, fn, dem = listing
    hit = [d for d in dem if "::" + kernel + "(" in d]
    assert len(hit) == 1, sorted(dem)
    start, end = fn[dem[hit[0]]]
    res = ih.resources(lines, start, end)
    assert res["ScratchSize"] == 0 and res["NumAgprs"] == 0 and res["NumVgprs"] <= 128, res


def test_every_kernel_is_covered(listing):
    _, fn, dem = listing
    assert len(dem) == len(fn) == len(KERNELS), sorted(dem)
