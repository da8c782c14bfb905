"""Static guard on what the compiler makes of the running-sum fixed-base kernels (no GPU: hipcc -S cross-compiles gfx950;
bench/tools/isa_histogram.py reads the resource metadata): every kernel runs out of registers -- no scratch, no spill, no AGPR -- and
sits on no worse an occupancy step than the pass of ecc_fixed.hip's trace it was modelled on."""
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
        lines = ih.compile_s("ecc_fixed_sum.hip", td)
    fn = ih.functions(lines)
    names = list(fn)
    return lines, fn, dict(zip(ih.demangle(names), names))


# VGPR ceilings of the 512-register file: 128 is four waves per SIMD, 256 two.  Pass A (<false, .>) is the chain alone and sits where
# ecc_fixed_trace<false> does; pass B (<true, .>) emits the rows and ends on the complete addition's inversion, as ecc_fixed_trace<true>.
# The second template argument is the short form.
KERNELS = [("ecc_fixed_sum_trace<false, true>", 128), ("ecc_fixed_sum_trace<false, false>", 128),
           ("ecc_fixed_sum_trace<true, true>", 256), ("ecc_fixed_sum_trace<true, false>", 256)]


@pytest.mark.parametrize("kernel, vgprs", KERNELS)
def test_kernels_run_out_of_registers(listing, kernel, vgprs):
    lines, fn, dem = listing
    hit = [d for d in dem if kernel in d]
    assert len(hit) == 1, (kernel, list(dem))
    start, end = fn[dem[hit[0]]]
    res = ih.resources(lines, start, end)
    assert res["ScratchSize"] == 0 and res["NumAgprs"] == 0 and res["NumVgprs"] <= vgprs, res


def test_every_kernel_is_covered(listing):
    _, _, dem = listing
    kernels = [d for d in dem if "ecc_fixed_sum" in d]
    assert len(kernels) == len(KERNELS), kernels
