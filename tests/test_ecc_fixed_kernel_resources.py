"""Static guard on what the compiler makes of the fixed-base ECC kernels (no GPU: hipcc -S cross-compiles gfx950;
bench/tools/isa_histogram.py reads the resource metadata): every kernel runs out of registers -- no scratch, no spill, no AGPR -- and
stays on the occupancy step it was measured at."""
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
        lines = ih.compile_s("ecc_fixed.hip", td)
    fn = ih.functions(lines)
    names = list(fn)
    return lines, fn, dict(zip(ih.demangle(names), names))


# VGPR ceilings of the 512-register file: 64 is eight waves per SIMD, 128 four, 256 two.  The search, whose loop is one exponentiation,
# and the two small table kernels sit on eight; the product and the trace's first pass (the chain alone) on four; the pass that emits the
# rows, which ends on the complete addition's inversion, on two.
KERNELS = [("ecc_fixed_lagrange(", 64), ("ecc_fixed_search(", 64), ("ecc_fixed_roots(", 64), ("ecc_fixed_mul(", 128),
           ("ecc_fixed_trace<false>", 128), ("ecc_fixed_trace<true>", 256)]


@pytest.mark.parametrize("kernel, vgprs", KERNELS)
def test_kernels_run_out_of_registers(listing, kernel, vgprs):
    lines, fn, dem = listing
    hit = [d for d in dem if kernel in d][0]
    start, end = fn[dem[hit]]
    res = ih.resources(lines, start, end)
    assert res["ScratchSize"] == 0 and res["NumAgprs"] == 0 and res["NumVgprs"] <= vgprs, res


def test_every_kernel_is_covered(listing):
    _, _, dem = listing
    kernels = [d for d in dem if "ecc_fixed_" in d]
    assert len(kernels) == len(KERNELS), kernels
