"""Static guard on what the compiler makes of the ECC kernels (no GPU: hipcc -S cross-compiles gfx950; bench/tools/isa_histogram.py
reads the resource metadata): every kernel runs out of registers -- no scratch, no spill, no AGPR -- and stays on the occupancy step it
was measured at, a property a source change can lose silently while results stay bit-exact."""
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
        lines = ih.compile_s("ecc.hip", td)
    fn = ih.functions(lines)
    names = list(fn)
    return lines, fn, dict(zip(ih.demangle(names), names))


# VGPR ceilings of the 512-register file: 128 is four waves per SIMD, 168 three, 256 two.  The product lands on four; the trace's first
# pass (the chain alone, 136 registers: forcing four waves spills 36 bytes) on three; the pass that emits the rows, which also carries
# the row's inverses, and the complete additions with their inversion on two.
@pytest.mark.parametrize("kernel, vgprs", [("ecc_mul(", 128), ("ecc_mul_trace<false>", 168), ("ecc_mul_trace<true>", 256),
                                           ("ecc_mul_complete(", 256)])
def test_kernels_run_out_of_registers(listing, kernel, vgprs):
    lines, fn, dem = listing
    hit = [d for d in dem if kernel in d][0]
    start, end = fn[dem[hit]]
    res = ih.resources(lines, start, end)
    assert res["ScratchSize"] == 0 and res["NumAgprs"] == 0 and res["NumVgprs"] <= vgprs, res


def test_every_kernel_is_covered(listing):
    _, _, dem = listing
    kernels = [d for d in dem if "ecc_mul" in d]
    assert len(kernels) == 4, kernels
