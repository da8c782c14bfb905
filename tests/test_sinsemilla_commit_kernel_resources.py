"""Static guard on what the compiler makes of the kernels of sinsemilla_commit.hip (no GPU: hipcc -S cross-compiles gfx950;
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
        lines = ih.compile_s("sinsemilla_commit.hip", td)
    fn = ih.functions(lines)
    names = list(fn)
    return lines, fn, dict(zip(ih.demangle(names), names))


# VGPR ceilings of the 512-register file, as the neighbours': 128 (four waves per SIMD) for the kernels that only run chains, 256 (two)
# for the passes that end on a lane's inversion and emit rows.  The fused commit is the exception: it holds the hash M (four elements, 32
# registers) beside the accumulator of the second chain and compiles to 138 registers, ten over the four-wave step; its ceiling is the
# three-wave step, 168.  Parking M in LDS across the 85 windows brings it to 111 registers and four waves and was measured beside this
# form: 12.73 ms against 12.70 for 2^20 commitments of 50 words, no difference -- the chains are bound by the multiplier, not by
# occupancy -- so the kernel keeps M in registers and uses no LDS.
KERNELS = [("sinsemilla_hash_from(", 128), ("sinsemilla_commit(", 168), ("sinsemilla_trace_from<false>", 128),
           ("sinsemilla_trace_from<true>", 256), ("ecc_add_trace(", 256)]


@pytest.mark.parametrize("kernel, vgprs", KERNELS)
def test_kernels_run_out_of_registers(listing, kernel, vgprs):
    lines, fn, dem = listing
    hit = [d for d in dem if kernel in d][0]
    start, end = fn[dem[hit]]
    res = ih.resources(lines, start, end)
    assert res["ScratchSize"] == 0 and res["NumAgprs"] == 0 and res["NumVgprs"] <= vgprs, res
    assert not any(line.split()[:1] and line.split()[0].startswith("scratch_") for line in lines[start + 1:end])


def test_every_kernel_is_covered(listing):
    _, fn, dem = listing
    assert len(dem) == len(fn) == len(KERNELS), sorted(dem)
