"""Static guard on what the compiler makes of the Sinsemilla kernels (no GPU: hipcc -S cross-compiles gfx950; bench/tools/isa_histogram.py
does the parsing): the round loop of every kernel runs out of registers -- no scratch, no spill -- a property a source change can lose
silently while results stay bit-exact."""
import collections
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
        lines = ih.compile_s("sinsemilla.hip", td)
    fn = ih.functions(lines)
    names = list(fn)
    return lines, fn, dict(zip(ih.demangle(names), names))


# a round is 18 products (the trace's first pass: 21, its second: 32); VGPR ceilings: two waves per SIMD for the pass that emits
# the rows, four for the others
@pytest.mark.parametrize("kernel, vgprs, products", [
    ("sinsemilla_hash<false>", 128, 18), ("sinsemilla_merkle", 128, 18), ("sinsemilla_trace<false>", 128, 21), ("sinsemilla_trace<true>", 256, 32)])
def test_round_loops_run_out_of_registers(listing, kernel, vgprs, products):
    lines, fn, dem = listing
    hit = [d for d in dem if kernel in d][0]
    start, end = fn[dem[hit]]
    res, blocks = ih.resources(lines, start, end), ih.histogram(lines[start + 1:end])
    assert res["ScratchSize"] == 0 and res["NumAgprs"] == 0 and res["NumVgprs"] <= vgprs, res
    total = collections.Counter()
    for _, _, c in blocks:
        total.update(c)
    assert not any(op.startswith("scratch_") for op in total)
    # the round is inlined once per kernel: about 100 v_mad_u64_u32 per product (the inversion and the epilogue add theirs on top)
    assert products * 90 <= total["v_mad_u64_u32"] <= products * 100 + 900, total["v_mad_u64_u32"]
