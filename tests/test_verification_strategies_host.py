"""CPU-only checks of the batch-verification layer: argument validation of h2_ipa_s_combine / h2_ipa_s_combine_device before any
device work, the no-device error, BatchVerifier's bookkeeping, and a static guard on what hipcc makes of the s-combine kernel."""
import importlib.util
import os
import tempfile

import numpy as np
import pytest

import halo2_amd as h
from halo2_amd import _lib
from halo2_amd import batch as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(_lib.u64p)


def test_s_combine_argument_validation():
    lib = h.lib()
    ch, co, out = np.zeros((3 * 4, 4), np.uint64), np.zeros((3, 4), np.uint64), np.zeros((16, 4), np.uint64)
    dev_out = _lib.vp(1)                 # never dereferenced: every case below is refused before any device work
    host = lambda *a: lib.h2_ipa_s_combine(*a[:7], _p(out) if a[7] is None else a[7])
    device = lambda *a: lib.h2_ipa_s_combine_device(*a[:7], dev_out if a[7] is None else a[7], None)
    bad = [
        (2, 4, 3, _p(ch), _p(co), 1, 0, None),            # bad field
        (0, 4, 3, _p(ch), _p(co), 7, 0, None),            # bad form
        (0, 0, 3, _p(ch), _p(co), 1, 0, None),            # k = 0
        (0, 31, 3, _p(ch), _p(co), 1, 0, None),           # k > 30
        (0, 4, 0, _p(ch), _p(co), 1, 0, None),            # batch = 0
        (0, 4, 3, None, _p(co), 1, 0, None),              # null challenges
        (0, 4, 3, _p(ch), None, 1, 0, None),              # null coefficients
        (0, 4, 3, _p(ch), _p(co), 1, 2, None),            # accumulate not 0 / 1
    ]
    for args in bad:
        assert host(*args) == _lib.H2_ERR_ARGS, args
        assert device(*args) == _lib.H2_ERR_ARGS, args
    assert lib.h2_ipa_s_combine(0, 4, 3, _p(ch), _p(co), 1, 0, None) == _lib.H2_ERR_ARGS                 # null out
    assert lib.h2_ipa_s_combine_device(0, 4, 3, _p(ch), _p(co), 1, 0, None, None) == _lib.H2_ERR_ARGS    # null d_out
    with pytest.raises(ValueError):                                    # the wrapper checks shapes first
        h.ipa_s_combine(4, ch[:5], co, h.FP, out)
    with pytest.raises(ValueError):
        h.ipa_s_combine(4, ch, co, h.FP, np.zeros((8, 4), np.uint64))


def test_s_combine_fails_loudly_without_device():
    if h.lib().h2_device_count() > 0:
        pytest.skip("a GPU is present")
    ch, co = np.zeros((4, 4), np.uint64), np.zeros((1, 4), np.uint64)
    with pytest.raises(h.H2Error, match="no MI355X device|no HIP device"):
        h.ipa_s_combine(4, ch, co, h.FP, np.zeros((16, 4), np.uint64))


def test_batch_verifier_bookkeeping():
    bv = hb.BatchVerifier()
    assert bv.finalize(None, None) is True                            # empty: params.empty_msm().eval(), no device work
    bv.add_proof([[[1, 2]]], b"\x01")
    bv.add_proof([[[3]], [[4]]], bytearray(b"\x02\x03"))
    assert bv.items == [([[[1, 2]]], b"\x01"), ([[[3]], [[4]]], b"\x02\x03")]
    assert all(isinstance(p, bytes) for _, p in bv.items)


def test_weights_are_nonzero_and_seeded_weights_repeat():
    from halo2_amd import fields
    m = fields.MODULUS[h.FQ]
    w = hb.draw_weights(64, h.FQ)
    assert len(w) == 64 and all(0 < x < m for x in w) and len(set(w)) == 64

    def seeded():
        state = np.random.Generator(np.random.PCG64(7))

        def rng(count):
            out = state.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
            out[:, 3] &= np.uint64((1 << 62) - 1)
            return out
        return rng
    assert hb.draw_weights(5, h.FQ, seeded()) == hb.draw_weights(5, h.FQ, seeded())


def test_s_combine_kernel_resources():
    """s_combine<F>: no scratch for either field, and at most 160 VGPRs (129 when this guard was written: the eight accumulators and
    the doubling's live products stay in registers; three waves per SIMD by the register file)."""
    spec = importlib.util.spec_from_file_location("isa_histogram", os.path.join(ROOT, "bench", "tools", "isa_histogram.py"))
    ih = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ih)
    if not os.path.exists(ih.HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        lines = ih.compile_s("verify.hip", td)
    fn = ih.functions(lines)
    dem = dict(zip(ih.demangle(list(fn)), fn))
    for field in (0, 1):
        hit = [d for d in dem if d.startswith(f"void h2::s_combine<{field}>")]
        assert len(hit) == 1, list(dem)
        start, end = fn[dem[hit[0]]]
        res = ih.resources(lines, start, end)
        assert res["ScratchSize"] == 0 and res["NumAgprs"] == 0, res
        assert res["NumVgprs"] <= 160, res
