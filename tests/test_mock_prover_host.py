"""The host side of halo2_amd.dev and the argument validation of its three entry points (no GPU): which cells a lowered gate
queries, H2_ERR_ARGS for what the C ABI refuses before touching a device, H2_ERR_NODEV (no CPU fallback) for valid arguments
without one, and the ValueErrors of MockProver.run."""
import ctypes as C

import numpy as np
import pytest

import evaluator_cases as ec
import halo2_amd as h
import mock_prover_cases as cases
import mock_prover_model as model
from halo2_amd import _lib, dev
from halo2_amd.plonk import ConstraintSystem
from oracle import pasta as o
from oracle import plonk_api

vp = C.c_void_p
FAKE = 0x1000            # a non-null "device pointer": validation never dereferences it


def test_recording_cells_find_the_queried_cells():
    cs = plonk_api.constraint_system(ConstraintSystem)
    got = dev.queried_cells(cs.gates[0])
    assert got == model.queried_cells(cs.gates[0]) and len(got) == len(set(got)) == 10
    assert set(got) == {("advice", plonk_api.ADV_A, 0), ("advice", plonk_api.ADV_B, 0), ("advice", plonk_api.ADV_C, 0),
                        ("advice", plonk_api.ADV_D, 1), ("advice", plonk_api.ADV_E, -1), ("fixed", plonk_api.SA, 0), ("fixed", plonk_api.SB, 0),
                        ("fixed", plonk_api.SM, 0), ("fixed", plonk_api.SC, 0), ("fixed", plonk_api.SF, 0)}
    assert dev.queried_cells(cs.gates[1]) == [("fixed", plonk_api.SP, 0), ("advice", plonk_api.ADV_A, 0), ("instance", 0, 0)]
    with pytest.raises(AttributeError):
        dev.queried_cells(lambda q: q.selector(0))


def test_failures_are_small_frozen_values():
    f = dev.ConstraintNotSatisfied(0, 3, (("advice", 0, 0, 2),))
    assert f == dev.ConstraintNotSatisfied(0, 3, (("advice", 0, 0, 2),)) and f != dev.ConstraintNotSatisfied(0, 4, (("advice", 0, 0, 2),))
    with pytest.raises(Exception):
        f.row = 4
    assert dev.Lookup(1, 2) == dev.Lookup(1, 2) and dev.Permutation(("advice", 1), 6) != dev.Permutation(("advice", 2), 6)
    assert "row 3" in str(f) and "0x2" in str(f) and "unusable" in str(dev.ConstraintPoisoned(0, 2, 31))
    assert model.as_tuples([f, dev.ConstraintPoisoned(1, 2, 31), dev.Lookup(0, 3), dev.Permutation(("fixed", 0), 1)]) == [
        ("ConstraintNotSatisfied", 0, 3, (("advice", 0, 0, 2),)), ("ConstraintPoisoned", 1, 2, 31), ("Lookup", 0, 3), ("Permutation", ("fixed", 0), 1)]


def _expression_args(**over):
    """Valid arguments of h2_check_expressions_device for `polys[0] * polys[1] + consts[0]` over 16 rows; `over` replaces some."""
    prog = [1 | 0 << 8, 0, 1 | 1 << 8, 1, 5, 2 | 0 << 8, 4]
    a = dict(field=0, prog=prog, offsets=[0, len(prog)], n_programs=1, consts=np.ones((1, 4), np.uint64), n_consts=1, polys=[FAKE, FAKE],
             flags=[1, 0], n_polys=2, log_len=4, usable=10, nz=FAKE, po=FAKE, counts=FAKE, values=None)
    a.update(over)
    return a


def _check_expressions(**over):
    a = _expression_args(**over)
    prog = (C.c_uint32 * len(a["prog"]))(*a["prog"]) if a["prog"] is not None else None
    offsets = (C.c_size_t * len(a["offsets"]))(*a["offsets"]) if a["offsets"] is not None else None
    polys = (vp * len(a["polys"]))(*a["polys"]) if a["polys"] is not None else None
    flags = (C.c_uint8 * len(a["flags"]))(*a["flags"]) if a["flags"] is not None else None
    values = (vp * len(a["values"]))(*a["values"]) if a["values"] is not None else None
    consts = a["consts"].ctypes.data_as(_lib.u64p) if a["consts"] is not None else None
    return h.lib().h2_check_expressions_device(a["field"], prog, offsets, a["n_programs"], consts, a["n_consts"], polys, flags, a["n_polys"],
                                               a["log_len"], a["usable"], a["nz"], a["po"], a["counts"], values, None)


def _check_lookup(field=0, inputs=(FAKE,), tables=(FAKE,), w=1, n=16, usable=10, form=1, fail=FAKE, count=FAKE):
    arr = lambda ps: (vp * len(ps))(*ps) if ps is not None else None
    return h.lib().h2_lookup_check_device(field, arr(inputs), None, arr(tables), None, w, n, usable, form, fail, count, None)


def _check_permutation(field=0, cols=(FAKE, FAKE), flags=(1, 0), n_columns=2, mapping=FAKE, log_len=4, usable=10, form=1, fail=FAKE, counts=FAKE):
    ptrs = (vp * len(cols))(*cols) if cols is not None else None
    fl = (C.c_uint8 * len(flags))(*flags) if flags is not None else None
    return h.lib().h2_permutation_check_device(field, ptrs, fl, n_columns, mapping, log_len, usable, form, fail, counts, None)


def test_entry_points_refuse_bad_arguments():
    E = _lib.H2_ERR_ARGS
    assert _check_expressions(field=2) == E
    assert _check_expressions(prog=None) == E and _check_expressions(offsets=None) == E and _check_expressions(n_programs=0) == E
    assert _check_expressions(polys=None) == E and _check_expressions(flags=None) == E and _check_expressions(consts=None) == E
    assert _check_expressions(nz=None) == E and _check_expressions(po=None) == E and _check_expressions(counts=None) == E
    assert _check_expressions(usable=17) == E and _check_expressions(log_len=31) == E
    assert _check_expressions(polys=[FAKE, None]) == E                                   # a registered polynomial the program reads is null
    assert _check_expressions(values=[None]) == E
    assert _check_expressions(offsets=[0, 0]) == E and _check_expressions(offsets=[0, 4, 4], n_programs=2) == E
    # programs h2_evaluate_device refuses too: operand out of range, stack underflow, leftovers, a rotation larger than the vector (one of
    # exactly its length is the identity, as in the reference), an unknown opcode, a stack deeper than nine -- and the LINEAR node, which
    # lowered expressions do not have
    # -- and, one validator serving both entry points, every program of the evaluator's own refusal list (tests/evaluator_cases.py: the
    # entries that change nothing but the words of a Lagrange-basis call with two polynomials and one constant over 16 rows, as here)
    listed = [(name, over["words"]) for name, over in ec.REFUSALS if set(over) == {"words"}]
    assert len(listed) >= 18 and ec.REFUSAL_BASE["basis"] == ec.LAGRANGE and ec.REFUSAL_BASE["log_len"] == _expression_args()["log_len"]
    listed = [(name, [ec.word(ec.CONST, 0)] + [ec.word(ec.SCALE, 0)] * (1 << 20) if words == "2^20+1" else words) for name, words in listed]
    for name, bad in [(None, b) for b in ([1 | 2 << 8, 0], [2 | 1 << 8], [1, 0, 4], [1, 0, 1, 0], [1, 17], [1, (-17) & 0xFFFFFFFF], [9], [1], [3 | 0 << 8],
                                          [1, 0, 6 | 1 << 8], [1, 0, 1, 0, 7 | 1 << 8], [2] * 10 + [4] * 9)] + listed:
        assert _check_expressions(prog=bad, offsets=[0, len(bad)]) == E, name or bad
    assert _check_expressions(prog=[1, 0, 1, 0, 4, 9], offsets=[0, 5, 6], n_programs=2) == E     # the second of two programs is bad

    assert _check_lookup(field=5) == E and _check_lookup(form=3) == E and _check_lookup(w=0, inputs=(), tables=()) == E
    assert _check_lookup(inputs=None) == E and _check_lookup(tables=None) == E and _check_lookup(inputs=(None,)) == E
    assert _check_lookup(tables=(None,)) == E and _check_lookup(usable=17) == E and _check_lookup(n=0, usable=0) == E
    assert _check_lookup(fail=None) == E and _check_lookup(count=None) == E

    assert _check_permutation(field=-1) == E and _check_permutation(form=2) == E and _check_permutation(cols=None) == E
    assert _check_permutation(flags=None) == E and _check_permutation(n_columns=0) == E and _check_permutation(mapping=None) == E
    assert _check_permutation(cols=(FAKE, None)) == E and _check_permutation(usable=17) == E and _check_permutation(log_len=31) == E
    assert _check_permutation(fail=None) == E and _check_permutation(counts=None) == E


def test_entry_points_fail_loudly_without_a_device():
    if h.lib().h2_device_count() > 0:
        pytest.skip("a GPU is present")
    assert _check_expressions() == _lib.H2_ERR_NODEV
    assert _check_expressions(values=[FAKE]) == _lib.H2_ERR_NODEV
    for whole in ([1, 16], [1, (-16) & 0xFFFFFFFF]):                                      # |shift| == len passes the validation
        assert _check_expressions(prog=whole, offsets=[0, 2]) == _lib.H2_ERR_NODEV
    assert _check_lookup() == _lib.H2_ERR_NODEV
    assert _check_permutation() == _lib.H2_ERR_NODEV


def test_run_refuses_what_the_reference_refuses():
    m = o.P
    k, cs, fixed, advice, instance, mapping = cases.plonk_api_case(m)
    run = lambda **kw: dev.MockProver.run(**dict(dict(k=k, cs=cs, fixed_columns=fixed, advice_columns=advice, instance_columns=instance,
                                                      mapping=mapping, field=h.FP), **kw))
    with pytest.raises(ValueError, match="NotEnoughRowsAvailable"):
        run(k=2)                                                                          # 4 rows, 6 of them blinding
    with pytest.raises(ValueError, match="InstanceTooLarge"):
        run(instance_columns=[[1] * (32 - 6 + 1)])
    with pytest.raises(ValueError, match="longer than"):
        run(advice_columns=[advice[0] + [0]] + advice[1:])
    with pytest.raises(ValueError, match="number of columns"):
        run(advice_columns=advice[:-1])
    with pytest.raises(ValueError, match="number of columns"):
        run(fixed_columns=fixed + [fixed[0]])
    with pytest.raises(ValueError, match="number of columns"):
        run(instance_columns=[])
    with pytest.raises(ValueError, match="field"):
        run(field=7)
    with pytest.raises(TypeError):
        dev.MockProver()
