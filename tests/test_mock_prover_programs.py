"""CPU-only: what halo2_amd.dev hands to the device, executed on Python integers.  The linked programs of
`dev.compile_programs` run through an interpreter of the poison-tracking bytecode as include/halo2_mi355x.h documents it
(h2_check_expressions_device), and the lookup expressions' values go through a restatement of the rank / pack / search scheme of
h2_lookup_check_device (csrc/mock_prover.hip); both must give what tests/mock_prover_model.py gives.  The kernels themselves are
compared with the same model in tests/test_gpu_mock_prover.py."""
import bisect

import pytest

import mock_prover_cases as cases
import mock_prover_model as model
import plonk_circuits as pc
from halo2_amd import dev, fields
from halo2_amd import evaluator as hev
from halo2_amd.evaluator import LAGRANGE, Evaluator
from oracle import plonk_api

FIELDS = [0, 1]
POISON = None


def _interpret(words, consts, polys, is_advice, n, usable, m):
    """One program at every row: a list of values, POISON where the result is poisoned."""
    out = []
    for row in range(n):
        stack, i = [], 0
        while i < len(words):
            op, arg = words[i] & 0xFF, words[i] >> 8
            i += 1
            if op == hev._POLY:
                shift = words[i] if words[i] < (1 << 31) else words[i] - (1 << 32)
                i += 1
                src = (row + shift) % n
                stack.append(POISON if is_advice[arg] and src >= usable else polys[arg][src])
            elif op == hev._CONST:
                stack.append(consts[arg])
            elif op == hev._SCALE:
                x = stack.pop()
                stack.append(0 if consts[arg] == 0 else POISON if x is POISON else x * consts[arg] % m)
            elif op in (hev._ADD, hev._MUL, hev._MULADD):
                b, a = stack.pop(), stack.pop()
                if op == hev._MULADD:                       # SCALE of the accumulator, then ADD
                    a = 0 if consts[arg] == 0 else POISON if a is POISON else a * consts[arg] % m
                if op == hev._MUL:
                    stack.append(a * b % m if a is not POISON and b is not POISON else 0 if a == 0 or b == 0 else POISON)
                else:
                    stack.append(POISON if a is POISON or b is POISON else (a + b) % m)
            else:
                raise AssertionError(f"opcode {op} is not part of a check program")
            assert len(stack) <= 9
        assert len(stack) == 1
        out.append(stack[0])
    return out


def _run_linked(linked, case, field):
    """Every program of a linked set at every row."""
    k, cs, fixed, advice, instance, _ = case
    n, m = 1 << k, fields.MODULUS[field]
    usable = n - (cs.blinding_factors + 1)
    prog, offsets, table, n_consts = linked
    consts = fields.from_limbs(table[:n_consts], field, True) if n_consts else []
    pad = lambda col: [int(v) % m for v in col] + [0] * (n - len(col))
    polys = [pad(c) for c in list(fixed) + list(advice) + list(instance)]
    is_advice = [0] * len(fixed) + [1] * len(advice) + [0] * len(instance)
    words = list(prog)
    return [_interpret(words[offsets[p]:offsets[p + 1]], consts, polys, is_advice, n, usable, m) for p in range(len(offsets) - 1)]


def _membership(inputs, tables, usable):
    """The scheme of h2_lookup_check_device on rows < usable: per component the rank in the sorted table column (POISON: one past the
    largest; an input value the column lacks: absent), seven ranks per packed key, a full key replaced by its own rank among the sorted
    packed table keys; a row fails when its final key is not among the table's."""
    ABSENT = 0xFFFFFFFF
    key_t, key_i = [()] * usable, [()] * usable

    def rank(sorted_keys, key, is_input):
        p = bisect.bisect_left(sorted_keys, key)
        return ABSENT if is_input and (p >= len(sorted_keys) or sorted_keys[p] != key) else p
    for c in range(len(inputs)):
        if len(key_t[0]) == 7:
            s = sorted(key_t)
            key_t = [(rank(s, k, False),) for k in key_t]
            key_i = [(rank(s, k, True),) for k in key_i]
        column = sorted(0 if v is POISON else v for v in tables[c][:usable])      # a poisoned cell is stored as 0 and sorted with the rest
        key_t = [k + (usable if v is POISON else rank(column, v, False),) for k, v in zip(key_t, tables[c][:usable])]
        key_i = [k + (usable if v is POISON else rank(column, v, True),) for k, v in zip(key_i, inputs[c][:usable])]
    have = set(key_t)
    return [r for r in range(usable) if key_i[r] not in have]


def _emulate(case, field):
    k, cs, fixed, advice, instance, mapping = case
    n = 1 << k
    usable = n - (cs.blinding_factors + 1)
    gates, lookups = dev.compile_programs(cs, k, field, Evaluator(LAGRANGE))
    failures = []
    for g, values in enumerate(_run_linked(gates, case, field) if gates else []):
        bad = [(r, ("ConstraintNotSatisfied", g, r)) for r, v in enumerate(values) if v is not POISON and v != 0]
        poisoned = [r for r, v in enumerate(values) if v is POISON]
        if poisoned:
            bad.append((poisoned[0], ("ConstraintPoisoned", g, len(poisoned), poisoned[0])))
        failures += [f for _, f in sorted(bad)]
    for l, (w, linked) in enumerate(lookups):
        values = _run_linked(linked, case, field)
        failures += [("Lookup", l, r) for r in _membership(values[:w], values[w:], usable)]
    return failures


def _model(case, field):
    got = model.verify(*case, fields.MODULUS[field])
    return [f[:3] if f[0] == "ConstraintNotSatisfied" else f for f in got if f[0] != "Permutation"]


@pytest.mark.parametrize("field", FIELDS)
def test_gate_programs_with_poison_tracking(field):
    m = fields.MODULUS[field]
    k, cs, fixed, advice, instance, mapping = cases.plonk_api_case(m)
    n = 1 << k
    assert _emulate((k, cs, fixed, advice, instance, mapping), field) == []
    for rows in ([0], [3], [n - 7], range(n)):
        on = [c if i != plonk_api.SF else [1 if r in rows else 0 for r in range(n)] for i, c in enumerate(fixed)]
        case = (k, cs, on, advice, instance, mapping)
        assert _emulate(case, field) == _model(case, field)
    assert _emulate(cases.doc_example_case(m), field) == [("ConstraintNotSatisfied", 0, 0)]
    for variant in ("full", "two_lookups", "gates_only"):
        for kind in ("gate", "copy", "lookup"):
            case = cases.variant_case(variant, m, 7, cases.seeded_faults(m, 7, kind, 10))
            assert _emulate(case, field) == _model(case, field)


@pytest.mark.parametrize("field", FIELDS)
def test_lookup_scheme_is_exact_on_tuples(field):
    m = fields.MODULUS[field]
    assert _emulate(cases.bad_lookup_case(m), field) == [("Lookup", 0, 3)]
    assert _emulate(cases.pair_lookup_case(m), field) == [("Lookup", 0, r) for r in range(58)]
    for case in (cases.rotated_lookup_case(m, False), cases.rotated_lookup_case(m, True), cases.wide_lookup_case(m),
                 cases.wide_lookup_case(m, faults=0), cases.wide_lookup_case(m, k=7, width=16, seed=5, faults=20)):
        assert _emulate(case, field) == _model(case, field)
    assert len(_emulate(cases.wide_lookup_case(m), field)) > 0


def test_linked_programs_share_one_constant_table():
    """dev._link: per-program constant indices are rebased onto the shared table; rotation words are left alone."""
    cs = pc.make_cs("full")
    cs.gates = [lambda q: q.advice(0, -1) * 3 + 5, lambda q: 7 * q.fixed(1, 2) - 11]
    (prog, offsets, table, n_consts), _ = dev.compile_programs(cs, 4, 0, Evaluator(LAGRANGE))
    consts = fields.from_limbs(table[:n_consts], 0, True)
    m = fields.MODULUS[0]
    assert list(offsets) == [0, 5, 11] and consts == [3, 5, 7, 11, m - 1]
    words = list(prog)
    assert words[0] == (hev._POLY | 6 << 8) and words[1] == 0xFFFFFFFF and words[5] == (hev._POLY | 1 << 8) and words[6] == 2
    used = [w >> 8 for i, w in enumerate(words) if (w & 0xFF) in (hev._CONST, hev._SCALE) and i not in (1, 6)]
    assert sorted(used) == list(range(n_consts))
