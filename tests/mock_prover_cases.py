"""Shared by the CPU and GPU MockProver tests: small circuits in the lowered form (the reference's own MockProver examples among
them) and seeded faults for the witnesses of tests/plonk_circuits.py.  A case is (k, cs, fixed, advice, instance, mapping)."""
import random

import plonk_circuits as pc
from halo2_amd.plonk import ConstraintSystem
from oracle import plonk_api

import mock_prover_model as model


def plonk_api_case(m):
    """tests/plonk_api.rs at K = 5: the circuit the reference itself runs through MockProver (:438-442)."""
    cs = plonk_api.constraint_system(ConstraintSystem)
    fixed, mapping = plonk_api.keygen_columns(m)
    advice, instance = plonk_api.witness(m)
    return plonk_api.K, cs, fixed, advice, instance, mapping


def doc_example_case(m):
    """dev.rs:166-261: the buggy R1CS gate s * (a * b + c) with a = 2, b = 4, c = 8 in row 0; the selector is a fixed column."""
    k = 5
    n = 1 << k
    cs = ConstraintSystem(num_fixed_columns=1, num_advice_columns=3, num_instance_columns=0,
                          gates=[lambda q: q.fixed(0) * (q.advice(0) * q.advice(1) + q.advice(2))],
                          advice_queries=[(0, 0), (1, 0), (2, 0)], instance_queries=[], fixed_queries=[(0, 0)], degree=3, blinding_factors=5)
    col = lambda v: [v] + [0] * (n - 1)
    return k, cs, [col(1)], [col(2), col(4), col(8)], [], []


def bad_lookup_case(m):
    """dev.rs:1015-1140: K = 4, a doubling table 2, 4 .. 14 filled up with its first value, a = 2, 6, 4, 5 with the selector on;
    the input is q * a + (1 - q) * 2.  fixed: [q, table]."""
    k = 4
    n = 1 << k
    usable = n - 6
    table = [2 * i for i in range(1, 1 << (k - 1))]
    table = table + [table[0]] * (usable - len(table)) + [0] * (n - usable)
    q = [1, 1, 1, 1] + [0] * (n - 4)
    a = [2, 6, 4, 5] + [0] * (n - 4)
    cs = ConstraintSystem(num_fixed_columns=2, num_advice_columns=1, num_instance_columns=0, gates=[],
                          advice_queries=[(0, 0)], instance_queries=[], fixed_queries=[(0, 0), (1, 0)],
                          lookups=[([lambda c: c.fixed(0) * c.advice(0) + (1 - c.fixed(0)) * 2], [lambda c: c.fixed(1)])],
                          degree=4, blinding_factors=5)
    return k, cs, [q, table], [a], [], []


def pair_lookup_case(m, k=6):
    """(advice A, advice B) looked up in (SL, SL at rotation 1): every A value occurs in SL and every B value in the rotated SL, but
    never as that pair -- every usable row fails, which a per-column or rank-only check would miss."""
    n = 1 << k
    usable = n - 6
    sl = [r + 1 for r in range(n)]                                    # table tuples (r + 1, r + 2)
    a = [r + 1 for r in range(usable)] + [0] * (n - usable)
    b = [2 + (r + 1) % usable for r in range(usable)] + [0] * (n - usable)      # in 2 .. usable + 1, never r + 2
    cs = ConstraintSystem(num_fixed_columns=1, num_advice_columns=2, num_instance_columns=0, gates=[],
                          advice_queries=[(0, 0), (1, 0)], instance_queries=[], fixed_queries=[(0, 0), (0, 1)],
                          lookups=[([lambda c: c.advice(0), lambda c: c.advice(1)], [lambda c: c.fixed(0), lambda c: c.fixed(0, 1)])],
                          degree=4, blinding_factors=5)
    return k, cs, [sl], [a, b], [], []


def wide_lookup_case(m, k=8, width=9, seed=3, faults=12):
    """A lookup of `width` components (past one packed key of seven ranks): advice columns 0 .. width-1 in fixed columns
    0 .. width-1.  Table values come from a small set so that ranks repeat; some input rows get one component replaced by
    another value of the same column."""
    rnd = random.Random(seed)
    n = 1 << k
    usable = n - 6
    small = [rnd.randrange(m) for _ in range(5)]
    table = [[rnd.choice(small) for _ in range(usable)] + [0] * (n - usable) for _ in range(width)]
    picks = [rnd.randrange(usable) for _ in range(usable)]
    advice = [[table[c][picks[r]] for r in range(usable)] + [0] * (n - usable) for c in range(width)]
    for i, r in enumerate(rnd.sample(range(usable), faults)):
        c = (0, width - 1, 7, 6)[i % 4] % width
        advice[c][r] = rnd.choice([v for v in small if v != advice[c][r]])
    cs = ConstraintSystem(num_fixed_columns=width, num_advice_columns=width, num_instance_columns=0, gates=[],
                          advice_queries=[(c, 0) for c in range(width)], instance_queries=[], fixed_queries=[(c, 0) for c in range(width)],
                          lookups=[([(lambda q, c=c: q.advice(c)) for c in range(width)], [(lambda q, c=c: q.fixed(c)) for c in range(width)])],
                          degree=4, blinding_factors=5)
    return k, cs, table, advice, [], []


def rotated_lookup_case(m, poisoned_table, k=5):
    """The input advice(0) at rotation 1 reads a blinding row on the last usable row: Poison.  Against a fixed table nothing equals
    it; against the table advice(1) at rotation 1, whose last usable row is Poison too, it is found."""
    n = 1 << k
    usable = n - 6
    vals = [3 * r + 1 for r in range(n)]
    a = list(vals)
    t = list(vals)
    table = (lambda c: c.advice(1, 1)) if poisoned_table else (lambda c: c.fixed(0, 1))
    cs = ConstraintSystem(num_fixed_columns=1, num_advice_columns=2, num_instance_columns=0, gates=[],
                          advice_queries=[(0, 1), (1, 1)], instance_queries=[], fixed_queries=[(0, 1)],
                          lookups=[([lambda c: c.advice(0, 1)], [table])], degree=4, blinding_factors=5)
    return k, cs, [list(vals)], [a, t], [], []


_WITNESS = {}


def circuit_witness(m, k, seed=7):
    """plonk_circuits.make_witness for n = 2^k (cached: fixed, advice, mapping, instance)."""
    key = (m, k, seed)
    if key not in _WITNESS:
        n = 1 << k
        _WITNESS[key] = pc.make_witness(random.Random(seed), m, n, n - 6)
    fixed, advice, mapping, instance = _WITNESS[key]
    return fixed, [list(c) for c in advice], mapping, instance


def variant_case(variant, m, k, advice=None):
    fixed, adv, mapping, instance = circuit_witness(m, k)
    cs = pc.make_cs(variant)
    if variant == "gates_only":
        return k, cs, fixed, advice or adv, [], []
    return k, cs, fixed, advice or adv, instance, mapping


def fault_rows(rnd, usable, count):
    """Rows for `count` seeded faults: row 0 and the last usable row first."""
    rows = [0, usable - 1][:count]
    if count > len(rows):
        rows += rnd.sample(range(1, usable - 1), count - len(rows))
    return rows


def seeded_faults(m, k, kind, count, seed=11):
    """Advice columns of circuit_witness with `count` faults of one kind -- "gate" (an output value), "copy" (a copied b cell) or
    "lookup" (an a value outside the table) -- and, always, changed blinding rows of every advice column (never reported by
    themselves: no selector of these circuits reaches them)."""
    rnd = random.Random(seed * 1000 + count)
    _, (a, b, c), _, _ = circuit_witness(m, k)
    n = 1 << k
    usable = n - 6
    for col in (a, b, c):
        col[usable] = rnd.randrange(m)
        col[n - 1] = rnd.randrange(m)
    for r in fault_rows(rnd, usable, count):
        if kind == "gate":
            c[r] = (c[r] + 1) % m
        elif kind == "copy":
            b[r] = (b[r] + 1 + rnd.randrange(5)) % m
        else:
            a[r] = rnd.randrange(m)
    return [a, b, c]


def planted_faults(variant, m, k, gate_rows, copy_rows, lookup_rows):
    """Faults whose consequences follow from how make_witness builds its circuit; returns (advice, expected failures).
      gate_rows    r % 3 != 2: c[r] is in no copy cycle and no lookup, so c[r] + 1 breaks gate 0 at r and nothing else;
      copy_rows    r % 3 == 0, r > 0: b[r] is tied to c[r - 1]; b[r] + 1 with c[r] recomputed keeps the gate and breaks both cells;
      lookup_rows  r > 0: a[r] replaced by a value outside the table, c[r] recomputed (r % 3 != 2): every lookup fails at r, and the
                   cycle of equal `a` cells breaks at r and at the cell that points to it."""
    fixed, (a, b, c), mapping, _ = circuit_witness(m, k)
    n = 1 << k
    usable = n - 6
    full = variant != "gates_only"
    cs = pc.make_cs(variant)
    table = set(fixed[pc.SL][:usable])
    expected_gate, expected_lookup, expected_perm = [], [], set()
    recompute = lambda r: a[r] * b[r] % m if r % 2 else (a[r] + b[r]) % m
    for r in copy_rows:
        assert r % 3 == 0 and 0 < r < usable
        b[r] = (b[r] + 1) % m
        c[r] = recompute(r)
        expected_perm |= {(pc.B, r), (pc.C_, r - 1)}
    for r in lookup_rows:
        assert r % 3 != 2 and 0 < r < usable
        fresh = 5
        while fresh in table:
            fresh += 1
        a[r] = fresh
        c[r] = recompute(r)
        expected_lookup += [("Lookup", l, r) for l in range(len(cs.lookups))]
        pred = [r2 for r2 in range(usable) if mapping[pc.A][r2] == (pc.A, r)]
        if pred != [r]:
            expected_perm |= {(pc.A, r), (pc.A, pred[0])}
    for r in gate_rows:
        assert r % 3 != 2 and r < usable and r not in copy_rows and r not in lookup_rows
        c[r] = (c[r] + 1) % m
        cols = {"advice": [a, b, c], "fixed": fixed}
        cells = model.queried_cells(cs.gates[0])
        expected_gate.append(("ConstraintNotSatisfied", 0, r, tuple((kd, col, rot, cols[kd][col][(r + rot) % n]) for kd, col, rot in cells)))
    expected = sorted(expected_gate, key=lambda f: f[2])
    if full:
        expected += sorted(expected_lookup, key=lambda f: (f[1], f[2]))
        expected += [("Permutation", ("advice", col), r) for col, r in sorted(expected_perm)]
    return [a, b, c], expected
