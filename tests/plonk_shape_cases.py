"""Shared by test_plonk_shape_case_coverage.py (CPU) and test_gpu_plonk_shapes.py: constraint systems in the lowered form halo2_amd/plonk.py
takes, one per SHAPE the prover and the verifiers branch on -- which rotations are queried, how many permutation columns of which kind fall
into how many sets, how many lookups of which width and degree, the degree (so the extended domain and the number of h pieces), the
blinding factors (so the usable rows and the permutation's omega^-(bf+1) opening point), the column counts, the curve and the number of
circuits in one proof.  Pure Python, deterministic, no generator: every circuit is written out with its row-by-row witness rule.

Layout rules every shape keeps:
* a gate that reads a rotated cell is multiplied by a fixed selector, switched on only where every row + rotation lies in [0, active):
  rows >= usable are overwritten with randomness by the prover (prover.rs:293-298);
* active = usable - 3: the last three usable rows (the pad, rows p0 p1 p2) carry no gate, so a copy constraint between pad cells can be broken
  without breaking a gate;
* a lookup input that reads a rotated cell is multiplied by a selector too, and its table holds 0.

`degree` and `blinding_factors` are not chosen: `_cs` derives them from the shape's gates, lookups and declared queries by the reference's
rules (ConstraintSystem::degree / blinding_factors, plonk/circuit.rs:1403-1431, :1435-1460; lookup::Argument::required_degree,
plonk/lookup.rs:25-75; permutation::Argument::required_degree, plonk/permutation.rs:26-59).  test_plonk_shape_case_coverage.py recomputes both with
its own probe, checks the declared query lists against the queries the expressions make, and holds every `covers` list to the shape's
structure."""
import random
from dataclasses import dataclass

import halo2_amd as h
from halo2_amd import fields
from halo2_amd.plonk import ConstraintSystem

VESTA, PALLAS = h.VESTA, h.PALLAS
PAD = 3
GENERATOR_SEED = 1300                        # co.generate_bases(curve, GENERATOR_SEED + k, n); w, u from seeds 60, 61 as test_gpu_plonk.py
RNG_SEED = 7700
VK_REPR = 0x0123456789ABCDEF ** 3

# what the issue's list names but the code under test rules out, with the reference line (filled in when a shape turns out to be one)
NOT_CASES = {}

VALUES = (
    "rot:advice{0,1,2}", "rot:advice{-1,0,1}", "rot:far", "rot:fixed!=0", "rot:instance@1", "rot:four",
    "bf:5", "bf:6", "bf:7",
    "perm:none", "perm:<chunk", "perm:=chunk", "perm:chunk+1", "perm:2chunks", "perm:deg3x4", "perm:fixed", "perm:instance",
    "perm:cycle-x-chunk", "perm:cycle-x-kind",
    "lookups:0", "lookups:1", "lookups:3", "lookup:width1", "lookup:width3", "lookup:rotated-input", "lookup:deg2-input",
    "lookup:advice-table", "lookup:heavy-repeats", "lookup:several-circuits",
    "degree:3", "degree:4", "degree:5", "degree:6", "degree:9",
    "cols:no-instance", "cols:two-instance-empty-full", "cols:unqueried", "cols:no-advice",
    "curve:vesta", "curve:pallas", "circuits:1", "circuits:2", "circuits:3", "k:4", "k:5", "k:6",
    "broken:gate", "broken:copy_inside", "broken:copy_across", "broken:public", "broken:lookup",
)


def modulus(curve):
    return fields.MODULUS[fields.CURVE_FIELDS[curve][1]]


# ---- the two reference rules ---------------------------------------------------------------------------------------------------------
class _Deg:
    """Expression::degree (plonk/circuit.rs:613-626): a query 1, a constant 0, a product the sum, a sum the maximum, a scaling nothing."""

    def __init__(self, d):
        self.d = d

    @staticmethod
    def of(v):
        return v.d if isinstance(v, _Deg) else 0

    def __add__(self, other):
        return _Deg(max(self.d, _Deg.of(other)))

    __radd__ = __sub__ = __rsub__ = __add__

    def __neg__(self):
        return self

    def __mul__(self, other):
        return _Deg(self.d + _Deg.of(other))

    __rmul__ = __mul__


class _DegCells:
    def fixed(self, col, rot=0):
        return _Deg(1)

    advice = instance = fixed


def _degree(gates, lookups):
    deg = lambda e: _Deg.of(e(_DegCells()))
    degree = 3                                                                            # permutation.required_degree(), :1406
    for ins, tabs in lookups:                                                             # lookup.rs:52-75
        degree = max(degree, 4, 2 + max([1] + [deg(e) for e in ins]) + max([1] + [deg(e) for e in tabs]))
    return max([degree, 1] + [deg(g) for g in gates])                                     # :1421-1430 (no minimum_degree is set)


def _blinding_factors(num_advice_columns, advice_queries):
    per_column = [sum(1 for c, _ in advice_queries if c == col) for col in range(num_advice_columns)]        # num_advice_queries
    return max(3, max(per_column, default=1)) + 2                                         # :1437-1459


def _cs(nf, na, ni, gates, aq, iq=(), fq=(), perm=(), lookups=()):
    assert len(set(aq)) == len(aq) and len(set(iq)) == len(iq) and len(set(fq)) == len(fq)
    return ConstraintSystem(num_fixed_columns=nf, num_advice_columns=na, num_instance_columns=ni, gates=list(gates), advice_queries=list(aq),
                            instance_queries=list(iq), fixed_queries=list(fq), permutation_columns=list(perm), lookups=list(lookups),
                            degree=_degree(gates, lookups), blinding_factors=_blinding_factors(na, aq))


# ---- a shape -----------------------------------------------------------------------------------------------------------------------
@dataclass
class Shape:
    name: str
    curve: int
    k: int
    cs: ConstraintSystem
    fixed: list                   # fixed columns, n integers each
    mapping: list                 # mapping[c][r] = (c', r'), c over cs.permutation_columns ([] when there are none)
    circuits: list                # [(advice columns, instance columns)]
    broken: dict                  # variant ("gate" | "copy_inside" | "copy_across" | "public" | "lookup") -> (circuit, "advice" | "instance", column, row, new value or None = +1)
    covers: tuple                 # the VALUES this shape is in the list for

    @property
    def n(self):
        return 1 << self.k

    @property
    def usable(self):
        return self.n - (self.cs.blinding_factors + 1)


def broken_circuits(shape, variant):
    """The shape's circuits with the one cell of `variant` changed."""
    ci, kind, col, row, new = shape.broken[variant]
    m = modulus(shape.curve)
    out = [([list(c) for c in adv], [list(c) for c in inst]) for adv, inst in shape.circuits]
    cells = out[ci][0 if kind == "advice" else 1][col]
    cells[row] = (cells[row] + 1) % m if new is None else new
    return out


class _Ties:
    """Copy constraints as classes of cells (position in permutation_columns, row); `mapping` walks each class as one cycle
    (permutation/keygen.rs:24-107 joins cycles the same way, in whatever order `copy` was called)."""

    def __init__(self, n_columns, n):
        self.n_columns, self.n, self.parent = n_columns, n, {}

    def _find(self, x):
        while self.parent.setdefault(x, x) != x:
            x = self.parent[x]
        return x

    def tie(self, *cells):
        for c in cells[1:]:
            self.parent[self._find(c)] = self._find(cells[0])

    def mapping(self):
        out = [[(c, r) for r in range(self.n)] for c in range(self.n_columns)]
        classes = {}
        for cell in sorted(self.parent):
            classes.setdefault(self._find(cell), []).append(cell)
        for cells in classes.values():
            for i, (c, r) in enumerate(cells):
                out[c][r] = cells[(i + 1) % len(cells)]
        return out


def _geometry(k, cs):
    n = 1 << k
    usable = n - (cs.blinding_factors + 1)
    active = usable - PAD
    return n, usable, active, (active, active + 1, active + 2)


def _zeros(count, n):
    return [[0] * n for _ in range(count)]


# ---- the shapes --------------------------------------------------------------------------------------------------------------------
def _fibonacci():
    """a(r+2) = a(r) + a(r+1) in one column; no permutation column, no lookup, no instance column; a second advice and a second fixed column
    that nothing queries.  The smallest size there is: n = 16, 10 usable rows."""
    SEL, A = 0, 0
    cs = _cs(2, 2, 0, [lambda q: q.fixed(SEL) * (q.advice(A, 2) - q.advice(A, 0) - q.advice(A, 1))],
             aq=[(A, 2), (A, 0), (A, 1)], fq=[(SEL, 0)])
    k = 4
    n, usable, _, _ = _geometry(k, cs)
    fixed = _zeros(2, n)
    a = [0] * n
    a[0], a[1] = 3, 4
    for r in range(usable - 2):
        fixed[SEL][r] = 1
        a[r + 2] = a[r] + a[r + 1]
    fixed[1] = [r + 1 for r in range(n)]
    return Shape("fibonacci", VESTA, k, cs, fixed, [], [([a, [7 * r + 3 for r in range(n)]], [])], {"gate": (0, "advice", A, 5, None)},
                 ("rot:advice{0,1,2}", "bf:5", "perm:none", "lookups:0", "degree:3", "cols:no-instance", "cols:unqueried", "curve:vesta",
                  "circuits:1", "k:4", "broken:gate"))


def _chain_of_four_sets():
    """c = a + b, the sum carried to the next row's a and b mirrored in d; a(0) is public: four permutation columns at degree 3, so four sets
    of one column and three chain links z_i(omega^0) = z_{i-1}(omega^last).  Every copy crosses a set boundary but the pad's d ~ d.  Two
    circuits with different public inputs."""
    (SEL, PUB), (A, B, C, D) = range(2), range(4)
    cs = _cs(2, 4, 1, [lambda q: q.fixed(SEL) * (q.advice(A) + q.advice(B) - q.advice(C)),
                       lambda q: q.fixed(PUB) * (q.advice(A) - q.instance(0))],
             aq=[(A, 0), (B, 0), (C, 0), (D, 0)], iq=[(0, 0)], fq=[(SEL, 0), (PUB, 0)], perm=[("advice", c) for c in range(4)])
    k = 4
    n, usable, active, (p0, p1, p2) = _geometry(k, cs)
    fixed = _zeros(2, n)
    fixed[PUB][0] = 1
    ties = _Ties(4, n)
    for r in range(active):
        fixed[SEL][r] = 1
        ties.tie((B, r), (D, r))
        if r + 1 < active:
            ties.tie((C, r), (A, r + 1))
    ties.tie((D, p0), (D, p1))
    ties.tie((A, p2), (D, p2))

    def witness(seed):
        a, b, c, d = _zeros(4, n)
        a[0] = seed
        for r in range(active):
            b[r] = d[r] = r + 2 + seed
            c[r] = a[r] + b[r]
            if r + 1 < active:
                a[r + 1] = c[r]
        d[p0] = d[p1] = 99 + seed
        a[p2] = d[p2] = 77 + seed
        return [a, b, c, d], [[seed]]
    return Shape("chain_of_four_sets", VESTA, k, cs, fixed, ties.mapping(), [witness(1), witness(2)],
                 {"gate": (1, "advice", C, 3, None), "copy_inside": (0, "advice", D, p1, None), "copy_across": (1, "advice", D, p2, None),
                  "public": (1, "instance", 0, 0, None)},
                 ("bf:5", "perm:deg3x4", "perm:cycle-x-chunk", "lookups:0", "degree:3", "curve:vesta", "circuits:2", "k:4",
                  "broken:gate", "broken:copy_inside", "broken:copy_across", "broken:public"))


def _window_sum():
    """b(r) = a(r-1) + a(r) + a(r+1); two of the sums are public through the instance column read one row ahead; a is looked up in a fixed
    table; b and the instance column are the permutation's one full chunk, with b(0) copied from instance(0).  Over Pallas."""
    (S0, S1, T), (A, B) = range(3), range(2)
    cs = _cs(3, 2, 1, [lambda q: q.fixed(S0) * (q.advice(B) - q.advice(A, -1) - q.advice(A, 0) - q.advice(A, 1)),
                       lambda q: q.fixed(S1) * (q.advice(B) - q.instance(0, 1))],
             aq=[(B, 0), (A, -1), (A, 0), (A, 1)], iq=[(0, 1), (0, 0)], fq=[(S0, 0), (S1, 0), (T, 0)],
             perm=[("advice", B), ("instance", 0)], lookups=[([lambda q: q.advice(A)], [lambda q: q.fixed(T)])])
    k = 5
    n, usable, active, (p0, p1, p2) = _geometry(k, cs)
    fixed = _zeros(3, n)
    a, b = _zeros(2, n)
    for r in range(usable):
        fixed[T][r] = 3 * (r % 8) + 1
    for r in range(usable):
        a[r] = fixed[T][(5 * r + 1) % 8]
    for r in range(1, active - 1):
        fixed[S0][r] = 1
        b[r] = a[r - 1] + a[r] + a[r + 1]
    instance = [12345, 0, 0, b[2], 0, b[4]]
    fixed[S1][2] = fixed[S1][4] = 1
    b[0] = instance[0]
    b[p0] = b[p1] = 55
    ties = _Ties(2, n)
    ties.tie((0, 0), (1, 0))
    ties.tie((0, p0), (0, p1))
    return Shape("window_sum", PALLAS, k, cs, fixed, ties.mapping(), [([a, b], [instance])],
                 {"gate": (0, "advice", B, 6, None), "copy_inside": (0, "advice", B, p1, None), "public": (0, "instance", 0, 3, None),
                  "lookup": (0, "advice", A, 0, 2)},
                 ("rot:advice{-1,0,1}", "rot:instance@1", "bf:5", "perm:=chunk", "perm:instance", "perm:cycle-x-kind", "lookups:1",
                  "lookup:width1", "degree:4", "curve:pallas", "circuits:1", "k:5", "broken:gate", "broken:copy_inside", "broken:public",
                  "broken:lookup"))


def _far_product():
    """p(r) = p(r-4) * a(r): a running product that looks four rows back; a(r) is the fixed column `const` one row AHEAD (a rotated fixed
    query); a selected a(r+1) is looked up (rotated input of degree 2, so degree 5); `const` and a are two permutation columns in a chunk
    of three, with a pad cell of a copied from const(3).  (The reference's `VirtualCells::query_fixed` of this version takes no rotation
    (plonk/circuit.rs:1500-1507); its prover and verifier open `fixed_queries` at whatever rotation they hold (prover.rs:642-653, :709-719,
    verifier.rs:326-337), and the lowered form here can state one.)"""
    (SEL, CONST, QL, T), (A, P) = range(4), range(2)
    cs = _cs(4, 2, 0, [lambda q: q.fixed(SEL) * (q.advice(P) - q.advice(P, -4) * q.advice(A)),
                       lambda q: q.fixed(SEL) * (q.advice(A) - q.fixed(CONST, 1))],
             aq=[(P, 0), (P, -4), (A, 0), (A, 1)], fq=[(SEL, 0), (CONST, 1), (QL, 0), (T, 0), (CONST, 0)],
             perm=[("fixed", CONST), ("advice", A)], lookups=[([lambda q: q.fixed(QL) * q.advice(A, 1)], [lambda q: q.fixed(T)])])
    k = 5
    m = modulus(VESTA)
    n, usable, active, (p0, p1, p2) = _geometry(k, cs)
    fixed = _zeros(4, n)
    a, p = _zeros(2, n)
    for r in range(usable):
        fixed[CONST][r] = r + 2
        fixed[T][r] = r
    p[:4] = [2, 3, 5, 7]
    for r in range(4, active - 1):
        fixed[SEL][r] = 1
        a[r] = fixed[CONST][r + 1]
        p[r] = p[r - 4] * a[r] % m
    for r in range(4, 11):
        fixed[QL][r] = 1                          # reads a(r+1) = r + 4, a table value
    a[p0] = fixed[CONST][3]
    a[p1] = a[p2] = 9
    ties = _Ties(2, n)
    ties.tie((0, 3), (1, p0))
    ties.tie((1, p1), (1, p2))
    return Shape("far_product", VESTA, k, cs, fixed, ties.mapping(), [([a, p], [])],
                 {"gate": (0, "advice", P, 9, None), "copy_inside": (0, "advice", A, p0, None), "lookup": (0, "advice", A, 6, 1000)},
                 ("rot:far", "rot:fixed!=0", "bf:5", "perm:<chunk", "perm:fixed", "perm:cycle-x-kind", "lookups:1", "lookup:width1",
                  "lookup:rotated-input", "lookup:deg2-input", "degree:5", "cols:no-instance", "curve:vesta", "circuits:1", "k:5",
                  "broken:gate", "broken:copy_inside", "broken:lookup"))


def _four_rotations():
    """a(r+3) = a(r) a(r+1) a(r+2): one column at four rotations, so six blinding factors and the opening point omega^-7; three permutation
    columns at degree 4: a full chunk {a, b} and a last set of one {c}; b mirrors a one row down (inside the set), c mirrors a (across)."""
    SEL, (A, B, C) = 0, range(3)
    cs = _cs(1, 3, 0, [lambda q: q.fixed(SEL) * (q.advice(A, 3) - q.advice(A, 0) * q.advice(A, 1) * q.advice(A, 2))],
             aq=[(A, 3), (A, 0), (A, 1), (A, 2), (B, 0), (C, 0)], fq=[(SEL, 0)], perm=[("advice", c) for c in range(3)])
    k = 5
    m = modulus(VESTA)
    n, usable, active, (p0, p1, p2) = _geometry(k, cs)
    fixed = _zeros(1, n)
    a, b, c = _zeros(3, n)
    a[:3] = [2, 3, 5]
    for r in range(active - 3):
        fixed[SEL][r] = 1
        a[r + 3] = a[r] * a[r + 1] * a[r + 2] % m
    ties = _Ties(3, n)
    for r in range(active):
        c[r] = a[r]
        ties.tie((C, r), (A, r))
        if r + 1 < active:
            b[r] = a[r + 1]
            ties.tie((B, r), (A, r + 1))
    b[p0] = b[p1] = 41
    a[p2] = c[p2] = 43
    ties.tie((B, p0), (B, p1))
    ties.tie((A, p2), (C, p2))
    return Shape("four_rotations", VESTA, k, cs, fixed, ties.mapping(), [([a, b, c], [])],
                 {"gate": (0, "advice", A, 7, None), "copy_inside": (0, "advice", B, p1, None), "copy_across": (0, "advice", C, p2, None)},
                 ("rot:four", "rot:far", "bf:6", "perm:chunk+1", "perm:cycle-x-chunk", "lookups:0", "degree:4", "cols:no-instance", "curve:vesta",
                  "circuits:1", "k:5", "broken:gate", "broken:copy_inside", "broken:copy_across"))


def _five_rotations():
    """b(r) = a(r-2) a(r-1) a(r) + a(r+1) + a(r+2): five rotations of one column, seven blinding factors (opening point omega^-8); four
    permutation columns at degree 4 are exactly two chunks; c mirrors b (across), d mirrors c one row down (inside).  Over Pallas."""
    SEL, (A, B, C, D) = 0, range(4)
    cs = _cs(1, 4, 0, [lambda q: q.fixed(SEL) * (q.advice(B) - q.advice(A, -2) * q.advice(A, -1) * q.advice(A, 0) - q.advice(A, 1) - q.advice(A, 2))],
             aq=[(B, 0), (A, -2), (A, -1), (A, 0), (A, 1), (A, 2), (C, 0), (D, 0)], fq=[(SEL, 0)], perm=[("advice", c) for c in range(4)])
    k = 5
    m = modulus(PALLAS)
    n, usable, active, (p0, p1, p2) = _geometry(k, cs)
    fixed = _zeros(1, n)
    a, b, c, d = _zeros(4, n)
    ties = _Ties(4, n)
    for r in range(active):
        a[r] = r * r + 3
        c[r] = r + 100
    for r in range(2, active - 2):
        fixed[SEL][r] = 1
        b[r] = c[r] = (a[r - 2] * a[r - 1] * a[r] + a[r + 1] + a[r + 2]) % m
        ties.tie((C, r), (B, r))
    for r in range(active - 1):
        d[r] = c[r + 1]
        ties.tie((D, r), (C, r + 1))
    a[p0] = b[p0] = 61
    b[p1] = d[p1] = 67
    ties.tie((A, p0), (B, p0))
    ties.tie((B, p1), (D, p1))
    return Shape("five_rotations", PALLAS, k, cs, fixed, ties.mapping(), [([a, b, c, d], [])],
                 {"gate": (0, "advice", B, 5, None), "copy_inside": (0, "advice", A, p0, None), "copy_across": (0, "advice", D, p1, None)},
                 ("rot:four", "bf:7", "perm:2chunks", "perm:cycle-x-chunk", "lookups:0", "degree:4", "cols:no-instance", "curve:pallas",
                  "circuits:1", "k:5", "broken:gate", "broken:copy_inside", "broken:copy_across"))


def _three_lookups():
    """e = a * b beside three lookups: a in t0; the tuple (a, b, c) in (t0, t1, t2); a^2 in w^2, where the table column w is ADVICE, tied cell by
    cell to the fixed t0 by the permutation (two columns in a chunk of four).  The last lookup has degree 2 on both sides: degree 6."""
    (SEL, T0, T1, T2), (A, B, C, W, E) = range(4), range(5)
    cs = _cs(4, 5, 0, [lambda q: q.fixed(SEL) * (q.advice(E) - q.advice(A) * q.advice(B))],
             aq=[(E, 0), (A, 0), (B, 0), (C, 0), (W, 0)], fq=[(SEL, 0), (T0, 0), (T1, 0), (T2, 0)], perm=[("advice", W), ("fixed", T0)],
             lookups=[([lambda q: q.advice(A)], [lambda q: q.fixed(T0)]),
                      ([lambda q: q.advice(A), lambda q: q.advice(B), lambda q: q.advice(C)],
                       [lambda q: q.fixed(T0), lambda q: q.fixed(T1), lambda q: q.fixed(T2)]),
                      ([lambda q: q.advice(A) * q.advice(A)], [lambda q: q.advice(W) * q.advice(W)])])
    k = 5
    n, usable, active, _ = _geometry(k, cs)
    fixed = _zeros(4, n)
    a, b, c, w, e = _zeros(5, n)
    ties = _Ties(2, n)
    for r in range(usable):
        t = r % 8 + 1
        fixed[T0][r], fixed[T1][r], fixed[T2][r] = t, t + 10, t * t
        w[r] = t
        ties.tie((0, r), (1, r))
    for r in range(usable):
        a[r] = fixed[T0][(3 * r + 1) % 8]
        b[r], c[r] = a[r] + 10, a[r] * a[r]
    for r in range(active):
        fixed[SEL][r] = 1
        e[r] = a[r] * b[r]
    return Shape("three_lookups", VESTA, k, cs, fixed, ties.mapping(), [([a, b, c, w, e], [])],
                 {"gate": (0, "advice", E, 4, None), "copy_inside": (0, "advice", W, 3, None), "lookup": (0, "advice", A, 2, 100)},
                 ("bf:5", "perm:<chunk", "perm:fixed", "perm:cycle-x-kind", "lookups:3", "lookup:width1", "lookup:width3", "lookup:deg2-input",
                  "lookup:advice-table", "degree:6", "cols:no-instance", "curve:vesta", "circuits:1", "k:5", "broken:gate", "broken:copy_inside",
                  "broken:lookup"))


def _pow8(x):
    x2 = x * x
    x4 = x2 * x2
    return x4 * x4


def _eighth_power():
    """b = a^8 behind a selector: a gate of degree 9, eight h pieces over an extended domain of 2^(k+3); three permutation columns in a chunk of
    seven; c mirrors b."""
    SEL, (A, B, C) = 0, range(3)
    cs = _cs(1, 3, 0, [lambda q: q.fixed(SEL) * (q.advice(B) - _pow8(q.advice(A)))],
             aq=[(B, 0), (A, 0), (C, 0)], fq=[(SEL, 0)], perm=[("advice", c) for c in range(3)])
    k = 4
    m = modulus(VESTA)
    n, usable, active, (p0, p1, p2) = _geometry(k, cs)
    fixed = _zeros(1, n)
    a, b, c = _zeros(3, n)
    ties = _Ties(3, n)
    for r in range(active):
        fixed[SEL][r] = 1
        a[r] = r + 2
        b[r] = c[r] = pow(a[r], 8, m)
        ties.tie((C, r), (B, r))
    a[p0] = c[p1] = 71
    ties.tie((A, p0), (C, p1))
    return Shape("eighth_power", VESTA, k, cs, fixed, ties.mapping(), [([a, b, c], [])],
                 {"gate": (0, "advice", B, 2, None), "copy_inside": (0, "advice", C, p1, None)},
                 ("bf:5", "perm:<chunk", "lookups:0", "degree:9", "cols:no-instance", "curve:vesta", "circuits:1", "k:4", "broken:gate",
                  "broken:copy_inside"))


def _two_instance_columns():
    """a = instance1 + instance0, with instance0 EMPTY and instance1 holding exactly `usable` values; instance1 and a are two permutation columns
    at degree 3 (two sets of one), the pad rows of a copied from instance1.  Three circuits, over Pallas."""
    SEL, A = 0, 0
    cs = _cs(1, 1, 2, [lambda q: q.fixed(SEL) * (q.advice(A) - q.instance(1) - q.instance(0))],
             aq=[(A, 0)], iq=[(1, 0), (0, 0)], fq=[(SEL, 0)], perm=[("instance", 1), ("advice", A)])
    k = 4
    n, usable, active, pads = _geometry(k, cs)
    fixed = _zeros(1, n)
    ties = _Ties(2, n)
    for r in range(active):
        fixed[SEL][r] = 1
    for r in pads:
        ties.tie((0, r), (1, r))

    def witness(seed):
        full = [100 * seed + r for r in range(usable)]
        return [full + [0] * (n - usable)], [[], full]
    return Shape("two_instance_columns", PALLAS, k, cs, fixed, ties.mapping(), [witness(1), witness(2), witness(3)],
                 {"public": (1, "instance", 1, 4, None), "copy_across": (2, "advice", A, pads[1], None)},
                 ("bf:5", "perm:2chunks", "perm:chunk+1", "perm:instance", "perm:cycle-x-chunk", "perm:cycle-x-kind", "lookups:0", "degree:3",
                  "cols:two-instance-empty-full", "curve:pallas", "circuits:3", "k:4", "broken:public", "broken:copy_across"))


def _no_advice():
    """No advice column at all: the instance column equals the fixed column `const` on the selected rows, and one pad cell of it is a copy of a
    pad cell of `const` (fixed and instance are the two permutation columns)."""
    SEL, CONST = 0, 1
    cs = _cs(2, 0, 1, [lambda q: q.fixed(SEL) * (q.instance(0) - q.fixed(CONST))],
             aq=[], iq=[(0, 0)], fq=[(SEL, 0), (CONST, 0)], perm=[("fixed", CONST), ("instance", 0)])
    k = 4
    n, usable, active, (p0, p1, p2) = _geometry(k, cs)
    fixed = _zeros(2, n)
    for r in range(active):
        fixed[SEL][r] = 1
        fixed[CONST][r] = r * r + 1
    fixed[CONST][p0] = 500
    instance = fixed[CONST][:active] + [0, 500]
    ties = _Ties(2, n)
    ties.tie((0, p0), (1, p1))
    return Shape("no_advice", VESTA, k, cs, fixed, ties.mapping(), [([], [instance])],
                 {"public": (0, "instance", 0, 2, None), "copy_across": (0, "instance", 0, p1, None)},
                 ("bf:5", "perm:2chunks", "perm:chunk+1", "perm:fixed", "perm:instance", "perm:cycle-x-chunk", "perm:cycle-x-kind", "lookups:0",
                  "degree:3", "cols:no-advice", "curve:vesta", "circuits:1", "k:4", "broken:public", "broken:copy_across"))


def _heavy_repeats():
    """No gate: a is looked up in a table of three distinct values, each about twenty times, and is 1 on nine rows of ten; all cells of a that
    hold 1 are one copy cycle, those that hold 2 another (one permutation column in a chunk of two).  n = 64, over Pallas."""
    T, A = 0, 0
    cs = _cs(1, 1, 0, [], aq=[(A, 0)], fq=[(T, 0)], perm=[("advice", A)], lookups=[([lambda q: q.advice(A)], [lambda q: q.fixed(T)])])
    k = 6
    n, usable, _, _ = _geometry(k, cs)
    fixed = _zeros(1, n)
    a = [0] * n
    ties = _Ties(1, n)
    for r in range(usable):
        fixed[T][r] = r % 3 + 1
        a[r] = 2 if r % 10 == 3 else 1
    a[usable - 1] = 3
    for v in (1, 2):
        ties.tie(*[(0, r) for r in range(usable) if a[r] == v])
    return Shape("heavy_repeats", PALLAS, k, cs, fixed, ties.mapping(), [([a], [])],
                 {"copy_inside": (0, "advice", A, 6, 2), "lookup": (0, "advice", A, 5, 4)},
                 ("bf:5", "perm:<chunk", "lookups:1", "lookup:width1", "lookup:heavy-repeats", "degree:4", "cols:no-instance", "curve:pallas",
                  "circuits:1", "k:6", "broken:copy_inside", "broken:lookup"))


def _squares_in_two_circuits():
    """b = a^2 with a looked up in a fixed table and b(0) public, in TWO circuits: the permuted columns of both circuits are committed before
    beta, the products of both after the permutation's, and the second circuit's evaluations follow the first's group by group.  The lookup
    variant breaks the SECOND circuit, after the first one's permuted columns are in the transcript.  Over Pallas, n = 16."""
    (SEL, T), (A, B) = range(2), range(2)
    cs = _cs(2, 2, 1, [lambda q: q.fixed(SEL) * (q.advice(B) - q.advice(A) * q.advice(A))],
             aq=[(B, 0), (A, 0)], iq=[(0, 0)], fq=[(SEL, 0), (T, 0)], perm=[("advice", B), ("instance", 0)],
             lookups=[([lambda q: q.advice(A)], [lambda q: q.fixed(T)])])
    k = 4
    n, usable, active, (p0, p1, p2) = _geometry(k, cs)
    fixed = _zeros(2, n)
    for r in range(usable):
        fixed[T][r] = r + 1
    for r in range(active):
        fixed[SEL][r] = 1
    ties = _Ties(2, n)
    ties.tie((0, 0), (1, 0))
    ties.tie((0, p0), (0, p1))

    def witness(seed):
        a, b = _zeros(2, n)
        for r in range(usable):
            a[r] = fixed[T][(r + seed) % 5]
        for r in range(active):
            b[r] = a[r] * a[r]
        b[p0] = b[p1] = 30 + seed
        return [a, b], [[b[0]]]
    return Shape("squares_in_two_circuits", PALLAS, k, cs, fixed, ties.mapping(), [witness(1), witness(2)],
                 {"gate": (1, "advice", B, 3, None), "copy_inside": (1, "advice", B, p1, None), "public": (0, "instance", 0, 0, None),
                  "lookup": (1, "advice", A, 4, 77)},
                 ("bf:5", "perm:=chunk", "perm:instance", "perm:cycle-x-kind", "lookups:1", "lookup:width1", "lookup:several-circuits", "degree:4",
                  "curve:pallas", "circuits:2", "k:4", "broken:gate", "broken:copy_inside", "broken:public", "broken:lookup"))


SHAPES = [f() for f in (_fibonacci, _chain_of_four_sets, _window_sum, _far_product, _four_rotations, _five_rotations, _three_lookups,
                        _eighth_power, _two_instance_columns, _no_advice, _heavy_repeats, _squares_in_two_circuits)]
BY_NAME = {s.name: s for s in SHAPES}


def value_table(shapes=None):
    """value -> names of the shapes that are in the list for it."""
    return {v: tuple(s.name for s in (SHAPES if shapes is None else shapes) if v in s.covers) for v in VALUES}


# ---- the proof's section map -------------------------------------------------------------------------------------------------------
def point_set_count(shape):
    """How many distinct point sets the multi-point opening groups the shape's queries into (poly/multiopen.rs:193-209): one evaluation each.
    A commitment's point set is the set of rotations it is opened at."""
    cs = shape.cs
    rotations = {}
    for kind, queries in (("instance", cs.instance_queries), ("advice", cs.advice_queries), ("fixed", cs.fixed_queries)):
        for col, rot in queries:
            rotations.setdefault((kind, col), set()).add(rot)
    n_sets = _n_sets(cs)
    last = -(cs.blinding_factors + 1)
    for i in range(n_sets):                                                               # permutation/prover.rs:389-433
        rotations[("z", i)] = {0, 1} | ({last} if i + 1 < n_sets else set())
    if cs.lookups:                                                                        # lookup/prover.rs:513-553
        rotations.update({"lookup z": {0, 1}, "lookup a'": {0, -1}, "lookup s'": {0}})
    rotations["sigma, h, random"] = {0}
    return len({frozenset(r) for r in rotations.values()})


def _n_sets(cs):
    return -(-len(cs.permutation_columns) // (cs.degree - 2))


def sections(shape):
    """[(name, first byte, end byte)] of the proof in transcript order (plonk/prover.rs:301-724, poly/multiopen/prover.rs:99-110,
    poly/commitment/prover.rs:95-150), from the shape alone; empty sections are left out.  Every element is 32 bytes."""
    cs, circuits = shape.cs, len(shape.circuits)
    n_sets, n_lookups = _n_sets(cs), len(cs.lookups)
    counts = [
        ("advice commitments", circuits * cs.num_advice_columns),
        ("permuted lookup commitments", circuits * 2 * n_lookups),
        ("permutation products", circuits * n_sets),
        ("lookup products", circuits * n_lookups),
        ("vanishing random commitment", 1),
        ("h pieces", cs.degree - 1),
        ("instance evaluations", circuits * len(cs.instance_queries)),
        ("advice evaluations", circuits * len(cs.advice_queries)),
        ("fixed evaluations", len(cs.fixed_queries)),
        ("vanishing evaluation", 1),
        ("permutation common evaluations", len(cs.permutation_columns)),
        ("permutation set evaluations", circuits * (3 * n_sets - 1) if n_sets else 0),
        ("lookup evaluations", circuits * 5 * n_lookups),
        ("multiopen commitment", 1),
        ("multiopen evaluations", point_set_count(shape)),
        ("opening blind commitment", 1),
        ("opening rounds", 2 * shape.k),
        ("opening final scalars", 2),
    ]
    out, pos = [], 0
    for name, count in counts:
        if count:
            out.append((name, pos, pos + 32 * count))
        pos += 32 * count
    return out


def section_flips(shape):
    """One seeded bit per section: [(section name, byte offset, bit mask)]."""
    rnd = random.Random("flip " + shape.name)
    return [(name, rnd.randrange(lo, hi), 1 << rnd.randrange(8)) for name, lo, hi in sections(shape)]


def section_at(shape, offset):
    return next((name for name, lo, hi in sections(shape) if lo <= offset < hi), "past the end")
