"""TEST INFRASTRUCTURE ONLY.  `dev::MockProver::verify` (halo2_proofs/src/dev.rs:76-156, 576-904) restated on Python integers for
the lowered constraint systems of halo2_amd.plonk: gate and lookup expressions are callables over a `cells` object, columns are
integer lists.  The device checker (halo2_amd.dev) is compared against THIS, never the other way round.

Failures are plain tuples, in the order halo2_amd.dev documents:
    ("ConstraintNotSatisfied", gate_index, row, ((kind, column, rotation, value | None), ...))
    ("ConstraintPoisoned", gate_index, poisoned_rows, first_row)
    ("Lookup", lookup_index, row)
    ("Permutation", (kind, index), row)
"""
from __future__ import annotations


class Value:
    """dev.rs:86-91: Real(x) or Poison (x is None), over the field of modulus m."""
    __slots__ = ("x", "m")

    def __init__(self, x, m):
        self.x, self.m = x, m

    @property
    def poison(self) -> bool:
        return self.x is None

    def _of(self, other) -> "Value":
        # an integer is a constant: Expression::Constant evaluates to Value::Real (dev.rs:654), and `Value * F` (:144-156) treats its
        # scalar exactly as `Value * Real(scalar)` does (:126-142)
        return other if isinstance(other, Value) else Value(int(other) % self.m, self.m)

    def __neg__(self):                                        # dev.rs:104-113
        return Value(None if self.poison else -self.x % self.m, self.m)

    def __add__(self, other):                                 # dev.rs:115-124
        other = self._of(other)
        if self.poison or other.poison:
            return Value(None, self.m)
        return Value((self.x + other.x) % self.m, self.m)

    def __mul__(self, other):                                 # dev.rs:126-156
        other = self._of(other)
        if not self.poison and not other.poison:
            return Value(self.x * other.x % self.m, self.m)
        if (not self.poison and self.x == 0) or (not other.poison and other.x == 0):
            return Value(0, self.m)                           # poison times zero is unconstrained, not propagated (:132-138, :150-152)
        return Value(None, self.m)

    def __sub__(self, other):                                 # Expression's a - b is a + (-b)
        return self + (-self._of(other))

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, other):
        return self._of(other) - self

    def __eq__(self, other):                                  # derived Eq (:87): Poison equals Poison
        return isinstance(other, Value) and self.x == other.x

    def __hash__(self):
        return hash(self.x)

    def __repr__(self):
        return "Poison" if self.poison else f"Real({self.x:#x})"


class Cells:
    """util::load / load_instance at one row (dev.rs:650-663): rotations wrap modulo n; an advice cell in a row >= usable is
    Poison (:529-533), fixed and instance cells are Real (an instance column is zero past its values)."""

    def __init__(self, model, row):
        self.model, self.row = model, row

    def fixed(self, col, rot=0):
        return Value(self.model.fixed[col][(self.row + rot) % self.model.n], self.model.m)

    def instance(self, col, rot=0):
        return Value(self.model.instance[col][(self.row + rot) % self.model.n], self.model.m)

    def advice(self, col, rot=0):
        r = (self.row + rot) % self.model.n
        return Value(None if r >= self.model.usable else self.model.advice[col][r], self.model.m)


class _PlainCells:
    """The same loads as bare integers, for rows on which no queried advice cell can be a blinding row: there every value is Real
    and the algebra above is ordinary arithmetic modulo m (reduced by the caller).  A shortcut of this model, not of the semantics."""

    def __init__(self, model):
        self.model, self.row = model, 0

    def fixed(self, col, rot=0):
        return self.model.fixed[col][(self.row + rot) % self.model.n]

    def instance(self, col, rot=0):
        return self.model.instance[col][(self.row + rot) % self.model.n]

    def advice(self, col, rot=0):
        return self.model.advice[col][(self.row + rot) % self.model.n]


class _Recorder:
    def __init__(self):
        self.cells = []

    def _note(self, kind, col, rot):
        if (kind, col, rot) not in self.cells:
            self.cells.append((kind, col, rot))
        return 1

    def fixed(self, col, rot=0):
        return self._note("fixed", col, rot)

    def advice(self, col, rot=0):
        return self._note("advice", col, rot)

    def instance(self, col, rot=0):
        return self._note("instance", col, rot)


def queried_cells(expression):
    rec = _Recorder()
    expression(rec)
    return rec.cells


class MockProverModel:
    def __init__(self, k, cs, fixed, advice, instance, mapping, m):
        self.k, self.n, self.cs, self.m = k, 1 << k, cs, m
        self.usable = self.n - (cs.blinding_factors + 1)                          # dev.rs:517-533
        pad = lambda col: [int(v) % m for v in col] + [0] * (self.n - len(col))
        self.fixed, self.advice, self.instance = [pad(c) for c in fixed], [pad(c) for c in advice], [pad(c) for c in instance]
        self.mapping = mapping

    def _touches_blinding_rows(self, cells, row) -> bool:
        return any(kind == "advice" and (row + rot) % self.n >= self.usable for kind, _, rot in cells)

    def _evaluate(self, expression, cells, row, plain) -> Value:
        if self._touches_blinding_rows(cells, row):
            v = expression(Cells(self, row))
            return v if isinstance(v, Value) else Value(int(v) % self.m, self.m)
        plain.row = row
        return Value(int(expression(plain)) % self.m, self.m)

    def _cell(self, kind, col, row):
        """CellValue (dev.rs:76-84) for the permutation check: ("poison", column, row) is unique per cell."""
        if kind == "advice":
            return ("poison", col, row) if row >= self.usable else self.advice[col][row]
        return (self.fixed if kind == "fixed" else self.instance)[col][row]

    def verify(self):
        n, usable, cs = self.n, self.usable, self.cs
        plain = _PlainCells(self)
        failures = []
        # gates at every row (dev.rs:643-707)
        for g, gate in enumerate(cs.gates):
            cells = queried_cells(gate)
            per_gate, poisoned = [], []
            for row in range(n):
                v = self._evaluate(gate, cells, row, plain)
                if v.poison:
                    poisoned.append(row)
                elif v.x != 0:
                    at = Cells(self, row)
                    values = tuple((kind, col, rot, getattr(at, kind)(col, rot).x) for kind, col, rot in cells)       # util::cell_values
                    per_gate.append((row, ("ConstraintNotSatisfied", g, row, values)))
            if poisoned:                                                          # one per gate (the dedup of :892-901), at its first row
                per_gate.append((poisoned[0], ("ConstraintPoisoned", g, len(poisoned), poisoned[0])))
            failures += [f for _, f in sorted(per_gate, key=lambda t: t[0])]
        # lookups over the usable rows (dev.rs:709-833); the fill-row shortcut (:756-766) changes nothing and is left out
        for l, (ins, tabs) in enumerate(cs.lookups):
            assert len(ins) == len(tabs)                                          # :753
            in_cells, tab_cells = [queried_cells(e) for e in ins], [queried_cells(e) for e in tabs]
            table = {tuple(self._evaluate(e, c, row, plain) for e, c in zip(tabs, tab_cells)) for row in range(usable)}
            for row in range(usable):
                if tuple(self._evaluate(e, c, row, plain) for e, c in zip(ins, in_cells)) not in table:
                    failures.append(("Lookup", l, row))
        # copy constraints (dev.rs:835-881)
        for c, (kind, idx) in enumerate(cs.permutation_columns):
            for row in range(n):
                to = self.mapping[c][row]
                c2, r2 = (int(to) // n, int(to) % n) if not isinstance(to, (tuple, list)) else to
                kind2, idx2 = cs.permutation_columns[c2]
                if self._cell(kind, idx, row) != self._cell(kind2, idx2, r2):
                    failures.append(("Permutation", (kind, idx), row))
        return failures


def verify(k, cs, fixed, advice, instance, mapping, m):
    return MockProverModel(k, cs, fixed, advice, instance, mapping, m).verify()


def counts(failures):
    return {kind: sum(1 for f in failures if f[0] == kind) for kind in ("ConstraintNotSatisfied", "ConstraintPoisoned", "Lookup", "Permutation")}


def as_tuples(device_failures):
    """halo2_amd.dev failures in this model's form."""
    out = []
    for f in device_failures:
        name = type(f).__name__
        if name == "ConstraintNotSatisfied":
            out.append((name, f.gate_index, f.row, tuple(f.cell_values)))
        elif name == "ConstraintPoisoned":
            out.append((name, f.gate_index, f.rows, f.first_row))
        elif name == "Lookup":
            out.append((name, f.lookup_index, f.row))
        else:
            out.append((name, tuple(f.column), f.row))
    return out


def capped(failures, limit):
    """What verify(max_failures=limit) keeps: the first `limit` of each kind, order unchanged."""
    seen, out = {}, []
    for f in failures:
        seen[f[0]] = seen.get(f[0], 0) + 1
        if seen[f[0]] <= limit:
            out.append(f)
    return out
