"""Running a `Circuit`: the front-end of halo2_proofs that `halo2_amd.plonk` leaves to its caller.

  * columns, `Expression` trees, `ConstraintSystem`      plonk/circuit.rs:20-1547
  * `Assigned` (a value with a deferred inversion)        plonk/assigned.rs
  * `Layouter` / `Region` / `Table`, `SimpleFloorPlanner` circuit.rs, circuit/layouter.rs, circuit/table_layouter.rs,
                                                          circuit/floor_planner/single_pass.rs
  * the copy-constraint assembly                          plonk/permutation/keygen.rs:16-103
  * selector compression                                  plonk/circuit.rs:1237-1343 (+ halo2_amd/compress_selectors.py)
  * `keygen_vk` / `keygen_pk` / `create_proof`            plonk/keygen.rs:188-380, plonk/prover.rs:35-341, plonk.rs:61-101

All of it is host bookkeeping except three loops over rows, which are device kernels: the deferred inversions of every assigned
cell (`arithmetic.assigned_to_field`), the selectors' conflict matrix and the combined selector columns (`selector_conflicts`,
`selector_combine`).  `lower(cs)` turns the trees into the callables `plonk` / `dev` / `verifier` take, so everything after
synthesis is the existing prover.  A key made here prints as the reference's `PinnedVerificationKey` (`vk.pinned()`), and its
`vk_repr` is the reference's `transcript_repr` (plonk.rs:75-101).

One extension: `Region.assign_advice_column` / `assign_fixed_column` assign a whole vector of rows in one call (a 2^20-row column
is otherwise a million Python calls) and `Region.enable_selector_rows` enables a selector on an array of offsets; they lay out
exactly as that many single calls would.

`synthesize(..., regions=True)` also records, per region and table, what dev::MockProver keeps of it (dev.rs:42-73, `RegionRecord`):
the layouters bracket their assignment pass with `Assembly.enter_region` / `exit_region` where the reference's do, and a bulk
assignment is recorded as one range, not as its cells."""
from __future__ import annotations

import hashlib
from dataclasses import dataclass

import numpy as np

from . import compress_selectors, fields
from . import plonk as _plonk


# ---- errors (plonk/error.rs) ---------------------------------------------------------------------------------------------------
class Error(Exception):
    pass


class NotEnoughRowsAvailable(Error):
    def __init__(self, current_k: int):
        super().__init__(f"NotEnoughRowsAvailable {{ current_k: {current_k} }}")
        self.current_k = current_k


class NotEnoughColumnsForConstants(Error):
    pass


class Synthesis(Error):
    pass


class BoundsFailure(Error):
    pass


class ColumnNotInPermutation(Error):
    pass


class TableError(Error):
    """plonk/error.rs TableError: kind is ColumnNotAssigned, UnevenColumnLengths, UsedColumn or OverwriteDefault."""

    def __init__(self, kind: str, detail=""):
        super().__init__(f"{kind}: {detail}")
        self.kind = kind


# ---- columns (circuit.rs:20-330) ----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Rotation:
    value: int = 0

    @staticmethod
    def cur():
        return Rotation(0)

    @staticmethod
    def prev():
        return Rotation(-1)

    @staticmethod
    def next():
        return Rotation(1)


def _rot(at) -> int:
    return at.value if isinstance(at, Rotation) else int(at)


ADVICE, FIXED, INSTANCE = "advice", "fixed", "instance"
_TYPE_NAME = {ADVICE: "Advice", FIXED: "Fixed", INSTANCE: "Instance"}


@dataclass(frozen=True)
class Column:
    kind: str
    index: int

    def debug(self) -> str:
        return f"Column {{ index: {self.index}, column_type: {_TYPE_NAME[self.kind]} }}"


@dataclass(frozen=True)
class Selector:
    index: int
    simple: bool = True

    def is_simple(self) -> bool:
        return self.simple

    def enable(self, region, offset: int) -> None:                            # circuit.rs:300-304
        region.enable_selector(self, offset)


@dataclass(frozen=True)
class TableColumn:
    inner: Column


def _hex(v: int) -> str:
    return "0x" + format(v, "064x")                                           # how pasta_curves prints a field element


# ---- Expression (circuit.rs:487-764) --------------------------------------------------------------------------------------------------
class Expression:
    """kind in Constant, Selector, Fixed, Advice, Instance, Negated, Sum, Product, Scaled.  Constant: (value,); Selector:
    (Selector,); the three queries: (query_index, column_index, rotation); Scaled: (expression, value)."""
    __slots__ = ("kind", "args")

    def __init__(self, kind: str, *args):
        self.kind, self.args = kind, args

    @staticmethod
    def constant(v: int) -> "Expression":
        return Expression("Constant", int(v))

    @staticmethod
    def _of(x) -> "Expression":
        return x if isinstance(x, Expression) else Expression.constant(x)

    def evaluate(self, constant, selector_column, fixed_column, advice_column, instance_column, negated, sum, product, scaled):    # :514-611
        """One callback per node kind.  The queries are passed as (query_index, column_index, rotation)."""
        rec = lambda e: e.evaluate(constant, selector_column, fixed_column, advice_column, instance_column, negated, sum, product, scaled)
        k, a = self.kind, self.args
        if k == "Constant":
            return constant(a[0])
        if k == "Selector":
            return selector_column(a[0])
        if k == "Fixed":
            return fixed_column(a)
        if k == "Advice":
            return advice_column(a)
        if k == "Instance":
            return instance_column(a)
        if k == "Negated":
            return negated(rec(a[0]))
        if k == "Sum":
            return sum(rec(a[0]), rec(a[1]))
        if k == "Product":
            return product(rec(a[0]), rec(a[1]))
        return scaled(rec(a[0]), a[1])

    def degree(self) -> int:                                                  # :614-626
        one = lambda _: 1
        return self.evaluate(lambda _: 0, one, one, one, one, lambda a: a, max, lambda a, b: a + b, lambda a, _: a)

    def square(self) -> "Expression":
        return self * self

    def contains_simple_selector(self) -> bool:                               # :634-646
        no = lambda _: False
        either = lambda a, b: a or b
        return self.evaluate(no, lambda s: s.is_simple(), no, no, no, lambda a: a, either, either, lambda a, _: a)

    def extract_simple_selector(self):                                        # :649-673
        def op(a, b):
            if a is not None and b is not None:
                raise ValueError("two simple selectors cannot be in the same expression")
            return a if a is not None else b
        none = lambda _: None
        return self.evaluate(none, lambda s: s if s.is_simple() else None, none, none, none, lambda a: a, op, op, lambda a, _: a)

    def debug(self, m: int | None = None) -> str:                             # :676-720, the `{:?}` form
        fe = lambda v: _hex(v % m if m else v)
        query = lambda name: lambda q: f"{name} {{ query_index: {q[0]}, column_index: {q[1]}, rotation: Rotation({q[2]}) }}"
        return self.evaluate(
            lambda c: f"Constant({fe(c)})", lambda s: f"Selector(Selector({s.index}, {'true' if s.simple else 'false'}))",
            query("Fixed"), query("Advice"), query("Instance"), lambda a: f"Negated({a})", lambda a, b: f"Sum({a}, {b})",
            lambda a, b: f"Product({a}, {b})", lambda a, f: f"Scaled({a}, {fe(f)})")

    def __neg__(self):                                                        # :722-727
        return Expression("Negated", self)

    def __add__(self, rhs):                                                   # :729-737
        rhs = Expression._of(rhs)
        if self.contains_simple_selector() or rhs.contains_simple_selector():
            raise ValueError("attempted to use a simple selector in an addition")
        return Expression("Sum", self, rhs)

    def __radd__(self, lhs):
        return Expression._of(lhs) + self

    def __sub__(self, rhs):                                                   # :739-747
        rhs = Expression._of(rhs)
        if self.contains_simple_selector() or rhs.contains_simple_selector():
            raise ValueError("attempted to use a simple selector in a subtraction")
        return Expression("Sum", self, -rhs)

    def __rsub__(self, lhs):
        return Expression._of(lhs) - self

    def __mul__(self, rhs):                                                   # :749-764: Mul<Expression> or Mul<F>
        if not isinstance(rhs, Expression):
            return Expression("Scaled", self, int(rhs))
        if self.contains_simple_selector() and rhs.contains_simple_selector():
            raise ValueError("attempted to multiply two expressions containing simple selectors")
        return Expression("Product", self, rhs)

    def __rmul__(self, lhs):
        return self * lhs


@dataclass
class Gate:                                                                   # :897-929
    name: str
    constraint_names: list
    polys: list
    queried_selectors: list
    queried_cells: list


class VirtualCells:                                                           # :1478-1547
    def __init__(self, meta: "ConstraintSystem"):
        self.meta, self.queried_selectors, self.queried_cells = meta, [], []

    def query_selector(self, selector: Selector) -> Expression:
        self.queried_selectors.append(selector)
        return Expression("Selector", selector)

    def query_fixed(self, column: Column) -> Expression:
        self.queried_cells.append((column, 0))
        return Expression("Fixed", self.meta._query_fixed_index(column), column.index, 0)

    def query_advice(self, column: Column, at=0) -> Expression:
        at = _rot(at)
        self.queried_cells.append((column, at))
        return Expression("Advice", self.meta._query_advice_index(column, at), column.index, at)

    def query_instance(self, column: Column, at=0) -> Expression:
        at = _rot(at)
        self.queried_cells.append((column, at))
        return Expression("Instance", self.meta._query_instance_index(column, at), column.index, at)

    def query_any(self, column: Column, at=0) -> Expression:
        if column.kind == ADVICE:
            return self.query_advice(column, at)
        if column.kind == FIXED:
            if _rot(at) != 0:
                raise ValueError("Fixed columns can only be queried at the current rotation")
            return self.query_fixed(column)
        return self.query_instance(column, at)


class ConstraintSystem:
    """plonk::ConstraintSystem (:934-1473).  `modulus` is only needed to print constants (`pinned`)."""

    def __init__(self, modulus: int | None = None):
        self.modulus = modulus
        self.num_fixed_columns = self.num_advice_columns = self.num_instance_columns = self.num_selectors = 0
        self.selector_map, self.gates = [], []
        self.advice_queries, self.instance_queries, self.fixed_queries = [], [], []      # (Column, rotation)
        self.num_advice_queries = []
        self.permutation_columns, self.lookups, self.constants = [], [], []              # lookups: (inputs, tables)
        self.minimum_degree = None

    # columns (:1349-1399)
    def selector(self) -> Selector:
        self.num_selectors += 1
        return Selector(self.num_selectors - 1, True)

    def complex_selector(self) -> Selector:
        self.num_selectors += 1
        return Selector(self.num_selectors - 1, False)

    def fixed_column(self) -> Column:
        self.num_fixed_columns += 1
        return Column(FIXED, self.num_fixed_columns - 1)

    def lookup_table_column(self) -> TableColumn:
        return TableColumn(self.fixed_column())

    def advice_column(self) -> Column:
        self.num_advice_columns += 1
        self.num_advice_queries.append(0)
        return Column(ADVICE, self.num_advice_columns - 1)

    def instance_column(self) -> Column:
        self.num_instance_columns += 1
        return Column(INSTANCE, self.num_instance_columns - 1)

    def enable_constant(self, column: Column) -> None:                        # :1043-1048
        if column not in self.constants:
            self.constants.append(column)
            self.enable_equality(column)

    def enable_equality(self, column) -> None:                                # :1051-1055
        column = column.inner if isinstance(column, TableColumn) else column
        self._query_any_index(column, 0)
        if column not in self.permutation_columns:
            self.permutation_columns.append(column)

    # queries (:1086-1140)
    @staticmethod
    def _index(queries, entry) -> int:
        if entry in queries:
            return queries.index(entry)
        queries.append(entry)
        return len(queries) - 1

    def _query_fixed_index(self, column: Column) -> int:
        return self._index(self.fixed_queries, (column, 0))

    def _query_advice_index(self, column: Column, at: int) -> int:
        before = len(self.advice_queries)
        index = self._index(self.advice_queries, (column, at))
        if len(self.advice_queries) != before:
            self.num_advice_queries[column.index] += 1
        return index

    def _query_instance_index(self, column: Column, at: int) -> int:
        return self._index(self.instance_queries, (column, at))

    def _query_any_index(self, column: Column, at: int) -> int:
        if column.kind == ADVICE:
            return self._query_advice_index(column, at)
        if column.kind == FIXED:
            return self._query_fixed_index(column)
        return self._query_instance_index(column, at)

    def lookup(self, table_map) -> int:                                       # :1061-1084
        cells = VirtualCells(self)
        inputs, tables = [], []
        for pair in table_map(cells):
            expression, table = pair
            if not isinstance(table, TableColumn):
                raise TypeError("a lookup maps an expression to a TableColumn")
            expression = Expression._of(expression)
            if expression.contains_simple_selector():
                raise ValueError("expression containing simple selector supplied to lookup argument")
            inputs.append(expression)
            tables.append(cells.query_fixed(table.inner))
        self.lookups.append((inputs, tables))
        return len(self.lookups) - 1

    def set_minimum_degree(self, degree: int) -> None:
        self.minimum_degree = degree

    def create_gate(self, name: str, constraints) -> None:                    # :1200-1228
        cells = VirtualCells(self)
        names, polys = [], []
        for c in constraints(cells):
            cname, poly = c if isinstance(c, tuple) else ("", c)
            names.append(cname)
            polys.append(Expression._of(poly))
        if not polys:
            raise ValueError("Gates must contain at least one constraint.")
        self.gates.append(Gate(name, names, polys, cells.queried_selectors, cells.queried_cells))

    def polynomials(self) -> list:
        return [p for g in self.gates for p in g.polys]

    def degree(self) -> int:                                                  # :1403-1431
        degree = 3                                                            # permutation::Argument::required_degree
        for inputs, tables in self.lookups:                                   # lookup::Argument::required_degree (lookup.rs:25-71)
            degree = max(degree, 4, 2 + max([1] + [e.degree() for e in inputs]) + max([1] + [e.degree() for e in tables]))
        degree = max([degree] + [p.degree() for p in self.polynomials()])
        return max(degree, self.minimum_degree or 1)

    def blinding_factors(self) -> int:                                        # :1435-1460
        return max(3, max(self.num_advice_queries, default=1)) + 2

    def minimum_rows(self) -> int:                                            # :1464-1472
        return self.blinding_factors() + 3

    def pinned(self) -> str:
        """`format!("{:?}", cs.pinned())` (:971-1040)."""
        m = self.modulus
        exprs = lambda es: "[" + ", ".join(e.debug(m) for e in es) + "]"
        queries = lambda qs: "[" + ", ".join(f"({c.debug()}, Rotation({r}))" for c, r in qs) + "]"
        columns = lambda cs_: "[" + ", ".join(c.debug() for c in cs_) + "]"
        lookups = "[" + ", ".join(f"Argument {{ input_expressions: {exprs(i)}, table_expressions: {exprs(t)} }}" for i, t in self.lookups) + "]"
        minimum = "None" if self.minimum_degree is None else f"Some({self.minimum_degree})"
        return ("PinnedConstraintSystem { "
                f"num_fixed_columns: {self.num_fixed_columns}, num_advice_columns: {self.num_advice_columns}, "
                f"num_instance_columns: {self.num_instance_columns}, num_selectors: {self.num_selectors}, "
                f"gates: {exprs(self.polynomials())}, advice_queries: {queries(self.advice_queries)}, "
                f"instance_queries: {queries(self.instance_queries)}, fixed_queries: {queries(self.fixed_queries)}, "
                f"permutation: Argument {{ columns: {columns(self.permutation_columns)} }}, lookups: {lookups}, "
                f"constants: {columns(self.constants)}, minimum_degree: {minimum} }}")

    def selector_degrees(self) -> list:                                       # :1246-1251
        degrees = [0] * self.num_selectors
        for poly in self.polynomials():
            s = poly.extract_simple_selector()
            if s is not None:
                degrees[s.index] = max(degrees[s.index], poly.degree())
        return degrees

    def compress_selectors(self, conflicts):
        """:1237-1343 given the conflict matrix (conflicts[i][j]) instead of the activations.  Substitutes in place; returns the
        combinations `compress_selectors.process` made, (selector, root) pairs per new fixed column in allocation order."""
        new_columns = []

        def allocate():
            column = self.fixed_column()
            new_columns.append(column)
            return Expression("Fixed", self._query_fixed_index(column), column.index, 0)
        descriptions = [compress_selectors.SelectorDescription(i, d) for i, d in enumerate(self.selector_degrees())]
        combinations, assignments = compress_selectors.process(descriptions, conflicts, self.degree(), allocate)
        replacements = [None] * self.num_selectors
        self.selector_map = [None] * self.num_selectors
        for a in assignments:
            replacements[a.selector] = a.expression
            self.selector_map[a.selector] = new_columns[a.combination_index]

        def replace(e, must_be_nonsimple):                                    # :1299-1324
            def sel(s):
                if must_be_nonsimple and s.is_simple():
                    raise AssertionError("a simple selector in a lookup")
                return replacements[s.index]
            leaf = lambda kind: lambda q: Expression(kind, *q)
            return e.evaluate(Expression.constant, sel, leaf("Fixed"), leaf("Advice"), leaf("Instance"), lambda a: -a,
                              lambda a, b: a + b, lambda a, b: a * b, lambda a, f: a * f)
        for g in self.gates:
            g.polys = [replace(p, False) for p in g.polys]
        self.lookups = [([replace(e, True) for e in i], [replace(e, True) for e in t]) for i, t in self.lookups]
        return combinations


def lower(cs: ConstraintSystem, modulus: int | None = None) -> _plonk.ConstraintSystem:
    """The trees as the callables `plonk.create_proof`, `dev.MockProver.run` and `verifier.verify_proof` take.  Selectors must have
    been compressed away."""
    m = modulus or cs.modulus
    red = (lambda v: v % m) if m else (lambda v: v)

    def callable_of(e):
        def selector(_):
            raise ValueError("lower: compress the selectors first")
        return lambda cells: e.evaluate(
            red, selector, lambda q: cells.fixed(q[1], q[2]), lambda q: cells.advice(q[1], q[2]), lambda q: cells.instance(q[1], q[2]),
            lambda a: -a, lambda a, b: a + b, lambda a, b: a * b, lambda a, f: a * red(f))
    plain = lambda qs: [(c.index, r) for c, r in qs]
    return _plonk.ConstraintSystem(
        num_fixed_columns=cs.num_fixed_columns, num_advice_columns=cs.num_advice_columns, num_instance_columns=cs.num_instance_columns,
        gates=[callable_of(p) for p in cs.polynomials()], advice_queries=plain(cs.advice_queries),
        instance_queries=plain(cs.instance_queries), fixed_queries=plain(cs.fixed_queries),
        permutation_columns=[(c.kind, c.index) for c in cs.permutation_columns],
        lookups=[([callable_of(e) for e in i], [callable_of(e) for e in t]) for i, t in cs.lookups],
        degree=cs.degree(), blinding_factors=cs.blinding_factors())


# ---- Assigned, Value (plonk/assigned.rs, circuit/value.rs) ---------------------------------------------------------------------------------
class Assigned:
    """Zero, Trivial(x) or Rational(numerator, denominator) over integers, reduced modulo `m` when one is given.  x / 0 = 0."""
    __slots__ = ("kind", "num", "den", "m")

    def __init__(self, kind: str, num: int = 0, den: int = 1, m: int | None = None):
        self.kind, self.m = kind, m
        self.num, self.den = (num % m, den % m) if m else (num, den)

    @staticmethod
    def zero(m=None):
        return Assigned("Zero", 0, 1, m)

    @staticmethod
    def trivial(x: int, m=None):
        return Assigned("Trivial", x, 1, m)

    @staticmethod
    def rational(num: int, den: int, m=None):
        return Assigned("Rational", num, den, m)

    @staticmethod
    def of(x, m=None) -> "Assigned":
        return x if isinstance(x, Assigned) else Assigned.trivial(int(x), m)

    def numerator(self) -> int:
        return self.num

    def denominator(self):
        return self.den if self.kind == "Rational" else None

    def is_zero_vartime(self) -> bool:                                        # :299-308
        if self.kind == "Zero":
            return True
        return self.num == 0 or (self.kind == "Rational" and self.den == 0)

    def __neg__(self):                                                        # :64-74
        return self if self.kind == "Zero" else Assigned(self.kind, -self.num, self.den, self.m)

    def __add__(self, rhs):                                                   # :77-121
        rhs = Assigned.of(rhs, self.m)
        m = self.m or rhs.m
        a, b = self, rhs
        if a.kind == "Zero":
            return b
        if b.kind == "Zero":
            return a
        if a.kind == "Rational" and a.den == 0:                               # one side is x/0, which is zero
            return b
        if b.kind == "Rational" and b.den == 0:
            return a
        if a.kind == "Trivial" and b.kind == "Trivial":
            return Assigned.trivial(a.num + b.num, m)
        if a.kind == "Trivial":
            a, b = b, a
        if b.kind == "Trivial":
            return Assigned.rational(a.num + a.den * b.num, a.den, m)
        return Assigned.rational(a.num * b.den + a.den * b.num, a.den * b.den, m)

    __radd__ = __add__

    def __sub__(self, rhs):
        return self + (-Assigned.of(rhs, self.m))

    def __rsub__(self, lhs):
        return Assigned.of(lhs, self.m) + (-self)

    def __mul__(self, rhs):                                                   # :225-244
        rhs = Assigned.of(rhs, self.m)
        m = self.m or rhs.m
        a, b = self, rhs
        if a.kind == "Zero" or b.kind == "Zero":
            return Assigned.zero(m)
        if a.kind == "Trivial" and b.kind == "Trivial":
            return Assigned.trivial(a.num * b.num, m)
        if a.kind == "Trivial":
            a, b = b, a
        if b.kind == "Trivial":
            return Assigned.rational(a.num * b.num, a.den, m)
        return Assigned.rational(a.num * b.num, a.den * b.den, m)

    __rmul__ = __mul__

    def double(self):
        return self if self.kind == "Zero" else Assigned(self.kind, 2 * self.num, self.den, self.m)

    def square(self):
        return self if self.kind == "Zero" else Assigned(self.kind, self.num * self.num, self.den * self.den, self.m)

    def cube(self):
        return self.square() * self

    def invert(self):                                                         # :341-347
        if self.kind == "Zero":
            return self
        if self.kind == "Trivial":
            return Assigned.rational(1, self.num, self.m)
        return Assigned.rational(self.den, self.num, self.m)

    def evaluate(self, m: int | None = None) -> int:                          # :353-365
        m = m or self.m
        if m is None:
            raise ValueError("Assigned.evaluate needs the modulus")
        if self.kind != "Rational" or self.den % m == 1:
            return self.num % m
        return self.num * pow(self.den, -1, m) % m if self.den % m else 0

    def __repr__(self):
        return {"Zero": "Zero", "Trivial": f"Trivial({self.num})"}.get(self.kind, f"Rational({self.num}, {self.den})")


class Value:
    """circuit::Value: a witness that may be unknown (None inside)."""
    __slots__ = ("inner",)

    def __init__(self, inner=None):
        self.inner = inner

    @staticmethod
    def known(v):
        return Value(v)

    @staticmethod
    def unknown():
        return Value(None)

    def is_none(self) -> bool:
        return self.inner is None

    def map(self, f):
        return Value(None if self.inner is None else f(self.inner))

    def zip(self, other):
        return Value(None if self.inner is None or other.inner is None else (self.inner, other.inner))

    def _bin(self, other, f):
        o = other.inner if isinstance(other, Value) else other
        return Value(None if self.inner is None or o is None else f(self.inner, o))

    def __add__(self, other):
        return self._bin(other, lambda a, b: a + b)

    def __sub__(self, other):
        return self._bin(other, lambda a, b: a - b)

    def __mul__(self, other):
        return self._bin(other, lambda a, b: a * b)

    def square(self):
        return self.map(lambda a: a.square() if isinstance(a, Assigned) else a * a)


def _unwrap(v):
    return v.inner if isinstance(v, Value) else v


# ---- the copy-constraint assembly (plonk/permutation/keygen.rs:16-103) ---------------------------------------------------------------------
class PermutationAssembly:
    """mapping / aux / sizes over flat cell indices column * n + row, the columns in `enable_equality` order."""

    def __init__(self, n: int, columns):
        self.n, self.columns = n, list(columns)
        total = n * len(self.columns)
        self.mapping = np.arange(total, dtype=np.int64)
        self.aux = np.arange(total, dtype=np.int64)
        self.sizes = np.ones(total, dtype=np.int64)

    def copy(self, left_column: Column, left_row: int, right_column: Column, right_row: int) -> None:      # :47-103
        try:
            lc, rc = self.columns.index(left_column), self.columns.index(right_column)
        except ValueError:
            raise ColumnNotInPermutation(str(left_column if left_column not in self.columns else right_column)) from None
        if left_row >= self.n or right_row >= self.n:
            raise BoundsFailure()
        a, b = lc * self.n + left_row, rc * self.n + right_row
        mapping, aux, sizes = self.mapping, self.aux, self.sizes
        left, right = int(aux[a]), int(aux[b])
        if left == right:
            return
        if sizes[left] < sizes[right]:
            left, right = right, left
        sizes[left] += sizes[right]
        i = right
        while True:                                                           # the smaller cycle takes the larger one's representative
            aux[i] = left
            i = int(mapping[i])
            if i == right:
                break
        mapping[a], mapping[b] = mapping[b], mapping[a]

    def flat(self) -> np.ndarray:
        """(columns, n) of c' * n + r': what `plonk.keygen_pk` and `dev.MockProver.run` take."""
        return self.mapping.reshape(len(self.columns), self.n)

    def pairs(self) -> list:
        n = self.n
        return [[(int(v) // n, int(v) % n) for v in row] for row in self.flat()]


# ---- what synthesis writes into (plonk::Assignment: keygen.rs:46-186, prover.rs:145-245, dev.rs:296-461) ------------------------------------------
class _ColumnCells:
    """One column's assigned cells: single assignments as integers on the host, whole vectors as (limbs, limbs | None) tensors or
    arrays; `materialise` replays them in call order into (n, 4) numerators and, if any value is Rational, denominators."""

    def __init__(self):
        self.ops = []                                                         # ("cells", {row: (num, den | None)}) | ("vector", row, num, den) | ("fill", lo, hi, (num, den))
        self.rational = False

    def put(self, row: int, value: Assigned) -> None:
        den = value.den if value.kind == "Rational" else None
        self.rational |= den is not None
        if not self.ops or self.ops[-1][0] != "cells":
            self.ops.append(("cells", {}))
        self.ops[-1][1][row] = (value.num, den)

    def put_vector(self, row: int, num, den) -> None:
        self.rational |= den is not None
        self.ops.append(("vector", row, num, den))

    def fill(self, lo: int, hi: int, value: Assigned) -> None:
        den = value.den if value.kind == "Rational" else None
        self.rational |= den is not None
        self.ops.append(("fill", lo, hi, (value.num, den)))

    def integers(self, n: int, field: int) -> list:
        """The column as n canonical integers, evaluated on the host cell by cell (`Assigned::evaluate`): for small circuits and for
        checking a layout; the provers use `materialise` and the device."""
        m = fields.MODULUS[field]
        div = lambda num, den: num % m if den is None else Assigned.rational(num, den, m).evaluate()
        ints = lambda a: fields.from_limbs(a.cpu().numpy().view(np.uint64) if type(a).__module__.startswith("torch") else a, field, True)
        out = [0] * n
        for op in self.ops:
            if op[0] == "cells":
                for row, (num, den) in op[1].items():
                    out[row] = div(num, den)
            elif op[0] == "vector":
                _, row, v_num, v_den = op
                dens = [None] * v_num.shape[0] if v_den is None else ints(v_den)
                out[row:row + v_num.shape[0]] = [div(a, b) for a, b in zip(ints(v_num), dens)]
            else:
                _, lo, hi, (num, den) = op
                out[lo:hi] = [div(num, den)] * (hi - lo)
        return out

    def materialise(self, num, den, field: int) -> None:
        """num / den: (n, 4) int64 device views, zero / one initialised."""
        import torch
        dev = num.device
        limbs = lambda ints: torch.from_numpy(fields.to_limbs(ints, field, True).view(np.int64)).to(dev)
        as_dev = lambda a: a.to(dev) if type(a).__module__.startswith("torch") else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)
        for op in self.ops:
            if op[0] == "cells":
                rows = sorted(op[1])
                idx = torch.tensor(rows, dtype=torch.int64, device=dev)
                num[idx] = limbs([op[1][r][0] for r in rows])
                if den is not None:
                    den[idx] = limbs([1 if op[1][r][1] is None else op[1][r][1] for r in rows])
            elif op[0] == "vector":
                _, row, v_num, v_den = op
                count = v_num.shape[0]
                num[row:row + count] = as_dev(v_num)
                if den is not None:
                    den[row:row + count] = as_dev(v_den) if v_den is not None else limbs([1])[0]
            else:
                _, lo, hi, (v_num, v_den) = op
                num[lo:hi] = limbs([v_num])[0]
                if den is not None:
                    den[lo:hi] = limbs([1 if v_den is None else v_den])[0]


class RegionRecord:
    """dev::Region (dev.rs:42-73): what the MockProver keeps of one region.  `rows` is (first, last) over the assigned cells alone, None
    while nothing is assigned (enabling a selector does not extend it); `enabled_selectors` maps a selector's index to the absolute rows
    it was enabled on, in enable order; `cells` lists the assignments as ranges (column, first row, count) in call order -- a single
    cell is a range of one, a whole vector is one range however long, a cell assigned twice is listed twice."""
    __slots__ = ("index", "name", "columns", "rows", "enabled_selectors", "cells")

    def __init__(self, index: int, name: str):
        self.index, self.name = index, name
        self.columns, self.rows, self.enabled_selectors, self.cells = set(), None, {}, []

    def assigned(self, column: Column, row: int, count: int = 1) -> None:      # update_extent + cells.push, for `count` rows at once
        self.columns.add(column)
        first, last = self.rows or (row, row)
        self.rows = (min(first, row), max(last, row + count - 1))
        self.cells.append((column, row, count))

    def __repr__(self):
        return (f"RegionRecord({self.index}, {self.name!r}, columns={sorted(self.columns, key=lambda c: (c.kind, c.index))}, rows={self.rows}, "
                f"enabled_selectors={self.enabled_selectors}, cells={self.cells})")


class Assembly:
    """The `Assignment` every synthesis here runs against.  fixed=True collects fixed cells, selectors and copies (keygen.rs:46-186);
    advice=True collects advice cells (prover.rs:145-245); both: dev.rs:296-461.  regions=True also keeps a `RegionRecord` per
    `enter_region` / `exit_region` bracket in `.regions` (dev.rs:314-331); what is assigned outside a bracket belongs to no region."""

    def __init__(self, k: int, cs: ConstraintSystem, field: int, fixed: bool, advice: bool, instances=None, regions: bool = False):
        self.k, self.n, self.cs, self.field, self.m = k, 1 << k, cs, field, fields.MODULUS[field]
        self.usable = self.n - (cs.blinding_factors() + 1)
        self.collect_fixed, self.collect_advice = fixed, advice
        self.instances = instances
        self.fixed = [_ColumnCells() for _ in range(cs.num_fixed_columns)] if fixed else None
        self.advice = [_ColumnCells() for _ in range(cs.num_advice_columns)] if advice else None
        self.selectors = np.zeros((cs.num_selectors, self.n), dtype=bool) if fixed else None
        self.permutation = PermutationAssembly(self.n, cs.permutation_columns) if fixed else None
        self.regions = [] if regions else None
        self.current_region = None

    def enter_region(self, name) -> None:                                     # dev.rs:314-327
        if self.regions is not None:
            assert self.current_region is None, "regions do not nest"
            self.current_region = RegionRecord(len(self.regions), str(name() if callable(name) else name))

    def exit_region(self) -> None:                                            # dev.rs:329-331
        if self.regions is not None:
            self.regions.append(self.current_region)
            self.current_region = None

    def _row(self, row: int, count: int = 1) -> None:
        if row < 0 or row + count > self.usable:
            raise NotEnoughRowsAvailable(self.k)

    def _assigned(self, to) -> Assigned:
        v = _unwrap(to() if callable(to) else to)
        if v is None:
            raise Synthesis("an unknown value where one is needed")
        return Assigned.of(v, self.m)

    def enable_selector(self, selector: Selector, row: int) -> None:
        if self.collect_fixed:
            self._row(row)
            if self.current_region is not None:                               # dev.rs:342-350
                self.current_region.enabled_selectors.setdefault(selector.index, []).append(row)
            self.selectors[selector.index][row] = True

    def enable_selector_rows(self, selector: Selector, rows: np.ndarray) -> None:
        if self.collect_fixed and rows.size:
            if int(rows.min()) < 0 or int(rows.max()) >= self.usable:
                raise NotEnoughRowsAvailable(self.k)
            if self.current_region is not None:
                self.current_region.enabled_selectors.setdefault(selector.index, []).extend(rows.tolist())
            self.selectors[selector.index][rows] = True

    def query_instance(self, column: Column, row: int) -> Value:
        self._row(row)
        if self.instances is None:
            return Value.unknown()
        values = self.instances[column.index]
        return Value.known(int(values[row]) % self.m if row < len(values) else 0)

    def assign_advice(self, column: Column, row: int, to):
        """Returns the assigned value where this assembly asks for it, else None (the closure is not called: keygen.rs:94-109)."""
        if not self.collect_advice:
            return None
        self._row(row)
        if self.current_region is not None:                                   # dev.rs:390-393
            self.current_region.assigned(column, row)
        value = self._assigned(to)
        self.advice[column.index].put(row, value)
        return value

    def assign_fixed(self, column: Column, row: int, to):
        if not self.collect_fixed:
            return None
        self._row(row)
        if column.index >= len(self.fixed):
            raise BoundsFailure()
        if self.current_region is not None:                                   # dev.rs:422-425
            self.current_region.assigned(column, row)
        value = self._assigned(to)
        self.fixed[column.index].put(row, value)
        return value

    def assign_vector(self, column: Column, row: int, num, den) -> None:
        cells = self.advice if column.kind == ADVICE else self.fixed
        if (column.kind == ADVICE and not self.collect_advice) or (column.kind == FIXED and not self.collect_fixed):
            return
        self._row(row, int(num.shape[0]))
        if self.current_region is not None:
            self.current_region.assigned(column, row, int(num.shape[0]))
        cells[column.index].put_vector(row, num, den)

    def copy(self, left_column: Column, left_row: int, right_column: Column, right_row: int) -> None:
        if self.collect_fixed:
            self._row(left_row)
            self._row(right_row)
            self.permutation.copy(left_column, left_row, right_column, right_row)

    def fill_from_row(self, column: Column, from_row: int, to) -> None:       # keygen.rs:152-173
        if self.collect_fixed:
            self._row(from_row)
            if self.current_region is not None:                               # dev.rs:462-464 assigns row by row: inside a region they are its cells
                self.current_region.assigned(column, from_row, self.usable - from_row)
            self.fixed[column.index].fill(from_row, self.usable, self._assigned(to))

    def host_columns(self, cells) -> list:
        return [c.integers(self.n, self.field) for c in cells]

    def columns_to_field(self, cells, device=None):
        """Every column of `cells` as one (columns * n, 4) device tensor of field elements: ONE `assigned_to_field` launch over the
        concatenation (poly.rs:135-180).  Returns the list of (n, 4) views."""
        import torch
        from .arithmetic import assigned_to_field
        dev = torch.device(device) if device else fields.current_device()
        count, n = len(cells), self.n
        num = torch.zeros((count * n, 4), dtype=torch.int64, device=dev)
        den = None
        if any(c.rational for c in cells):
            one = torch.from_numpy(fields.to_limbs([1], self.field, True).view(np.int64)).to(dev)
            den = one.repeat(count * n, 1)
        for i, c in enumerate(cells):
            c.materialise(num[i * n:(i + 1) * n], None if den is None else den[i * n:(i + 1) * n], self.field)
        if count:
            assigned_to_field(num, den, self.field)
        return [num[i * n:(i + 1) * n] for i in range(count)]


# ---- Layouter, Region, Table and the single-pass floor planner ------------------------------------------------------------------------------
@dataclass(frozen=True)
class Cell:
    region_index: int
    row_offset: int
    column: Column


class AssignedCell:
    def __init__(self, value, cell: Cell):
        self._value, self._cell = value, cell

    def cell(self) -> Cell:
        return self._cell

    def value(self) -> Value:
        return Value(self._value)

    def copy_advice(self, region: "Region", column: Column, offset: int) -> "AssignedCell":      # circuit.rs:150-166
        out = region.assign_advice(column, offset, lambda: self._value)
        region.constrain_equal(out.cell(), self._cell)
        return out


class AssignedVector:
    """What the bulk assignments return: `.cell(i)` is the cell of the i-th row, for copy constraints."""

    def __init__(self, region_index: int, column: Column, offset: int, count: int):
        self.region_index, self.column, self.offset, self.count = region_index, column, offset, count

    def cell(self, i: int) -> Cell:
        if not 0 <= i < self.count:
            raise IndexError(i)
        return Cell(self.region_index, self.offset + i, self.column)


def _vector(values):
    """An (m, 4) Montgomery tensor / array, or a (numerators, denominators) pair of them -> (num, den | None)."""
    num, den = values if isinstance(values, (tuple, list)) and len(values) == 2 and hasattr(values[0], "shape") else (values, None)
    for v in (num, den):
        if v is not None and (v.ndim != 2 or v.shape[1] != 4):
            raise ValueError("a vector of cells is an (m, 4) array of Montgomery limbs")
    if den is not None and den.shape[0] != num.shape[0]:
        raise ValueError("numerators and denominators differ in length")
    return num, den


class Region:
    """circuit::Region over one of the two passes of the layouter: the shape pass (`layouter` is None: circuit/layouter.rs:121-250
    records columns and the row count, calls no closure) and the assignment pass (single_pass.rs:218-363)."""

    def __init__(self, region_index: int, layouter=None):
        self.region_index, self.layouter = region_index, layouter
        self.columns, self.row_count = [], 0                                  # the shape; columns: Column or Selector
        self.constants = []                                                   # (Assigned, Cell) to place afterwards

    def _note(self, column, offset: int, count: int = 1) -> None:
        if column not in self.columns:
            self.columns.append(column)
        self.row_count = max(self.row_count, offset + count)

    def _start(self) -> int:
        return self.layouter.regions[self.region_index]

    def enable_selector(self, selector: Selector, offset: int) -> None:
        self._note(selector, offset)
        if self.layouter:
            self.layouter.cs.enable_selector(selector, self._start() + offset)

    def enable_selector_rows(self, selector: Selector, offsets) -> None:
        """`enable_selector` on every offset of an integer array in one call."""
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.size:
            if int(offsets.min()) < 0:
                raise ValueError("a negative offset")
            self._note(selector, int(offsets.max()))
            if self.layouter:
                self.layouter.cs.enable_selector_rows(selector, self._start() + offsets)

    def _assign(self, column: Column, offset: int, to) -> AssignedCell:
        self._note(column, offset)
        value = None
        if self.layouter:
            backend = self.layouter.cs
            value = (backend.assign_advice if column.kind == ADVICE else backend.assign_fixed)(column, self._start() + offset, to)
        return AssignedCell(value, Cell(self.region_index, offset, column))

    def assign_advice(self, column: Column, offset: int, to) -> AssignedCell:
        assert column.kind == ADVICE
        return self._assign(column, offset, to)

    def assign_fixed(self, column: Column, offset: int, to) -> AssignedCell:
        assert column.kind == FIXED
        return self._assign(column, offset, to)

    def _assign_column(self, column: Column, offset: int, values) -> AssignedVector:
        num, den = _vector(values)
        count = int(num.shape[0])
        if count:
            self._note(column, offset, count)
            if self.layouter:
                self.layouter.cs.assign_vector(column, self._start() + offset, num, den)
        return AssignedVector(self.region_index, column, offset, count)

    def assign_advice_column(self, column: Column, offset: int, values) -> AssignedVector:
        assert column.kind == ADVICE
        return self._assign_column(column, offset, values)

    def assign_fixed_column(self, column: Column, offset: int, values) -> AssignedVector:
        assert column.kind == FIXED
        return self._assign_column(column, offset, values)

    def assign_advice_from_constant(self, column: Column, offset: int, constant) -> AssignedCell:      # single_pass.rs:283-295
        cell = self.assign_advice(column, offset, lambda: constant)
        self.constrain_constant(cell.cell(), constant)
        return cell

    def assign_advice_from_instance(self, instance: Column, row: int, advice: Column, offset: int) -> AssignedCell:      # :297-317
        value = None
        if self.layouter:
            value = self.layouter.cs.query_instance(instance, row).inner
        cell = self.assign_advice(advice, offset, lambda: value)
        if self.layouter:
            self.layouter.cs.copy(advice, self._start() + offset, instance, row)
        return cell

    def constrain_constant(self, cell: Cell, constant) -> None:
        if self.layouter:
            self.constants.append((constant, cell))

    def constrain_equal(self, left: Cell, right: Cell) -> None:
        if self.layouter:
            regions = self.layouter.regions
            self.layouter.cs.copy(left.column, regions[left.region_index] + left.row_offset,
                                  right.column, regions[right.region_index] + right.row_offset)


class Table:
    """circuit::Table over SimpleTableLayouter (circuit/table_layouter.rs:41-116)."""

    def __init__(self, cs: Assembly, used_columns):
        self.cs, self.used_columns = cs, used_columns
        self.default_and_assigned = {}                                        # TableColumn -> [default | None, [bool]]

    def assign_cell(self, column: TableColumn, offset: int, to) -> None:
        if column in self.used_columns:
            raise TableError("UsedColumn", column)
        entry = self.default_and_assigned.setdefault(column, [None, []])
        holder = []

        def capture():
            holder.append(Assigned.of(_unwrap(to() if callable(to) else to), self.cs.m))
            return holder[0]
        self.cs.assign_fixed(column.inner, offset, capture)                   # tables are always assigned starting at row 0
        value = holder[0] if holder else None
        if offset == 0:
            if entry[0] is not None:
                raise TableError("OverwriteDefault", column)
            entry[0] = (value,)
        if len(entry[1]) <= offset:
            entry[1] += [False] * (offset + 1 - len(entry[1]))
        entry[1][offset] = True


def _table_length(default_and_assigned) -> int:                               # table_layouter.rs:118-150
    length, first = 0, None
    for column, (default, assigned) in default_and_assigned.items():
        if default is None or not assigned or not all(assigned):
            raise TableError("ColumnNotAssigned", column)
        if length not in (0, len(assigned)):
            raise TableError("UnevenColumnLengths", sorted([(column.inner.index, len(assigned)), (first.inner.index, length)]))
        length, first = len(assigned), column
    return length


def assign_table(cs: Assembly, table_columns: list, assignment, name="") -> None:
    """`assign_table` of every layouter (single_pass.rs:150-185, v1.rs:289-326): the cells, the length check, the columns recorded in
    `table_columns` so that no later table takes them, and the default value filled in below the table.  The cells are a region of
    their own under `name` (:158-165); the fill below them is not."""
    table = Table(cs, table_columns)
    cs.enter_region(name)
    assignment(table)
    cs.exit_region()
    first_unused = _table_length(table.default_and_assigned)
    table_columns += list(table.default_and_assigned)
    for column, (default, _) in table.default_and_assigned.items():
        cs.fill_from_row(column.inner, first_unused, lambda: default[0])


class _Namespace:
    def __init__(self, layouter):
        self._layouter = layouter

    def __getattr__(self, name):
        return getattr(self._layouter, name)


class SingleChipLayouter:
    """single_pass.rs:41-216."""

    def __init__(self, cs: Assembly, constants):
        self.cs, self.constants = cs, list(constants)
        self.regions, self.columns, self.table_columns = [], {}, []
        self.shapes = []                                                      # (columns, row_count) per region: what the shape pass saw

    def assign_region(self, name, assignment):                                # :80-148
        region_index = len(self.regions)
        shape = Region(region_index)
        assignment(shape)
        start = max([self.columns.get(c, 0) for c in shape.columns], default=0)
        self.regions.append(start)
        self.shapes.append((list(shape.columns), shape.row_count))
        for c in shape.columns:
            self.columns[c] = start + shape.row_count
        self.cs.enter_region(name)                                            # :109-116: the assignment pass alone
        region = Region(region_index, self)
        result = assignment(region)
        self.cs.exit_region()
        if not self.constants:                                                # :120-145
            if region.constants:
                raise NotEnoughColumnsForConstants()
        else:
            column = self.constants[0]
            for constant, advice in region.constants:
                row = self.columns.get(column, 0)
                self.cs.assign_fixed(column, row, lambda: constant)
                self.cs.copy(column, row, advice.column, self.regions[advice.region_index] + advice.row_offset)
                self.columns[column] = row + 1
        return result

    def assign_table(self, name, assignment) -> None:                         # :150-185
        assign_table(self.cs, self.table_columns, assignment, name)

    def constrain_instance(self, cell: Cell, instance: Column, row: int) -> None:      # :187-199
        self.cs.copy(cell.column, self.regions[cell.region_index] + cell.row_offset, instance, row)

    def namespace(self, name=None):
        return _Namespace(self)


class SimpleFloorPlanner:
    @staticmethod
    def synthesize(cs: Assembly, circuit, config, constants) -> SingleChipLayouter:      # :28-38
        layouter = SingleChipLayouter(cs, constants)
        circuit.synthesize(config, layouter)
        return layouter


class Circuit:
    """plonk::Circuit (circuit.rs:466-485): subclass and provide the three methods.  `configure` may be a static or an instance method."""
    floor_planner = SimpleFloorPlanner

    def without_witnesses(self):
        raise NotImplementedError

    def configure(self, meta: ConstraintSystem):
        raise NotImplementedError

    def synthesize(self, config, layouter) -> None:
        raise NotImplementedError


def synthesize(circuit, k: int, field: int, fixed: bool, advice: bool, instances=None, regions: bool = False):
    """configure + floor-plan one circuit: (constraint system, assembly, layouter).  Raises NotEnoughRowsAvailable as
    keygen.rs:200-202 does.  regions=True: `assembly.regions` holds a `RegionRecord` per region and table, as dev::MockProver keeps."""
    cs = ConstraintSystem(fields.MODULUS[field])
    config = circuit.configure(cs)
    if (1 << k) < cs.minimum_rows():
        raise NotEnoughRowsAvailable(k)
    assembly = Assembly(k, cs, field, fixed, advice, instances, regions)
    layouter = getattr(circuit, "floor_planner", SimpleFloorPlanner).synthesize(assembly, circuit, config, cs.constants)
    return cs, assembly, layouter


def pack_selectors(selectors: np.ndarray) -> np.ndarray:
    """(S, n) booleans -> (S, ceil(n / 32)) int32 words, row r = bit r % 32 of word r / 32."""
    s, n = selectors.shape
    words = (n + 31) // 32
    padded = np.zeros((s, words * 32), dtype=np.uint8)
    padded[:, :n] = selectors
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32).view(np.int32).reshape(s, words)


def fixed_columns_of(assembly: Assembly, cs: ConstraintSystem, device=None):
    """keygen.rs:221-227: the assigned fixed columns through `assigned_to_field`, the selectors compressed into further fixed columns
    (`cs` is rewritten in place).  Returns the (n, 4) device columns in the compressed system's order."""
    import torch
    from .arithmetic import selector_combine, selector_conflicts
    fixed = assembly.columns_to_field(assembly.fixed, device)
    if cs.num_selectors:
        dev = torch.device(device) if device else fields.current_device()
        bits = torch.from_numpy(pack_selectors(assembly.selectors)).to(dev)
        conflicts = selector_conflicts(bits).cpu().numpy()
        combinations = cs.compress_selectors(conflicts)
        roots, columns = [0] * cs.num_selectors, [0] * cs.num_selectors
        for c, members in enumerate(combinations):
            for s, root in members:
                roots[s], columns[s] = root, c
        combined = selector_combine(bits, roots, columns, assembly.n, len(combinations), assembly.field)
        fixed += [combined[c] for c in range(len(combinations))]
    return fixed


# ---- keys (plonk/keygen.rs:188-380, plonk.rs:61-116) ---------------------------------------------------------------------------------------------
def _point(p) -> str:
    return "Infinity" if p is None else f"({_hex(p[0])}, {_hex(p[1])})"


def pinned_verification_key(params, domain, cs: ConstraintSystem, fixed_commitments, permutation_commitments) -> str:
    """`format!("{:?}", vk.pinned())` (plonk.rs:103-116, 142-158; poly/domain.rs PinnedEvaluationDomain; permutation.rs VerifyingKey)."""
    bf, sf = fields.CURVE_FIELDS[params.curve]
    points = lambda ps: "[" + ", ".join(_point(p) for p in ps) + "]"
    return ("PinnedVerificationKey { "
            f"base_modulus: \"{_hex(fields.MODULUS[bf])}\", scalar_modulus: \"{_hex(fields.MODULUS[sf])}\", "
            f"domain: PinnedEvaluationDomain {{ k: {domain.k}, extended_k: {domain.extended_k}, omega: {_hex(domain.omega)} }}, "
            f"cs: {cs.pinned()}, fixed_commitments: {points(fixed_commitments)}, "
            f"permutation: VerifyingKey {{ commitments: {points(permutation_commitments)} }} }}")


def transcript_repr(pinned: str, modulus: int) -> int:
    """plonk.rs:75-101: Blake2b-512, personal "Halo2-Verify-Key", over the length of the Debug text and the text; from_uniform_bytes."""
    s = pinned.encode()
    digest = hashlib.blake2b(len(s).to_bytes(8, "little") + s, digest_size=64, person=b"Halo2-Verify-Key").digest()
    return int.from_bytes(digest, "little") % modulus


def keygen_pk(params, circuit, device=None):
    """keygen_vk + keygen_pk of the reference in one (keygen.rs:188-380): a `plonk.ProvingKey` whose `.vk` is the
    `verifier.VerifyingKey`; both carry `circuit_cs` (the compressed front-end system), `pinned()` and the reference's `vk_repr`."""
    from .verifier import keygen_vk as commitments_of
    sf = fields.CURVE_FIELDS[params.curve][1]
    cs, assembly, _ = synthesize(circuit.without_witnesses(), params.k, sf, fixed=True, advice=False)
    fixed = fixed_columns_of(assembly, cs, device)
    pk = _plonk.keygen_pk(params, lower(cs), fixed, assembly.permutation.flat(), vk_repr=0, device=device)
    vk = commitments_of(params, pk)
    text = pinned_verification_key(params, pk.domain, cs, vk.fixed_commitments, vk.permutation_commitments)
    pk.vk_repr = vk.vk_repr = transcript_repr(text, fields.MODULUS[sf])
    for key in (pk, vk):
        key.circuit_cs = cs
        key.pinned = lambda text=text: text
    pk.vk = vk
    return pk


def keygen_vk(params, circuit, device=None):
    return keygen_pk(params, circuit, device).vk


def create_proof(params, pk, circuits, instances, rng, transcript, schedule: str | None = None) -> None:
    """plonk::create_proof (prover.rs:35-341 in front of `plonk.create_proof_many`): every circuit is synthesized into its advice
    cells (fixed cells, selectors and copies are ignored, :104-245), ONE `assigned_to_field` inverts the denominators of all advice
    columns of all instances (:291), and the existing prover takes over.  instances[i]: the instance columns of circuits[i]."""
    circuits, instances = list(circuits), [list(i) for i in instances]
    if len(circuits) != len(instances):
        raise ValueError("InvalidInstances")
    sf = fields.CURVE_FIELDS[params.curve][1]
    dev = pk.l0.device
    assemblies = []
    for circuit, inst in zip(circuits, instances):
        if len(inst) != pk.cs.num_instance_columns:
            raise ValueError("InvalidInstances")
        _, assembly, _ = synthesize(circuit, params.k, sf, fixed=False, advice=True, instances=inst)
        assemblies.append(assembly)
    cells = [c for a in assemblies for c in a.advice]
    columns = assemblies[0].columns_to_field(cells, dev) if assemblies else []
    per = pk.cs.num_advice_columns
    _plonk.create_proof_many(params, pk, [(columns[i * per:(i + 1) * per], inst) for i, inst in enumerate(instances)], rng, transcript,
                             schedule=schedule)
