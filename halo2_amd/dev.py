"""`dev::MockProver` (halo2_proofs/src/dev.rs:158-924) for the lowered interface of `halo2_amd.plonk`: which constraints does a
witness break, and where?  `create_proof` turns a broken witness into a proof that does not verify -- one bit; this checker names
the gate, lookup or copy constraint and the row, from the columns as they already sit in device memory.

    prover = MockProver.run(k, cs, fixed_columns, advice_columns, instance_columns, mapping, field)
    prover.verify(max_failures=1024)     # [] when satisfied
    prover.failure_counts                 # exact totals per kind, also when the lists are capped
    prover.assert_satisfied()             # AssertionError with the failures printed (dev.rs:915-923)

Semantics (dev.rs:576-904, restated for columns that are already assigned): n = 2^k rows, usable = n - (blinding_factors + 1).

* An advice cell in a row >= usable is Poison (dev.rs:529-533; `create_proof` overwrites those rows with randomness).  Fixed and
  instance cells never are.  Expressions follow dev.rs:104-156: negation and addition propagate poison, a product with Real(0)
  or the constant 0 is Real(0), rotations wrap modulo n.
* Gates: every entry of `cs.gates` at every row.  Real(x != 0) -> ConstraintNotSatisfied(gate_index, row, cell_values); Poison ->
  ConstraintPoisoned(gate_index, rows, first_row), once per gate, placed at its first poisoned row.
* Lookups: input row r < usable fails when its tuple of values does not occur among the table tuples of rows < usable; exact
  comparison of canonical values, Poison being one more value equal only to itself -> Lookup(lookup_index, row).
* Permutation: cell (c, r) must equal the cell mapping[c][r]; two poisoned cells are equal only when they are the same cell
  -> Permutation((kind, index), row).
* Order: gates by (gate_index, row), lookups by (lookup_index, row), permutation by (column, row).  (The reference lists a
  lookup's failures by sorted input value, dev.rs:807, and keeps a ConstraintPoisoned per run of poisoned rows; rows are the
  stable order here.)  The lowered form has no regions and no selectors, so CellNotAssigned / InstanceCellNotAssigned and
  FailureLocation::InRegion do not exist.
* `verify(max_failures=N)` returns at most N failures per kind, the first N in the order above; `failure_counts` is exact.

The checks are three kernels' worth of C ABI (halo2_amd/csrc/mock_prover.hip): `h2_check_expressions_device`,
`h2_lookup_check_device`, `h2_permutation_check_device`.  They leave bit planes and counts on the device; `verify` reads the
counts back once (its only synchronisation) and fetches a plane only for what failed."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import fields
from ._lib import check, lib
from .arithmetic import _p, _stream_ptr
from .evaluator import _CONST, _LINEAR, _MULADD, _POLY, _SCALE, LAGRANGE, AstLeaf, Evaluator, _as_ast
from .plonk import ConstraintSystem, _Cells


@dataclass(frozen=True)
class ConstraintNotSatisfied:
    """VerifyFailure::ConstraintNotSatisfied.  cell_values: ((kind, column, rotation, canonical value), ...) for every cell the gate
    queries (util::cell_values); the value of a poisoned cell (it met a zero factor) is None."""
    gate_index: int
    row: int
    cell_values: tuple

    def __str__(self):
        cells = ", ".join(f"{kind}[{col}]@{rot:+d} = " + ("poison" if v is None else hex(v)) for kind, col, rot, v in self.cell_values)
        return f"Constraint {self.gate_index} is not satisfied on row {self.row}: {cells}"


@dataclass(frozen=True)
class ConstraintPoisoned:
    """VerifyFailure::ConstraintPoisoned: the gate is active on `rows` rows where it reads a blinding row; the first is `first_row`."""
    gate_index: int
    rows: int
    first_row: int

    def __str__(self):
        return (f"Constraint {self.gate_index} is active on an unusable row ({self.rows} row(s), first {self.first_row}): "
                "missing selector?")


@dataclass(frozen=True)
class Lookup:
    """VerifyFailure::Lookup: the input tuple of `row` is not in the table."""
    lookup_index: int
    row: int

    def __str__(self):
        return f"Lookup {self.lookup_index} is not satisfied on row {self.row}"


@dataclass(frozen=True)
class Permutation:
    """VerifyFailure::Permutation: the cell of permutation column `column` = (kind, index) at `row` differs from its copy."""
    column: tuple
    row: int

    def __str__(self):
        return f"Equality constraint not satisfied by cell ({self.column[0]}[{self.column[1]}], row {self.row})"


KINDS = ("ConstraintNotSatisfied", "ConstraintPoisoned", "Lookup", "Permutation")


class _RecordingCells:
    """Applies a lowered expression once to learn which cells it queries, in the style of plonk._FingerprintCells."""

    def __init__(self):
        self.cells = []

    def _note(self, kind, col, rot):
        if (kind, col, rot) not in self.cells:
            self.cells.append((kind, col, rot))
        return 1

    def fixed(self, col: int, rot: int = 0):
        return self._note("fixed", col, rot)

    def advice(self, col: int, rot: int = 0):
        return self._note("advice", col, rot)

    def instance(self, col: int, rot: int = 0):
        return self._note("instance", col, rot)

    def __getattr__(self, name):
        raise AttributeError(f"lowered expressions may only query cells.fixed / advice / instance, not cells.{name}")


def queried_cells(expression) -> list:
    """(kind, column, rotation) of every distinct cell a lowered expression queries, in the order it first asks for them."""
    rec = _RecordingCells()
    expression(rec)
    return rec.cells


class _Rows:
    """What Evaluator.compile asks of a domain for Lagrange-basis trees without linear terms: the field and its modulus."""

    def __init__(self, k: int, field: int):
        self.k, self.n, self.field, self.m = k, 1 << k, field, fields.MODULUS[field]


def _link(compiled):
    """Several compiled trees as one program array with offsets and one constant table (h2_check_expressions_device)."""
    words, offsets, consts = [], [0], []
    for c in compiled:
        base, pc = len(consts), 0
        while pc < c.n_words:
            word = c.prog[pc]
            op = word & 0xFF
            if op == _POLY:
                words += [word, c.prog[pc + 1]]
                pc += 2
                continue
            words.append(word + (base << 8) if op in (_CONST, _LINEAR, _SCALE, _MULADD) else word)
            pc += 1
        consts += [c.consts[i] for i in range(c.n_consts)]
        offsets.append(len(words))
    table = np.ascontiguousarray(np.stack(consts)) if consts else np.zeros((1, 4), dtype=np.uint64)
    return (C.c_uint32 * len(words))(*words), (C.c_size_t * len(offsets))(*offsets), table, len(consts)


def compile_programs(cs: ConstraintSystem, k: int, field: int, evaluator: Evaluator):
    """The host half of `run`: every gate flattened into one linked program set, and per lookup (w, its w input then its w table
    expressions).  Registered polynomials are numbered fixed columns first, then advice, then instance."""
    counts = (cs.num_fixed_columns, cs.num_advice_columns, cs.num_instance_columns)
    starts = (0, counts[0], counts[0] + counts[1])
    leaves = [[AstLeaf(evaluator, s + i) for i in range(c)] for s, c in zip(starts, counts)]
    cells, rows = _Cells(*leaves), _Rows(k, field)
    flat = lambda expressions: _link([evaluator.compile(_as_ast(e(cells)), rows) for e in expressions])
    lookups = []
    for ins, tabs in cs.lookups:
        if len(ins) != len(tabs) or not ins:
            raise ValueError("a lookup has as many table expressions as input expressions, at least one")       # dev.rs:753
        lookups.append((len(ins), flat(list(ins) + list(tabs))))
    return (flat(cs.gates) if cs.gates else None), lookups


def _set_rows(plane, limit=None) -> list:
    """Row numbers of the set bits of one bit plane (a device tensor of 64-bit words), ascending, at most `limit`."""
    bits = np.unpackbits(plane.cpu().numpy().view(np.uint8), bitorder="little")
    rows = np.flatnonzero(bits)
    return [int(r) for r in (rows if limit is None else rows[:limit])]


def _length(col) -> int:
    return int(col.shape[0]) if hasattr(col, "shape") else len(col)


class MockProver:
    def __init__(self):
        raise TypeError("use MockProver.run(...)")

    @classmethod
    def run(cls, k: int, cs: ConstraintSystem, fixed_columns, advice_columns, instance_columns, mapping, field: int, device=None) -> "MockProver":
        """dev.rs:463-574 after synthesis.  Columns as `keygen_pk` / `create_proof` take them: integer lists or (n, 4) Montgomery CUDA
        tensors (tensors are used in place, not copied); instance columns of at most `usable` values; `mapping` as nested (c', r')
        pairs or the flat c' * n + r' array, one row per permutation column.  Raises ValueError where the reference returns
        Error::NotEnoughRowsAvailable / InstanceTooLarge or panics on a column of the wrong length."""
        import torch
        self = object.__new__(cls)
        if field not in (0, 1):
            raise ValueError("unknown field")
        n = 1 << k
        usable = n - (cs.blinding_factors + 1)
        if usable < 1:
            raise ValueError("NotEnoughRowsAvailable")                                    # dev.rs:470-474
        if (len(fixed_columns) != cs.num_fixed_columns or len(advice_columns) != cs.num_advice_columns
                or len(instance_columns) != cs.num_instance_columns):
            raise ValueError("InvalidInstances: wrong number of columns")                  # dev.rs:476-478, prover.rs:49-57
        for col in list(fixed_columns) + list(advice_columns):
            if _length(col) > n:
                raise ValueError("NotEnoughRowsAvailable: a column is longer than 2^k")
        for col in instance_columns:
            if _length(col) > usable:
                raise ValueError("InstanceTooLarge")                                       # dev.rs:480-487
        n_perm = len(cs.permutation_columns)
        dev = torch.device(device) if device else fields.current_device()

        def up(col):
            if type(col).__module__.startswith("torch"):
                t = col.to(dev)
                if t.ndim != 2 or t.shape[1] != 4 or t.dtype != torch.int64:
                    raise ValueError("a device column is an (n, 4) int64 tensor of Montgomery limbs")
                t = t.contiguous()
            else:
                t = torch.from_numpy(fields.to_limbs(col, field, True).view(np.int64)).to(dev) if len(col) else \
                    torch.zeros((0, 4), dtype=torch.int64, device=dev)
            if t.shape[0] < n:                                                             # unassigned cells are zero (dev.rs:97)
                t = torch.cat([t, torch.zeros((n - t.shape[0], 4), dtype=torch.int64, device=dev)])
            return t
        self.k, self.n, self.usable, self.cs, self.field, self.device = k, n, usable, cs, field, dev
        self.fixed, self.advice, self.instance = [up(c) for c in fixed_columns], [up(c) for c in advice_columns], [up(c) for c in instance_columns]
        self.mapping = None
        if n_perm:
            if type(mapping).__module__.startswith("torch"):
                flat = mapping.to(dev).to(torch.int64)
            else:
                arr = np.asarray(mapping, dtype=np.int64)
                if arr.ndim == 3 and arr.shape[2] == 2:                                    # nested (c', r') pairs
                    arr = arr[:, :, 0] * n + arr[:, :, 1]
                flat = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
            if tuple(flat.shape) != (n_perm, n):
                raise ValueError("mapping: one row of 2^k entries per permutation column")
            self.mapping = flat.contiguous()
        self._ev = Evaluator(LAGRANGE)
        for t in self.fixed + self.advice + self.instance:
            self._ev.register_poly(t)
        self._is_advice = [0] * len(self.fixed) + [1] * len(self.advice) + [0] * len(self.instance)
        self._gates, self._lookups = compile_programs(cs, k, field, self._ev)
        self._gate_cells = [queried_cells(g) for g in cs.gates]
        self._counts = None
        return self

    @classmethod
    def run_circuit(cls, k: int, circuit, instances, field: int, device=None) -> "MockProver":
        """dev.rs:463-574 from a `halo2_amd.circuit.Circuit`: configure, synthesize with the witness (the circuit's floor planner), invert the
        assigned cells' denominators, compress the selectors, lower, `run`.  instances: the instance columns, integer lists."""
        from . import circuit as front
        instances = [list(col) for col in instances]
        cs, assembly, _ = front.synthesize(circuit, k, field, fixed=True, advice=True, instances=instances)
        fixed = front.fixed_columns_of(assembly, cs, device)
        advice = assembly.columns_to_field(assembly.advice, device)
        return cls.run(k, front.lower(cs), fixed, advice, instances, assembly.permutation.flat(), field, device)

    # ---- the three device checks: enqueue only ---------------------------------------------------------------------------------------
    def _check_expressions(self, linked, n_programs: int, store: bool):
        import torch
        prog, offsets, consts, n_consts = linked
        words = (self.n + 63) // 64
        nz = torch.empty((n_programs, words), dtype=torch.int64, device=self.device)
        po = torch.empty((n_programs, words), dtype=torch.int64, device=self.device)
        counts = torch.empty(2 * n_programs, dtype=torch.int32, device=self.device)
        values = torch.empty((n_programs, self.n, 4), dtype=torch.int64, device=self.device) if store else None
        polys = self._ev.polys
        ptrs = (C.c_void_p * max(1, len(polys)))(*[p.data_ptr() for p in polys])
        flags = (C.c_uint8 * max(1, len(polys)))(*self._is_advice)
        vals = (C.c_void_p * n_programs)(*[values[p].data_ptr() for p in range(n_programs)]) if store else None
        check(lib().h2_check_expressions_device(self.field, prog, offsets, n_programs, _p(consts), n_consts, ptrs, flags, len(polys), self.k,
                                                self.usable, nz.data_ptr(), po.data_ptr(), counts.data_ptr(), vals, _stream_ptr()),
              "h2_check_expressions_device")
        return nz, po, counts, values

    def _check_lookup(self, w: int, linked):
        import torch
        _, po, _, values = self._check_expressions(linked, 2 * w, True)
        fail = torch.empty((self.n + 63) // 64, dtype=torch.int64, device=self.device)
        count = torch.empty(1, dtype=torch.int32, device=self.device)
        arr = lambda ts: (C.c_void_p * w)(*[t.data_ptr() for t in ts])
        check(lib().h2_lookup_check_device(self.field, arr([values[c] for c in range(w)]), arr([po[c] for c in range(w)]),
                                           arr([values[w + c] for c in range(w)]), arr([po[w + c] for c in range(w)]), w, self.n, self.usable,
                                           1, fail.data_ptr(), count.data_ptr(), _stream_ptr()), "h2_lookup_check_device")
        return fail, count

    def _check_permutation(self):
        import torch
        by_kind = {"fixed": self.fixed, "advice": self.advice, "instance": self.instance}
        columns = self.cs.permutation_columns
        cols = [by_kind[kind][idx] for kind, idx in columns]
        fail = torch.empty((len(cols), (self.n + 63) // 64), dtype=torch.int64, device=self.device)
        counts = torch.empty(len(cols), dtype=torch.int32, device=self.device)
        ptrs = (C.c_void_p * len(cols))(*[t.data_ptr() for t in cols])
        flags = (C.c_uint8 * len(cols))(*[1 if kind == "advice" else 0 for kind, _ in columns])
        check(lib().h2_permutation_check_device(self.field, ptrs, flags, len(cols), self.mapping.data_ptr(), self.k, self.usable, 1,
                                                fail.data_ptr(), counts.data_ptr(), _stream_ptr()), "h2_permutation_check_device")
        return fail, counts

    def _cell_values(self, gate_index: int, rows: list) -> list:
        """util::cell_values for the reported rows only: one gather per queried cell, on the device."""
        import torch
        by_kind = {"fixed": self.fixed, "advice": self.advice, "instance": self.instance}
        at = torch.tensor(rows, dtype=torch.int64, device=self.device)
        per_cell = []
        for kind, col, rot in self._gate_cells[gate_index]:
            idx = (at + rot) % self.n
            vals = fields.from_limbs(by_kind[kind][col].index_select(0, idx).cpu().numpy().view(np.uint64), self.field, True)
            src = idx.cpu().tolist()
            per_cell.append([None if kind == "advice" and s >= self.usable else v for s, v in zip(src, vals)])
        return [tuple((kind, col, rot, per_cell[c][i]) for c, (kind, col, rot) in enumerate(self._gate_cells[gate_index]))
                for i in range(len(rows))]

    def verify(self, max_failures: int = 1024) -> list:
        """MockProver::verify (dev.rs:576-904): [] when the circuit is satisfied, else the failures in the order of the module's
        docstring, at most `max_failures` of each kind.  Everything is enqueued first; the one read-back of the counts synchronises."""
        import torch
        if max_failures < 0:
            raise ValueError("max_failures")
        n_gates = len(self.cs.gates)
        gates = self._check_expressions(self._gates, n_gates, False) if n_gates else None
        lookups = [self._check_lookup(w, linked) for w, linked in self._lookups]
        perm = self._check_permutation() if self.mapping is not None else None
        parts = ([gates[2]] if gates else []) + [c for _, c in lookups] + ([perm[1]] if perm else [])
        counts = torch.cat(parts).cpu().tolist() if parts else []
        gate_counts, counts = counts[:2 * n_gates], counts[2 * n_gates:]
        lookup_counts, perm_counts = counts[:len(lookups)], counts[len(lookups):]
        self._counts = {"ConstraintNotSatisfied": sum(gate_counts[0::2]), "ConstraintPoisoned": sum(1 for c in gate_counts[1::2] if c),
                        "Lookup": sum(lookup_counts), "Permutation": sum(perm_counts)}
        gate_failures, left_ns, left_po = [], max_failures, max_failures
        for g in range(n_gates):
            bad, poisoned = gate_counts[2 * g], gate_counts[2 * g + 1]
            if bad and left_ns:
                rows = _set_rows(gates[0][g], left_ns)
                left_ns -= len(rows)
                gate_failures += [ConstraintNotSatisfied(g, r, cv) for r, cv in zip(rows, self._cell_values(g, rows))]
            if poisoned and left_po:
                left_po -= 1
                gate_failures.append(ConstraintPoisoned(g, poisoned, _set_rows(gates[1][g], 1)[0]))
        gate_failures.sort(key=lambda f: (f.gate_index, f.first_row if isinstance(f, ConstraintPoisoned) else f.row))
        failures, left = gate_failures, max_failures
        for l, ((fail, _), c) in enumerate(zip(lookups, lookup_counts)):
            if c and left:
                rows = _set_rows(fail, left)
                left -= len(rows)
                failures += [Lookup(l, r) for r in rows]
        left = max_failures
        for col, c in enumerate(perm_counts):
            if c and left:
                rows = _set_rows(perm[0][col], left)
                left -= len(rows)
                failures += [Permutation(tuple(self.cs.permutation_columns[col]), r) for r in rows]
        return failures

    @property
    def failure_counts(self) -> dict:
        """Exact number of failures per kind (KINDS), whatever cap `verify` was given."""
        if self._counts is None:
            self.verify(0)
        return dict(self._counts)

    def assert_satisfied(self) -> None:
        """dev.rs:915-923: raises AssertionError with every failure (up to verify's default cap per kind) printed."""
        failures = self.verify()
        if failures:
            total = sum(self._counts.values())
            raise AssertionError(f"circuit was not satisfied ({total} failure(s)):\n" + "\n".join("  " + str(f) for f in failures))
