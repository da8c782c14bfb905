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
  stable order here.)  The lowered form has no regions and no selectors: `run` knows neither CellNotAssigned nor a location.
* Regions: `MockProver.run_circuit(k, circuit, instances, field, regions=True)` keeps the regions of the synthesis
  (`circuit.RegionRecord`, dev.rs:42-73) and the circuit's own constraint system.  `verify` then starts, as dev.rs:581-641 does,
  with every cell that a gate queries where one of its selectors is enabled: CellNotAssigned(gate, region, gate_offset, column,
  offset) unless the region that enabled the selector assigned that cell, InstanceCellNotAssigned(gate, region, gate_offset, column,
  row) for an instance cell past the values given.  These come first, in the order (gate index, position of the selector in the
  gate's queried_selectors, enable order -- region by region, within a region as enabled --, position in the gate's queried_cells).
  (The reference walks regions, then a HashMap of selectors: its order changes from run to run and is not copied.)  The other
  failures follow as above, each with `location`: InRegion(region, offset) for the first region whose assigned rows contain the row
  and whose columns meet the failure's (failure.rs:80-106), else OutsideRegion(row); gate failures carry `constraint` = (gate index,
  gate name, index in the gate, constraint name), print as failure.rs:217-246 does, and list the cells the gate queried in
  VirtualCell's order.  `gate_index` stays the flat polynomial index.  Without regions=True nothing of this exists: the same
  classes, `location` and `constraint` None, the strings above.
* `verify(max_failures=N)` returns at most N failures per kind, the first N in the order above; `failure_counts` is exact.

The checks are three kernels' worth of C ABI (halo2_amd/csrc/mock_prover.hip): `h2_check_expressions_device`,
`h2_lookup_check_device`, `h2_permutation_check_device`.  They leave bit planes and counts on the device; `verify` reads the
counts back once (its only synchronisation) and fetches a plane only for what failed.  The regions' check is a fourth,
`h2_cells_assigned_check`: host records in, host records out, two kernels in between (who assigned each cell; is every queried cell
its region's), with exact counts and the first N failures."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import fields
from ._lib import check, lib
from .arithmetic import _p, _stream_ptr
from .evaluator import _CONST, _LINEAR, _MULADD, _POLY, _SCALE, LAGRANGE, AstLeaf, Evaluator, _as_ast
from .plonk import ConstraintSystem, _Cells


_ANY = {"advice": "Advice", "fixed": "Fixed", "instance": "Instance"}


def _region_str(region) -> str:                                               # metadata.rs:156-160
    return f"Region {region[0]} ('{region[1]}')"


def _gate_str(gate) -> str:                                                   # metadata.rs:96-100
    return f"Gate {gate[0]} ('{gate[1]}')"


def _column_debug(column) -> str:                                             # `{:?}` of plonk::Column
    return f"Column {{ index: {column[1]}, column_type: {_ANY[column[0]]} }}"


def _constraint_str(constraint) -> str:                                       # metadata.rs:122-137
    gate_index, gate_name, index, name = constraint
    return f"Constraint {index}" + (f" ('{name}')" if name else "") + f" in gate {gate_index} ('{gate_name}')"


@dataclass(frozen=True)
class InRegion:
    """FailureLocation::InRegion: region = (index, name); offset from the region's first assigned row."""
    region: tuple
    offset: int

    def __str__(self):                                                        # failure.rs:39
        return f"in {_region_str(self.region)} at offset {self.offset}"


@dataclass(frozen=True)
class OutsideRegion:
    """FailureLocation::OutsideRegion."""
    row: int

    def __str__(self):                                                        # failure.rs:40-42
        return f"outside any region, on row {self.row}"


class FailureLocation:
    """failure.rs:18-107 over `circuit.RegionRecord`s (or anything with .index, .name, .rows and .columns)."""
    InRegion, OutsideRegion = InRegion, OutsideRegion

    @staticmethod
    def find(regions, row: int, columns):
        """failure.rs:80-106: the first region whose rows contain `row` and whose columns meet `columns`, a set of (kind, index); a
        region without an assigned cell never matches."""
        columns = set(columns)
        for r in regions:
            if r.rows is not None and r.rows[0] <= row <= r.rows[1] and any((c.kind, c.index) in columns for c in r.columns):
                return InRegion((r.index, r.name), row - r.rows[0])
        return OutsideRegion(row)


@dataclass(frozen=True)
class CellNotAssigned:
    """VerifyFailure::CellNotAssigned: gate = (index, name), region = (index, name), column = (kind, index).  `gate_offset` is what the
    reference stores, the ABSOLUTE row of the selector (dev.rs:629); `offset` is the cell's row minus the region's first assigned row,
    negative when the gate looks above it.  A region that enabled a selector and assigned nothing has no first row (the reference
    panics on `rows.unwrap()`): its smallest enabled row stands in."""
    gate: tuple
    region: tuple
    gate_offset: int
    column: tuple
    offset: int

    def __str__(self):                                                        # failure.rs:191-203
        return (f"{_region_str(self.region)} uses {_gate_str(self.gate)} at offset {self.gate_offset}, which requires cell in column "
                f"{_column_debug(self.column)} at offset {self.offset} to be assigned.")


@dataclass(frozen=True)
class InstanceCellNotAssigned:
    """VerifyFailure::InstanceCellNotAssigned: as CellNotAssigned; `row` is the absolute row of the instance cell."""
    gate: tuple
    region: tuple
    gate_offset: int
    column: tuple
    row: int

    def __str__(self):                                                        # failure.rs:204-216
        return (f"{_region_str(self.region)} uses {_gate_str(self.gate)} at offset {self.gate_offset}, which requires cell in instance "
                f"column {_column_debug(self.column)} at row {self.row} to be assigned.")


def _format_value(v) -> str:
    """util.rs:58-73.  A failure does not carry its field: -1 is p - 1 of either Pasta field (q - 1 is no element of Fp, and p - 1 as a
    value of Fq is as likely as any other 255-bit number)."""
    if v is None:
        return "poison"
    return "0" if v == 0 else "1" if v == 1 else "-1" if v + 1 in fields.MODULUS.values() else hex(v)


@dataclass(frozen=True)
class ConstraintNotSatisfied:
    """VerifyFailure::ConstraintNotSatisfied.  cell_values: ((kind, column, rotation, canonical value), ...) for every cell the gate
    queries (util::cell_values); the value of a poisoned cell (it met a zero factor) is None.  From a prover that kept its regions:
    location (InRegion / OutsideRegion) and constraint = (gate index, gate name, index within the gate, constraint name);
    `gate_index` stays the flat index of the polynomial."""
    gate_index: int
    row: int
    cell_values: tuple
    location: object = None
    constraint: tuple = None

    def __str__(self):
        if self.location is not None:                                         # failure.rs:217-227
            cells = "".join(f"- Column('{_ANY[kind]}', {col})@{rot} = {_format_value(v)}\n" for kind, col, rot, v in self.cell_values)
            return f"{_constraint_str(self.constraint)} is not satisfied {self.location}\n" + cells
        cells = ", ".join(f"{kind}[{col}]@{rot:+d} = " + ("poison" if v is None else hex(v)) for kind, col, rot, v in self.cell_values)
        return f"Constraint {self.gate_index} is not satisfied on row {self.row}: {cells}"


@dataclass(frozen=True)
class ConstraintPoisoned:
    """VerifyFailure::ConstraintPoisoned: the gate is active on `rows` rows where it reads a blinding row; the first is `first_row`."""
    gate_index: int
    rows: int
    first_row: int
    constraint: tuple = None

    def __str__(self):
        if self.constraint is not None:                                       # failure.rs:228-234
            return f"{_constraint_str(self.constraint)} is active on an unusable row - missing selector?"
        return (f"Constraint {self.gate_index} is active on an unusable row ({self.rows} row(s), first {self.first_row}): "
                "missing selector?")


@dataclass(frozen=True)
class Lookup:
    """VerifyFailure::Lookup: the input tuple of `row` is not in the table."""
    lookup_index: int
    row: int
    location: object = None

    def __str__(self):
        if self.location is not None:                                         # failure.rs:235-238
            return f"Lookup {self.lookup_index} is not satisfied {self.location}"
        return f"Lookup {self.lookup_index} is not satisfied on row {self.row}"


@dataclass(frozen=True)
class Permutation:
    """VerifyFailure::Permutation: the cell of permutation column `column` = (kind, index) at `row` differs from its copy."""
    column: tuple
    row: int
    location: object = None

    def __str__(self):
        if self.location is not None:                                         # failure.rs:239-245; `{:?}` of metadata::Column
            return (f"Equality constraint not satisfied by cell (Column {{ column_type: {_ANY[self.column[0]]}, index: {self.column[1]} }}, "
                    f"{self.location})")
        return f"Equality constraint not satisfied by cell ({self.column[0]}[{self.column[1]}], row {self.row})"


KINDS = ("ConstraintNotSatisfied", "ConstraintPoisoned", "Lookup", "Permutation")
REGION_KINDS = ("CellNotAssigned", "InstanceCellNotAssigned")


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


def cells_assigned_check(k: int, n_planes: int, ranges, instance_lens, event_rows, event_regions, selector_offsets, pair_selector, pair_cells,
                         max_records: int):
    """h2_cells_assigned_check on host arrays.  ranges: (n, 4) of (plane, first row, count, region); the events grouped by selector
    with their CSR offsets; pair_cells: per pair the (column code, rotation) list.  -> (counts: uint64 per pair, records: (m, 3) uint32
    of (pair, event within its selector, cell within its pair), number of conflicting assignments)."""
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)) if a.size else None
    ranges, rows, owners, selectors = u32(ranges).reshape(-1, 4), u32(event_rows), u32(event_regions), u32(pair_selector)
    lens = np.ascontiguousarray(instance_lens, dtype=np.uint64)
    offsets = np.ascontiguousarray(selector_offsets, dtype=np.uintp)
    cell_offsets = np.concatenate([[0], np.cumsum([len(cells) for cells in pair_cells])]).astype(np.uintp)
    flat = [(code, rot & 0xFFFFFFFF) for cells in pair_cells for code, rot in cells]
    cells = np.array(flat, dtype=np.uint32).reshape(-1, 2)
    counts = np.zeros(len(selectors), dtype=np.uint64)
    records = np.zeros((max_records, 3), dtype=np.uint32)
    n_records, conflicts = C.c_size_t(0), C.c_uint64(0)
    sizes = lambda a: a.ctypes.data_as(C.POINTER(C.c_size_t))
    check(lib().h2_cells_assigned_check(k, n_planes, p32(ranges), len(ranges), _p(lens) if lens.size else None, len(lens), p32(rows), p32(owners),
                                        sizes(offsets), len(offsets) - 1, p32(selectors), sizes(cell_offsets), len(selectors), p32(cells),
                                        _p(counts) if counts.size else None, p32(records), max_records, C.byref(n_records), C.byref(conflicts)),
          "h2_cells_assigned_check")
    return counts, records[:n_records.value], int(conflicts.value)


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
        self.regions = self.circuit_cs = self.instance_lens = None
        return self

    @classmethod
    def run_circuit(cls, k: int, circuit, instances, field: int, device=None, regions: bool = False) -> "MockProver":
        """dev.rs:463-574 from a `halo2_amd.circuit.Circuit`: configure, synthesize with the witness (the circuit's floor planner), invert the
        assigned cells' denominators, compress the selectors, lower, `run`.  instances: the instance columns, integer lists.
        regions=True keeps what the reference's prover keeps beside the columns -- the regions synthesis went through (`.regions`,
        `circuit.RegionRecord`s), the circuit's own constraint system with its gates' names, selectors and queried cells
        (`.circuit_cs`) and the instance columns' lengths -- and `verify` then reports unassigned cells and where each failure lies."""
        from . import circuit as front
        instances = [list(col) for col in instances]
        cs, assembly, _ = front.synthesize(circuit, k, field, fixed=True, advice=True, instances=instances, regions=regions)
        fixed = front.fixed_columns_of(assembly, cs, device)
        advice = assembly.columns_to_field(assembly.advice, device)
        self = cls.run(k, front.lower(cs), fixed, advice, instances, assembly.permutation.flat(), field, device)
        if regions:
            self.regions, self.circuit_cs, self.instance_lens = assembly.regions, cs, [len(col) for col in instances]
            self._flat_polys = [(g, p) for g, gate in enumerate(cs.gates) for p in range(len(gate.polys))]
        return self

    # ---- the regions' check (dev.rs:581-641) ------------------------------------------------------------------------------------------
    def region_check_inputs(self):
        """The arrays of h2_cells_assigned_check from the kept regions, in two parts: the cells of fixed and advice columns
        (CellNotAssigned) and the cells of instance columns (InstanceCellNotAssigned), so that each kind has its own cap.
        -> (ranges, events, parts); ranges: (n_ranges, 4) uint32; events: (rows, regions, selector offsets), region-major within a
        selector; parts: two lists of (gate index, position of the selector among the gate's queried_selectors, selector index,
        [(position in queried_cells, column code, rotation)]), in the order (gate, selector position)."""
        n_fixed = len(self.fixed)
        plane = lambda column: column.index + (n_fixed if column.kind == "advice" else 0)
        ranges = np.array([(plane(column), first, count, r.index) for r in self.regions for column, first, count in r.cells],
                          dtype=np.uint32).reshape(-1, 4)
        rows, owners, offsets = [], [], [0]
        for s in range(self.circuit_cs.num_selectors):
            for r in self.regions:
                at = r.enabled_selectors.get(s)
                if at:
                    rows += at
                    owners += [r.index] * len(at)
            offsets.append(len(rows))
        parts = ([], [])
        for g, gate in enumerate(self.circuit_cs.gates):
            plain = [(i, plane(c), rot) for i, (c, rot) in enumerate(gate.queried_cells) if c.kind != "instance"]
            inst = [(i, 0x80000000 | c.index, rot) for i, (c, rot) in enumerate(gate.queried_cells) if c.kind == "instance"]
            for position, selector in enumerate(dict.fromkeys(s.index for s in gate.queried_selectors)):
                for part, cells in zip(parts, (plain, inst)):
                    if cells:
                        part.append((g, position, selector, cells))
        return ranges, (np.array(rows, dtype=np.uint32), np.array(owners, dtype=np.uint32), np.array(offsets, dtype=np.uintp)), parts

    def _check_regions(self, max_failures: int):
        """-> (failures, count of CellNotAssigned, count of InstanceCellNotAssigned): the first `max_failures` of each kind, merged into
        the order (gate, selector position, enable order, position in queried_cells)."""
        ranges, (rows, owners, offsets), parts = self.region_check_inputs()
        n_planes, n_selectors = len(self.fixed) + len(self.advice), self.circuit_cs.num_selectors
        starts = [r.rows[0] if r.rows is not None else min((min(at) for at in r.enabled_selectors.values() if at), default=0)
                  for r in self.regions]
        names = [r.name for r in self.regions]
        lens = np.array(self.instance_lens, dtype=np.uint64)
        found, totals = [], []
        for kind, pairs in enumerate(parts):
            if not pairs:
                totals.append(0)
                continue
            mine = ranges if kind == 0 else ranges[:0]                        # instance cells are in no owner plane
            counts, records, conflicts = cells_assigned_check(self.k, n_planes, mine, lens, rows, owners, offsets,
                                                              [s for _, _, s, _ in pairs],
                                                              [[(code, rot) for _, code, rot in cells] for _, _, _, cells in pairs], max_failures)
            if conflicts:
                raise ValueError(f"{conflicts} cell(s) are assigned by two regions: no floor planner lays regions over each other")
            totals.append(int(counts.sum()))
            for p, e, c in records.tolist():
                g, selector_position, selector, cells = pairs[p]
                position, code, rot = cells[c]
                row, region = int(rows[offsets[selector] + e]), int(owners[offsets[selector] + e])
                gate = self.circuit_cs.gates[g]
                column = gate.queried_cells[position][0]
                cell_row = (row + rot) % self.n
                where = ((g, gate.name), (region, names[region]), row, (column.kind, column.index))
                failure = InstanceCellNotAssigned(*where, cell_row) if kind else CellNotAssigned(*where, cell_row - starts[region])
                found.append(((g, selector_position, e, position), failure))
        found.sort(key=lambda kf: kf[0])
        return [f for _, f in found], totals[0], totals[1]

    def _polynomial_columns(self, expressions) -> set:
        """failure.rs:48-77: the (kind, index) of every column the expressions query."""
        leaf = lambda kind: lambda q: {(kind, q[1])}
        none, union = lambda _: set(), lambda a, b: a | b
        out = set()
        for e in expressions:
            out |= e.evaluate(none, none, leaf("fixed"), leaf("advice"), leaf("instance"), lambda a: a, union, union, lambda a, _: a)
        return out

    def _locate(self, failure):
        """The failure with its FailureLocation and, for a gate, its constraint's names (dev.rs:670-703, :819-827, :870-877)."""
        cs = self.circuit_cs
        if isinstance(failure, (ConstraintNotSatisfied, ConstraintPoisoned)):
            g, p = self._flat_polys[failure.gate_index]
            gate = cs.gates[g]
            constraint = (g, gate.name, p, gate.constraint_names[p])
            if isinstance(failure, ConstraintPoisoned):
                return ConstraintPoisoned(failure.gate_index, failure.rows, failure.first_row, constraint)
            location = FailureLocation.find(self.regions, failure.row, self._polynomial_columns([gate.polys[p]]))
            # util::cell_values: the cells the gate queried (the combined selector's column is not one), in VirtualCell's order
            queried = {(c.kind, c.index, rot) for c, rot in gate.queried_cells}
            order = {"instance": 0, "advice": 1, "fixed": 2}
            values = tuple(sorted((cv for cv in failure.cell_values if cv[:3] in queried), key=lambda cv: (order[cv[0]], cv[1], cv[2])))
            return ConstraintNotSatisfied(failure.gate_index, failure.row, values, location, constraint)
        if isinstance(failure, Lookup):
            columns = self._polynomial_columns(cs.lookups[failure.lookup_index][0])
            return Lookup(failure.lookup_index, failure.row, FailureLocation.find(self.regions, failure.row, columns))
        return Permutation(failure.column, failure.row, FailureLocation.find(self.regions, failure.row, {tuple(failure.column)}))

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
        if self.regions is not None:                                          # dev.rs:883-888: the unassigned cells come first
            unassigned, n_cells, n_instance = self._check_regions(max_failures)
            self._counts = {"CellNotAssigned": n_cells, "InstanceCellNotAssigned": n_instance, **self._counts}
            failures = unassigned + [self._locate(f) for f in failures]
        return failures

    @property
    def failure_counts(self) -> dict:
        """Exact number of failures per kind (KINDS; with regions kept also REGION_KINDS), whatever cap `verify` was given."""
        if self._counts is None:
            self.verify(0)
        return dict(self._counts)

    def assert_satisfied(self) -> None:
        """dev.rs:915-923: raises AssertionError with every failure (up to verify's default cap per kind) printed."""
        failures = self.verify()
        if failures:
            total = sum(self._counts.values())
            raise AssertionError(f"circuit was not satisfied ({total} failure(s)):\n" + "\n".join("  " + str(f) for f in failures))
