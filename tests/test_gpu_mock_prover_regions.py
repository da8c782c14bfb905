"""`MockProver.run_circuit(..., regions=True)` on the device at k = 4 .. 6: the reference's `unassigned_cell` with its sentence, absolute
gate offsets against relative cell offsets, instance padding, every failure kind with its location and names, the caps with exact
counts -- and, for every broken circuit, that without the keyword nothing has changed."""
import importlib.util
import os

import pytest

from halo2_amd import dev
from halo2_amd.circuit import Circuit, Value
from halo2_amd.dev import (CellNotAssigned, ConstraintNotSatisfied, InRegion, InstanceCellNotAssigned, Lookup, MockProver, OutsideRegion,
                           Permutation)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP = 0


def _example():
    spec = importlib.util.spec_from_file_location("unassigned_cell", os.path.join(ROOT, "examples", "unassigned_cell.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_unassigned_cell():
    """dev.rs:941-1012, the failure and failure.rs:191-203's sentence; the fix is satisfied."""
    mod = _example()
    prover = MockProver.run_circuit(mod.K, mod.FaultyCircuit(), [], FP, regions=True)
    failures = prover.verify()
    assert failures == [CellNotAssigned(gate=(0, "Equality check"), region=(0, "Faulty synthesis"), gate_offset=1, column=("advice", 1), offset=1)]
    assert str(failures[0]) == ("Region 0 ('Faulty synthesis') uses Gate 0 ('Equality check') at offset 1, which requires cell in column "
                                "Column { index: 1, column_type: Advice } at offset 1 to be assigned.")
    assert prover.failure_counts == {"CellNotAssigned": 1, "InstanceCellNotAssigned": 0, "ConstraintNotSatisfied": 0, "ConstraintPoisoned": 0,
                                     "Lookup": 0, "Permutation": 0}
    with pytest.raises(AssertionError, match="requires cell in column"):
        prover.assert_satisfied()
    MockProver.run_circuit(mod.K, mod.FaultyCircuit(forget_b=False), [], FP, regions=True).assert_satisfied()
    # without the keyword the forgotten cell is invisible, as before
    plain = MockProver.run_circuit(mod.K, mod.FaultyCircuit(), [], FP)
    assert plain.verify() == [] and plain.regions is None and set(plain.failure_counts) == set(dev.KINDS)
    assert mod.main()


# ---- one circuit, broken one way at a time ------------------------------------------------------------------------------------------------
K = 5
PUBLIC = 5
FORGOTTEN = 5                                             # rows of the region that forgets b


class Probe(Circuit):
    """Regions, in order: "first" (row 0), "second" (rows 1 .. 2), "public" (rows 3 .. 4), then with "forgot" a region "forgetful" (rows
    5 .. 9) that enables "eq" on five rows and assigns a alone, and last the table "bits" (0 .. 3).  Gates: 0 "eq" s_eq * (a - b);
    1 "public" s_pub * (a - p); 2 "flags", no selector, f * (1 - f) on the second instance column.  One lookup: b in the table."""

    def __init__(self, broken=None):
        self.broken = broken

    def without_witnesses(self):
        return Probe(self.broken)

    @staticmethod
    def configure(meta):
        a, b = meta.advice_column(), meta.advice_column()
        p, flags = meta.instance_column(), meta.instance_column()
        table = meta.lookup_table_column()
        meta.enable_equality(a)
        s_eq, s_pub = meta.selector(), meta.selector()
        meta.create_gate("eq", lambda q: [("a equals b", q.query_selector(s_eq) * (q.query_advice(a, 0) - q.query_advice(b, 0)))])
        meta.create_gate("public", lambda q: [q.query_selector(s_pub) * (q.query_advice(a, 0) - q.query_instance(p, 0))])

        def bits(q):
            f = q.query_instance(flags, 0)
            return [("flag is a bit", f * (1 - f))]
        meta.create_gate("flags", bits)
        meta.lookup(lambda q: [(q.query_advice(b, 0), table)])
        return dict(a=a, b=b, table=table, s_eq=s_eq, s_pub=s_pub)

    def synthesize(self, cfg, layouter):
        a, b, s_eq, s_pub = cfg["a"], cfg["b"], cfg["s_eq"], cfg["s_pub"]
        known = lambda v: (lambda: Value.known(v))

        def first(region):
            s_eq.enable(region, 0)
            region.assign_advice(b, 0, known(1))
            return region.assign_advice(a, 0, known(1))
        one = layouter.assign_region("first", first)

        def second(region):
            for offset, (va, vb) in enumerate([(9, 9) if self.broken == "lookup" else (2, 2), (3, 2) if self.broken == "gate" else (3, 3)]):
                s_eq.enable(region, offset)
                cell = region.assign_advice(a, offset, known(va))
                region.assign_advice(b, offset, known(vb))
                if offset == 0 and self.broken == "copy":
                    region.constrain_equal(cell.cell(), one.cell())
        layouter.assign_region("second", second)

        def public(region):
            for offset, v in enumerate([PUBLIC, 0]):
                s_pub.enable(region, offset)
                region.assign_advice(a, offset, known(v))
        layouter.assign_region("public", public)
        if self.broken == "forgot":
            def forgetful(region):
                for offset in range(FORGOTTEN):
                    s_eq.enable(region, offset)
                    region.assign_advice(a, offset, known(0))
            layouter.assign_region("forgetful", forgetful)
        layouter.assign_table("bits", lambda t: [t.assign_cell(cfg["table"], i, known(i)) for i in range(4)])


def _instances(broken=None):
    public = [0, 0, 0, PUBLIC] + ([] if broken == "instance" else [0])               # the gate reads rows 3 and 4
    flags = [0, 1, 1, 0, 0, 0, 0, 5 if broken == "outside" else 1]
    return [public, flags]


def _run(broken, regions=True):
    return MockProver.run_circuit(K, Probe(broken), _instances(broken), FP, regions=regions)


def test_the_probe_is_satisfied():
    prover = _run(None)
    prover.assert_satisfied()
    assert [(r.index, r.name, r.rows) for r in prover.regions] == [(0, "first", (0, 0)), (1, "second", (1, 2)), (2, "public", (3, 4)), (3, "bits", (0, 3))]
    assert all(v == 0 for v in prover.failure_counts.values()) and len(prover.failure_counts) == 6


def test_gate_offset_is_absolute_and_offset_relative():
    """The forgetful region starts at row 5: the selector's rows are 5 .. 9, the missing cells' offsets 0 .. 4; max_failures caps the
    list, never the counts."""
    prover = _run("forgot")
    want = [CellNotAssigned((0, "eq"), (3, "forgetful"), 5 + i, ("advice", 1), i) for i in range(FORGOTTEN)]
    assert prover.verify() == want
    assert str(want[2]) == ("Region 3 ('forgetful') uses Gate 0 ('eq') at offset 7, which requires cell in column "
                            "Column { index: 1, column_type: Advice } at offset 2 to be assigned.")
    for cap in (0, 1, FORGOTTEN - 1, FORGOTTEN):
        capped = _run("forgot")
        assert capped.verify(max_failures=cap) == want[:cap]
        assert capped.failure_counts["CellNotAssigned"] == FORGOTTEN and capped.failure_counts["InstanceCellNotAssigned"] == 0
    assert _run("forgot", regions=False).verify() == []


def test_a_short_instance_column():
    """p has four values, the gate is enabled on rows 3 and 4: row 4 is padding (dev.rs:606-619).  a = 0 there, so the gate holds."""
    prover = _run("instance")
    want = InstanceCellNotAssigned((1, "public"), (2, "public"), 4, ("instance", 0), 4)
    assert prover.verify() == [want]
    assert str(want) == ("Region 2 ('public') uses Gate 1 ('public') at offset 4, which requires cell in instance column "
                         "Column { index: 0, column_type: Instance } at row 4 to be assigned.")
    assert prover.failure_counts["InstanceCellNotAssigned"] == 1 and prover.failure_counts["CellNotAssigned"] == 0
    assert _run("instance", regions=False).verify() == []


def _old_strings(failures):
    """What the classes printed before they knew locations."""
    out = []
    for f in failures:
        if isinstance(f, ConstraintNotSatisfied):
            cells = ", ".join(f"{kind}[{col}]@{rot:+d} = " + ("poison" if v is None else hex(v)) for kind, col, rot, v in f.cell_values)
            out.append(f"Constraint {f.gate_index} is not satisfied on row {f.row}: {cells}")
        elif isinstance(f, Lookup):
            out.append(f"Lookup {f.lookup_index} is not satisfied on row {f.row}")
        else:
            out.append(f"Equality constraint not satisfied by cell ({f.column[0]}[{f.column[1]}], row {f.row})")
    return out


def _unchanged_without_regions(broken, located):
    """regions=False: the same classes at the same places, no location, no constraint, the old strings."""
    plain = _run(broken, regions=False).verify()
    assert [type(f) for f in plain] == [type(f) for f in located] and plain
    for old, new in zip(plain, located):
        assert old.location is None and getattr(old, "constraint", None) is None and new.location is not None
        assert old.row == new.row
        if isinstance(old, ConstraintNotSatisfied):
            assert old.gate_index == new.gate_index and set(new.cell_values) <= set(old.cell_values)
            assert old == ConstraintNotSatisfied(old.gate_index, old.row, old.cell_values)
        elif isinstance(old, Lookup):
            assert old == Lookup(new.lookup_index, new.row)
        else:
            assert old == Permutation(new.column, new.row)
    assert [str(f) for f in plain] == _old_strings(plain)
    return plain


def test_a_broken_gate_in_region_1():
    failures = _run("gate").verify()
    want = ConstraintNotSatisfied(0, 2, (("advice", 0, 0, 3), ("advice", 1, 0, 2)), InRegion((1, "second"), 1), (0, "eq", 0, "a equals b"))
    assert failures == [want]
    assert str(want) == ("Constraint 0 ('a equals b') in gate 0 ('eq') is not satisfied in Region 1 ('second') at offset 1\n"
                         "- Column('Advice', 0)@0 = 0x3\n- Column('Advice', 1)@0 = 0x2\n")
    plain = _unchanged_without_regions("gate", failures)
    assert len(plain[0].cell_values) == 3                 # the combined selector's column is a cell of the lowered polynomial


def test_a_gate_without_a_selector_failing_past_all_regions():
    failures = _run("outside").verify()
    want = ConstraintNotSatisfied(2, 7, (("instance", 1, 0, 5),), OutsideRegion(7), (2, "flags", 0, "flag is a bit"))
    assert failures == [want]
    assert str(want) == "Constraint 0 ('flag is a bit') in gate 2 ('flags') is not satisfied outside any region, on row 7\n- Column('Instance', 1)@0 = 0x5\n"
    _unchanged_without_regions("outside", failures)


def test_a_lookup_failure_and_a_copy_failure_with_their_locations():
    failures = _run("lookup").verify()
    assert failures == [Lookup(0, 1, InRegion((1, "second"), 0))]
    assert str(failures[0]) == "Lookup 0 is not satisfied in Region 1 ('second') at offset 0"
    _unchanged_without_regions("lookup", failures)
    failures = _run("copy").verify()
    assert failures == [Permutation(("advice", 0), 0, InRegion((0, "first"), 0)), Permutation(("advice", 0), 1, InRegion((1, "second"), 0))]
    assert str(failures[1]) == ("Equality constraint not satisfied by cell (Column { column_type: Advice, index: 0 }, "
                                "in Region 1 ('second') at offset 0)")
    _unchanged_without_regions("copy", failures)


def test_find_on_the_recorded_regions():
    """failure.rs:80-106 over the prover's own records: the first region that shares a column; the table's rows 0 .. 3 hold no advice."""
    regions = _run(None).regions
    find = dev.FailureLocation.find
    assert find(regions, 2, {("fixed", 0)}) == InRegion((3, "bits"), 2)
    assert find(regions, 2, {("fixed", 0), ("advice", 1)}) == InRegion((1, "second"), 1)
    assert find(regions, 5, {("advice", 0)}) == OutsideRegion(5) and find(regions, 0, {("instance", 0)}) == OutsideRegion(0)
