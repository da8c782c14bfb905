"""tests/region_model.py held to literal expectations taken from the reference's own tests: `unassigned_cell` (dev.rs:941-1012) and the
behaviour of `FailureLocation::find` (dev/failure.rs:80-106)."""
import region_model as rm

A0, A1, F0 = ("advice", 0), ("advice", 1), ("fixed", 0)


def test_unassigned_cell():
    """dev.rs:941-1012 at K = 4: q enabled at offset 1, a assigned at offset 0, b forgotten.  The gate queries a at Rotation::prev() and b
    at Rotation::cur(); a's cell (row 0) is assigned, b's (row 1) is not."""
    regions = [rm.region_of("Faulty synthesis", [(A0, 0, 1)], {0: [1]})]
    gates = [("Equality check", [0], [(A0, -1), (A1, 0)])]
    got = rm.selector_errors(16, regions, gates, [])
    assert [f for _, f in got] == [("CellNotAssigned", (0, "Equality check"), (0, "Faulty synthesis"), 1, A1, 1)]
    assert [k for k, _ in got] == [(0, 0, 0, 1)]
    # the fix: assign b as well
    fixed = [rm.region_of("Faulty synthesis", [(A0, 0, 1), (A1, 1, 1)], {0: [1]})]
    assert rm.selector_errors(16, fixed, gates, []) == []
    assert fixed[0]["rows"] == (0, 1) and fixed[0]["columns"] == {A0, A1}


def test_gate_offset_is_absolute_and_offset_is_relative_and_signed():
    """dev.rs:615, :629 store *selector_row; :631-632 subtract the region's first assigned row."""
    regions = [rm.region_of("first", [(A0, 0, 4)]), rm.region_of("second", [(A0, 5, 1)], {0: [5]})]
    gates = [("g", [0], [(A0, -1), (A0, 0), (A1, 1)])]
    got = [f for _, f in rm.selector_errors(16, regions, gates, [])]
    assert got == [("CellNotAssigned", (0, "g"), (1, "second"), 5, A0, -1), ("CellNotAssigned", (0, "g"), (1, "second"), 5, A1, 1)]


def test_instance_cells_are_assigned_up_to_the_values_given():
    """dev.rs:606-619: Padding past the instance's length, whatever the region."""
    regions = [rm.region_of("r", [(A0, 2, 1)], {0: [2]})]
    gates = [("g", [0], [(("instance", 0), 0), (("instance", 1), 0), (("instance", 0), 1)])]
    got = [f for _, f in rm.selector_errors(16, regions, gates, [3, 2])]
    assert got == [("InstanceCellNotAssigned", (0, "g"), (0, "r"), 2, ("instance", 1), 2),
                   ("InstanceCellNotAssigned", (0, "g"), (0, "r"), 2, ("instance", 0), 3)]


def test_find_takes_the_first_region_that_shares_a_column():
    """A row inside two regions' extents; only the second holds one of the failure's columns."""
    regions = [rm.region_of("left", [(A0, 0, 8)]), rm.region_of("right", [(A1, 2, 8)])]
    assert rm.find(regions, 4, {A1, F0}) == ("InRegion", (1, "right"), 2)
    assert rm.find(regions, 4, {A0, A1}) == ("InRegion", (0, "left"), 4)
    assert rm.find(regions, 4, {F0}) == ("OutsideRegion", 4)


def test_find_never_matches_a_zero_area_region():
    regions = [rm.region_of("empty", [], {0: [3]}), rm.region_of("real", [(A0, 3, 1)])]
    assert regions[0]["rows"] is None
    assert rm.find(regions, 3, {A0}) == ("InRegion", (1, "real"), 0)
    assert rm.find(regions[:1], 3, {A0}) == ("OutsideRegion", 3)


def test_find_past_every_region():
    regions = [rm.region_of("r", [(A0, 0, 4)])]
    assert rm.find(regions, 4, {A0}) == ("OutsideRegion", 4) and rm.find(regions, 3, {A0}) == ("InRegion", (0, "r"), 3)
    assert rm.find([], 0, {A0}) == ("OutsideRegion", 0)


def test_enable_order_is_region_major():
    regions = [rm.region_of("a", [], {0: [7, 3]}), rm.region_of("b", [], {1: [1], 0: [2]})]
    assert rm.event_bases(regions) == {(0, 0): 0, (1, 1): 0, (1, 0): 2}
    gates = [("g", [1, 0], [(A0, 0)])]
    keys = sorted(k for k, _ in rm.selector_errors(16, regions, gates, []))
    assert keys == [(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 1, 0), (0, 1, 2, 0)]
