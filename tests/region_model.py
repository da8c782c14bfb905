"""The reference's check that every cell an enabled gate queries is assigned (halo2_proofs/src/dev.rs:581-641) and its
`FailureLocation::find` (dev/failure.rs:80-106), restated with the reference's nested loops over plain tuples.  Test infrastructure: the
device check (h2_cells_assigned_check) and `dev.FailureLocation.find` are compared against this, never the other way round.

  region   {"name": str, "columns": set of (kind, index), "rows": (first, last) | None,
            "enabled_selectors": {selector index: [absolute rows, in enable order]}, "cells": set of ((kind, index), row)}
  gate     (name, [selector indices the gate queries], [((kind, index), rotation) of its queried cells])
  instance_lens[c]: how many values instance column c was given; a cell past them is InstanceValue::Padding (dev.rs:298-302)."""


def region_of(name, ranges, enabled_selectors=None):
    """A region from its assignments as ranges ((kind, index), first row, count): the extent and the columns as `update_extent`
    (dev.rs:58-72) leaves them, the cells as a set."""
    cells, columns, rows = set(), set(), None
    for column, first, count in ranges:
        for row in range(first, first + count):
            columns.add(column)
            rows = (row, row) if rows is None else (min(rows[0], row), max(rows[1], row))
            cells.add((column, row))
    return {"name": name, "columns": columns, "rows": rows, "enabled_selectors": dict(enabled_selectors or {}), "cells": cells}


def event_bases(regions):
    """Where each region's enablings of a selector start among all enablings of that selector, regions in order: {(region, selector): n}."""
    seen, bases = {}, {}
    for r_i, r in enumerate(regions):
        for selector, at in r["enabled_selectors"].items():
            bases[(r_i, selector)] = seen.get(selector, 0)
            seen[selector] = seen.get(selector, 0) + len(at)
    return bases


def selector_errors(n, regions, gates, instance_lens):
    """dev.rs:581-641, loop for loop.  -> [(key, failure)] in the reference's iteration order (regions, a region's selectors, gates, rows,
    cells).  failure: ("CellNotAssigned", (gate index, name), (region index, name), gate_offset, column, offset) or
    ("InstanceCellNotAssigned", ..., column, row).  key: (gate index, position of the selector in the gate's list, index of the
    enabling among all enablings of its selector -- region-major --, position of the cell in the gate's list): the order in which this
    project reports them (the reference's own depends on a HashMap).  One deviation, as in `dev.CellNotAssigned`: a region that enabled
    a selector and assigned nothing has no first row (the reference panics on `rows.unwrap()`); its smallest enabled row stands in."""
    bases = event_bases(regions)
    out = []
    for r_i, r in enumerate(regions):
        for selector, at in r["enabled_selectors"].items():
            for gate_index, (gate_name, queried_selectors, queried_cells) in enumerate(gates):
                if selector not in queried_selectors:
                    continue
                for j, selector_row in enumerate(at):
                    gate_row = selector_row
                    for c, (column, rotation) in enumerate(queried_cells):
                        cell_row = (gate_row + n + rotation) % n
                        key = (gate_index, queried_selectors.index(selector), bases[(r_i, selector)] + j, c)
                        head = ((gate_index, gate_name), (r_i, r["name"]), selector_row, column)
                        if column[0] == "instance":
                            if not cell_row < instance_lens[column[1]]:
                                out.append((key, ("InstanceCellNotAssigned",) + head + (cell_row,)))
                        elif (column, cell_row) not in r["cells"]:
                            start = r["rows"][0] if r["rows"] is not None else min(min(rows) for rows in r["enabled_selectors"].values() if rows)
                            out.append((key, ("CellNotAssigned",) + head + (cell_row - start,)))
    return out


def find(regions, failure_row, failure_columns):
    """failure.rs:80-106 -> ("InRegion", (index, name), offset) | ("OutsideRegion", row)."""
    failure_columns = set(failure_columns)
    for r_i, r in enumerate(regions):
        if r["rows"] is not None:
            start, end = r["rows"]
            if start <= failure_row <= end and not failure_columns.isdisjoint(r["columns"]):
                return ("InRegion", (r_i, r["name"]), failure_row - start)
    return ("OutsideRegion", failure_row)
