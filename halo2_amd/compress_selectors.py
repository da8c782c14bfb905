"""Selector compression, the host half (halo2_proofs/src/plonk/circuit/compress_selectors.rs:51-227): which selectors share a fixed
column, with which roots, and the expression each one is replaced by.  A pure function of the selectors' degrees and of the conflict
matrix; the two loops over rows -- the matrix itself (:103-124) and the combined columns (:180-213) -- are the device's
(`halo2_amd.arithmetic.selector_conflicts` / `selector_combine`)."""
from __future__ import annotations

from dataclasses import dataclass


@dataclass
class SelectorDescription:
    """:6-18 without the activations: they reach `process` as the conflict matrix."""
    selector: int
    max_degree: int      # the largest degree of a gate polynomial holding this simple selector, the selector included; 0: complex or unused


@dataclass
class SelectorAssignment:
    """:23-32, with the root the combined column holds on this selector's rows."""
    selector: int
    combination_index: int
    root: int
    expression: object


def process(descriptions, conflicts, max_degree: int, allocate_fixed_column):
    """:51-227.  descriptions: SelectorDescription per selector; conflicts[i][j] (indexed by `.selector`) is true when selectors i
    and j are enabled on a common row; allocate_fixed_column() returns the query expression of a fresh fixed column.  Returns
    (combinations, assignments): combinations[c] lists the (selector, root) pairs of new column c, in allocation order; one
    SelectorAssignment per selector, in the reference's order."""
    from .circuit import Expression
    descriptions = list(descriptions)
    combinations, assignments = [], []
    if not descriptions:
        return combinations, assignments
    simple = []
    for d in descriptions:                                                    # :73-96: degree 0 first, one column each
        if d.max_degree == 0:
            expression = allocate_fixed_column()
            assignments.append(SelectorAssignment(d.selector, len(combinations), 1, expression))
            combinations.append([(d.selector, 1)])
        else:
            simple.append(d)
    added = [False] * len(simple)
    for i, first in enumerate(simple):                                        # :129-224
        if added[i]:
            continue
        added[i] = True
        if first.max_degree > max_degree:
            raise AssertionError("a selector's gate exceeds the degree bound")  # :134
        d = first.max_degree - 1
        combination = [i]
        for j in range(i + 1, len(simple)):                                   # :144-177
            if d + len(combination) == max_degree:
                break
            if added[j]:
                continue
            if any(conflicts[simple[j].selector][simple[q].selector] for q in combination):
                continue
            new_d = max(d, simple[j].max_degree - 1)
            if new_d + len(combination) + 1 > max_degree:
                continue
            d = new_d
            combination.append(j)
            added[j] = True
        query = allocate_fixed_column()
        index = len(combinations)
        members = []
        for pos, q in enumerate(combination):                                 # :186-222: q * prod_{r != root} (r - q)
            root = pos + 1
            expression = query
            for r in range(1, len(combination) + 1):
                if r != root:
                    expression = expression * (Expression.constant(r) - query)
            assignments.append(SelectorAssignment(simple[q].selector, index, root, expression))
            members.append((simple[q].selector, root))
        combinations.append(members)
    return combinations, assignments
