"""Which NTT pass shapes the GPU sweep of tests/test_gpu_ntt_shapes.py executes, proved on the CPU from the plan file: every shape
(plan kind, first, last, r, logT) that a default plan produces up to 2^28 is reached by the sweep's size lists, except five that exist
only above 2^22 (vectors of 512 MiB and up).  The list of exceptions is a cap: a plan change that adds a shape the sweep does not reach
fails here instead of quietly shrinking what is executed."""
import ntt_shapes as ns

# (kind, first, last, r, logT): the sizes that produce it
NOT_EXECUTED = {
    (0, False, False, 10, 2): [28],
    (0, False, True, 9, 3): [27],
    (0, True, False, 9, 3): [25],
    (0, False, True, 8, 3): [24, 25, 26, 28],
    (1, False, False, 7, 3): [27],
}


def fmt(shapes):
    return sorted(shapes)


def test_the_sweep_reaches_every_default_shape_but_the_listed_five():
    swept, every = ns.swept_shapes(), ns.all_shapes()
    assert len(NOT_EXECUTED) == 5
    missing, extra = every - set(NOT_EXECUTED) - swept, swept - every
    assert not missing, f"default-plan shapes (kind, first, last, r, logT) that no swept size executes: {fmt(missing)}"
    assert not extra, f"swept shapes that no default plan up to 2^{ns.MAX_L} has: {fmt(extra)}"
    assert swept == every - set(NOT_EXECUTED), fmt(swept & set(NOT_EXECUTED))      # a listed shape the sweep does reach comes off the list


def test_the_listed_shapes_exist_only_above_the_sweep():
    for shape, sizes in NOT_EXECUTED.items():
        got = [L for L in range(1, ns.MAX_L + 1) if shape in ns.shapes_of(L, shape[0])]
        assert got == sizes and min(got) > max(ns.SWEEP_PLAN0 + ns.SWEEP_PLAN1), (shape, got)


def test_every_kernel_instantiation_of_a_default_plan_is_swept():
    """The pass kernels are templates over (R, FIRST); logT, `last` and the plan kind are runtime values.  Every (first, r) pair of a default
    plan up to 2^28 -- the five unexecuted shapes included -- runs in the sweep at some size, and no default plan has a later pass
    of 1, 2 or 3 stages (instantiations that only the laboratory's knobs reach)."""
    pairs = lambda shapes: {(first, r) for _, first, _, r, _ in shapes}
    missing = pairs(ns.all_shapes()) - pairs(ns.swept_shapes())
    assert not missing, f"(first, r) instantiations that no swept size executes: {sorted(missing)}"
    short = sorted(s for s in ns.all_shapes() if not s[1] and s[3] <= 3)
    assert not short, short


def test_the_plan_rows_the_sweep_was_chosen_for():
    assert ns.passes(0, 0) == [] and ns.passes(0, 1) == []
    assert ns.passes(9, 0) == [(9, 0)] and ns.passes(9, 1) == [(5, 4), (4, 5)]
    assert ns.passes(10, 1) == [(6, 4), (4, 6)]                                    # 64 columns: wider than the logT knob's 0 .. 5
    assert ns.passes(17, 0) == [(9, 1), (8, 2)] and ns.passes(17, 1) == [(6, 4), (6, 4), (5, 5)]
    assert [L for L in range(1, ns.MAX_L + 1) for k in (0, 1) if any(not f and r == 4 for _, f, _, r, _ in ns.shapes_of(L, k))] == [9, 10]
    assert [r for r, _ in ns.passes(20, 1)] == [8, 6, 6] and [r for r, _ in ns.passes(22, 0)] == [8, 8, 6]


def test_the_sweep_is_every_size_up_to_2_22():
    """A shape names what the kernel is handed, not where in the transform it runs: the same (r, logT) at another size is another first
    stage, tile count and twiddle stride.  So the sweep is every size, and every size below 2^11 (one pass, or under plan 1 at 2^9 and
    2^10 the only 4-stage later passes) carries a shape no other size has."""
    for kind, sizes in ((0, ns.SWEEP_PLAN0), (1, ns.SWEEP_PLAN1)):
        dropped = sorted(set(range(23)) - set(sizes))
        assert not dropped and len(sizes) == len(set(sizes)), f"plan {kind}: sizes 2^L missing from the sweep: L = {dropped}"
        for L in range(1, 11):
            others = ns.shapes([x for x in sizes if x != L], kind)
            assert ns.shapes_of(L, kind) - others, (kind, L)
