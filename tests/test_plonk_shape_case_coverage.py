"""CPU-only: what keeps tests/test_gpu_plonk_shapes.py honest.  (1) Every constraint-system value the list in tests/plonk_shape_cases.py is
there for is reached, by the shapes named here, and what a shape claims is recomputed from its structure by this file's own probe.  (2) Every
shape's degree, blinding factors and declared query lists equal what its gates, lookups and permutation columns give under the reference's rules
(plonk/circuit.rs:1403-1460, plonk/lookup.rs:25-75).  (3) The restated prover and verifier (oracle/plonk.py) alone, on every shape: the proof is
accepted, every broken variant rejected (the lookup variant refused at the permuted columns), the section map sums to the proof's length and a
one-bit flip in every section is rejected -- the conditions under which equality with the restated prover's bytes means anything."""
import pytest

import plonk_shape_cases as cases
from oracle import c_oracle as co
from oracle import ipa
from oracle import plonk as oplonk

SHAPES = cases.SHAPES
IDS = [s.name for s in SHAPES]

# value -> the shapes that reach it.  Asserted as a whole: dropping a shape, or a claim, fails here by name.
REACHED_BY = {
    "rot:advice{0,1,2}": ("fibonacci",),
    "rot:advice{-1,0,1}": ("window_sum",),
    "rot:far": ("far_product", "four_rotations"),
    "rot:fixed!=0": ("far_product",),
    "rot:instance@1": ("window_sum",),
    "rot:four": ("four_rotations", "five_rotations"),
    "bf:5": ("fibonacci", "chain_of_four_sets", "window_sum", "far_product", "three_lookups", "eighth_power", "two_instance_columns",
             "no_advice", "heavy_repeats", "squares_in_two_circuits"),
    "bf:6": ("four_rotations",),
    "bf:7": ("five_rotations",),
    "perm:none": ("fibonacci",),
    "perm:<chunk": ("far_product", "three_lookups", "eighth_power", "heavy_repeats"),
    "perm:=chunk": ("window_sum", "squares_in_two_circuits"),
    "perm:chunk+1": ("four_rotations", "two_instance_columns", "no_advice"),
    "perm:2chunks": ("five_rotations", "two_instance_columns", "no_advice"),
    "perm:deg3x4": ("chain_of_four_sets",),
    "perm:fixed": ("far_product", "three_lookups", "no_advice"),
    "perm:instance": ("window_sum", "two_instance_columns", "no_advice", "squares_in_two_circuits"),
    "perm:cycle-x-chunk": ("chain_of_four_sets", "four_rotations", "five_rotations", "two_instance_columns", "no_advice"),
    "perm:cycle-x-kind": ("window_sum", "far_product", "three_lookups", "two_instance_columns", "no_advice", "squares_in_two_circuits"),
    "lookups:0": ("fibonacci", "chain_of_four_sets", "four_rotations", "five_rotations", "eighth_power", "two_instance_columns", "no_advice"),
    "lookups:1": ("window_sum", "far_product", "heavy_repeats", "squares_in_two_circuits"),
    "lookups:3": ("three_lookups",),
    "lookup:width1": ("window_sum", "far_product", "three_lookups", "heavy_repeats", "squares_in_two_circuits"),
    "lookup:width3": ("three_lookups",),
    "lookup:rotated-input": ("far_product",),
    "lookup:deg2-input": ("far_product", "three_lookups"),
    "lookup:advice-table": ("three_lookups",),
    "lookup:heavy-repeats": ("heavy_repeats",),
    "lookup:several-circuits": ("squares_in_two_circuits",),
    "degree:3": ("fibonacci", "chain_of_four_sets", "two_instance_columns", "no_advice"),
    "degree:4": ("window_sum", "four_rotations", "five_rotations", "heavy_repeats", "squares_in_two_circuits"),
    "degree:5": ("far_product",),
    "degree:6": ("three_lookups",),
    "degree:9": ("eighth_power",),
    "cols:no-instance": ("fibonacci", "far_product", "four_rotations", "five_rotations", "three_lookups", "eighth_power",
                         "heavy_repeats"),
    "cols:two-instance-empty-full": ("two_instance_columns",),
    "cols:unqueried": ("fibonacci",),
    "cols:no-advice": ("no_advice",),
    "curve:vesta": ("fibonacci", "chain_of_four_sets", "far_product", "four_rotations", "three_lookups", "eighth_power", "no_advice"),
    "curve:pallas": ("window_sum", "five_rotations", "two_instance_columns", "heavy_repeats", "squares_in_two_circuits"),
    "circuits:1": ("fibonacci", "window_sum", "far_product", "four_rotations", "five_rotations", "three_lookups", "eighth_power", "no_advice",
                   "heavy_repeats"),
    "circuits:2": ("chain_of_four_sets", "squares_in_two_circuits"),
    "circuits:3": ("two_instance_columns",),
    "k:4": ("fibonacci", "chain_of_four_sets", "eighth_power", "two_instance_columns", "no_advice", "squares_in_two_circuits"),
    "k:5": ("window_sum", "far_product", "four_rotations", "five_rotations", "three_lookups"),
    "k:6": ("heavy_repeats",),
    "broken:gate": ("fibonacci", "chain_of_four_sets", "window_sum", "far_product", "four_rotations", "five_rotations", "three_lookups",
                    "eighth_power", "squares_in_two_circuits"),
    "broken:copy_inside": ("chain_of_four_sets", "window_sum", "far_product", "four_rotations", "five_rotations", "three_lookups", "eighth_power",
                           "heavy_repeats", "squares_in_two_circuits"),
    "broken:copy_across": ("chain_of_four_sets", "four_rotations", "five_rotations", "two_instance_columns", "no_advice"),
    "broken:public": ("chain_of_four_sets", "window_sum", "two_instance_columns", "no_advice", "squares_in_two_circuits"),
    "broken:lookup": ("window_sum", "far_product", "three_lookups", "heavy_repeats", "squares_in_two_circuits"),
}


# ---- this file's own probe: degree and queries of a lowered expression ----------------------------------------------------------------
class _Term:
    """Expression::degree (plonk/circuit.rs:613-626) of what a lowered callable builds."""

    def __init__(self, degree):
        self.degree = degree

    def _other(self, v):
        return v.degree if isinstance(v, _Term) else 0

    def __add__(self, v):
        return _Term(max(self.degree, self._other(v)))

    def __mul__(self, v):
        return _Term(self.degree + self._other(v))

    def __neg__(self):
        return _Term(self.degree)

    __radd__ = __sub__ = __rsub__ = __add__
    __rmul__ = __mul__


class _Recorder:
    def __init__(self):
        self.queries = {"fixed": set(), "advice": set(), "instance": set()}

    def _query(kind):
        def q(self, col, rot=0):
            self.queries[kind].add((col, rot))
            return _Term(1)
        return q

    fixed, advice, instance = _query("fixed"), _query("advice"), _query("instance")


def _probe(expr):
    rec = _Recorder()
    v = expr(rec)
    return (v.degree if isinstance(v, _Term) else 0), rec.queries


def _reference_degree(cs):
    degree = 3                                                                             # permutation::Argument::required_degree
    for ins, tabs in cs.lookups:
        input_degree = max([1] + [_probe(e)[0] for e in ins])
        table_degree = max([1] + [_probe(e)[0] for e in tabs])
        degree = max(degree, 4, 2 + input_degree + table_degree)                          # lookup.rs:65-74
    return max([degree] + [_probe(g)[0] for g in cs.gates])


def _reference_blinding_factors(cs):
    counts = {}
    for col, _ in cs.advice_queries:
        counts[col] = counts.get(col, 0) + 1
    return max(3, max(counts.values(), default=1)) + 2


def _queries_made(cs):
    made = {"fixed": set(), "advice": set(), "instance": set()}
    for e in list(cs.gates) + [e for ins, tabs in cs.lookups for e in list(ins) + list(tabs)]:
        for kind, qs in _probe(e)[1].items():
            made[kind] |= qs
    for kind, col in cs.permutation_columns:                                               # enable_equality queries the column at Rotation::cur()
        made[kind].add((col, 0))
    return made


def _facts(s):
    """The VALUES a shape reaches, from its structure alone."""
    cs, out = s.cs, set()
    rots = {}
    for col, rot in cs.advice_queries:
        rots.setdefault(col, set()).add(rot)
    if {0, 1, 2} in rots.values():
        out.add("rot:advice{0,1,2}")
    if {-1, 0, 1} in rots.values():
        out.add("rot:advice{-1,0,1}")
    if any(abs(r) >= 3 for _, r in cs.advice_queries + cs.fixed_queries + cs.instance_queries):
        out.add("rot:far")
    if any(r != 0 for _, r in cs.fixed_queries):
        out.add("rot:fixed!=0")
    if any(r == 1 for _, r in cs.instance_queries):
        out.add("rot:instance@1")
    if any(len(r) >= 4 for r in rots.values()):
        out.add("rot:four")
    out.add("bf:%d" % cs.blinding_factors)
    n_perm, chunk = len(cs.permutation_columns), cs.degree - 2
    if n_perm == 0:
        out.add("perm:none")
    else:
        out |= {name for name, hit in (("perm:<chunk", n_perm < chunk), ("perm:=chunk", n_perm == chunk), ("perm:chunk+1", n_perm == chunk + 1),
                                       ("perm:2chunks", n_perm == 2 * chunk), ("perm:deg3x4", cs.degree == 3 and n_perm == 4)) if hit}
        kinds = [kind for kind, _ in cs.permutation_columns]
        out |= {"perm:" + kind for kind in kinds if kind != "advice"}
        links = [(c, s.mapping[c][r][0]) for c in range(n_perm) for r in range(s.usable) if s.mapping[c][r] != (c, r)]
        if any(a // chunk != b // chunk for a, b in links):
            out.add("perm:cycle-x-chunk")
        if any(kinds[a] != kinds[b] for a, b in links):
            out.add("perm:cycle-x-kind")
    out.add("lookups:%d" % len(cs.lookups))
    for li, (ins, tabs) in enumerate(cs.lookups):
        out.add("lookup:width%d" % len(ins))
        if any(r != 0 for e in ins for qs in _probe(e)[1].values() for _, r in qs):
            out.add("lookup:rotated-input")
        if any(_probe(e)[0] == 2 for e in ins):
            out.add("lookup:deg2-input")
        if any(_probe(e)[1]["advice"] for e in tabs):
            out.add("lookup:advice-table")
        if len(ins) == 1 and _probe(ins[0])[1]["advice"] and not _probe(tabs[0])[1]["advice"]:
            (col, _), = _probe(ins[0])[1]["advice"]
            (tcol, _), = _probe(tabs[0])[1]["fixed"]
            inputs, table = s.circuits[0][0][col][:s.usable], s.fixed[tcol][:s.usable]
            if _probe(ins[0])[0] == 1 and len(set(table)) * 8 <= s.usable and 2 * max(inputs.count(v) for v in set(inputs)) >= s.usable:
                out.add("lookup:heavy-repeats")
    if cs.lookups and len(s.circuits) > 1:
        out.add("lookup:several-circuits")
    out.add("degree:%d" % cs.degree)
    if cs.num_instance_columns == 0:
        out.add("cols:no-instance")
    if cs.num_instance_columns == 2 and any(sorted(len(c) for c in inst) == [0, s.usable] for _, inst in s.circuits):
        out.add("cols:two-instance-empty-full")
    made = _queries_made(cs)
    if ({c for c, _ in made["advice"]} != set(range(cs.num_advice_columns)) and {c for c, _ in made["fixed"]} != set(range(cs.num_fixed_columns))):
        out.add("cols:unqueried")
    if cs.num_advice_columns == 0:
        out.add("cols:no-advice")
    out |= {"curve:vesta" if s.curve == cases.VESTA else "curve:pallas", "circuits:%d" % len(s.circuits), "k:%d" % s.k}
    out |= {"broken:" + v for v in s.broken}
    return out


# ---- (1) coverage ---------------------------------------------------------------------------------------------------------------------
def test_every_value_is_reached_by_the_shapes_named():
    assert len(SHAPES) <= 16 and len(set(IDS)) == len(IDS)
    assert set(REACHED_BY) == set(cases.VALUES)
    table = cases.value_table()
    lost = {v: sorted(set(REACHED_BY[v]) - set(table[v])) for v in cases.VALUES if set(REACHED_BY[v]) - set(table[v])}
    assert not lost, "no longer reached by: %r" % lost
    assert table == REACHED_BY
    assert all(table[v] for v in cases.VALUES)
    assert all(s.k in (4, 5, 6) for s in SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_shape_reaches_what_it_claims(shape):
    assert _facts(shape) == set(shape.covers)
    assert set(shape.covers) <= set(cases.VALUES)


@pytest.mark.parametrize("dropped", SHAPES, ids=IDS)
def test_dropping_a_shape_is_noticed(dropped):
    table = cases.value_table([s for s in SHAPES if s is not dropped])
    assert [v for v in cases.VALUES if table[v] != REACHED_BY[v]], "the table does not notice that %s is gone" % dropped.name


# ---- (2) consistency --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_degree_blinding_factors_and_queries_follow_the_reference_rules(shape):
    cs = shape.cs
    assert cs.degree == _reference_degree(cs)
    assert cs.blinding_factors == _reference_blinding_factors(cs)
    made = _queries_made(cs)
    for kind, declared in (("fixed", cs.fixed_queries), ("advice", cs.advice_queries), ("instance", cs.instance_queries)):
        assert len(set(declared)) == len(declared), kind
        assert set(declared) == made[kind], kind
    n = shape.n
    assert shape.usable >= cases.PAD + 1 and n - shape.usable == cs.blinding_factors + 1
    assert len(shape.fixed) == cs.num_fixed_columns and all(len(c) == n for c in shape.fixed)
    assert len(shape.mapping) == len(cs.permutation_columns) and all(len(c) == n for c in shape.mapping)
    for advice, instance in shape.circuits:
        assert len(advice) == cs.num_advice_columns and all(len(c) == n for c in advice)
        assert len(instance) == cs.num_instance_columns and all(len(c) <= shape.usable for c in instance)
    # no copy constraint reaches into the rows the prover overwrites
    assert all(shape.mapping[c][r] == (c, r) for c in range(len(shape.mapping)) for r in range(shape.usable, n))


class _RowCells:
    """A lowered expression on plain integers at one row (rotations wrap at n, as the polynomials' do)."""

    def __init__(self, fixed, advice, instance, row, n):
        self.f, self.a, self.i, self.row, self.n = fixed, advice, instance, row, n

    def fixed(self, col, rot=0):
        return self.f[col][(self.row + rot) % self.n]

    def advice(self, col, rot=0):
        return self.a[col][(self.row + rot) % self.n]

    def instance(self, col, rot=0):
        return self.i[col][(self.row + rot) % self.n]


def _violations(s, circuits):
    """Which kinds of constraint the witness breaks on the usable rows, checked on integers: "gate", "lookup", "copy_inside" (a broken link
    between two columns of one permutation set), "copy_across" (between two sets), and "public" beside any of them that reads an instance cell."""
    cs, n, m, out = s.cs, s.n, cases.modulus(s.curve), set()
    chunk = cs.degree - 2
    for advice, instance in circuits:
        instance = [list(c) + [0] * (n - len(c)) for c in instance]
        for row in range(s.usable):
            cells = _RowCells(s.fixed, advice, instance, row, n)
            for gate in cs.gates:
                if int(gate(cells)) % m:
                    out |= {"gate"} | ({"public"} if _probe(gate)[1]["instance"] else set())
        column = {"advice": advice, "fixed": s.fixed, "instance": instance}
        values = [column[kind][idx] for kind, idx in cs.permutation_columns]
        for c, col in enumerate(s.mapping):
            for r, (c2, r2) in enumerate(col):
                if values[c][r] % m != values[c2][r2] % m:
                    out.add("copy_inside" if c // chunk == c2 // chunk else "copy_across")
                    if "instance" in (cs.permutation_columns[c][0], cs.permutation_columns[c2][0]):
                        out.add("public")
        for ins, tabs in cs.lookups:
            at = lambda es, row: tuple(int(e(_RowCells(s.fixed, advice, instance, row, n))) % m for e in es)
            table = {at(tabs, row) for row in range(s.usable)}
            if any(at(ins, row) not in table for row in range(s.usable)):
                out.add("lookup")
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_witness_holds_and_each_variant_breaks_what_it_names(shape):
    assert _violations(shape, shape.circuits) == set()
    for variant in shape.broken:
        broken = _violations(shape, cases.broken_circuits(shape, variant))
        assert variant in broken, (variant, broken)
        if variant.startswith("copy"):                             # the pad cells: a copy constraint and nothing else
            assert broken - {"public"} == {variant}, (variant, broken)


def test_degrees_give_the_extended_domains_and_piece_counts_the_issue_lists():
    from oracle import pasta as o
    for s in SHAPES:
        dom = o.EvaluationDomain(s.cs.degree, s.k, cases.modulus(s.curve))
        assert (dom.extended_k - s.k, dom.quotient_poly_degree) == {3: (1, 2), 4: (2, 3), 5: (2, 4), 6: (3, 5), 9: (3, 8)}[s.cs.degree]


# ---- (3) the oracle alone ---------------------------------------------------------------------------------------------------------------
def _rng(sf, seed):
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


def _setup(s):
    g = co.generate_bases(s.curve, cases.GENERATOR_SEED + s.k, s.n)
    w, u = co.generate_bases(s.curve, 60, 1)[0], co.generate_bases(s.curve, 61, 1)[0]
    return g, w, u, co.field_of_curve(s.curve, "scalar")


def _prove(s, g, w, u, sf, circuits):
    t = ipa.Transcript(s.curve)
    try:
        oplonk.create_proof_many(s.curve, s.k, g, w, u, s.cs, s.fixed, s.mapping, cases.VK_REPR, circuits, _rng(sf, cases.RNG_SEED), t)
    finally:
        _prove.written = len(t.out)
    return bytes(t.out)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_restated_prover_and_verifier_on_the_shape(shape):
    s = shape
    g, w, u, sf = _setup(s)
    vk = oplonk.keygen_vk(s.curve, s.k, g, w, s.cs, s.fixed, s.mapping, cases.VK_REPR)
    verify = lambda circuits, proof: oplonk.verify_proof_many(s.curve, s.k, g, w, u, vk, [inst for _, inst in circuits], proof)
    proof = _prove(s, g, w, u, sf, s.circuits)
    assert verify(s.circuits, proof)
    ranges = cases.sections(s)
    assert ranges[0][1] == 0 and ranges[-1][2] == len(proof)
    assert all(hi > lo and lo % 32 == 0 for _, lo, hi in ranges)
    assert all(a[2] == b[1] for a, b in zip(ranges, ranges[1:]))
    for variant in s.broken:
        circuits = cases.broken_circuits(s, variant)
        if variant == "lookup":
            with pytest.raises(ValueError, match="ConstraintSystemFailure"):
                _prove(s, g, w, u, sf, circuits)
            lo, hi = next((lo, hi) for name, lo, hi in ranges if name == "permuted lookup commitments")
            assert lo <= _prove.written < hi, "refused where the permuted columns are committed"
            continue
        bad = _prove(s, g, w, u, sf, circuits)
        assert len(bad) == len(proof)
        assert not verify(circuits, bad), variant
        if variant == "public":
            assert not verify(circuits, proof) and not verify(s.circuits, bad)
    for name, offset, mask in cases.section_flips(s):
        assert cases.section_at(s, offset) == name
        flipped = bytearray(proof)
        flipped[offset] ^= mask
        assert not verify(s.circuits, bytes(flipped)), name
    assert not verify(s.circuits, proof[:-1]) and not verify(s.circuits, proof + b"\0")
    if len(s.circuits) > 1:
        swapped = [s.circuits[1], s.circuits[0]] + s.circuits[2:]
        assert not verify(swapped, proof)
        assert not verify(s.circuits[:-1], proof)
