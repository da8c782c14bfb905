"""Circuits written against `halo2_amd.circuit` for the front-end tests: the reference's `tests/plonk_api.rs` circuit (standard
PLONK with a fifth-wire term and one lookup), its `examples/simple-example.rs` circuit (FieldChip: c = constant * a^2 * b^2), and a
small circuit whose six selectors exercise every branch of selector compression.  Written from the circuits' descriptions."""
from halo2_amd import fields
from halo2_amd.circuit import Assigned, Circuit, Rotation, Value

FP = 0
M = fields.MODULUS[FP]
PLONK_API_A = 2834758237 * fields.zeta(FP) % M


# ---- tests/plonk_api.rs ------------------------------------------------------------------------------------------------------------------
class PlonkApiCircuit(Circuit):
    """a: the witness (None: unknown).  rational: the first wire of every multiplication is assigned as (7a, 7)."""

    def __init__(self, a=None, lookup_table=None, rational: bool = False):
        self.a, self.rational = a, rational
        self.lookup_table = [2, PLONK_API_A, PLONK_API_A, 0] if lookup_table is None else lookup_table

    def without_witnesses(self):
        return PlonkApiCircuit(None, self.lookup_table)

    @staticmethod
    def configure(meta):
        e, a, b = meta.advice_column(), meta.advice_column(), meta.advice_column()
        sf = meta.fixed_column()
        c, d = meta.advice_column(), meta.advice_column()
        p = meta.instance_column()
        for col in (a, b, c):
            meta.enable_equality(col)
        sm, sa, sb, sc, sp = (meta.fixed_column() for _ in range(5))
        sl = meta.lookup_table_column()
        meta.lookup(lambda q: [(q.query_any(a, Rotation.cur()), sl)])

        def combined(q):
            d_ = q.query_advice(d, Rotation.next())
            a_ = q.query_advice(a, Rotation.cur())
            sf_ = q.query_fixed(sf)
            e_ = q.query_advice(e, Rotation.prev())
            b_ = q.query_advice(b, Rotation.cur())
            c_ = q.query_advice(c, Rotation.cur())
            sa_, sb_, sc_, sm_ = q.query_fixed(sa), q.query_fixed(sb), q.query_fixed(sc), q.query_fixed(sm)
            return [a_ * sa_ + b_ * sb_ + a_ * b_ * sm_ - (c_ * sc_) + sf_ * (d_ * e_)]
        meta.create_gate("Combined add-mult", combined)

        def public(q):
            a_ = q.query_advice(a, Rotation.cur())
            p_ = q.query_instance(p, Rotation.cur())
            sp_ = q.query_fixed(sp)
            return [sp_ * (a_ - p_)]
        meta.create_gate("Public input", public)
        for col in (sf, e, d, p, sm, sa, sb, sc, sp):
            meta.enable_equality(col)
        return dict(a=a, b=b, c=c, d=d, e=e, sa=sa, sb=sb, sc=sc, sm=sm, sp=sp, sl=sl)

    @staticmethod
    def _raw(layouter, cfg, name, f, fixed):
        """One row: wires (a, b, c) = f(), d = a^4, e = b^4, and the four fixed coefficients."""
        def assign(region):
            value = []

            def first():
                value.append(f())
                return value[0].map(lambda v: v[0])
            lhs = region.assign_advice(cfg["a"], 0, first)
            region.assign_advice(cfg["d"], 0, lambda: value[0].map(lambda v: v[0]).square().square())
            rhs = region.assign_advice(cfg["b"], 0, lambda: value[0].map(lambda v: v[1]))
            region.assign_advice(cfg["e"], 0, lambda: value[0].map(lambda v: v[1]).square().square())
            out = region.assign_advice(cfg["c"], 0, lambda: value[0].map(lambda v: v[2]))
            for col, v in zip(("sa", "sb", "sc", "sm"), fixed):
                region.assign_fixed(cfg[col], 0, lambda v=v: Value.known(v))
            return lhs.cell(), rhs.cell(), out.cell()
        return layouter.assign_region(name, assign)

    def synthesize(self, cfg, layouter):
        def public_input(region):
            region.assign_advice(cfg["a"], 0, lambda: Value.known(2))
            region.assign_fixed(cfg["sp"], 0, lambda: Value.known(1))
        layouter.assign_region("public_input", public_input)

        def copy(left, right):
            def both(region):
                region.constrain_equal(left, right)
                region.constrain_equal(left, right)
            layouter.assign_region("copy", both)
        for _ in range(10):
            a = Value(None if self.a is None else Assigned.trivial(self.a, M))
            first = a if not (self.rational and self.a is not None) else Value(Assigned.rational(7 * self.a, 7, M))
            a_squared = a.square()
            a0, _, c0 = self._raw(layouter, cfg, "raw_multiply", lambda: first.zip(a).zip(a_squared).map(lambda t: (t[0][0], t[0][1], t[1])),
                                  (0, 0, 1, 1))
            fin = a_squared + a
            a1, b1, _ = self._raw(layouter, cfg, "raw_add", lambda: a.zip(a_squared).zip(fin).map(lambda t: (t[0][0], t[0][1], t[1])),
                                  (1, 1, 1, 0))
            copy(a0, a1)
            copy(b1, c0)

        def table(t):
            for index, value in enumerate(self.lookup_table):
                t.assign_cell(cfg["sl"], index, lambda value=value: Value.known(value))
        layouter.assign_table("", table)


# ---- examples/simple-example.rs -----------------------------------------------------------------------------------------------------------
class SimpleExampleCircuit(Circuit):
    """FieldChip: load a, b and the constant, three multiplications, expose c = constant * a^2 * b^2."""

    def __init__(self, constant, a=None, b=None):
        self.constant, self.a, self.b = constant, a, b

    def without_witnesses(self):
        return SimpleExampleCircuit(self.constant)

    @staticmethod
    def configure(meta):
        advice = [meta.advice_column(), meta.advice_column()]
        instance = meta.instance_column()
        constant = meta.fixed_column()
        meta.enable_equality(instance)
        meta.enable_constant(constant)
        for col in advice:
            meta.enable_equality(col)
        s_mul = meta.selector()

        def mul(q):
            lhs = q.query_advice(advice[0], Rotation.cur())
            rhs = q.query_advice(advice[1], Rotation.cur())
            out = q.query_advice(advice[0], Rotation.next())
            return [q.query_selector(s_mul) * (lhs * rhs - out)]
        meta.create_gate("mul", mul)
        return dict(advice=advice, instance=instance, s_mul=s_mul)

    def synthesize(self, cfg, layouter):
        a0, a1 = cfg["advice"]
        load = lambda v: layouter.assign_region("load private", lambda region: region.assign_advice(a0, 0, lambda: Value(v)))
        a, b = load(self.a), load(self.b)
        constant = layouter.assign_region("load constant", lambda region: region.assign_advice_from_constant(a0, 0, self.constant))

        def mul(x, y):
            def assign(region):
                cfg["s_mul"].enable(region, 0)
                x.copy_advice(region, a0, 0)
                y.copy_advice(region, a1, 0)
                return region.assign_advice(a0, 1, lambda: x.value() * y.value())
            return layouter.assign_region("mul", assign)
        ab = mul(a, b)
        absq = mul(ab, ab)
        c = mul(constant, absq)
        layouter.constrain_instance(c.cell(), cfg["instance"], 0)


# ---- five simple selectors and a complex one ---------------------------------------------------------------------------------------------
class SelectorCircuit(Circuit):
    """Rows, one region each: (add and eq together) 3 + 3 = 6, 3 == 3 | mul 3 * 4 = 12 | bool 1 | dbl 5 + 5 = 10 | complex 7 * 7 = 49 |
    add 6 + 1 = 7 with its first wire copied from the first row's sum.  Degree bound 3: add (degree 2) conflicts with eq and takes
    dbl into its column; mul and bool (degree 3) never share; the complex selector gets a column of its own first.
    bad=True breaks the multiplication (gate 1, row 1)."""
    K = 6
    MUL_GATE, MUL_ROW = 1, 1

    def __init__(self, witness: bool = True, bad: bool = False):
        self.witness, self.bad = witness, bad

    def without_witnesses(self):
        return SelectorCircuit(False)

    @staticmethod
    def configure(meta):
        a, b, c = meta.advice_column(), meta.advice_column(), meta.advice_column()
        meta.enable_equality(a)
        meta.enable_equality(c)
        s_add, s_mul, s_bool, s_eq, s_dbl = (meta.selector() for _ in range(5))
        s_cx = meta.complex_selector()
        cur = lambda q: (q.query_advice(a, 0), q.query_advice(b, 0), q.query_advice(c, 0))

        def gate(name, selector, body):
            def build(q):
                wa, wb, wc = cur(q)
                return [q.query_selector(selector) * body(wa, wb, wc)]
            meta.create_gate(name, build)
        gate("add", s_add, lambda wa, wb, wc: wa + wb - wc)
        gate("mul", s_mul, lambda wa, wb, wc: wa * wb - wc)
        gate("bool", s_bool, lambda wa, wb, wc: wa * (1 - wa))
        gate("eq", s_eq, lambda wa, wb, wc: wa - wb)
        gate("dbl", s_dbl, lambda wa, wb, wc: wa + wa - wc)

        def complex_gate(q):
            wa, _, wc = cur(q)
            s = q.query_selector(s_cx)
            return [s * (wa * wa) - s * wc]                    # a complex selector may appear in a sum
        meta.create_gate("complex", complex_gate)
        return dict(a=a, b=b, c=c, add=s_add, mul=s_mul, bool=s_bool, eq=s_eq, dbl=s_dbl, cx=s_cx)

    def synthesize(self, cfg, layouter):
        def row(selectors, va, vb, vc, copy_from=None):
            def assign(region):
                for s in selectors:
                    cfg[s].enable(region, 0)
                val = lambda v: (lambda: Value(v if self.witness else None))
                wa = region.assign_advice(cfg["a"], 0, val(va))
                region.assign_advice(cfg["b"], 0, val(vb))
                wc = region.assign_advice(cfg["c"], 0, val(vc))
                if copy_from is not None:
                    region.constrain_equal(wa.cell(), copy_from.cell())
                return wc
            return layouter.assign_region("+".join(selectors), assign)
        total = row(("add", "eq"), 3, 3, 6)
        row(("mul",), 3, 4, 13 if self.bad else 12)
        row(("bool",), 1, 0, 0)
        row(("dbl",), 5, 0, 10)
        row(("cx",), 7, 0, 49)
        row(("add",), 6, 1, 7, copy_from=total)
