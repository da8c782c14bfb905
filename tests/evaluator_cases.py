"""What the evaluation kernels are run on (a helper: nothing here is collected).

`ev_run` (csrc/evaluator.hip) and its copy in the MockProver, `mp_check` (csrc/mock_prover.hip), interpret post-order bytecode with a
nine-slot stack per element: the top in registers, eight spilled levels in LDS.  CASES lists programs that between them reach every
opcode at every stack depth it can legally have, every rotation that wraps somewhere interesting, the field's extreme values, the
LINEAR term at every length, and the launch shapes (one workgroup, two, eight).  A case is either
  * an `Ast` builder with its oracle/evaluator.py tuple tree, run through EvaluationDomain / Evaluator, or
  * a hand-written program for the C ABI (what the Python compiler never emits: length 1, a chosen root of unity, a chosen depth).
Everything is independent of the field: constants are integers reduced modulo the field at `materialize` (-1 is p - 1), polynomials
are recipes.  tests/test_evaluator_case_coverage.py proves on the CPU what the list reaches and that tests/evaluator_model.py agrees
with the oracle on it; tests/test_gpu_evaluator_shapes.py runs it on the device."""
import functools
import random
from types import SimpleNamespace

import evaluator_model as em
import halo2_amd as h
from halo2_amd import evaluator as hev
from halo2_amd import fields
from halo2_amd.evaluator import COEFF, EXTENDED, LAGRANGE, Ast, AstLeaf, Evaluator, LateConstant
from oracle import evaluator as oev

POLY, CONST, LINEAR, ADD, MUL, SCALE, MULADD = hev._POLY, hev._CONST, hev._LINEAR, hev._ADD, hev._MUL, hev._SCALE, hev._MULADD
PUSHES, BINARIES = (POLY, CONST, LINEAR), (ADD, MUL, MULADD)
BASES = (COEFF, LAGRANGE, EXTENDED)
BASIS_NAME = {COEFF: "coeff", LAGRANGE: "lagrange", EXTENDED: "extended"}
FIELDS = (h.FP, h.FQ)
MAX_DEPTH = em.SPILL_LEVELS + 1

LOG_LENS = (1, 2, 6, 8, 9, 11)                 # 2^8 is exactly one 256-lane workgroup, 2^9 two, 2^11 eight
# extended basis: the cs.degree() values j whose domain has this extended length; step = 2^(extended_k - k) is 2, 4, 8 for j = 3, 5, 9
EXT_JS = {1: (3,), 2: (3, 5), 6: (9,), 8: (5,), 9: (3, 9), 11: (5, 9)}
STEP_OF_J = {3: 2, 5: 4, 9: 8}

Y = 0x1D2C3B4A5968778695A4B3C2D1E0F00112233445566778899AABBCCDDEEFF01       # a challenge-like scalar, below both moduli


def word(op, arg=0):
    return op | arg << 8


def u32(shift):
    return shift & 0xFFFFFFFF


def instructions(words):
    """[(opcode, operand)] of a program, the shift words of its POLY instructions left out."""
    out, pc = [], 0
    while pc < len(words):
        out.append((words[pc] & 0xFF, words[pc] >> 8))
        pc += 2 if words[pc] & 0xFF == POLY else 1
    return out


def poly_reads(words):
    """[(polynomial, signed element shift)] of a program's POLY instructions, in order."""
    out, pc = [], 0
    while pc < len(words):
        if words[pc] & 0xFF == POLY:
            out.append((words[pc] >> 8, em.signed(words[pc + 1])))
            pc += 1
        pc += 1
    return out


class Case:
    """name; basis; log_len (of the vector the kernel sees); polys: one recipe per registered polynomial -- ("random", seed), "zero",
    "pm1" (all p - 1), "alt" (0 and p - 1 alternating), "last1" (1 at len - 1 only).
    Ast cases: build(leaves) -> (Ast, oracle tree), j = cs.degree() of the domain.  C ABI cases: words, consts (integers, reduced at
    materialize), step (what one rotation is in elements, for the shift classes), omega_pow (the root handed over is omega^omega_pow).
    tags: what the case is in the list for."""

    def __init__(self, name, basis, log_len, polys, build=None, j=3, words=None, consts=(), step=1, omega_pow=1, tags=()):
        assert (build is None) != (words is None)
        self.name, self.basis, self.log_len, self.polys, self.build, self.j = name, basis, log_len, list(polys), build, j
        self.words, self.consts, self.omega_pow, self.tags = words, list(consts), omega_pow, set(tags)
        self.step = step if build is None else (STEP_OF_J[j] if basis == EXTENDED else 1)
        self.is_ast = build is not None

    def domain(self, field):
        """The EvaluationDomain of an Ast case."""
        k = self.log_len - (self.step.bit_length() - 1 if self.basis == EXTENDED else 0)
        dom = h.EvaluationDomain(self.j, k, field)
        assert (dom.extended_len() if self.basis == EXTENDED else dom.n) == 1 << self.log_len
        return dom

    def __repr__(self):
        return self.name


def poly_values(recipe, n, m, salt):
    if recipe == "zero":
        return [0] * n
    if recipe == "pm1":
        return [m - 1] * n
    if recipe == "alt":
        return [0 if i % 2 == 0 else m - 1 for i in range(n)]
    if recipe == "last1":
        return [0] * (n - 1) + [1]
    kind, seed = recipe
    assert kind == "random"
    rnd = random.Random(f"{salt}/{seed}")
    return [rnd.randrange(m) for _ in range(n)]


def primitive_root(field, log_len, power=1):
    """A primitive 2^log_len-th root of unity: the field's 2^32-th root squared down, to an odd power."""
    assert power % 2 == 1
    m = fields.MODULUS[field]
    w = fields.root_of_unity(field)
    for _ in range(log_len, fields.S):
        w = w * w % m
    w = pow(w, power, m)
    assert log_len == 0 or pow(w, 1 << (log_len - 1), m) == m - 1                 # the kernel relies on omega^(len/2) = -1
    return w


def _fake_evaluator(basis, n, n_polys):
    ev = Evaluator(basis)
    ev.polys = [SimpleNamespace(shape=(n, 4)) for _ in range(n_polys)]            # the compiler only needs to know they exist
    return ev


@functools.lru_cache(maxsize=None)
def _materialize(name, field):
    case = BY_NAME[name]
    m, n = fields.MODULUS[field], 1 << case.log_len
    out = SimpleNamespace(case=case, field=field, m=m, n=n, tree=None, dom=None)
    out.polys = [poly_values(r, n, m, name) for r in case.polys]
    if case.is_ast:
        dom = out.dom = case.domain(field)
        ev = _fake_evaluator(case.basis, n, len(case.polys))
        ast, out.tree = case.build([AstLeaf(ev, i) for i in range(len(case.polys))])
        out.words, out.consts = [], []
        ev._compile(hev._as_ast(ast), dom, out.words, out.consts)
        out.omega = dom.extended_omega if case.basis == EXTENDED else dom.omega
    else:
        out.words, out.consts = list(case.words), [c % m for c in case.consts]
        out.omega = primitive_root(field, case.log_len, case.omega_pow)
    out.trace = em.Trace()
    out.values, out.depth = em.interpret(out.words, out.consts, out.polys, case.basis, n, m, out.omega, out.trace)
    return out


def materialize(case, field):
    """The case over one field: polys (integers), words, consts, omega, dom and tree (Ast cases), and the model's run of the program --
    values, depth, trace.  Computed once per process and shared: treat it as read-only."""
    return _materialize(case.name, field)


def oracle_values(mat):
    """oracle/evaluator.py on an Ast case's tuple tree."""
    d = mat.dom
    return oev.evaluate(mat.tree, mat.polys, mat.case.basis, mat.m, d.k, d.extended_k, d.omega, d.extended_omega, d.g_coset)


# ---- the stack: every opcode at every depth -----------------------------------------------------------------------------------------
def staircase(basis, push_kinds, s, t, step, seed):
    """(words, consts, n_polys).  Nine pushes with a SCALE after each climb to the full stack (pushes with 0 .. 8 values below them, SCALE
    with 1 .. 9); then a sawtooth -- two binary nodes, one push -- walks back down, so that binary nodes run with 9 .. 2 values, pushes
    spill the running value into level 6, 5, ... 0 in turn, and the node after each push reads that level back.  The push with d values
    on the stack is push_kinds[(d + s) mod len], the binary node with d values is the basis' binaries[(d + t) mod len]: s and t over
    their ranges reach every pair.  Every POLY is another polynomial, every constant another value, so a read or write of the wrong
    level changes the result."""
    binaries = (ADD, MULADD) if basis == COEFF else BINARIES
    rnd = random.Random(seed)
    st = SimpleNamespace(words=[], consts=[], n_polys=0, depth=0)

    def const():
        st.consts.append(rnd.randrange(2, 1 << 250))
        return len(st.consts) - 1

    def push():
        kind = push_kinds[(st.depth + s) % len(push_kinds)]
        if kind == POLY:
            st.words += [word(POLY, st.n_polys), u32(0 if basis == COEFF else (st.depth - 4) * step)]
            st.n_polys += 1
        else:
            st.words.append(word(kind, const()))
        st.depth += 1

    def binary():
        kind = binaries[(st.depth + t) % len(binaries)]
        st.words.append(word(kind, const() if kind == MULADD else 0))
        st.depth -= 1

    for _ in range(MAX_DEPTH):
        push()
        st.words.append(word(SCALE, const()))
    while st.depth > 2:
        binary()
        binary()
        push()
    binary()
    assert st.depth == 1
    return st.words, st.consts, st.n_polys


def _stack_cases():
    out = []
    for basis in BASES:
        for log_len in (9, 11):
            for v in range(3):
                step = 4 if basis == EXTENDED else 1
                words, consts, n_polys = staircase(basis, PUSHES, v, v, step, f"stack/{basis}/{v}")
                out.append(Case(f"stack-{BASIS_NAME[basis]}-L{log_len}-v{v}", basis, log_len, [("random", i) for i in range(n_polys)],
                                words=words, consts=consts, step=step, tags={"stack"}))
    return out


MOCK_LOG_LEN = 9
MOCK_UNUSABLE = 37                       # usable_rows = len - 37 in the poisoned run
MOCK_ADVICE = (3, 4)                     # the two registered polynomials marked advice there


def _mock_cases():
    """The Lagrange staircases without LINEAR: what h2_check_expressions_device accepts.  They run through the evaluator like every other
    case and, the three of them in one launch, through the MockProver kernel."""
    out = []
    for v in range(3):
        words, consts, n_polys = staircase(LAGRANGE, (POLY, CONST), v % 2, v, 1, f"mock/{v}")
        out.append(Case(f"mockstack-L{MOCK_LOG_LEN}-v{v}", LAGRANGE, MOCK_LOG_LEN, [("random", i) for i in range(n_polys)], words=words, consts=consts,
                        tags={"stack", "mock"}))
    return out


@functools.lru_cache(maxsize=None)
def mock_programs(field):
    """The MockProver launch: (programs, offsets, consts, polys) of the three programs over one constant table and one polynomial table."""
    mats = [materialize(c, field) for c in CASES if "mock" in c.tags]
    programs, offsets, consts = [], [0], []
    for mat in mats:
        for w in _relocate(mat.words, len(consts)):
            programs.append(w)
        consts += mat.consts
        offsets.append(len(programs))
    n_polys = max(len(mat.polys) for mat in mats)
    polys = [poly_values(("random", i), mats[0].n, mats[0].m, "mock-shared") for i in range(n_polys)]
    return programs, offsets, consts, polys


@functools.lru_cache(maxsize=None)
def mock_model(field, poisoned):
    """The model's run of the MockProver launch: [(values, trace)] per program; with `poisoned`, MOCK_ADVICE are advice columns and the last
    MOCK_UNUSABLE rows are not usable, and entries of `values` are em.POISON where the kernel must report Poison."""
    programs, offsets, consts, polys = mock_programs(field)
    n, m = len(polys[0]), fields.MODULUS[field]
    runs = []
    for p in range(len(offsets) - 1):
        trace = em.Trace()
        kw = dict(advice=set(MOCK_ADVICE), usable=n - MOCK_UNUSABLE) if poisoned else {}
        values, _ = em.interpret(programs[offsets[p]:offsets[p + 1]], consts, polys, LAGRANGE, n, m, None, trace, **kw)
        runs.append((values, trace))
    return runs


def _relocate(words, base):
    """The program with its constant indices moved up by `base`."""
    out, i = [], 0
    while i < len(words):
        op, arg = words[i] & 0xFF, words[i] >> 8
        if op == POLY:
            out += [words[i], words[i + 1]]
            i += 2
            continue
        out.append(word(op, arg + base) if op in (CONST, LINEAR, SCALE, MULADD) else words[i])
        i += 1
    return out


# ---- rotations ----------------------------------------------------------------------------------------------------------------------
def shift_classes(shift, n, step, basis):
    """The names under which an element shift counts towards coverage (a shift can have several at a small length)."""
    a, sign = abs(shift), "+" if shift > 0 else "-"
    names = []
    if shift == 0:
        return names
    for name, size in (("rot1", step), ("half", n // 2), ("len-step", n - step), ("len", n)):
        if a == size:
            names.append(sign + name)
    if n >= 512 and a in (255, 256, 257):
        names.append(sign + str(a))
    return names


def wanted_shift_classes(basis, log_len):
    names = ["rot1", "half", "len-step", "len"]
    if log_len >= 9:
        names += ["255", "256", "257"] if basis == LAGRANGE else ["256"]
    return {sign + name for name in names for sign in "+-"}


def _shift_builder(basis, log_len, step):
    n = 1 << log_len
    sizes = {step, n // 2, n - step, n}
    if n >= 512:
        sizes |= {255, 256, 257} if basis == LAGRANGE else {256}
    shifts = sorted(sign * e for e in sizes for sign in (1, -1))
    assert all(e % step == 0 for e in shifts)

    def build(leaves):
        """sum_q c_q * poly_(q mod 2) rotated by shift q: a term at the wrong element is a wrong sum (the c_q differ)."""
        rnd = random.Random(f"shifts/{basis}/{log_len}")
        ast = tree = None
        for q, e in enumerate(shifts):
            c, rot = rnd.randrange(2, 1 << 250), e // step
            term, tterm = Ast.of(leaves[q % 2].with_rotation(rot)) * c, ("scale", ("poly", q % 2, rot), c)
            ast, tree = (term, tterm) if ast is None else (ast + term, ("add", tree, tterm))
        return ast, tree
    return build


def _product_builder(basis, log_len, step):
    def build(leaves):
        """One polynomial at five rotations inside one product, plus another at two."""
        a, b, half = leaves[0], leaves[1], (1 << log_len) // 2 // step
        rots = (0, 1, -1, half, -2)
        ast, tree = Ast.of(a.with_rotation(rots[0])), ("poly", 0, rots[0])
        for r in rots[1:]:
            ast, tree = ast * Ast.of(a.with_rotation(r)), ("mul", tree, ("poly", 0, r))
        ast = ast + Ast.of(b.with_rotation(2)) * Ast.of(b.with_rotation(-half))
        tree = ("add", tree, ("mul", ("poly", 1, 2), ("poly", 1, -half)))
        return ast, tree
    return build


def _shift_cases():
    out = []
    two = [("random", 0), ("random", 1)]
    for log_len in LOG_LENS[1:]:                                               # every len >= 4
        out.append(Case(f"shifts-lagrange-L{log_len}", LAGRANGE, log_len, two, build=_shift_builder(LAGRANGE, log_len, 1), tags={"shifts"}))
        for j in (EXT_JS[log_len] if log_len >= 9 else EXT_JS[log_len][:1]):
            out.append(Case(f"shifts-extended-L{log_len}-j{j}", EXTENDED, log_len, two, build=_shift_builder(EXTENDED, log_len, STEP_OF_J[j]),
                            j=j, tags={"shifts"}))
    out.append(Case("product-lagrange-L9", LAGRANGE, 9, two, build=_product_builder(LAGRANGE, 9, 1), tags={"shifts"}))
    out.append(Case("product-extended-L9-j5", EXTENDED, 9, two, build=_product_builder(EXTENDED, 9, 4), j=5, tags={"shifts"}))
    # a single element: +1 and -1 are rotations by the whole length (C ABI only: no domain is that small in the extended basis)
    out.append(Case("shifts-lagrange-L0", LAGRANGE, 0, two, words=[word(POLY, 0), u32(1), word(POLY, 1), u32(-1), word(MUL), word(POLY, 1), 0,
                                                                  word(MULADD, 0)], consts=[Y], tags={"shifts"}))
    return out


# ---- the field's extreme values -----------------------------------------------------------------------------------------------------
EXTREME_POLYS = ["zero", "pm1", "alt", "last1", ("random", 0)]
EXTREME_CONSTS = (0, 1, -1)


def _values_builder(basis):
    def build(leaves):
        """Every pair of the extreme polynomials under ADD and MUL, each under SCALE by and ADD / MUL with the constants 0, 1, p - 1, each pair
        folded by MULADD with the bases 0 and p - 1; the terms folded once more with powers of Y, so that one wrong term is a wrong result."""
        terms = []
        idx = range(len(leaves))
        P = lambda i: (Ast.of(leaves[i]), ("poly", i, 0))
        K = lambda c: (Ast.constant(c), ("constant", c))
        for i in idx:
            for k in idx:
                (a, ta), (b, tb) = P(i), P(k)
                terms.append((a + b, ("add", ta, tb)))
                if basis != COEFF:
                    terms.append((a * b, ("mul", ta, tb)))
                for base in (0, -1):
                    terms.append((Ast.distribute_powers([a, b], base), ("distribute", [ta, tb], base)))
            for c in EXTREME_CONSTS:
                (a, ta), (kc, tkc) = P(i), K(c)
                terms.append((a * c, ("scale", ta, c)))
                terms.append((a + kc, ("add", ta, tkc)))
                if basis != COEFF:
                    terms.append((a * kc, ("mul", ta, tkc)))
                for base in (0, -1):
                    terms.append((Ast.distribute_powers([kc, a, kc], base), ("distribute", [tkc, ta, tkc], base)))
        for c in EXTREME_CONSTS:
            for d in EXTREME_CONSTS:
                (kc, tkc), (kd, tkd) = K(c), K(d)
                terms.append((kc + kd, ("add", tkc, tkd)))
                terms.append((kc * d, ("scale", tkc, d)))
                if basis != COEFF:
                    terms.append((kc * kd, ("mul", tkc, tkd)))
        return Ast.distribute_powers([t[0] for t in terms], Y), ("distribute", [t[1] for t in terms], Y)
    return build


def _value_cases():
    return [Case(f"values-{BASIS_NAME[basis]}-L{log_len}", basis, log_len, EXTREME_POLYS, build=_values_builder(basis), j=5, tags={"values"})
            for basis, log_len in ((COEFF, 6), (LAGRANGE, 6), (EXTENDED, 6), (LAGRANGE, 9))]


# ---- LINEAR -------------------------------------------------------------------------------------------------------------------------
LINEAR_RANDOM = 0x2F0E1D3C5B7A99887766554433221100FFEEDDCCBBAA99887766554433221101
LINEAR_CONSTS = (0, 1, -1, LINEAR_RANDOM)


def _linear_build(leaves):
    """((poly + 0 * w^i) * Y + 1 * w^i) * Y + (p - 1) * w^i) * Y + r * w^i: four LINEAR nodes, each with a different weight in the result."""
    terms = [(Ast.linear(LINEAR_CONSTS[0]) + Ast.of(leaves[0]), ("add", ("linear", LINEAR_CONSTS[0]), ("poly", 0, 0)))]
    terms += [(Ast.linear(c), ("linear", c)) for c in LINEAR_CONSTS[1:]]
    return Ast.distribute_powers([t[0] for t in terms], Y), ("distribute", [t[1] for t in terms], Y)


def _linear_cases():
    out = []
    one = [("random", 0)]
    for log_len in LOG_LENS:
        out.append(Case(f"linear-coeff-L{log_len}", COEFF, log_len, one, build=_linear_build, tags={"linear"}))
        out.append(Case(f"linear-lagrange-L{log_len}", LAGRANGE, log_len, one, build=_linear_build, tags={"linear"}))
        for j in EXT_JS[log_len]:
            out.append(Case(f"linear-extended-L{log_len}-j{j}", EXTENDED, log_len, one, build=_linear_build, j=j, tags={"linear"}))
    # one element (C ABI only): halfn = 0, LINEAR is the constant itself; in the coefficient basis it sits at i = 1, which does not exist
    lin0 = [word(LINEAR, 0), word(CONST, 1), word(MULADD, 2), word(LINEAR, 3), word(ADD)]
    for basis in BASES:
        out.append(Case(f"linear-{BASIS_NAME[basis]}-L0", basis, 0, one, words=lin0, consts=[LINEAR_RANDOM, 5, Y, -1], tags={"linear"}))
    # the twiddle cache is keyed by the root: the same length under omega and under omega^3
    roots = [word(POLY, 0), 0, word(LINEAR, 0), word(MUL), word(LINEAR, 1), word(ADD)]
    for basis in (LAGRANGE, EXTENDED):
        for power in (1, 3):
            out.append(Case(f"roots-{BASIS_NAME[basis]}-L9-w{power}", basis, 9, one, words=roots, consts=[LINEAR_RANDOM, -1], omega_pow=power,
                            step=2 if basis == EXTENDED else 1, tags={"linear", "roots"}))
    return out


# ---- launch state -------------------------------------------------------------------------------------------------------------------
def _many_polys_build(leaves):
    rnd = random.Random("many")
    ast = tree = None
    for i, leaf in enumerate(leaves):
        c, rot = rnd.randrange(2, 1 << 250), i % 5 - 2
        term, tterm = Ast.of(leaf.with_rotation(rot)) * c, ("scale", ("poly", i, rot), c)
        ast, tree = (term, tterm) if ast is None else (ast + term, ("add", tree, tterm))
    return ast, tree


def _chain_program(links):
    """poly_0, then `links` times: + c_q * poly_(q mod 3) shifted by (q mod 7) - 3.  Two slots, 2 + 4 * links words."""
    rnd = random.Random("chain")
    words, consts = [word(POLY, 0), 0], []
    for q in range(links):
        consts.append(rnd.randrange(2, 1 << 250))
        words += [word(POLY, q % 3), u32(q % 7 - 3), word(SCALE, q), word(ADD)]
    return words, consts


def _launch_cases():
    words, consts = _chain_program(700)
    return [Case("polys64-lagrange-L9", LAGRANGE, 9, [("random", i) for i in range(64)], build=_many_polys_build, tags={"launch"}),
            Case("chain-lagrange-L9", LAGRANGE, 9, [("random", i) for i in range(3)], words=words, consts=consts, tags={"launch"})]


CASES = _stack_cases() + _mock_cases() + _shift_cases() + _value_cases() + _linear_cases() + _launch_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# two programs over one basis, length and polynomial count: launched back to back on one stream, then on two
BACK_TO_BACK = ("shifts-lagrange-L9", "product-lagrange-L9")


# ---- late constants -----------------------------------------------------------------------------------------------------------------
LATE_YS = (Y, LINEAR_RANDOM)


def late_build(leaves, base):
    """A quotient-like fold whose base is known only at run time; returns (Ast, tree) for a LateConstant or an integer base."""
    a, b = leaves
    terms = [(Ast.of(a) * Ast.of(b.with_rotation(1)), ("mul", ("poly", 0, 0), ("poly", 1, 1))),
             (Ast.of(a.with_rotation(-1)) + 3, ("add", ("poly", 0, -1), ("constant", 3))),
             (Ast.linear(7), ("linear", 7)), (Ast.of(b) * 11, ("scale", ("poly", 1, 0), 11))]
    return Ast.distribute_powers([t[0] for t in terms], base), ("distribute", [t[1] for t in terms], base)


def late_empty_build(leaves, base):
    """An empty expression list folds to 0 whatever the base: the compiled program never mentions the LateConstant."""
    return Ast.distribute_powers([], base) + Ast.of(leaves[0]), ("add", ("distribute", [], base), ("poly", 0, 0))


LATE_CASES = [("late-lagrange-L9", LAGRANGE, 9, 3, late_build), ("late-extended-L9", EXTENDED, 9, 5, late_build),
              ("late-empty-lagrange-L9", LAGRANGE, 9, 3, late_empty_build)]


@functools.lru_cache(maxsize=None)
def materialize_late(name, field):
    """polys, dom, and per value of y: the oracle's values of the tree with y as the base (`want`), and the model's run of the program
    compiled with a LateConstant whose slot then receives y (`values`)."""
    _, basis, log_len, j, build = next(c for c in LATE_CASES if c[0] == name)
    case = Case(name, basis, log_len, [("random", 0), ("random", 1)], build=lambda leaves: build(leaves, 0), j=j)
    m, n = fields.MODULUS[field], 1 << log_len
    dom = case.domain(field)
    out = SimpleNamespace(basis=basis, field=field, m=m, n=n, dom=dom, build=build, polys=[poly_values(r, n, m, name) for r in case.polys])
    ev = _fake_evaluator(basis, n, 2)
    leaves = [AstLeaf(ev, i) for i in range(2)]
    slot = LateConstant()
    words, consts = [], []
    ev._compile(hev._as_ast(build(leaves, slot)[0]), dom, words, consts)
    omega = dom.extended_omega if basis == EXTENDED else dom.omega
    out.slot_used, out.values, out.want = slot.index is not None, [], []
    for y in LATE_YS:
        filled = list(consts)
        if slot.index is not None:
            filled[slot.index] = y % m
        out.values.append(em.interpret(words, filled, out.polys, basis, n, m, omega)[0])
        out.want.append(oev.evaluate(build(leaves, y)[1], out.polys, basis, m, dom.k, dom.extended_k, dom.omega, dom.extended_omega, dom.g_coset))
    return out


# ---- what h2_evaluate_device refuses (C ABI) ----------------------------------------------------------------------------------------
REFUSAL_LOG_LEN = 4
# a valid call: polys[0] * polys[1](+1) + consts[0], Lagrange basis, 16 elements, two polynomials, one constant, a root of unity.
REFUSAL_BASE = dict(field=h.FP, basis=LAGRANGE, words=[word(POLY, 0), 0, word(POLY, 1), 1, word(MUL), word(CONST, 0), word(ADD)], n_words=None,
                    null_poly=None, log_len=REFUSAL_LOG_LEN, omega=True)
_LEN = 1 << REFUSAL_LOG_LEN
REFUSALS = [
    ("poly-index", dict(words=[word(POLY, 2), 0])),
    ("const-index", dict(words=[word(CONST, 1)])),
    ("linear-const-index", dict(words=[word(LINEAR, 1)])),
    ("scale-const-index", dict(words=[word(POLY, 0), 0, word(SCALE, 1)])),
    ("muladd-const-index", dict(words=[word(POLY, 0), 0, word(POLY, 1), 0, word(MULADD, 1)])),
    ("null-poly", dict(null_poly=1)),
    ("poly-last-word", dict(words=[word(POLY, 0)])),
    ("poly-last-word-after-a-node", dict(words=[word(CONST, 0), word(POLY, 0)])),
    ("underflow-add", dict(words=[word(POLY, 0), 0, word(ADD)])),
    ("underflow-mul", dict(words=[word(POLY, 0), 0, word(MUL)])),
    ("underflow-scale", dict(words=[word(SCALE, 0)])),
    ("underflow-muladd", dict(words=[word(POLY, 0), 0, word(MULADD, 0)])),
    ("two-left", dict(words=[word(POLY, 0), 0, word(POLY, 1), 0])),
    ("depth-10", dict(words=[word(CONST, 0)] * (MAX_DEPTH + 1) + [word(ADD)] * MAX_DEPTH)),
    ("coeff-shift", dict(basis=COEFF, words=[word(POLY, 0), 1])),
    ("coeff-mul", dict(basis=COEFF, words=[word(POLY, 0), 0, word(POLY, 1), 0, word(MUL)])),
    ("linear-no-omega-lagrange", dict(words=[word(LINEAR, 0)], omega=False)),
    ("linear-no-omega-extended", dict(basis=EXTENDED, words=[word(LINEAR, 0)], omega=False)),
    ("shift-len+1", dict(words=[word(POLY, 0), u32(_LEN + 1)])),
    ("shift-minus-len-1", dict(words=[word(POLY, 0), u32(-_LEN - 1)])),
    ("no-words", dict(n_words=0)),
    ("too-many-words", dict(words="2^20+1")),              # CONST 0, then 2^20 times SCALE 0: valid but for its length
    ("opcode-0", dict(words=[0])),
    ("opcode-8", dict(words=[word(POLY, 0), 0, 8])),
    ("field-2", dict(field=2)),
    ("basis-3", dict(basis=3)),
    ("basis-minus-1", dict(basis=-1)),
]
