"""Shared by test_h2c_edge_cases.py and test_gpu_h2c_edges.py: inputs that reach the branches of fe_sqrt (csrc/field_sqrt.cuh), of the
simplified SWU map, the affine sum and the isogeny (csrc/h2c_map.cuh) and of the point decoder (csrc/points.hip) which hashed or random
inputs reach with probability 2^-32 or less, and what `oracle.pasta` / `oracle.hash_to_curve` compute from them.  Deterministic, built
for both fields; everything is a canonical integer."""
import functools
import random

from oracle import hash_to_curve as oh
from oracle import pasta as o

FIELDS = ("pallas", "vesta")                 # the curve whose BASE field is meant: Fp for Pallas, Fq for Vesta
S = o.S                                      # 32: p - 1 = 2^32 T in both fields
ORDERS = range(S + 1)                        # j: a^T has order exactly 2^j; j = 32 are the non-residues
PER_ORDER = 4
N_RANDOM_SQRT = 256
N_SWU_EACH = 16                              # u with g(x1) a square / not a square
N_RANDOM_SWU = 128
N_SAME_X = 8                                 # pairs with equal mapped points / with opposite mapped points
N_RANDOM_PAIRS = 128
N_ISO_POINTS = 32


def modulus(cid):
    return oh.BASE[cid]


def t_of(m):
    return (m - 1) >> S


def two_adic_order(a, m):
    """j with a^T of order exactly 2^j (a != 0)"""
    b, j = pow(a, t_of(m), m), 0
    while b != 1:
        b, j = b * b % m, j + 1
    return j


def order_element(j, rng, m):
    """g^(2^(32-j) odd) r^(2^32) with g = 5^T: the first factor has order exactly 2^j, the second has odd order"""
    g = pow(o.GENERATOR, t_of(m), m)
    r = rng.randrange(1, m)
    odd = rng.randrange(1 << 40) | 1
    head = pow(g, (1 << (S - j)) * odd, m) if j else 1
    return head * pow(r, 1 << S, m) % m


def fixed_sqrt_values(m):
    return [0, 1, 4, m - 1, m - 4, 5, (1 << 256) % m]


@functools.lru_cache(maxsize=None)
def sqrt_classes(cid):
    """{"orders": {j: [a] * 4}, "fixed": [...], "random": [a] * 256}"""
    m, rng = modulus(cid), random.Random("h2c-edges sqrt " + cid)
    orders = {j: [order_element(j, rng, m) for _ in range(PER_ORDER)] for j in ORDERS}
    return {"orders": orders, "fixed": fixed_sqrt_values(m), "random": [rng.randrange(m) for _ in range(N_RANDOM_SQRT)]}


@functools.lru_cache(maxsize=None)
def sqrt_runs(cid):
    """The driver runs of mode `sqrt`: name -> inputs.  interleaved: consecutive lanes cycle through the 33 orders (every wave
    diverges), then the fixed values and the random ones; grouped: each of the 132 order elements 64 times, so whole waves share an
    order; single: one lane, p - 1."""
    c, m = sqrt_classes(cid), modulus(cid)
    interleaved = [c["orders"][j][k] for k in range(PER_ORDER) for j in ORDERS] + c["fixed"] + c["random"]
    grouped = [a for j in ORDERS for a in c["orders"][j] for _ in range(64)]
    return {"interleaved": interleaved, "grouped": grouped, "single": [m - 1]}


def sqrt_expected(a, m):
    """(flag, root) as fe_sqrt leaves them; the root of a non-residue is not specified (None)"""
    r = o.sqrt_mod(a, m)
    return (0, None) if r is None else (1, r)


# ---- simplified SWU -------------------------------------------------------------------------------------------------------------
def swu(u, cid):
    return oh.map_to_curve_simple_swu(u, oh.ISO_A[cid], oh.ISO_B, modulus(cid))


def swu_tv(u, m):
    z = oh.SWU_Z % m
    return (z * z * pow(u, 4, m) + z * u * u) % m


def iso_rhs(x, cid):
    m = modulus(cid)
    return (pow(x, 3, m) + oh.ISO_A[cid] * x + oh.ISO_B) % m


def gx1_is_square(u, cid):
    m = modulus(cid)
    tv = swu_tv(u, m)
    assert tv
    x1 = (-oh.ISO_B) * pow(oh.ISO_A[cid], -1, m) % m * (1 + pow(tv, -1, m)) % m
    return o.sqrt_mod(iso_rhs(x1, cid), m) is not None


@functools.lru_cache(maxsize=None)
def swu_classes(cid):
    m, rng = modulus(cid), random.Random("h2c-edges swu " + cid)
    sq, nsq = [], []
    while len(sq) < N_SWU_EACH or len(nsq) < N_SWU_EACH:
        u = rng.randrange(1, m)
        dst = sq if gx1_is_square(u, cid) else nsq
        if len(dst) < N_SWU_EACH:
            dst.append(u)
    return {"fixed": [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2], "square": sq, "nonsquare": nsq,
            "negated": [m - u for u in sq + nsq], "random": [rng.randrange(m) for _ in range(N_RANDOM_SWU)]}


def swu_inputs(cid):
    c = swu_classes(cid)
    return c["fixed"] + c["square"] + c["nonsquare"] + c["negated"] + c["random"]


# ---- pairs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def isogeny(cid):
    return oh.derive_isogeny(cid)


def pair_expected(u0, u1, cid):
    """iso_map(swu(u0) + swu(u1)); the identity as (0, 0)"""
    m = modulus(cid)
    r = oh.iso_map(oh._add_general(swu(u0, cid), swu(u1, cid), oh.ISO_A[cid], m), isogeny(cid), m)
    return (0, 0) if r is None else r


def same_x_pairs(cid, rng, want_equal_y, count):
    """(u0, u1) with u1^2 = (-1 - Z u0^2) / Z.  With w = Z u^2 the map's tv is w (w + 1), and w0 + w1 = -1 gives tv0 = tv1, so both
    u share the first candidate x1; when g(x1) is a square both maps return it (otherwise they return w0 x1 != w1 x1 and the pair is
    dropped).  |u0| != |u1|, and y is +-sqrt(g(x1)) with the sign of sgn0(u): negating u1 turns equal y into opposite y."""
    m = modulus(cid)
    z = oh.SWU_Z % m
    zi = pow(z, -1, m)
    out = []
    while len(out) < count:
        u0 = rng.randrange(1, m)
        u1 = o.sqrt_mod((-1 - z * u0 * u0) * zi % m, m)
        if u1 is None or u1 in (0, u0, m - u0):
            continue
        q0, q1 = swu(u0, cid), swu(u1, cid)
        if q0[0] != q1[0]:
            continue                                  # g(x1) is not a square: the maps return Z u^2 x1, which differ
        if (q0[1] == q1[1]) != want_equal_y:
            u1 = m - u1
            q1 = swu(u1, cid)
        assert q0[0] == q1[0] and (q0[1] == q1[1]) == want_equal_y and q0[1] != 0
        out.append((u0, u1))
    return out


@functools.lru_cache(maxsize=None)
def pair_classes(cid):
    m, rng = modulus(cid), random.Random("h2c-edges pair " + cid)
    us = [rng.randrange(1, m) for _ in range(8)]
    return {"tangent": [(u, u) for u in us], "opposite": [(u, m - u) for u in us],
            "zero": [(0, 0)] + [(0, u) for u in us[:4]] + [(u, 0) for u in us[:4]],
            "same_x_equal_y": same_x_pairs(cid, rng, True, N_SAME_X), "same_x_opposite_y": same_x_pairs(cid, rng, False, N_SAME_X),
            "random": [(rng.randrange(m), rng.randrange(m)) for _ in range(N_RANDOM_PAIRS)]}


IDENTITY_PAIR_CLASSES = ("opposite", "same_x_opposite_y")


@functools.lru_cache(maxsize=None)
def pair_runs(cid):
    """name -> [(class, (u0, u1))]: one lane, a partial wave (63 lanes: every crafted pair, then random ones) and more than one block
    of 128 lanes (every pair, then the crafted ones with u0 and u1 swapped)."""
    c = pair_classes(cid)
    crafted = [(k, p) for k in ("tangent", "opposite", "zero", "same_x_equal_y", "same_x_opposite_y") for p in c[k]]
    rand = [("random", p) for p in c["random"]]
    return {"single": [("same_x_opposite_y", c["same_x_opposite_y"][0])], "wave63": (crafted + rand)[:63],
            "all": crafted + rand + [(k, (b, a)) for k, (a, b) in crafted]}


# ---- add / iso: polynomial code, inputs need not lie on the curve --------------------------------------------------------------
def add_expected(x0, y0, x1, y1, cid):
    """(x3, y3, identity flag) of the affine sum as h2c_iso_add computes it; (0, 0, 1) for the identity.  Differs from _add_general
    in one documented place: a point with y = 0 added to itself is the identity (2-torsion), where _add_general would divide by 0."""
    m = modulus(cid)
    if x0 == x1 and ((y0 + y1) % m == 0):
        return (0, 0, 1)
    r = oh._add_general((x0, y0), (x1, y1), oh.ISO_A[cid], m)
    return (r[0], r[1], 0)


@functools.lru_cache(maxsize=None)
def add_classes(cid):
    m, rng = modulus(cid), random.Random("h2c-edges add " + cid)
    f = lambda: rng.randrange(1, m)
    pts = [swu(f(), cid) for _ in range(8)]
    distinct = [(f(), f(), f(), f()) for _ in range(16)] + [(*pts[i], *pts[i + 1]) for i in range(7)]
    return {"self_y0": [(x, 0, x, 0) for x in (0, 1, f(), f())],
            "opposite": [(x, y, x, m - y) for x, y in [(f(), f()) for _ in range(4)] + pts[:4]],
            "double": [(x, y, x, y) for x, y in [(f(), f()) for _ in range(4)] + pts[:4]],
            "distinct": distinct}


def add_inputs(cid):
    c = add_classes(cid)
    return c["self_y0"] + c["opposite"] + c["double"] + c["distinct"]


def iso_expected(x, y, cid):
    r = oh.iso_map((x, y), isogeny(cid), modulus(cid))
    return (0, 0) if r is None else r


@functools.lru_cache(maxsize=None)
def iso_classes(cid):
    m, rng = modulus(cid), random.Random("h2c-edges iso " + cid)
    x0 = isogeny(cid)[0]
    ys = [rng.randrange(1, m) for _ in range(2)]
    return {"kernel": [(x0, ys[0]), (x0, ys[1]), (x0, 0)], "next_to_kernel": [((x0 + 1) % m, ys[0]), ((x0 - 1) % m, ys[1])],
            "on_curve": [swu(rng.randrange(m), cid) for _ in range(N_ISO_POINTS)]}


def iso_inputs(cid):
    c = iso_classes(cid)
    return c["kernel"] + c["next_to_kernel"] + c["on_curve"]


# ---- decoder: x with x^3 + 5 of a prescribed 2-adic order -----------------------------------------------------------------------
def cube_root(c, m):
    """A cube root of c in F_m, or None.  3^v || m - 1; c^(3^-1 mod (m-1)/3^v) is a cube root up to a 3^v-th root of unity."""
    v, rest = 0, m - 1
    while rest % 3 == 0:
        rest, v = rest // 3, v + 1
    base = pow(c, pow(3, -1, rest), m)
    w = pow(o.GENERATOR, rest, m)                    # generates the 3^v-th roots of unity
    for i in range(3 ** v):
        x = base * pow(w, i, m) % m
        if pow(x, 3, m) == c % m:
            return x
    return None


@functools.lru_cache(maxsize=None)
def decoder_xs(cid):
    """{j: x} with x^3 + 5 of 2-adic order 2^j, j = 0 .. 32 (j = 32: not a point)"""
    m, rng = modulus(cid), random.Random("h2c-edges decoder " + cid)
    out = {}
    for j in ORDERS:
        while j not in out:
            a = order_element(j, rng, m)
            x = cube_root((a - o.CURVE_B) % m, m)
            if x is not None and x != 0:
                out[j] = x
    return out


def encode_x(x, sign):
    b = bytearray(int(x).to_bytes(32, "little"))
    b[31] |= sign << 7
    return bytes(b)


# ---- BLAKE2b block boundaries -----------------------------------------------------------------------------------------------
def dst_len(cid, prefix_len):
    """len(DST'): prefix || "-" || curve || "_XMD:BLAKE2b_SSWU_RO_" || one length byte"""
    return prefix_len + 1 + len(cid) + len("_XMD:BLAKE2b_SSWU_RO_") + 1


def positional(n, salt):
    """n printable bytes that differ by position (a misplaced byte changes the digest); no NUL, the prefix is a C string"""
    return bytes(33 + (salt + 7 * i) % 90 for i in range(n))


@functools.lru_cache(maxsize=None)
def blake_cases(cid):
    """[(prefix, message)]: the prefix sweep 0 .. 64 at message lengths 0 and 64, and for b0 inputs of 255, 256, 257 bytes
    (msg_len + dl in {124, 125, 126}) six splits between prefix and message each, msg_len = 64 and the shortest message among them."""
    cases = [(positional(lp, 3).decode(), positional(ml, 11 + lp)) for lp in range(65) for ml in (0, 64)]
    dl0 = dst_len(cid, 0)
    splits = {}
    for total in (124, 125, 126):
        shortest = max(0, total - dl0 - 64)                       # the prefix holds at most 64 bytes
        lens = sorted({shortest, shortest + 1, shortest + 7, 48, 63, 64})
        assert len(lens) == 6 and all(0 <= total - dl0 - ml <= 64 for ml in lens)
        splits[total] = [(positional(total - dl0 - ml, 5).decode(), positional(ml, total)) for ml in lens]
        cases += splits[total]
    return cases, splits


def b0_len(cid, prefix, msg):
    return 131 + len(msg) + dst_len(cid, len(prefix))


def b1_len(cid, prefix):
    return 65 + dst_len(cid, len(prefix))
