"""Scalars that stress the endomorphism split of the generic multiexp (k = k1 + lambda k2, csrc/glv.cuh) and the top window of its digit
rows.  Shared by tests/test_gpu_parity.py (the default forms) and tests/test_gpu_generic_paths.py (the same scalars under profiling, which
routes a large call through the two-pass sort's own split)."""
from oracle import pasta as o

# the endomorphism's eigenvalue on each curve's scalar field: lambda^2 + lambda + 1 = 0 (mod q)
LAMBDA = {0: 0x6819a58283e528e511db4d81cf70f5a0fed467d47c033af2aa9d2e050aa0e4f,
          1: 0x2d33357cb532458ed3552a23a8554e5005270d29d19fc7d27b7fd22f0201b547}


def endomorphism_edge_values(curve):
    """0, +-1, lambda and its neighbours (k2 = +-1, k1 = 0), powers of two around the 128-bit half length, the largest scalars, and every
    digit position set to +-2^(c-1) for c = 16, 13, 10 (the extreme signed digits); reduced mod q."""
    sm = o.CURVES[curve][1]
    lam = LAMBDA[curve]
    assert (lam * lam + lam + 1) % sm == 0
    vals = [0, 1, 2, sm - 1, sm - 2, lam, lam + 1, lam - 1, sm - lam, (sm - lam) - 1, lam * lam % sm, 1 << 127, 1 << 128,
            (1 << 128) - 1, (1 << 128) + 1, 1 << 129, 1 << 254, (sm - 1) // 2, (sm + 1) // 2, 0x8000, 0x8001, 0x7FFF,
            sum(0x8000 << (16 * i) for i in range(15)), sum(0x8000 << (13 * i) for i in range(19)) % sm,
            sum(0x200 << (10 * i) for i in range(25)) % sm, (lam << 1) % sm, (lam * 0x8000) % sm]
    return [v % sm for v in vals]


def top_window_boundary_values(curve, rng):
    """Scalars k = +-k1 +- lambda k2 whose 128-bit halves carry every boundary value of the top 16-bit window -- 0, 1, 2^15 - 1, 2^15,
    2^15 + 1 (the first digit that recodes negative and carries), 2^16 - 2, 2^16 - 1 -- over every boundary value of the window below
    (with and without a carry into the top); random low bits from `rng` (a random.Random), which the caller goes on using."""
    sm = o.CURVES[curve][1]
    lam = LAMBDA[curve]
    tops = [0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFE, 0xFFFF]
    below = [0, 0x7FFF, 0x8000, 0x8001, 0xFFFF]
    halves = [(t << 112) | (b << 96) | rng.getrandbits(96) for t in tops for b in below] + [(1 << 128) - 1, 1 << 127, (1 << 127) - 1]
    crafted = []
    for k1 in halves:
        for k2 in (0, halves[rng.randrange(len(halves))]):
            for s1, s2 in ((1, 1), (-1, 1), (1, -1)):
                crafted.append((s1 * k1 + s2 * k2 * lam) % sm)
    return crafted
