"""The field layer (csrc/field.cuh, field9.cuh, field_inv.cuh) on the device, on the crafted operands of tests/field_edge_cases.py: a zero running
low word at every reduction step, sums and differences on and next to p and 2p, carries and borrows through every limb, the lazy
representatives, the 29 / 32-bit seams of the repacking, k p in five limb layouts, the operands the CPU interpreter of the generated multipliers
is trusted on, and the whole inversion list.  build/field_edge_driver (tests/native/field_edge_driver.hip) applies one device function per
lane; every comparison here is equality or congruence of Python integers (field_edge_cases.judge), on every lane, in two lane orders."""
import glob
import os
import subprocess

import pytest

import field_edge_cases as ec
import test_field_inv_host as host_inv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver():
    """build/field_edge_driver, built here when it is missing or older than its sources (build() makes it).  No compiler and no binary
    is a failure, not a skip."""
    exe = os.path.join(ROOT, "build", "field_edge_driver")
    csrc = os.path.join(ROOT, "halo2_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "field_edge_driver.hip")] + glob.glob(os.path.join(csrc, "*.cuh")) + glob.glob(os.path.join(csrc, "*.inc"))
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", srcs[0], "-o", exe])
    return exe


def run_driver(exe, tmp_path, mode, field, cases, tag=""):
    """one driver process: cases -> one result per lane (an integer, or nine signed limbs)"""
    src, dst = tmp_path / f"{mode}_{field}{tag}.in", tmp_path / f"{mode}_{field}{tag}.out"
    src.write_bytes(ec.encode(mode, cases))
    done = subprocess.run([exe, mode, ec.FIELD_ARG[field], str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (mode, field, done.returncode, done.stdout, done.stderr)
    return ec.decode(mode, dst.read_bytes(), len(cases))


def check_mode(exe, tmp_path, mode, field):
    """Both lane orders of a mode, every lane judged; the same operands give the same result in both.  {case: result}"""
    seen = {}
    for order in ("interleaved", "grouped"):
        cases = ec.runs(mode, field)[order]
        got = run_driver(exe, tmp_path, mode, field, cases, "_" + order)
        for lane, (case, out) in enumerate(zip(cases, got)):
            verdict = ec.judge(mode, field, case, out)
            assert verdict is None, (mode, field, order, lane, case, out, verdict)
            key = ec._key(case)
            first = seen.setdefault(key, out)
            assert first == out, (mode, field, order, lane, case, first, out)
    return seen


def test_the_driver_holds_the_shipped_implementations(driver):
    """fe_mulx is the scheduled asm multiplier, fe9_mul the generated statement, fe_inv the divstep inversion; no experiment switch"""
    done = subprocess.run([driver, "config"], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0
    assert done.stdout.split() == ["H2_MUL_IMPL", "4", "H2_FE9_IMPL", "1", "H2_FE_INV_FERMAT", "0"], done.stdout


@pytest.mark.parametrize("field", ec.FIELDS)
def test_montgomery_products(driver, tmp_path, field):
    """fe_mulx, fe_mul_c, fe_sqr, fe_to_mont == a b R^-1 mod p on the cross product of the pair palette (about 18 000 lanes), the crafted
    pairs (a zero running low word at every row of fe_mul_c, products on both sides of p before the subtraction) and the operands of
    test_field_mul_asm_model.py; fe_mul_c and fe_mulx give identical words on every pair."""
    mul, mul_c = check_mode(driver, tmp_path, "mul", field), check_mode(driver, tmp_path, "mul_c", field)
    assert mul == mul_c and len(mul) > 14000
    check_mode(driver, tmp_path, "sqr", field)
    check_mode(driver, tmp_path, "to_mont", field)


@pytest.mark.parametrize("field", ec.FIELDS)
def test_redc_and_from_mont(driver, tmp_path, field):
    """fe_redc(a) == fe_from_mont(a) == a R^-1 mod p, canonical, for any 256-bit word: the running low word zero at step s and at no
    earlier step for s = 0 .. 7, all zero, low word 1, p, 2p, 3p, the word that reduces to p - 1, words up to 2^256 - 1."""
    redc, from_mont = check_mode(driver, tmp_path, "redc", field), check_mode(driver, tmp_path, "from_mont", field)
    assert redc == from_mont and all(v < ec.P[field] for v in redc.values())


@pytest.mark.parametrize("field", ec.FIELDS)
def test_add_sub_neg_dbl_and_reduce_once(driver, tmp_path, field):
    """fe_add / fe_sub on the cross product and on a + b in {p - 1, p, p + 1, 2p - 2}, a - b in {0, +-1}, carries and borrows through one
    and through all eight limbs; fe_neg, fe_dbl on the unary palette; fe_reduce_once at 0, p - 1, p, p + 1, 2p - 1."""
    for mode in ("add", "sub", "neg", "dbl", "reduce_once"):
        got = check_mode(driver, tmp_path, mode, field)
        assert all(v < ec.P[field] for v in got.values()), mode


@pytest.mark.parametrize("field", ec.FIELDS)
def test_lazy_operations(driver, tmp_path, field):
    """fe_mul_lazy (congruent, below 2p + 2^130), fe_add_lazy (sums 2p - 1, 2p, past 2^256), fe_sub_lazy (subtrahends with bit 255 set:
    its loop, wave-uniform in the grouped order and divergent in the interleaved one), fe_reduce_lazy, fe_is_zero_lazy at 0, p, 2p
    against +-1 of each -- on the representatives a, a + p and, for a < 2^128, a + 2p."""
    for mode in ("mul_lazy", "add_lazy", "sub_lazy", "reduce_lazy", "is_zero_lazy"):
        check_mode(driver, tmp_path, mode, field)


@pytest.mark.parametrize("field", ec.FIELDS)
def test_inversion(driver, tmp_path, field):
    """fe_inv (Montgomery in and out, 0 for 0; output times input == R^2 mod p, the Montgomery one) and modinv30 as hipcc compiles it, on
    2^k, 2^k +- 1, p - 2^k for every k in 0 .. 254, p - 1, p - 2, (p +- 1) / 2, single limbs: every inverse == pow(x, -1, p), and the
    device's modinv30 gives the same words as the host program tests/native/modinv_edge_check.cpp (built plain here; test_field_inv_host.py
    runs it under the sanitizers on the same inputs and holds both builds to the same words)."""
    p = ec.P[field]
    inv = check_mode(driver, tmp_path, "inv", field)
    for (a,), out in inv.items():
        assert out < p and (out * a % p == ec.R * ec.R % p if a else out == 0), hex(a)
    dev = check_mode(driver, tmp_path, "modinv30", field)
    values = ec.inversion_values(field)
    host = host_inv.run_host(host_inv.host_program(sanitized=False), tmp_path, field, values)
    assert [dev[(x,)] for x in values] == [h[0] for h in host]


@pytest.mark.parametrize("field", ec.FIELDS)
def test_repacking_and_form_conversion(driver, tmp_path, field):
    """fe9_unpack / fe9_pack at 2^(29 i) +- 1, 2^(32 w) +- 1, all ones, single fields of ones; pack(unpack(x)) == x for x < 2^256 with the
    device's own limbs in between; fe9_from_r256 (a product: congruent to 32 x, limbs and value in range), fe9_to_r256 (exact), and
    to_r256(from_r256(x)) == x for x < p."""
    p = ec.P[field]
    unpacked = check_mode(driver, tmp_path, "unpack9", field)
    check_mode(driver, tmp_path, "pack9", field)
    xs = [c[0] for c in ec.runs("unpack9", field)["interleaved"]]
    assert run_driver(driver, tmp_path, "pack9", field, [(unpacked[(x,)],) for x in xs], "_roundtrip") == xs
    m9 = check_mode(driver, tmp_path, "from_r256", field)
    check_mode(driver, tmp_path, "to_r256", field)
    below_p = [x for x in xs if x < p]
    assert len(below_p) > 40
    assert run_driver(driver, tmp_path, "to_r256", field, [(m9[(x,)],) for x in below_p], "_roundtrip") == below_p


@pytest.mark.parametrize("field", ec.FIELDS)
def test_carry_free_products(driver, tmp_path, field):
    """fe9_mul, fe9_mul_c, fe9_sqr, fe9_dot2, fe9_sqr_minus on exactly the operands the CPU interpreter runs (test_field9_asm_model.py: signed,
    un-normalised, at the bounds of curve9.cuh, limb 0 equal to 2^29, the NTT's raw limbs by a twiddle): value congruent, limbs 1 .. 7
    in [0, 2^29), limb 0 in [1, 2^29] for the generated statements, the value inside the bound the header gives."""
    for mode in ("mul9", "mul9_c", "sqr9", "dot2", "sqr_minus"):
        check_mode(driver, tmp_path, mode, field)


@pytest.mark.parametrize("field", ec.FIELDS)
def test_carry_passes_and_canonical_forms(driver, tmp_path, field):
    """fe9_norm and fe9_quadruple_norm at the ends of their limb ranges and with a carry through all limbs (value unchanged resp. times 4,
    limbs 0 .. 7 in [0, 2^29)); fe9_canonical at k p + d, |k| <= 15, d in {0, +-1}, five limb layouts (each of its five subtractions
    taken and not taken, wave-uniform and divergent); fe9_canonical_small at -p + 1, -1, 0, 1, p - 1, p, p + 1, 2p - 1; the zero filter
    and the full zero test on k p and its near misses."""
    for mode in ("norm9", "quadruple_norm9", "canonical9", "canonical_small9", "maybe_zero9", "is_zero9"):
        check_mode(driver, tmp_path, mode, field)
