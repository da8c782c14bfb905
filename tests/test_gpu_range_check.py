"""Range checks on the device: the kernels of halo2_amd/csrc/range_check.hip against `LookupRangeCheckConfig.range_check` and
`short_range_check` run on a host synthesis (the field-arithmetic mirror of the reference), the bulk assignments against the loop of
single calls, and the eleven keys and proofs the reference stored for its circuits over the 4_5b lookup and its short range checks."""
import functools
import random

import numpy as np
import pytest

import halo2_amd as h
from halo2_amd import circuit as front
from halo2_amd import dev, ecc, fields, range_check
from halo2_amd import verifier as hv
from halo2_amd._lib import H2_ERR_ARGS, H2_OK, lib
from halo2_amd.circuit import Circuit
from halo2_amd.gadgets import sinsemilla as g
from halo2_amd.gadgets.ecc import FixedBaseTables
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co
from oracle import plonk_api

import ecc_fixed_cases as fx
import range_check_cases as rc
import sinsemilla_cases as sc
import sinsemilla_commit_cases as cc

pytestmark = pytest.mark.gpu
FP, FQ = 0, 1
VESTA = h.VESTA
P = sc.P
K = 10
COUNTS = [1, 63, 64, 65, 257]


def _ints(t, field=FP):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), field, True)


# ---- the oracle: the gadget's own big-integer arithmetic, on a host synthesis -------------------------------------------------------------------
class OracleCircuit(Circuit):
    """one witness_check (num_words) or witness_short_check (num_bits) per value through the plain config; no table is loaded, nothing
    is verified: the synthesis is run for the cells it assigns"""

    def __init__(self, values, num_words=None, num_bits=None):
        self.values, self.num_words, self.num_bits = values, num_words, num_bits

    def configure(self, meta):
        return rc.configure_lookup(meta, LookupRangeCheckConfig)

    def synthesize(self, config, layouter):
        for v in self.values:
            if self.num_words is not None:
                config.witness_check(layouter, v, self.num_words, False)
            else:
                config.witness_short_check(layouter, v, self.num_bits)


def _oracle_rows(field, values, rows, **kind):
    """[value][row] of the running_sum column as integers"""
    k = max(4, (len(values) * rows + 16).bit_length())
    _, assembly, layouter = front.synthesize(OracleCircuit(values, **kind), k, field, fixed=False, advice=True, instances=[])
    assert layouter.regions == [rows * i for i in range(len(values))]
    column = assembly.advice[0].integers(assembly.n, field)
    return [[int(v) for v in column[rows * i:rows * (i + 1)]] for i in range(len(values))]


def _decompose_values(field, num_words):
    m = fields.MODULUS[field]
    edge = 1 << (K * num_words)
    rng = random.Random(100 * field + num_words)
    special = [0, edge - 1, edge, edge + 1, m - 1, (1 << 64) - 1, 1 << 128, 1 << 192]
    return special + [rng.randrange(m) for _ in range(max(COUNTS) - len(special))]


@functools.lru_cache(maxsize=None)
def _decompose_reference(field, num_words):
    values = _decompose_values(field, num_words)
    return values, _oracle_rows(field, values, num_words + 1, num_words=num_words)


@pytest.mark.parametrize("field", [FP, FQ], ids=["fp", "fq"])
@pytest.mark.parametrize("num_words", [1, 6, 7, 13, 25])
def test_decompose_against_the_gadget(field, num_words):
    """bit-exact z_0 .. z_W; a lone lane, partial waves and more than one workgroup of rows; word 6 of 7 crosses the first limb boundary,
    25 words reach the last limb; the status is value >= 2^(10 W) for every value"""
    values, want = _decompose_reference(field, num_words)
    for count in COUNTS:
        rows, status = range_check.decompose(values[:count], num_words, field=field, with_status=True)
        assert rows.shape == (count, num_words + 1, 4) and status.shape == (count,)
        got = _ints(rows, field)
        assert [got[i * (num_words + 1):(i + 1) * (num_words + 1)] for i in range(count)] == want[:count], count
        assert [int(s) for s in status] == [int(v >= 1 << (K * num_words)) for v in values[:count]]


def test_decompose_takes_limbs_and_device_tensors():
    import torch
    values, want = _decompose_reference(FP, 13)
    limbs = fields.to_limbs(values[:65], FP, montgomery=False)
    a = range_check.decompose(limbs, 13)
    t = torch.from_numpy(limbs.view(np.int64)).to(fields.current_device())
    b = range_check.decompose(t, 13)
    assert isinstance(a, np.ndarray) and torch.is_tensor(b) and b.is_cuda
    flat = [z for zs in want[:65] for z in zs]
    assert _ints(a) == flat and _ints(b) == flat


def _call(entry, field, values, count, parameter, out, status=None):
    return entry(field, values.data_ptr() if values is not None else None, count, parameter, out.data_ptr() if out is not None else None,
                 status, None)


def test_bad_arguments():
    import torch
    device = fields.current_device()
    v = torch.zeros((1, 4), dtype=torch.int64, device=device)
    out = torch.zeros((27, 4), dtype=torch.int64, device=device)
    words, short = lib().h2_range_check_trace_device, lib().h2_short_range_check_trace_device
    assert _call(words, FP, v, 1, 0, out) == H2_ERR_ARGS and _call(words, FP, v, 1, 26, out) == H2_ERR_ARGS
    assert _call(words, FP, v, 1, 25, out) == H2_OK and _call(words, 2, v, 1, 25, out) == H2_ERR_ARGS
    assert _call(words, FP, None, 1, 5, out) == H2_ERR_ARGS and _call(words, FP, v, 1, 5, None) == H2_ERR_ARGS
    assert _call(words, FP, v, (1 << 30) + 1, 5, out) == H2_ERR_ARGS
    assert _call(words, FP, None, 0, 5, None) == H2_OK                        # nothing to do, nothing launched
    assert _call(short, FP, v, 1, 11, out) == H2_ERR_ARGS and _call(short, FP, v, 1, 10, out) == H2_OK
    assert _call(short, FP, None, 0, 4, None) == H2_OK and _call(short, FP, None, 1, 4, out) == H2_ERR_ARGS
    with pytest.raises(ValueError):
        range_check.decompose([1], 26)
    with pytest.raises(ValueError):
        range_check.decompose([1], 0)
    with pytest.raises(ValueError):
        range_check.short([1], 11)
    assert range_check.decompose([], 5).shape == (0, 6, 4) and range_check.short([], 5).shape == (0, 3, 4)
    torch.cuda.synchronize()


def _short_values(field, num_bits):
    m = fields.MODULUS[field]
    rng = random.Random(200 * field + num_bits)
    crafted = 63 * pow(1 << (K - num_bits), -1, m) % m                        # its shift is 63: only the first lookup catches it
    special = [0, (1 << num_bits) - 1, 1 << num_bits, 1023, 1024, crafted, m - 1]
    return special + [rng.randrange(m) for _ in range(65 - len(special))]


@pytest.mark.parametrize("field", [FP, FQ], ids=["fp", "fq"])
@pytest.mark.parametrize("num_bits", range(11))
def test_short_against_the_gadget(field, num_bits):
    """bit-exact value, value 2^(10 - s) in the field and 2^-s; the status is value >= 2^s"""
    values = _short_values(field, num_bits)
    want = _oracle_rows(field, values, 3, num_bits=num_bits)
    assert want[5][1] == 63                                                   # the crafted value's shift
    for count in (1, 64, 65):
        rows, status = range_check.short(values[:count], num_bits, field=field, with_status=True)
        assert rows.shape == (count, 3, 4)
        got = _ints(rows, field)
        assert [got[3 * i:3 * i + 3] for i in range(count)] == want[:count], count
        assert [int(s) for s in status] == [int(v >= 1 << num_bits) for v in values[:count]]


# ---- the bulk assignments ----------------------------------------------------------------------------------------------------------------------
K_BULK = 12                                                                   # 65 * (14 + 26 + 1 + 1 + 3) = 2925 rows


def _sides(checks, lookup="4_5b", copy=False):
    sides = []
    for many in (False, True):
        circuit = rc.BulkCircuit(checks, lookup, many=many, copy=copy)
        cs, assembly, layouter = front.synthesize(circuit, K_BULK, FP, fixed=True, advice=True, instances=[])
        selectors = assembly.selectors.copy()
        fixed = [_ints(c) for c in front.fixed_columns_of(assembly, cs)]
        advice = [_ints(c) for c in assembly.columns_to_field(assembly.advice)]
        sides.append((selectors, fixed, advice, assembly.permutation.flat().copy(), cs.pinned(), layouter))
    return sides


@pytest.mark.parametrize("lookup, copy", [("4_5b", False), ("4_5b", True), ("plain", False)], ids=["4_5b", "4_5b-copy", "plain"])
def test_bulk_equals_the_loop(lookup, copy):
    """65 values at 13 words, strict; 65 at 25 words, not strict, some wider than 250 bits; 65 short checks each at 4, 5 and 6 bits:
    every advice, fixed and selector column and the permutation mapping of the `*_many` layout are the loop's"""
    checks = rc.bulk_checks()
    assert any(v >= 1 << 250 for v in checks[1][1])
    a, b = _sides(checks, lookup, copy)
    assert np.array_equal(a[0], b[0]) and a[0].sum() >= 65 * (2 * 13 + 2 * 25 + 3)
    assert a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and a[4] == b[4]
    assert len(b[5].regions) == (65 * 5 if copy else 0) + 5


def test_the_mock_prover_accepts_both_layouts_and_names_what_breaks():
    checks = rc.bulk_checks()
    for many in (False, True):
        dev.MockProver.run_circuit(K_BULK, rc.BulkCircuit(checks, "4_5b", many=many), [], FP).assert_satisfied()
    # 2^130 among the strict checks: z_13 = 1 is tied to the constant 0
    wide = list(checks)
    wide[0] = ("words", checks[0][1][:7] + [1 << 130] + checks[0][1][8:], 13, True)
    failures = dev.MockProver.run_circuit(K_BULK, rc.BulkCircuit(wide, "4_5b", many=True), [], FP).verify()
    assert failures and {type(f).__name__ for f in failures} == {"Permutation"}
    assert (("advice", 0), 7 * 14 + 13) in {(tuple(f.column), f.row) for f in failures}
    # 16 among the 4-bit checks: (16, 4) is not a row of the table; the check is one row, 65 * (14 + 26) rows down
    four = list(checks)
    four[2] = ("bits", checks[2][1][:9] + [16] + checks[2][1][10:], 4)
    failures = dev.MockProver.run_circuit(K_BULK, rc.BulkCircuit(four, "4_5b", many=True), [], FP).verify()
    assert [(type(f).__name__, f.lookup_index, f.row) for f in failures] == [("Lookup", 0, 65 * 40 + 9)]


# ---- the reference's keys and proofs ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def params11():
    params = h.Params.new(VESTA, 11)
    yield params
    params.close()


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


@functools.lru_cache(maxsize=None)
def _ecc_tables():
    base = fields.to_limbs(list(fx.GENERATOR), FP).reshape(8)
    return FixedBaseTables.of(ecc.FixedBase(base)), FixedBaseTables.of(ecc.FixedBase(base, fx.NUM_WINDOWS_SHORT))


@functools.lru_cache(maxsize=None)
def _domain():
    from halo2_amd import sinsemilla
    return g.CommitDomains.of(sinsemilla.CommitDomain(cc.PERSONALIZATION))


@pytest.mark.parametrize("name", rc.STORED_NAMES)
def test_the_references_key_and_proof(params11, name):
    """keygen of the mirror over the DEVICE's tables reproduces the pinned key text bit for bit -- through the fixed-column commitments
    that is the tagged table, every selector and the floor plan -- and the verifier accepts the proof the reference stored"""
    make, vk_name, size = rc.stored_circuits(_ecc_tables, _domain)[name]
    text = sc.fixture_text(vk_name)
    vk = h.keygen_vk(params11, make())
    assert vk.pinned() == plonk_api.compact_debug(text)
    assert vk.vk_repr == plonk_api.transcript_repr(text)
    proof = open(sc.os.path.join(sc.GOLDEN, "proof_" + name + ".bin"), "rb").read()
    assert len(proof) == size
    assert hv.verify_proof_many(params11, vk, [[]], proof)
    bad = bytearray(proof)
    bad[size // 2] ^= 1
    assert not hv.verify_proof_many(params11, vk, [[]], bytes(bad))


# ---- fresh proofs ----------------------------------------------------------------------------------------------------------------------------------
def _prove(params, circuit, seed):
    pk = h.keygen_pk(params, circuit)
    tr = Blake2bWrite(VESTA)
    h.create_proof(params, pk, [circuit], [[]], _rng(seed), tr)
    return pk, tr.finalize()


def test_a_fresh_merkle_proof_over_the_4_5b_lookup(params11):
    rng = random.Random(45)
    leaf, pos, path = rng.randrange(P), rng.getrandbits(32), [rng.randrange(P) for _ in range(sc.MERKLE_DEPTH)]
    circuit = rc.MerkleCircuit45(leaf, pos, path)
    dev.MockProver.run_circuit(11, circuit, [], FP).assert_satisfied()
    assert circuit.root.value().inner.evaluate(P) == sc.merkle_path_root(sc.q_of(sc.TEST_DOMAIN), leaf, pos, path)
    pk, proof = _prove(params11, circuit, 45)
    assert pk.vk_repr == plonk_api.transcript_repr(sc.fixture_text("vk_merkle_with_private_init_chip_4_5b.rdata.gz"))
    assert len(proof) == 4160 and hv.verify_proof(params11, pk.vk, [], proof)


def test_a_fresh_sinsemilla_proof_over_the_4_5b_lookup(params11):
    circuit = rc.SinsemillaCircuit45(_domain(), seed=9)
    dev.MockProver.run_circuit(11, circuit, [], FP).assert_satisfied()
    pk, proof = _prove(params11, circuit, 46)
    assert len(proof) == 4672 and hv.verify_proof(params11, pk.vk, [], proof)


def test_the_example_runs(capsys):
    """examples/range_check.py end to end at 256 values: bulk-assigned, mock-proved, proved and verified; one row a short check"""
    mod = sc._example("range_check")
    assert mod.main(["--count", "256"])
    out = capsys.readouterr().out
    assert "took 512 rows (1 each)" in out and "they take 1536 (3 each)" in out
    wide, four, five = mod.witness(16, 3)
    sides = []
    for bulk in (True, False):
        _, assembly, _ = front.synthesize(mod.RangeCheckCircuit(wide, four, five, bulk=bulk), 11, FP, fixed=True, advice=True, instances=[])
        sides.append(([_ints(c) for c in assembly.columns_to_field(assembly.advice)], assembly.selectors.copy()))
    assert sides[0][0] == sides[1][0] and np.array_equal(sides[0][1], sides[1][1])
