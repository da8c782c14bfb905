"""Variable-base multiplication on the device: the kernels of halo2_amd/csrc/ecc.hip against `oracle.pasta.ec_mul` and the restated
witness of tests/ecc_cases.py.  Every comparison is bit for bit."""
import functools

import numpy as np
import pytest

from halo2_amd import ecc, fields
from halo2_amd._lib import lib

import ecc_cases as ec
from ecc_cases import ORDER, P, ROWS

pytestmark = pytest.mark.gpu
FP = 0
OK, ERR_ARGS = 0, 1


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(fields.current_device())


def _ints(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), FP, True)


def _points(t):
    v = _ints(t)
    return [(v[i], v[i + 1]) for i in range(0, len(v), 2)]


def _base_limbs(bases):
    return fields.to_limbs([c for pt in bases for c in pt], FP).reshape(-1, 8)


# ---- mul ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mul_pool():
    """257 (base, scalar) pairs and their products: the edge scalars, q, q +- 1, 2^255 - 1, then random 255-bit values; lane 5 (an
    interior lane of every size but 1) multiplies the identity"""
    scalars = ec.EDGE_SCALARS + [ORDER, ORDER - 1, ORDER + 1, (1 << 255) - 1]
    scalars = scalars + ec.random_scalars(257 - len(scalars))
    bases = list(ec.random_bases(257))
    bases[5] = (0, 0)
    return bases, scalars, [ec.ec_mul(k, b) for k, b in zip(scalars, bases)]


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_mul_against_ec_mul(n):
    """a partial wave, more than one wave, more than one workgroup; n = 1 takes a random 255-bit scalar"""
    bases, scalars, want = mul_pool()
    first = 256 if n == 1 else 0
    b = _base_limbs(bases[first:first + n])
    k = fields.to_limbs(scalars[first:first + n], FP, montgomery=False)
    pts, status = ecc.mul(_up(b), _up(k), with_status=True)
    assert pts.shape == (n, 8) and not status.any()
    assert _points(pts) == want[first:first + n]
    if n > 5:
        assert want[5] == (0, 0) and (0, 0) in want[:4]                        # the identity base, and k = 0
    if n == 65:                                                               # numpy in, numpy out
        host = ecc.mul(b, k)
        assert isinstance(host, np.ndarray) and (host.view(np.int64) == pts.cpu().numpy()).all()


def test_mul_flags_a_base_off_the_curve():
    bases = list(ec.random_bases(3))
    bases[1] = (bases[1][0], (bases[1][1] + 1) % P)
    k = fields.to_limbs([3, 3, 3], FP, montgomery=False)
    _, status = ecc.mul(_base_limbs(bases), k, with_status=True)
    assert status.tolist() == [0, 1, 0]
    with pytest.raises(ecc.OffCurve):
        ecc.mul(_base_limbs(bases), k)


# ---- mul_trace ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trace_pool():
    """65 (base, alpha) pairs and their restated witnesses: alpha = 0 on lane 0, p - 1 on lane 37, 2^254 - t_q on lane 64, the other
    fifteen edge scalars on lanes 1 .. 15, random elements of Fp elsewhere"""
    edge = list(ec.EDGE_SCALARS)
    alphas = [a % P for a in ec.random_scalars(65, bits=254, seed=13)]
    for lane, a in ((0, 0), (37, P - 1), (64, (1 << 254) - ec.T_Q)):
        alphas[lane] = a
        edge.remove(a)
    alphas[1:16] = edge
    bases = ec.random_bases(65, seed=14)
    return bases, alphas, [ec.mul_trace(b, a) for b, a in zip(bases, alphas)]


@pytest.mark.parametrize("count", [1, 65])
def test_trace_against_the_restated_witness(count):
    """all ten columns at every row, all 16 aux entries, a status of zeros; the last row is `mul`'s product.  count = 1 is alpha = 0,
    the one scalar below p that reaches the exceptional branches of complete addition"""
    bases, alphas, want = trace_pool()
    b, a = _up(_base_limbs(bases[:count])), _up(fields.to_limbs(alphas[:count], FP))
    cols, aux, status = ecc.mul_trace(b, a, with_status=True)
    assert cols.shape == (10, ROWS * count, 4) and aux.shape == (count, 16, 4) and status.shape == (count,) and not status.any()
    got, got_aux = [_ints(cols[c]) for c in range(10)], _ints(aux)
    for i in range(count):
        w_cols, w_aux, result = want[i]
        for c in range(10):
            assert got[c][i * ROWS:(i + 1) * ROWS] == w_cols[c], (i, c)
        assert got_aux[16 * i:16 * (i + 1)] == w_aux, i
        assert (w_cols[2][ROWS - 1], w_cols[3][ROWS - 1]) == result == ec.ec_mul(alphas[i], bases[i])
    assert want[0][2] == (0, 0)
    products = ecc.mul(b, _up(fields.to_limbs(alphas[:count], FP, montgomery=False)))
    last = [(got[2][i * ROWS + ROWS - 1], got[3][i * ROWS + ROWS - 1]) for i in range(count)]
    assert _points(products) == last
    if count == 65:                                                           # numpy in, numpy out
        h_cols, h_aux = ecc.mul_trace(_base_limbs(bases), fields.to_limbs(alphas, FP))
        assert isinstance(h_cols, np.ndarray) and (h_cols.view(np.int64) == cols.cpu().numpy()).all()
        assert (h_aux.view(np.int64) == aux.cpu().numpy()).all()


def test_trace_reports_an_identity_base():
    bases = [ec.random_bases(2)[0], (0, 0), ec.random_bases(2)[1]]
    alphas = fields.to_limbs([5, 5, 5], FP)
    _, _, status = ecc.mul_trace(_base_limbs(bases), alphas, with_status=True)
    assert status.tolist() == [0, 1, 0]
    with pytest.raises(ecc.Vanishing):
        ecc.mul_trace(_base_limbs(bases), alphas)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """a null pointer with n > 0 is H2_ERR_ARGS and nothing is written; n = 0 is H2_OK whatever the pointers"""
    import torch
    dev = fields.current_device()
    b, k = _up(_base_limbs(ec.random_bases(2))), _up(fields.to_limbs([1, 2], FP))
    out = torch.full((2, 8), 7, dtype=torch.int64, device=dev)
    cols = torch.full((10, 2 * ROWS, 4), 7, dtype=torch.int64, device=dev)
    aux = torch.full((2, 16, 4), 7, dtype=torch.int64, device=dev)
    status = torch.full((2,), 7, dtype=torch.uint8, device=dev)
    mul_args = [b.data_ptr(), k.data_ptr(), 2, out.data_ptr(), status.data_ptr(), None]
    for null in (0, 1, 3, 4):
        args = list(mul_args)
        args[null] = None
        assert lib().h2_ecc_mul_device(*args) == ERR_ARGS
    trace_args = [b.data_ptr(), k.data_ptr(), 2, cols.data_ptr(), aux.data_ptr(), status.data_ptr(), None]
    for null in (0, 1, 3, 4, 5):
        args = list(trace_args)
        args[null] = None
        assert lib().h2_ecc_mul_trace_device(*args) == ERR_ARGS
    torch.cuda.synchronize()
    assert (out == 7).all() and (cols == 7).all() and (aux == 7).all() and (status == 7).all()
    assert lib().h2_ecc_mul_device(None, None, 0, None, None, None) == OK
    assert lib().h2_ecc_mul_trace_device(None, None, 0, None, None, None, None) == OK
    pts = ecc.mul(np.zeros((0, 8), np.uint64), np.zeros((0, 4), np.uint64))
    assert pts.shape == (0, 8)


# ---- the gadget: the bulk path against the mirror, the MockProver, a proof ------------------------------------------------------------------
import halo2_amd as h                                                         # noqa: E402
from halo2_amd import circuit as front                                        # noqa: E402
from halo2_amd import dev                                                     # noqa: E402
from halo2_amd import verifier as hv                                          # noqa: E402
from halo2_amd.transcript import Blake2bWrite                                 # noqa: E402
from oracle import c_oracle as co                                             # noqa: E402

VESTA = h.VESTA                                                               # its scalar field is Fp, the field of the circuits


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


def _pairs(count):
    bases, alphas, _ = trace_pool()
    return list(zip(bases[:count], alphas[:count]))


def _names(circuit, k):
    cs, _, _ = front.synthesize(circuit.without_witnesses(), k, FP, fixed=True, advice=False)
    return [(g.name, n) for g in cs.gates for n in g.constraint_names]


def test_mul_many_lays_the_rows_of_mul():
    """count = 2 (alpha = 0 and an edge scalar): the ten advice columns of the bulk region are the two regions of the host `mul`
    one after the other, row for row; the overflow checks hold the same s, running sums and eta"""
    pairs = _pairs(2)
    sides = []
    for cls in (ec.MulCircuit, ec.MulManyCircuit):
        circuit = cls(pairs)
        _, assembly, layouter = front.synthesize(circuit, 11, FP, fixed=True, advice=True, instances=[])
        sides.append((circuit, [_ints(c) for c in assembly.columns_to_field(assembly.advice)], layouter))
    (one, a, la), (many, b, lb) = sides
    start = lb.regions[many.many.region_index]
    per_call = [la.regions[p.inner().x().cell().region_index] for p in one.products]
    for c in range(10):
        assert b[c][start:start + 2 * ROWS] == a[c][per_call[0]:per_call[0] + ROWS] + a[c][per_call[1]:per_call[1] + ROWS], c
    s_at, sums_at, gate_at = (lb.regions[many.many.region_index + j] for j in (1, 2, 3))
    for i, p in enumerate(one.products):
        r = p.inner().x().cell().region_index
        s1, sums1, gate1 = (la.regions[r + j] for j in (1, 2, 3))
        assert b[6][s_at + i] == a[6][s1] and b[9][sums_at + 14 * i:sums_at + 14 * i + 14] == a[9][sums1:sums1 + 14]
        assert [b[c][gate_at + 3 * i:gate_at + 3 * i + 3] for c in (6, 7, 8)] == [a[c][gate1:gate1 + 3] for c in (6, 7, 8)]
    assert _points(many.many.outputs) == [ec.ec_mul(alpha, base) for base, alpha in pairs]


def test_mock_prover_accepts_both_paths():
    """the bulk path at k = 14 with 65 multiplications, alpha = 0 on lane 0; the per-call path at k = 11"""
    dev.MockProver.run_circuit(14, ec.MulManyCircuit(_pairs(65)), [], FP).assert_satisfied()
    dev.MockProver.run_circuit(11, ec.MulCircuit(_pairs(3)), [], FP).assert_satisfied()


@pytest.mark.parametrize("what, gate, constraint", [("z_hi", "q_mul_2 == 1 checks", "bool_check"), ("lambda", "complete addition", "1"),
                                                    ("eta", "overflow checks", "canonicity")])
def test_mock_prover_names_a_mutated_cell(what, gate, constraint):
    """in the second of two bulk multiplications; alpha = 2^200 + 12345 constrains eta (k_254 = 0, z_130 and s >> 130 not zero)"""
    pairs = [_pairs(1)[0], (ec.random_bases(1)[0], (1 << 200) + 12345)]
    circuit = ec.MulManyCircuit(pairs, mutate=(1, what))
    failures = dev.MockProver.run_circuit(11, circuit, [], FP).verify()
    names = _names(circuit, 11)
    row = circuit.mutated_row - (1 if what == "eta" else 0)
    assert failures and all(type(f).__name__ == "ConstraintNotSatisfied" for f in failures), failures[:3]
    named = [names[f.gate_index] + (f.row,) for f in failures]
    assert (gate, constraint, row) in named and all(n[0] == gate and abs(n[2] - row) <= 1 for n in named), named


def test_a_proof_of_65_multiplications():
    """keygen, create_proof and verify_proof at k = 14 with the products as public inputs; one changed input is rejected; keygen
    without a witness and with one give the same key"""
    pairs = _pairs(65)
    want = [c for base, alpha in pairs for c in ec.ec_mul(alpha, base)]
    circuit = ec.MulManyCircuit(pairs, expose=True)
    params = h.Params.new(VESTA, 14)
    try:
        pk = h.keygen_pk(params, circuit)
        assert h.keygen_vk(params, circuit.without_witnesses()).vk_repr == pk.vk_repr == h.keygen_vk(params, circuit).vk_repr
        tr = Blake2bWrite(VESTA)
        h.create_proof(params, pk, [circuit], [[want]], _rng(14), tr)
        proof = tr.finalize()
        assert hv.verify_proof(params, pk.vk, [want], proof)
        wrong = list(want)
        wrong[7] = (wrong[7] + 1) % P
        assert not hv.verify_proof(params, pk.vk, [wrong], proof)
    finally:
        params.close()


def test_the_example_proves_eight_multiplications():
    """examples/ecc_mul.py end to end (8 of its 64 multiplications): mock-proved, proved, verified, and rejected with a changed input"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "ecc_mul.py")
    spec = importlib.util.spec_from_file_location("ecc_mul", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main(["--count", "8"]) is True


def test_trace_across_a_chunk_of_scratch():
    """the trace goes through its scratch in chunks of 2^23 / 253 = 33 156 multiplications: 70 more than one chunk, the 65 pairs of
    the pool over and over, so the rows on both sides of the boundary must be the rows of the same pairs in a call of their own"""
    import torch
    bases, alphas, _ = trace_pool()
    per_chunk = (1 << 23) // 253
    count = per_chunk + 70
    b65, a65 = _up(_base_limbs(bases)), _up(fields.to_limbs(alphas, FP))
    reps = (count + 64) // 65
    cols, aux, status = ecc.mul_trace(b65.repeat(reps, 1)[:count].contiguous(), a65.repeat(reps, 1)[:count].contiguous(), with_status=True)
    want_cols, want_aux = ecc.mul_trace(b65, a65)
    assert not status.any()
    for i in (0, per_chunk - 1, per_chunk, per_chunk + 1, count - 1):
        j = i % 65
        assert torch.equal(cols[:, ROWS * i:ROWS * (i + 1)], want_cols[:, ROWS * j:ROWS * (j + 1)]), i
        assert torch.equal(aux[i], want_aux[j]), i
    # and every multiplication's product, against the 65 of the pool
    last = ROWS * torch.arange(count, device=cols.device) + ROWS - 1
    pool_last = ROWS * torch.arange(65, device=cols.device) + ROWS - 1
    assert torch.equal(cols[2:4][:, last], want_cols[2:4][:, pool_last].repeat(1, reps, 1)[:, :count])
