"""The circuit front-end on the device: the reference's pinned verifying key and stored proof from nothing but running the circuit,
fresh proofs through `halo2_amd.circuit.create_proof`, and the three kernels underneath (`h2_assigned_to_field_device`,
`h2_selector_conflicts_device`, `h2_selector_combine_device`) against Python integers and numpy."""
import importlib.util
import os
import random
import re

import numpy as np
import pytest

import halo2_amd as h
from halo2_amd import dev, fields
from halo2_amd import verifier as hv
from halo2_amd.arithmetic import assigned_to_field, selector_combine, selector_conflicts
from halo2_amd.circuit import pack_selectors
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co
from oracle import pasta as o
from oracle import plonk_api as pa
from test_reference_goldens import GOLDEN, PINNED

from circuit_cases import FP, PLONK_API_A, PlonkApiCircuit, SelectorCircuit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VESTA = h.VESTA
INSTANCES = [[[2]], [[2]]]


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


@pytest.fixture(scope="module")
def params5():
    params = h.Params.new(VESTA, 5)
    yield params
    params.close()


@pytest.fixture(scope="module")
def golden_text():
    return open(os.path.join(GOLDEN, "plonk_api_pinned_vk.txt")).read()


@pytest.fixture(scope="module")
def plonk_api_pk(params5):
    return h.keygen_pk(params5, PlonkApiCircuit())


@pytest.fixture(scope="module")
def restated_params():
    g, _, w, u = pa.params_new("vesta", 5, with_lagrange=False)
    return co.points_to_mont(VESTA, g), co.points_to_mont(VESTA, [w])[0], co.points_to_mont(VESTA, [u])[0]


# ---- 7: the pinned key, from the circuit alone ------------------------------------------------------------------------------------------------
def test_pinned_key_through_keygen_vk(params5, golden_text):
    vk = h.keygen_vk(params5, PlonkApiCircuit())
    assert vk.fixed_commitments + vk.permutation_commitments == PINNED
    assert pa.compact_debug(vk.pinned()) == pa.compact_debug(golden_text)
    assert vk.vk_repr == pa.transcript_repr(golden_text)
    proof = open(os.path.join(GOLDEN, "plonk_api_proof.bin"), "rb").read()
    assert hv.verify_proof_many(params5, vk, INSTANCES, proof)
    assert not hv.verify_proof_many(params5, vk, [[[2]], [[3]]], proof)
    bad = bytearray(proof)
    bad[1000] ^= 1
    assert not hv.verify_proof_many(params5, vk, INSTANCES, bytes(bad))


# ---- 8: fresh proofs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rational", [False, True])
def test_fresh_proof_through_the_front_end(params5, plonk_api_pk, golden_text, restated_params, rational):
    from halo2_amd.plonk import ConstraintSystem
    from oracle import plonk as op
    pk = plonk_api_pk
    circuits = [PlonkApiCircuit(PLONK_API_A, rational=rational), PlonkApiCircuit(PLONK_API_A)]
    tr = Blake2bWrite(VESTA)
    h.create_proof(params5, pk, circuits, INSTANCES, _rng(4242 + rational), tr)
    proof = tr.finalize()
    assert len(proof) == os.path.getsize(os.path.join(GOLDEN, "plonk_api_proof.bin"))
    assert hv.verify_proof_many(params5, pk.vk, INSTANCES, proof)
    assert not hv.verify_proof_many(params5, pk.vk, [[[2]], [[3]]], proof)
    gm, wm, um = restated_params
    cs = pa.constraint_system(ConstraintSystem)
    ovk = {"cs": cs, "vk_repr": pa.transcript_repr(golden_text), "domain": o.EvaluationDomain(cs.degree, 5, o.P),
           "fixed_commitments": PINNED[:7], "permutation_commitments": PINNED[7:]}
    assert op.verify_proof_many(VESTA, 5, gm, wm, um, ovk, INSTANCES, proof)


# ---- 9: h2_assigned_to_field_device --------------------------------------------------------------------------------------------------------------
def _tile() -> int:
    src = open(os.path.join(ROOT, "halo2_amd", "csrc", "poly.hip")).read()
    return int(re.search(r"constexpr int kPT = (\d+);", src).group(1)) * int(re.search(r"constexpr int kPC = (\d+);", src).group(1))


TILE = _tile()


def _fractions(n_total, m, seed, pattern):
    """(numerators, denominators): three columns of unequal length one after the other, so a tile spans their boundaries."""
    rng = random.Random(seed)
    lengths = [n_total // 2 + 1, n_total // 3]
    lengths = [min(lengths[0], n_total), min(lengths[1], n_total - min(lengths[0], n_total))]
    lengths.append(n_total - sum(lengths))
    num, den = [], []
    for column, length in enumerate(lengths):
        for i in range(length):
            kind = (i + column) % 7
            num.append(0 if kind == 2 else rng.randrange(1, m))
            den.append(0 if kind == 0 else 1 if kind == 1 else rng.randrange(2, m))
    for t in range((n_total + TILE - 1) // TILE):
        lo, hi = t * TILE, min((t + 1) * TILE, n_total)
        if pattern == "empty" or (pattern == "mixed" and t == 1):              # nothing to invert in this tile
            den[lo:hi] = [rng.choice([0, 1]) for _ in range(lo, hi)]
        if pattern == "last" or (pattern == "mixed" and t == 2):               # the tile's last element is the only inversion
            den[lo:hi] = [rng.choice([0, 1]) for _ in range(lo, hi - 1)] + [rng.randrange(2, m)]
    return num, den


CASES = [(n, "mixed") for n in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)] + [(TILE, "empty"), (TILE, "last"), (TILE + 1, "last")]


@pytest.mark.parametrize("field", [h.FP, h.FQ])
@pytest.mark.parametrize("n_total,pattern", CASES)
def test_assigned_to_field_against_integers(field, n_total, pattern):
    import torch
    m = fields.MODULUS[field]
    num, den = _fractions(n_total, m, 1000 * n_total + field, pattern)
    want = [a * pow(d, -1, m) % m if d else 0 for a, d in zip(num, den)]
    dev_ = fields.current_device()
    for form, mont in ((h.FORM_MONTGOMERY, True), (h.FORM_CANONICAL, False)):
        up = lambda v: torch.from_numpy(fields.to_limbs(v, field, mont).view(np.int64)).to(dev_)
        d_num, d_den = up(num), up(den)
        out = torch.full_like(d_num, -1)
        assert assigned_to_field(d_num, d_den, field, form, out=out) is out
        assert fields.from_limbs(out.cpu().numpy().view(np.uint64), field, mont) == want
        assert torch.equal(d_num, up(num)) and torch.equal(d_den, up(den))       # inputs untouched
        aliased = assigned_to_field(d_num, d_den, field, form)                   # d_out == d_num
        assert aliased is d_num and torch.equal(aliased, out)
        # no denominators: a copy
        d_num = up(num)
        out = torch.full_like(d_num, -1)
        assigned_to_field(d_num, None, field, form, out=out)
        assert torch.equal(out, d_num) and assigned_to_field(d_num, None, field, form) is d_num and torch.equal(d_num, up(num))
    if pattern == "mixed" and n_total in (65, TILE + 1):                         # the host-pointer wrapper
        got = assigned_to_field(fields.to_limbs(num, field, True), fields.to_limbs(den, field, True), field)
        assert fields.from_limbs(got, field, True) == want
        assert fields.from_limbs(assigned_to_field(fields.to_limbs(num, field, True), None, field), field, True) == num


# ---- 10: the selector kernels ------------------------------------------------------------------------------------------------------------------
def _activations(s, n, place, seed):
    """(s, n) booleans: rows owned by at most one selector, selector 2 (when there is one) empty, a few planted pairs in the larger
    sets, and for the pair (0, s - 1) exactly one common row at `place` -- or none."""
    rng = np.random.default_rng(seed)
    owner = rng.integers(0, 3 * s, size=n)                                      # two thirds of the rows stay free
    act = np.stack([owner == i for i in range(s)])
    if s >= 3:
        act[2] = False
    if s >= 33:
        for i, j in ((5, 17), (31, 32), (s - 2, 1)):
            row = int(rng.integers(0, n))
            act[i, row] = act[j, row] = True
    if s >= 2:
        act[0] &= ~act[s - 1]
        row = {"first": 0, "last": n - 1, "middle": (n // 2) | 1 if n > 32 else 13, "none": None}[place]
        if row is not None:
            act[:, row] = False
            act[0, row] = act[s - 1, row] = True
    return act


@pytest.mark.parametrize("place", ["first", "last", "middle", "none"])
@pytest.mark.parametrize("n", [32, 160, 1 << 11, 9600, 1 << 16])
@pytest.mark.parametrize("s", [1, 2, 3, 33, 65])
def test_selector_kernels_against_numpy(s, n, place):
    import torch
    act = _activations(s, n, place, 7 * s + n)
    counts = act.astype(np.int32) @ act.astype(np.int32).T
    want = (counts > 0).astype(np.uint8)
    np.fill_diagonal(want, 0)
    if s >= 2:
        assert want[0, s - 1] == (place != "none")
    bits = torch.from_numpy(pack_selectors(act)).to(fields.current_device())
    got = selector_conflicts(bits).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(got, got.T) and not got.diagonal().any()
    # combine: greedy columns without conflicts, roots 1, 2, ... within a column
    members = []
    roots, columns = [0] * s, [0] * s
    for i in range(s):
        c = next((c for c, ms in enumerate(members) if not any(want[i, j] for j in ms)), len(members))
        if c == len(members):
            members.append([])
        members[c].append(i)
        roots[i], columns[i] = len(members[c]), c
    root_at = np.zeros((len(members), n), dtype=np.int64)
    for i in range(s):
        root_at[columns[i]][act[i]] = roots[i]
    for field in (h.FP, h.FQ):
        table = fields.to_limbs(list(range(s + 1)), field, True)
        out = selector_combine(bits, roots, columns, n, len(members), field).cpu().numpy().view(np.uint64)
        assert out.shape == (len(members), n, 4) and np.array_equal(out, table[root_at])


def test_selector_circuit_end_to_end():
    k = SelectorCircuit.K
    params = h.Params.new(VESTA, k)
    circuit = SelectorCircuit()
    pk = h.keygen_pk(params, circuit)
    assert pk.cs.num_fixed_columns == 5 and "Selector" not in pk.pinned()
    assert dev.MockProver.run_circuit(k, circuit, [], FP).verify() == []
    tr = Blake2bWrite(VESTA)
    h.create_proof(params, pk, [circuit], [[]], _rng(99), tr)
    proof = tr.finalize()
    assert hv.verify_proof(params, pk.vk, [], proof)
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 1
    assert not hv.verify_proof(params, pk.vk, [], bytes(bad))
    # one wrong witness cell: the mock prover names the gate and the row
    failures = dev.MockProver.run_circuit(k, SelectorCircuit(bad=True), [], FP).verify()
    assert [(type(f).__name__, f.gate_index, f.row) for f in failures] == [("ConstraintNotSatisfied", SelectorCircuit.MUL_GATE, SelectorCircuit.MUL_ROW)]
    assert f"Constraint {SelectorCircuit.MUL_GATE} is not satisfied on row {SelectorCircuit.MUL_ROW}" in str(failures[0])
    params.close()


# ---- 11: the example ---------------------------------------------------------------------------------------------------------------------------
def test_circuit_api_example_proves_and_verifies():
    spec = importlib.util.spec_from_file_location("circuit_api", os.path.join(ROOT, "examples", "circuit_api.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main([]) is True
