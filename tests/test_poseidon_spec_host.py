"""Poseidon for any Spec, without a GPU: the model of tests/poseidon_model.py against the reference's vectors at (3, 2, 8, 56), the
constants of halo2_amd.poseidon_spec.Spec against the model, the argument checks of the three h2_poseidon_spec_*_device entry points,
what the header and the source promise about streams and device memory, and the generalised Pow5 chip evaluated with Python
integers at a small width.

Ground truth.  tests/poseidon_model.py restates halo2_poseidon/src/{lib,grain,mds}.rs in Python integers, independently of
halo2_amd/poseidon_spec.py.  Reference VALUES exist only for width 3 (tests/golden/poseidon_kat.json, poseidon_hash_kat.json): the
reference is Rust, nothing here can build it, and oracle/ is closed.  Every other width therefore rests on the model and on the pins
of this file -- the model reproduces the reference's vectors at width 3, two independent restatements agree on the constants at every
width tested, and the drawn MDS matrix times its drawn inverse is the identity."""
import ast
import ctypes as C
import os
import re

import pytest

import poseidon_cases as pc
import poseidon_model as pm
import poseidon_spec_cases as psc
from halo2_amd import _lib, poseidon_spec
from halo2_amd import circuit as front
from halo2_amd.poseidon_spec import Spec
from poseidon_cases import FP, FQ, HASH_KAT, KAT, NAME

GPU_TEST_FILE = os.path.join(psc.ROOT, "tests", "test_gpu_poseidon_spec.py")
CONSTANT_KEYS = [(2, 1, 8, 56, 0), (3, 2, 8, 56, 0), (9, 8, 8, 56, 0), (12, 11, 8, 56, 0), (4, 2, 8, 56, 0), (3, 2, 8, 56, 1)]


# ---- the model is the reference at width 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FP, FQ])
def test_the_model_is_the_reference_at_p128pow5t3(field):
    model = pm.model(field, 3, 2, 8, 56)
    rcs, mds = pc.kat_constants(field)
    assert model.round_constants == rcs and model.mds == mds
    for v in KAT[NAME[field]]["permute"]:
        assert model.permute([int(x, 16) for x in v["initial_state"]]) == [int(x, 16) for x in v["final_state"]]
    for v in HASH_KAT[NAME[field]]["hash"]:
        assert model.hash([int(x, 16) for x in v["input"]]) == int(v["output"], 16)
    # the restatements the suite already has agree with it beyond the vectors: other lengths, the trace
    for length in (1, 3, 4, 5):
        message = pm.random_states(1, length, field, 90 + length)[0]
        assert model.hash(message) == pc.hash_ints(message, field)
    state = pm.random_states(1, 3, field, 3)[0]
    assert model.trace(state) == pc.trace_ints(state, field)


# ---- Spec against the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FP, FQ])
@pytest.mark.parametrize("key", CONSTANT_KEYS, ids=str)
def test_spec_constants_are_the_models(field, key):
    width, rate, full, partial, secure = key
    spec, model = Spec(field, width, rate, full, partial, secure), pm.model(field, width, rate, full, partial, secure)
    assert (spec.round_constants, spec.mds, spec.mds_inv) == (model.round_constants, model.mds, model.mds_inv)
    assert len(spec.round_constants) == full + partial and all(len(row) == width for row in spec.round_constants)
    m = pm.MOD[field]
    product = [[sum(spec.mds[i][k] * spec.mds_inv[k][j] for k in range(width)) % m for j in range(width)] for i in range(width)]
    assert product == [[int(i == j) for j in range(width)] for i in range(width)]
    state = pm.random_states(1, width, field, 11)[0]
    assert spec.permute_ints(state) == poseidon_spec.permute_spec(state, spec) == model.permute(state)
    for length in (1, rate, rate + 1):
        message = pm.random_states(1, length, field, 12 + length)[0]
        assert spec.hash_ints(message) == model.hash(message)


def test_secure_mds_passes_over_matrices_and_the_rate_does_not_matter():
    first, second = Spec(FP, 3, 2, 8, 56, 0), Spec(FP, 3, 2, 8, 56, 1)
    assert first.round_constants == second.round_constants and first.mds != second.mds
    assert Spec(FP, 4, 2).mds == Spec(FP, 4, 3).mds                            # the Grain seed has no rate in it


@pytest.mark.parametrize("field", [FP, FQ])
def test_the_default_instance(field):
    spec = Spec.p128pow5t3(field)
    assert (spec.round_constants, spec.mds, spec.mds_inv) == poseidon_spec.constants(field)
    assert (spec.width, spec.rate, spec.full_rounds, spec.partial_rounds, spec.rows) == (poseidon_spec.WIDTH, poseidon_spec.RATE, 8, 56, poseidon_spec.ROWS)
    assert spec is Spec(field, 3, 2) is Spec(field, 3, 2, 8, 56, 0)           # cached per parameter tuple
    state = [0, 1, 2]
    assert spec.permute_ints(state) == poseidon_spec.permute(state, field)


@pytest.mark.parametrize("args", [(2, 3, 2), (FP, 1, 1), (FP, 13, 12), (FP, 3, 0), (FP, 3, 3), (FP, 3, 2, 7, 56), (FP, 3, 2, 0, 56), (FP, 3, 2, 8, 1017)], ids=str)
def test_spec_refuses_what_the_library_refuses(args):
    with pytest.raises(ValueError):
        Spec(*args)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_the_descriptor_is_the_headers_struct():
    header = re.sub(r"/\*.*?\*/", "", open(psc.HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct h2_poseidon_spec \{(.*?)\} h2_poseidon_spec_t;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [name for name, _ in _lib.PoseidonSpec._fields_]
    assert C.sizeof(_lib.PoseidonSpec) == 40 and _lib.PoseidonSpec.d_constants.offset == 24 and _lib.PoseidonSpec.stream.offset == 32
    assert "#define H2_POSEIDON_MAX_WIDTH 12" in header and _lib.POSEIDON_MAX_WIDTH == poseidon_spec.MAX_WIDTH == 12
    for name in psc.STREAM_ENTRIES:
        assert name in _lib.SIGNATURES


def test_argument_validation_without_gpu():
    lib = _lib.lib()
    rows = psc.refusals()
    assert len(rows) == 3 * 15 + 4
    for row in rows:
        assert psc.refuse(lib, row) == _lib.H2_ERR_ARGS, row[:2]


def test_the_stream_travels_in_the_descriptor_and_every_entry_point_has_a_stream_case():
    import stream_cases as sc
    protos = psc.spec_prototypes()
    assert set(protos) == set(psc.STREAM_ENTRIES) and len(protos) == 3
    # no `void *stream` parameter (the table of tests/stream_cases.py is closed); each takes the descriptor, which carries the stream
    assert not set(protos) & sc.prototypes_with_stream()
    assert all(re.match(r"\s*const\s+h2_poseidon_spec_t\s*\*\s*spec\b", params) for params in protos.values())
    cases = psc.stream_cases()
    assert set(cases) == set(protos) and all(case.entry == name for name, case in cases.items())
    for case in cases.values():                                               # what test_stream_case_coverage.py asks of a case
        real, decoy = case.inputs(sc.REAL), case.inputs(sc.DECOY)
        assert list(real) == list(decoy) and real
        for key in real:
            assert real[key].shape == decoy[key].shape and real[key].tobytes() != decoy[key].tobytes()
            case.valid({key: sc.mixture(real[key], decoy[key])})
        want = case.expected(sc.REAL)
        assert len(want) == sum(size for _, size in case.output_bytes()) and want != case.expected(sc.DECOY)
    # the GPU file runs every case through the ordered modes
    tree = ast.parse(open(GPU_TEST_FILE).read())
    marks = [node for node in tree.body if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "pytestmark" for t in node.targets)]
    assert len(marks) == 1 and ast.unparse(marks[0].value) == "pytest.mark.gpu"
    funcs = {node.name: ast.unparse(node) for node in tree.body if isinstance(node, ast.FunctionDef)}
    for name in ("test_stream_mode_a_late_producer_early_overwrite", "test_stream_mode_b_a_misplaced_stream_is_seen",
                 "test_stream_producer_on_another_stream_with_an_event_wait"):
        assert name in funcs and "psc.STREAM_ENTRIES" in funcs[name], name


def test_the_unit_keeps_no_device_memory():
    text = open(psc.SOURCE).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert not re.search(r"\bDevBuf\b", code) and not re.search(r"\bStreamContexts\b", code) and not re.search(r"\w+_release_workspaces", code)
    assert not re.search(r"\bhipMalloc|\bhipStreamCreate|\bhipEventCreate|__constant__", code)
    import test_call_sequence_coverage as cov
    assert "poseidon_spec.hip" not in cov.owning_units()
    # every launch names the descriptor's stream
    launches = re.findall(r"hipLaunchKernelGGL\(([^;]*)\);", code)
    assert len(launches) == 6 and all(re.search(r"lds_bytes\(a\), st,", launch) for launch in launches)
    assert code.count("hipStream_t st = (hipStream_t)spec->stream;") == 3
    makefile = open(os.path.join(psc.ROOT, "halo2_amd", "csrc", "Makefile")).read()
    assert "poseidon_spec.hip" in makefile.split("SRCS :=")[1].split("\n")[0]


# ---- the chip, on the host ---------------------------------------------------------------------------------------------------------------------
SMALL = (4, 3, 2, 2)                                                          # four rows a permutation


def _columns(meta, width):
    return ([meta.advice_column() for _ in range(width)], meta.advice_column(), [meta.fixed_column() for _ in range(width)],
            [meta.fixed_column() for _ in range(width)])


def test_configure_refuses_what_pow5_rs_asserts():
    from halo2_amd.gadgets.poseidon import Pow5Chip
    configure = lambda width, spec: Pow5Chip.configure(meta := front.ConstraintSystem(pm.P), *_columns(meta, width), spec=spec)
    configure(4, Spec(FP, *SMALL))
    for width, spec in ((3, Spec(FP, *SMALL)), (4, Spec(FP, 4, 2, 2, 2)), (5, Spec(FP, 5, 4, 8, 57)), (4, Spec(FQ, *SMALL)), (4, None)):
        with pytest.raises(ValueError):
            configure(width, spec)


def test_spec_none_is_the_t3_chip_unchanged():
    from halo2_amd.gadgets.poseidon import Pow5Chip
    pinned = []
    for spec in (None, Spec.p128pow5t3(FP)):
        meta = front.ConstraintSystem(pm.P)
        config = Pow5Chip.configure(meta, *_columns(meta, 3), spec=spec)
        assert (config.width, config.rate, config.rows, config.full_offsets, config.partial_offsets) == (3, 2, 37, pc_full_rows(), list(range(4, 32)))
        pinned.append(meta.pinned())
    assert pinned[0] == pinned[1]


def pc_full_rows():
    return list(range(4)) + list(range(32, 36))


@pytest.mark.parametrize("length", [3, 4, 7])
def test_small_wide_hash_circuit_on_the_host(length):
    model = pm.model(FP, *SMALL)
    message = pm.random_states(1, length, FP, 500 + length)[0]
    digest = model.hash(message)
    circuit = psc.WideHashCircuit(SMALL, length, message)
    assert pc.host_failures(circuit, 6, FP, [[digest]]) == []
    failures = pc.host_failures(circuit, 6, FP, [[(digest + 1) % pm.P]])
    assert failures and {f[0] for f in failures} == {"copy"}
    # a wrong word of the message breaks nothing but the copy of the digest either: the hash of another message is another digest
    other = psc.WideHashCircuit(SMALL, length, [(message[0] + 1) % pm.P] + message[1:])
    assert {f[0] for f in pc.host_failures(other, 6, FP, [[digest]])} == {"copy"}
