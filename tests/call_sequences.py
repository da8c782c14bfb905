"""What the call-sequence tests drive (a helper: nothing here is collected).

The library keeps device memory between calls: a grow-only workspace per unit and (device, stream), handed back by h2_trim through the
`*_release_workspaces` functions of csrc/api.hip.  PROBES has, for every unit that owns such memory, a *probe*: one call of the unit at
a size class ("small" or "large") on a given stream, returned as bytes, and the bytes the oracle (oracle.c_oracle, oracle.ipa,
oracle.lookup) or the unit's case module expects.  The two size classes ask the unit for workspaces of different sizes and are the
smallest shapes that do; a probe with `single_size` has one shape for both.  (Asking is not always growing: DevBuf::reserve allocates an
eighth and 256 bytes more than it is asked for, which covers the three scan tiles of the large poly shapes, and the generator collapse
keeps one fixed-size digit table -- so the GPU test asserts what never may happen, a reallocation behind a larger call, not that the
large call reallocates.)  Expected bytes are computed once per process.

tests/test_gpu_call_sequences.py runs every probe through small / large / small on two streams around an h2_trim;
tests/test_call_sequence_coverage.py proves on the CPU that no unit with cached device memory is without a probe."""
import ctypes as C
import functools
import random

import numpy as np

import halo2_amd as h
from halo2_amd import _lib, ecc, fields, sinsemilla
from halo2_amd.arithmetic import _p, ipa_round_scalars, permute_expression_pair, sort_field
from oracle import c_oracle as co
from oracle import ipa as oipa
from oracle import lookup as olk
from oracle import pasta as o

SMALL, LARGE = "small", "large"
SIZES = (SMALL, LARGE)
FP = h.FP

# h2_debug_counters_t, in the header's order (tests/test_call_sequence_coverage.py holds the header and halo2_amd/_lib.py to this list)
COUNTER_FIELDS = ("devbuf_epoch", "host_msm_plain", "host_msm_captured", "host_msm_replayed", "host_msm_graphs_dropped",
                  "ipa_table_registered", "ipa_table_refilled", "ipa_table_freed", "twiddle_built", "twiddle_hits")


def counters() -> dict:
    """h2_debug_counters as a dict (host bookkeeping: no device work)."""
    c = _lib.DebugCounters()
    rc = h.lib().h2_debug_counters(C.byref(c))
    assert rc == _lib.H2_OK, rc
    return c.as_dict()


def delta(before: dict, after: dict) -> dict:
    """The counters that moved between two readings (they only rise)."""
    assert all(after[k] >= before[k] for k in before), (before, after)
    return {k: after[k] - before[k] for k in before if after[k] != before[k]}


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _up(a, dtype=np.int64):
    """A host array on the current device, copied on torch's current stream."""
    return _torch().from_numpy(np.ascontiguousarray(a).view(dtype)).to(fields.current_device())


def _down(*tensors) -> bytes:
    """The bytes of device tensors (the copy back waits for the current stream)."""
    return b"".join(t.contiguous().cpu().numpy().tobytes() for t in tensors)


def _limbs(ints, field=FP) -> bytes:
    return fields.to_limbs(ints, field, True).tobytes()


def _mont(field, v):
    return fields.scalar_limbs(v, field, True)


def _affine_limbs(curve, point) -> bytes:
    """A point of the oracle (Jacobian or affine Montgomery limbs) as the 8 affine Montgomery limbs H2_OUT_AFFINE writes."""
    point = np.ascontiguousarray(point, dtype=np.uint64)
    xy = co.jac_to_affine_ints(curve, point) if point.shape[0] == 12 else co.affine_to_ints(curve, point)
    assert xy is not None
    return _limbs(list(xy), co.field_of_curve(curve, "base"))


class Probe:
    """name; files: the csrc translation units whose cached device memory the call goes through; releases: the `*_release_workspaces`
    functions of h2_trim that hand that memory back; shapes: {size class: what sizes the call}; run(shape, stream) -> bytes with torch's
    current stream set to `stream`; expected(shape) -> bytes."""

    def __init__(self, name, files, releases, shapes, run, expected, single_size=False):
        self.name, self.files, self.releases, self.single_size = name, tuple(files), tuple(releases), single_size
        self.shapes = {SMALL: shapes, LARGE: shapes} if single_size else dict(zip(SIZES, shapes))
        self._run, self._expected = run, functools.lru_cache(maxsize=None)(expected)

    def run(self, size, stream) -> bytes:
        with _torch().cuda.stream(stream):
            return self._run(self.shapes[size], stream)

    def expected(self, size) -> bytes:
        return self._expected(self.shapes[size])

    def __repr__(self):
        return self.name


# ---- multiexps ------------------------------------------------------------------------------------------------------------------------
MSM_CURVE = h.PALLAS
MSM_PATHS = {300: 1, 70000: 2}                                    # H2_MSM_PATH_ONE_PASS, H2_MSM_PATH_TWO_PASS


@functools.lru_cache(maxsize=None)
def _msm_inputs(n):
    sf = co.field_of_curve(MSM_CURVE, "scalar")
    return co.random_field(sf, 7100 + n % 97, n), co.generate_bases(MSM_CURVE, 7200 + n % 97, n)


def _run_generic_msm(n, stream):
    scal, bases = _msm_inputs(n)
    out = h.best_multiexp(_up(scal), _up(bases), MSM_CURVE, affine=True)
    path = C.c_int(0)
    assert h.lib().h2_msm_last_path(C.c_void_p(stream.cuda_stream), C.byref(path), None, None, None) == _lib.H2_OK
    assert path.value == MSM_PATHS[n], (n, path.value)           # the two sizes are the two sorts, each with its own scratch
    return _down(out)


def _want_generic_msm(n):
    scal, bases = _msm_inputs(n)
    return _affine_limbs(MSM_CURVE, co.best_multiexp(MSM_CURVE, scal, bases))


COMMIT_CURVE = h.VESTA
COMMIT_SHAPES = ((1 << 10, False), ((1 << 16) + 5, True))         # (points of the registered table, with a blind)
_commit_tables = {}


@functools.lru_cache(maxsize=None)
def _commit_inputs(n):
    sf = co.field_of_curve(COMMIT_CURVE, "scalar")
    g, col = co.generate_bases(COMMIT_CURVE, 7300 + n % 97, n), co.random_field(sf, 7400 + n % 97, n)
    return g, col, co.generate_bases(COMMIT_CURVE, 7500, 1)[0], co.random_field(sf, 7501, 1)[0]


def commit_table(n) -> C.c_uint64:
    """The handle of the registered table of n points with the blind base installed: registered once, it outlives every h2_trim."""
    if n not in _commit_tables:
        g, _, w, _ = _commit_inputs(n)
        hd = C.c_uint64(0)
        assert h.lib().h2_bases_register(COMMIT_CURVE, _p(g), n, h.FORM_MONTGOMERY, C.byref(hd)) == _lib.H2_OK
        assert h.lib().h2_bases_set_blind_base(hd, _p(w), h.FORM_MONTGOMERY) == _lib.H2_OK
        _commit_tables[n] = hd
    return _commit_tables[n]


def commit_table_state(n):
    """(h2_bases_info, h2_bases_blind_base_set) of the table: what must not change across an h2_trim."""
    size, bits, curve = C.c_size_t(0), C.c_int(0), C.c_int(-1)
    rc = h.lib().h2_bases_info(commit_table(n), C.byref(size), C.byref(bits), C.byref(curve))
    return rc, size.value, bits.value, curve.value, h.lib().h2_bases_blind_base_set(commit_table(n))


def _run_commit_device(shape, stream):
    n, blinded = shape
    _, col, _, blind = _commit_inputs(n)
    torch = _torch()
    d_col, d_blind = _up(col), _up(blind)
    out = torch.empty(8, dtype=torch.int64, device=d_col.device)
    rc = h.lib().h2_commit_device(commit_table(n), d_col.data_ptr(), n, None, d_blind.data_ptr() if blinded else None, h.FORM_MONTGOMERY,
                                  _lib.OUT_AFFINE, out.data_ptr(), C.c_void_p(stream.cuda_stream))
    assert rc == _lib.H2_OK, h.lib().h2_last_error()
    return _down(out)


def _run_commit_host(shape, stream):
    n, blinded = shape
    _, col, _, blind = _commit_inputs(n)
    out = np.zeros(8, dtype=np.uint64)
    rc = h.lib().h2_commit(commit_table(n), _p(col), n, None, _p(blind) if blinded else None, h.FORM_MONTGOMERY, _lib.OUT_AFFINE, _p(out))
    assert rc == _lib.H2_OK, h.lib().h2_last_error()
    return out.tobytes()


def _want_commit(shape):
    n, blinded = shape
    g, col, w, blind = _commit_inputs(n)
    return _affine_limbs(COMMIT_CURVE, co.commit(COMMIT_CURVE, g, w, col, blind) if blinded else co.best_multiexp(COMMIT_CURVE, col, g))


# ---- transforms -----------------------------------------------------------------------------------------------------------------------
NTT_FIELD = h.FP
NTT_LOGS = (5, 13)                                                # one pass; two passes through the per-stream scratch vector


@functools.lru_cache(maxsize=None)
def _ntt_input(log_n):
    return co.random_field(NTT_FIELD, 7600 + log_n, 1 << log_n)


@functools.lru_cache(maxsize=None)
def _domains(k):
    return h.EvaluationDomain(3, k, NTT_FIELD), o.EvaluationDomain(3, k, fields.MODULUS[NTT_FIELD])


def _omega(log_n):
    return _mont(NTT_FIELD, o.omega_for(fields.MODULUS[NTT_FIELD], log_n))


def _run_ntt(log_n, stream):
    return _down(h.best_fft(_up(_ntt_input(log_n)), _omega(log_n), log_n, NTT_FIELD))


def _want_ntt(log_n):
    return co.best_fft(NTT_FIELD, _ntt_input(log_n), _omega(log_n), log_n).tobytes()


def _run_ifft(k, stream):
    return _down(_domains(k)[0].lagrange_to_coeff(_up(_ntt_input(k))))


def _want_ifft(k):
    ref = _domains(k)[1]
    return co.ifft(NTT_FIELD, _ntt_input(k), _mont(NTT_FIELD, ref.omega_inv), k, _mont(NTT_FIELD, ref.ifft_divisor)).tobytes()


def _run_coeff_to_extended(k, stream):
    """From host memory: the transform's device form is out of place and needs no scratch; this one goes through the staging vectors."""
    return np.ascontiguousarray(_domains(k)[0].coeff_to_extended(_ntt_input(k).copy())).tobytes()


def _want_coeff_to_extended(k):
    ref, f = _domains(k)[1], NTT_FIELD
    return co.coeff_to_extended(f, _ntt_input(k), k, ref.extended_k, _mont(f, ref.g_coset), _mont(f, ref.g_coset_inv),
                                _mont(f, ref.extended_omega)).tobytes()


# ---- polynomial helpers: the scans work in tiles of 2048 elements, two tiles and one element need the carry level ------------------------
POLY_FIELD = h.FQ
POLY_SIZES = (9, 2 * 2048 + 1)


@functools.lru_cache(maxsize=None)
def _poly_inputs(n):
    return co.random_field(POLY_FIELD, 7700, n), co.random_field(POLY_FIELD, 7701, n), co.random_field(POLY_FIELD, 7702, 1)[0]


def _poly_probe(name, device, oracle):
    def run(n, stream):
        a, b, x = _poly_inputs(n)
        return _down(device(_up(a), _up(b), x, n))

    def want(n):
        a, b, x = _poly_inputs(n)
        return np.ascontiguousarray(oracle(a, b, x, n)).tobytes()
    return Probe(name, ["poly.hip"], ["poly_release_workspaces"], POLY_SIZES, run, want)


# ---- the opening argument's pieces ----------------------------------------------------------------------------------------------------------
IPA_CURVE = h.VESTA
IPA_KS = (4, 11)


@functools.lru_cache(maxsize=None)
def _ipa_generators(k):
    return co.generate_bases(IPA_CURVE, 7800 + k, 1 << k)


def _ipa_challenge():
    return co.random_field(co.field_of_curve(IPA_CURVE, "scalar"), 7801, 1)[0]


def _run_generator_collapse(k, stream):
    return _down(h.parallel_generator_collapse(_up(_ipa_generators(k)), _ipa_challenge(), IPA_CURVE))


def _want_generator_collapse(k):
    return np.ascontiguousarray(co.generator_collapse(IPA_CURVE, _ipa_generators(k), _ipa_challenge())).tobytes()


ROUND_SCALARS = ((4, 1), (11, 3))                                 # (k, j): round j of a 2^k argument


@functools.lru_cache(maxsize=None)
def _round_inputs(k, j):
    field = co.field_of_curve(IPA_CURVE, "scalar")
    return field, co.random_field(field, 7900 + k, 1 << (k - j)), co.random_field(field, 7901 + k, j)


def _run_round_scalars(shape, stream):
    k, j = shape
    field, p, u = _round_inputs(k, j)
    torch = _torch()
    d_l, d_r = (torch.full(((1 << k) + 1, 4), -1, dtype=torch.int64, device=fields.current_device()) for _ in range(2))
    ipa_round_scalars(_up(p), k, j, [u[r] for r in range(j)], field, d_l, d_r)
    return _down(d_l[:1 << k], d_r[:1 << k])


def _want_round_scalars(shape):
    """The definition: p'[i ^ half] times the challenges picked by the bits of the block number, placed by the half i falls in."""
    k, j = shape
    field, p, u = _round_inputs(k, j)
    m = fields.MODULUS[field]
    p_i, u_i = fields.from_limbs(p, field, True), fields.from_limbs(u, field, True)
    blk = k - j
    half = 1 << (blk - 1)
    left, right = [], []
    for row in range(1 << k):
        block, i = row >> blk, row & ((1 << blk) - 1)
        s = 1
        for r in range(j):
            if (block >> (j - 1 - r)) & 1:
                s = s * u_i[r] % m
        v = p_i[i ^ half] * s % m
        left.append(v if i < half else 0)
        right.append(0 if i < half else v)
    return _limbs(left, field) + _limbs(right, field)


def seeded_rng(field, seed, device_first=False):
    """rng(count) of the opening argument: the oracle's seeded field elements, another seed per draw.  device_first: the first draw
    (the n coefficients of s_poly) is handed over as a CUDA tensor, which takes create_proof through h2_open_device."""
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        vals = co.random_field(field, ctr[0], count)
        return _up(vals) if device_first and ctr[0] == seed + 1 else vals
    return rng


_params = {}
# Generators that are the identity, by seed: every g_i with i = column mod 2^14.  The collapsed generator of such a column is the
# identity whatever the challenges are, and an identity's rows of a registered table are the zeros a (re)fill starts from: a refill
# that left the column's earlier rows behind would commit over another argument's points.
IDENTITY_COLUMNS = {0x2700: (0, 5, (1 << 14) - 1)}


def opening_params(curve, k, seed):
    """Params over seeded generators (g_lagrange plays no part in the opening argument): built once, closed by nobody."""
    key = (curve, k, seed)
    if key not in _params:
        g = co.generate_bases(curve, seed, 1 << k)
        for column in IDENTITY_COLUMNS.get(seed, ()):
            g[column::1 << 14] = 0
        w, u = co.generate_bases(curve, 60, 1)[0], co.generate_bases(curve, 61, 1)[0]
        _params[key] = (h.Params(curve, k, g, g, w, u), g, w, u)
    return _params[key]


@functools.lru_cache(maxsize=None)
def _opening_inputs(curve, k, seed):
    sf = co.field_of_curve(curve, "scalar")
    return co.random_field(sf, seed + 1, 1 << k), h.Blind(co.random_field(sf, seed + 2, 1)[0]), co.random_field(sf, seed + 3, 1)[0]


def opening_proof(curve, k, seed, p_poly=None, device_first=False) -> bytes:
    """opening.create_proof with the default schedule into a fresh transcript: the proof's bytes."""
    from halo2_amd.opening import create_proof
    from halo2_amd.transcript import Blake2bWrite
    params = opening_params(curve, k, seed)[0]
    px, blind, x = _opening_inputs(curve, k, seed)
    tr = Blake2bWrite(curve)
    create_proof(params, seeded_rng(co.field_of_curve(curve, "scalar"), seed + 10, device_first), tr, px if p_poly is None else p_poly, blind, x)
    return tr.finalize()


@functools.lru_cache(maxsize=None)
def opening_proof_wanted(curve, k, seed) -> bytes:
    """The same from the sequential restatement of commitment::create_proof over the C oracle (oracle/ipa.py)."""
    _, g, w, u = opening_params(curve, k, seed)
    px, blind, x = _opening_inputs(curve, k, seed)
    ot = oipa.Transcript(curve)
    oipa.create_proof(curve, k, g, w, u, seeded_rng(co.field_of_curve(curve, "scalar"), seed + 10), ot, px, blind.value, x)
    return bytes(ot.out)


def _run_open_device(k, stream):
    px = _opening_inputs(IPA_CURVE, k, 8000 + k)[0]
    return opening_proof(IPA_CURVE, k, 8000 + k, p_poly=_up(px), device_first=True)


def _want_open_device(k):
    return opening_proof_wanted(IPA_CURVE, k, 8000 + k)


S_COMBINE = ((7, 2), (12, 64))                                    # (k, batch): the staging of batch * (k + 1) scalars


@functools.lru_cache(maxsize=None)
def _s_combine_inputs(k, batch):
    rnd = random.Random(8100 + k)
    m = fields.MODULUS[FP]
    return [[rnd.randrange(m) for _ in range(k)] for _ in range(batch)], [rnd.randrange(m) for _ in range(batch)]


def _run_s_combine(shape, stream):
    k, batch = shape
    us, cs = _s_combine_inputs(k, batch)
    torch = _torch()
    out = torch.full((1 << k, 4), -1, dtype=torch.int64, device=fields.current_device())
    h.ipa_s_combine(k, fields.to_limbs([v for u in us for v in u], FP, True), fields.to_limbs(cs, FP, True), FP, out)
    return _down(out)


def _want_s_combine(shape):
    k, batch = shape
    us, cs = _s_combine_inputs(k, batch)
    m = fields.MODULUS[FP]
    total = [0] * (1 << k)
    for u, c in zip(us, cs):
        s = [c % m]
        for u_j in reversed(u):                                   # compute_s, poly/commitment/verifier.rs:156-172
            s += [v * u_j % m for v in s]
        total = [(a + b) % m for a, b in zip(total, s)]
    return _limbs(total)


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------------
EVAL_SHAPES = ("two-opcodes-L5", "stack-lagrange-L11-v0")        # one POLY and one SCALE over 2^5; every stack level over 2^11


@functools.lru_cache(maxsize=None)
def _eval_case(name):
    """(basis, log_len, words, consts, polys, omega, values) of an evaluator program and the integer model's run of it."""
    import evaluator_cases as ec
    import evaluator_model as em
    if name in ec.BY_NAME:
        mat = ec.materialize(ec.BY_NAME[name], FP)
        assert mat.depth == ec.MAX_DEPTH
        return mat.case.basis, mat.case.log_len, mat.words, mat.consts, mat.polys, mat.omega, mat.values
    log_len, m = 5, fields.MODULUS[FP]
    words, consts = [ec.word(ec.POLY, 0), ec.u32(3), ec.word(ec.SCALE, 0)], [ec.Y % m]
    polys = [ec.poly_values(("random", 0), 1 << log_len, m, name)]
    omega = ec.primitive_root(FP, log_len)
    values, _ = em.interpret(words, consts, polys, ec.LAGRANGE, 1 << log_len, m, omega)
    return ec.LAGRANGE, log_len, words, consts, polys, omega, values


def _run_evaluator(name, stream):
    basis, log_len, words, consts, polys, omega, _ = _eval_case(name)
    torch = _torch()
    tensors = [_up(fields.to_limbs(p, FP, True)) for p in polys]
    out = torch.empty((1 << log_len, 4), dtype=torch.int64, device=fields.current_device())
    prog = (C.c_uint32 * len(words))(*words)
    cst = np.ascontiguousarray(fields.to_limbs(consts or [0], FP, True))
    ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    rc = h.lib().h2_evaluate_device(FP, basis, prog, len(words), _p(cst), len(consts), ptrs, len(tensors), log_len, _p(_mont(FP, omega)),
                                    out.data_ptr(), C.c_void_p(stream.cuda_stream))
    assert rc == _lib.H2_OK, h.lib().h2_last_error()
    return _down(out)                                             # (the host arrays above live until the copy back has waited for the stream)


def _want_evaluator(name):
    return _limbs(_eval_case(name)[6])


# ---- the lookup argument's sort and permutation ---------------------------------------------------------------------------------------------
LOOKUP_SIZES = (31, 5000)                                         # padded to 32 keys, one tile; to 8192, several


@functools.lru_cache(maxsize=None)
def _lookup_inputs(n):
    rnd = random.Random(8200 + n)
    m = fields.MODULUS[FP]
    table_vals = [rnd.randrange(m) for _ in range(max(1, n // 8))]
    table = [rnd.choice(table_vals) for _ in range(n)]
    table[:len(table_vals)] = table_vals
    rnd.shuffle(table)
    present = sorted(set(table))
    return [rnd.choice(present) for _ in range(n)], table


def _run_sort(n, stream):
    return _down(sort_field(_up(fields.to_limbs(_lookup_inputs(n)[0], FP, True)), FP))


def _want_sort(n):
    return _limbs(sorted(_lookup_inputs(n)[0]))


def _run_permute(n, stream):
    inputs, table = _lookup_inputs(n)
    return _down(*permute_expression_pair(_up(fields.to_limbs(inputs, FP, True)), _up(fields.to_limbs(table, FP, True)), n, FP))


def _want_permute(n):
    a, s = olk.permute_expression_pair(*_lookup_inputs(n), n)
    return _limbs(a) + _limbs(s)


# ---- the MockProver's three checks ------------------------------------------------------------------------------------------------------
MOCK_KS = (5, 8)


@functools.lru_cache(maxsize=None)
def _mock_cases(k):
    """The shared test circuit with gate, copy and lookup faults (expressions, one-column lookups, the permutation) and a lookup of nine
    components with faults (two packed keys)."""
    import mock_prover_cases as cases
    m = fields.MODULUS[FP]
    return (cases.variant_case("full", m, k, cases.seeded_faults(m, k, "gate", 3)), cases.variant_case("full", m, k, cases.seeded_faults(m, k, "copy", 2)),
            cases.variant_case("full", m, k, cases.seeded_faults(m, k, "lookup", 2)), cases.wide_lookup_case(m, k=k, width=9, faults=5))


def _run_mock_prover(k, stream):
    import mock_prover_model as model
    from halo2_amd.dev import MockProver
    return repr([model.as_tuples(MockProver.run(*case, FP).verify(max_failures=1 << 30)) for case in _mock_cases(k)]).encode()


def _want_mock_prover(k):
    import mock_prover_model as model
    want = [model.verify(*case, fields.MODULUS[FP]) for case in _mock_cases(k)]
    assert all(want), "every case of the probe reports failures"
    return repr(want).encode()


# ---- the gadgets' bulk witness traces: 3 and 65 lanes of scratch ----------------------------------------------------------------------------
TRACE_COUNTS = (3, 65)


def _columns(per_lane, n_columns, field=FP) -> bytes:
    """Per-lane column lists [lane][column][row] as the (columns, rows * lanes, 4) array of the traces."""
    return b"".join(_limbs([v for lane in per_lane for v in lane[c]], field) for c in range(n_columns))


@functools.lru_cache(maxsize=None)
def _sinsemilla_messages(count):
    import sinsemilla_cases as sc
    nw = sc.STRUCTURES["merkle"]
    return nw, [sc.random_pieces(nw, 8300 + i, high_zero=i % 3 == 1) for i in range(count)]


def _pieces(msgs, nw):
    return fields.to_limbs([p for m in msgs for p in m], FP, montgomery=False).reshape(len(msgs), len(nw), 4)


def _run_sinsemilla_trace(count, stream):
    import sinsemilla_cases as sc
    nw, msgs = _sinsemilla_messages(count)
    cols, status = sinsemilla.trace(_up(_pieces(msgs, nw)), nw, sc.q_of(sc.MERKLE_DOMAIN), with_status=True)
    return _down(cols, status)


def _want_sinsemilla_trace(count):
    import sinsemilla_cases as sc
    nw, msgs = _sinsemilla_messages(count)
    q = sc.q_of(sc.MERKLE_DOMAIN)
    return _columns([sc.trace(q, m, nw) for m in msgs], 5) + bytes(count)


@functools.lru_cache(maxsize=None)
def _commit_messages(count):
    import sinsemilla_commit_cases as cc
    return cc.COMMIT_WORDS, cc.random_messages(cc.COMMIT_WORDS, count, seed=83), cc.private_qs()[:count]


def _run_commit_trace(count, stream):
    nw, msgs, qs = _commit_messages(count)
    q_limbs = fields.to_limbs([c for pt in qs for c in pt], FP).reshape(count, 8)
    cols, status = sinsemilla.trace_from(_up(_pieces(msgs, nw)), nw, _up(q_limbs), with_status=True)
    return _down(cols, status)


def _want_commit_trace(count):
    import sinsemilla_commit_cases as cc
    nw, msgs, qs = _commit_messages(count)
    return _columns([cc.trace_from(q, m, nw) for q, m in zip(qs, msgs)], 5) + bytes(count)


@functools.lru_cache(maxsize=None)
def _mul_inputs(count):
    import ecc_cases as ec
    alphas = [a % ec.P for a in ec.random_scalars(count, bits=254, seed=84)]
    alphas[0] = 0                                                 # the scalar that reaches the exceptional branches of complete addition
    return ec.random_bases(count, seed=85), alphas


def _run_mul_trace(count, stream):
    bases, alphas = _mul_inputs(count)
    b = fields.to_limbs([c for pt in bases for c in pt], FP).reshape(-1, 8)
    cols, aux, status = ecc.mul_trace(_up(b), _up(fields.to_limbs(alphas, FP)), with_status=True)
    return _down(cols, aux, status)


def _want_mul_trace(count):
    import ecc_cases as ec
    want = [ec.mul_trace(b, a) for b, a in zip(*_mul_inputs(count))]
    return _columns([w[0] for w in want], 10) + _limbs([v for w in want for v in w[1]]) + bytes(count)


@functools.lru_cache(maxsize=None)
def generator_fixed_base():
    """The Pallas generator's tables over 85 windows, built on the device once (torch tensors: no h2_trim touches them)."""
    import ecc_fixed_cases as fx
    return ecc.FixedBase(fields.to_limbs(list(fx.GENERATOR), FP).reshape(8), fx.NUM_WINDOWS)


@functools.lru_cache(maxsize=None)
def _fixed_scalars(count):
    import ecc_cases as ec
    import ecc_fixed_cases as fx
    return (fx.EDGE_SCALARS + ec.random_scalars(count, seed=86))[:count]


def _run_mul_fixed_trace(count, stream):
    cols, aux = ecc.mul_fixed_trace(generator_fixed_base(), _up(fields.to_limbs(_fixed_scalars(count), FP, montgomery=False)))
    return _down(cols, aux)


def _want_mul_fixed_trace(count):
    """The restated witness over the restated tables; the roots u are the device's (either root of y + z is a valid table: the table
    probe below checks their squares)."""
    import ecc_fixed_cases as fx
    table, us = fx.window_table(fx.GENERATOR, fx.NUM_WINDOWS), generator_fixed_base().u()
    want = [fx.mul_fixed_trace(table, us, k) for k in _fixed_scalars(count)]
    return _columns([w[0] for w in want], 6) + _limbs([v for w in want for v in w[1]])


def _run_fixed_tables(_, stream):
    """The four tables of a fixed base; the roots u leave as their squares (find_zs_and_us fixes them up to the sign)."""
    import ecc_fixed_cases as fx
    base = ecc.FixedBase(fields.to_limbs(list(fx.GENERATOR), FP).reshape(8), fx.NUM_WINDOWS)
    squares = [u * u % fx.P for row in base.u() for u in row]
    return _down(base.points, base.lagrange, base.zs) + _limbs(squares)


def _want_fixed_tables(_):
    import ecc_fixed_cases as fx
    table, coeffs, zs, _ = fx.generator_tables(fx.NUM_WINDOWS)
    return (_limbs([c for row in table for pt in row for c in pt]) + _limbs([c for row in coeffs for c in row]) + np.array(zs, dtype=np.uint64).tobytes()
            + _limbs([(pt[1] + z) % fx.P for row, z in zip(table, zs) for pt in row]))


MSM_FILES = ["msm_launch.hip"]
PROBES = [
    Probe("generic-multiexp-device", MSM_FILES, ["msm_release_workspaces"], (300, 70000), _run_generic_msm, _want_generic_msm),
    Probe("registered-commit-device", MSM_FILES, ["msm_release_workspaces"], COMMIT_SHAPES, _run_commit_device, _want_commit),
    Probe("registered-commit-host", MSM_FILES + ["msm_host.hip"], ["msm_release_workspaces"], COMMIT_SHAPES, _run_commit_host, _want_commit),
    Probe("ntt", ["ntt.hip"], ["ntt_release_workspaces"], NTT_LOGS, _run_ntt, _want_ntt),
    Probe("ifft", ["ntt.hip"], ["ntt_release_workspaces"], NTT_LOGS, _run_ifft, _want_ifft),
    Probe("coeff-to-extended", ["ntt.hip"], ["ntt_release_workspaces"], NTT_LOGS, _run_coeff_to_extended, _want_coeff_to_extended),
    _poly_probe("kate-division", lambda a, b, x, n: h.kate_division(a, x, POLY_FIELD), lambda a, b, x, n: co.kate_division(POLY_FIELD, a, x)),
    _poly_probe("grand-product", lambda a, b, x, n: h.grand_product(a, n, x, POLY_FIELD), lambda a, b, x, n: co.grand_product(POLY_FIELD, a, n, x)),
    _poly_probe("eval-polynomial", lambda a, b, x, n: h.eval_polynomial(a, x, POLY_FIELD), lambda a, b, x, n: co.eval_polynomial(POLY_FIELD, a, x)),
    _poly_probe("inner-product", lambda a, b, x, n: h.compute_inner_product(a, b, POLY_FIELD), lambda a, b, x, n: co.inner_product(POLY_FIELD, a, b)),
    Probe("generator-collapse", ["ipa.hip"], ["ipa_release_workspaces"], IPA_KS, _run_generator_collapse, _want_generator_collapse),
    Probe("ipa-round-scalars", ["ipa.hip"], ["ipa_release_workspaces"], ROUND_SCALARS, _run_round_scalars, _want_round_scalars),
    Probe("open-device", ["ipa.hip"] + MSM_FILES, ["ipa_release_workspaces", "msm_release_workspaces", "poly_release_workspaces"], IPA_KS,
          _run_open_device, _want_open_device),
    Probe("ipa-s-combine", ["verify.hip"], ["verify_release_workspaces"], S_COMBINE, _run_s_combine, _want_s_combine),
    Probe("evaluator", ["evaluator.hip"], ["eval_release_workspaces"], EVAL_SHAPES, _run_evaluator, _want_evaluator),
    Probe("sort-field", ["lookup.hip"], ["lookup_release_workspaces"], LOOKUP_SIZES, _run_sort, _want_sort),
    Probe("permute-expression-pair", ["lookup.hip"], ["lookup_release_workspaces"], LOOKUP_SIZES, _run_permute, _want_permute),
    Probe("mock-prover", ["mock_prover.hip", "lookup.hip", "evaluator.hip"], ["mock_release_workspaces"], MOCK_KS, _run_mock_prover, _want_mock_prover),
    Probe("sinsemilla-trace", ["sinsemilla.hip"], ["sinsemilla_release_workspaces"], TRACE_COUNTS, _run_sinsemilla_trace, _want_sinsemilla_trace),
    Probe("ecc-mul-trace", ["ecc.hip"], ["ecc_release_workspaces"], TRACE_COUNTS, _run_mul_trace, _want_mul_trace),
    Probe("ecc-mul-fixed-trace", ["ecc_fixed.hip"], ["ecc_fixed_release_workspaces"], TRACE_COUNTS, _run_mul_fixed_trace, _want_mul_fixed_trace),
    Probe("commit-domain-trace", ["sinsemilla_commit.hip"], ["sinsemilla_commit_release_workspaces"], TRACE_COUNTS, _run_commit_trace, _want_commit_trace),
    Probe("fixed-base-tables", ["ecc_fixed.hip"], ["ecc_fixed_release_workspaces"], ("generator", 85), _run_fixed_tables, _want_fixed_tables,
          single_size=True),
]
BY_NAME = {p.name: p for p in PROBES}
