"""Shared by test_poseidon_spec_host.py and the test_gpu_poseidon_spec*.py files (a helper: nothing here is collected): the grid of
specifications, every call h2_poseidon_spec_*_device must refuse, the stream-order case of each of the three entry points (the pieces
tests/stream_cases.py defines, whose table cannot hold them because their stream travels in the descriptor), and the reference
benchmark's HashCircuit<S, WIDTH, RATE, L> (halo2_gadgets/benches/poseidon.rs:22-105) against halo2_amd.circuit."""
import ctypes as C
import os
import re

import numpy as np

import poseidon_model as pm
from halo2_amd import _lib
from halo2_amd.circuit import Circuit

FP, FQ = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "halo2_mi355x.h")
SOURCE = os.path.join(ROOT, "halo2_amd", "csrc", "poseidon_spec.hip")

# (width, rate, full rounds, partial rounds)
GRID = [(2, 1, 8, 56), (3, 2, 8, 56), (9, 8, 8, 56), (12, 11, 8, 56), (4, 2, 2, 0), (5, 4, 8, 57)]
TRACE_GRID = [(3, 2, 8, 56), (9, 8, 8, 56), (12, 11, 8, 56), (4, 3, 2, 2)]
COUNTS = [1, 65, 257]                                    # one lane, two waves, more than two workgroups


def spec_prototypes(header=HEADER):
    """{name: parameter list} of the h2_poseidon_spec_* functions the header declares"""
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    return {name: params for name, params in re.findall(r"\bint\s+(h2_poseidon_spec_\w+)\s*\(([^()]*)\)\s*;", text)}


def descriptor(field=FP, width=3, rate=2, full=8, partial=56, constants=0x1000, stream=0):
    return _lib.PoseidonSpec(field, width, rate, full, partial, constants, stream)


def refusals(d_in=0x1000, d_out=0x2000, d_constants=0x3000):
    """[(what, entry point, descriptor or None, the arguments after it)]: every one is H2_ERR_ARGS before anything touches the device.
    The pointers are never read, so without a device any nonzero value does."""
    big = (1 << 30) + 1
    good = lambda **kw: descriptor(constants=d_constants, **kw)
    rows = []
    for entry, tail in (("h2_poseidon_spec_permute_device", (d_in, 1, d_out)), ("h2_poseidon_spec_hash_device", (d_in, 1, 3, d_out)),
                        ("h2_poseidon_spec_trace_device", (d_in, 1, d_out))):
        with_n = lambda n, tail=tail: (tail[0], n) + tail[2:]
        rows += [
            ("a null spec", entry, None, tail),
            ("an unknown field", entry, good(field=2), tail),
            ("a negative field", entry, good(field=-1), tail),
            ("width 1", entry, good(width=1, rate=1), tail),
            ("width 13", entry, good(width=13, rate=12), tail),
            ("rate 0", entry, good(rate=0), tail),
            ("rate = width", entry, good(rate=3), tail),
            ("odd full rounds", entry, good(full=7), tail),
            ("no full rounds", entry, good(full=0), tail),
            ("1025 rounds", entry, good(full=8, partial=1017), tail),
            ("partial rounds that wrap", entry, good(full=8, partial=0xFFFFFFFC), tail),
            ("null constants", entry, descriptor(constants=None), tail),
            ("null input", entry, good(), (None,) + tail[1:]),
            ("null output", entry, good(), tail[:-1] + (None,)),
            ("2^30 + 1 of them", entry, good(), with_n(big)),
        ]
    hash_ = "h2_poseidon_spec_hash_device"
    rows += [
        ("len 0", hash_, good(), (d_in, 1, 0, d_out)),
        ("len 2^32", hash_, good(), (d_in, 1, 1 << 32, d_out)),
        ("n * len above 2^40", hash_, good(), (d_in, 1 << 30, 1025, d_out)),
        ("odd partial rounds", "h2_poseidon_spec_trace_device", good(width=5, rate=4, partial=57), (d_in, 1, d_out)),
    ]
    return rows


def refuse(lib, row):
    _, entry, spec, tail = row
    return getattr(lib, entry)(None if spec is None else C.byref(spec), *tail)


# ---- stream order ---------------------------------------------------------------------------------------------------------------------------
STREAM_SPEC = (9, 8, 8, 56)
STREAM_LANES = 65                                        # two workgroups
STREAM_LEN = 9                                           # two permutations a message, seven words of padding


def _stream_cases():
    import stream_cases as sc
    model = pm.model(FP, *STREAM_SPEC)
    width = model.width
    states = lambda seed: pm.random_states(STREAM_LANES, width, FP, 0x5EC0 + seed)
    flat = lambda rows: sc.limbs([v for row in rows for v in row], FP).reshape(len(rows), -1, 4)

    def call(entry, tail):
        def run(ins, outs, stream_ptr):
            from halo2_amd import poseidon
            d = poseidon.spec_descriptor(model.spec(), "cuda:0", stream=stream_ptr)
            sc.ok(getattr(sc._lib(), entry)(C.byref(d), *tail(ins, outs)))
        return run
    return {
        "h2_poseidon_spec_permute_device": sc.Case(
            "poseidon-spec-permute", "h2_poseidon_spec_permute_device", STREAM_LANES, lambda seed: {"states": flat(states(seed))},
            lambda: {"out": 32 * width * STREAM_LANES},
            call("h2_poseidon_spec_permute_device", lambda i, u: (i["states"].data_ptr(), STREAM_LANES, u["out"].data_ptr())),
            lambda seed: sc._b(flat([model.permute(s) for s in states(seed)])), sc.fields_valid(FP, "states")),
        "h2_poseidon_spec_hash_device": sc.Case(
            "poseidon-spec-hash", "h2_poseidon_spec_hash_device", (STREAM_LANES, STREAM_LEN), lambda seed: {"messages": flat(states(seed))},
            lambda: {"out": 32 * STREAM_LANES},
            call("h2_poseidon_spec_hash_device", lambda i, u: (i["messages"].data_ptr(), STREAM_LANES, STREAM_LEN, u["out"].data_ptr())),
            lambda seed: sc._b(sc.limbs([model.hash(msg) for msg in states(seed)], FP)), sc.fields_valid(FP, "messages")),
        "h2_poseidon_spec_trace_device": sc.Case(
            "poseidon-spec-trace", "h2_poseidon_spec_trace_device", STREAM_LANES, lambda seed: {"states": flat(states(seed))},
            lambda: {"columns": (width + 1) * model.rows * STREAM_LANES * 32},
            call("h2_poseidon_spec_trace_device", lambda i, u: (i["states"].data_ptr(), STREAM_LANES, u["columns"].data_ptr())),
            lambda seed: sc._b(model.trace_limbs(states(seed))), sc.fields_valid(FP, "states")),
    }


_cases = None


def stream_cases():
    global _cases
    if _cases is None:
        _cases = _stream_cases()
    return _cases


STREAM_ENTRIES = ("h2_poseidon_spec_permute_device", "h2_poseidon_spec_hash_device", "h2_poseidon_spec_trace_device")


# ---- the reference benchmark's circuit ----------------------------------------------------------------------------------------------------
class WideHashCircuit(Circuit):
    """HashCircuit<S, WIDTH, RATE, L> (benches/poseidon.rs): the message is witnessed in the state columns, hashed with
    ConstantLength<L>, and the digest is constrained to row 0 of the instance column `expected`."""

    def __init__(self, key, length, message=None, field=FP):
        self.key, self.length, self.message, self.field = key, length, message, field

    def without_witnesses(self):
        return WideHashCircuit(self.key, self.length, field=self.field)

    def configure(self, meta):
        from halo2_amd.gadgets.poseidon import Pow5Chip
        from halo2_amd.poseidon_spec import Spec
        width = self.key[0]
        state = [meta.advice_column() for _ in range(width)]
        expected = meta.instance_column()
        meta.enable_equality(expected)
        partial_sbox = meta.advice_column()
        rc_a = [meta.fixed_column() for _ in range(width)]
        rc_b = [meta.fixed_column() for _ in range(width)]
        meta.enable_constant(rc_b[0])
        return Pow5Chip.configure(meta, state, partial_sbox, rc_a, rc_b, spec=Spec(self.field, *self.key)), expected

    def synthesize(self, config, layouter):
        from halo2_amd.gadgets.poseidon import ConstantLength, Hash, Pow5Chip
        config, expected_column = config
        chip = Pow5Chip.construct(config)
        width = self.key[0]
        word = lambda i: None if self.message is None else self.message[i]
        # the bench loads L <= RATE words on one row; a longer message goes on further rows of the same columns
        message = layouter.assign_region("load message", lambda region: [
            region.assign_advice(config.state[i % width], i // width, lambda i=i: word(i)) for i in range(self.length)])
        hasher = Hash.init(chip, layouter.namespace("init"), ConstantLength(self.length))
        output = hasher.hash(layouter.namespace("hash"), message)
        self.output_cell = output.cell()
        layouter.constrain_instance(output.cell(), expected_column, 0)


def configure_wide(meta, key, field=FP):
    from halo2_amd.gadgets.poseidon import Pow5Chip
    from halo2_amd.poseidon_spec import Spec
    width = key[0]
    state = [meta.advice_column() for _ in range(width)]
    partial_sbox = meta.advice_column()
    rc_a = [meta.fixed_column() for _ in range(width)]
    rc_b = [meta.fixed_column() for _ in range(width)]
    meta.enable_constant(rc_b[0])
    return Pow5Chip.configure(meta, state, partial_sbox, rc_a, rc_b, spec=Spec(field, *key))


class WidePermuteManyCircuit(Circuit):
    """`count` permutations through `permute_many` alone, the region on row 0.  states: (count, width, 4) limbs or None; trace: the
    chip's columns where the test hands in its own (a tampered witness)."""

    def __init__(self, key, count, states=None, trace=None):
        self.key, self.count, self.states, self.trace = key, count, states, trace
        self.result = None

    def without_witnesses(self):
        return WidePermuteManyCircuit(self.key, self.count)

    def configure(self, meta):
        return configure_wide(meta, self.key)

    def synthesize(self, config, layouter):
        from halo2_amd.gadgets.poseidon import Pow5Chip
        self.result = Pow5Chip.construct(config).permute_many(layouter, self.count, self.states, trace=self.trace)


class WideMirrorCircuit(Circuit):
    """An inputs region of `width` columns x `count` rows, then the permutations of those rows: `count` calls of `permute`
    (bulk=False) or one `permute_many` whose input cells are copied from the same input cells (bulk=True).  With hashing=True the
    rows are messages of `rate` words: `count` times Hash<ConstantLength<rate>>.hash, or one `hash_many`."""

    def __init__(self, key, inputs, bulk, hashing=False, field=FP):
        self.key, self.inputs, self.bulk, self.hashing, self.field = key, inputs, bulk, hashing, field
        self.outputs = None

    def without_witnesses(self):
        return WideMirrorCircuit(self.key, self.inputs, self.bulk, self.hashing, self.field)      # its witness is no secret

    def configure(self, meta):
        return configure_wide(meta, self.key, self.field)

    def synthesize(self, config, layouter):
        from halo2_amd.gadgets.poseidon import ConstantLength, Hash, Pow5Chip
        count, per_row = len(self.inputs), len(self.inputs[0])
        cells = layouter.assign_region("inputs", lambda region: [
            [region.assign_advice(config.state[j], i, self.inputs[i][j]) for j in range(per_row)] for i in range(count)])
        chip = Pow5Chip.construct(config)
        limbs = limbs_of([w for row in self.inputs for w in row], config.field).reshape(count, per_row, 4)
        if not self.bulk:
            if self.hashing:
                self.outputs = [Hash.init(chip, layouter.namespace("init"), ConstantLength(per_row)).hash(layouter.namespace("hash"), cells[i]).cell()
                                for i in range(count)]
            else:
                self.outputs = [[c.cell() for c in chip.permute(layouter, cells[i])] for i in range(count)]
            return
        many = chip.hash_many(layouter, count, limbs) if self.hashing else chip.permute_many(layouter, count, limbs)
        self.many = many

        def tie(region):
            for i in range(count):
                for j in range(per_row):
                    region.constrain_equal(many.input_cell(i, j), cells[i][j].cell())
        layouter.assign_region("tie inputs", tie)


def limbs_of(ints, field):
    from halo2_amd import fields
    return fields.to_limbs([int(v) for v in ints], field, True)


def ints_of(a, field):
    from halo2_amd import fields
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), field, True)
