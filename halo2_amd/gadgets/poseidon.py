"""The Poseidon gadget of halo2_gadgets (src/poseidon.rs, src/poseidon/pow5.rs) against `halo2_amd.circuit`: `Pow5Chip`, `Sponge`,
`Hash` and `ConstantLength` over the field of the constraint system: P128Pow5T3 (width 3, rate 2) by default, and with `spec=` any
`halo2_amd.poseidon_spec.Spec` of rate = width - 1 and even round counts, as Pow5Chip<F, WIDTH, RATE> is generic over them.

The mirror assigns cell by cell with host integers -- the same regions, offsets, gate names and copy constraints as the reference:
one full round per row, two partial rounds per row, R_F + R_P / 2 + 1 rows per permutation (37 for P128Pow5T3).

    config = Pow5Chip.configure(meta, state, partial_sbox, rc_a, rc_b)
    digest = Hash.init(Pow5Chip(config), layouter, ConstantLength(2)).hash(layouter, [left, right])      # AssignedCells

What the reference does not have is the bulk path: `Pow5Chip.permute_many` / `hash2_many` / `hash_many` lay `count` permutations back
to back in ONE region whose width + 1 advice columns come from the device (`halo2_amd.poseidon.trace`, or `Spec.trace` with a spec)
and whose fixed columns are the constant pattern of one permutation tiled on the device; cell for cell the same layout as `count`
calls of `permute`."""
from __future__ import annotations

import numpy as np

from .. import fields, poseidon, poseidon_spec
from ..circuit import AssignedCell, Cell, Column, ConstraintSystem, Selector, Synthesis
from ..poseidon_spec import FULL_ROUNDS, PARTIAL_ROUNDS, RATE, ROWS, WIDTH, Spec

HALF_FULL, HALF_PARTIAL = FULL_ROUNDS // 2, PARTIAL_ROUNDS // 2
FULL_OFFSETS = list(range(HALF_FULL)) + list(range(HALF_FULL + HALF_PARTIAL, ROWS - 1))        # rows 0-3 and 32-35 of a permutation
PARTIAL_OFFSETS = list(range(HALF_FULL, HALF_FULL + HALF_PARTIAL))                              # rows 4-31
# (the five names above are P128Pow5T3's; a chip reads its own from its config)


class ConstantLength:
    """primitives::ConstantLength<L>: a hash of exactly L field elements."""

    def __init__(self, length: int):
        if length < 1:
            raise ValueError("ConstantLength: at least one element")
        self.length = length

    def name(self) -> str:
        return f"ConstantLength<{self.length}>"

    def initial_capacity_element(self) -> int:
        return poseidon_spec.capacity(self.length)

    def padding(self, rate: int = RATE) -> list:
        """zeros up to the next multiple of the rate"""
        return [0] * (-self.length % rate)


class Pow5Config:
    def __init__(self, field, state, partial_sbox, rc_a, rc_b, s_full, s_partial, s_pad_and_add, spec=None):
        self.field, self.modulus = field, fields.MODULUS[field]
        self.state, self.partial_sbox, self.rc_a, self.rc_b = list(state), partial_sbox, list(rc_a), list(rc_b)
        self.s_full, self.s_partial, self.s_pad_and_add = s_full, s_partial, s_pad_and_add
        self.spec = spec                                                      # None: P128Pow5T3 through the kernels of csrc/poseidon.hip
        shape = Spec.p128pow5t3(field) if spec is None else spec
        self.round_constants, self.m_reg, self.m_inv = shape.round_constants, shape.mds, shape.mds_inv
        self.width, self.rate, self.rows = shape.width, shape.rate, shape.rows
        self.full_rounds, self.partial_rounds = shape.full_rounds, shape.partial_rounds
        self.half_full, self.half_partial = shape.full_rounds // 2, shape.partial_rounds // 2
        self.full_offsets = list(range(self.half_full)) + list(range(self.half_full + self.half_partial, self.rows - 1))
        self.partial_offsets = list(range(self.half_full, self.half_full + self.half_partial))

    def trace(self, states):
        """the chip's advice columns of the permutations of `states`, from the device"""
        return poseidon.trace(states, self.field) if self.spec is None else self.spec.trace(states)


def _pow_5(v):
    v2 = v * v
    return v2 * v2 * v


def _sum(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def _value(cell: AssignedCell, m: int):
    """the integer in an assigned cell, None where the pass has no witness"""
    v = cell.value().inner
    return None if v is None else v.evaluate(m) if hasattr(v, "evaluate") else int(v) % m


class PermuteMany:
    """What `permute_many` returns: the cells of every permutation's input and output words, and the outputs on the device."""

    def __init__(self, region_index: int, state, count: int, outputs, rows: int = ROWS):
        self.region_index, self.state, self.count, self.outputs, self.rows = region_index, state, count, outputs, rows

    def _cell(self, i: int, j: int, row: int) -> Cell:
        if not (0 <= i < self.count and 0 <= j < len(self.state)):
            raise IndexError((i, j))
        return Cell(self.region_index, self.rows * i + row, self.state[j])

    def input_cell(self, i: int, j: int) -> Cell:
        return self._cell(i, j, 0)

    def output_cell(self, i: int, j: int) -> Cell:
        return self._cell(i, j, self.rows - 1)


class Hash2Many:
    """What `hash2_many` returns: `left_cell(i)`, `right_cell(i)`, `output_cell(i)` and the (count, 4) digests on the device."""

    def __init__(self, permutations: PermuteMany):
        self.permutations, self.count = permutations, permutations.count
        self.digests = None if permutations.outputs is None else permutations.outputs[:, 0]

    def left_cell(self, i: int) -> Cell:
        return self.permutations.input_cell(i, 0)

    def right_cell(self, i: int) -> Cell:
        return self.permutations.input_cell(i, 1)

    def output_cell(self, i: int) -> Cell:
        return self.permutations.output_cell(i, 0)


class HashMany:
    """What `hash_many` returns: `input_cell(i, j)` of word j of message i, `output_cell(i)` and the (count, 4) digests on the device."""

    def __init__(self, permutations: PermuteMany):
        self.permutations, self.count = permutations, permutations.count
        self.digests = None if permutations.outputs is None else permutations.outputs[:, 0]

    def input_cell(self, i: int, j: int) -> Cell:
        if not 0 <= j < len(self.permutations.state) - 1:
            raise IndexError((i, j))
        return self.permutations.input_cell(i, j)

    def output_cell(self, i: int) -> Cell:
        return self.permutations.output_cell(i, 0)


class Pow5Chip:
    """poseidon::Pow5Chip<F, WIDTH, RATE> (pow5.rs:42-208)."""

    def __init__(self, config: Pow5Config):
        self.config = config

    @classmethod
    def construct(cls, config: Pow5Config) -> "Pow5Chip":
        return cls(config)

    @staticmethod
    def configure(meta: ConstraintSystem, state, partial_sbox: Column, rc_a, rc_b, field: int | None = None, spec: Spec | None = None) -> Pow5Config:
        """The three gates (pow5.rs:56-202).  Side effect: the state and rc_b columns become equality-enabled.  `field` defaults to the
        one whose modulus the constraint system carries.  spec: None is P128Pow5T3; a Spec must have rate = width - 1 and even round
        counts (pow5.rs:63-67), its field must be the chip's, and `width` columns of each kind are wanted."""
        if field is None:
            field = next((f for f, m in fields.MODULUS.items() if m == meta.modulus), None)
            if field is None:
                raise ValueError("Pow5Chip.configure: the constraint system has no Pasta modulus; pass field=")
        if spec is None:
            if not (len(state) == len(rc_a) == len(rc_b) == WIDTH):
                raise ValueError("Pow5Chip.configure: three state, rc_a and rc_b columns")
        else:
            if spec.field != field:
                raise ValueError("Pow5Chip.configure: the spec is over the other field")
            if spec.rate != spec.width - 1:
                raise ValueError("Pow5Chip.configure: the chip needs rate = width - 1")
            if spec.full_rounds % 2 or spec.partial_rounds % 2:
                raise ValueError("Pow5Chip.configure: the chip needs even numbers of full and of partial rounds")
            if not (len(state) == len(rc_a) == len(rc_b) == spec.width):
                raise ValueError(f"Pow5Chip.configure: {spec.width} state, rc_a and rc_b columns")
        for column in list(state) + list(rc_b):
            meta.enable_equality(column)
        s_full, s_partial, s_pad_and_add = meta.selector(), meta.selector(), meta.selector()
        c = config = Pow5Config(field, state, partial_sbox, rc_a, rc_b, s_full, s_partial, s_pad_and_add, spec)
        m_reg, m_inv = config.m_reg, config.m_inv

        def full_round(cells):
            s = cells.query_selector(s_full)
            polys = []
            for next_idx in range(c.width):
                state_next = cells.query_advice(state[next_idx], 1)
                terms = []
                for idx in range(c.width):
                    state_cur = cells.query_advice(state[idx], 0)
                    rc = cells.query_fixed(rc_a[idx])
                    terms.append(_pow_5(state_cur + rc) * m_reg[next_idx][idx])
                polys.append(s * (_sum(terms) - state_next))
            return polys
        meta.create_gate("full round", full_round)

        def partial_rounds(cells):
            cur_0 = cells.query_advice(state[0], 0)
            mid_0 = cells.query_advice(partial_sbox, 0)
            rc_a0, rc_b0 = cells.query_fixed(rc_a[0]), cells.query_fixed(rc_b[0])
            s = cells.query_selector(s_partial)

            def mid(idx):
                acc = mid_0 * m_reg[idx][0]
                for cur_idx in range(1, c.width):
                    cur = cells.query_advice(state[cur_idx], 0)
                    rc = cells.query_fixed(rc_a[cur_idx])
                    acc = acc + (cur + rc) * m_reg[idx][cur_idx]
                return acc

            def nxt(idx):
                return _sum([cells.query_advice(state[next_idx], 1) * m_inv[idx][next_idx] for next_idx in range(c.width)])

            def partial_round_linear(idx):
                rc = cells.query_fixed(rc_b[idx])
                return mid(idx) + rc - nxt(idx)
            polys = [_pow_5(cur_0 + rc_a0) - mid_0,                            # state[0] round a
                     _pow_5(mid(0) + rc_b0) - nxt(0)]                          # state[0] round b
            polys += [partial_round_linear(idx) for idx in range(1, c.width)]
            return [s * p for p in polys]
        meta.create_gate("partial rounds", partial_rounds)

        def pad_and_add(cells):
            initial_state_rate = cells.query_advice(state[c.rate], -1)
            output_state_rate = cells.query_advice(state[c.rate], 1)
            s = cells.query_selector(s_pad_and_add)
            polys = []
            for idx in range(c.rate):
                initial_state = cells.query_advice(state[idx], -1)
                word = cells.query_advice(state[idx], 0)
                output_state = cells.query_advice(state[idx], 1)
                polys.append(initial_state + word - output_state)             # the padding sits in rc_b, copied into `word`
            polys.append(initial_state_rate - output_state_rate)              # the capacity element is never altered by the input
            return [s * p for p in polys]
        meta.create_gate("pad-and-add", pad_and_add)
        return config

    # ---- PoseidonInstructions (pow5.rs:223-271, 435-597) ---------------------------------------------------------------------------
    def _round(self, region, state, round_: int, offset: int, gate: Selector, round_fn):
        c = self.config
        gate.enable(region, offset)
        for i in range(c.width):
            region.assign_fixed(c.rc_a[i], offset, c.round_constants[round_][i])
        next_state = round_fn(region, state)
        return [region.assign_advice(c.state[i], offset + 1, lambda v=next_state[i]: v) for i in range(c.width)]

    def _apply_mds(self, r):
        c, m, mds = self.config, self.config.modulus, self.config.m_reg
        return [sum(mds[i][j] * r[j] for j in range(c.width)) % m for i in range(c.width)]

    def _full_round(self, region, state, round_: int, offset: int):
        c, m = self.config, self.config.modulus

        def fn(_, words):
            p = [_value(w, m) for w in words]
            if None in p:
                return [None] * c.width
            return self._apply_mds([pow((p[i] + c.round_constants[round_][i]) % m, 5, m) for i in range(c.width)])
        return self._round(region, state, round_, offset, c.s_full, fn)

    def _partial_round(self, region, state, round_: int, offset: int):
        c, m = self.config, self.config.modulus

        def sbox_first(p, rc):
            return [pow((p[0] + rc[0]) % m, 5, m)] + [(p[i] + rc[i]) % m for i in range(1, c.width)]

        def fn(region_, words):
            p = [_value(w, m) for w in words]
            known = None not in p
            r = sbox_first(p, c.round_constants[round_]) if known else None
            region_.assign_advice(c.partial_sbox, offset, lambda: r[0] if known else None)
            for i in range(c.width):                                            # the second round's constants
                region_.assign_fixed(c.rc_b[i], offset, c.round_constants[round_ + 1][i])
            if not known:
                return [None] * c.width
            return self._apply_mds(sbox_first(self._apply_mds(r), c.round_constants[round_ + 1]))
        return self._round(region, state, round_, offset, c.s_partial, fn)

    def permute(self, layouter, initial_state) -> list:
        """One permutation in a region of `rows` rows (37); initial_state and the result are `width` AssignedCells."""
        c = self.config

        def assign(region):
            state = [initial_state[i].copy_advice(region, c.state[i], 0) for i in range(c.width)]
            for r in range(c.half_full):
                state = self._full_round(region, state, r, r)
            for r in range(c.half_partial):
                state = self._partial_round(region, state, c.half_full + 2 * r, c.half_full + r)
            for r in range(c.half_full):
                state = self._full_round(region, state, c.half_full + 2 * c.half_partial + r, c.half_full + c.half_partial + r)
            return state
        return layouter.assign_region("permute state", assign)

    # ---- PoseidonSpongeInstructions (pow5.rs:273-406) --------------------------------------------------------------------------------
    def initial_state(self, layouter, domain: ConstantLength) -> list:
        c = self.config

        def assign(region):
            values = [0] * c.rate + [domain.initial_capacity_element()]
            return [region.assign_advice_from_constant(c.state[i], 0, values[i]) for i in range(c.width)]
        return layouter.assign_region(f"initial state for domain {domain.name()}", assign)

    def add_input(self, layouter, initial_state, words, domain: ConstantLength) -> list:
        """words: `rate` entries, ("message", AssignedCell) or ("padding", integer)."""
        c, m = self.config, self.config.modulus
        if len(words) != c.rate:
            raise ValueError("Input is not padded")

        def assign(region):
            c.s_pad_and_add.enable(region, 1)
            initial = [initial_state[i].copy_advice(region, c.state[i], 0) for i in range(c.width)]
            loaded = []
            for i, (kind, word) in enumerate(words):
                if kind == "message":
                    cell, value = word.cell(), _value(word, m)
                else:
                    cell, value = region.assign_fixed(c.rc_b[i], 1, word).cell(), word
                var = region.assign_advice(c.state[i], 1, lambda v=value: v)
                region.constrain_equal(cell, var.cell())
                loaded.append(value)
            out = []
            for i in range(c.width):
                a, b = _value(initial[i], m), loaded[i] if i < c.rate else 0
                out.append(region.assign_advice(c.state[i], 2, lambda v=(None if a is None or b is None else (a + b) % m): v))
            return out
        return layouter.assign_region(f"add input for domain {domain.name()}", assign)

    def get_output(self, state) -> list:
        return list(state[:self.config.rate])

    # ---- the bulk path ---------------------------------------------------------------------------------------------------------------
    def _pattern(self, device):
        """(rc_a x width, rc_b x width) as (rows, 4) device tensors: rc_a holds the constant of the round that starts on the row, rc_b
        the second round of a partial pair, zero elsewhere."""
        import torch
        c = self.config
        first = list(range(c.half_full)) + [c.half_full + 2 * r for r in range(c.half_partial)] + \
            [c.half_full + c.partial_rounds + r for r in range(c.half_full)]
        columns = []
        for i in range(c.width):
            columns.append([c.round_constants[r][i] for r in first] + [0])
        for i in range(c.width):
            columns.append([c.round_constants[c.half_full + 2 * (o - c.half_full) + 1][i] if o in c.partial_offsets else 0 for o in range(c.rows)])
        return [torch.from_numpy(fields.to_limbs(col, c.field, True).view(np.int64)).to(device) for col in columns]

    def permute_many(self, layouter, count: int, states=None, trace=None, constants=()) -> PermuteMany:
        """`count` permutations back to back in one region of rows * count rows (rows = 37 for P128Pow5T3); permutation i owns rows
        rows i .. rows i + rows - 1.

        states: a (count, width, 4) Montgomery tensor or array of the inputs; None when there is no witness (keygen), which lays out the
        same shape and launches nothing.  trace: the (width + 1, rows * count, 4) columns where the caller already has them (else
        `poseidon.trace(states)` or the spec's `trace`, once).  constants: (word, integer) pairs -- that input word of every permutation is constrained to
        the constant (needs `enable_constant`)."""
        import torch
        c = self.config
        backend = layouter.cs
        rows = c.rows * count
        if states is None and trace is None and backend.collect_advice:
            raise Synthesis("permute_many: a witness is needed and there is none")
        if not backend.collect_advice:
            trace = None                                                      # keygen never looks at a witness
        elif trace is None:
            trace = c.trace(states)
        if trace is not None:
            if not torch.is_tensor(trace):
                trace = torch.from_numpy(np.ascontiguousarray(trace, dtype=np.uint64).view(np.int64))
            if tuple(trace.shape) != (c.width + 1, rows, 4):
                raise ValueError(f"permute_many: the trace is ({c.width + 1}, {c.rows} * count, 4)")
        blank = np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (rows, 4))    # the shape of a column, for the passes that keep none
        advice = [blank] * (c.width + 1) if trace is None else [trace[j] for j in range(c.width + 1)]
        fixed = [blank] * (2 * c.width)
        if backend.collect_fixed and count:
            fixed = [p.repeat(count, 1) for p in self._pattern(fields.current_device())]
        base = c.rows * np.arange(count, dtype=np.int64)[:, None]
        full = (base + np.array(c.full_offsets, dtype=np.int64)[None, :]).reshape(-1)
        partial = (base + np.array(c.partial_offsets, dtype=np.int64)[None, :]).reshape(-1)

        def assign(region):
            for j in range(c.width):
                region.assign_advice_column(c.state[j], 0, advice[j])
            region.assign_advice_column(c.partial_sbox, 0, advice[c.width])
            for j in range(c.width):
                region.assign_fixed_column(c.rc_a[j], 0, fixed[j])
                region.assign_fixed_column(c.rc_b[j], 0, fixed[c.width + j])
            region.enable_selector_rows(c.s_full, full)
            region.enable_selector_rows(c.s_partial, partial)
            for word, constant in constants:
                for i in range(count):
                    region.constrain_constant(Cell(region.region_index, c.rows * i, c.state[word]), constant)
            return region.region_index
        region_index = layouter.assign_region("permute many", assign)
        outputs = None
        if trace is not None:
            outputs = torch.stack([trace[j].view(count, c.rows, 4)[:, c.rows - 1] for j in range(c.width)], dim=1)
        return PermuteMany(region_index, c.state, count, outputs, c.rows)

    def hash2_many(self, layouter, count: int, left=None, right=None) -> Hash2Many:
        """`count` hashes of two elements (ConstantLength<2>): the permutation of (left, right, 2^65), word 0 of the output.  left,
        right: (count, 4) Montgomery tensors or arrays, None without a witness.  Every capacity cell is constrained to the constant
        2^65, so the circuit needs `enable_constant` on some fixed column."""
        import torch
        c = self.config
        if c.rate != 2:
            raise ValueError("hash2_many: a chip of rate 2; hash_many takes any rate")
        cap = poseidon_spec.capacity(2)
        states = None
        if left is not None and right is not None and layouter.cs.collect_advice:
            dev = fields.current_device()
            l, r = fields.to_device_limbs(left, dev), fields.to_device_limbs(right, dev)
            if tuple(l.shape) != (count, 4) or tuple(r.shape) != (count, 4):
                raise ValueError("hash2_many: left and right are (count, 4)")
            capacity = torch.from_numpy(fields.to_limbs([cap], c.field, True).view(np.int64)).to(dev).expand(count, 4)
            states = torch.stack([l, r, capacity], dim=1).contiguous()
        return Hash2Many(self.permute_many(layouter, count, states, constants=((c.rate, cap),)))

    def hash_many(self, layouter, count: int, messages=None) -> HashMany:
        """`count` hashes of `rate` elements each (ConstantLength<rate>, one permutation a message): the permutation of (message,
        rate * 2^64), word 0 of the output.  messages: a (count, rate, 4) Montgomery tensor or array, None without a witness.  Every
        capacity cell is constrained to the constant, so the circuit needs `enable_constant` on some fixed column."""
        import torch
        c = self.config
        cap = poseidon_spec.capacity(c.rate)
        states = None
        if messages is not None and layouter.cs.collect_advice:
            dev = fields.current_device()
            if not torch.is_tensor(messages):
                messages = torch.from_numpy(np.ascontiguousarray(messages, dtype=np.uint64).view(np.int64))
            messages = messages.to(dev)
            if tuple(messages.shape) != (count, c.rate, 4):
                raise ValueError(f"hash_many: messages are (count, {c.rate}, 4)")
            capacity = torch.from_numpy(fields.to_limbs([cap], c.field, True).view(np.int64)).to(dev).expand(count, 1, 4)
            states = torch.cat([messages, capacity], dim=1).contiguous()
        return HashMany(self.permute_many(layouter, count, states, constants=((c.rate, cap),)))


# ---- Sponge and Hash (poseidon.rs:100-286) ----------------------------------------------------------------------------------------------
class Sponge:
    """The duplex sponge: absorbing until `finish_absorbing`, squeezing afterwards."""

    def __init__(self, chip: Pow5Chip, layouter, domain: ConstantLength):
        self.chip, self.domain = chip, domain
        self.state = chip.initial_state(layouter, domain)
        self.absorbing, self.squeezing = [], None

    def _permute(self, layouter, words) -> list:                              # poseidon_sponge (:100-118)
        if words is not None:
            self.state = self.chip.add_input(layouter, self.state, words, self.domain)
        self.state = self.chip.permute(layouter, self.state)
        return self.chip.get_output(self.state)

    def absorb(self, layouter, word) -> None:
        """word: ("message", AssignedCell) or ("padding", integer)"""
        assert self.squeezing is None
        if len(self.absorbing) < self.chip.config.rate:
            self.absorbing.append(word)
            return
        self._permute(layouter.namespace("PoseidonSponge"), self.absorbing)  # as many elements absorbed as the rate holds
        self.absorbing = [word]

    def finish_absorbing(self, layouter) -> "Sponge":
        self.squeezing = self._permute(layouter.namespace("PoseidonSponge"), self.absorbing)
        self.absorbing = None
        return self

    def squeeze(self, layouter) -> AssignedCell:
        assert self.squeezing is not None
        if not self.squeezing:
            self.squeezing = self._permute(layouter.namespace("PoseidonSponge"), None)
        return self.squeezing.pop(0)


class Hash:
    def __init__(self, sponge: Sponge):
        self.sponge = sponge

    @staticmethod
    def init(chip: Pow5Chip, layouter, domain: ConstantLength) -> "Hash":
        return Hash(Sponge(chip, layouter, domain))

    def hash(self, layouter, message) -> AssignedCell:
        """message: domain.length AssignedCells -> the AssignedCell of the digest."""
        domain = self.sponge.domain
        if len(message) != domain.length:
            raise ValueError(f"a message of {domain.length} cells")
        words = [("message", w) for w in message] + [("padding", p) for p in domain.padding(self.sponge.chip.config.rate)]
        for i, word in enumerate(words):
            self.sponge.absorb(layouter.namespace(f"absorb_{i}"), word)
        return self.sponge.finish_absorbing(layouter.namespace("finish absorbing")).squeeze(layouter.namespace("squeeze"))
