"""The Sinsemilla gadget of halo2_gadgets (src/sinsemilla.rs, sinsemilla/chip.rs, chip/hash_to_point.rs, chip/generator_table.rs,
sinsemilla/merkle.rs, merkle/chip.rs) against `halo2_amd.circuit`: `SinsemillaChip`, `Message` / `MessagePiece`, `HashDomain`,
`MerkleChip`, `MerklePath`, `MerklePaths` and `CommitDomain`, over the Pallas base field, with Q public or -- on a chip configured with
`allow_init_from_private_point` -- a witnessed point (`hash_to_point_with_private_init`).

The mirror assigns cell by cell with host `Assigned` rationals -- the same regions, offsets, gate and lookup shapes and copy
constraints as the reference, one message word per row:

    config = SinsemillaChip.configure(meta, advices[5], witness_pieces, fixed_y_q, lookup(3), range_check)
    SinsemillaChip.load(config, layouter)
    point, zs = SinsemillaChip(config).hash_to_point(layouter, Q, [piece, ...])

What the reference does not have is the bulk path: `SinsemillaChip.hash_to_point_many` lays `count` hashes of one piece structure
back to back in ONE region whose five advice columns come from the device (`halo2_amd.sinsemilla.trace`, or `trace_from` where a
hash starts under a row of its own for y_Q), with the q_sinsemilla2 pattern tiled; cell for cell the layout of `count` calls of
`hash_to_point`.  `CommitDomain.commit_many` puts `count` commitments M_i + [r_i]R into three bulk regions: the fixed-base products
(`EccChip.mul_fixed_many`), the hashes, and the complete additions (`halo2_amd.ecc.add_trace`).

The generator table is `halo2_amd.sinsemilla`'s, built on the device once per process; `table=` injects another (1024 (x, y) pairs)."""
from __future__ import annotations

import numpy as np

from .. import ecc as ecc_primitive
from .. import fields
from .. import sinsemilla as primitive
from ..circuit import Assigned, AssignedCell, Cell, Column, ConstraintSystem, Expression, Rotation, Synthesis
from .utilities import CondSwapChip, K, LookupRangeCheckConfig, RangeConstrained, i2lebsp, load_private, value_int

FP = 0
C_MAX = primitive.C_MAX
PIECE_MAX_WORDS = 25                                                          # floor(CAPACITY / K) = floor(254 / 10)


class GeneratorTableConfig:
    def __init__(self, table_idx, table_x, table_y):
        self.table_idx, self.table_x, self.table_y = table_idx, table_x, table_y


class DoubleAndAdd:
    """ecc/chip/mul/incomplete.rs:28-56: the columns of the merged double-and-add and its two derived expressions."""

    def __init__(self, x_a, x_p, lambda_1, lambda_2):
        self.x_a, self.x_p, self.lambda_1, self.lambda_2 = x_a, x_p, lambda_1, lambda_2

    def x_r(self, cells, rotation) -> Expression:
        x_a = cells.query_advice(self.x_a, rotation)
        x_p = cells.query_advice(self.x_p, rotation)
        lambda_1 = cells.query_advice(self.lambda_1, rotation)
        return lambda_1.square() - x_a - x_p

    def Y_A(self, cells, rotation) -> Expression:                             # noqa: N802 -- the reference's name; lacks the factor 1/2
        x_a = cells.query_advice(self.x_a, rotation)
        lambda_1 = cells.query_advice(self.lambda_1, rotation)
        lambda_2 = cells.query_advice(self.lambda_2, rotation)
        return (lambda_1 + lambda_2) * (x_a - self.x_r(cells, rotation))


class SinsemillaConfig:
    def __init__(self, modulus, q_sinsemilla1, q_sinsemilla2, q_sinsemilla4, fixed_y_q, double_and_add, bits, witness_pieces,
                 generator_table, lookup_config, table, injected_table=None, allow_init_from_private_point=False):
        self.modulus, self.allow_init_from_private_point = modulus, allow_init_from_private_point
        self.q_sinsemilla1, self.q_sinsemilla2, self.q_sinsemilla4, self.fixed_y_q = q_sinsemilla1, q_sinsemilla2, q_sinsemilla4, fixed_y_q
        self.double_and_add, self.bits, self.witness_pieces = double_and_add, bits, witness_pieces
        self.generator_table, self.lookup_config = generator_table, lookup_config
        self.table, self.injected_table = table, injected_table              # 1024 (x, y) integers; what the caller passed, if anything

    def advices(self) -> list:
        d = self.double_and_add
        return [d.x_a, d.x_p, self.bits, d.lambda_1, d.lambda_2]

    def q_s3(self, cells) -> Expression:
        """q_s3 = q_s2 (q_s2 - 1)"""
        q_s2 = cells.query_fixed(self.q_sinsemilla2)
        return q_s2 * (q_s2 - Expression.constant(1))


class MessagePiece:
    """sinsemilla/message.rs: a witnessed field element carrying num_words K-bit words."""

    def __init__(self, cell_value: AssignedCell, num_words: int):
        assert 1 <= num_words <= PIECE_MAX_WORDS
        self.cell_value, self.num_words = cell_value, num_words

    def field_elem(self, modulus: int):
        return value_int(self.cell_value.value(), modulus)

    @staticmethod
    def from_field_elem(chip, layouter, field_elem, num_words: int) -> "MessagePiece":
        return chip.witness_message_piece(layouter, field_elem, num_words)

    @staticmethod
    def from_bitstring(chip, layouter, bitstring) -> "MessagePiece":
        """sinsemilla.rs MessagePiece::from_bitstring: a multiple of K bits (booleans, or None each without a witness), low bit first"""
        bits = list(bitstring)
        assert len(bits) % K == 0 and len(bits) // K <= PIECE_MAX_WORDS
        elem = None if any(b is None for b in bits) else sum(int(bool(b)) << i for i, b in enumerate(bits))
        return MessagePiece.from_field_elem(chip, layouter, elem, len(bits) // K)

    @staticmethod
    def from_subpieces(chip, layouter, subpieces) -> "MessagePiece":
        """sinsemilla.rs:256-278: the subpieces (RangeConstrained integers) concatenated, low bits first; assigned, not constrained"""
        elem, total_bits = 0, 0
        for sub in subpieces:
            assert total_bits < 64
            elem = None if elem is None or sub.inner is None else elem + (sub.inner << total_bits)
            total_bits += sub.num_bits
        assert total_bits % K == 0
        return MessagePiece.from_field_elem(chip, layouter, elem, total_bits // K)


class Message(list):
    """sinsemilla.rs Message: the pieces in order (a list of MessagePiece, which is all the chip asks for)."""

    @staticmethod
    def from_pieces(chip, pieces) -> "Message":
        return Message(pieces)

    @staticmethod
    def from_bitstring(chip, layouter, bitstring) -> "Message":
        """a multiple of K bits, at most C words, cut into pieces of floor(CAPACITY / K) = 25 words, the last one shorter"""
        bits = list(bitstring)
        assert len(bits) % K == 0 and len(bits) // K <= C_MAX
        step = PIECE_MAX_WORDS * K
        return Message(MessagePiece.from_bitstring(chip, layouter, bits[at:at + step]) for at in range(0, len(bits), step))


class IllegalHashFromPrivatePoint(ValueError):
    """Error::IllegalHashFromPrivatePoint: the chip was configured without allow_init_from_private_point"""


class NonIdentityEccPoint:
    def __init__(self, x: AssignedCell, y: AssignedCell):
        self._x, self._y = x, y

    def x(self) -> AssignedCell:
        return self._x

    def y(self) -> AssignedCell:
        return self._y


class HashMany:
    """What `hash_to_point_many` returns: the cells of hash i by position.  outputs: (count, 2, 4) Montgomery x and y of the hashes
    (None without a witness)."""

    def __init__(self, region_index, config, count, num_words, outputs, first=0):
        self.region_index, self.config, self.count, self.num_words, self.outputs = region_index, config, count, list(num_words), outputs
        self.first = first                                                    # 1 where every hash starts under a row for y_Q
        self.rows = sum(num_words) + 1 + first
        self.piece_offsets = [first + sum(num_words[:k]) for k in range(len(num_words))]

    def x_a(self, i: int) -> Cell:
        return Cell(self.region_index, self.rows * i + self.rows - 1, self.config.double_and_add.x_a)

    def y_a(self, i: int) -> Cell:
        return Cell(self.region_index, self.rows * i + self.rows - 1, self.config.double_and_add.lambda_1)

    def z(self, i: int, piece: int, j: int) -> Cell:
        """the running sum z_j of that piece of hash i (z_0 is the copy of the piece)"""
        if not 0 <= j < self.num_words[piece]:
            raise IndexError(j)
        return Cell(self.region_index, self.rows * i + self.piece_offsets[piece] + j, self.config.bits)


class SinsemillaChip:
    def __init__(self, config: SinsemillaConfig):
        self.config = config

    @staticmethod
    def load(config: SinsemillaConfig, layouter) -> None:
        config.lookup_config.load(config.generator_table, layouter, config.table)

    @staticmethod
    def configure(meta: ConstraintSystem, advices, witness_pieces: Column, fixed_y_q: Column, lookup, range_check: LookupRangeCheckConfig,
                  table=None, allow_init_from_private_point: bool = False) -> SinsemillaConfig:
        """chip.rs:170-288.  All five advice columns become equality-enabled.  With allow_init_from_private_point the gate "Initial y_Q"
        reads y_Q from x_p one row above instead of from fixed_y_q: the chip can hash from a witnessed point, and a hash from a public
        Q takes one row more."""
        advices = list(advices)
        assert len(advices) == 5
        for advice in advices:
            meta.enable_equality(advice)
        injected = table
        table = primitive.generator_table_ints(table)
        config = SinsemillaConfig(
            meta.modulus, q_sinsemilla1=meta.complex_selector(), q_sinsemilla2=meta.fixed_column(), q_sinsemilla4=meta.selector(),
            fixed_y_q=fixed_y_q, double_and_add=DoubleAndAdd(advices[0], advices[1], advices[3], advices[4]), bits=advices[2],
            witness_pieces=witness_pieces, generator_table=GeneratorTableConfig(*lookup), lookup_config=range_check, table=table,
            injected_table=injected, allow_init_from_private_point=allow_init_from_private_point)
        dna = config.double_and_add

        def generator_lookup(cells):                                          # generator_table.rs:46-82
            q_s1 = cells.query_selector(config.q_sinsemilla1)
            q_s2 = cells.query_fixed(config.q_sinsemilla2)
            q_s3 = config.q_s3(cells)
            q_run = q_s2 - q_s3
            z_cur = cells.query_advice(config.bits, Rotation.cur())
            z_next = cells.query_advice(config.bits, Rotation.next())
            word = z_cur - (q_run * z_next * (1 << K))                        # m_{i+1} = z_i - 2^K q_run z_{i+1}
            x_p = cells.query_advice(dna.x_p, Rotation.cur())
            lambda1 = cells.query_advice(dna.lambda_1, Rotation.cur())
            x_a = cells.query_advice(dna.x_a, Rotation.cur())
            y_a = dna.Y_A(cells, Rotation.cur())
            y_p = (y_a * pow(2, -1, meta.modulus)) - (lambda1 * (x_a - x_p))  # y_p = Y_A / 2 - lambda_1 (x_a - x_p)
            init_x, init_y = table[0]                                         # the lookup defaults to the first entry without q_s1
            not_q_s1 = Expression.constant(1) - q_s1
            m = q_s1 * word
            x_p = q_s1 * x_p + not_q_s1 * init_x
            y_p = q_s1 * y_p + not_q_s1 * init_y
            return [(m, config.generator_table.table_idx), (x_p, config.generator_table.table_x), (y_p, config.generator_table.table_y)]
        meta.lookup(generator_lookup)

        def initial_y_q(cells):
            q_s4 = cells.query_selector(config.q_sinsemilla4)
            y_q = cells.query_advice(dna.x_p, Rotation.prev()) if allow_init_from_private_point else cells.query_fixed(config.fixed_y_q)
            y_a_cur = dna.Y_A(cells, Rotation.cur())
            return [("init_y_q_check", q_s4 * (y_q * 2 - y_a_cur))]           # 2 y_Q - Y_{A,0} = 0
        meta.create_gate("Initial y_Q", initial_y_q)

        def sinsemilla_gate(cells):
            q_s1 = cells.query_selector(config.q_sinsemilla1)
            q_s3 = config.q_s3(cells)
            lambda_1_next = cells.query_advice(dna.lambda_1, Rotation.next())
            lambda_2_cur = cells.query_advice(dna.lambda_2, Rotation.cur())
            x_a_cur = cells.query_advice(dna.x_a, Rotation.cur())
            x_a_next = cells.query_advice(dna.x_a, Rotation.next())
            x_r = dna.x_r(cells, Rotation.cur())
            y_a_cur = dna.Y_A(cells, Rotation.cur())
            y_a_next = dna.Y_A(cells, Rotation.next())
            secant_line = lambda_2_cur.square() - (x_a_next + x_r + x_a_cur)
            lhs = lambda_2_cur * 4 * (x_a_cur - x_a_next)
            y_a_final = lambda_1_next                                         # on the last row lambda_1 holds y_a
            rhs = y_a_cur * 2 + (Expression.constant(2) - q_s3) * y_a_next + q_s3 * 2 * y_a_final
            return [("Secant line", q_s1 * secant_line), ("y check", q_s1 * (lhs - rhs))]
        meta.create_gate("Sinsemilla gate", sinsemilla_gate)
        return config

    # ---- SinsemillaInstructions (chip.rs:315-372) ---------------------------------------------------------------------------------------------
    def witness_message_piece(self, layouter, field_elem, num_words: int) -> MessagePiece:
        cell = layouter.assign_region("witness message piece",
                                      lambda region: region.assign_advice(self.config.witness_pieces, 0, lambda: field_elem))
        return MessagePiece(cell, num_words)

    def hash_to_point(self, layouter, Q, message):                            # noqa: N803
        """message: a list of MessagePiece.  -> (NonIdentityEccPoint, the running sums of every piece)"""
        assert sum(p.num_words for p in message) <= C_MAX
        return layouter.assign_region("hash_to_point", lambda region: self._hash_message(region, Q, message))

    def hash_to_point_with_private_init(self, layouter, Q: NonIdentityEccPoint, message):      # noqa: N803
        """the hash from a witnessed Q, whose two cells are copied in (chip.rs, hash_to_point.rs:68-105)"""
        assert sum(p.num_words for p in message) <= C_MAX
        if not self.config.allow_init_from_private_point:
            raise IllegalHashFromPrivatePoint("hash_to_point_with_private_init: the chip was configured without allow_init_from_private_point")
        return layouter.assign_region("hash_to_point", lambda region: self._hash_message(region, Q, message, private=True))

    @staticmethod
    def extract(point: NonIdentityEccPoint) -> AssignedCell:
        return point.x()

    # ---- hash_to_point.rs ------------------------------------------------------------------------------------------------------------------
    def _public_q_initialization(self, region, Q):                            # noqa: N803 -- hash_to_point.rs:107-166
        c, m = self.config, self.config.modulus
        x_q, y_q = int(Q[0]) % m, int(Q[1]) % m
        offset = 0
        if c.allow_init_from_private_point:                                   # y_Q in x_p on a row of its own, q_sinsemilla4 on the second
            c.q_sinsemilla4.enable(region, 1)
            region.assign_advice_from_constant(c.double_and_add.x_p, 0, y_q)
            offset = 1
        else:                                                                 # q_sinsemilla4 and y_Q (fixed) on the first row
            c.q_sinsemilla4.enable(region, 0)
            region.assign_fixed(c.fixed_y_q, 0, lambda: y_q)
        x_a = region.assign_advice_from_constant(c.double_and_add.x_a, offset, x_q)
        y_a = Assigned.trivial(y_q, m) if region.layouter and region.layouter.cs.collect_advice else None
        return offset, x_a, y_a

    def _private_q_initialization(self, region, Q: NonIdentityEccPoint):      # noqa: N803 -- hash_to_point.rs:168-213
        c = self.config
        if not c.allow_init_from_private_point:
            raise IllegalHashFromPrivatePoint("the chip was configured without allow_init_from_private_point")
        c.q_sinsemilla4.enable(region, 1)
        y_cell = Q.y().copy_advice(region, c.double_and_add.x_p, 0)
        x_a = Q.x().copy_advice(region, c.double_and_add.x_a, 1)
        return 1, x_a, y_cell.value().inner

    def _hash_message(self, region, Q, message, private=False):               # noqa: N803
        c = self.config
        offset, x_a, y_a = self._private_q_initialization(region, Q) if private else self._public_q_initialization(region, Q)
        zs_sum = []
        for idx, piece in enumerate(message):
            x_a, y_a, zs = self._hash_piece(region, offset, piece, x_a, y_a, idx == len(message) - 1)
            offset += piece.num_words
            zs_sum.append(zs)
        y_a_cell = region.assign_advice(c.double_and_add.lambda_1, offset, lambda: y_a)
        region.assign_advice(c.double_and_add.lambda_2, offset, lambda: 0)    # queried by the gate, multiplied by zero
        region.assign_advice(c.double_and_add.x_p, offset, lambda: 0)
        if y_a is not None:
            x_val = x_a.value().inner
            if x_val.is_zero_vartime() or y_a.is_zero_vartime():
                raise Synthesis("Sinsemilla: the hash has no value (an exceptional addition)")
        return NonIdentityEccPoint(x_a, y_a_cell), zs_sum

    def _hash_piece(self, region, offset, piece: MessagePiece, x_a: AssignedCell, y_a, final_piece: bool):
        c, m = self.config, self.config.modulus
        dna = c.double_and_add
        n = piece.num_words
        for row in range(n):
            c.q_sinsemilla1.enable(region, offset + row)
        for row in range(n - 1):
            region.assign_fixed(c.q_sinsemilla2, offset + row, lambda: 1)
        region.assign_fixed(c.q_sinsemilla2, offset + n - 1, lambda: 2 if final_piece else 0)

        elem = piece.field_elem(m)
        words = [None] * n if elem is None else [(elem >> (K * j)) & ((1 << K) - 1) for j in range(n)]
        # the running sum: z_0 is a copy of the piece, z_{i+1} = (z_i - m_{i+1}) / 2^K; z_n = 0 is not assigned
        zs = [piece.cell_value.copy_advice(region, c.bits, offset)]
        z, inv_2_k = elem, pow(1 << K, -1, m)
        for idx in range(n - 1):
            z = None if z is None else (z - words[idx]) * inv_2_k % m
            zs.append(region.assign_advice(c.bits, offset + idx + 1, lambda v=z: v))

        for row, word in enumerate(words):
            if word is None or y_a is None:
                for column in (dna.x_p, dna.lambda_1, dna.lambda_2):
                    region.assign_advice(column, offset + row, lambda: None)
                x_a = region.assign_advice(dna.x_a, offset + row + 1, lambda: None)
                continue
            x_p, y_p = c.table[word]
            x_a_val = x_a.value().inner
            region.assign_advice(dna.x_p, offset + row, lambda: x_p)
            lambda_1 = (y_a - y_p) * (x_a_val - x_p).invert()
            region.assign_advice(dna.lambda_1, offset + row, lambda: lambda_1)
            x_r = lambda_1.square() - x_a_val - x_p
            lambda_2 = y_a * 2 * (x_a_val - x_r).invert() - lambda_1
            region.assign_advice(dna.lambda_2, offset + row, lambda: lambda_2)
            x_a_new = lambda_2.square() - x_a_val - x_r
            x_a = region.assign_advice(dna.x_a, offset + row + 1, lambda: x_a_new)
            y_a = lambda_2 * (x_a_val - x_a_new) - y_a
        return x_a, y_a, zs

    # ---- the bulk path ---------------------------------------------------------------------------------------------------------------------
    def witness_message_pieces_many(self, layouter, num_words, values=None, column=None) -> list:
        """`witness_message_piece` of len(num_words) pieces back to back in one region of the witness_pieces column; piece i carries
        num_words[i] words.  values: the pieces as integers (None each, or None for all, without a witness); column: the
        (len(num_words), 4) Montgomery vector where the caller has it on the device (then `values` is not read).  Without a witness
        (keygen) the same shape is laid out.  -> the MessagePieces; one built from `column` carries its cell and no value."""
        import torch
        num_words = [int(w) for w in num_words]
        count = len(num_words)
        if not layouter.cs.collect_advice or not count:
            column, known = np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (count, 4)), [None] * count
        elif column is None:
            if values is None or any(v is None for v in values) or len(values) != count:
                raise Synthesis("witness_message_pieces_many: a witness is needed and there is none")
            known = [Assigned.trivial(int(v) % self.config.modulus, self.config.modulus) for v in values]
            column = fields.to_limbs([int(v) % self.config.modulus for v in values], FP)
        else:
            known = [None] * count
            if not torch.is_tensor(column):
                column = torch.from_numpy(np.ascontiguousarray(column, dtype=np.uint64).view(np.int64))
            if tuple(column.shape) != (count, 4):
                raise ValueError("witness_message_pieces_many: the column is (len(num_words), 4)")
        index = layouter.assign_region("witness message pieces many",
                                       lambda region: region.assign_advice_column(self.config.witness_pieces, 0, column).region_index)
        return [MessagePiece(AssignedCell(known[i], Cell(index, i, self.config.witness_pieces)), w) for i, w in enumerate(num_words)]

    def hash_to_point_many(self, layouter, Q, num_words, pieces, values=None, trace=None) -> HashMany:      # noqa: N803
        """`count` hashes of one piece structure back to back in one region; cell for cell what `count` calls of `hash_to_point` (or of
        `hash_to_point_with_private_init`) lay out.  Q: an (x, y) pair, public and shared, or a list of `count` NonIdentityEccPoint,
        one witnessed Q per hash, on a chip configured with allow_init_from_private_point.  Each hash takes sum(num_words) + 1 rows,
        and one more in front, for y_Q, on such a chip.

        pieces: pieces[i][k] is the MessagePiece k of hash i (their cells are copied into z_0).  values: the (count, n_pieces, 4)
        CANONICAL limbs of the pieces where the caller has them on the device already (else they are read from the cells); trace:
        the (5, rows * count, 4) columns where the caller has them (else `sinsemilla.trace` or `trace_from`, once).  Without a witness
        (keygen) the same shape is laid out and nothing is launched."""
        import torch
        c, m = self.config, self.config.modulus
        num_words = [int(w) for w in num_words]
        private = not (len(Q) == 2 and not any(hasattr(q, "x") for q in Q))     # cells, not the two coordinates of a public point
        if private and not c.allow_init_from_private_point:
            raise IllegalHashFromPrivatePoint("hash_to_point_many: the chip was configured without allow_init_from_private_point")
        first = 1 if c.allow_init_from_private_point else 0
        count, n_pieces, rows = len(pieces), len(num_words), sum(num_words) + 1 + first
        if any(len(p) != n_pieces or any(q.num_words != w for q, w in zip(p, num_words)) for p in pieces):
            raise ValueError("hash_to_point_many: every hash has the pieces of the one structure")
        if private and len(Q) != count:
            raise ValueError("hash_to_point_many: one Q per hash")
        backend = layouter.cs
        total = rows * count
        if not backend.collect_advice:
            trace = None
        elif trace is None and count:
            if values is None:
                ints = [q.field_elem(m) for p in pieces for q in p]
                if any(v is None for v in ints):
                    raise Synthesis("hash_to_point_many: a witness is needed and there is none")
                values = fields.to_limbs(ints, FP, montgomery=False).reshape(count, n_pieces, 4)
            if not torch.is_tensor(values):
                values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)).to(fields.current_device())
            if private:
                coords = [value_int(cell.value(), m) for q in Q for cell in (q.x(), q.y())]
                if any(v is None for v in coords):
                    raise Synthesis("hash_to_point_many: a witness is needed and there is none")
                start = torch.from_numpy(fields.to_limbs(coords, FP).reshape(count, 8).view(np.int64)).to(values.device)
                trace = primitive.trace_from(values, num_words, start, table=c.injected_table)
            elif first:
                trace = primitive.trace_from(values, num_words, (int(Q[0]) % m, int(Q[1]) % m), table=c.injected_table)
            else:
                trace = primitive.trace(values, num_words, Q, table=c.injected_table)
        if trace is not None:
            if not torch.is_tensor(trace):
                trace = torch.from_numpy(np.ascontiguousarray(trace, dtype=np.uint64).view(np.int64))
            if tuple(trace.shape) != (5, total, 4):
                raise ValueError("hash_to_point_many: the trace is (5, rows * count, 4)")
        blank = np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (total, 4))
        advice = [blank] * 5 if trace is None else [trace[j] for j in range(5)]
        # q_sinsemilla2 of one hash: 1 on the rows of a piece but its last, 0 there, 2 on the last word row; nothing on the row of y_Q
        # nor on the final row (a fixed cell nobody assigns is zero, so the tiled pattern carries a zero there)
        pattern = [0] * first
        for k, w in enumerate(num_words):
            pattern += [1] * (w - 1) + [2 if k == n_pieces - 1 else 0]
        q_s2 = blank
        if backend.collect_fixed and count:
            q_s2 = np.tile(fields.to_limbs(pattern + [0], FP), (count, 1))
        base = rows * np.arange(count, dtype=np.int64)
        word_rows = (base[:, None] + np.arange(first, rows - 1, dtype=np.int64)[None, :]).reshape(-1)
        dna = c.double_and_add
        result = HashMany(None, c, count, num_words, None, first)

        def assign(region):
            index = region.region_index
            for column, values_ in zip((dna.x_a, dna.x_p, c.bits, dna.lambda_1, dna.lambda_2), advice):
                region.assign_advice_column(column, 0, values_)
            region.enable_selector_rows(c.q_sinsemilla1, word_rows)
            region.enable_selector_rows(c.q_sinsemilla4, base + first)
            region.assign_fixed_column(c.q_sinsemilla2, 0, q_s2)
            for i in range(count):
                at = rows * i
                if private:
                    region.constrain_equal(Cell(index, at, dna.x_p), Q[i].y().cell())
                    region.constrain_equal(Cell(index, at + 1, dna.x_a), Q[i].x().cell())
                else:
                    x_q, y_q = int(Q[0]) % m, int(Q[1]) % m
                    if first:
                        region.constrain_constant(Cell(index, at, dna.x_p), y_q)
                    else:
                        region.assign_fixed(c.fixed_y_q, at, lambda: y_q)
                    region.constrain_constant(Cell(index, at + first, dna.x_a), x_q)
                at += first
                for k, w in enumerate(num_words):
                    region.constrain_equal(Cell(index, at, c.bits), pieces[i][k].cell_value.cell())
                    at += w
            return index
        result.region_index = layouter.assign_region("hash_to_point many", assign)
        if trace is not None and count:
            last = torch.from_numpy(base + rows - 1).to(trace.device)
            result.outputs = torch.stack([trace[0][last], trace[3][last]], dim=1)
        return result


class HashDomain:
    """sinsemilla.rs HashDomain over a SinsemillaChip (or a MerkleChip) and a public Q."""

    def __init__(self, chip, Q):                                              # noqa: N803
        self.chip, self.Q = chip, (int(Q[0]), int(Q[1]))

    def hash_to_point(self, layouter, message):
        return self.chip.hash_to_point(layouter, self.Q, message)

    def hash_to_point_with_private_init(self, layouter, Q: NonIdentityEccPoint, message):      # noqa: N803 -- sinsemilla.rs:344-360
        return self.chip.hash_to_point_with_private_init(layouter, Q, message)

    def hash(self, layouter, message):                                        # noqa: A003
        point, zs = self.hash_to_point(layouter, message)
        return self.chip.extract(point), zs


# ---- CommitDomain (sinsemilla.rs:395-520) -----------------------------------------------------------------------------------------------------
class CommitDomains:
    """What a CommitDomain reads of its domain (sinsemilla.rs CommitDomains): the hash's public Q as (x, y) integers and R's tables, an
    `ecc.FixedBaseTables` of 85 windows."""

    def __init__(self, Q, R):                                                 # noqa: N803
        self.Q, self.R = (int(Q[0]), int(Q[1])), R

    @staticmethod
    def of(domain: "primitive.CommitDomain") -> "CommitDomains":
        """from `halo2_amd.sinsemilla.CommitDomain`, whose tables of R are built on the device"""
        from .ecc import FixedBaseTables
        return CommitDomains(domain.M.Q, FixedBaseTables.of(domain.fixed_base))


class CommitMany:
    """What `commit_many` returns: the cells of commitment i by position, the bulk hashes (`hashes.z(i, piece, j)` are the running sums)
    and the bulk blinding products.  outputs: (count, 2, 4) Montgomery x and y of the commitments (None without a witness)."""

    def __init__(self, add_config, blinds, hashes):
        self.add_config, self.blinds, self.hashes, self.add_region_index, self.outputs = add_config, blinds, hashes, None, None

    def result_x(self, i: int) -> Cell:
        return Cell(self.add_region_index, 2 * i + 1, self.add_config.x_qr)

    def result_y(self, i: int) -> Cell:
        return Cell(self.add_region_index, 2 * i + 1, self.add_config.y_qr)


class CommitDomain:
    """SinsemillaCommit and SinsemillaShortCommit over a SinsemillaChip and an EccChip: M + [r]R, the regions in the reference's
    order -- "[r] R", then "M", then "M + [r] R"."""

    def __init__(self, sinsemilla_chip, ecc_chip, domain: CommitDomains):
        from .ecc import FixedPoint
        self.M = HashDomain(sinsemilla_chip, domain.Q)
        self.R = FixedPoint.from_inner(ecc_chip, domain.R)
        self.ecc_chip, self._tables = ecc_chip, domain.R

    def _point(self, inner):
        from .ecc import NonIdentityPoint
        return NonIdentityPoint(self.ecc_chip, inner)

    def hash_with_private_init(self, layouter, Q, message):                   # noqa: N803
        """Q: an ecc NonIdentityPoint (or the chip's NonIdentityEccPoint).  -> (NonIdentityPoint, running sums)"""
        point, zs = self.M.hash_to_point_with_private_init(layouter, Q.inner() if hasattr(Q, "inner") else Q, message)
        return self._point(point), zs

    def q_init(self) -> tuple:
        return self.M.Q

    def blinding_factor(self, layouter, r):
        """[r]R for a ScalarFixed r -> Point"""
        blind, _ = self.R.mul(layouter, r)
        return blind

    def commit(self, layouter, message, r):
        """-> (Point, running sums)"""
        blind, _ = self.R.mul(layouter, r)
        p, zs = self.M.hash_to_point(layouter, message)
        return self._point(p).add(layouter, blind), zs

    def short_commit(self, layouter, message, r):
        """-> (the x cell, running sums)"""
        p, zs = self.commit(layouter, message, r)
        return p.extract_p(), zs

    def commit_many(self, layouter, pieces, num_words, scalars, values=None, trace=None) -> CommitMany:
        """`count` commitments M_i + [r_i]R in three bulk regions, in the order of `commit`: one `mul_fixed_many` (with its region of
        closing additions), one `hash_to_point_many`, and one region of `count` complete additions, two rows each as the bulk
        additions of `mul_fixed_many`, filled from `ecc.add_trace` and copy-constrained to the outputs of the other two.

        pieces, num_words: as `hash_to_point_many`; scalars: integers below 2^255 (None each without a witness).  values: (the pieces'
        limbs, the scalars' limbs) as the two bulk calls take them, either may be None; trace: (the `mul_fixed_trace` pair, the hash's
        columns, the additions' (count, 11, 4) rows), each None where the caller has none."""
        import torch
        piece_values, scalar_values = values if values is not None else (None, None)
        fixed_trace, hash_trace, add_trace = trace if trace is not None else (None, None, None)
        count = len(pieces)
        if len(scalars) != count:
            raise ValueError("commit_many: one scalar per message")
        blinds = self.ecc_chip.mul_fixed_many(layouter, self._tables, scalars, values=scalar_values, trace=fixed_trace)
        hashes = self.M.chip.hash_to_point_many(layouter, self.M.Q, num_words, pieces, values=piece_values, trace=hash_trace)
        add = self.ecc_chip.config.add
        result = CommitMany(add, blinds, hashes)
        aux = None
        if layouter.cs.collect_advice and count:
            if add_trace is None:
                add_trace = ecc_primitive.add_trace(hashes.outputs.reshape(count, 8), blinds.outputs.reshape(count, 8))
            aux = add_trace if torch.is_tensor(add_trace) else torch.from_numpy(np.ascontiguousarray(add_trace, dtype=np.uint64).view(np.int64))
            if tuple(aux.shape) != (count, ecc_primitive.FIXED_AUX, 4):
                raise ValueError("commit_many: the additions' trace is (count, 11, 4)")

        # p = M_i, q = [r_i]R, in the layout of EccChip.add_many
        result.add_region_index = self.ecc_chip.additions_many(
            layouter, "M + [r] R many", count, aux, lambda i: (hashes.x_a(i), hashes.y_a(i), blinds.result_x(i), blinds.result_y(i)))
        if aux is not None:
            result.outputs = aux[:, 9:11].contiguous()
        return result


# ---- MerkleChip, MerklePath (merkle/chip.rs, merkle.rs) ------------------------------------------------------------------------------------
class MerkleConfig:
    def __init__(self, advices, q_decompose, cond_swap_config, sinsemilla_config):
        self.advices, self.q_decompose = advices, q_decompose
        self.cond_swap_config, self.sinsemilla_config = cond_swap_config, sinsemilla_config


class MerkleChip:
    """hash_layer = MerkleCRH: SinsemillaHash(Q, l (10 bits) || left (255 bits) || right (255 bits)); left and right are not
    constrained to be canonical."""

    def __init__(self, config: MerkleConfig):
        self.config = config
        self._sinsemilla = SinsemillaChip(config.sinsemilla_config)
        self._cond_swap = CondSwapChip(config.cond_swap_config)

    @staticmethod
    def configure(meta: ConstraintSystem, sinsemilla_config: SinsemillaConfig) -> MerkleConfig:
        advices = sinsemilla_config.advices()
        cond_swap_config = CondSwapChip.configure(meta, advices)
        q_decompose = meta.selector()

        # |  A_0  |  A_1  |  A_2  |  A_3  |  A_4  | q_decompose |
        # |   a   |   b   |   c   |  left | right |      1      |
        # |  z1_a |  z1_b |  b_1  |  b_2  |   l   |      0      |
        def gate(cells):
            q = cells.query_selector(q_decompose)
            l_whole = cells.query_advice(advices[4], Rotation.next())
            two_pow_5, two_pow_10 = 1 << 5, 1 << 10
            a_whole = cells.query_advice(advices[0], Rotation.cur())
            b_whole = cells.query_advice(advices[1], Rotation.cur())
            c_whole = cells.query_advice(advices[2], Rotation.cur())
            left_node = cells.query_advice(advices[3], Rotation.cur())
            right_node = cells.query_advice(advices[4], Rotation.cur())
            a_1 = cells.query_advice(advices[0], Rotation.next())             # z_1 of SinsemillaHash(a)
            a_0 = a_whole - a_1 * two_pow_10
            z1_b = cells.query_advice(advices[1], Rotation.next())
            b_1 = cells.query_advice(advices[2], Rotation.next())
            b_2 = cells.query_advice(advices[3], Rotation.next())
            b1_b2_check = z1_b - (b_1 + b_2 * two_pow_5)
            b_0 = b_whole - (z1_b * two_pow_10)
            left_check = (a_1 + (b_0 + b_1 * two_pow_10) * (1 << 240)) - left_node
            right_check = b_2 + c_whole * two_pow_5 - right_node
            return [("l_check", q * (a_0 - l_whole)), ("left_check", q * left_check), ("right_check", q * right_check),
                    ("b1_b2_check", q * b1_b2_check)]
        meta.create_gate("Decomposition check", gate)
        return MerkleConfig(advices, q_decompose, cond_swap_config, sinsemilla_config)

    # what the chip forwards to its two parts
    def witness_message_piece(self, layouter, value, num_words):
        return self._sinsemilla.witness_message_piece(layouter, value, num_words)

    def hash_to_point(self, layouter, Q, message):                            # noqa: N803
        return self._sinsemilla.hash_to_point(layouter, Q, message)

    def hash_to_point_with_private_init(self, layouter, Q, message):          # noqa: N803 -- merkle/chip.rs:568-577
        return self._sinsemilla.hash_to_point_with_private_init(layouter, Q, message)

    extract = staticmethod(SinsemillaChip.extract)

    def swap(self, layouter, pair, swap):
        return self._cond_swap.swap(layouter, pair, swap)

    def mux(self, layouter, choice, left, right):                             # merkle/chip.rs:471-481
        return self._cond_swap.mux(layouter, choice, left, right)

    def load_private(self, layouter, column, value):
        return load_private(layouter, column, value)

    def hash_layer(self, layouter, Q, l: int, left: AssignedCell, right: AssignedCell) -> AssignedCell:      # noqa: N803, E741
        """a = l || bits 0..239 of left;  b = bits 240..249 of left || bits 250..254 of left || bits 0..4 of right;
        c = bits 5..254 of right.  b_1 and b_2 are range-constrained to 5 bits, the pieces by the hash itself."""
        config = self.config
        m = config.sinsemilla_config.modulus
        lookup_config = config.sinsemilla_config.lookup_config
        left_v, right_v = value_int(left.value(), m), value_int(right.value(), m)
        a = MessagePiece.from_subpieces(self, layouter, [RangeConstrained.bitrange_of(l, 0, 10), RangeConstrained.bitrange_of(left_v, 0, 240)])
        b_0 = RangeConstrained.bitrange_of(left_v, 240, 250)
        b_1 = RangeConstrained.witness_short(lookup_config, layouter, left_v, 250, 255)
        b_2 = RangeConstrained.witness_short(lookup_config, layouter, right_v, 0, 5)
        b = MessagePiece.from_subpieces(self, layouter, [b_0, b_1.value(m), b_2.value(m)])
        c = MessagePiece.from_subpieces(self, layouter, [RangeConstrained.bitrange_of(right_v, 5, 255)])
        point, zs = self.hash_to_point(layouter, Q, [a, b, c])
        digest = self.extract(point)
        z1_a, z1_b = zs[0][1], zs[1][1]

        def assign(region):
            config.q_decompose.enable(region, 0)
            region.assign_advice_from_constant(config.advices[4], 1, l)
            a.cell_value.copy_advice(region, config.advices[0], 0)
            b.cell_value.copy_advice(region, config.advices[1], 0)
            c.cell_value.copy_advice(region, config.advices[2], 0)
            left.copy_advice(region, config.advices[3], 0)
            right.copy_advice(region, config.advices[4], 0)
            z1_a.copy_advice(region, config.advices[0], 1)
            z1_b.copy_advice(region, config.advices[1], 1)
            b_1.inner.copy_advice(region, config.advices[2], 1)
            b_2.inner.copy_advice(region, config.advices[3], 1)
        layouter.assign_region("Check piece decomposition", assign)
        return digest


    # ---- the bulk path ---------------------------------------------------------------------------------------------------------------------
    def swap_many(self, layouter, a_cells, b_values, swaps, trace=None):
        return self._cond_swap.swap_many(layouter, a_cells, b_values, swaps, trace=trace)

    def witness_message_pieces_many(self, layouter, num_words, values=None, column=None):
        return self._sinsemilla.witness_message_pieces_many(layouter, num_words, values=values, column=column)

    def hash_to_point_many(self, layouter, Q, num_words, pieces, values=None, trace=None):      # noqa: N803
        return self._sinsemilla.hash_to_point_many(layouter, Q, num_words, pieces, values=values, trace=trace)

    def hash_layer_many(self, layouter, Q, layers, lefts, rights, trace=None, hash_trace=None, copy_digests_to=None) -> HashMany:      # noqa: N803
        """`hash_layer` of count = len(layers) items in five bulk regions: the 3 * count pieces, the two 5-bit range checks of b_1 and
        b_2 (`short_range_check_many` on the chip's lookup config), the hashes (`hash_to_point_many`), and "Check piece decomposition
        many": 2 * count rows over the five advice columns, q_decompose on every even row; per item the gates and equality
        constraints of the single call.  layers[t]: the constant l of item t; lefts[t], rights[t]: the Cells (or AssignedCells) of
        the pair.  trace: the `sinsemilla.MerklePathTrace` of exactly these items, hash_trace: their (5, 53 * count, 4) columns from
        `sinsemilla.trace(trace.canonical, MERKLE_PIECE_WORDS, Q)` (computed here when absent); both None without a witness
        (keygen): the same shape, nothing launched.  copy_digests_to[t]: a cell the digest of item t is copied into, or None -- a
        swap row laid out before this hash.  -> the HashMany; `.x_a(t)` is the digest cell of item t."""
        config, sin = self.config, self.config.sinsemilla_config
        m, count = sin.modulus, len(layers)
        structure = list(primitive.MERKLE_PIECE_WORDS)
        if len(lefts) != count or len(rights) != count or (copy_digests_to is not None and len(copy_digests_to) != count):
            raise ValueError("hash_layer_many: one left, one right and one digest target per layer")
        witness = bool(layouter.cs.collect_advice and count)
        if witness and (trace is None or trace.count != count):
            raise Synthesis("hash_layer_many: a witness is needed: the MerklePathTrace of these items")
        if not witness:
            trace = hash_trace = None
        elif hash_trace is None:
            hash_trace = primitive.trace(trace.canonical, structure, Q, table=sin.injected_table)
        flat = self.witness_message_pieces_many(layouter, structure * count, column=None if trace is None else trace.pieces,
                                                values=None)
        pieces = [flat[3 * t:3 * t + 3] for t in range(count)]
        unknown = [None] * count
        b_1 = sin.lookup_config.short_range_check_many(layouter, unknown, 5, values=None if trace is None else trace.b_1)
        b_2 = sin.lookup_config.short_range_check_many(layouter, unknown, 5, values=None if trace is None else trace.b_2)
        hashes = self.hash_to_point_many(layouter, Q, structure, pieces, values=None if trace is None else trace.canonical, trace=hash_trace)
        blank = np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (2 * count, 4))
        cell_of = lambda c: c.cell() if isinstance(c, AssignedCell) else c

        def assign(region):
            index = region.region_index
            for j, column in enumerate(config.advices):
                region.assign_advice_column(column, 0, blank if trace is None else trace.decompose[j])
            region.enable_selector_rows(config.q_decompose, 2 * np.arange(count, dtype=np.int64))
            for t in range(count):
                row = 2 * t
                region.constrain_constant(Cell(index, row + 1, config.advices[4]), int(layers[t]) % m)
                for j in range(3):
                    region.constrain_equal(Cell(index, row, config.advices[j]), pieces[t][j].cell_value.cell())
                region.constrain_equal(Cell(index, row, config.advices[3]), cell_of(lefts[t]))
                region.constrain_equal(Cell(index, row, config.advices[4]), cell_of(rights[t]))
                region.constrain_equal(Cell(index, row + 1, config.advices[0]), hashes.z(t, 0, 1))
                region.constrain_equal(Cell(index, row + 1, config.advices[1]), hashes.z(t, 1, 1))
                region.constrain_equal(Cell(index, row + 1, config.advices[2]), b_1[t])
                region.constrain_equal(Cell(index, row + 1, config.advices[3]), b_2[t])
                if copy_digests_to is not None and copy_digests_to[t] is not None:
                    region.constrain_equal(cell_of(copy_digests_to[t]), hashes.x_a(t))
        layouter.assign_region("Check piece decomposition many", assign)
        return hashes


class MerklePath:
    """merkle.rs:46-171: the path from a leaf to the root, its layers shared out over the chips (ceil(len / chips) layers each)."""

    def __init__(self, chips, Q, leaf_pos, path, path_length: int | None = None):      # noqa: N803
        assert chips
        self.chips, self.Q, self.leaf_pos = list(chips), Q, leaf_pos
        self.path = None if path is None else list(path)
        self.path_length = len(self.path) if path_length is None else path_length

    def calculate_root(self, layouter, leaf: AssignedCell) -> AssignedCell:
        n = self.path_length
        layers_per_chip = (n + len(self.chips) - 1) // len(self.chips)
        pos = [None] * n if self.leaf_pos is None else i2lebsp(self.leaf_pos, n)
        path = [None] * n if self.path is None else self.path
        node = leaf
        for l in range(n):                                                    # noqa: E741 -- l counts from the leaf
            chip = self.chips[l // layers_per_chip]
            pair = chip.swap(layouter, (node, path[l]), pos[l])
            node = chip.hash_layer(layouter, self.Q, l, pair[0], pair[1])
        return node


class MerklePaths:
    """`MerklePath` for n paths of one length at once: the walk comes from the device in one launch (`sinsemilla.merkle_paths`), and
    every chip lays its layers of ALL paths out in bulk regions -- "swap many", then `hash_layer_many`'s "witness message pieces many",
    two "Range check 5 bits many", "hash_to_point many" and "Check piece decomposition many" -- filled from one
    `sinsemilla.merkle_path_trace` and one `sinsemilla.trace`.  The layers are shared out over the chips as `MerklePath` does (ceil(len / chips) consecutive layers
    each); per (path, layer) the gates, lookups and equality constraints are those of `MerklePath.calculate_root`.

    leaf_positions: n integers below 2^32; paths: n lists of path_length siblings, from the leaf up; None each for keygen."""

    def __init__(self, chips, Q, leaf_positions, paths, path_length: int | None = None):      # noqa: N803
        assert chips
        self.chips, self.Q = list(chips), (int(Q[0]), int(Q[1]))
        self.leaf_positions = None if leaf_positions is None else [int(p) for p in leaf_positions]
        self.paths = None if paths is None else [list(p) for p in paths]
        if path_length is None:
            if not self.paths:
                raise ValueError("MerklePaths: a path length, or paths to read it from")
            path_length = len(self.paths[0])
        self.path_length = int(path_length)
        if not 1 <= self.path_length <= primitive.MAX_MERKLE_DEPTH:
            raise ValueError("MerklePaths: 1 .. 32 layers")
        if self.paths is not None and any(len(p) != self.path_length for p in self.paths):
            raise ValueError("MerklePaths: every path has path_length siblings")

    def calculate_roots(self, layouter, leaves) -> list:
        """leaves: n AssignedCells.  -> the n root cells (with their values where there is a witness)"""
        import torch
        n, depth = len(leaves), self.path_length
        per_chip = (depth + len(self.chips) - 1) // len(self.chips)
        sin = self.chips[0].config.sinsemilla_config
        m = sin.modulus
        witness = bool(layouter.cs.collect_advice and n)
        nodes = pos = sib = None
        if witness:
            leaf_ints = [value_int(leaf.value(), m) for leaf in leaves]
            if self.leaf_positions is None or self.paths is None or any(v is None for v in leaf_ints):
                raise Synthesis("MerklePaths: a witness is needed and there is none")
            if len(self.leaf_positions) != n or len(self.paths) != n:
                raise ValueError("MerklePaths: one position and one path per leaf")
            dev = fields.current_device()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)
            sib = up(fields.to_limbs([int(s) % m for p in self.paths for s in p], FP)).reshape(n, depth, 4)
            pos = torch.from_numpy(np.array(self.leaf_positions, dtype=np.uint32).view(np.int32)).to(dev)
            nodes = primitive.merkle_paths(up(fields.to_limbs(leaf_ints, FP)), pos, sib, domain=primitive.HashDomain(self.Q, table=sin.injected_table))
        previous, previous_layers = None, 0
        for at, chip in enumerate(self.chips):
            lo, hi = at * per_chip, min(depth, (at + 1) * per_chip)
            if lo >= hi:
                break
            layers = hi - lo
            count = n * layers
            trace = primitive.merkle_path_trace(nodes, pos, sib, lo, hi) if witness else None
            # the `a` of a chip's first layer is copied from the leaf or from the digest the chip before laid out; the `a` of its other
            # layers from a digest of its own hash region, which comes after the swaps: hash_layer_many ties those
            firsts = [leaves[p] if previous is None else previous.x_a(p * previous_layers + previous_layers - 1) for p in range(n)]
            a_cells = [firsts[t // layers] if t % layers == 0 else None for t in range(count)]
            swaps = chip.swap_many(layouter, a_cells, [None] * count, [None] * count, trace=None if trace is None else trace.swap_rows)
            targets = [swaps.a(t + 1) if (t + 1) % layers else None for t in range(count)]
            previous = chip.hash_layer_many(layouter, self.Q, [lo + t % layers for t in range(count)], [swaps.a_swapped(t) for t in range(count)],
                                            [swaps.b_swapped(t) for t in range(count)], trace=trace, copy_digests_to=targets)
            previous_layers = layers
        roots = [None] * n
        if witness:
            roots = [Assigned.trivial(v, m) for v in fields.from_limbs(nodes[:, depth].cpu().numpy().view(np.uint64), FP)]
        return [AssignedCell(roots[p], previous.x_a(p * previous_layers + previous_layers - 1)) for p in range(n)]
