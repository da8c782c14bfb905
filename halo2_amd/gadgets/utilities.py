"""The utility gadgets of halo2_gadgets (src/utilities.rs, utilities/lookup_range_check.rs, utilities/cond_swap.rs) against
`halo2_amd.circuit`, mirrored cell by cell: the same regions, offsets, gate and lookup shapes, selector kinds and `enable_equality`
calls, so that a circuit built from them prints the reference's pinned key.

    LookupRangeCheckConfig   the K = 10 running-sum range check over a lookup table (the plain variant)
    LookupRangeCheck4_5BConfig   the same with a tag column: 4- and 5-bit checks take one row instead of three
    CondSwapChip             a' , b' = swap ? (b, a) : (a, b), and mux
    RunningSumConfig         the running-sum decomposition into windows of at most 3 bits (utilities/decompose_running_sum.rs)
    bool_check, ternary, range_check, bitrange_subset, i2lebsp, lebs2ip, load_private

What the reference does not have is the bulk path: `range_check_many` and `short_range_check_many` lay the checks of many values back
to back in ONE region whose running_sum column comes from the device (`halo2_amd.range_check`), cell for cell the layout of as many
single calls; `CondSwapChip.swap_many` does the same for the conditional swaps."""
from __future__ import annotations

import numpy as np

from .. import range_check as primitive
from ..circuit import Assigned, AssignedCell, Cell, Column, ConstraintSystem, Expression, Rotation, Selector, Synthesis, TableColumn, Value

K = 10


# ---- expressions and integers (utilities.rs:132-238) -------------------------------------------------------------------------------------
def range_check(word: Expression, bound: int) -> Expression:
    """word (1 - word) ... (bound - 1 - word): zero iff 0 <= word < bound"""
    acc = word
    for i in range(1, bound):
        acc = acc * (Expression.constant(i) - word)
    return acc


def bool_check(value: Expression) -> Expression:
    return range_check(value, 2)


def ternary(a: Expression, b: Expression, c: Expression) -> Expression:
    """a b + (1 - a) c"""
    one_minus_a = Expression.constant(1) - a
    return a * b + one_minus_a * c


def bitrange_subset(value: int, lo: int, hi: int) -> int:
    """bits lo .. hi - 1 of the canonical value"""
    return (value >> lo) & ((1 << (hi - lo)) - 1)


def i2lebsp(value: int, num_bits: int) -> list:
    return [bool(value >> i & 1) for i in range(num_bits)]


def lebs2ip(bits) -> int:
    return sum(1 << i for i, b in enumerate(bits) if b)


def decompose_word(word: int, word_num_bits: int, window_num_bits: int) -> list:
    """utilities.rs:184-204: the low word_num_bits bits of `word` in windows of window_num_bits, low window first, the last one padded"""
    word &= (1 << word_num_bits) - 1
    count = -(-word_num_bits // window_num_bits)
    return [word >> (window_num_bits * i) & ((1 << window_num_bits) - 1) for i in range(count)]


def value_int(value, modulus: int):
    """A cell's or a Value's content as a canonical integer, None when unknown."""
    v = value.inner if isinstance(value, Value) else value
    if v is None:
        return None
    return v.evaluate(modulus) if isinstance(v, Assigned) else int(v) % modulus


def load_private(layouter, column: Column, value) -> AssignedCell:
    """UtilitiesInstructions::load_private: one cell in a region of its own."""
    return layouter.assign_region("load private", lambda region: region.assign_advice(column, 0, lambda: value))


class RangeConstrained:
    """utilities.rs RangeConstrained: a value (an integer or None, or an AssignedCell) known to fit num_bits bits."""

    def __init__(self, inner, num_bits: int):
        self.inner, self.num_bits = inner, num_bits

    @staticmethod
    def bitrange_of(value, lo: int, hi: int) -> "RangeConstrained":
        return RangeConstrained(None if value is None else bitrange_subset(value, lo, hi), hi - lo)

    @staticmethod
    def witness_short(lookup_config: "LookupRangeCheckConfig", layouter, value, lo: int, hi: int) -> "RangeConstrained":
        """lookup_range_check.rs:37-58: witnesses bits lo .. hi - 1 of `value` and constrains them to hi - lo < K bits."""
        num_bits = hi - lo
        assert num_bits < K
        cell = lookup_config.witness_short_check(layouter, None if value is None else bitrange_subset(value, lo, hi), num_bits)
        return RangeConstrained(cell, num_bits)

    def value(self, modulus: int) -> "RangeConstrained":
        if isinstance(self.inner, AssignedCell):
            return RangeConstrained(value_int(self.inner.value(), modulus), self.num_bits)
        return self


# ---- LookupRangeCheckConfig (lookup_range_check.rs:61-491) -------------------------------------------------------------------------------------
class LookupRangeCheckConfig:
    def __init__(self, modulus, q_lookup, q_running, q_bitshift, running_sum, table_idx):
        self.modulus = modulus
        self.q_lookup, self.q_running, self.q_bitshift = q_lookup, q_running, q_bitshift
        self.running_sum, self.table_idx = running_sum, table_idx

    @staticmethod
    def configure(meta: ConstraintSystem, running_sum: Column, table_idx: TableColumn) -> "LookupRangeCheckConfig":
        meta.enable_equality(running_sum)
        q_lookup = meta.complex_selector()
        q_running = meta.complex_selector()
        q_bitshift = meta.selector()
        config = LookupRangeCheckConfig(meta.modulus, q_lookup, q_running, q_bitshift, running_sum, table_idx)

        def lookup(cells):
            q_lookup_ = cells.query_selector(q_lookup)
            q_running_ = cells.query_selector(q_running)
            z_cur = cells.query_advice(running_sum, Rotation.cur())
            one = Expression.constant(1)
            z_next = cells.query_advice(running_sum, Rotation.next())
            running_sum_word = z_cur - z_next * (1 << K)                      # a_i = z_i - 2^K z_{i+1}
            running_sum_lookup = q_running_ * running_sum_word
            q_short = one - q_running_                                        # the short check looks the witnessed word up directly
            short_lookup = q_short * z_cur
            return [(q_lookup_ * (running_sum_lookup + short_lookup), table_idx)]
        meta.lookup(lookup)

        def bitshift(cells):
            q = cells.query_selector(q_bitshift)
            word = cells.query_advice(running_sum, Rotation.prev())
            shifted_word = cells.query_advice(running_sum, Rotation.cur())
            inv_two_pow_s = cells.query_advice(running_sum, Rotation.next())
            return [q * (word * (1 << K) * inv_two_pow_s - shifted_word)]     # shifted = word 2^K 2^-s
        meta.create_gate("Short lookup bitshift", bitshift)
        return config

    def load(self, generator_table_config, layouter, table) -> None:
        """The Sinsemilla generator table: (index, x(S[index]), y(S[index])) for the 1024 generators (`table`: (x, y) integers)."""
        def assign(t):
            for index, (x, y) in enumerate(table):
                t.assign_cell(generator_table_config.table_idx, index, index)
                t.assign_cell(generator_table_config.table_x, index, x)
                t.assign_cell(generator_table_config.table_y, index, y)
        layouter.assign_table("generator_table", assign)

    def load_range_check_table(self, layouter) -> None:
        """table_idx alone (the reference's test-only loader, for circuits without the Sinsemilla chip)"""
        def assign(t):
            for index in range(1 << K):
                t.assign_cell(self.table_idx, index, index)
        layouter.assign_table("table_idx", assign)

    def copy_check(self, layouter, element: AssignedCell, num_words: int, strict: bool) -> list:
        def assign(region):
            z_0 = element.copy_advice(region, self.running_sum, 0)
            return self.range_check(region, z_0, num_words, strict)
        return layouter.assign_region(f"{num_words} words range check", assign)

    def witness_check(self, layouter, value, num_words: int, strict: bool) -> list:
        def assign(region):
            z_0 = region.assign_advice(self.running_sum, 0, lambda: value)
            return self.range_check(region, z_0, num_words, strict)
        return layouter.assign_region("Witness element", assign)

    def range_check(self, region, element: AssignedCell, num_words: int, strict: bool) -> list:
        """The running sum z_0 .. z_W of `element` (already at offset 0): z_{i+1} = (z_i - a_i) / 2^K with a_i the i-th K-bit word
        of the element's low W K bits; strict: z_W is constrained to zero."""
        m = self.modulus
        assert num_words * K <= m.bit_length() - 1
        element_int = value_int(element.value(), m)
        inv_two_pow_k = pow(1 << K, -1, m)
        zs, z, z_int = [element], element, element_int
        for idx in range(num_words):
            self.q_lookup.enable(region, idx)
            self.q_running.enable(region, idx)
            if z_int is not None:
                word = (element_int >> (K * idx)) & ((1 << K) - 1)
                z_int = (z_int - word) * inv_two_pow_k % m
            z = region.assign_advice(self.running_sum, idx + 1, lambda v=z_int: v)
            zs.append(z)
        if strict:
            region.constrain_constant(zs[-1].cell(), 0)
        return zs

    def copy_short_check(self, layouter, element: AssignedCell, num_bits: int) -> None:
        assert num_bits < K

        def assign(region):
            copied = element.copy_advice(region, self.running_sum, 0)
            self.short_range_check(region, copied, num_bits)
        layouter.assign_region(f"Range check {num_bits} bits", assign)

    def witness_short_check(self, layouter, element, num_bits: int) -> AssignedCell:
        assert num_bits <= K

        def assign(region):
            cell = region.assign_advice(self.running_sum, 0, lambda: element)
            self.short_range_check(region, cell, num_bits)
            return cell
        return layouter.assign_region(f"Range check {num_bits} bits", assign)

    def short_range_check(self, region, element: AssignedCell, num_bits: int) -> None:
        """element (at offset 0) and element 2^(K - num_bits) are both looked up; 2^-num_bits comes from a constant"""
        m = self.modulus
        self.q_lookup.enable(region, 0)
        self.q_lookup.enable(region, 1)
        self.q_bitshift.enable(region, 1)
        v = value_int(element.value(), m)
        region.assign_advice(self.running_sum, 1, lambda: None if v is None else v * (1 << (K - num_bits)) % m)
        region.assign_advice_from_constant(self.running_sum, 2, pow(1 << num_bits, -1, m))

    # ---- the bulk path ---------------------------------------------------------------------------------------------------------------------
    def _field(self) -> int:
        from .. import fields
        return next(f for f, m in fields.MODULUS.items() if m == self.modulus)

    def _bulk_rows(self, layouter, elements, values, trace, rows: int, what: str, launch):
        """The running_sum column of a bulk region, (len(elements) * rows, 4): zeros without a witness, else `trace` or launch(values)."""
        import torch

        from .. import fields
        count, m = len(elements), self.modulus
        if not layouter.cs.collect_advice or not count:
            return np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (count * rows, 4))
        if trace is None:
            if values is None:
                ints = [value_int(e.value(), m) if isinstance(e, AssignedCell) else (None if e is None else int(e) % m) for e in elements]
                if any(v is None for v in ints):
                    raise Synthesis(f"{what}: a witness is needed and there is none")
                values = fields.to_limbs(ints, self._field(), montgomery=False)
            if not torch.is_tensor(values):
                values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)).to(fields.current_device())
            trace = launch(values)
        if not torch.is_tensor(trace):
            trace = torch.from_numpy(np.ascontiguousarray(trace, dtype=np.uint64).view(np.int64))
        if trace.numel() != count * rows * 4:
            raise ValueError(f"{what}: the trace is (count, {rows}, 4)")
        return trace.reshape(count * rows, 4)

    def range_check_many(self, layouter, elements, num_words: int, strict: bool, values=None, trace=None) -> list:
        """`witness_check` (an integer, or None without a witness) or `copy_check` (an AssignedCell) of every element, back to back in one
        region of len(elements) * (num_words + 1) rows; per element the gates, lookups and equality constraints of the single call.
        values: the (count, 4) CANONICAL limbs of the elements where the caller has them on the device (else they are read from the
        elements); trace: the (count, num_words + 1, 4) rows where the caller has them (else `range_check.decompose`, once).  Without a
        witness (keygen) the same shape is laid out and nothing is launched.  -> per element the cells z_0 .. z_W."""
        num_words = int(num_words)
        assert 1 <= num_words and num_words * K <= self.modulus.bit_length() - 1
        count, rows = len(elements), num_words + 1
        column = self._bulk_rows(layouter, elements, values, trace, rows, "range_check_many",
                                 lambda v: primitive.decompose(v, num_words, field=self._field()))
        base = rows * np.arange(count, dtype=np.int64)
        word_rows = (base[:, None] + np.arange(num_words, dtype=np.int64)[None, :]).reshape(-1)

        def assign(region):
            index = region.region_index
            region.assign_advice_column(self.running_sum, 0, column)
            region.enable_selector_rows(self.q_lookup, word_rows)
            region.enable_selector_rows(self.q_running, word_rows)
            for i, element in enumerate(elements):
                if isinstance(element, AssignedCell):
                    region.constrain_equal(Cell(index, rows * i, self.running_sum), element.cell())
                if strict:
                    region.constrain_constant(Cell(index, rows * i + num_words, self.running_sum), 0)
            return index
        index = layouter.assign_region(f"{num_words} words range check many", assign)
        return [[Cell(index, rows * i + j, self.running_sum) for j in range(rows)] for i in range(count)]

    def _short_selectors(self, num_bits: int):
        """the selectors a short check of num_bits enables beside q_lookup on its one row, or None where it takes the three rows"""
        return None

    def short_range_check_many(self, layouter, elements, num_bits: int, values=None, trace=None) -> list:
        """`witness_short_check` (an integer, or None) or `copy_short_check` (an AssignedCell) of every element in one region: three rows
        each -- the element, its shift (q_lookup on both, q_bitshift on the second) and the constant 2^-num_bits -- or one row each
        where the config has a selector for num_bits (the 4- and 5-bit checks of LookupRangeCheck4_5BConfig).  values: as
        `range_check_many`; trace: the (count, 3, 4) rows of `range_check.short`.  -> per element the cell of the element."""
        num_bits = int(num_bits)
        assert 0 <= num_bits <= K
        count, m = len(elements), self.modulus
        rows3 = self._bulk_rows(layouter, elements, values, trace, 3, "short_range_check_many",
                                lambda v: primitive.short(v, num_bits, field=self._field()))
        tagged = self._short_selectors(num_bits)
        rows = 3 if tagged is None else 1
        column = rows3 if tagged is None else rows3[0::3]
        base = rows * np.arange(count, dtype=np.int64)
        inv_two_pow_s = pow(1 << num_bits, -1, m)

        def assign(region):
            index = region.region_index
            region.assign_advice_column(self.running_sum, 0, column)
            if tagged is None:
                region.enable_selector_rows(self.q_lookup, np.stack([base, base + 1], axis=1).reshape(-1))
                region.enable_selector_rows(self.q_bitshift, base + 1)
            else:
                region.enable_selector_rows(self.q_lookup, base)
                region.enable_selector_rows(tagged, base)
            for i, element in enumerate(elements):
                if isinstance(element, AssignedCell):
                    region.constrain_equal(Cell(index, rows * i, self.running_sum), element.cell())
                if tagged is None:
                    region.constrain_constant(Cell(index, rows * i + 2, self.running_sum), inv_two_pow_s)
            return index
        index = layouter.assign_region(f"Range check {num_bits} bits many", assign)
        return [Cell(index, rows * i, self.running_sum) for i in range(count)]


# ---- LookupRangeCheck4_5BConfig (lookup_range_check.rs:504-851) ----------------------------------------------------------------------------------
class LookupRangeCheck4_5BConfig(LookupRangeCheckConfig):
    """The range check over a table of 2^10 + 2^4 + 2^5 rows with a tag column (0, 4, 5): a 4- or 5-bit check is ONE lookup of
    (value, tag) instead of the three rows of the shifted pair.  The shared methods are the base's; they read q_lookup, q_running,
    q_bitshift and running_sum from this object, as the reference's trait reads them through config()."""

    def __init__(self, modulus, q_lookup, q_running, q_bitshift, running_sum, table_idx, q_range_check_4, q_range_check_5,
                 table_range_check_tag):
        super().__init__(modulus, q_lookup, q_running, q_bitshift, running_sum, table_idx)
        self.q_range_check_4, self.q_range_check_5, self.table_range_check_tag = q_range_check_4, q_range_check_5, table_range_check_tag

    @staticmethod
    def configure(meta: ConstraintSystem, running_sum: Column, table_idx: TableColumn) -> "LookupRangeCheck4_5BConfig":
        table_range_check_tag = meta.lookup_table_column()
        return LookupRangeCheck4_5BConfig.configure_with_tag(meta, running_sum, table_idx, table_range_check_tag)

    @staticmethod
    def configure_with_tag(meta: ConstraintSystem, running_sum: Column, table_idx: TableColumn,
                           table_range_check_tag: TableColumn) -> "LookupRangeCheck4_5BConfig":
        meta.enable_equality(running_sum)
        q_lookup = meta.complex_selector()
        q_running = meta.complex_selector()
        q_bitshift = meta.selector()
        q_range_check_4 = meta.complex_selector()
        q_range_check_5 = meta.complex_selector()
        config = LookupRangeCheck4_5BConfig(meta.modulus, q_lookup, q_running, q_bitshift, running_sum, table_idx, q_range_check_4,
                                            q_range_check_5, table_range_check_tag)

        def lookup(cells):                                                    # the trees in the reference's order: the pinned key prints them
            q_lookup_ = cells.query_selector(q_lookup)
            q_running_ = cells.query_selector(q_running)
            q_4 = cells.query_selector(q_range_check_4)
            q_5 = cells.query_selector(q_range_check_5)
            z_cur = cells.query_advice(running_sum, Rotation.cur())
            one = Expression.constant(1)
            z_next = cells.query_advice(running_sum, Rotation.next())
            running_sum_word = z_cur - z_next * (1 << K)                      # a_i = z_i - 2^K z_{i+1}
            running_sum_lookup = q_running_ * running_sum_word
            q_short = one - q_running_
            short_lookup = q_short * z_cur
            q_range_check = one - (one - q_4) * (one - q_5)                   # 1 iff q_4 or q_5
            num_bits = q_5 * Expression.constant(5) + (one - q_5) * q_4 * Expression.constant(4)
            return [(q_lookup_ * ((one - q_range_check) * (running_sum_lookup + short_lookup) + q_range_check * z_cur), table_idx),
                    (q_lookup_ * q_range_check * num_bits, table_range_check_tag)]
        meta.lookup(lookup)

        def bitshift(cells):
            q = cells.query_selector(q_bitshift)
            word = cells.query_advice(running_sum, Rotation.prev())
            shifted_word = cells.query_advice(running_sum, Rotation.cur())
            inv_two_pow_s = cells.query_advice(running_sum, Rotation.next())
            return [q * (word * (1 << K) * inv_two_pow_s - shifted_word)]
        meta.create_gate("Short lookup bitshift", bitshift)
        return config

    def load(self, generator_table_config, layouter, table) -> None:
        """The generator table with its tag: rows 0 .. 1023 tagged 0, the first 16 again at 1024 .. tagged 4, the first 32 again at
        1040 .. tagged 5; assigned in the reference's interleaved order."""
        g = generator_table_config

        def assign(t):
            for index, (x, y) in enumerate(table):
                copies = [(index, 0)]
                if index < 1 << 4:
                    copies.append((index + (1 << K), 4))
                if index < 1 << 5:
                    copies.append((index + (1 << K) + (1 << 4), 5))
                for row, tag in copies:
                    t.assign_cell(g.table_idx, row, index)
                    t.assign_cell(g.table_x, row, x)
                    t.assign_cell(g.table_y, row, y)
                    t.assign_cell(self.table_range_check_tag, row, tag)
        layouter.assign_table("generator_table", assign)

    def load_range_check_table(self, layouter) -> None:
        def assign(t):
            offset = 0
            for size, tag in ((1 << K, 0), (1 << 4, 4), (1 << 5, 5)):
                for index in range(size):
                    t.assign_cell(self.table_idx, offset + index, index)
                    t.assign_cell(self.table_range_check_tag, offset + index, tag)
                offset += size
        layouter.assign_table("table_idx", assign)

    def _short_selectors(self, num_bits: int):
        return {4: self.q_range_check_4, 5: self.q_range_check_5}.get(num_bits)

    def short_range_check(self, region, element: AssignedCell, num_bits: int) -> None:
        tagged = self._short_selectors(num_bits)
        if tagged is None:
            return super().short_range_check(region, element, num_bits)
        self.q_lookup.enable(region, 0)
        tagged.enable(region, 0)


# ---- CondSwapChip (cond_swap.rs:61-296) ----------------------------------------------------------------------------------------------------
class SwapMany:
    """What `swap_many` returns: the cells of pair i by position."""

    def __init__(self, region_index, config, count):
        self.region_index, self.config, self.count = region_index, config, count

    def a(self, i: int) -> Cell:
        return Cell(self.region_index, i, self.config.a)

    def a_swapped(self, i: int) -> Cell:
        return Cell(self.region_index, i, self.config.a_swapped)

    def b_swapped(self, i: int) -> Cell:
        return Cell(self.region_index, i, self.config.b_swapped)


class CondSwapConfig:
    def __init__(self, q_swap: Selector, a, b, a_swapped, b_swapped, swap):
        self.q_swap, self.a, self.b, self.a_swapped, self.b_swapped, self.swap = q_swap, a, b, a_swapped, b_swapped, swap


class CondSwapChip:
    def __init__(self, config: CondSwapConfig):
        self.config = config

    @staticmethod
    def configure(meta: ConstraintSystem, advices) -> CondSwapConfig:
        a = advices[0]
        meta.enable_equality(a)
        q_swap = meta.selector()
        config = CondSwapConfig(q_swap, a, advices[1], advices[2], advices[3], advices[4])

        def gate(cells):
            q = cells.query_selector(q_swap)
            a_ = cells.query_advice(config.a, Rotation.cur())
            b_ = cells.query_advice(config.b, Rotation.cur())
            a_swapped = cells.query_advice(config.a_swapped, Rotation.cur())
            b_swapped = cells.query_advice(config.b_swapped, Rotation.cur())
            swap = cells.query_advice(config.swap, Rotation.cur())
            a_check = a_swapped - ternary(swap, b_, a_)
            b_check = b_swapped - ternary(swap, a_, b_)
            return [("a check", q * a_check), ("b check", q * b_check), ("swap is bool", q * bool_check(swap))]
        meta.create_gate("a' = b ⋅ swap + a ⋅ (1-swap)", gate)
        return config

    def swap(self, layouter, pair, swap):
        """pair: (AssignedCell a, value b); swap: bool or None.  -> (a', b') cells"""
        c = self.config
        a_in, b_in = pair

        def assign(region):
            c.q_swap.enable(region, 0)
            a = a_in.copy_advice(region, c.a, 0)
            b = region.assign_advice(c.b, 0, lambda: b_in)
            region.assign_advice(c.swap, 0, lambda: None if swap is None else int(bool(swap)))
            known = swap is not None and a.value().inner is not None and b.value().inner is not None
            first = (b.value().inner if swap else a.value().inner) if known else None
            second = (a.value().inner if swap else b.value().inner) if known else None
            a_swapped = region.assign_advice(c.a_swapped, 0, lambda: first)
            b_swapped = region.assign_advice(c.b_swapped, 0, lambda: second)
            return a_swapped, b_swapped
        return layouter.assign_region("swap", assign)

    # ---- the bulk path ---------------------------------------------------------------------------------------------------------------------
    def swap_many(self, layouter, a_cells, b_values, swaps, trace=None) -> "SwapMany":
        """`swap` of count = len(a_cells) pairs back to back in one region of count rows; per pair the gate and the one equality
        constraint of the single call.  a_cells[i]: the AssignedCell or Cell that row i's `a` is a copy of, or None where the caller
        ties that cell itself (to a cell of a region laid out later); b_values[i], swaps[i]: an integer and a bool, None each without
        a witness.  trace: the (5, count, 4) Montgomery columns a, b, a_swapped, b_swapped, swap where the caller has them on the
        device (else they are formed here from the cells' values).  Without a witness (keygen) the same shape is laid out."""
        import torch

        from .. import fields
        c, count = self.config, len(a_cells)
        if len(b_values) != count or len(swaps) != count:
            raise ValueError("swap_many: one b and one swap per a")
        blank = np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (count, 4))
        if not layouter.cs.collect_advice or not count:
            columns = [blank] * 5
        else:
            if trace is None:
                m, field = layouter.cs.m, layouter.cs.field
                a_ints = [value_int(a.value(), m) if isinstance(a, AssignedCell) else None for a in a_cells]
                if any(v is None for v in a_ints) or any(v is None for v in b_values) or any(s is None for s in swaps):
                    raise Synthesis("swap_many: a witness is needed and there is none")
                b_ints, bits = [int(v) % m for v in b_values], [int(bool(s)) for s in swaps]
                rows = [a_ints, b_ints, [b if s else a for a, b, s in zip(a_ints, b_ints, bits)],
                        [a if s else b for a, b, s in zip(a_ints, b_ints, bits)], bits]
                trace = fields.to_limbs([v for row in rows for v in row], field).reshape(5, count, 4)
            if not torch.is_tensor(trace):
                trace = torch.from_numpy(np.ascontiguousarray(trace, dtype=np.uint64).view(np.int64))
            if tuple(trace.shape) != (5, count, 4):
                raise ValueError("swap_many: the trace is (5, count, 4)")
            columns = [trace[j] for j in range(5)]

        def assign(region):
            index = region.region_index
            for column, values in zip((c.a, c.b, c.a_swapped, c.b_swapped, c.swap), columns):
                region.assign_advice_column(column, 0, values)
            region.enable_selector_rows(c.q_swap, np.arange(count, dtype=np.int64))
            for i, a in enumerate(a_cells):
                if a is not None:
                    region.constrain_equal(Cell(index, i, c.a), a.cell() if isinstance(a, AssignedCell) else a)
            return index
        return SwapMany(layouter.assign_region("swap many", assign), c, count)

    def mux(self, layouter, choice: AssignedCell, left: AssignedCell, right: AssignedCell) -> AssignedCell:
        """cond_swap.rs:137-190: `left` where choice is 0, else `right`; the three cells are copied in"""
        c = self.config

        def is_zero(v):
            return v.is_zero_vartime() if isinstance(v, Assigned) else int(v) == 0

        def assign(region):
            c.q_swap.enable(region, 0)
            left_ = left.copy_advice(region, c.a, 0)
            right_ = right.copy_advice(region, c.b, 0)
            choice_ = choice.copy_advice(region, c.swap, 0)
            l_v, r_v, c_v = left_.value().inner, right_.value().inner, choice_.value().inner
            known = l_v is not None and r_v is not None and c_v is not None
            a_swapped = (l_v if is_zero(c_v) else r_v) if known else None
            b_swapped = (r_v if is_zero(c_v) else l_v) if known else None
            region.assign_advice(c.b_swapped, 0, lambda: b_swapped)
            return region.assign_advice(c.a_swapped, 0, lambda: a_swapped)
        return layouter.assign_region("mux", assign)

    def mux_on_points(self, layouter, choice: AssignedCell, left, right):
        """cond_swap.rs:196-209 -> EccPoint (from unchecked coordinates)"""
        from .ecc import EccPoint
        x_cell = self.mux(layouter, choice, left.x(), right.x())
        y_cell = self.mux(layouter, choice, left.y(), right.y())
        return EccPoint(x_cell, y_cell)

    def mux_on_non_identity_points(self, layouter, choice: AssignedCell, left, right):
        """cond_swap.rs:213-226 -> NonIdentityEccPoint (from unchecked coordinates)"""
        from .sinsemilla import NonIdentityEccPoint
        x_cell = self.mux(layouter, choice, left.x(), right.x())
        y_cell = self.mux(layouter, choice, left.y(), right.y())
        return NonIdentityEccPoint(x_cell, y_cell)


# ---- RunningSumConfig (decompose_running_sum.rs:47-206) ----------------------------------------------------------------------------------------
class RunningSumConfig:
    """z_0 = alpha, z_(i+1) = (z_i - k_i) / 2^window_num_bits with every k_i range-checked by a polynomial of degree 2^window_num_bits."""

    def __init__(self, modulus, q_range_check, z, window_num_bits):
        self.modulus, self.q_range_check, self.z, self.window_num_bits = modulus, q_range_check, z, window_num_bits

    @staticmethod
    def configure(meta: ConstraintSystem, q_range_check: Selector, z: Column, window_num_bits: int = 3) -> "RunningSumConfig":
        assert window_num_bits <= 3
        meta.enable_equality(z)
        config = RunningSumConfig(meta.modulus, q_range_check, z, window_num_bits)

        def gate(cells):
            q = cells.query_selector(config.q_range_check)
            z_cur = cells.query_advice(config.z, Rotation.cur())
            z_next = cells.query_advice(config.z, Rotation.next())
            word = z_cur - z_next * (1 << window_num_bits)                    # k_i = z_i - 2^K z_(i+1)
            return [("range check", q * range_check(word, 1 << window_num_bits))]
        meta.create_gate("range check", gate)
        return config

    def witness_decompose(self, region, offset: int, alpha, strict: bool, word_num_bits: int, num_windows: int) -> list:
        z_0 = region.assign_advice(self.z, offset, lambda: alpha)
        return self._decompose(region, offset, z_0, strict, word_num_bits, num_windows)

    def copy_decompose(self, region, offset: int, alpha: AssignedCell, strict: bool, word_num_bits: int, num_windows: int) -> list:
        z_0 = alpha.copy_advice(region, self.z, offset)
        return self._decompose(region, offset, z_0, strict, word_num_bits, num_windows)

    def _decompose(self, region, offset: int, z_0: AssignedCell, strict: bool, word_num_bits: int, num_windows: int) -> list:
        """-> [z_0 .. z_num_windows]"""
        bits, m = self.window_num_bits, self.modulus
        assert bits * num_windows < word_num_bits + bits                      # no empty window
        for idx in range(num_windows):
            self.q_range_check.enable(region, offset + idx)
        z_v = value_int(z_0.value(), m)
        words = [None] * num_windows if z_v is None else decompose_word(z_v, word_num_bits, bits)[:num_windows]
        inv = pow(1 << bits, -1, m)
        zs = [z_0]
        for i, word in enumerate(words):
            z_v = None if z_v is None else (z_v - word) * inv % m
            zs.append(region.assign_advice(self.z, offset + i + 1, lambda v=z_v: v))
        if strict:
            region.constrain_constant(zs[-1].cell(), 0)
        return zs
