"""The utility gadgets of halo2_gadgets (src/utilities.rs, utilities/lookup_range_check.rs, utilities/cond_swap.rs) against
`halo2_amd.circuit`, mirrored cell by cell: the same regions, offsets, gate and lookup shapes, selector kinds and `enable_equality`
calls, so that a circuit built from them prints the reference's pinned key.

    LookupRangeCheckConfig   the K = 10 running-sum range check over a lookup table (the plain variant)
    CondSwapChip             a' , b' = swap ? (b, a) : (a, b)
    RunningSumConfig         the running-sum decomposition into windows of at most 3 bits (utilities/decompose_running_sum.rs)
    bool_check, ternary, range_check, bitrange_subset, i2lebsp, lebs2ip, load_private"""
from __future__ import annotations

from ..circuit import Assigned, AssignedCell, Column, ConstraintSystem, Expression, Rotation, Selector, TableColumn, Value

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


# ---- CondSwapChip (cond_swap.rs:61-296) ----------------------------------------------------------------------------------------------------
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
