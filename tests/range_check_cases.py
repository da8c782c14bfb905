"""Shared by test_range_check_host.py and test_gpu_range_check.py: the reference's test circuits over either lookup range check --
MyLookupCircuit and MyShortRangeCheckCircuit (utilities/lookup_range_check.rs, tests), MyCondSwapCircuit and MyMuxCircuit
(utilities/cond_swap.rs, tests), and the ECC, Merkle and Sinsemilla circuits of the neighbouring helper modules with their `configure`
swapped for the 4_5b lookup -- the eleven pinned keys they print, and the circuit of the bulk path."""
import random

import ecc_cases as ec
import ecc_fixed_cases as fx
import sinsemilla_cases as sc
import sinsemilla_commit_cases as cc
from halo2_amd.circuit import Circuit
from halo2_amd.gadgets.ecc import EccChip, FixedPoints, NonIdentityPoint, Point
from halo2_amd.gadgets.sinsemilla import MerkleChip, SinsemillaChip
from halo2_amd.gadgets.utilities import CondSwapChip, LookupRangeCheck4_5BConfig, LookupRangeCheckConfig, load_private

P = sc.P
K = 10
LOOKUPS = {"plain": LookupRangeCheckConfig, "4_5b": LookupRangeCheck4_5BConfig}


def configure_lookup(meta, lookup):
    """MyLookupCircuit::configure and MyShortRangeCheckCircuit::configure (lookup_range_check.rs:908-915, :1031-1038)"""
    running_sum = meta.advice_column()
    table_idx = meta.lookup_table_column()
    constants = meta.fixed_column()
    meta.enable_constant(constants)
    return lookup.configure(meta, running_sum, table_idx)


class LookupCircuit(sc.LookupCircuit):
    """MyLookupCircuit over either config; its synthesize is sinsemilla_cases.LookupCircuit's"""

    def __init__(self, num_words, lookup="4_5b"):
        super().__init__(num_words)
        self.lookup = lookup

    def without_witnesses(self):
        return LookupCircuit(self.num_words, self.lookup)

    def configure(self, meta):
        return configure_lookup(meta, LOOKUPS[self.lookup])


class ShortRangeCheckCircuit(Circuit):
    """MyShortRangeCheckCircuit (lookup_range_check.rs:1004-1057): the table, then one witness_short_check"""

    def __init__(self, element, num_bits, lookup):
        self.element, self.num_bits, self.lookup = element, num_bits, lookup

    def without_witnesses(self):
        return ShortRangeCheckCircuit(None, self.num_bits, self.lookup)

    def configure(self, meta):
        return configure_lookup(meta, LOOKUPS[self.lookup])

    def synthesize(self, config, layouter):
        config.load_range_check_table(layouter)
        config.witness_short_check(layouter, self.element, self.num_bits)


# the reference's short_range_check cases (lookup_range_check.rs:1076-1248): (element, num_bits, failing offsets of the check's region)
CRAFTED = 63 * pow(1 << 4, -1, P) % P                                         # not 6 bits, but its shift by 2^(K - 6) is
SHORT_CASES = [(0, 0, []), ((1 << K) - 1, K, []), (63, 6, []), (64, 6, [1]), (1 << K, 6, [0, 1]), (CRAFTED, 6, [0])]
SHORT_CASES_4_5B = [(15, 4, []), (32, 5, [0]), (16, 4, [0]), (31, 5, [])]
# name of the stored key -> (circuit, proof length)
STORED_SHORT = {f"short_range_check{tag}_case{i}": (lambda e=e, s=s, n=n: ShortRangeCheckCircuit(e, s, n), size)
                for n, tag, size in (("plain", "", 1888), ("4_5b", "_4_5b", 2048))
                for i, (e, s) in enumerate([(0, 0), ((1 << K) - 1, K), (63, 6)] + ([(15, 4)] if n == "4_5b" else []))}


def region_offsets(layouter, failures):
    """("Lookup", index, row) of the model -> (index, region as the reference counts it, offset): the reference's MockProver counts the
    table's assignment as region 0, this layouter does not"""
    out = []
    for kind, index, row in failures:
        assert kind == "Lookup"
        region = max(i for i, start in enumerate(layouter.regions) if start <= row and row < start + layouter.shapes[i][1])
        out.append((index, region + 1, row - layouter.regions[region]))
    return out


# ---- cond_swap.rs tests ------------------------------------------------------------------------------------------------------------------
class CondSwapCircuit(Circuit):
    """MyCondSwapCircuit (cond_swap.rs:320-377)"""

    def __init__(self, a=None, b=None, swap=None):
        self.a, self.b, self.swap, self.pair = a, b, swap, None

    def without_witnesses(self):
        return CondSwapCircuit()

    def configure(self, meta):
        return CondSwapChip.configure(meta, [meta.advice_column() for _ in range(5)])

    def synthesize(self, config, layouter):
        chip = CondSwapChip(config)
        a = load_private(layouter, config.a, self.a)
        self.pair = chip.swap(layouter, (a, self.b), self.swap)


class MuxCircuit(Circuit):
    """MyMuxCircuit (cond_swap.rs:422-598): the mux of two non-identity points, then of two points, both bound to the instance"""

    def __init__(self, left=None, right=None, choice=None, lookup="plain"):
        self.left, self.right, self.choice, self.lookup = left, right, choice, lookup

    def without_witnesses(self):
        return MuxCircuit(lookup=self.lookup)

    def configure(self, meta):
        advices = [meta.advice_column() for _ in range(10)]
        for advice in advices:
            meta.enable_equality(advice)
        primary = meta.instance_column()
        meta.enable_equality(primary)
        cond_swap_config = CondSwapChip.configure(meta, advices[:5])
        table_idx = meta.lookup_table_column()
        lagrange = [meta.fixed_column() for _ in range(8)]
        meta.enable_constant(lagrange[0])
        range_check = LOOKUPS[self.lookup].configure(meta, advices[9], table_idx)
        ecc_config = EccChip.configure(meta, advices, lagrange, range_check,
                                       fixed_bases=FixedPoints(full_width=("generator",), short=("generator",), base_field=("generator",)))
        return primary, advices[0], cond_swap_config, ecc_config

    def synthesize(self, config, layouter):
        primary, advice, cond_swap_config, ecc_config = config
        cond_swap_chip, ecc_chip = CondSwapChip(cond_swap_config), EccChip(ecc_config)
        choice = load_private(layouter, advice, self.choice)
        left = NonIdentityPoint.new(ecc_chip, layouter, self.left)
        right = NonIdentityPoint.new(ecc_chip, layouter, self.right)
        result = cond_swap_chip.mux_on_non_identity_points(layouter, choice, left.inner(), right.inner())
        layouter.constrain_instance(result.x().cell(), primary, 0)
        layouter.constrain_instance(result.y().cell(), primary, 1)
        left = Point.new(ecc_chip, layouter, self.left)
        right = Point.new(ecc_chip, layouter, self.right)
        result = cond_swap_chip.mux_on_points(layouter, choice, left.inner(), right.inner())
        layouter.constrain_instance(result.x().cell(), primary, 0)
        layouter.constrain_instance(result.y().cell(), primary, 1)


# ---- the stored circuits over the 4_5b lookup ----------------------------------------------------------------------------------------------
def configure_fixed_4_5b(meta):
    """ecc_fixed_cases.configure_fixed with Lookup = PallasLookupRangeCheck4_5BConfig"""
    advices = [meta.advice_column() for _ in range(10)]
    lookup_table = meta.lookup_table_column()
    lagrange = [meta.fixed_column() for _ in range(8)]
    constants = meta.fixed_column()
    meta.enable_constant(constants)
    range_check = LookupRangeCheck4_5BConfig.configure(meta, advices[9], lookup_table)
    return EccChip.configure(meta, advices, lagrange, range_check,
                             fixed_bases=FixedPoints(full_width=("generator",), short=("generator",), base_field=("generator",)))


class EccCircuit45(fx.MyEccCircuit):
    """MyEccCircuit<PallasLookupRangeCheck4_5BConfig> (ecc.rs:776-1010)"""

    def without_witnesses(self):
        return EccCircuit45(self.full, self.short, self.seed, witness=False)

    configure = staticmethod(configure_fixed_4_5b)


class MerkleCircuit45(sc.MerkleCircuit):
    """MyMerkleCircuitWithHashFromPrivatePoint<PallasLookupRangeCheck4_5BConfig> (merkle.rs:450-573): MyMerkleCircuit's synthesize over
    chips configured with allow_init_from_private_point"""

    def configure(self, meta):
        advices = [meta.advice_column() for _ in range(10)]
        constants = meta.fixed_column()
        meta.enable_constant(constants)
        fixed_y_q_1, fixed_y_q_2 = meta.fixed_column(), meta.fixed_column()
        lookup = (meta.lookup_table_column(), meta.lookup_table_column(), meta.lookup_table_column())
        range_check = LookupRangeCheck4_5BConfig.configure(meta, advices[9], lookup[0])
        sinsemilla_1 = SinsemillaChip.configure(meta, advices[5:], advices[7], fixed_y_q_1, lookup, range_check, table=self.table,
                                                allow_init_from_private_point=True)
        config_1 = MerkleChip.configure(meta, sinsemilla_1)
        sinsemilla_2 = SinsemillaChip.configure(meta, advices[:5], advices[2], fixed_y_q_2, lookup, range_check, table=self.table,
                                                allow_init_from_private_point=True)
        config_2 = MerkleChip.configure(meta, sinsemilla_2)
        return config_1, config_2


class SinsemillaCircuit45(cc.MySinsemillaCircuit):
    """MySinsemillaCircuitWithHashFromPrivatePoint<PallasLookupRangeCheck4_5BConfig> (sinsemilla.rs:863-897): MySinsemillaCircuit's
    synthesize -- no hash from a private point in it -- over chips configured with allow_init_from_private_point"""

    def __init__(self, domain, table=None, seed=1, witness=True):
        super().__init__(domain, table, seed, witness, private=False, flag=True)

    def without_witnesses(self):
        return SinsemillaCircuit45(self.domain, self.table, self.seed, witness=False)

    def configure(self, meta):
        advices = [meta.advice_column() for _ in range(10)]
        constants = meta.fixed_column()
        meta.enable_constant(constants)
        table_idx = meta.lookup_table_column()
        lagrange = [meta.fixed_column() for _ in range(8)]
        lookup = (table_idx, meta.lookup_table_column(), meta.lookup_table_column())
        range_check = LookupRangeCheck4_5BConfig.configure(meta, advices[9], table_idx)
        ecc_config = EccChip.configure(meta, advices, lagrange, range_check,
                                       fixed_bases=FixedPoints(full_width=("R",), short=("R",), base_field=("R",)))
        config1 = SinsemillaChip.configure(meta, advices[:5], advices[2], lagrange[0], lookup, range_check, table=self.table,
                                           allow_init_from_private_point=True)
        config2 = SinsemillaChip.configure(meta, advices[5:], advices[7], lagrange[1], lookup, range_check, table=self.table,
                                           allow_init_from_private_point=True)
        return ecc_config, config1, config2


def stored_circuits(ecc_tables, domain, table=None):
    """name of the stored key -> (circuit without witnesses, file of the key, proof length), all eleven.  ecc_tables: the generator's
    (full, short) tables; domain: the CommitDomains of the Sinsemilla circuit; table: the generator table to inject, if any."""
    out = {"lookup_range_check_4_5b": (lambda: LookupCircuit(6, "4_5b"), "vk_lookup_range_check_4_5b.rdata", 2048)}
    for name, (make, size) in STORED_SHORT.items():
        out[name] = (make, f"vk_{name}.rdata", size)
    out["ecc_chip_4_5b"] = (lambda: EccCircuit45(*ecc_tables()).without_witnesses(), "vk_ecc_chip_4_5b.rdata.gz", 3968)
    out["merkle_with_private_init_chip_4_5b"] = (lambda: MerkleCircuit45(q=None if table is None else sc.q_of(sc.TEST_DOMAIN), table=table),
                                                 "vk_merkle_with_private_init_chip_4_5b.rdata.gz", 4160)
    out["sinsemilla_with_private_init_chip_4_5b"] = (lambda: SinsemillaCircuit45(domain(), table=table).without_witnesses(),
                                                     "vk_sinsemilla_with_private_init_chip_4_5b.rdata.gz", 4672)
    return out


STORED_NAMES = ["lookup_range_check_4_5b"] + list(STORED_SHORT) + ["ecc_chip_4_5b", "merkle_with_private_init_chip_4_5b",
                                                                   "sinsemilla_with_private_init_chip_4_5b"]
assert len(STORED_NAMES) == 11


# ---- the bulk path -------------------------------------------------------------------------------------------------------------------------
class BulkCircuit(Circuit):
    """checks: ("words", elements, num_words, strict) and ("bits", elements, num_bits), each through one `*_many` call (many=True) or a
    loop of witness_check / witness_short_check (many=False).  copy: every element is first witnessed in a second advice column and
    the checks copy it in (copy_check / copy_short_check) instead."""

    def __init__(self, checks, lookup="4_5b", many=False, witness=True, copy=False):
        self.checks, self.lookup, self.many, self.witness, self.copy = checks, lookup, many, witness, copy
        self.cells = []

    def without_witnesses(self):
        return BulkCircuit(self.checks, self.lookup, self.many, witness=False, copy=self.copy)

    def configure(self, meta):
        config = configure_lookup(meta, LOOKUPS[self.lookup])
        self.inputs = meta.advice_column()
        meta.enable_equality(self.inputs)
        return config

    def synthesize(self, config, layouter):
        config.load_range_check_table(layouter)
        self.cells = []
        for check in self.checks:
            elements = [e if self.witness else None for e in check[1]]
            if self.copy:
                elements = [load_private(layouter, self.inputs, e) for e in elements]
            if check[0] == "words":
                _, _, num_words, strict = check
                if self.many:
                    self.cells.append(config.range_check_many(layouter, elements, num_words, strict))
                elif self.copy:
                    self.cells.append([[z.cell() for z in config.copy_check(layouter, e, num_words, strict)] for e in elements])
                else:
                    self.cells.append([[z.cell() for z in config.witness_check(layouter, e, num_words, strict)] for e in elements])
            else:
                num_bits = check[2]
                if self.many:
                    self.cells.append(config.short_range_check_many(layouter, elements, num_bits))
                elif self.copy:
                    for e in elements:
                        config.copy_short_check(layouter, e, num_bits)
                else:
                    self.cells.append([config.witness_short_check(layouter, e, num_bits).cell() for e in elements])


def bulk_checks(count=65, seed=5):
    """the circuit of the device test: `count` values at 13 words, strict; at 25 words, not strict, some wider than 250 bits; and
    `count` short checks each at 4, 5 and 6 bits"""
    rng = random.Random(seed)
    wide = [rng.randrange(P) if i % 4 == 0 else rng.getrandbits(250) for i in range(count)]
    return [("words", [0, (1 << 130) - 1] + [rng.getrandbits(130) for _ in range(count - 2)], 13, True),
            ("words", wide, 25, False)] + \
           [("bits", [0, (1 << s) - 1] + [rng.getrandbits(s) for _ in range(count - 2)], s) for s in (4, 5, 6)]
