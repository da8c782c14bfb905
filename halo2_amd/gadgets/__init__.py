"""Circuit gadgets over `halo2_amd.circuit`: `poseidon` (Pow5Chip, Sponge, Hash, ConstantLength and the bulk `permute_many` / `hash2_many`),
`utilities` (LookupRangeCheckConfig, LookupRangeCheck4_5BConfig with the bulk `range_check_many` / `short_range_check_many`, CondSwapChip), `sinsemilla` (SinsemillaChip, MerkleChip, MerklePath and the bulk `hash_to_point_many`)
and `ecc` (EccChip: witness_point, add_incomplete, add, variable-base mul and the bulk `mul_many`)."""
from .ecc import (EccChip, EccConfig, EccPoint, MulMany, NonIdentityEccPoint, NonIdentityPoint, Point, ScalarVar)  # noqa: F401
