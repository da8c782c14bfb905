"""Circuit gadgets over `halo2_amd.circuit`: `poseidon` (Pow5Chip, Sponge, Hash, ConstantLength and the bulk `permute_many` / `hash2_many`),
`utilities` (LookupRangeCheckConfig, CondSwapChip) and `sinsemilla` (SinsemillaChip, MerkleChip, MerklePath and the bulk `hash_to_point_many`)."""
