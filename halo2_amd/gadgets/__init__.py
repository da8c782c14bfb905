"""Circuit gadgets over `halo2_amd.circuit`: `poseidon` (Pow5Chip, Sponge, Hash, ConstantLength and the bulk `permute_many` / `hash2_many`)."""
