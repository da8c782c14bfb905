"""halo2_amd: MI355X-native (gfx950) implementation of the halo2_proofs prover hot path --
Pasta MSM (`best_multiexp`, `Params::commit*`) and NTT (`best_fft`, `EvaluationDomain`) -- behind a
C ABI (include/halo2_mi355x.h, halo2_amd/libhalo2_mi355x.so).  This package is the thin host-side mirror
of the reference's interface; all compute is hand-written HIP in halo2_amd/csrc/."""
from ._lib import (FORM_CANONICAL, FORM_MONTGOMERY, FP, FQ, LIB_PATH, PALLAS, VESTA, H2Error, lib)  # noqa: F401
from .arithmetic import (assigned_to_field, batch_invert, best_fft, best_fft_batch, best_multiexp, compute_inner_product, eval_polynomial,  # noqa: F401
                         fold_scalars, grand_product, kate_division, msm_window_bits, parallel_generator_collapse,
                         ipa_s_combine, points_sum, powers, scale_add, selector_combine, selector_conflicts, small_multiexp)
from .commitment import Blind, Params, hash_to_curve, lagrange_basis, points_from_bytes, points_to_bytes  # noqa: F401
from .domain import EvaluationDomain  # noqa: F401
from . import poseidon  # noqa: F401
from . import sinsemilla  # noqa: F401
from . import ecc  # noqa: F401
from . import range_check  # noqa: F401
from .poly import Coeff, ExtendedLagrangeCoeff, LagrangeCoeff, Polynomial  # noqa: F401
from .circuit import (Assigned, Circuit, Column, ConstraintSystem, Expression, Rotation, Selector, SimpleFloorPlanner, TableColumn,  # noqa: F401
                      Value, create_proof, keygen_pk, keygen_vk, lower)
from . import floor_planner  # noqa: F401
from .floor_planner import V1  # noqa: F401
