"""Which test calls each entry point of the C ABI with H2_FORM_CANONICAL (a helper: nothing here is collected).

Every prototype of include/halo2_mi355x.h whose parameter list holds `int form` is a key of CASES.  Its value is the name of the test
function of tests/test_gpu_canonical_form.py that calls it with canonical data and compares values with the oracle, or an Excluded with
the one-line reason why one GPU cannot reach it.  tests/test_form_coverage.py holds the table to the header on the CPU: a prototype added
later without a case fails there.  WRAPPERS names the halo2_amd function a test may call instead of the symbol itself."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "halo2_mi355x.h")
GPU_TEST_FILE = os.path.join(ROOT, "tests", "test_gpu_canonical_form.py")


class Excluded(str):
    """The reason an entry point has no canonical case."""


def prototypes_with_form(header=HEADER):
    """Names of the functions declared in the header whose parameter list holds `int form`."""
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = re.findall(r"\bint\s+(h2_\w+)\s*\(([^()]*)\)\s*;", text)
    return {name for name, params in found if re.search(r"\bint\s+form\b", params)}


# the only entry points that may be left out: several devices, or RCCL between processes
MAY_BE_EXCLUDED = {"h2_commit_batch_multi", "h2_msm_split_multi", "h2_msm_split_rccl_device", "h2_commit_split_rccl_device"}

CASES = {
    # ---- a. registered commits, b. the blind-base cache
    "h2_bases_register": "test_registered_commits",
    "h2_bases_register_device": "test_registration_from_device_memory_and_with_a_chosen_width",
    "h2_bases_register_ex": "test_registration_from_device_memory_and_with_a_chosen_width",
    "h2_bases_set_blind_base": "test_registered_commits",
    "h2_commit": "test_registered_commits",
    "h2_commit_device": "test_registered_commits",
    "h2_commit_batch_device": "test_registered_commits",
    "h2_commit_range_device": "test_registered_commits",
    "h2_points_sum_device": "test_registered_commits",
    "h2_commit_pair_device": "test_paired_commit",
    # ---- c. generic multiexp
    "h2_msm": "test_generic_multiexp",
    "h2_msm_device": "test_generic_multiexp",
    "h2_msm_batch_device": "test_generic_multiexp_batch",
    # ---- d. poly.hip
    "h2_eval_polynomial": "test_eval_polynomial_and_inner_product",
    "h2_eval_polynomial_device": "test_eval_polynomial_and_inner_product",
    "h2_inner_product": "test_eval_polynomial_and_inner_product",
    "h2_inner_product_device": "test_eval_polynomial_and_inner_product",
    "h2_kate_division": "test_kate_division_powers_scale_add",
    "h2_kate_division_device": "test_kate_division_powers_scale_add",
    "h2_powers": "test_kate_division_powers_scale_add",
    "h2_powers_device": "test_kate_division_powers_scale_add",
    "h2_scale_add": "test_kate_division_powers_scale_add",
    "h2_scale_add_device": "test_kate_division_powers_scale_add",
    "h2_batch_invert": "test_batch_invert",
    "h2_batch_invert_device": "test_batch_invert",
    "h2_grand_product": "test_grand_product",
    "h2_grand_product_device": "test_grand_product",
    "h2_assigned_to_field": "test_assigned_to_field",
    "h2_assigned_to_field_device": "test_assigned_to_field",
    # ---- e. NTT family
    "h2_ntt": "test_ntt_and_ifft",
    "h2_ntt_device": "test_ntt_and_ifft",
    "h2_ifft": "test_ntt_and_ifft",
    "h2_ifft_device": "test_ntt_and_ifft",
    "h2_ntt_batch_device": "test_batched_ntt_and_ifft",
    "h2_ifft_batch_device": "test_batched_ntt_and_ifft",
    "h2_coeff_to_extended": "test_extended_domain_transforms",
    "h2_coeff_to_extended_device": "test_extended_domain_transforms",
    "h2_extended_to_coeff": "test_extended_domain_transforms",
    "h2_extended_to_coeff_device": "test_extended_domain_transforms",
    "h2_divide_by_vanishing_poly": "test_extended_domain_transforms",
    "h2_divide_by_vanishing_poly_device": "test_extended_domain_transforms",
    # ---- f. IPA pieces
    "h2_fold_scalars": "test_fold_scalars",
    "h2_fold_scalars_device": "test_fold_scalars",
    "h2_generator_collapse": "test_generator_collapse",
    "h2_generator_collapse_device": "test_generator_collapse",
    "h2_ipa_round_scalars_device": "test_ipa_round_scalars",
    "h2_ipa_s_combine": "test_ipa_s_combine",
    "h2_ipa_s_combine_device": "test_ipa_s_combine",
    "h2_ipa_collapsed_generators_device": "test_collapsed_generators",
    # ---- g. points and lookups
    "h2_lagrange_basis": "test_lagrange_basis",
    "h2_lagrange_basis_device": "test_lagrange_basis",
    "h2_points_compress": "test_points_compress_and_decompress",
    "h2_points_compress_device": "test_points_compress_and_decompress",
    "h2_points_decompress": "test_points_compress_and_decompress",
    "h2_points_decompress_device": "test_points_compress_and_decompress",
    "h2_hash_to_curve": "test_hash_to_curve",
    "h2_hash_to_curve_device": "test_hash_to_curve",
    "h2_sort_device": "test_sort",
    "h2_permute_expression_pair_device": "test_permute_expression_pair",
    "h2_lookup_check_device": "test_mock_prover_lookup_check",
    "h2_permutation_check_device": "test_mock_prover_permutation_check",
    # ---- out of reach on one GPU
    "h2_commit_batch_multi": Excluded("spreads columns over several devices from one process"),
    "h2_msm_split_multi": Excluded("cuts one multiexp into ranges over several devices"),
    "h2_msm_split_rccl_device": Excluded("one process per GPU with an RCCL exchange between them"),
    "h2_commit_split_rccl_device": Excluded("one process per GPU with an RCCL exchange between them"),
}

# entry point -> the halo2_amd function that calls it (host arrays reach the plain symbol, device tensors the _device one)
WRAPPERS = {
    "h2_msm": "best_multiexp", "h2_msm_device": "best_multiexp", "h2_msm_batch_device": "best_multiexp_batch",
    "h2_ntt": "best_fft", "h2_ntt_device": "best_fft", "h2_ntt_batch_device": "best_fft_batch",
    "h2_eval_polynomial": "eval_polynomial", "h2_eval_polynomial_device": "eval_polynomial",
    "h2_inner_product": "compute_inner_product", "h2_inner_product_device": "compute_inner_product",
    "h2_kate_division": "kate_division", "h2_kate_division_device": "kate_division",
    "h2_powers": "powers", "h2_powers_device": "powers",
    "h2_scale_add": "scale_add", "h2_scale_add_device": "scale_add",
    "h2_batch_invert": "batch_invert", "h2_batch_invert_device": "batch_invert",
    "h2_grand_product": "grand_product", "h2_grand_product_device": "grand_product",
    "h2_assigned_to_field": "assigned_to_field", "h2_assigned_to_field_device": "assigned_to_field",
    "h2_fold_scalars": "fold_scalars", "h2_fold_scalars_device": "fold_scalars",
    "h2_generator_collapse": "parallel_generator_collapse", "h2_generator_collapse_device": "parallel_generator_collapse",
    "h2_ipa_round_scalars_device": "ipa_round_scalars",
    "h2_ipa_s_combine": "ipa_s_combine", "h2_ipa_s_combine_device": "ipa_s_combine",
    "h2_sort_device": "sort_field", "h2_permute_expression_pair_device": "permute_expression_pair",
    "h2_lagrange_basis": "lagrange_basis", "h2_points_compress": "points_to_bytes", "h2_points_decompress": "points_from_bytes",
    "h2_hash_to_curve": "hash_to_curve",
}
