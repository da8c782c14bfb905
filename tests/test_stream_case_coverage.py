"""Every entry point that takes a `void *stream` has a stream-order case, proved on the CPU from the header: the table of
tests/stream_cases.py has exactly the prototypes of include/halo2_mi355x.h with a `void *stream` parameter, only the four that cannot
run in one process on one stream are excluded, both seeds of every case (and their element-wise mixture) are valid input of the same
shape, the oracle's bytes have the size the case announces, and every shape is what the plan replicas say it is: the smallest that
takes more than one launch or leaves the caller's stream.  tests/test_gpu_stream_order.py runs the table; it is read with `ast`
here, never imported."""
import ast
import os

import pytest

import call_sequences as cs
import commit_plans as cp
import generic_plans as gp
import ntt_shapes as ns
import scan_sort_cases as ssc
import stream_cases as sc

GPU_TEST_FILE = os.path.join(sc.ROOT, "tests", "test_gpu_stream_order.py")
CASE_IDS = [case.name for case in sc.ALL_CASES]


def test_the_parser_finds_the_prototypes_it_should():
    protos = sc.prototypes_with_stream()
    assert {"h2_msm_device", "h2_commit_batch_device", "h2_open_device_host_s", "h2_evaluate_device", "h2_ecc_fixed_tables_device",
            "h2_short_range_check_trace_device", "h2_msm_last_path", "h2_commit_last_plan"} <= protos
    # host-memory entry points and the ones without a stream are not in the set
    assert not protos & {"h2_msm", "h2_commit", "h2_ntt", "h2_open", "h2_ipa_rounds", "h2_bases_register_device", "h2_trim", "h2_debug_counters",
                         "h2_commit_batch_multi", "h2_msm_split_multi", "h2_points_sum"}
    assert len(protos) >= 63


def test_every_prototype_with_a_stream_has_a_case():
    protos = sc.prototypes_with_stream()
    missing, stale = protos - set(sc.CASES), set(sc.CASES) - protos
    assert not missing, f"entry points that take `void *stream` and have no case in tests/stream_cases.py: {sorted(missing)}"
    assert not stale, f"tests/stream_cases.py names entry points the header does not declare with `void *stream`: {sorted(stale)}"


def test_a_prototype_added_to_the_header_is_missed(tmp_path):
    header = tmp_path / "halo2_mi355x.h"
    header.write_text(open(sc.HEADER).read() + "\nint h2_brand_new_device(const void *d_a, size_t n,\n                        void *stream);\n")
    assert sc.prototypes_with_stream(str(header)) - set(sc.CASES) == {"h2_brand_new_device"}


def test_only_the_four_named_entry_points_are_excluded():
    excluded = {name for name, case in sc.CASES.items() if isinstance(case, sc.Excluded)}
    assert excluded == sc.MAY_BE_EXCLUDED == {"h2_msm_last_path", "h2_commit_last_plan", "h2_msm_split_rccl_device", "h2_commit_split_rccl_device"}
    assert all(sc.CASES[name].strip() and "\n" not in sc.CASES[name] for name in excluded)
    for entry, value in sc.CASES.items():
        assert all(case.entry == entry for case in sc.cases_of(entry)), entry
        assert isinstance(value, sc.Excluded) or sc.cases_of(entry)


def test_the_entry_points_without_a_device_input_are_the_three_the_header_shows():
    """x, the challenges and the base are host pointers, the registered table is a set-up object: nothing of the call lies in a buffer the
    caller's stream could still be writing"""
    assert {case.entry for case in sc.ALL_CASES if not case.inputs(sc.REAL)} == sc.NO_DEVICE_INPUT


@pytest.mark.parametrize("name", CASE_IDS)
def test_both_seeds_are_valid_input_of_one_shape_and_so_is_their_mixture(name):
    case = sc.BY_NAME[name]
    real, decoy, third = (case.inputs(seed) for seed in sc.SEEDS)
    assert list(real) == list(decoy) == list(third)
    for key in real:
        for other in (decoy[key], third[key]):
            assert real[key].shape == other.shape and real[key].dtype == other.dtype, key
            assert real[key].tobytes() != other.tobytes(), f"{key}: two seeds give the same bytes"
        assert decoy[key].tobytes() != third[key].tobytes(), key
    for arrays in (real, decoy, third, {key: sc.mixture(real[key], decoy[key]) for key in real},
                   {key: sc.mixture(decoy[key], real[key]) for key in real}):
        case.valid(arrays)
    # in-place outputs name an input and fit into it
    for out, spec in case.outputs().items():
        if not isinstance(spec, int):
            kind, source, size = spec
            assert kind == "in" and 0 < size <= real[source].nbytes, out
        else:
            assert spec > 0 and out not in real, out


@pytest.mark.parametrize("name", CASE_IDS)
def test_the_oracle_bytes_have_the_announced_size(name):
    case = sc.BY_NAME[name]
    want = case.expected(sc.REAL)
    assert isinstance(want, bytes) and len(want) == sum(size for _, size in case.output_bytes()) + case.host_bytes
    assert case.host_bytes or case.outputs(), "a case compares something"
    if case.mode_c:                                               # the second stream's data has an answer of its own
        assert case.expected(sc.THIRD) != want and len(case.expected(sc.THIRD)) == len(want)


def test_the_opening_cases_take_the_small_k_of_the_call_sequences():
    """(that expected(REAL) is call_sequences.opening_proof_wanted's proof is asserted on the GPU: its Params need a device)"""
    for entry in ("h2_open_device", "h2_open_device_host_s"):
        (case,) = sc.cases_of(entry)
        assert case.shape == cs.IPA_KS[0]
        assert len(case.expected(sc.REAL)) == sc.open_proof_length()
    assert sc.cases_of("h2_ipa_rounds_device")[0].shape == cs.IPA_KS[0]


# ---- the shape claims, against the replicas of the plans --------------------------------------------------------------------------------------
def test_the_scans_take_two_tiles_and_the_carry_level():
    n = ssc.K_TILE + 1
    assert n == 2049 == sc.POLY_N == sc.LOOKUP_N == sc.SEL_N == sc.CHECK_N
    assert ssc.scan_geometry(n)[0] == 2 and ssc.scan_geometry(n - 1)[0] == 1                    # aggregate, carry, final
    for entry in ("h2_kate_division_device", "h2_grand_product_device", "h2_batch_invert_device", "h2_assigned_to_field_device", "h2_scale_add_device",
                  "h2_powers_device", "h2_eval_polynomial_device", "h2_inner_product_device"):
        assert sc.cases_of(entry)[0].shape == n, entry
    # the reductions: more than one workgroup, so partial sums and a second launch
    geometry = ssc.reduce_geometry(n)
    assert geometry["eval"][0] > 1 and geometry["inner"][0] > 1 and ssc.reduce_geometry(ssc.K_PT)["inner"][0] == 1


def test_the_sort_takes_one_global_pass_and_the_permutation_two_scan_blocks():
    n = sc.LOOKUP_N
    kinds = [step[0] for step in ssc.sort_schedule(n)]
    assert kinds.count("global") + kinds.count("global2") == 1 and kinds.count("tile") == 2
    assert all(step[0] == "tile" for step in ssc.sort_schedule(n - 1))                            # 2048 keys: the tile kernel alone
    assert ssc.permute_geometry(n)[0] > 1
    assert sc.cases_of("h2_sort_device")[0].shape == sc.cases_of("h2_permute_expression_pair_device")[0].shape == n


def test_the_transforms_are_the_smallest_two_pass_sizes_of_the_default_plans():
    for L, kind in ((sc.NTT_LOG, 0), (sc.NTT_BATCH_LOG, 1)):
        assert len(ns.passes(L, kind)) == 2 and len(ns.passes(L - 1, kind)) == 1
    for entry in ("h2_ntt_device", "h2_ifft_device", "h2_extended_to_coeff_device", "h2_divide_by_vanishing_poly_device"):
        assert sc.cases_of(entry)[0].shape == sc.NTT_LOG
    assert sc.cases_of("h2_coeff_to_extended_device")[0].shape == (sc.NTT_LOG - 2, sc.NTT_LOG)
    for entry in ("h2_ntt_batch_device", "h2_ifft_batch_device"):
        assert sc.cases_of(entry)[0].shape == (sc.NTT_BATCH_LOG, 2)
    # ntt_batch (csrc/ntt.hip): min(3, count) internal streams, the batched plan from two of them on.  No host replica and no counter
    # tells which stream or plan a column took, so the two lines that decide it are pinned as text: if they are rewritten, this fails
    # and whoever rewrote them looks at NTT_BATCH_COLUMNS again (a false alarm on a reformat is the price)
    text = open(os.path.join(sc.ROOT, "halo2_amd", "csrc", "ntt.hip")).read()
    assert "const size_t want = std::min<size_t>(3, count);" in text and "J.plan = want > 1 ? 1 : 0;" in text


def test_the_generic_multiexp_sizes_are_the_three_forms_of_the_dispatch():
    assert set(sc.MSM_SIZES) == set(cs.MSM_PATHS) | {sc.GROUPED} and sc.GROUPED == (1 << 18) + 1
    assert {n: path for n, path in sc.MSM_SIZES.items() if n in cs.MSM_PATHS} == cs.MSM_PATHS
    assert sc.MSM_SIZES[sc.GROUPED] == 4 and "#define H2_MSM_PATH_GROUPED_LATENCY 4" in open(sc.HEADER).read()      # never the one-group form on `stream`
    # the header's thresholds: one pass below 65536 scalars, two passes up to 2^18, the grouped form from 2^18 + 1 up to the replica's limit
    header = open(sc.HEADER).read()
    assert "one-pass counting sort (below 65536 scalars)" in header and "(65536 .. 2^18 scalars;" in header and "(2^18 + 1 .. 5120255 scalars)" in header
    assert 300 < 65536 <= 70000 <= 1 << 18 < sc.GROUPED <= gp.LATENCY_MAX == 5120255
    groups = gp.layout(sc.GROUPED, gp.LATENCY_SLICES)
    assert groups is not None and len(groups) == 3                                                # three groups on the library's own streams
    assert [cp.choose_c(n, False) for n in sc.MSM_SIZES] == [10, 13, 16]
    assert [case.shape for case in sc.cases_of("h2_msm_device")] == [300, 70000, sc.GROUPED]
    assert sc.cases_of("h2_msm_batch_device")[0].shape == (2049, 300)


def test_the_batched_commits_take_the_two_forms_at_their_smallest_column_counts():
    lanes = cp.LANES_MI355X
    batch = lambda points, count: cp.expected(cp.Case(points, 0, "batch", points, True, K=count), lanes)
    points, count = sc.ALTERNATING
    r = batch(points, count)
    assert (r["caller"], r["caller_count"]) == (cp.BATCH_COLUMNS, 2)                              # two groups alternate over two internal streams
    assert batch(points, count - 1)["caller_count"] == 1                                          # a single group stays on the caller's stream
    points, count = sc.SPREAD
    r = batch(points, count)
    assert (r["caller"], r["caller_count"]) == (cp.BATCH_FORK, 3) and min(3, count) == 3 and min(3, count - 1) == 2       # three streams from three columns on
    assert [case.shape for case in sc.cases_of("h2_commit_batch_device")] == [sc.ALTERNATING, sc.SPREAD]


def test_the_other_registered_commits():
    lanes = cp.LANES_MI355X
    n = sc.PAIR_TABLE
    assert cp.pair_supported(n) and not cp.pair_supported(n - 1)
    assert cp.expected(cp.Case(n, 0, "pair", n, False), lanes)["caller"] == cp.PAIR_SUBDIGIT
    assert sc.cases_of("h2_commit_pair_device")[0].shape == n
    assert cp.choose_c(sc.COMMIT_TABLE, True) == 16 == cp.choose_c(1 << sc.COLLAPSED[0], True)   # the read-out of the collapsed generators needs 16-bit windows
    assert cp.choose_c((1 << (sc.COLLAPSED[0] - 1)), True) != 16
    first, count = sc.cases_of("h2_commit_range_device")[0].shape
    assert 0 < first and first + count == sc.COMMIT_TABLE
    assert "blind" in sc.cases_of("h2_commit_device")[0].inputs(sc.REAL)


def test_the_remaining_shapes():
    assert sc.LAGRANGE_K == 9 and sc.cases_of("h2_lagrange_basis_device")[0].shape == 9
    text = open(os.path.join(sc.ROOT, "halo2_amd", "csrc", "ecfft.hip")).read()
    # the three stage kernels meet first at k = 9; ecfft.hip has no host-only plan to replicate, so the two conditions are pinned as text
    # (a rewrite of them fails here and sends its author to LAGRANGE_K; a reformat is a false alarm)
    assert "if (t + 7 <= k && k >= 9)" in text and "else if (t >= 2)" in text
    assert sc.LANES == 65 == cs.TRACE_COUNTS[1] and sc.LANES > 64                                 # two workgroups of 64 lanes
    for entry in ("h2_sinsemilla_trace_device", "h2_sinsemilla_trace_from_device", "h2_ecc_mul_trace_device", "h2_ecc_mul_fixed_trace_device",
                  "h2_poseidon_trace_device", "h2_range_check_trace_device", "h2_short_range_check_trace_device"):
        shape = sc.cases_of(entry)[0].shape
        assert (shape if isinstance(shape, int) else shape[0]) == 65, entry
    assert sc.cases_of("h2_ecc_fixed_tables_device")[0].shape == ("generator", 85) == tuple(cs.BY_NAME["fixed-base-tables"].shapes[cs.SMALL])
    assert sc.cases_of("h2_generator_collapse_device")[0].shape == cs.IPA_KS[1]
    assert sc.cases_of("h2_ipa_round_scalars_device")[0].shape == cs.ROUND_SCALARS[1]
    assert sc.cases_of("h2_ipa_s_combine_device")[0].shape == cs.S_COMBINE[1]
    assert sc.cases_of("h2_evaluate_device")[0].shape == cs.EVAL_SHAPES[1]


# ---- the GPU file ---------------------------------------------------------------------------------------------------------------------------
def test_the_gpu_file_is_marked_gpu_as_a_whole_and_runs_the_table():
    tree = ast.parse(open(GPU_TEST_FILE).read())
    marks = [node for node in tree.body if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "pytestmark" for t in node.targets)]
    assert len(marks) == 1 and ast.unparse(marks[0].value) == "pytest.mark.gpu"
    funcs = {node.name: ast.unparse(node) for node in tree.body if isinstance(node, ast.FunctionDef)}
    for name, cases in (("test_mode_a_late_producer_early_overwrite", "ALL_CASES"), ("test_mode_b_a_misplaced_stream_is_seen", "ALL_CASES"),
                        ("test_mode_c_two_streams_cold_shared_caches", "MODE_C")):
        assert name in funcs and f"sc.{cases}" in funcs[name], name


def test_mode_c_covers_the_shared_caches_the_issue_names():
    entries = {case.entry for case in sc.MODE_C}
    assert {"h2_ntt_device", "h2_ifft_device", "h2_ntt_batch_device", "h2_ifft_batch_device", "h2_coeff_to_extended_device", "h2_extended_to_coeff_device",
            "h2_evaluate_device", "h2_lagrange_basis_device", "h2_sinsemilla_hash_device", "h2_sinsemilla_merkle_layer_device", "h2_sinsemilla_trace_device",
            "h2_sinsemilla_commit_device", "h2_sinsemilla_hash_from_device", "h2_sinsemilla_trace_from_device", "h2_kate_division_device",
            "h2_grand_product_device", "h2_batch_invert_device", "h2_assigned_to_field_device", "h2_sort_device",
            "h2_permute_expression_pair_device"} <= entries
    assert not entries & sc.NO_DEVICE_INPUT                       # two streams need two data sets
