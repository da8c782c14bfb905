"""The canonical data form has a case for every entry point that takes one, proved on the CPU from the header: the table of
tests/form_cases.py has exactly the prototypes of include/halo2_mi355x.h with an `int form` parameter, each mapped to a test function
of tests/test_gpu_canonical_form.py that exists and whose source names the entry point (or the halo2_amd function that calls it), or
to a reason -- allowed only for the entry points that need several GPUs.  The GPU file is read with `ast`, never imported."""
import ast

import form_cases as fc


def _test_functions():
    tree = ast.parse(open(fc.GPU_TEST_FILE).read())
    return {node.name: node for node in tree.body if isinstance(node, ast.FunctionDef)}


def _names_in(node):
    """Every identifier, attribute name and string constant inside a function (nested functions included)."""
    out = set()
    for sub in ast.walk(node):
        if isinstance(sub, ast.Attribute):
            out.add(sub.attr)
        elif isinstance(sub, ast.Name):
            out.add(sub.id)
        elif isinstance(sub, ast.Constant) and isinstance(sub.value, str):
            out.add(sub.value)
    return out


def test_the_parser_finds_the_prototypes_it_should():
    protos = fc.prototypes_with_form()
    assert {"h2_msm", "h2_commit_batch_device", "h2_ipa_s_combine_device", "h2_hash_to_curve_device", "h2_permutation_check_device"} <= protos
    # entry points without a form, or whose data is Montgomery by contract, are not in the set
    assert not protos & {"h2_points_sum", "h2_evaluate_device", "h2_check_expressions_device", "h2_open", "h2_ipa_rounds_device", "h2_bases_info", "h2_msm_last_path",
                         "h2_commit_last_plan", "h2_debug_counters"}
    assert len(protos) >= 65


def test_every_prototype_with_a_form_has_exactly_one_case():
    protos = fc.prototypes_with_form()
    missing, stale = protos - set(fc.CASES), set(fc.CASES) - protos
    assert not missing, f"entry points that take `int form` and have no canonical case in tests/form_cases.py: {sorted(missing)}"
    assert not stale, f"tests/form_cases.py names entry points the header does not declare with `int form`: {sorted(stale)}"


def test_only_the_multi_device_entry_points_are_excluded():
    excluded = {name for name, case in fc.CASES.items() if isinstance(case, fc.Excluded)}
    assert excluded == fc.MAY_BE_EXCLUDED
    assert all(fc.CASES[name].strip() and "\n" not in fc.CASES[name] for name in excluded)


def test_every_named_test_exists_and_names_its_entry_point():
    funcs = _test_functions()
    for proto, case in sorted(fc.CASES.items()):
        if isinstance(case, fc.Excluded):
            continue
        assert case.startswith("test_") and case in funcs, f"{proto}: tests/test_gpu_canonical_form.py has no function {case}"
        names = _names_in(funcs[case])
        assert proto in names or fc.WRAPPERS.get(proto) in names, f"{case} does not mention {proto} or {fc.WRAPPERS.get(proto)}"
        assert names & {"FORM_CANONICAL", "CAN", "FORMS"}, f"{case} never names the canonical form"


def test_the_forms_the_cases_loop_over_start_with_the_canonical_one():
    tree = ast.parse(open(fc.GPU_TEST_FILE).read())
    assigns = {ast.unparse(node.targets[0]): ast.unparse(node.value) for node in tree.body if isinstance(node, ast.Assign)}
    assert assigns["(CAN, MONT)"] == "(h.FORM_CANONICAL, h.FORM_MONTGOMERY)" and assigns["FORMS"] == "(CAN, MONT)"


def test_the_gpu_file_is_marked_gpu_as_a_whole():
    tree = ast.parse(open(fc.GPU_TEST_FILE).read())
    marks = [node for node in tree.body if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "pytestmark" for t in node.targets)]
    assert len(marks) == 1 and ast.unparse(marks[0].value) == "pytest.mark.gpu"
