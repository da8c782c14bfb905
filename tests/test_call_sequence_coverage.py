"""No unit that keeps device memory between calls is without a call-sequence probe, proved on the CPU from the sources: every
`*_release_workspaces` that h2_trim (csrc/api.hip) calls, and every translation unit of csrc that declares a StreamContexts<...> or owns
a DevBuf, is named by a probe of tests/call_sequences.py; each probe has a small and a large shape that differ, except the single-size
ones; and the counter struct of h2_debug_counters is the same in the header, in halo2_amd/_lib.py and in the probes' field list.
tests/test_gpu_call_sequences.py is read with `ast`, never imported."""
import ast
import ctypes as C
import glob
import os
import re

import call_sequences as cs
from halo2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2_amd", "csrc")
GPU_TEST_FILE = os.path.join(ROOT, "tests", "test_gpu_call_sequences.py")
SINGLE_SIZE = {"fixed-base-tables"}                      # the rows of the issue's table with one size


def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _without_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def trim_releases():
    """The `*_release_workspaces` functions h2_trim calls, in order."""
    body = re.search(r'extern "C" int h2_trim\(void\) \{(.*?)\n\}', _source("api.hip"), flags=re.S).group(1)
    return re.findall(r"h2::(\w+_release_workspaces)\(\)", body)


def owning_units():
    """Translation units that declare a StreamContexts<...> instance, a DevBuf (a member, a local or a map of them) or define one of
    h2_trim's release functions."""
    owners = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        text = _without_comments(open(path).read())
        why = []
        if re.search(r"StreamContexts<\w+>\s+\w+\s*;", text):
            why.append("StreamContexts")
        if re.search(r"(?m)^\s*DevBuf\s+&?\w+", text) or re.search(r"std::map<[^;]*\bDevBuf>", text):
            why.append("DevBuf")
        if re.search(r"(?m)^void \w+_release_workspaces\(\)", text):
            why.append("release")
        if why:
            owners[os.path.basename(path)] = why
    return owners


def test_the_scans_find_what_they_should():
    releases, owners = trim_releases(), owning_units()
    assert len(releases) == len(set(releases)) >= 12 and {"msm_release_workspaces", "ntt_release_workspaces", "sinsemilla_commit_release_workspaces"} <= set(releases)
    # every release function h2_trim calls is declared in common.h and defined in exactly one translation unit
    declared = set(re.findall(r"void (\w+_release_workspaces)\(\);", _source("common.h")))
    assert declared == set(releases)
    defined = [name for path in glob.glob(os.path.join(CSRC, "*.hip")) for name in re.findall(r"(?m)^void (\w+_release_workspaces)\(\)", open(path).read())]
    assert sorted(defined) == sorted(releases)
    assert {"msm_launch.hip", "msm_host.hip", "ntt.hip", "poly.hip", "ipa.hip", "verify.hip", "evaluator.hip", "lookup.hip", "mock_prover.hip",
            "sinsemilla.hip", "ecc.hip", "ecc_fixed.hip", "sinsemilla_commit.hip"} <= set(owners)
    assert "DevBuf" in owners["msm_host.hip"] and "DevBuf" in owners["ntt.hip"] and "StreamContexts" in owners["ecc.hip"]
    assert "api.hip" not in owners and "poseidon.hip" not in owners


def test_every_release_of_h2_trim_has_a_probe():
    probed = {r for p in cs.PROBES for r in p.releases}
    missing = set(trim_releases()) - probed
    assert not missing, f"h2_trim releases workspaces no probe of tests/call_sequences.py goes through: {sorted(missing)}"
    stale = probed - set(trim_releases())
    assert not stale, f"tests/call_sequences.py names release functions h2_trim does not call: {sorted(stale)}"


def test_every_unit_with_cached_device_memory_has_a_probe():
    probed = {f for p in cs.PROBES for f in p.files}
    owners = owning_units()
    missing = set(owners) - probed
    assert not missing, f"translation units that keep device memory and have no probe in tests/call_sequences.py: {sorted(missing)}"
    assert all(os.path.exists(os.path.join(CSRC, f)) for f in probed)
    for p in cs.PROBES:                                  # a probe names a unit that owns something, and releases that exist
        assert p.files and p.releases and set(p.files) & set(owners), p.name


def test_small_and_large_differ_except_for_the_single_size_rows():
    assert len({p.name for p in cs.PROBES}) == len(cs.PROBES)
    assert {p.name for p in cs.PROBES if p.single_size} == SINGLE_SIZE
    for p in cs.PROBES:
        assert set(p.shapes) == set(cs.SIZES), p.name
        if p.single_size:
            assert p.shapes[cs.SMALL] == p.shapes[cs.LARGE], p.name
        else:
            assert p.shapes[cs.SMALL] != p.shapes[cs.LARGE], p.name
    # per release function at least one probe with two sizes: the regrowth sequence means something for every unit
    for release in trim_releases():
        assert any(release in p.releases and not p.single_size for p in cs.PROBES), release


def test_the_counter_struct_is_the_same_everywhere():
    header = _without_comments(open(os.path.join(ROOT, "include", "halo2_mi355x.h")).read())
    body = re.search(r"typedef struct h2_debug_counters \{(.*?)\} h2_debug_counters_t;", header, flags=re.S).group(1)
    in_header = re.findall(r"\b(?!uint64_t\b)([a-z_0-9]+)\s*[,;]", body)
    assert tuple(in_header) == cs.COUNTER_FIELDS == tuple(name for name, _ in _lib.DebugCounters._fields_)
    assert all(kind is C.c_uint64 for _, kind in _lib.DebugCounters._fields_)
    assert re.search(r"\bint h2_debug_counters\(h2_debug_counters_t \*out\);", header)
    # every counter but the epoch is incremented somewhere in csrc, and api.hip copies every field out
    api = _source("api.hip")
    assert all(re.search(rf"out->{name}\s*=", api) for name in cs.COUNTER_FIELDS)
    enum = re.search(r"enum DebugCounter \{(.*?)\}", _source("common.h"), flags=re.S).group(1)
    names = [n for n in re.findall(r"DBG_\w+", enum) if n != "DBG_COUNTERS"]
    assert [n[4:].lower() for n in names] == list(cs.COUNTER_FIELDS[1:])
    sources = "".join(_without_comments(open(p).read()) for p in glob.glob(os.path.join(CSRC, "*.hip")) if not p.endswith("api.hip"))
    for n in names:
        assert re.search(rf"debug_count\([^)]*\b{n}\b", sources), n


def test_the_gpu_file_runs_every_probe_and_is_marked_gpu():
    tree = ast.parse(open(GPU_TEST_FILE).read())
    marks = [node for node in tree.body if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "pytestmark" for t in node.targets)]
    assert len(marks) == 1 and ast.unparse(marks[0].value) == "pytest.mark.gpu"
    funcs = {node.name: node for node in tree.body if isinstance(node, ast.FunctionDef)}
    regrowth = funcs["test_regrowth_and_trim"]
    params = [ast.unparse(d) for d in regrowth.decorator_list]
    assert any("cs.PROBES" in d and "parametrize" in d for d in params), params
    assert {"test_host_slice_multiexp_graphs", "test_opening_keeps_and_refills_its_table", "test_twiddle_cache_follows_the_root"} <= set(funcs)
