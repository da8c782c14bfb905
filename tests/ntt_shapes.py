"""The default pass plans of the NTT as shapes, and the sizes the GPU sweep runs (a helper: nothing here is collected).

tests/ntt_plans_parent.txt holds the plan of every size under every knob setting; tests/test_ntt_plan.py holds csrc/ntt_plan.h to that
file.  Only the default knobs matter here -- maxr 10, logT 3, no first-pass width, 128 KiB: what the shipped library plans with.  A
pass is told apart by what its kernel is handed: the plan kind (0: a transform alone, 1: the batched column entry points), whether it
is the first and / or the last pass (FIRST is a template parameter, `last` picks the store), its stage count r (a template parameter)
and its runtime tile width logT.  tests/test_ntt_shape_coverage.py proves on the CPU that the sweep lists below reach every such shape
a default plan has up to 2^28, less an explicit list; tests/test_gpu_ntt_shapes.py runs them."""
import os

PLAN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ntt_plans_parent.txt")
DEFAULT_KNOBS = (10, 3, -1, 131072)          # maxr, logT, logT_first, lds
MAX_L = 28                                   # the carry-free kernels are planned up to 2^28 (csrc/ntt_plan.h)

SWEEP_PLAN0 = list(range(0, 23))             # h2_ntt_device / h2_ifft_device, one transform
SWEEP_PLAN1 = list(range(0, 23))             # h2_ntt_batch_device / h2_ifft_batch_device, two columns or more

_plans = None


def _load():
    global _plans
    if _plans is None:
        _plans = {}
        for line in open(PLAN_FILE):
            if line.startswith("#") or not line.strip():
                continue
            f = [int(x) for x in line.split()]
            if tuple(f[2:6]) != DEFAULT_KNOBS:
                continue
            npass, per = f[6], f[7:]
            assert len(per) == 6 * npass, line
            _plans[(f[0], f[1])] = [(per[6 * i], per[6 * i + 1]) for i in range(npass)]
    return _plans


def passes(L, kind):
    """[(r, logT)] of the default plan of a 2^L transform, in pass order; a 2^0 transform launches no pass."""
    return [] if L == 0 else list(_load()[(L, kind)])


def shapes_of(L, kind):
    p = passes(L, kind)
    return {(kind, i == 0, i == len(p) - 1, r, logT) for i, (r, logT) in enumerate(p)}


def shapes(sizes, kind):
    """{(kind, first, last, r, logT)} over the default plans of the given sizes."""
    out = set()
    for L in sizes:
        out |= shapes_of(L, kind)
    return out


def swept_shapes():
    return shapes(SWEEP_PLAN0, 0) | shapes(SWEEP_PLAN1, 1)


def all_shapes(max_l=MAX_L):
    return shapes(range(1, max_l + 1), 0) | shapes(range(1, max_l + 1), 1)
