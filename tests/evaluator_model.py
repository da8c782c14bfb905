"""The bytecode of `h2_evaluate_device` on Python integers (a helper: nothing here is collected): the documented semantics of the
H2_EV_* opcodes (include/halo2_mi355x.h), one whole vector per stack slot.  tests/test_evaluator_compile.py holds the compiler to it,
tests/test_evaluator_case_coverage.py holds it to oracle/evaluator.py on every case of tests/evaluator_cases.py and reads off what the
cases execute, tests/test_gpu_evaluator_shapes.py holds the kernels to it.

With `advice` and `usable` given it is the bytecode of `h2_check_expressions_device` instead: every slot entry is an integer or POISON,
by the rules the header states for that entry point (dev.rs:104-156)."""
from halo2_amd import evaluator as hev
from halo2_amd.evaluator import COEFF

POISON = None                     # CellValue::Poison / Value::Poison: an advice cell read outside the usable rows, and what it taints
SPILL_LEVELS = 8                  # the kernels keep the top of the stack in registers and the eight slots below it in LDS


class Trace:
    """What a run executed.  ops: {(opcode, values on the stack before the instruction)}; shifts: {signed element shift of a POLY};
    poison_spilled / poison_filled: the spilled stack levels (0 = the bottom) that a value with a Poison entry was written to by a push /
    read from by ADD, MUL or MULADD -- level l is bit l of the MockProver kernel's `pbits`."""

    def __init__(self):
        self.ops, self.shifts, self.poison_spilled, self.poison_filled = set(), set(), set(), set()


def signed(word):
    return word if word < (1 << 31) else word - (1 << 32)


def _scale(x, c, m):
    if x is POISON:
        return 0 if c == 0 else POISON                                  # Poison * 0 = Real(0), dev.rs:144-156
    return x * c % m


def _add(x, y, m):
    return POISON if x is POISON or y is POISON else (x + y) % m        # dev.rs:115-124


def _mul(x, y, m):
    if x is not POISON and y is not POISON:
        return x * y % m
    if (x is not POISON and x == 0) or (y is not POISON and y == 0):    # dev.rs:126-142
        return 0
    return POISON


def interpret(words, consts, polys, basis, n, m, omega, trace=None, advice=None, usable=None):
    """The program's value at every one of the n elements and the deepest the stack got: (values, maximum depth).
    trace: a Trace to fill.  advice (a set of polynomial indices) and usable (rows) switch the poison algebra on: a cell of an advice
    polynomial read at a row >= usable is POISON, and so is every entry of `values` that it taints."""
    poison = advice is not None
    if poison:
        assert basis == hev.LAGRANGE and usable is not None
    tainted = lambda v: poison and any(x is POISON for x in v)
    stack, depth, i = [], 0, 0
    while i < len(words):
        op, arg = words[i] & 0xFF, words[i] >> 8
        i += 1
        before = len(stack)
        if trace is not None:
            trace.ops.add((op, before))
        if op in (hev._POLY, hev._CONST, hev._LINEAR):
            if trace is not None and before > 0 and tainted(stack[-1]):
                trace.poison_spilled.add(before - 1)                    # the old top goes to level `before - 1`
            if op == hev._POLY:
                shift = signed(words[i])
                i += 1
                if trace is not None:
                    trace.shifts.add(shift)
                bad = poison and arg in advice
                stack.append([POISON if bad and (r + shift) % n >= usable else polys[arg][(r + shift) % n] for r in range(n)])
            elif op == hev._CONST:
                stack.append([consts[arg] if (basis != COEFF or r == 0) else 0 for r in range(n)])
            else:
                assert not poison, "h2_check_expressions_device refuses LINEAR"
                if basis == COEFF:
                    stack.append([consts[arg] if r == 1 else 0 for r in range(n)])
                else:
                    w, col = 1, []
                    for _ in range(n):
                        col.append(consts[arg] * w % m)
                        w = w * omega % m
                    stack.append(col)
        elif op == hev._SCALE:
            stack.append([_scale(x, consts[arg], m) for x in stack.pop()])
        elif op in (hev._ADD, hev._MUL, hev._MULADD):
            top, below = stack.pop(), stack.pop()
            if trace is not None and tainted(below):
                trace.poison_filled.add(before - 2)
            if op == hev._ADD:
                stack.append([_add(x, y, m) for x, y in zip(below, top)])
            elif op == hev._MUL:
                stack.append([_mul(x, y, m) for x, y in zip(below, top)])
            else:                                                       # SCALE of the accumulator, then ADD
                stack.append([_add(_scale(x, consts[arg], m), y, m) for x, y in zip(below, top)])
        else:
            raise AssertionError(f"unknown opcode {op}")
        depth = max(depth, len(stack))
    assert len(stack) == 1
    return stack[0], depth
