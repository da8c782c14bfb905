// The bytecode of the expression evaluator, for the two kernels that interpret it -- ev_run (evaluator.hip) and mp_check, the
// MockProver's interpreter with the poison algebra (mock_prover.hip): the opcodes, the stack's shape and its LDS spill / fill, and the
// one validator both entry points put a program through before anything is enqueued.  Node semantics: the head of evaluator.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "field.cuh"

namespace h2 {

enum : u32 { EV_POLY = 1, EV_CONST = 2, EV_LINEAR = 3, EV_ADD = 4, EV_MUL = 5, EV_SCALE = 6, EV_MULADD = 7 };   // = H2_EV_*
constexpr int kEvalDepth = 8;      // stack slots below the register-resident top
constexpr int kEvalThreads = 256;

// stack level `level` of this lane, word-major in LDS so that a wave's accesses are conflict-free
__device__ __forceinline__ void ev_spill(u32 *lds, int level, const fe &v) {
#pragma unroll
    for (int w = 0; w < 8; ++w) lds[(level * 8 + w) * kEvalThreads + threadIdx.x] = v.v[w];
}
__device__ __forceinline__ fe ev_fill(const u32 *lds, int level) {
    fe v;
#pragma unroll
    for (int w = 0; w < 8; ++w) v.v[w] = lds[(level * 8 + w) * kEvalThreads + threadIdx.x];
    return v;
}

// Whether program[begin, end) may run over vectors of `len` elements in `basis` (0 coefficient, 1 Lagrange, 2 extended Lagrange):
// operands in range, stack discipline, exactly one value left, rotations and products only where the reference allows them.
// has_linear: set to whether the program has a LINEAR node; null: a LINEAR node is refused.
inline bool ev_program_ok(const uint32_t *program, size_t begin, size_t end, size_t n_consts, const void *const *d_polys, size_t n_polys,
                          size_t len, int basis, bool *has_linear) {
    if (begin >= end) return false;
    if (has_linear) *has_linear = false;
    int depth = 0, max_depth = 0;
    for (size_t pc = begin; pc < end; ++pc) {
        const uint32_t op = program[pc] & 0xFFu, arg = program[pc] >> 8;
        switch (op) {
            case EV_POLY: {
                if (arg >= n_polys || pc + 1 >= end || !d_polys[arg]) return false;
                const long long shift = (int)program[++pc];
                // |shift| == len is the identity; beyond it the reference panics (poly.rs:251, :256: assert!(k <= self.len()))
                if (shift < -(long long)len || shift > (long long)len) return false;
                if (basis == 0 && shift != 0) return false;            // "Can't rotate polynomials in the standard basis" (:519)
                ++depth;
                break;
            }
            case EV_LINEAR:
                if (!has_linear) return false;
                *has_linear = true;
                [[fallthrough]];
            case EV_CONST:
                if (arg >= n_consts) return false;
                ++depth;
                break;
            case EV_SCALE:
                if (arg >= n_consts || depth < 1) return false;
                break;
            case EV_MUL:
                // Mul exists for Ast<_, _, LagrangeCoeff> and Ast<_, _, ExtendedLagrangeCoeff> (evaluator.rs:370-418)
                if (basis == 0) return false;
                [[fallthrough]];
            case EV_ADD:
                if (depth < 2) return false;
                --depth;
                break;
            case EV_MULADD:
                if (arg >= n_consts || depth < 2) return false;
                --depth;
                break;
            default:
                return false;
        }
        if (depth > max_depth) max_depth = depth;
    }
    return depth == 1 && max_depth <= kEvalDepth + 1;
}

}  // namespace h2
