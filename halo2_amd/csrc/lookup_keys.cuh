// 256-bit canonical sort keys: what lookup.hip's bitonic network orders and what binary searches over its output compare.
// Shared by lookup.hip (permute_expression_pair) and mock_prover.hip (exact tuple membership).
#pragma once
#include "field.cuh"

namespace h2 {

struct key256 {
    u32 v[8];
};

__device__ __forceinline__ bool key_less(const key256 &a, const key256 &b) {
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
    }
    return false;
}

__device__ __forceinline__ bool key_eq(const key256 &a, const key256 &b) {
    u32 d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d |= a.v[i] ^ b.v[i];
    return d == 0;
}

__device__ __forceinline__ key256 key_load(const u32 *p) {
    const uint4 lo = reinterpret_cast<const uint4 *>(p)[0], hi = reinterpret_cast<const uint4 *>(p)[1];
    return key256{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}

__device__ __forceinline__ void key_store(u32 *p, const key256 &k) {
    reinterpret_cast<uint4 *>(p)[0] = make_uint4(k.v[0], k.v[1], k.v[2], k.v[3]);
    reinterpret_cast<uint4 *>(p)[1] = make_uint4(k.v[4], k.v[5], k.v[6], k.v[7]);
}

// lower bound of `key` in the ascending array s[0..n): first index whose element is not less than key
__device__ __forceinline__ u32 lower_bound(const u32 *__restrict__ s, u32 n, const key256 &key) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (key_less(key_load(s + 8 * (size_t)mid), key)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace h2
