// One feature row [N, F] moved between its table and a batch buffer in runs of 8 elements per lane: a 16-byte load or store
// on the bf16 side, two on the fp32 side.  Shared by batch_gather.hip and pretrain_gather.hip, which differ only in where
// their rows lie.  Table base and output base are 16-byte aligned, F % 8 == 0 and the output row stride is a multiple of 8
// elements (the entry points refuse anything else), so no vector straddles a row end.
#pragma once
#include "common.h"

namespace feat_move {
constexpr int NT = 256;
constexpr int RUNS = 4;  // 8-element runs per lane: four independent 16-byte loads in flight
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

// the bits of torch's fp32 -> bf16 conversion (c10::detail::round_to_nearest_even): ties to even, a carry out of the
// mantissa moves into the exponent (the largest finite values become inf), NaN becomes the quiet NaN 0x7FC0
__device__ __forceinline__ unsigned bf16_bits(unsigned u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ unsigned pack2(unsigned lo, unsigned hi) { return bf16_bits(lo) | (bf16_bits(hi) << 16); }

// runs [chunk * NT * RUNS, (chunk + 1) * NT * RUNS) of a row of `runs` runs: src / dst point at the row's first vector
template <bool IN32, bool OUT32>
__device__ __forceinline__ void move_row(const u4* src, u4* dst, int64_t runs, int chunk) {
    const int64_t r0 = (int64_t)chunk * (NT * RUNS) + threadIdx.x;
    u4 lo[RUNS], hi[RUNS];
#pragma unroll
    for (int u = 0; u < RUNS; ++u) {
        const int64_t r = r0 + u * NT;
        if (r < runs) {
            if (IN32) {
                lo[u] = src[2 * r];
                hi[u] = src[2 * r + 1];
            } else {
                lo[u] = src[r];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < RUNS; ++u) {
        const int64_t r = r0 + u * NT;
        if (r >= runs) continue;
        if (IN32 == OUT32) {
            if (IN32) {
                dst[2 * r] = lo[u];
                dst[2 * r + 1] = hi[u];
            } else {
                dst[r] = lo[u];
            }
        } else if (IN32) {  // eight fp32 -> eight bf16
            u4 o;
            o.x = pack2(lo[u].x, lo[u].y);
            o.y = pack2(lo[u].z, lo[u].w);
            o.z = pack2(hi[u].x, hi[u].y);
            o.w = pack2(hi[u].z, hi[u].w);
            dst[r] = o;
        } else {  // eight bf16 -> eight fp32: bits << 16
            const u4 v = lo[u];
            dst[2 * r] = (u4){v.x << 16, v.x & 0xffff0000u, v.y << 16, v.y & 0xffff0000u};
            dst[2 * r + 1] = (u4){v.z << 16, v.z & 0xffff0000u, v.w << 16, v.w & 0xffff0000u};
        }
    }
}

// the four type pairs behind two run-time flags
__device__ __forceinline__ void move_row_any(int in32, int out32, const void* src, void* dst, int64_t runs, int chunk) {
    const u4* s = reinterpret_cast<const u4*>(src);
    u4* d = reinterpret_cast<u4*>(dst);
    if (in32) {
        if (out32) move_row<true, true>(s, d, runs, chunk);
        else move_row<true, false>(s, d, runs, chunk);
    } else {
        if (out32) move_row<false, true>(s, d, runs, chunk);
        else move_row<false, false>(s, d, runs, chunk);
    }
}
}  // namespace feat_move
