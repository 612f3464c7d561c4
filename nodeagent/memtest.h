// HBM data-integrity kernels for the MI355X node agent (included from
// agent.hip, and from mfmasweep.h for mt_mix64): pattern fill, verify, and
// fused verify-and-invert.
//
// Pattern (normative — tests/test_nodeagent_memtest.py carries an
// independent numpy copy). The region is addressed in 16-byte vectors; v is
// the vector index from the region start, arithmetic mod 2^64:
//
//   mix64(x): x ^= x>>30; x *= 0xBF58476D1CE4E5B9; x ^= x>>27;
//             x *= 0x94D049BB133111EB; x ^= x>>31
//   h  = mix64(v + seed * 0x9E3779B97F4A7C15)
//   lo = h                         (bytes 0..7)
//   hi = ~((h << 32) | (h >> 32))  (bytes 8..15)
//   invert stores ~lo, ~hi
//
// mix64 is a bijection, so no two vectors of a region share a `lo` and an
// aliased address line reads back as a mismatch; the inverted pass drives
// every cell to both 0 and 1; one hash per 16 B keeps the kernels
// bandwidth-bound.
//
// Access shape is the copy sweep's winner (profiles/
// hbm_copy_variant_sweep_mi355x.txt): each workgroup owns ONE contiguous
// 64 KiB tile, 16-byte nontemporal accesses, four independent vectors in
// flight per thread; the last, partial tile takes a bounds-checked loop. The
// grid is sized to the region (one workgroup per tile).

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

typedef unsigned long long mt_u64;
typedef mt_u64 mt_vec __attribute__((ext_vector_type(2)));  // one 16-byte vector

#define MT_BLOCK 1024
#define MT_UNROLL 4
#define MT_TILE (MT_BLOCK * MT_UNROLL)  // vectors per workgroup

enum { MT_FILL = 0, MT_VERIFY = 1, MT_VERIFY_FLIP = 2 };

// device-side accumulator: {bad 64-bit words, min bad byte offset, OR of got^want}
struct mt_accum {
    mt_u64 bad_words, first_bad_offset, xor_mask;
};

__device__ __host__ inline mt_u64 mt_mix64(mt_u64 x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}

// `base` = seed * 0x9E3779B97F4A7C15 (hoisted to the host); `inv` = 0 or ~0.
__device__ __host__ inline mt_vec mt_pattern(mt_u64 v, mt_u64 base, mt_u64 inv) {
    mt_u64 h = mt_mix64(v + base);
    mt_vec w;
    w.x = h ^ inv;
    w.y = ~((h << 32) | (h >> 32)) ^ inv;
    return w;
}

// Per-thread mismatch state lives in registers; the global accumulator is
// touched after the thread's last vector only (see mt_commit).
struct mt_local {
    mt_u64 bad, first, x;
};

__device__ inline void mt_compare(mt_vec got, mt_vec want, mt_u64 v, mt_local& m) {
    mt_u64 dl = got.x ^ want.x, dh = got.y ^ want.y;
    if (dl | dh) {
        m.bad += (dl != 0) + (dh != 0);
        m.x |= dl | dh;
        mt_u64 off = v * 16 + (dl ? 0 : 8);
        if (off < m.first) m.first = off;
    }
}

// Wave-level reduction, then at most one lane per wave issues the three
// 64-bit atomics — and only if the wave saw a mismatch, so a clean region
// issues none and a fully corrupt one issues 3 per wave, not 3 per word.
__device__ inline void mt_commit(mt_local m, mt_accum* acc) {
    if (!__any(m.bad != 0)) return;  // wave-uniform
    for (int o = 32; o > 0; o >>= 1) {
        m.bad += __shfl_xor(m.bad, o);
        mt_u64 f = __shfl_xor(m.first, o);
        if (f < m.first) m.first = f;
        m.x |= __shfl_xor(m.x, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&acc->bad_words, m.bad);
        atomicMin(&acc->first_bad_offset, m.first);
        atomicOr(&acc->xor_mask, m.x);
    }
}

// p: first vector of this launch; n: vectors in this launch; v0: index of
// p[0] within the whole region (pattern index and reported offsets are
// region-relative, so a region may be spread over several launches/chunks).
// MT_VERIFY_FLIP stores the complement of the EXPECTED value, not of what it
// read, so one bad read cannot poison the next pass.
template <int MODE>
__global__ void __launch_bounds__(MT_BLOCK)
memtest_kernel(mt_vec* p, size_t n, mt_u64 v0, mt_u64 base, mt_u64 inv, mt_accum* acc) {
    size_t i0 = (size_t)blockIdx.x * MT_TILE + threadIdx.x;
    mt_local m = {0, ~0ULL, 0};
    if (((size_t)blockIdx.x + 1) * MT_TILE <= n) {
        // full tile: no bounds checks, MT_UNROLL independent vectors in flight
        if (MODE == MT_FILL) {
#pragma unroll
            for (int k = 0; k < MT_UNROLL; ++k) {
                size_t i = i0 + (size_t)k * MT_BLOCK;
                __builtin_nontemporal_store(mt_pattern(v0 + i, base, inv), &p[i]);
            }
        } else {
            mt_vec got[MT_UNROLL];
#pragma unroll
            for (int k = 0; k < MT_UNROLL; ++k)
                got[k] = __builtin_nontemporal_load(&p[i0 + (size_t)k * MT_BLOCK]);
#pragma unroll
            for (int k = 0; k < MT_UNROLL; ++k) {
                size_t i = i0 + (size_t)k * MT_BLOCK;
                mt_vec want = mt_pattern(v0 + i, base, inv);
                mt_compare(got[k], want, v0 + i, m);
                if (MODE == MT_VERIFY_FLIP) {
                    mt_vec flipped = {~want.x, ~want.y};
                    __builtin_nontemporal_store(flipped, &p[i]);
                }
            }
        }
    } else {
        // tail tile
        for (size_t i = i0; i < n; i += MT_BLOCK) {
            mt_vec want = mt_pattern(v0 + i, base, inv);
            if (MODE == MT_FILL) {
                __builtin_nontemporal_store(want, &p[i]);
            } else {
                mt_compare(__builtin_nontemporal_load(&p[i]), want, v0 + i, m);
                if (MODE == MT_VERIFY_FLIP) {
                    mt_vec flipped = {~want.x, ~want.y};
                    __builtin_nontemporal_store(flipped, &p[i]);
                }
            }
        }
    }
    if (MODE != MT_FILL) mt_commit(m, acc);
}
