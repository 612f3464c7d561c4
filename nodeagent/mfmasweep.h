// Chip-wide matrix-core sweep for the MI355X node agent (included from
// agent.hip; operand packing and MFMA calls are mfma_frag.h's bf16 and fp8
// 16x16x32 traits and, for the MX sweep, its unit-scale 16x16x128 trait).
//
// The single-wave MFMA checks in agent.hip run on one SIMD of one CU. This
// kernel puts one wave on every SIMD of every CU, has each run a long MFMA
// chain on its own data, and leaves one record per wave: a checksum of every
// product it computed, the physical unit it ran on, and two clock deltas.
// The host recomputes each wave's checksum exactly, so a wrong wave is
// attributed to (XCC, SE, SH, CU, SIMD).
//
// Operands (normative — tests/test_nodeagent_mfmasweep.py carries an
// independent numpy copy); arithmetic mod 2^64, G = 0x9E3779B97F4A7C15,
// mix64 = mt_mix64 of memtest.h. For global wave w = blockIdx.x*4 +
// (threadIdx.x>>6), matrix m (0 = A, 1 = B), fragment t in 0..7, r in 0..15
// (row of A / column of B) and k in 0..31:
//
//   idx = (((w*2 + m)*8 + t)*16 + r)*32 + k
//   e   = mix64(seed*G + idx)
//   A   = ((e >> 40) % 7) - 3          B = ((e >> 40) % 5) - 2
//
// Per-lane layout as in the single-wave tile checks (A: row l&15,
// k = (l>>4)*8+i; B: col l&15, same k; D: col l&15, row (l>>4)*4+i). Small integers are
// exact in bf16 and in E4M3, every partial sum is an exact f32 integer
// (|D| <= 12288), so bf16 and fp8 give the same checksums in any order.
//
// One fold = every A fragment times every B fragment = 64 MFMAs, i.e.
// D = (sum_t A_t)(sum_t B_t). After each fold, per lane and for i = 0..3:
//   c = c*G + (uint64)(int64)D[(l>>4)*4+i][l&15]
// The wave checksum is sum_l c_l.
//
// The MX sweep (fp4 = E2M1, fp6 = E2M3 on v_mfma_scale_f32_16x16x128_f8f6f4,
// every scale 1.0) is the same kernel on K = 128: k runs over 0..127 with
// idx = (...)*128 + k and lane l holds k = (l>>4)*32+i, so |D| <= 49152,
// still exact, and fp4 and fp6 give the same checksums.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "memtest.h"
#include "mfma_frag.h"
#include "nodeagent.h"
#include "sweep_common.h"

#define MS_FRAGS 8
#define MS_MFMA_PER_FOLD (MS_FRAGS * MS_FRAGS)
#define MS_FLOP_PER_MFMA_K 512.0  // 16 x 16 x 2, per unit of K
#define MS_MAX_K 128

// MS_BF16 and MS_FP8 are the dtype codes of na_mfma_sweep*; the MX sweep's
// format f (0 = fp4, 1 = fp6) is MS_FP4 + f.
enum { MS_BF16 = 0, MS_FP8 = 1, MS_FP4 = 2, MS_FP6 = 3, MS_DTYPES };

// The kernel leaves one na_mfma_record (nodeagent.h) per wave.

// k_len: K of the MFMA, 32 or 128.
__device__ __host__ inline int ms_value(mt_u64 base, mt_u64 w, int m, int t, int r, int k,
                                        int k_len) {
    mt_u64 idx =
        ((((w * 2 + (mt_u64)m) * 8 + (mt_u64)t) * 16 + (mt_u64)r) * (mt_u64)k_len + (mt_u64)k);
    unsigned e = (unsigned)(mt_mix64(base + idx) >> 40);  // 24 bits
    return m == 0 ? (int)(e % 7u) - 3 : (int)(e % 5u) - 2;
}

#if defined(__gfx950__)

template <int DTYPE>
using ms_traits = typename std::conditional<
    DTYPE == MS_BF16, mfma_bf16_16x16x32,
    typename std::conditional<
        DTYPE == MS_FP8, mfma_fp8_16x16x32,
        mfma_mx1_16x16x128<DTYPE == MS_FP4 ? MX_E2M1 : MX_E2M3>>::type>::type;

// One fold. The operands never change, so without the empty asm the
// compiler may compute D once and drop the loop; "+v" tells it each A
// fragment might have, at no instruction. One accumulation chain: this shape
// issues back to back at the same ~16 cycles on 1, 4 or 16 accumulators, and
// a single one leaves nothing to sum after the last MFMA.
template <typename T>
__device__ inline f32x4 ms_fold(typename T::frag (&a)[MS_FRAGS],
                                const typename T::frag (&b)[MS_FRAGS]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ta = 0; ta < MS_FRAGS; ++ta) {
        asm volatile("" : "+v"(a[ta]));
#pragma unroll
        for (int tb = 0; tb < MS_FRAGS; ++tb) acc = T::mfma(a[ta], b[tb], acc);
    }
    return acc;
}

// Fragment t of matrix m as lane l holds it: T::PER_LANE consecutive k of
// row (A) or column (B) l&15.
template <typename T>
__device__ inline typename T::frag ms_fragment(mt_u64 base, mt_u64 w, int m, int t, int l) {
    typename T::frag f{};
    const int r = l & 15, k0 = (l >> 4) * T::PER_LANE;
#pragma unroll
    for (int i = 0; i < T::PER_LANE; ++i) T::set(f, i, ms_value(base, w, m, t, r, k0 + i, T::K));
    return f;
}

// All fragments, unrolled by pack expansion: with 32 hashed elements per MX
// fragment a loop over t is past the size to which a pragma unrolls, and a
// fragment array indexed at run time would live in scratch.
template <typename T, int... Ts>
__device__ inline void ms_fill(typename T::frag (&a)[MS_FRAGS], typename T::frag (&b)[MS_FRAGS],
                               mt_u64 base, mt_u64 w, int l, std::integer_sequence<int, Ts...>) {
    ((a[Ts] = ms_fragment<T>(base, w, 0, Ts, l), b[Ts] = ms_fragment<T>(base, w, 1, Ts, l)), ...);
}

__device__ inline mt_u64 ms_update(mt_u64 c, f32x4 d) {
#pragma unroll
    for (int i = 0; i < 4; ++i) c = c * MS_G + (mt_u64)(long long)(int)d[i];
    return c;
}

// One wave of the sweep: the operands of global wave w, `outer` folds, the
// checksum reduced over the wave, and lane 0's record into records[w]. The
// body of mfma_sweep_kernel, and of the matrix waves of the load sweep
// (loadsweep.h), which runs the same chain beside a memory stream.
template <int DTYPE>
__device__ __forceinline__ void ms_wave(na_mfma_record* __restrict__ records, mt_u64 base,
                                        mt_u64 w, int outer) {
    typedef ms_traits<DTYPE> T;
    typedef typename T::frag frag;
    const ms_hw_where at = ms_where();
    const int l = threadIdx.x & 63;

    frag a[MS_FRAGS], b[MS_FRAGS];
    ms_fill<T>(a, b, base, w, l, std::make_integer_sequence<int, MS_FRAGS>{});

    // The stamps bracket the whole loop, go only into the record, and no
    // output is computed from them.
    const ms_clock t0 = ms_stamp();

    // Software-pipelined by one fold: the checksum update of fold j-1 does
    // not depend on fold j's MFMAs, so its VALU work issues in their shadow.
    mt_u64 c = 0;
    f32x4 d = ms_fold<T>(a, b);
    for (int j = 1; j < outer; ++j) {
        f32x4 dn = ms_fold<T>(a, b);
        c = ms_update(c, d);
        d = dn;
    }
    c = ms_update(c, d);

    const ms_clock t1 = ms_stamp();

    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (l == 0) {
        na_mfma_record rec;
        rec.checksum = c;
        rec.wave = (uint32_t)w;
        ms_record_simd(rec, t0, t1, at);
        records[w] = rec;
    }
}

#endif  // __gfx950__

// records: 4 * gridDim.x entries. base = seed * G (hoisted to the host).
// Launch with MS_BLOCK threads and more than half of the CU's LDS as dynamic
// shared memory.
template <int DTYPE>
__global__ void __launch_bounds__(MS_BLOCK)
mfma_sweep_kernel(na_mfma_record* __restrict__ records, mt_u64 base, int outer) {
#if defined(__gfx950__)
    // The dynamic LDS is a placement device and is never touched: a
    // workgroup that holds more than half of a CU's LDS cannot share the CU
    // with a second one, so each of its four waves has a SIMD to itself —
    // the condition for back-to-back 16-cycle issue of this MFMA shape.
    ms_wave<DTYPE>(records, base, (mt_u64)blockIdx.x * MS_WAVES_PER_WG + (threadIdx.x >> 6),
                   outer);
#else
    // wrong arch: a checksum no reference produces, so verification fails
    if ((threadIdx.x & 63) == 0) {
        na_mfma_record rec = {};
        rec.checksum = ~0ULL;
        records[(size_t)blockIdx.x * MS_WAVES_PER_WG + (threadIdx.x >> 6)] = rec;
    }
#endif
}
