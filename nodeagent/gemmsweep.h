// Chip-wide GEMM sweep for the MI355X node agent (included from agent.hip;
// operand encodings and MFMA calls are mfma_frag.h's bf16 and fp8 16x16x32
// traits).
//
// The matrix-core sweeps run MFMA chains on operands that never leave
// registers, and the LDS, cache and memory sweeps move words nothing ever
// multiplies. This kernel is the path the workloads live on: operands from
// device memory, through L2 and LDS, into MFMA fragments, accumulated over a
// long K into a C tile. Every wave leaves an na_mfma_record whose checksum the
// host recomputes exactly, so a wrong wave is attributed to (XCC, SE, SH, CU,
// SIMD), and the launch yields the GEMM rate the chip delivers.
//
// The problem (normative — tests/test_nodeagent_gemmsweep.py carries an
// independent numpy copy): C[M x N] = reps * A[M x K] * B[N x K]^T, both
// operands K-contiguous, M and N multiples of 256, K a multiple of BK = 64
// elements (bf16) or 128 (E4M3): 128 bytes per row of a k-step in both.
// Arithmetic mod 2^64, G = MS_G, mix64 = mt_mix64, base = seed * G:
//
//   A[i][k] = ((mix64(base + i*K + k) >> 40) % 7) - 3
//   B[j][k] = ((mix64(base + M*K + j*K + k) >> 40) % 5) - 2
//   p_i     = mix64(base + M*K + N*K + i) | 1
//   q_j     = mix64(base + M*K + N*K + M + j) | 1
//
// Small integers are exact in bf16 and in E4M3 and every partial sum is an
// exact f32 integer while 6 * reps * K < 2^24, so both dtypes give the same C
// in any summation order.
//
// Tile t = ti*(N/256) + tj is C rows 256*ti.. and columns 256*tj..; one
// workgroup of four waves computes it, wave (wr, wc) = (wave>>1, wave&1) the
// 128 x 128 sub-tile at (128*wr, 128*wc). That wave leaves record 4*t + 2*wr +
// wc with checksum sum p_i * q_j * (uint64)(int64)C[i][j] over its sub-tile
// (p and q are odd, so any single wrong element changes it), computed from the
// accumulators in 64-bit integer VALU and summed over the wave.
//
// Data movement. A k-step is a 256-row x 128-byte slab of A and one of B. LDS
// holds two stages of both: 2 x (32 KiB + 32 KiB) = 128 KiB, more than half a
// CU's LDS, so the workgroup owns its CU and each wave a SIMD. Global to LDS
// is load-then-ds_write (not LDS-DMA, whose LDS address is fixed per lane and
// would move the swizzle into the global addresses): thread t loads vector
// t&7 of rows j*32 + (t>>3), j = 0..7, of each slab — eight consecutive lanes
// read one row's 128 bytes — for the NEXT k-step ahead of the MFMAs of the
// current one (A's slab over the first half of them, B's over the second) and
// writes them to the other stage after those MFMAs. One __syncthreads per
// hand-over: it orders this stage's writes before the next step's reads, and
// the step's reads (done before it) before the writes the step after that
// makes to the same stage. All four waves run the same trip counts, every
// loop is bounded by kernel arguments.
//
// Swizzle. A fragment read is ds_read_b128 by lane l of row r0 + (l&15),
// 16-byte chunk c = 4*s + (l>>4) of the row (traits' layout: row l&15,
// k = (l>>4)*8 + i within sub-step s; an E4M3 chunk is two fragments of 8
// k). Rows are 128 bytes apart and the 64 banks span 256 bytes, so unswizzled
// the 16 lanes of one chunk index fall on 2 bank groups of 16 bytes: 8-way
// conflict. Row r stores chunk c at chunk position c ^ ((r>>1) & 7): rows r0
// .. r0+15 (r0 a multiple of 16) at one c then take bank byte (r&1)*128 +
// 16*(c ^ (r>>1 & 7)), sixteen distinct 16-byte groups, all 256 bytes. The
// writer's sixteen consecutive lanes cover two whole rows, again all 256.
// XOR with a function of the row alone is a bijection on the row's chunks.
//
// Block to tile. Workgroups are dealt round-robin to the 8 XCDs, each with an
// L2 of its own, so block b = 8*i + x becomes the i-th of a contiguous range
// of positions owned by XCD x, and positions walk the tiles in groups of
// GS_GROUP tile rows, column by column: the 32 tiles an XCD runs at a time are
// 4 x 8 and share 4 row slabs of A and 8 of B in its L2. The record index
// follows the tile, not the block.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "memtest.h"
#include "mfma_frag.h"
#include "mfmasweep.h"
#include "nodeagent.h"
#include "sweep_common.h"

#define GS_TILE 256       // C tile edge per workgroup
#define GS_WAVE_TILE 128  // per wave
#define GS_FRAGS (GS_WAVE_TILE / 16)  // 16x16 accumulator tiles per wave and dimension
#define GS_ROW_VECS 8     // 16-byte vectors per row of a k-step
#define GS_SLAB_VECS (GS_TILE * GS_ROW_VECS)  // one operand's share of a stage: 32 KiB
#define GS_STAGE_VECS (2 * GS_SLAB_VECS)
#define GS_LDS_BYTES (2 * GS_STAGE_VECS * 16)
#define GS_LOADS (GS_SLAB_VECS / MS_BLOCK)  // vectors a thread moves per slab
#define GS_GROUP 4   // tile rows walked together
#define GS_XCDS 8
static_assert(GS_TILE == NA_GEMM_TILE && GS_ROW_VECS * 16 / 2 == NA_GEMM_BK_BF16 &&
                  GS_ROW_VECS * 16 == NA_GEMM_BK_FP8,
              "nodeagent.h tells callers otherwise");
static_assert(2 * GS_LDS_BYTES > MS_CU_LDS_BYTES, "a second workgroup would fit on the CU");

// Element `at` (its index in A, or M*K + its index in B, plus base) of the
// operand whose values are 0..mod-1 shifted to be centred on 0.
__device__ __host__ inline int gs_element(mt_u64 at, unsigned mod) {
    return (int)((unsigned)(mt_mix64(at) >> 40) % mod) - (int)(mod / 2);
}
#define GS_MOD_A 7u
#define GS_MOD_B 5u

__device__ __host__ inline mt_u64 gs_weight(mt_u64 at) { return mt_mix64(at) | 1; }

// The tile block b computes (see "Block to tile" above); a bijection of
// 0..mt*nt-1.
__device__ __host__ inline uint32_t gs_tile_of_block(uint32_t b, uint32_t mt, uint32_t nt) {
    const uint32_t tiles = mt * nt, q = tiles / GS_XCDS, rem = tiles % GS_XCDS;
    const uint32_t x = b % GS_XCDS, i = b / GS_XCDS;
    const uint32_t u = x * q + (x < rem ? x : rem) + i;  // XCD x owns q (+1 if x < rem) positions
    const uint32_t per = GS_GROUP * nt, first = u / per * GS_GROUP;
    const uint32_t rows = mt - first < GS_GROUP ? mt - first : GS_GROUP;
    const uint32_t w = u % per;
    return (first + w % rows) * nt + w / rows;
}

#if defined(__gfx950__)

// Fragment h of a 16-byte chunk: the whole chunk for bf16, its low or high 8
// bytes for E4M3.
template <typename T>
__device__ __forceinline__ typename T::frag gs_frag(mt_vec v, uint32_t h) {
    if constexpr (sizeof(typename T::frag) == sizeof(mt_vec))
        return __builtin_bit_cast(typename T::frag, v);
    else
        return (typename T::frag)(h ? v.y : v.x);
}

#endif  // __gfx950__

// a, b: a_vecs and b_vecs 16-byte vectors, the operands row by row. A's
// elements are 0..M*K-1 of the hashed sequence and B's follow, so vector v of
// the two together holds elements v*PER_VEC.. whichever operand it lies in.
template <int DTYPE>
__global__ void __launch_bounds__(MS_BLOCK)
gemm_fill_kernel(mt_vec* __restrict__ a, mt_vec* __restrict__ b, mt_u64 a_vecs, mt_u64 b_vecs,
                 mt_u64 base) {
#if defined(__gfx950__)
    typedef ms_traits<DTYPE> T;
    typedef typename T::frag frag;
    constexpr int FRAGS = sizeof(mt_vec) / sizeof(frag), PER_VEC = FRAGS * T::PER_LANE;
    const mt_u64 v = (mt_u64)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= a_vecs + b_vecs) return;
    const bool is_b = v >= a_vecs;
    frag f[FRAGS] = {};
#pragma unroll
    for (int i = 0; i < PER_VEC; ++i)
        T::set(f[i / T::PER_LANE], i % T::PER_LANE,
               gs_element(base + v * PER_VEC + i, is_b ? GS_MOD_B : GS_MOD_A));
    mt_vec out;
    __builtin_memcpy(&out, f, sizeof(out));
    if (is_b)
        b[v - a_vecs] = out;
    else
        a[v] = out;
#endif
}

// records: 4 * mt * nt entries. a: 256*mt rows, b: 256*nt rows, of ksteps *
// GS_ROW_VECS vectors each. c: null, or 256*mt x 256*nt floats, row-major.
// base = seed * G and wbase = base + M*K + N*K (where the weights start) are
// hoisted to the host. Launch with mt * nt workgroups of MS_BLOCK threads and
// GS_LDS_BYTES of dynamic shared memory.
template <int DTYPE>
__global__ void __launch_bounds__(MS_BLOCK)
gemm_sweep_kernel(na_mfma_record* __restrict__ records, const mt_vec* __restrict__ a,
                  const mt_vec* __restrict__ b, float* __restrict__ c, uint32_t mt, uint32_t nt,
                  uint32_t ksteps, uint32_t reps, mt_u64 wbase) {
    const int wave = threadIdx.x >> 6;
    const uint32_t t = gs_tile_of_block(blockIdx.x, mt, nt);
    na_mfma_record* const mine = records + (size_t)t * MS_WAVES_PER_WG + wave;
#if defined(__gfx950__)
    typedef ms_traits<DTYPE> T;
    constexpr int HALVES = sizeof(mt_vec) / sizeof(typename T::frag);
    extern __shared__ mt_vec gs_lds[];
    const ms_hw_where at = ms_where();
    const int l = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1;
    const uint32_t ti = t / nt, tj = t % nt;
    const size_t pitch = (size_t)ksteps * GS_ROW_VECS;  // vectors per operand row

    // global -> LDS: this thread's vector of row j*32 + lrow, j = 0..GS_LOADS-1.
    // A uniform 64-bit base plus a 32-bit lane offset (31 rows of under 2^23
    // bytes), so that the loads take their base from scalar registers.
    const int lrow = threadIdx.x >> 3, chunk = threadIdx.x & 7;
    const mt_vec* const ga = a + (size_t)ti * GS_TILE * pitch;
    const mt_vec* const gb = b + (size_t)tj * GS_TILE * pitch;
    const uint32_t lane_vec = (uint32_t)lrow * (uint32_t)pitch + chunk;
    const int put = lrow * GS_ROW_VECS + (chunk ^ ((lrow >> 1) & 7));
    // LDS -> fragments: chunk 4*s + (l>>4) of row (l&15) of each 16-row block
    const int get = (l & 15) * GS_ROW_VECS + ((l >> 4) ^ ((l >> 1) & 7));
    const int get_a = wr * GS_WAVE_TILE * GS_ROW_VECS + get;
    const int get_b = GS_SLAB_VECS + wc * GS_WAVE_TILE * GS_ROW_VECS + get;

    f32x4 acc[GS_FRAGS][GS_FRAGS];
#pragma unroll
    for (int i = 0; i < GS_FRAGS; ++i)
#pragma unroll
        for (int j = 0; j < GS_FRAGS; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // One operand's slab of k-step ks into registers, and from there into
    // its place (slab 0 = A, 1 = B) in a stage.
    mt_vec staged[GS_LOADS];
    auto load = [&](const mt_vec* g, uint32_t ks) {
#pragma unroll
        for (int j = 0; j < GS_LOADS; ++j)
            staged[j] = (g + ((size_t)j * 32 * pitch + (size_t)ks * GS_ROW_VECS))[lane_vec];
    };
    auto store = [&](int stage, int slab) {
        mt_vec* const s = gs_lds + stage * GS_STAGE_VECS + slab * GS_SLAB_VECS + put;
#pragma unroll
        for (int j = 0; j < GS_LOADS; ++j) s[j * 32 * GS_ROW_VECS] = staged[j];
    };

    const ms_clock t0 = ms_stamp();

    load(ga, 0);
    store(0, 0);
    load(gb, 0);
    store(0, 1);
    __syncthreads();

    // The K loop, `reps` times into the same accumulators, as one sequence of
    // reps * ksteps steps. A step has two sub-steps of four chunks per row, an
    // E4M3 sub-step two halves; one trip of the loop is one of those: ONE
    // MFMA per accumulator, so that each accumulator is one value updated in
    // place in its AGPRs (with two updates per trip the register allocator
    // shuffles the 256 of them through VGPRs). The first sub-step has the next
    // step's slab of A in flight and writes it to the other stage, the second
    // does the same for B, so 32 registers stage both; nobody reads that stage
    // before the barrier that ends the step. The loads of the step after the
    // last wrap to k-step 0 (in bounds) and land in a stage nobody reads.
    constexpr uint32_t PHASES = 2 * HALVES;
    const uint32_t trips = reps * ksteps * PHASES;
    uint32_t ks = ksteps == 1 ? 0 : 1, phase = 0, stage = 0;  // ks: the step being loaded
    mt_vec fa[GS_FRAGS], fb[GS_FRAGS];
    for (uint32_t it = 0; it < trips; ++it) {
        const uint32_t sub = phase / HALVES, h = phase % HALVES;
        if (h == 0) {
            load(sub == 0 ? ga : gb, ks);
            const mt_vec* const s = gs_lds + stage * GS_STAGE_VECS;
#pragma unroll
            for (int i = 0; i < GS_FRAGS; ++i) {
                fa[i] = s[(get_a ^ (sub * 4)) + i * 16 * GS_ROW_VECS];
                fb[i] = s[(get_b ^ (sub * 4)) + i * 16 * GS_ROW_VECS];
            }
        }
#pragma unroll
        for (int i = 0; i < GS_FRAGS; ++i)
#pragma unroll
            for (int j = 0; j < GS_FRAGS; ++j)
                acc[i][j] = T::mfma(gs_frag<T>(fa[i], h), gs_frag<T>(fb[j], h), acc[i][j]);
        if (h == HALVES - 1) store(stage ^ 1, sub);
        if (++phase == PHASES) {  // uniform: the same trip for all four waves
            __syncthreads();
            phase = 0;
            stage ^= 1;
            ks = ks + 1 == ksteps ? 0 : ks + 1;
        }
    }

    const ms_clock t1 = ms_stamp();

    // checksum = sum_i p_i * (sum_j q_j * C[i][j]) over this lane's elements:
    // accumulator register r of tile (i, j) is row i*16 + (l>>4)*4 + r,
    // column j*16 + (l&15) of the wave's sub-tile
    const uint32_t row0 = ti * GS_TILE + wr * GS_WAVE_TILE + (l >> 4) * 4;
    const uint32_t col0 = tj * GS_TILE + wc * GS_WAVE_TILE + (l & 15);
    mt_u64 q[GS_FRAGS];
#pragma unroll
    for (int j = 0; j < GS_FRAGS; ++j)
        q[j] = gs_weight(wbase + (mt_u64)mt * GS_TILE + col0 + j * 16);
    // row by row, so that a row's weight and its address in C live only
    // through its own eight columns
    float* const c0 = c == nullptr ? nullptr : c + (size_t)row0 * nt * GS_TILE + col0;
    mt_u64 sum = 0;
#pragma unroll
    for (int i = 0; i < GS_FRAGS; ++i) {
        // No instruction: row i's accumulators are in their AGPRs up to here.
        // Without it all 256 are copied out right after the loop, and some
        // of them on to scratch.
#pragma unroll
        for (int j = 0; j < GS_FRAGS; ++j) asm volatile("" : "+a"(acc[i][j]));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mt_u64 inner = 0;
#pragma unroll
            for (int j = 0; j < GS_FRAGS; ++j) inner += q[j] * (mt_u64)(long long)(int)acc[i][j][r];
            sum += gs_weight(wbase + row0 + i * 16 + r) * inner;
            if (c0 != nullptr) {
                float* const row = c0 + (size_t)(i * 16 + r) * nt * GS_TILE;
#pragma unroll
                for (int j = 0; j < GS_FRAGS; ++j) row[j * 16] = acc[i][j][r];
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (l == 0) {
        na_mfma_record rec;
        rec.checksum = sum;
        rec.wave = t * MS_WAVES_PER_WG + wave;
        ms_record_simd(rec, t0, t1, at);
        *mine = rec;
    }
#else
    // wrong arch: a checksum no reference produces, so verification fails
    if ((threadIdx.x & 63) == 0) {
        na_mfma_record rec = {};
        rec.checksum = ~0ULL;
        *mine = rec;
    }
#endif
}
