// Chip-wide block-scaled MX GEMM sweep for the MI355X node agent (included from
// agent.hip; element encodings and packing are mx_formats.h's, the k maps of
// the instruction's operands are stated at mx_frag in mfma_frag.h, and the
// tile, swizzle, block-to-tile map and checksum are gemmsweep.h's).
//
// The GEMM sweep drives operands from device memory through L2 and LDS into
// v_mfma_f32_16x16x32_{bf16,fp8_fp8}. The MI355X's fp8 peak, all of FP4 and the
// serving kernels are on v_mfma_scale_f32_16x16x128_f8f6f4, which issues at
// twice that rate and takes an E8M0 scale per 32 elements next to every operand
// block. The MX checks and the MX sweep run that instruction on registers, the
// sweep with every scale 1.0. This kernel feeds it from memory, at the data
// rate it needs, with scales that come from memory too: a broken scale path,
// or a CU that cannot sustain the pipe from LDS, shows here and nowhere else.
//
// The problem (normative — tests/test_nodeagent_mxgemmsweep.py carries an
// independent numpy copy):
//
//   C[M x N] = reps * sum_k 2^ea[i][k/32] * a[i][k] * 2^eb[j][k/32] * b[j][k]
//
// M and N multiples of 256, K a multiple of BK = 128 elements (fp8, E4M3) or
// 256 (fp4, E2M1): 128 bytes per row of a k-step in both. S = K / 32 scale
// blocks per row. Arithmetic mod 2^64, G = MS_G, mix64 = mt_mix64, base = seed
// * G, and every draw is (mix64(base + at) >> 40) % mod, one hashed sequence
// laid out in this order:
//
//   a[i][k]  at i*K + k,                        drawn % 7 - 3
//   b[j][k]  at M*K + j*K + k,                  drawn % 5 - 2
//   ea[i][g] at M*K + N*K + i*S + g,            drawn % 2
//   eb[j][g] at M*K + N*K + M*S + j*S + g,      drawn % 2
//   p_i      at M*K + N*K + M*S + N*S + i,      mix64(base + at) | 1
//   q_j      at M*K + N*K + M*S + N*S + M + j,  mix64(base + at) | 1
//
// -3..3 is exact in E2M1 and in E4M3 and the scales are 1 or 2, so every
// product is an integer of magnitude at most 24 and every partial sum an exact
// f32 integer while 24 * reps * K < NA_MXGEMM_EXACT = 2^24: both formats give
// the same C in any summation order.
//
// Memory layout, the one users' tensors have: operands row-major and
// K-contiguous, fp8 one byte per element, fp4 two per byte with the even k in
// the low nibble; scales in separate uint8[rows][K/32] arrays of E8M0 bytes
// (127 + ea: 127 or 128), row-major.
//
// Tile, record index and checksum are the GEMM sweep's: tile t = ti*(N/256) +
// tj, one workgroup of four waves, wave (wr, wc) = (wave>>1, wave&1) the 128 x
// 128 sub-tile, record 4*t + 2*wr + wc with checksum sum p_i * q_j *
// (uint64)(int64)C[i][j].
//
// Data movement. A k-step is a 256-row x 128-byte slab of A and one of B, and
// next to each its rows' scales of that k-step: 4 bytes (fp8) or 8 (fp4) per
// row. LDS holds two stages: 2 x (32 KiB + 32 KiB) of operands, as in the GEMM
// sweep and with its chunk swizzle c ^ ((r>>1) & 7), then 2 x (2 KiB + 2 KiB)
// of scales, two dwords per row (fp8 uses the first): 136 KiB, more than half
// a CU's LDS. Thread t moves vector t&7 of rows j*32 + (t>>3) of a slab and
// the scales of row t: load for the NEXT k-step ahead of MFMAs of the current
// one, ds_write to the other stage after them, one __syncthreads per k-step.
// The instruction takes 128 bytes of a row in 2048 cycles of a SIMD where the
// GEMM sweep's takes them in 4096, so a k-step has half the MFMAs to cover
// the same loads:
//   fp4: a k-step is two sub-steps of one MFMA per accumulator; the first has
//        the next slab of A in flight and writes it, the second B's.
//   fp8: a k-step is one MFMA per accumulator; the accumulator rows 0-3 have
//        A's slab in flight, rows 4-7 B's.
// One trip of the loop is one MFMA per accumulator in both (the GEMM sweep's
// lesson: with two the accumulators leave their AGPRs), and 32 registers stage
// both slabs.
//
// Fragments, by the measured k maps. Lane l, g = l>>4, holds row l&15 of a
// 16-row block.
//   fp4: k = 32 g + i: the 16 bytes of chunk 4*s + g of the row in sub-step s,
//        one ds_read_b128 into the four registers the instruction reads.
//   fp8: k = 16 g + (i & 15) + 64 (i >> 4): chunk g into registers 0-3 and
//        chunk 4 + g into registers 4-7.
// Scales. The lanes of group g supply the scale of block g (k / 32 == g within
// the MFMA's 128 k) of their row, for 4- and 8-bit operands alike. A lane
// reads the dword holding its row's four block scales of the MFMA (dword s of
// the row's two) and shifts it right by 8 g: its own block's byte is byte 0
// (opsel 0), and the neighbouring blocks' scales, which differ from it as
// often as not, sit in the bytes opsel must not pick.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gemmsweep.h"
#include "mx_formats.h"

#define XS_SCALE_DWORDS 2  // per row and k-step in LDS: 8 block scales (fp4), 4 used by fp8
#define XS_SCALE_SLAB (GS_TILE * XS_SCALE_DWORDS)  // dwords of one operand's scales in a stage
#define XS_LDS_BYTES (GS_LDS_BYTES + 2 * 2 * XS_SCALE_SLAB * 4)
static_assert(XS_LDS_BYTES <= MS_CU_LDS_BYTES, "the stages do not fit in a CU's LDS");
static_assert(2 * XS_LDS_BYTES > MS_CU_LDS_BYTES, "a second workgroup would fit on the CU");
static_assert(MS_BLOCK == GS_TILE, "thread t stages the scales of row t");
#define XS_E8M0_ONE 127  // the E8M0 byte of 1.0

// Elements per k-step: 128 bytes of a row.
__device__ __host__ constexpr int xs_bk(int fmt) { return 128 * 8 / mx_bits(fmt); }
static_assert(xs_bk(MX_E4M3) == NA_MXGEMM_BK_FP8 && xs_bk(MX_E2M1) == NA_MXGEMM_BK_FP4,
              "nodeagent.h tells callers otherwise");

// Where the hashed sequence keeps what follows the elements (base included).
struct xs_bases {
    mt_u64 a, b, ea, eb, p, q;
};
__device__ __host__ inline xs_bases xs_layout(mt_u64 base, mt_u64 m, mt_u64 n, mt_u64 k) {
    xs_bases at;
    at.a = base;
    at.b = at.a + m * k;
    at.ea = at.b + n * k;
    at.eb = at.ea + m * (k / 32);
    at.p = at.eb + n * (k / 32);
    at.q = at.p + m;
    return at;
}

// The exponent (0 or 1) of the scale block at `at`.
__device__ __host__ inline int xs_exponent(mt_u64 at) { return (int)((mt_mix64(at) >> 40) & 1); }

// a, b: a_vecs and b_vecs 16-byte vectors, the operands row by row; vector v
// of the two together holds elements v*PER_VEC.. of the hashed sequence. sa,
// sb: a_blocks and b_blocks scale bytes, block x of the two together the
// exponent at ebase + x. One thread per vector, then one per scale byte.
template <int FMT>
__global__ void __launch_bounds__(MS_BLOCK)
mxgemm_fill_kernel(mt_vec* __restrict__ a, mt_vec* __restrict__ b, unsigned char* __restrict__ sa,
                   unsigned char* __restrict__ sb, mt_u64 a_vecs, mt_u64 b_vecs, mt_u64 a_blocks,
                   mt_u64 b_blocks, mt_u64 base, mt_u64 ebase) {
#if defined(__gfx950__)
    constexpr int PER_VEC = 128 / mx_bits(FMT);
    const mt_u64 v = (mt_u64)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v < a_vecs + b_vecs) {
        const bool is_b = v >= a_vecs;
        unsigned f[4] = {};
#pragma unroll
        for (int i = 0; i < PER_VEC; ++i)
            mx_put(f, FMT, i,
                   mx_encode_int(FMT, gs_element(base + v * PER_VEC + i, is_b ? GS_MOD_B : GS_MOD_A)));
        mt_vec out;
        __builtin_memcpy(&out, f, sizeof(out));
        if (is_b)
            b[v - a_vecs] = out;
        else
            a[v] = out;
    } else if (v - (a_vecs + b_vecs) < a_blocks + b_blocks) {
        const mt_u64 x = v - (a_vecs + b_vecs);
        const unsigned char e = (unsigned char)(XS_E8M0_ONE + xs_exponent(ebase + x));
        if (x < a_blocks)
            sa[x] = e;
        else
            sb[x - a_blocks] = e;
    }
#endif
}

#if defined(__gfx950__)

// A lane's operand of one MFMA: exactly the 4 (fp4) or 8 (fp8) registers the
// instruction reads, as mfma_mx1_16x16x128 holds them. From LDS: chunk g of
// the lane's row for fp4 (`at` already carries the sub-step), chunks g and 4 +
// g for fp8.
template <int FMT>
struct xs_operand {
    typedef int frag __attribute__((ext_vector_type(mx_bits(FMT))));
    static __device__ __forceinline__ frag read(const mt_vec* s, int at) {
        const i32x4 lo = __builtin_bit_cast(i32x4, s[at]);
        if constexpr (mx_bits(FMT) == 4) {
            return lo;
        } else {
            const i32x4 hi = __builtin_bit_cast(i32x4, s[at ^ 4]);
            return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
    }
    static __device__ __forceinline__ i32x8 widen(frag f) {
        if constexpr (mx_bits(FMT) == 4)
            return __builtin_shufflevector(f, f, 0, 1, 2, 3, -1, -1, -1, -1);
        else
            return f;
    }
};

#endif  // __gfx950__

// records: 4 * mt * nt entries. a: 256*mt rows, b: 256*nt rows, of ksteps *
// GS_ROW_VECS vectors each; sa, sb: their scales, ksteps * SUBS dwords per row.
// c: null, or 256*mt x 256*nt floats, row-major. wbase is where the weights
// start in the hashed sequence. Launch with mt * nt workgroups of MS_BLOCK
// threads and XS_LDS_BYTES of dynamic shared memory.
template <int FMT>
__global__ void __launch_bounds__(MS_BLOCK)
mxgemm_sweep_kernel(na_mfma_record* __restrict__ records, const mt_vec* __restrict__ a,
                    const mt_vec* __restrict__ b, const uint32_t* __restrict__ sa,
                    const uint32_t* __restrict__ sb, float* __restrict__ c, uint32_t mt,
                    uint32_t nt, uint32_t ksteps, uint32_t reps, mt_u64 wbase) {
    // The wave index is the same in all of a wave's lanes: scalar, so that it,
    // the record's address and the sub-tile cost no vector register.
#if defined(__gfx950__)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#else
    const int wave = threadIdx.x >> 6;
#endif
    const uint32_t t = gs_tile_of_block(blockIdx.x, mt, nt);
    na_mfma_record* const mine = records + (size_t)t * MS_WAVES_PER_WG + wave;
#if defined(__gfx950__)
    constexpr int SUBS = mx_bits(FMT) == 4 ? 2 : 1;  // MFMAs per accumulator and k-step
    extern __shared__ mt_vec xs_lds[];
    uint32_t* const scale_lds = reinterpret_cast<uint32_t*>(xs_lds + 2 * GS_STAGE_VECS);
    const ms_hw_where at = ms_where();
    const int l = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1;
    const uint32_t ti = t / nt, tj = t % nt;
    const size_t pitch = (size_t)ksteps * GS_ROW_VECS;  // vectors per operand row
    const uint32_t spitch = ksteps * SUBS;              // scale dwords per row

    // global -> LDS, operands: as the GEMM sweep. Scales: row threadIdx.x.
    const int lrow = threadIdx.x >> 3, chunk = threadIdx.x & 7;
    const mt_vec* const ga = a + (size_t)ti * GS_TILE * pitch;
    const mt_vec* const gb = b + (size_t)tj * GS_TILE * pitch;
    const uint32_t* const gsa = sa + ((size_t)ti * GS_TILE + threadIdx.x) * spitch;
    const uint32_t* const gsb = sb + ((size_t)tj * GS_TILE + threadIdx.x) * spitch;
    const uint32_t lane_vec = (uint32_t)lrow * (uint32_t)pitch + chunk;
    const int put = lrow * GS_ROW_VECS + (chunk ^ ((lrow >> 1) & 7));
    // LDS -> fragments: chunk (l>>4) (+ 4*s) of row (l&15) of each 16-row
    // block, and that row's scale dwords
    const int get = (l & 15) * GS_ROW_VECS + ((l >> 4) ^ ((l >> 1) & 7));
    const int get_a = wr * GS_WAVE_TILE * GS_ROW_VECS + get;
    const int get_b = GS_SLAB_VECS + wc * GS_WAVE_TILE * GS_ROW_VECS + get;
    const int sget_a = (wr * GS_WAVE_TILE + (l & 15)) * XS_SCALE_DWORDS;
    const int sget_b = XS_SCALE_SLAB + (wc * GS_WAVE_TILE + (l & 15)) * XS_SCALE_DWORDS;
    const int shift = 8 * (l >> 4);

    f32x4 acc[GS_FRAGS][GS_FRAGS];
#pragma unroll
    for (int i = 0; i < GS_FRAGS; ++i)
#pragma unroll
        for (int j = 0; j < GS_FRAGS; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // One operand's slab of k-step ks and its scales into registers, and from
    // there into their place (slab 0 = A, 1 = B) in a stage.
    mt_vec staged[GS_LOADS];
    uint32_t staged_scale[SUBS];
    auto load = [&](int slab, uint32_t ks) {
        const mt_vec* const g = slab == 0 ? ga : gb;
        const uint32_t* const gs = slab == 0 ? gsa : gsb;
#pragma unroll
        for (int j = 0; j < GS_LOADS; ++j)
            staged[j] = (g + ((size_t)j * 32 * pitch + (size_t)ks * GS_ROW_VECS))[lane_vec];
#pragma unroll
        for (int s = 0; s < SUBS; ++s) staged_scale[s] = gs[ks * SUBS + s];
    };
    auto store = [&](int stage, int slab) {
        mt_vec* const s = xs_lds + stage * GS_STAGE_VECS + slab * GS_SLAB_VECS + put;
#pragma unroll
        for (int j = 0; j < GS_LOADS; ++j) s[j * 32 * GS_ROW_VECS] = staged[j];
        uint32_t* const sc =
            scale_lds + (stage * 2 + slab) * XS_SCALE_SLAB + threadIdx.x * XS_SCALE_DWORDS;
#pragma unroll
        for (int s = 0; s < SUBS; ++s) sc[s] = staged_scale[s];
    };

    const ms_clock t0 = ms_stamp();

    load(0, 0);
    store(0, 0);
    load(1, 0);
    store(0, 1);
    __syncthreads();

    // The K loop, `reps` times into the same accumulators, as one sequence of
    // reps * ksteps steps of SUBS trips; see "Data movement" above. The loads
    // of the step after the last wrap to k-step 0 (in bounds) and land in a
    // stage nobody reads.
    const uint32_t trips = reps * ksteps * SUBS;
    uint32_t ks = ksteps == 1 ? 0 : 1, sub = 0, stage = 0;  // ks: the step being loaded
    typedef xs_operand<FMT> X;
    typename X::frag fa[GS_FRAGS], fb[GS_FRAGS];
    int ea[GS_FRAGS], eb[GS_FRAGS];
    auto rows = [&](int first) {  // the MFMAs of accumulator rows first .. first + 3
#pragma unroll
        for (int i = first; i < first + GS_FRAGS / 2; ++i)
#pragma unroll
            for (int j = 0; j < GS_FRAGS; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                    X::widen(fa[i]), X::widen(fb[j]), acc[i][j], FMT, FMT, 0, ea[i], 0, eb[j]);
    };
    for (uint32_t it = 0; it < trips; ++it) {
        load(SUBS == 1 ? 0 : (int)sub, ks);
        const mt_vec* const s = xs_lds + stage * GS_STAGE_VECS;
        const uint32_t* const sc = scale_lds + stage * 2 * XS_SCALE_SLAB + sub;
#pragma unroll
        for (int i = 0; i < GS_FRAGS; ++i) {
            fa[i] = X::read(s, (get_a ^ (sub * 4)) + i * 16 * GS_ROW_VECS);
            fb[i] = X::read(s, (get_b ^ (sub * 4)) + i * 16 * GS_ROW_VECS);
            ea[i] = (int)(sc[sget_a + i * 16 * XS_SCALE_DWORDS] >> shift);
            eb[i] = (int)(sc[sget_b + i * 16 * XS_SCALE_DWORDS] >> shift);
        }
        rows(0);
        if constexpr (SUBS == 1) {
            store(stage ^ 1, 0);
            load(1, ks);
        }
        rows(GS_FRAGS / 2);
        store(stage ^ 1, SUBS == 1 ? 1 : (int)sub);
        if (++sub == SUBS) {  // uniform: the same trip for all four waves
            __syncthreads();
            sub = 0;
            stage ^= 1;
            ks = ks + 1 == ksteps ? 0 : ks + 1;
        }
    }

    const ms_clock t1 = ms_stamp();

    // The GEMM sweep's epilogue, on this kernel's accumulators: checksum =
    // sum_i p_i * (sum_j q_j * C[i][j]) over this lane's elements; accumulator
    // register r of tile (i, j) is row i*16 + (l>>4)*4 + r, column j*16 +
    // (l&15) of the wave's sub-tile. The lane is counted again here (mbcnt), so
    // that no register holds it through the K loop for the epilogue's sake:
    // kept alive, it and the wave index were spilled in the fp4 kernel.
    const int le = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t row0 = ti * GS_TILE + wr * GS_WAVE_TILE + (le >> 4) * 4;
    const uint32_t col0 = tj * GS_TILE + wc * GS_WAVE_TILE + (le & 15);
    mt_u64 q[GS_FRAGS];
#pragma unroll
    for (int j = 0; j < GS_FRAGS; ++j)
        q[j] = gs_weight(wbase + (mt_u64)mt * GS_TILE + col0 + j * 16);
    float* const c0 = c == nullptr ? nullptr : c + (size_t)row0 * nt * GS_TILE + col0;
    mt_u64 sum = 0;
#pragma unroll
    for (int i = 0; i < GS_FRAGS; ++i) {
        // No instruction: row i's accumulators are in their AGPRs up to here
        // (see gemm_sweep_kernel).
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
    if (le == 0) {
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
