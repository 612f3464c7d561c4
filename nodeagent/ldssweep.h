// Chip-wide LDS sweep for the MI355X node agent (included from agent.hip).
//
// na_lds_selftest writes and reads 32-bit words and adds every mismatch into
// one counter. This kernel puts one workgroup at a time on every CU (it holds
// the whole per-workgroup LDS allocation), drives the LDS through every
// access path gfx950 kernels use — 32- and 128-bit reads and writes, the
// LDS-DMA loads at 16, 4 and 12 bytes, the transposed read
// ds_read_b64_tr_b16, LDS atomics — and leaves one record per workgroup: a
// checksum per phase, the CU it ran on, an in-kernel diagnosis of the first
// wrong word, and two clock deltas around a read-only streaming phase. The
// host recomputes every checksum exactly, so a bad LDS is attributed to
// (XCC, SE, SH, CU).
//
// Specification (normative — tests/test_nodeagent_ldssweep.py carries an
// independent numpy copy); arithmetic mod 2^64, G = 0x9E3779B97F4A7C15,
// mix64 = mt_mix64 of memtest.h.
//
//   W = lds_bytes / 4 words, C = W / 256 chunks of 1 KiB (lds_bytes is a
//   multiple of 4096, so C is a multiple of 4), t = thread 0..255,
//   wave v = t >> 6, lane l = t & 63.
//   pat(p, j)    = (uint32)(mix64(seed*G + p*2^32 + j) >> 32)   pattern p, word j
//   src(p, i, r) = pat(p, (i + 256 r) mod W)     LDS word i under rotation r
//   rot          = workgroup mod C: LDS chunk c holds pattern chunk c + rot.
//                  Workgroups C apart hold the same data; the index in the
//                  record tells them apart.
//   perm(t)      = (t + 67) & 255: the read-back permutation. A lane reads
//                  what lane l+3 of the next wave (or the one after) wrote,
//                  and consecutive lanes still read consecutive addresses,
//                  which is conflict-free for every width used here.
//   Bytes, 16-bit elements and 64-bit values are the little-endian views of
//   the words: element e is bits 16(e&1).. of word e>>1, a 16-byte vector u
//   is words 4u..4u+3, its lo = w0 | w1<<32 and hi = w2 | w3<<32.
//
// Each thread folds what it reads, in read order, as c = c*G + value; the
// phase checksum is the sum of c over the 256 threads (the stream phase
// sums instead). Phases in order, each on the leading lds_bytes:
//
//   b32     pattern 0. For pol in (0, ~0): step k < C: thread t stores
//           src(0, 256k+t, rot) ^ pol to word 256k+t; barrier; step k < C:
//           it reads word 256k+perm(t) and folds it zero-extended; barrier.
//           One checksum runs through both polarities.
//   b128    pattern 1, the same with 16-byte vectors: step k < C/4, store
//           vector 256k+t, read vector 256k+perm(t), fold lo then hi.
//   dma16   pattern 2 lies in global memory, W words. Step k < C/4: wave
//           v issues one global_load_lds_dwordx4 to LDS bytes 4096k + 1024v
//           (+16 l by the hardware), lane l sourcing the 16 bytes of vector
//           ((256k + t) + 64 r) mod W/4, r = rot: LDS word i receives
//           src(2, i, r). vmcnt(0), barrier, read back as b128 does.
//   dma4    the same by global_load_lds_dword, step k < C: LDS bytes
//           1024k + 256v (+4 l), source word (256k + t + 256 r) mod W,
//           r = (rot + 1) mod C. Read back as b128 does.
//   dma12   global_load_lds_dwordx3. Measured on MI355X: the hardware puts
//           lane l's 12 bytes at the wave's base + 16 l, not + 12 l, and
//           leaves the fourth word of each 16-byte slot alone. So the steps
//           are dma16's: step k < C/4, LDS bytes 4096k + 1024v (+16 l), lane
//           l sourcing the first 12 bytes of vector ((256k + t) + 64 r) mod
//           W/4, r = (rot + 2) mod C. LDS word i then holds src(2, i, r)
//           where i mod 4 < 3, and still dma4's src(2, i, (rot + 1) mod C)
//           where i mod 4 = 3: 12 of every 16 bytes are new. Read back as
//           b128 does.
//   tr16    pattern 3, stored as 16-bit elements: step k < 2C, thread t
//           stores element 256k+t. Read with ds_read_b64_tr_b16 in tiles of
//           4 rows x 16 columns, a tile being 128 contiguous bytes (row
//           stride 32): step k < C/2, the 16-lane group g = l >> 4 of wave v
//           takes tile T = 16k + 4v + g, lane 4q+p of the group supplying
//           byte address 128T + 32q + 8p. Lane i of the group receives
//           column i: its value is sum_q elem(64T + 16q + i) << 16q.
//   atomic  pattern 4. Zero the region, barrier. Step k < C: thread t adds
//           a = src(4, 256k+t, rot) to word 256k+t; then, with no barrier
//           in between, step k < C: to word i = 256k + ((t+64) & 255), a
//           word of the next wave's, it adds src(4, i, rot) >> 16. Every word
//           ends as a + (a >> 16) mod 2^32. Barrier, read back as b32 does.
//   stream  pattern 5, stored as b128 stores. `iters` passes, each reading
//           every vector once (thread t reads vector 256k+t, k < C/4); the
//           thread adds every lo and hi it reads into one 64-bit sum, and
//           the checksum is the sum over threads: iters x the sum of all
//           64-bit values of the region. s_memtime / s_memrealtime are read
//           after the barrier before the first pass and after the barrier
//           behind the last.
//
// b32, b128 and the dma phases also compare every word they read with its
// expected value: bad_words counts the mismatches, first_bad_offset is the
// LDS byte offset of the first (earliest phase, then lowest offset),
// bad_phase that phase and xor_mask the OR of got ^ want. That is diagnosis
// for the operator; the verdict is the host's comparison of the checksums.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "memtest.h"
#include "nodeagent.h"
#include "sweep_common.h"

#define LS_BLOCK MS_BLOCK    // four waves, as every sweep
#define LS_CHUNK_WORDS 256   // 1 KiB: the unit of rotation
#define LS_GRANULE 4096      // lds_bytes is a multiple of this: one 16-byte access per thread
#define LS_MAX_BYTES MS_CU_LDS_BYTES
#define LS_PERM(t) (((t) + 67u) & 255u)

enum { LS_B32, LS_B128, LS_DMA16, LS_DMA4, LS_DMA12, LS_TR16, LS_ATOMIC, LS_STREAM, LS_PHASES };
enum { LS_PAT_B32, LS_PAT_B128, LS_PAT_DMA, LS_PAT_TR16, LS_PAT_ATOMIC, LS_PAT_STREAM };

// The kernel leaves one na_lds_record (nodeagent.h) per workgroup.
static_assert(LS_PHASES == NA_LDS_PHASES && LS_GRANULE == NA_LDS_GRANULE &&
                  LS_MAX_BYTES == NA_LDS_MAX_BYTES,
              "nodeagent.h tells callers otherwise");

__device__ __host__ inline uint32_t ls_pat(mt_u64 base, int pat, uint32_t j) {
    return (uint32_t)(mt_mix64(base + ((mt_u64)pat << 32) + j) >> 32);
}

#if defined(__gfx950__)

typedef __attribute__((address_space(3))) void ls_lds_void;
typedef __attribute__((address_space(1))) void ls_global_void;
typedef short ls_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) ls_s16x4 ls_lds_s16x4;

// LDS word i under a rotation of rotw = 256 r words; i < W and rotw < W.
__device__ inline uint32_t ls_src(mt_u64 base, int pat, uint32_t i, uint32_t rotw, uint32_t W) {
    uint32_t j = i + rotw;
    return ls_pat(base, pat, j >= W ? j - W : j);
}

// key = phase << 32 | byte offset of the first bad word; ~0 = none
struct ls_diag {
    mt_u64 bad, key, x;
};

__device__ inline void ls_check(ls_diag& d, int phase, uint32_t word, uint32_t got,
                                uint32_t want) {
    const uint32_t x = got ^ want;
    if (x == 0) return;
    d.bad++;
    d.x |= x;
    const mt_u64 key = ((mt_u64)phase << 32) | ((mt_u64)word * 4);
    if (key < d.key) d.key = key;
}

struct ls_ctx {
    unsigned char* mem;
    mt_u64 base;
    uint32_t t, W, C;
};

__device__ inline void ls_fill32(const ls_ctx& x, int pat, uint32_t rotw, uint32_t pol) {
    uint32_t* w = reinterpret_cast<uint32_t*>(x.mem);
    for (uint32_t k = 0; k < x.C; ++k) {
        const uint32_t i = k * 256 + x.t;
        w[i] = ls_src(x.base, pat, i, rotw, x.W) ^ pol;
    }
}

// The leading `chunks` chunks through perm; CHECK compares with the pattern.
template <bool CHECK>
__device__ inline mt_u64 ls_read32(const ls_ctx& x, mt_u64 c, uint32_t chunks, int phase, int pat,
                                   uint32_t rotw, uint32_t pol, ls_diag& d) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(x.mem);
    for (uint32_t k = 0; k < chunks; ++k) {
        const uint32_t i = k * 256 + LS_PERM(x.t);
        const uint32_t got = w[i];
        c = c * MS_G + got;
        if (CHECK) ls_check(d, phase, i, got, ls_src(x.base, pat, i, rotw, x.W) ^ pol);
    }
    return c;
}

__device__ inline void ls_fill128(const ls_ctx& x, int pat, uint32_t rotw, uint32_t pol) {
    uint4* v = reinterpret_cast<uint4*>(x.mem);
    for (uint32_t k = 0; k < x.C / 4; ++k) {
        const uint32_t u = k * 256 + x.t;
        uint32_t j = 4 * u + rotw;  // a vector never straddles the wrap
        if (j >= x.W) j -= x.W;
        v[u] = make_uint4(ls_pat(x.base, pat, j) ^ pol, ls_pat(x.base, pat, j + 1) ^ pol,
                          ls_pat(x.base, pat, j + 2) ^ pol, ls_pat(x.base, pat, j + 3) ^ pol);
    }
}

// rotw3 is the rotation of each vector's fourth word: rotw but for dma12.
__device__ inline mt_u64 ls_read128(const ls_ctx& x, mt_u64 c, int phase, int pat, uint32_t rotw,
                                    uint32_t rotw3, uint32_t pol, ls_diag& d) {
    const uint4* v = reinterpret_cast<const uint4*>(x.mem);
    for (uint32_t k = 0; k < x.C / 4; ++k) {
        const uint32_t u = k * 256 + LS_PERM(x.t);
        const uint4 got = v[u];
        c = c * MS_G + ((mt_u64)got.x | ((mt_u64)got.y << 32));
        c = c * MS_G + ((mt_u64)got.z | ((mt_u64)got.w << 32));
        uint32_t j = 4 * u + rotw;
        if (j >= x.W) j -= x.W;
        ls_check(d, phase, 4 * u, got.x, ls_pat(x.base, pat, j) ^ pol);
        ls_check(d, phase, 4 * u + 1, got.y, ls_pat(x.base, pat, j + 1) ^ pol);
        ls_check(d, phase, 4 * u + 2, got.z, ls_pat(x.base, pat, j + 2) ^ pol);
        ls_check(d, phase, 4 * u + 3, got.w, ls_src(x.base, pat, 4 * u + 3, rotw3, x.W) ^ pol);
    }
    return c;
}

// One LDS-DMA sub-phase of SIZE bytes per lane over the region. The LDS
// destination is the wave's base, wave-uniform; the hardware adds lane *
// STRIDE, STRIDE being SIZE but 16 for SIZE 12. A lane's source is the
// rotated image of its destination, STRIDE-aligned, so source offsets end at
// or below lds_bytes, the buffer's size.
template <int SIZE>
__device__ inline void ls_dma(const ls_ctx& x, const unsigned char* src, uint32_t rot_bytes) {
    constexpr uint32_t STRIDE = SIZE == 12 ? 16 : SIZE;
    const uint32_t lds_bytes = x.W * 4, wave = x.t >> 6;
    for (uint32_t k = 0; k < lds_bytes / (256 * STRIDE); ++k) {
        uint32_t from = k * 256 * STRIDE + x.t * STRIDE + rot_bytes;
        if (from >= lds_bytes) from -= lds_bytes;
        unsigned char* to = x.mem + k * 256 * STRIDE + wave * 64 * STRIDE;
        ls_global_void* g = (ls_global_void*)(src + from);
        ls_lds_void* s = (ls_lds_void*)to;
        // the builtin takes its size as a literal
        if (SIZE == 16) __builtin_amdgcn_global_load_lds(g, s, 16, 0, 0);
        if (SIZE == 12) __builtin_amdgcn_global_load_lds(g, s, 12, 0, 0);
        if (SIZE == 4) __builtin_amdgcn_global_load_lds(g, s, 4, 0, 0);
    }
    // the loads write LDS behind the compiler's back: drain them before the
    // barrier that precedes the read
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__device__ inline mt_u64 ls_sum(mt_u64 s, const mt_vec& v) { return s + v.x + v.y; }

#endif  // __gfx950__

// records: gridDim.x entries. src: the dma pattern, lds_bytes / 4 words. base = seed * G (hoisted to the host). Launch with
// LS_BLOCK threads and the whole per-workgroup LDS allocation (at least
// lds_bytes, a multiple of LS_GRANULE) as dynamic shared memory; iters >= 1.
__global__ void __launch_bounds__(LS_BLOCK)
lds_sweep_kernel(na_lds_record* __restrict__ records, const uint32_t* __restrict__ src_,
                 mt_u64 base, uint32_t lds_bytes, int iters) {
#if defined(__gfx950__)
    extern __shared__ __attribute__((aligned(16))) unsigned char ls_mem[];
    const ms_hw_where at = ms_where();
    const unsigned char* src = reinterpret_cast<const unsigned char*>(src_);
    ls_ctx x;
    x.mem = ls_mem;
    x.base = base;
    x.t = threadIdx.x;
    x.W = lds_bytes / 4;
    x.C = x.W / LS_CHUNK_WORDS;
    const uint32_t t = x.t, W = x.W, C = x.C;
    const uint32_t rot = blockIdx.x % C, rotw = rot * LS_CHUNK_WORDS;
    mt_u64 c[LS_PHASES] = {};
    ls_diag d = {0, ~0ULL, 0};

    // b32, b128: both polarities
    for (int p = 0; p < 2; ++p) {
        const uint32_t pol = p ? ~0u : 0u;
        ls_fill32(x, LS_PAT_B32, rotw, pol);
        __syncthreads();
        c[LS_B32] = ls_read32<true>(x, c[LS_B32], C, LS_B32, LS_PAT_B32, rotw, pol, d);
        __syncthreads();
    }
    for (int p = 0; p < 2; ++p) {
        const uint32_t pol = p ? ~0u : 0u;
        ls_fill128(x, LS_PAT_B128, rotw, pol);
        __syncthreads();
        c[LS_B128] = ls_read128(x, c[LS_B128], LS_B128, LS_PAT_B128, rotw, rotw, pol, d);
        __syncthreads();
    }

    // dma: LDS filled straight from global memory at each width
    {
        ls_dma<16>(x, src, rot * 1024);
        c[LS_DMA16] = ls_read128(x, 0, LS_DMA16, LS_PAT_DMA, rotw, rotw, 0, d);
        __syncthreads();
        const uint32_t r4 = (rot + 1) % C, rotw4 = r4 * LS_CHUNK_WORDS;
        ls_dma<4>(x, src, r4 * 1024);
        c[LS_DMA4] = ls_read128(x, 0, LS_DMA4, LS_PAT_DMA, rotw4, rotw4, 0, d);
        __syncthreads();
        const uint32_t r12 = (rot + 2) % C;
        ls_dma<12>(x, src, r12 * 1024);
        c[LS_DMA12] = ls_read128(x, 0, LS_DMA12, LS_PAT_DMA, r12 * LS_CHUNK_WORDS, rotw4, 0, d);
        __syncthreads();
    }

    // tr16: 16-bit stores, transposed 64-bit reads. Every lane of every wave
    // is active and supplies an in-bounds, 8-byte-aligned address.
    {
        uint16_t* h = reinterpret_cast<uint16_t*>(ls_mem);
        for (uint32_t k = 0; k < 2 * C; ++k) {
            const uint32_t e = k * 256 + t;
            h[e] = (uint16_t)(ls_src(base, LS_PAT_TR16, e >> 1, rotw, W) >> (16 * (e & 1)));
        }
        __syncthreads();
        const uint32_t l = t & 63, wave = t >> 6;
        const uint32_t lane_off = 128 * (4 * wave + (l >> 4)) + 32 * ((l >> 2) & 3) + 8 * (l & 3);
        mt_u64 cc = 0;
        for (uint32_t k = 0; k < C / 2; ++k) {
            const ls_s16x4 got = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (ls_lds_s16x4*)(ls_mem + k * 2048 + lane_off));
            cc = cc * MS_G + (((mt_u64)(uint16_t)got[0]) | ((mt_u64)(uint16_t)got[1] << 16) |
                              ((mt_u64)(uint16_t)got[2] << 32) | ((mt_u64)(uint16_t)got[3] << 48));
        }
        c[LS_TR16] = cc;
        __syncthreads();
    }

    // atomic: every word receives one add from each of two waves
    {
        uint32_t* w = reinterpret_cast<uint32_t*>(ls_mem);
        for (uint32_t k = 0; k < C; ++k) w[k * 256 + t] = 0;
        __syncthreads();
        for (uint32_t k = 0; k < C; ++k) {
            const uint32_t i = k * 256 + t;
            atomicAdd(&w[i], ls_src(base, LS_PAT_ATOMIC, i, rotw, W));
        }
        for (uint32_t k = 0; k < C; ++k) {
            const uint32_t i = k * 256 + ((t + 64) & 255);
            atomicAdd(&w[i], ls_src(base, LS_PAT_ATOMIC, i, rotw, W) >> 16);
        }
        __syncthreads();
        c[LS_ATOMIC] = ls_read32<false>(x, 0, C, LS_ATOMIC, LS_PAT_ATOMIC, rotw, 0, d);
        __syncthreads();
    }

    // stream: read-only passes at rate. The stamps bracket the whole phase
    // of the workgroup, go only into the record, and no output is computed
    // from them.
    ls_fill128(x, LS_PAT_STREAM, rotw, 0);
    __syncthreads();
    const ms_clock t0 = ms_stamp();
    {
        const mt_vec* v = reinterpret_cast<const mt_vec*>(ls_mem) + t;
        const uint32_t steps = C / 4;  // 4 KiB each: one vector per thread
        mt_u64 s = 0;
        if (steps % 8 == 0) {
            // Groups of eight reads at immediate offsets from one address,
            // two groups in registers: the reads of one are issued before the
            // other is summed, so 8 to 16 stay in flight and each use waits
            // only for its own read (a counted lgkmcnt, never 0 in the loop).
            const uint32_t per_pass = steps / 8, groups = (uint32_t)iters * per_pass;
            mt_vec a[8], b[8];
            uint32_t g = 0;  // group within the pass
#define LS_LOAD(r)                                            \
    do {                                                      \
        _Pragma("unroll") for (int u = 0; u < 8; ++u)(r)[u] = v[(g * 8 + u) * 256]; \
        if (++g == per_pass) g = 0;                           \
    } while (0)
#define LS_SUM(r) \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) s = ls_sum(s, (r)[u])
            uint32_t n = 0;
            LS_LOAD(a);
            for (; n + 2 < groups; n += 2) {
                // the scheduler otherwise sums first and ends on lgkmcnt(0)
                LS_LOAD(b);
                __builtin_amdgcn_sched_barrier(0);
                LS_SUM(a);
                __builtin_amdgcn_sched_barrier(0);
                LS_LOAD(a);
                __builtin_amdgcn_sched_barrier(0);
                LS_SUM(b);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (n + 1 < groups) {
                LS_LOAD(b);
                LS_SUM(a);
                LS_SUM(b);
            } else {
                LS_SUM(a);
            }
#undef LS_LOAD
#undef LS_SUM
        } else {
            for (int it = 0; it < iters; ++it)
                for (uint32_t k = 0; k < steps; ++k) s = ls_sum(s, v[k * 256]);
        }
        c[LS_STREAM] = s;
    }
    __syncthreads();
    const ms_clock t1 = ms_stamp();

    // reduce: lanes by shuffle, the four waves through LDS
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int p = 0; p < LS_PHASES; ++p) c[p] += __shfl_xor(c[p], o);
        d.bad += __shfl_xor(d.bad, o);
        const mt_u64 key = __shfl_xor(d.key, o);
        if (key < d.key) d.key = key;
        d.x |= __shfl_xor(d.x, o);
    }
    mt_u64* red = reinterpret_cast<mt_u64*>(ls_mem);
    const int slots = LS_PHASES + 3;
    if ((t & 63) == 0) {
        mt_u64* mine = red + (t >> 6) * slots;
#pragma unroll
        for (int p = 0; p < LS_PHASES; ++p) mine[p] = c[p];
        mine[LS_PHASES] = d.bad;
        mine[LS_PHASES + 1] = d.key;
        mine[LS_PHASES + 2] = d.x;
    }
    __syncthreads();
    if (t == 0) {
        na_lds_record rec;
        for (int p = 0; p < LS_PHASES; ++p)
            rec.checksum[p] = red[p] + red[slots + p] + red[2 * slots + p] + red[3 * slots + p];
        mt_u64 bad = 0, key = ~0ULL, xm = 0;
        for (int wv = 0; wv < 4; ++wv) {
            bad += red[wv * slots + LS_PHASES];
            if (red[wv * slots + LS_PHASES + 1] < key) key = red[wv * slots + LS_PHASES + 1];
            xm |= red[wv * slots + LS_PHASES + 2];
        }
        rec.bad_words = bad;
        rec.first_bad_offset = bad ? (key & 0xFFFFFFFFULL) : ~0ULL;
        rec.bad_phase = bad ? (uint32_t)(key >> 32) : ~0u;
        rec.xor_mask = xm;
        rec.workgroup = blockIdx.x;
        ms_record_cu(rec, t0, t1, at);
        records[blockIdx.x] = rec;
    }
#else
    // wrong arch: checksums no reference produces, so verification fails
    if (threadIdx.x == 0) {
        na_lds_record rec = {};
        for (int p = 0; p < LS_PHASES; ++p) rec.checksum[p] = ~0ULL;
        records[blockIdx.x] = rec;
    }
#endif
}
