// Chip-wide cache sweep for the MI355X node agent (included from agent.hip).
//
// The other sweeps test what sits inside a CU, the HBM memtest what sits
// behind the caches: it streams gigabytes with nontemporal accesses, each byte
// once, so that caches do not matter. This one tests what lies between: the
// vector L1 of every CU, the L2 of every XCD, the write-through and refill
// path from L2 to the fabric, global atomics, the scalar data cache, and the
// path by which data written on one XCD is read on another. One workgroup at
// a time owns a CU (it holds the whole per-workgroup LDS allocation, the
// placement device of every sweep) and a slice of device memory of its own,
// small enough to stay in cache, and leaves one record per launch: a checksum
// per phase, the CU it ran on, an in-kernel diagnosis of the first wrong word,
// and two clock deltas around a read-only streaming phase. The host
// recomputes every checksum exactly, so a bad cache is attributed to (XCC,
// SE, SH, CU) and phase. The records are na_lds_record: the shape is the LDS
// sweep's.
//
// Specification (normative — tests/test_nodeagent_cachesweep.py carries an
// independent numpy copy); arithmetic mod 2^64, G = 0x9E3779B97F4A7C15,
// mix64 = mt_mix64 of memtest.h.
//
//   The agent allocates workgroups * slice_bytes of device memory; workgroup
//   w owns slice w. S = slice_bytes (a multiple of 4096 up to 1 MiB),
//   W = S / 4 words, C = W / 256, t = thread 0..255, wave v = t >> 6.
//   g(w, i)   = w * W + i: the global word index of word i of slice w
//   pat(p, g) = (uint32)(mix64(seed*G + p*2^40 + g) >> 32)
//               Every word carries its own address chip-wide: a cache that
//               returns another line, set or slice reads as a mismatch, not
//               only a flipped bit.
//   perm(t)   = (t + 67) & 255: the read-back permutation of the LDS sweep.
//   A 16-byte vector u is words 4u..4u+3, its lo = w0 | w1<<32 and
//   hi = w2 | w3<<32. A step is one vector per thread, 4 KiB: step k < C/4
//   has thread t at vector 256k+t (stores, and the stream's loads) or
//   256k+perm(t) (every other load).
//
// Each thread folds what it reads, in read order, as c = c*G + value; the
// phase checksum is the sum of c over the 256 threads (stream sums instead,
// scalar has one c per wave). Phases 0-5 run in launch A, phase 6 in launch B:
//
//   l1      Region: the first min(S, 16 KiB) of the slice. For pol in (0, ~0):
//           plain 16-byte stores of pat(0, .) ^ pol; vmcnt(0); barrier; 4
//           passes of plain 16-byte loads (no sc bits, no nt), folding lo then
//           hi; barrier. Passes 2-4 are served by the CU's 32 KiB L1. One
//           checksum runs through both polarities, here and below.
//   l2      The whole slice, pattern 1, both polarities, plain stores. Two
//           passes of sc1 16-byte global loads: they bypass the L1 and are
//           served by the XCD's L2.
//   wt      Pattern 2, both polarities, stored with sc0 sc1 16-byte stores:
//           write-through, and the line is dropped from L2. One pass of plain
//           loads then refills from the fabric side.
//   atomic  Pattern 3. Zero the slice, vmcnt(0), barrier. Step k < C: thread
//           t does a no-return agent-scope atomic add u32 of
//           a = pat(3, g(w, 256k+t)) to word 256k+t; then, with no barrier in
//           between, step k < C: it adds pat(3, g(w, i)) >> 16 to word
//           i = 256k + ((t+64) & 255), a word of the next wave's. vmcnt(0),
//           barrier, one pass of sc1 loads as in l2. Every word ends as
//           a + (a >> 16) mod 2^32.
//   scalar  The host fills a second, read-only buffer of CS_TABLE_WORDS words
//           with pat(4, j) and copies it to the device before the launch; the
//           kernel never writes it. Wave v reads the whole table with scalar
//           loads (s_load_dwordx8: a uniform address in the constant address
//           space), starting at word 256 * ((w + v) mod 16) and wrapping, and
//           folds every word in read order. The checksum is the sum over the
//           four waves. The size of the scalar data cache is in none of our
//           sources: the 16 KiB table is a choice, not a claim of coverage.
//   stream  Pattern 5, plain 16-byte stores, vmcnt(0), barrier. `iters`
//           passes of sc1 16-byte loads, thread t reading vector 256k+t; the
//           thread adds every lo and hi it reads into one 64-bit sum and the
//           checksum is the sum over threads. s_memtime / s_memrealtime are
//           read after the barrier before the first pass and after the
//           barrier behind the last.
//   xread   Launch B, after launch A has completed on the same stream: the
//           kernel boundary is the only synchronisation, and nothing in
//           either kernel waits for another workgroup. Workgroup w reads
//           slice (w + 1) mod workgroups, which still holds the pattern-5
//           image, with one pass of plain 16-byte loads, stamped around the
//           phase. Workgroups are dealt round-robin over the XCDs, so for
//           two or more the writer normally ran on another XCD; both
//           launches' records carry xcc, so the verify knows.
//
// l1, l2, wt, xread and the read-back of atomic also compare every word they
// read with its expected value: bad_words counts the mismatches,
// first_bad_offset is the byte offset within the slice of the first (earliest
// phase, then lowest offset), bad_phase that phase and xor_mask the OR of
// got ^ want. That is diagnosis for the operator; the verdict is the host's
// comparison of the checksums.
//
// A record of launch A has checksum[6] = checksum[7] = 0. A record of launch
// B has only checksum[6], its own location, clocks and diagnosis, and
// workgroup = w.
//
// Every access to the slices is an asm volatile statement with its cache
// bits spelled out, so a pass is a pass: the compiler can neither merge the
// repeated loads nor choose other bits. A load statement ends in its own
// s_waitcnt vmcnt(0): its results are complete when the compiler first sees
// them.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "memtest.h"
#include "nodeagent.h"
#include "sweep_common.h"

#define CS_BLOCK MS_BLOCK   // four waves, as every sweep
#define CS_GRANULE 4096     // slice_bytes is a multiple of this: one 16-byte access per thread
#define CS_MAX_BYTES (1 << 20)
#define CS_L1_BYTES (16 * 1024)  // the l1 phase's region: half of a CU's L1
#define CS_L1_PASSES 4
#define CS_L2_PASSES 2
#define CS_TABLE_WORDS 4096      // the scalar phase's table, 16 KiB
#define CS_TABLE_STARTS 16       // a wave starts at a multiple of 256 words
#define CS_PERM(t) (((t) + 67u) & 255u)

enum { CS_L1, CS_L2, CS_WT, CS_ATOMIC, CS_SCALAR, CS_STREAM, CS_XREAD, CS_PHASES };

static_assert(CS_PHASES == NA_CACHE_PHASES && CS_GRANULE == NA_CACHE_GRANULE &&
                  CS_MAX_BYTES == NA_CACHE_MAX_BYTES && CS_TABLE_WORDS == NA_CACHE_TABLE_WORDS,
              "nodeagent.h tells callers otherwise");
static_assert(CS_PHASES <= NA_LDS_PHASES, "the record is na_lds_record");

// g: the global word index, or the table index for pattern CS_SCALAR.
__device__ __host__ inline uint32_t cs_pat(mt_u64 base, int pat, mt_u64 g) {
    return (uint32_t)(mt_mix64(base + ((mt_u64)pat << 40) + g) >> 32);
}

#if defined(__gfx950__)

typedef uint32_t cs_vec __attribute__((ext_vector_type(4)));  // one 16-byte vector
typedef uint32_t cs_x8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(4))) cs_x8 cs_const_x8;

// The vectors at byte offsets off[0..N-1] of `slice` (uniform), complete on
// return. BITS is the instruction's cache policy: "" or " sc1".
#define CS_LOAD1(BITS, slice, off, v)                                                        \
    asm volatile("global_load_dwordx4 %0, %1, %2" BITS "\n\ts_waitcnt vmcnt(0)"              \
                 : "=&v"((v)[0])                                                             \
                 : "v"((off)[0]), "s"(slice)                                                 \
                 : "memory")
#define CS_LOAD4(BITS, slice, off, v)                                                        \
    asm volatile("global_load_dwordx4 %0, %4, %8" BITS "\n\t"                                \
                 "global_load_dwordx4 %1, %5, %8" BITS "\n\t"                                \
                 "global_load_dwordx4 %2, %6, %8" BITS "\n\t"                                \
                 "global_load_dwordx4 %3, %7, %8" BITS "\n\t"                                \
                 "s_waitcnt vmcnt(0)"                                                        \
                 : "=&v"((v)[0]), "=&v"((v)[1]), "=&v"((v)[2]), "=&v"((v)[3])                \
                 : "v"((off)[0]), "v"((off)[1]), "v"((off)[2]), "v"((off)[3]), "s"(slice)    \
                 : "memory")
// the stream's: sc1, eight in flight
#define CS_LOAD8_SC1(slice, off, v)                                                          \
    asm volatile("global_load_dwordx4 %0, %8, %16 sc1\n\t"                                   \
                 "global_load_dwordx4 %1, %9, %16 sc1\n\t"                                   \
                 "global_load_dwordx4 %2, %10, %16 sc1\n\t"                                  \
                 "global_load_dwordx4 %3, %11, %16 sc1\n\t"                                  \
                 "global_load_dwordx4 %4, %12, %16 sc1\n\t"                                  \
                 "global_load_dwordx4 %5, %13, %16 sc1\n\t"                                  \
                 "global_load_dwordx4 %6, %14, %16 sc1\n\t"                                  \
                 "global_load_dwordx4 %7, %15, %16 sc1\n\t"                                  \
                 "s_waitcnt vmcnt(0)"                                                        \
                 : "=&v"((v)[0]), "=&v"((v)[1]), "=&v"((v)[2]), "=&v"((v)[3]),               \
                   "=&v"((v)[4]), "=&v"((v)[5]), "=&v"((v)[6]), "=&v"((v)[7])                \
                 : "v"((off)[0]), "v"((off)[1]), "v"((off)[2]), "v"((off)[3]),               \
                   "v"((off)[4]), "v"((off)[5]), "v"((off)[6]), "v"((off)[7]), "s"(slice)    \
                 : "memory")

template <bool SC1>
__device__ inline void cs_load1(const void* slice, const uint32_t* off, cs_vec* v) {
    if (SC1)
        CS_LOAD1(" sc1", slice, off, v);
    else
        CS_LOAD1("", slice, off, v);
}
template <bool SC1>
__device__ inline void cs_load4(const void* slice, const uint32_t* off, cs_vec* v) {
    if (SC1)
        CS_LOAD4(" sc1", slice, off, v);
    else
        CS_LOAD4("", slice, off, v);
}

// One 16-byte store; WT = write-through (sc0 sc1). Not waited for: cs_drain.
template <bool WT>
__device__ inline void cs_store(void* slice, uint32_t off, cs_vec v) {
    if (WT)
        asm volatile("global_store_dwordx4 %0, %1, %2 sc0 sc1" ::"v"(off), "v"(v), "s"(slice)
                     : "memory");
    else
        asm volatile("global_store_dwordx4 %0, %1, %2" ::"v"(off), "v"(v), "s"(slice) : "memory");
}

// No-return, no sc bit: agent scope, performed at the L2.
__device__ inline void cs_atomic_add(void* slice, uint32_t off, uint32_t a) {
    asm volatile("global_atomic_add %0, %1, %2" ::"v"(off), "v"(a), "s"(slice) : "memory");
}

// This wave's stores and atomics have completed; then the workgroup's.
__device__ inline void cs_drain() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// key = phase << 32 | byte offset of the first bad word; ~0 = none
struct cs_diag {
    mt_u64 bad, key, x;
};

__device__ inline void cs_check(cs_diag& d, int phase, uint32_t word, uint32_t got,
                                uint32_t want) {
    const uint32_t x = got ^ want;
    if (x == 0) return;
    d.bad++;
    d.x |= x;
    const mt_u64 key = ((mt_u64)phase << 32) | ((mt_u64)word * 4);
    if (key < d.key) d.key = key;
}

// want(i): what word i of the slice holds.
template <bool WT, typename WANT>
__device__ inline void cs_fill(void* slice, uint32_t t, uint32_t steps, WANT want) {
    for (uint32_t k = 0; k < steps; ++k) {
        const uint32_t i = 4 * (k * 256 + t);
        cs_vec v = {want(i), want(i + 1), want(i + 2), want(i + 3)};
        cs_store<WT>(slice, i * 4, v);
    }
    cs_drain();
}

__device__ inline mt_u64 cs_fold(mt_u64 c, cs_vec v) {
    c = c * MS_G + ((mt_u64)v.x | ((mt_u64)v.y << 32));
    return c * MS_G + ((mt_u64)v.z | ((mt_u64)v.w << 32));
}

__device__ inline mt_u64 cs_sum(mt_u64 s, cs_vec v) {
    return s + ((mt_u64)v.x | ((mt_u64)v.y << 32)) + ((mt_u64)v.z | ((mt_u64)v.w << 32));
}

// One pass over the leading `steps` steps through perm: fold and compare.
template <bool SC1, typename WANT>
__device__ inline mt_u64 cs_read(const void* slice, uint32_t t, uint32_t steps, mt_u64 c,
                                 int phase, cs_diag& d, WANT want) {
    const uint32_t u0 = CS_PERM(t);
    uint32_t k = 0;
    while (k < steps) {
        const uint32_t n = steps - k >= 4 ? 4 : 1;
        uint32_t off[4];
        cs_vec v[4];
        for (uint32_t m = 0; m < 4; ++m) off[m] = ((k + m) * 256 + u0) * 16;
        if (n == 4)
            cs_load4<SC1>(slice, off, v);
        else
            cs_load1<SC1>(slice, off, v);
        for (uint32_t m = 0; m < n; ++m) {
            c = cs_fold(c, v[m]);
            const uint32_t i = off[m] / 4;
            cs_check(d, phase, i, v[m].x, want(i));
            cs_check(d, phase, i + 1, v[m].y, want(i + 1));
            cs_check(d, phase, i + 2, v[m].z, want(i + 2));
            cs_check(d, phase, i + 3, v[m].w, want(i + 3));
        }
        k += n;
    }
    return c;
}

// The records' tail: lanes by shuffle, the four waves through LDS (`red`,
// 4 x (CS_PHASES + 3) words of 8 bytes), one record by thread 0.
__device__ inline void cs_finish(na_lds_record* records, mt_u64* red, mt_u64* c, cs_diag d,
                                 ms_clock t0, ms_clock t1, ms_hw_where at) {
    const uint32_t t = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int p = 0; p < CS_PHASES; ++p) c[p] += __shfl_xor(c[p], o);
        d.bad += __shfl_xor(d.bad, o);
        const mt_u64 key = __shfl_xor(d.key, o);
        if (key < d.key) d.key = key;
        d.x |= __shfl_xor(d.x, o);
    }
    const int slots = CS_PHASES + 3;
    __syncthreads();
    if ((t & 63) == 0) {
        mt_u64* mine = red + (t >> 6) * slots;
#pragma unroll
        for (int p = 0; p < CS_PHASES; ++p) mine[p] = c[p];
        mine[CS_PHASES] = d.bad;
        mine[CS_PHASES + 1] = d.key;
        mine[CS_PHASES + 2] = d.x;
    }
    __syncthreads();
    if (t == 0) {
        na_lds_record rec;
        for (int p = 0; p < NA_LDS_PHASES; ++p) rec.checksum[p] = 0;
        for (int p = 0; p < CS_PHASES; ++p)
            rec.checksum[p] = red[p] + red[slots + p] + red[2 * slots + p] + red[3 * slots + p];
        mt_u64 bad = 0, key = ~0ULL, xm = 0;
        for (int wv = 0; wv < 4; ++wv) {
            bad += red[wv * slots + CS_PHASES];
            if (red[wv * slots + CS_PHASES + 1] < key) key = red[wv * slots + CS_PHASES + 1];
            xm |= red[wv * slots + CS_PHASES + 2];
        }
        rec.bad_words = bad;
        rec.first_bad_offset = bad ? (key & 0xFFFFFFFFULL) : ~0ULL;
        rec.bad_phase = bad ? (uint32_t)(key >> 32) : ~0u;
        rec.xor_mask = xm;
        rec.workgroup = blockIdx.x;
        ms_record_cu(rec, t0, t1, at);
        records[blockIdx.x] = rec;
    }
}

#endif  // __gfx950__

// wrong arch: checksums no reference produces, so verification fails
__device__ inline void cs_wrong_arch(na_lds_record* records) {
    if (threadIdx.x == 0) {
        na_lds_record rec = {};
        for (int p = 0; p < CS_PHASES; ++p) rec.checksum[p] = ~0ULL;
        records[blockIdx.x] = rec;
    }
}

// Launch A. records: gridDim.x entries. mem: gridDim.x slices of slice_bytes
// (a multiple of CS_GRANULE up to CS_MAX_BYTES), 16-byte aligned. table:
// CS_TABLE_WORDS words of pattern CS_SCALAR, read-only. base = seed * G
// (hoisted to the host). Launch with CS_BLOCK threads and the whole
// per-workgroup LDS allocation as dynamic shared memory; iters >= 1.
__global__ void __launch_bounds__(CS_BLOCK)
cache_sweep_kernel(na_lds_record* __restrict__ records, unsigned char* __restrict__ mem,
                   const uint32_t* __restrict__ table, mt_u64 base, uint32_t slice_bytes,
                   int iters) {
#if defined(__gfx950__)
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
    const ms_hw_where at = ms_where();
    const uint32_t t = threadIdx.x, W = slice_bytes / 4, steps = slice_bytes / CS_GRANULE;
    const mt_u64 g0 = (mt_u64)blockIdx.x * W;  // g(w, 0)
    void* slice = mem + (size_t)blockIdx.x * slice_bytes;
    mt_u64 c[CS_PHASES] = {};
    cs_diag d = {0, ~0ULL, 0};

    // l1: a region the L1 holds, read four times
    {
        const uint32_t l1_steps = (slice_bytes < CS_L1_BYTES ? slice_bytes : CS_L1_BYTES) / CS_GRANULE;
        for (int p = 0; p < 2; ++p) {
            const uint32_t pol = p ? ~0u : 0u;
            auto want = [=](uint32_t i) { return cs_pat(base, CS_L1, g0 + i) ^ pol; };
            cs_fill<false>(slice, t, l1_steps, want);
            for (int pass = 0; pass < CS_L1_PASSES; ++pass)
                c[CS_L1] = cs_read<false>(slice, t, l1_steps, c[CS_L1], CS_L1, d, want);
            __syncthreads();
        }
    }

    // l2: the whole slice, read twice past the L1
    for (int p = 0; p < 2; ++p) {
        const uint32_t pol = p ? ~0u : 0u;
        auto want = [=](uint32_t i) { return cs_pat(base, CS_L2, g0 + i) ^ pol; };
        cs_fill<false>(slice, t, steps, want);
        for (int pass = 0; pass < CS_L2_PASSES; ++pass)
            c[CS_L2] = cs_read<true>(slice, t, steps, c[CS_L2], CS_L2, d, want);
        __syncthreads();
    }

    // wt: written through the L2, read back from behind it
    for (int p = 0; p < 2; ++p) {
        const uint32_t pol = p ? ~0u : 0u;
        auto want = [=](uint32_t i) { return cs_pat(base, CS_WT, g0 + i) ^ pol; };
        cs_fill<true>(slice, t, steps, want);
        c[CS_WT] = cs_read<false>(slice, t, steps, c[CS_WT], CS_WT, d, want);
        __syncthreads();
    }

    // atomic: every word receives one add from each of two waves
    {
        cs_fill<false>(slice, t, steps, [](uint32_t) { return 0u; });
        const uint32_t C = W / 256;
        for (uint32_t k = 0; k < C; ++k) {
            const uint32_t i = k * 256 + t;
            cs_atomic_add(slice, i * 4, cs_pat(base, CS_ATOMIC, g0 + i));
        }
        for (uint32_t k = 0; k < C; ++k) {
            const uint32_t i = k * 256 + ((t + 64) & 255);
            cs_atomic_add(slice, i * 4, cs_pat(base, CS_ATOMIC, g0 + i) >> 16);
        }
        cs_drain();
        c[CS_ATOMIC] = cs_read<true>(slice, t, steps, 0, CS_ATOMIC, d, [=](uint32_t i) {
            const uint32_t a = cs_pat(base, CS_ATOMIC, g0 + i);
            return a + (a >> 16);
        });
        __syncthreads();
    }

    // scalar: the table through the scalar data cache, one fold per wave.
    // Address and value are uniform and the pointer is in the constant
    // address space, so the loads are s_load_dwordx8 and the fold scalar ALU.
    {
        const cs_const_x8* tab = (const cs_const_x8*)table;
        const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
        const uint32_t start = 256 * ((blockIdx.x + wave) % CS_TABLE_STARTS);
        mt_u64 cc = 0;
        for (uint32_t j = 0; j < CS_TABLE_WORDS; j += 8) {
            const cs_x8 v = tab[((start + j) % CS_TABLE_WORDS) / 8];
#pragma unroll
            for (int u = 0; u < 8; ++u) cc = cc * MS_G + v[u];
        }
        c[CS_SCALAR] = (t & 63) == 0 ? cc : 0;
    }

    // stream: read-only passes from the L2 at rate. The stamps bracket the
    // whole phase of the workgroup, go only into the record, and no output is
    // computed from them.
    cs_fill<false>(slice, t, steps,
                   [=](uint32_t i) { return cs_pat(base, CS_STREAM, g0 + i); });
    const ms_clock t0 = ms_stamp();
    {
        mt_u64 s = 0;
        for (int it = 0; it < iters; ++it) {
            uint32_t k = 0;
            while (k < steps) {
                // eight vectors in flight per thread where the slice has them
                uint32_t off[8];
                cs_vec v[8];
                for (uint32_t m = 0; m < 8; ++m) off[m] = ((k + m) * 256 + t) * 16;
                const uint32_t n = steps - k >= 8 ? 8 : steps - k >= 4 ? 4 : 1;
                if (n == 8)
                    CS_LOAD8_SC1(slice, off, v);
                else if (n == 4)
                    cs_load4<true>(slice, off, v);
                else
                    cs_load1<true>(slice, off, v);
                for (uint32_t m = 0; m < n; ++m) s = cs_sum(s, v[m]);
                k += n;
            }
        }
        c[CS_STREAM] = s;
    }
    __syncthreads();
    const ms_clock t1 = ms_stamp();

    cs_finish(records, reinterpret_cast<mt_u64*>(cs_lds), c, d, t0, t1, at);
#else
    cs_wrong_arch(records);
#endif
}

// Launch B, on the stream of launch A and after it: workgroup w reads the
// slice that workgroup (w + 1) mod gridDim.x left. Arguments as above.
__global__ void __launch_bounds__(CS_BLOCK)
cache_xread_kernel(na_lds_record* __restrict__ records, const unsigned char* __restrict__ mem,
                   mt_u64 base, uint32_t slice_bytes) {
#if defined(__gfx950__)
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
    const ms_hw_where at = ms_where();
    const uint32_t t = threadIdx.x, W = slice_bytes / 4, steps = slice_bytes / CS_GRANULE;
    const uint32_t writer = blockIdx.x + 1 == gridDim.x ? 0 : blockIdx.x + 1;
    const mt_u64 g0 = (mt_u64)writer * W;
    const void* slice = mem + (size_t)writer * slice_bytes;
    mt_u64 c[CS_PHASES] = {};
    cs_diag d = {0, ~0ULL, 0};
    __syncthreads();
    const ms_clock t0 = ms_stamp();
    c[CS_XREAD] = cs_read<false>(slice, t, steps, 0, CS_XREAD, d, [=](uint32_t i) {
        return cs_pat(base, CS_STREAM, g0 + i);
    });
    __syncthreads();
    const ms_clock t1 = ms_stamp();
    cs_finish(records, reinterpret_cast<mt_u64*>(cs_lds), c, d, t0, t1, at);
#else
    cs_wrong_arch(records);
#endif
}
