// Chip-wide load sweep for the MI355X node agent (included from agent.hip).
//
// The other sweeps test one unit with the rest of the chip idle. This kernel
// keeps the matrix cores, the LDS and the memory path of every CU busy in the
// same cycles: one workgroup of eight waves per CU at a time, two waves on
// each SIMD. Waves 0..3 run the matrix-core sweep's MFMA chain (ms_wave of
// mfmasweep.h: same operands, folds and checksum, so the reference is that
// sweep's); waves 4..7 stream a slice of pattern-filled device memory through
// LDS and compare every word (the memtest's pattern, comparison and
// accumulator, memtest.h). Every wave leaves an na_mfma_record, and the host
// recomputes every checksum exactly.
//
// Stream waves (normative — tests/test_nodeagent_loadsweep.py carries an
// independent numpy copy). The region is workgroups * slice_bytes bytes of
// the memtest pattern (seed, not inverted), addressed in 16-byte vectors from
// its start; workgroup g owns vectors [g*V, (g+1)*V), V = slice_bytes / 16,
// slice_bytes a multiple of NA_LOAD_GRANULE. Stream wave q = (threadIdx.x>>6)
// - 4, lane l, thread t = q*64 + l; for pass p < passes and step j < V/1024:
//
//   1. four nontemporal 16-byte loads of slice vectors i_k = j*1024 + k*256 + t,
//      k = 0..3;
//   2. written to the wave's own 4 KiB of LDS at byte q*4096 + k*1024 + l*16;
//   3. read back from the slots of lane l' = (l + 17) & 63;
//   4. compared with mt_pattern(g*V + j*1024 + k*256 + q*64 + l') through
//      mt_compare (offsets are region-relative);
//   5. c += lo*G + hi of what came back (mod 2^64, G = MS_G).
//
// After the last pass mt_commit runs into the launch's one mt_accum, c is
// summed over the wave and lane 0 writes stream[g*4 + q]; the record's clocks
// bracket the loop. Expected checksum: passes * sum (lo_i*G + hi_i) over the
// slice's vectors i with (i >> 6) & 3 == q.
//
// outer == 0 switches the matrix waves off, passes == 0 the stream waves: a
// wave of a role that is off writes an all-zero record and does nothing else,
// which gives the "alone" figures from the same kernel.
//
// No workgroup barrier anywhere: the roles have different trip counts, and a
// barrier only one of them reaches would hang the CU. A wave's LDS write and
// its read-back are ordered by the hardware within the wave (LDS instructions
// of one wave complete in order); ld_wave_sync keeps the compiler from
// reordering them. Every loop is bounded by the kernel's arguments.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "memtest.h"
#include "mfmasweep.h"
#include "nodeagent.h"
#include "sweep_common.h"

#define LD_BLOCK (2 * MS_BLOCK)  // eight waves: two per SIMD of the CU
#define LD_UNROLL 4              // vectors in flight per thread
#define LD_STEP_VECS (MS_BLOCK * LD_UNROLL)  // vectors the four stream waves take per step
#define LD_GRANULE (LD_STEP_VECS * 16)
#define LD_MAX_BYTES (16 << 20)
#define LD_LDS_BYTES (MS_WAVES_PER_WG * 64 * LD_UNROLL * 16)  // what the stream waves touch
static_assert(LD_GRANULE == NA_LOAD_GRANULE && LD_MAX_BYTES == NA_LOAD_MAX_BYTES,
              "nodeagent.h tells callers otherwise");

// A vector's contribution to a stream checksum.
__device__ __host__ inline mt_u64 ld_term(mt_u64 lo, mt_u64 hi) { return lo * MS_G + hi; }

#if defined(__gfx950__)

// Orders this wave's LDS accesses before the call against those after it, for
// the compiler only: no instruction, and nothing any other wave waits for.
__device__ inline void ld_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The four vectors thread t of the stream waves takes in step j.
__device__ __forceinline__ void ld_load(mt_vec (&v)[LD_UNROLL], const mt_vec* __restrict__ slice,
                                        uint32_t j, int t) {
#pragma unroll
    for (int k = 0; k < LD_UNROLL; ++k)
        v[k] = __builtin_nontemporal_load(&slice[(size_t)j * LD_STEP_VECS + k * MS_BLOCK + t]);
}

// What a stream wave carries from step to step.
struct ld_state {
    mt_vec* lds;  // the wave's own 4 KiB, as 256 vectors
    int l, back;  // this lane, and the lane whose slots it reads back
    mt_u64 base;
    mt_local m;
    mt_u64 c;
};

// Steps 2 to 5 on the vectors `cur` of one step: through LDS, compared, summed.
// v is the region-relative index of the vector lane 0 of this wave loaded at
// k = 0.
__device__ __forceinline__ void ld_step(const mt_vec (&cur)[LD_UNROLL], mt_u64 v, ld_state& s) {
#pragma unroll
    for (int k = 0; k < LD_UNROLL; ++k) s.lds[k * 64 + s.l] = cur[k];
    ld_wave_sync();
    mt_vec got[LD_UNROLL];
#pragma unroll
    for (int k = 0; k < LD_UNROLL; ++k) got[k] = s.lds[k * 64 + s.back];
    ld_wave_sync();
#pragma unroll
    for (int k = 0; k < LD_UNROLL; ++k) {
        const mt_u64 vk = v + k * MS_BLOCK + s.back;
        mt_compare(got[k], mt_pattern(vk, s.base, 0), vk, s.m);
        s.c += ld_term(got[k].x, got[k].y);
    }
}

// One stream wave: q in 0..3, lds its own 4 KiB as 256 vectors.
__device__ __forceinline__ void ld_stream_wave(na_mfma_record* __restrict__ stream,
                                               const mt_vec* __restrict__ region, mt_u64 base,
                                               uint32_t steps, int passes, mt_accum* acc,
                                               mt_vec* lds, int q) {
    const ms_hw_where at = ms_where();
    const int l = threadIdx.x & 63, t = q * 64 + l;
    const mt_u64 g = blockIdx.x;
    const mt_u64 v0 = g * steps * LD_STEP_VECS;  // the slice's first vector in the region
    const mt_vec* __restrict__ slice = region + v0;
    ld_state s = {lds, l, (l + 17) & 63, base, {0, ~0ULL, 0}, 0};

    const ms_clock t0 = ms_stamp();

    // Software-pipelined by one step over two sets of registers, so that no
    // copy waits for a load: the four loads of the next step are in flight
    // while this one goes through LDS and the comparison. Steps run in the
    // order pass by pass, j = 0..steps-1 in each. The loads are
    // unconditional, so that the wait ahead of a step counts on the next
    // step's four being the newest: after the last step one or two sets are
    // loaded (from inside the slice: j1, j2 < steps) and never used.
    const mt_u64 total = (mt_u64)passes * steps;
    mt_vec a[LD_UNROLL], b[LD_UNROLL];
    ld_load(a, slice, 0, t);
    uint32_t j = 0;
    for (mt_u64 it = 0; it < total; it += 2) {
        const uint32_t j1 = j + 1 == steps ? 0 : j + 1, j2 = j1 + 1 == steps ? 0 : j1 + 1;
        ld_load(b, slice, j1, t);
        ld_step(a, v0 + (mt_u64)j * LD_STEP_VECS + q * 64, s);
        if (it + 1 == total) break;
        ld_load(a, slice, j2, t);
        ld_step(b, v0 + (mt_u64)j1 * LD_STEP_VECS + q * 64, s);
        j = j2;
    }

    const ms_clock t1 = ms_stamp();

    mt_commit(s.m, acc);
    mt_u64 c = s.c;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (l == 0) {
        na_mfma_record rec;
        rec.checksum = c;
        rec.wave = (uint32_t)(g * MS_WAVES_PER_WG + q);
        ms_record_simd(rec, t0, t1, at);
        stream[g * MS_WAVES_PER_WG + q] = rec;
    }
}

#endif  // __gfx950__

// matrix, stream: 4 * gridDim.x records each. region: gridDim.x * steps *
// LD_STEP_VECS vectors of the memtest pattern. base = seed * G (hoisted to
// the host). Launch with LD_BLOCK threads and more than half of the CU's LDS
// (at least LD_LDS_BYTES) as dynamic shared memory: the workgroup then has
// the CU to itself, two of its waves on each SIMD.
template <int DTYPE>
__global__ void __launch_bounds__(LD_BLOCK)
load_sweep_kernel(na_mfma_record* __restrict__ matrix, na_mfma_record* __restrict__ stream,
                  const mt_vec* __restrict__ region, mt_u64 base, int outer, uint32_t steps,
                  int passes, mt_accum* acc) {
    const int wv = threadIdx.x >> 6, role_wave = wv & (MS_WAVES_PER_WG - 1);
    const bool is_matrix = wv < MS_WAVES_PER_WG;
    na_mfma_record* const mine =
        (is_matrix ? matrix : stream) + (size_t)blockIdx.x * MS_WAVES_PER_WG + role_wave;
#if defined(__gfx950__)
    extern __shared__ mt_vec ld_lds[];
    if ((is_matrix ? outer : passes) == 0) {
        // a role that is off
        if ((threadIdx.x & 63) == 0) *mine = na_mfma_record{};
    } else if (is_matrix) {
        ms_wave<DTYPE>(matrix, base, (mt_u64)blockIdx.x * MS_WAVES_PER_WG + wv, outer);
    } else {
        ld_stream_wave(stream, region, base, steps, passes, acc, ld_lds + role_wave * 64 * LD_UNROLL,
                       role_wave);
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
