// What the chip-wide sweep kernels of the MI355X node agent share (mfmasweep.h,
// ldssweep.h, cachesweep.h, valusweep.h): the launch shape, the checksum multiplier, where a
// wave runs, the clock stamp around the timed phase, and how both go into a
// record with the fields cycles, realtime, xcc, se, sh, cu (and simd). The
// host's counterpart is "Shared host side of the chip-wide sweeps" in agent.hip.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "memtest.h"
#include "nodeagent.h"

#define MS_BLOCK 256  // four waves: one per SIMD of the CU
#define MS_WAVES_PER_WG (MS_BLOCK / 64)
static_assert(MS_WAVES_PER_WG == NA_SWEEP_WAVES_PER_WG, "nodeagent.h tells callers otherwise");
#define MS_G 0x9E3779B97F4A7C15ULL
// The LDS of one gfx950 CU. A workgroup launched with more than half of it
// has the CU, and each of its four waves a SIMD, to itself.
#define MS_CU_LDS_BYTES (160 * 1024)

// s_getreg operand: SIZE-1 in 15:11, OFFSET in 10:6, register id in 5:0
// (encodings: amd_device_functions.h). HW_ID is register 4, XCC_ID 20.
#define MS_GETREG(size, offset, reg) ((((size)-1) << 11) | ((offset) << 6) | (reg))

// The CU of any of the sweeps' records, as an 11-bit key.
template <typename R>
static inline uint32_t ms_cu_key(const R& r) {
    return ((r.xcc & 15) << 7) | ((r.se & 3) << 5) | ((r.sh & 1) << 4) | (r.cu & 15);
}

#if defined(__gfx950__)

struct ms_hw_where {
    unsigned hw_id, xcc_id;
};

__device__ inline ms_hw_where ms_where() {
    ms_hw_where at;
    at.hw_id = __builtin_amdgcn_s_getreg(MS_GETREG(32, 0, 4));
    at.xcc_id = __builtin_amdgcn_s_getreg(MS_GETREG(4, 0, 20));
    return at;
}

// s_memtime (shader clock) and s_memrealtime (100 MHz), fenced so that
// nothing is scheduled across the stamp.
struct ms_clock {
    mt_u64 cycles, realtime;
};

__device__ inline ms_clock ms_stamp() {
    ms_clock t;
    __builtin_amdgcn_sched_barrier(0);
    t.cycles = __builtin_amdgcn_s_memtime();
    t.realtime = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

// The clock deltas and the CU into a record. HW_ID: SE in 14:13, SH in 12,
// CU in 11:8, SIMD in 5:4.
template <typename R>
__device__ inline void ms_record_cu(R& rec, ms_clock t0, ms_clock t1, ms_hw_where at) {
    rec.cycles = t1.cycles - t0.cycles;
    rec.realtime = t1.realtime - t0.realtime;
    rec.xcc = at.xcc_id & 15;
    rec.se = (at.hw_id >> 13) & 3;
    rec.sh = (at.hw_id >> 12) & 1;
    rec.cu = (at.hw_id >> 8) & 15;
}

// The same for a record per wave, with the SIMD.
template <typename R>
__device__ inline void ms_record_simd(R& rec, ms_clock t0, ms_clock t1, ms_hw_where at) {
    ms_record_cu(rec, t0, t1, at);
    rec.simd = (at.hw_id >> 4) & 3;
}

#endif  // __gfx950__
