// MFMA operand traits for the MI355X node agent (included from agent.hip and
// mfmasweep.h): the vector typedefs, the kind codes of the single-wave
// checks, and one struct per operand kind carrying the fragment type `frag`,
// a branch-free set(frag&, i, value) for element i of a lane's fragment
// (value a small integer, exact in every format here; a fragment starts
// zeroed), the mfma() call, M = N as MN, K, the elements per lane PER_LANE,
// the accumulator type `acc` with its 32-bit element type `word`, and the
// C/D row map d_row().
//
// Per-lane maps, all kinds: lane l holds PER_LANE consecutive k of one row of
// A and of one column of B — row of A = column of B = l % MN,
// k = (l / MN) * PER_LANE + i — and accumulator register r of lane l is
// D[d_row(l, r)][l % MN].

#pragma once

#include <hip/hip_runtime.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// Kinds of na_mfma_check_run / na_mfma_check_verify
// (gpu_provisioner_amd/nodeagent.py mirrors them in MFMA_CHECK_KINDS).
enum {
    NA_MFMA_F32_UNIFORM = 0,
    NA_MFMA_BF16_UNIFORM,
    NA_MFMA_FP8_UNIFORM,
    NA_MFMA_BF16_TILE,
    NA_MFMA_F16_TILE,
    NA_MFMA_FP8_TILE,
    NA_MFMA_I8_TILE,
    NA_MFMA_BF16_TILE32,
    NA_MFMA_MX_TILE,     // E8M0 scale of A 127 = 1.0
    NA_MFMA_MX_TILE_X2,  // E8M0 scale of A 128 = 2.0
    NA_MFMA_KINDS
};

__device__ __host__ inline unsigned char e4m3(int v) {
    // encodings for -3..3 (sign | exp(bias 7) | 3-bit mantissa)
    switch (v) {
        case 0: return 0x00;
        case 1: return 0x38;
        case 2: return 0x40;
        case 3: return 0x44;
        case -1: return 0xB8;
        case -2: return 0xC0;
        default: return 0xC4;  // -3
    }
}

// e4m3()'s seven encodings packed into one constant (folded at compile
// time), so the fragment set-up stays branch-free.
__device__ inline unsigned long long e4m3_byte(int v) {
    unsigned long long table = 0;
#pragma unroll
    for (int x = -3; x <= 3; ++x) table |= (unsigned long long)e4m3(x) << (8 * (x + 3));
    return (table >> (8 * (v + 3))) & 0xFF;
}

// C/D of the 16x16 family: col = l&15, row = (l>>4)*4 + r, 4 registers.
struct mfma_16x16 {
    typedef f32x4 acc;
    typedef float word;
    enum { MN = 16 };
    static __device__ int d_row(int l, int r) { return (l >> 4) * 4 + r; }
};

// Eight bf16 / f16 per lane; eight E4M3 bytes per lane in one i64, element
// i at byte i.
struct mfma_bf16_frag {
    typedef bf16x8 frag;
    enum { PER_LANE = 8 };
    static __device__ void set(frag& f, int i, int v) { f[i] = (__bf16)(float)v; }
};
struct mfma_f16_frag {
    typedef f16x8 frag;
    enum { PER_LANE = 8 };
    static __device__ void set(frag& f, int i, int v) { f[i] = (_Float16)(float)v; }
};
struct mfma_fp8_frag {
    typedef long frag;
    enum { PER_LANE = 8 };
    static __device__ void set(frag& f, int i, int v) { f |= (long)e4m3_byte(v) << (8 * i); }
};

// v_mfma_f32_16x16x4_f32: one f32 per lane, k = l>>4.
struct mfma_f32_16x16x4 : mfma_16x16 {
    typedef float frag;
    enum { K = 4, PER_LANE = 1 };
    static __device__ void set(frag& f, int, int v) { f = (float)v; }
    static __device__ acc mfma(frag a, frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
};

// v_mfma_f32_16x16x32_bf16, gfx950's 2xK form: the CDNA4 training workhorse.
struct mfma_bf16_16x16x32 : mfma_16x16, mfma_bf16_frag {
    enum { K = 32 };
    static __device__ acc mfma(frag a, frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

struct mfma_f16_16x16x32 : mfma_16x16, mfma_f16_frag {
    enum { K = 32 };
    static __device__ acc mfma(frag a, frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

// v_mfma_f32_16x16x32_fp8_fp8 (E4M3): the serving path.
struct mfma_fp8_16x16x32 : mfma_16x16, mfma_fp8_frag {
    enum { K = 32 };
    static __device__ acc mfma(frag a, frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
    }
};

// v_mfma_i32_16x16x64_i8, CDNA4's 2xK int8 path: 16 per-lane elements
// packed 4 per i32.
struct mfma_i8_16x16x64 : mfma_16x16 {
    typedef i32x4 frag;
    typedef i32x4 acc;
    typedef int word;
    enum { K = 64, PER_LANE = 16 };
    static __device__ void set(frag& f, int i, int v) {
        f[i / 4] |= (int)(unsigned char)(signed char)v << (8 * (i % 4));
    }
    static __device__ acc mfma(frag a, frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
    }
};

// v_mfma_f32_32x32x16_bf16: same pipes, the OTHER tile shape. C/D per the
// ISA: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5), 16 registers.
struct mfma_bf16_32x32x16 : mfma_bf16_frag {
    typedef f32x16 acc;
    typedef float word;
    enum { MN = 32, K = 16 };
    static __device__ int d_row(int l, int r) { return (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); }
    static __device__ acc mfma(frag a, frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

// v_mfma_scale_f32_16x16x128_f8f6f4 (gfx950-only): the ONLY large-K
// low-precision MFMA and the fp4/fp6/MX serving pipe, here on fp8-e4m3
// data: 32 per-lane bytes in <8 x i32>, element i at byte i. scale_a is the
// E8M0 exponent of every block of A (127 = 1.0, 128 doubles the result);
// B's is fixed at 1.0.
struct mfma_mx_16x16x128 : mfma_16x16 {
    typedef i32x8 frag;
    enum { K = 128, PER_LANE = 32 };
    static __device__ void set(frag& f, int i, int v) {
        f[i / 4] |= (int)e4m3_byte(v) << (8 * (i % 4));
    }
    static __device__ acc mfma(frag a, frag b, acc c, int scale_a) {
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a, b, c, /*cbsz=*/0, /*blgp=*/0, /*opselA=*/0, scale_a * 0x01010101, /*opselB=*/0,
            0x7F7F7F7F);
    }
};
