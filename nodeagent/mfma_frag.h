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
// D[d_row(l, r)][l % MN]. (The block-scaled traits at the end of this file
// state their own k maps: 8-bit operands of the f8f6f4 instruction are not
// consecutive in k.)

#pragma once

#include <hip/hip_runtime.h>

#include "mx_formats.h"

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

// ---------------------------------------------------------------------------
// Block-scaled MX operands in every format of the f8f6f4 instructions
// (encodings, packing and the scale register: mx_formats.h)
// ---------------------------------------------------------------------------

// Kinds of na_mx_check_run / na_mx_check_verify
// (gpu_provisioner_amd/nodeagent.py mirrors them in MX_CHECK_KINDS).
enum {
    NA_MX_FP4 = 0,    // 16x16x128 tiles: E2M1 x E2M1
    NA_MX_FP6,        // E2M3 x E2M3
    NA_MX_BF6,        // E3M2 x E3M2
    NA_MX_BF8,        // E5M2 x E5M2
    NA_MX_FP8_FP4,    // A in E4M3, B in E2M1: W4A8 serving
    NA_MX_FP4_32,     // 32x32x64 tile, E2M1 x E2M1
    NA_MX_FP4_CODES,  // every code of E2M1 through A's decoder
    NA_MX_FP6_CODES,  // every code of E2M3
    NA_MX_BF6_CODES,  // every code of E3M2
    NA_MX_KINDS
};

// A lane's 32 elements and its scale register. Lanes l with the same l / MN
// form a lane group g; the scale register of a lane in group g is the scale
// of K block g (k / 32 == g) of the lane's row or column. Which k a lane's
// elements are depends on the element width (measured on MI355X with the
// bf8 kind below, whose per-block scales differ):
//   4- and 6-bit formats: k = 32 g + i, so a lane holds exactly the block its
//     scale register scales;
//   8-bit formats (16x16x128): k = 16 g + (i & 15) + 64 (i >> 4): registers
//     0-3 are 16 consecutive k of block g / 2 and registers 4-7 the 16 at
//     k + 64, of block 2 + g / 2. A lane's scale register then scales a block
//     that other lanes hold.
// With one scale for the whole operand and both operands in one format the
// two maps compute the same D, which is why mfma_mx_16x16x128 above is right
// with the first on E4M3 data.
struct mx_frag {
    i32x8 v;
    int scale;
};

// What both shapes share: A in format FA with its scale in byte OA of the
// scale register, B in FB with its scale in byte OB. set_a / set_b take the
// element's code, scale_a / scale_b the E8M0 byte of block g; k_a / k_b give
// the k of element i of a lane in group g.
template <int FA, int FB, int OA, int OB>
struct mfma_mxs_frag {
    typedef mx_frag frag;
    enum { PER_LANE = 32, FMT_A = FA, FMT_B = FB };
    static __device__ int k_of(int fmt, int g, int i) {
        return mx_bits(fmt) == 8 ? 16 * g + (i & 15) + 64 * (i >> 4) : 32 * g + i;
    }
    static __device__ int k_a(int g, int i) { return k_of(FA, g, i); }
    static __device__ int k_b(int g, int i) { return k_of(FB, g, i); }
    static __device__ void set_a(frag& f, int i, unsigned code) { mx_put(f.v, FA, i, code); }
    static __device__ void set_b(frag& f, int i, unsigned code) { mx_put(f.v, FB, i, code); }
    static __device__ void scale_a(frag& f, int e8m0) { f.scale = mx_scale_word(OA, e8m0); }
    static __device__ void scale_b(frag& f, int e8m0) { f.scale = mx_scale_word(OB, e8m0); }
};

// v_mfma_scale_f32_16x16x128_f8f6f4: four K blocks, lane group g = l / 16.
template <int FA, int FB, int OA, int OB>
struct mfma_mxs_16x16x128 : mfma_16x16, mfma_mxs_frag<FA, FB, OA, OB> {
    enum { K = 128 };
    static __device__ acc mfma(mx_frag a, mx_frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a.v, b.v, c, FA, FB, OA, a.scale,
                                                                OB, b.scale);
    }
};

// v_mfma_scale_f32_32x32x64_f8f6f4: two K blocks, lane group g = l / 32;
// C/D as mfma_bf16_32x32x16. Sub-byte formats only: the k map of 8-bit
// operands has been measured on the 16x16x128 shape alone.
template <int FA, int FB, int OA, int OB>
struct mfma_mxs_32x32x64 : mfma_mxs_frag<FA, FB, OA, OB> {
    static_assert(mx_bits(FA) < 8 && mx_bits(FB) < 8, "8-bit k map of 32x32x64 not established");
    typedef f32x16 acc;
    typedef float word;
    enum { MN = 32, K = 64 };
    static __device__ int d_row(int l, int r) { return mfma_bf16_32x32x16::d_row(l, r); }
    static __device__ acc mfma(mx_frag a, mx_frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.v, b.v, c, FA, FB, OA, a.scale,
                                                               OB, b.scale);
    }
};

// The 16x16x128 instruction for the chip-wide sweep: A and B both in FMT
// (E2M1 or E2M3), every scale 1.0, and a fragment of exactly the 4 or 6
// registers the instruction reads, so eight A and eight B fragments cost 64
// or 96 VGPRs. set() takes the integer value, as the non-scaled traits do.
template <int FMT>
struct mfma_mx1_16x16x128 : mfma_16x16 {
    typedef int frag __attribute__((ext_vector_type(mx_bits(FMT))));
    enum { K = 128, PER_LANE = 32 };
    static __device__ void set(frag& f, int i, int v) { mx_put(f, FMT, i, mx_encode_int(FMT, v)); }
    static __device__ i32x8 widen(frag f) {
        if constexpr (mx_bits(FMT) == 4)
            return __builtin_shufflevector(f, f, 0, 1, 2, 3, -1, -1, -1, -1);
        else
            return __builtin_shufflevector(f, f, 0, 1, 2, 3, 4, 5, -1, -1);
    }
    static __device__ acc mfma(frag a, frag b, acc c, int = 0) {
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(widen(a), widen(b), c, FMT, FMT, 0,
                                                                0x7F7F7F7F, 0, 0x7F7F7F7F);
    }
};
