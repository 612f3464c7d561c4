// Chip-wide vector-unit sweep for the MI355X node agent (included from
// agent.hip): the vector register file and the VALU of every SIMD.
//
// na_fma_selftest is one short f32 chain on whichever SIMDs the dispatcher
// picks, summed into one counter. This kernel puts one wave on every SIMD of
// every CU (the matrix-core sweep's launch shape; compiled to 512 registers
// per lane, which alone allows one wave per SIMD), has each write a pattern
// to the register file and read it back at both polarities, run integer,
// f32, f64, packed, cross-lane and transcendental chains and a timed
// packed-f32 stream, and leaves one record per wave: a checksum per phase,
// the physical unit it ran on, an in-kernel diagnosis of the first wrong
// register, and two clock deltas. The host recomputes every exact checksum,
// so a bad SIMD is attributed to (XCC, SE, SH, CU, SIMD) and phase.
//
// Specification (normative — tests/test_nodeagent_valusweep.py carries an
// independent numpy copy). Arithmetic mod 2^64 unless said otherwise,
// G = 0x9E3779B97F4A7C15 and mix64 = mt_mix64 of memtest.h; w is the global
// wave (workgroup * 4 + wave of the workgroup), l the lane 0..63,
// gl = w*64 + l the global lane, p the phase index, and
//
//   h(p, i) = mix64(seed*G + (p << 32) + i)
//
// Except where said, a lane folds each value v it produces as c = c*G + v
// (signed integers sign-extended to 64 bits), starting from c = 0, and the
// phase checksum is the sum of c over the 64 lanes. Phases in order:
//
//   0 rf, 1 rf_inv   Register-file pattern, pol = 0 (rf) or 0xFFFFFFFF
//           (rf_inv). Slots s = 0..R-1 are the accumulator registers
//           a0..a255, then the architectural registers vF..v255,
//           F = VS_FIRST_VGPR = 32 and R = 512 - F = 480. v0..v(F-1) hold
//           the live state of the test itself and are NOT pattern-tested.
//           Per lane, mod 2^32: x_0 = (uint32)(h(p, gl) >> 32),
//           x_{s+1} = x_s * 1664525 + 1013904223, and slot s receives
//           x_{s+1} ^ pol. The LCG has full period, so no two slots of a
//           lane share a value and an aliased register reads back wrong.
//           All R slots are written; then all R are read back from the
//           registers, in slot order, and folded per lane in two halves
//           mod 2^32: lo = lo*0x9E3779B1 + v, hi = hi*0x85EBCA77 + v from
//           lo = hi = 0. The lane value is hi << 32 | lo and the checksum the
//           sum over lanes. Beside the read-back the chain is regenerated
//           and compared for the diagnosis fields of the record.
//   2 i32   State a, b, c, d (32 bits each): a | b << 32 = h(2, 2 gl),
//           c | d << 32 = h(2, 2 gl + 1). Step k = 0..63, mod 2^32 unless
//           64 bits are named:
//             t = a*b              u = (c * (d|1)) >> 32 (64-bit product)
//             m = a*c + (d << 32 | b)                    (64 bits)
//             e = t + u + lo32(m)  f = e ^ hi32(m) ^ k
//             g = lo32((f << 32 | e) >> (k & 31))        (funnel shift)
//             q = byte permute of g and t, below
//             fold q << 32 | g, then f << 32 | e
//             a = q + 0x9E3779B9, b = g | 1, c = f, d = e + k
//           q permutes bytes of g (high) and t (low): byte 0 of q is byte 0
//           of g, byte 1 is byte 3 of t, byte 2 is byte 2 of g, byte 3 is
//           byte 1 of t (v_perm_b32 with selector 0x01060304).
//   3 f32, 4 f64   Four chains j = 0..3 per lane, e = h(p, 4 gl + j):
//           x = (e & 0xFFF) - 2048, a = ((e >> 12) mod 7) - 3,
//           b = ((e >> 20) mod 15) - 7. Step k = 0..63, chains in order
//           within a step: r = fma(x, a, b) in the format of the phase,
//           converted to a 32-bit integer; fold r; x = (r & 0xFFF) - 2048
//           (r in two's complement), converted back. |r| <= 6151: every
//           value is an exact small integer in f32 and f64.
//   5 pk    Eight chains j = 0..7 per lane, e = h(5, 8 gl + j), a and b as
//           above. Chains 0..3 are the two halves of two v_pk_fma_f32
//           (chains 2i and 2i+1 share register pair i): x = (e & 0xFFF) -
//           2048, x = (r & 0xFFF) - 2048. Chains 4..7 are the halves of two
//           v_pk_fma_f16: x = (e & 0x3FF) - 512, x = (r & 0x3FF) - 512, so
//           |r| <= 1543 < 2048, exact in f16. 64 steps, chains in order
//           within a step, folded as f32 does.
//   6 xlane v = (uint32)(h(6, gl) >> 32). Moves n = 0..7 in order; move n
//           replaces v by v' and then, mod 2^32, v = v' * 0x9E3779B1 + l;
//           fold v (zero-extended) after each move. With v[i] the v of
//           lane i:
//             0  DPP quad_perm:[1,2,3,0]  v'[l] = v[(l & ~3) | ((l+1) & 3)]
//             1  DPP row_ror:3            v'[l] = v[(l & ~15) | ((l-3) & 15)]
//             2  DPP row_mirror           v'[l] = v[l ^ 15]
//             3  DPP row_half_mirror      v'[l] = v[l ^ 7]
//             4  ds_bpermute              v'[l] = v[(5 l + 3) & 63]
//             5  v_permlane16_swap on (A, B) = (v, v ^ 0xA5A5A5A5): rows of
//                16 lanes; odd rows of A are exchanged with the even rows
//                below them of B: A'[l] = l & 16 ? B[l - 16] : A[l],
//                B'[l] = l & 16 ? B[l] : A[l + 16].
//                v' = A' ^ rotl32(B', 7)
//             6  v_permlane32_swap on (A, B) = (v, v ^ 0x5A5A5A5A): lanes
//                32..63 of A are exchanged with lanes 0..31 of B:
//                A'[l] = l & 32 ? B[l - 32] : A[l],
//                B'[l] = l & 32 ? B[l] : A[l + 32]. v' as in move 5.
//             7  v_readlane broadcast     v'[l] = v[37]
//           These are the ISA's semantics, and what MI355X does: a probe in
//           which every lane supplied its own number returned exactly
//           these tables from one wave on each of the chip's 1024 SIMDs.
//   7 trans Consensus phase: no exact host reference exists for the
//           hardware's approximations, so the inputs depend on lane and
//           step only, NOT on the wave or the seed, every SIMD must produce
//           the same checksum, and the host flags the records that differ
//           from the strict majority. A fault common to the whole chip
//           passes this phase. Step k = 0..15: m = ((64 k + l) * 2654435761
//           mod 2^32) >> 9, t = the float with bits 0x3F800000 | m (in
//           [1, 2)); fold the bits (zero-extended) of v_exp_f32(t),
//           v_log_f32(t), v_rcp_f32(t), v_rsq_f32(t), v_sqrt_f32(t),
//           v_sin_f32(t - 1.5), v_cos_f32(t - 1.5), in this order.
//   8 stream  Timed. 32 chains j = 0..31 per lane, the halves of 16
//           v_pk_fma_f32 (chains 2i, 2i+1 in pair i), e = h(8, 32 gl + j):
//           x = (e & 0xFFF) - 2048, s = (e >> 12) & 1 ? -1 : 1,
//           b = ((e >> 13) mod 5) - 2. `iters` rounds of x = fma(x, s, b) on
//           every chain, exact while 2048 + 2 iters < 2^24
//           (iters <= VS_MAX_ITERS). Then fold the 32 final values as
//           integers, j in order. Closed form: s = 1 gives x + iters b;
//           s = -1 gives x for even iters and b - x for odd.
//           s_memtime / s_memrealtime are read before the first round and
//           after the last. FLOP per wave = iters * 16 * 64 * 2 * 2.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "memtest.h"
#include "nodeagent.h"
#include "sweep_common.h"

#define VS_BLOCK MS_BLOCK  // four waves: one per SIMD of the CU
#define VS_FIRST_VGPR 32
#define VS_SLOTS (512 - VS_FIRST_VGPR)
#define VS_STEPS 64
#define VS_TRANS_STEPS 16
#define VS_STREAM_PAIRS 16
#define VS_MAX_ITERS (((1 << 24) - 2048) / 2 - 1)
#define VS_FLOP_PER_ITER (VS_STREAM_PAIRS * 64 * 2 * 2)
#define VS_LCG_A 1664525u
#define VS_LCG_B 1013904223u
#define VS_FOLD_LO 0x9E3779B1u
#define VS_FOLD_HI 0x85EBCA77u
#define VS_XLANE_MUL 0x9E3779B1u
#define VS_XLANE_MOVES 8
#define VS_BCAST_LANE 37
#define VS_PERM_SEL 0x01060304u

enum { VS_RF, VS_RF_INV, VS_I32, VS_F32, VS_F64, VS_PK, VS_XLANE, VS_TRANS, VS_STREAM, VS_PHASES };

// The kernel leaves one na_valu_record (nodeagent.h) per wave.
static_assert(VS_PHASES == NA_VALU_PHASES && VS_MAX_ITERS == NA_VALU_MAX_ITERS,
              "nodeagent.h tells callers otherwise");

__device__ __host__ inline mt_u64 vs_h(mt_u64 base, int p, mt_u64 i) {
    return mt_mix64(base + ((mt_u64)p << 32) + i);
}

#if defined(__gfx950__)

typedef float vs_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 vs_h2 __attribute__((ext_vector_type(2)));

// Register numbers for the assembler's .irp, and the same registers as
// clobbers: a statement that names registers must list them (which also
// makes the kernel allocate all 512).
#define VS_TEN(p, t, s) \
    p t "0" s p t "1" s p t "2" s p t "3" s p t "4" s p t "5" s p t "6" s p t "7" s p t "8" s p t "9"
#define VS_SIX(p, t, s) p t "0" s p t "1" s p t "2" s p t "3" s p t "4" s p t "5"
#define VS_HUNDRED(p, h, s)                                                              \
    VS_TEN(p, h "0", s) s VS_TEN(p, h "1", s) s VS_TEN(p, h "2", s) s VS_TEN(p, h "3", s) \
    s VS_TEN(p, h "4", s) s VS_TEN(p, h "5", s) s VS_TEN(p, h "6", s) s VS_TEN(p, h "7", s) \
    s VS_TEN(p, h "8", s) s VS_TEN(p, h "9", s)
// 40..255 and 0..255 with prefix p and separator s
#define VS_40_255(p, s)                                                                  \
    VS_TEN(p, "4", s) s VS_TEN(p, "5", s) s VS_TEN(p, "6", s) s VS_TEN(p, "7", s)         \
    s VS_TEN(p, "8", s) s VS_TEN(p, "9", s) s VS_HUNDRED(p, "1", s) s VS_TEN(p, "20", s)  \
    s VS_TEN(p, "21", s) s VS_TEN(p, "22", s) s VS_TEN(p, "23", s) s VS_TEN(p, "24", s)   \
    s VS_SIX(p, "25", s)
#define VS_0_255(p, s) \
    VS_TEN(p, "", s) s VS_TEN(p, "1", s) s VS_TEN(p, "2", s) s VS_TEN(p, "3", s) s VS_40_255(p, s)
#define VS_32_255(p, s)                                                               \
    p "32" s p "33" s p "34" s p "35" s p "36" s p "37" s p "38" s p "39" s VS_40_255(p, s)
static_assert(VS_FIRST_VGPR == 32, "VS_32_255 spells the first pattern-tested VGPR");

// The same registers as a clobber list: separate literals, so macros of
// their own.
#define VS_CLOBBER_TEN(p, t) \
    p t "0", p t "1", p t "2", p t "3", p t "4", p t "5", p t "6", p t "7", p t "8", p t "9"
#define VS_CLOBBER_HUNDRED(p, h)                                                       \
    VS_CLOBBER_TEN(p, h "0"), VS_CLOBBER_TEN(p, h "1"), VS_CLOBBER_TEN(p, h "2"),       \
    VS_CLOBBER_TEN(p, h "3"), VS_CLOBBER_TEN(p, h "4"), VS_CLOBBER_TEN(p, h "5"),       \
    VS_CLOBBER_TEN(p, h "6"), VS_CLOBBER_TEN(p, h "7"), VS_CLOBBER_TEN(p, h "8"),       \
    VS_CLOBBER_TEN(p, h "9")
#define VS_CLOBBER_40_255(p)                                                            \
    VS_CLOBBER_TEN(p, "4"), VS_CLOBBER_TEN(p, "5"), VS_CLOBBER_TEN(p, "6"),              \
    VS_CLOBBER_TEN(p, "7"), VS_CLOBBER_TEN(p, "8"), VS_CLOBBER_TEN(p, "9"),              \
    VS_CLOBBER_HUNDRED(p, "1"), VS_CLOBBER_TEN(p, "20"), VS_CLOBBER_TEN(p, "21"),        \
    VS_CLOBBER_TEN(p, "22"), VS_CLOBBER_TEN(p, "23"), VS_CLOBBER_TEN(p, "24"),           \
    p "250", p "251", p "252", p "253", p "254", p "255"
#define VS_CLOBBERS                                                                       \
    VS_CLOBBER_TEN("a", ""), VS_CLOBBER_TEN("a", "1"), VS_CLOBBER_TEN("a", "2"),           \
    VS_CLOBBER_TEN("a", "3"), VS_CLOBBER_40_255("a"), "v32", "v33", "v34", "v35", "v36",   \
    "v37", "v38", "v39", VS_CLOBBER_40_255("v"), "vcc"

// The generator step and the per-slot work of the two passes. Operands:
// x the chain, t and d temporaries, cnt the slot counter; every dependence
// between these instructions is VALU -> VALU through a VGPR, an AGPR (one
// register file on gfx950, v_accvgpr_* are plain moves) or VCC into
// v_cndmask / v_addc, none of which needs a wait state.
#define VS_ASM_NEXT                            \
    "v_mul_lo_u32 %[x], %[x], %[la]\n\t"       \
    "v_add_u32 %[x], %[lb], %[x]\n\t"
// val: the register holding what the slot read back
#define VS_ASM_CHECK(val)                             \
    "v_mul_lo_u32 %[lo], %[lo], %[k1]\n\t"            \
    "v_mul_lo_u32 %[hi], %[hi], %[k2]\n\t"            \
    "v_add_u32 %[lo], %[lo], " val "\n\t"             \
    "v_add_u32 %[hi], %[hi], " val "\n\t"             \
    VS_ASM_NEXT                                       \
    "v_xor_b32 %[d], %[pol], %[x]\n\t"                \
    "v_xor_b32 %[d], %[d], " val "\n\t"               \
    "v_or_b32 %[xm], %[xm], %[d]\n\t"                 \
    "v_cmp_ne_u32 vcc, 0, %[d]\n\t"                   \
    "v_cndmask_b32 %[d], -1, %[cnt], vcc\n\t"         \
    "v_min_u32 %[first], %[first], %[d]\n\t"          \
    "v_addc_co_u32 %[bad], vcc, 0, %[bad], vcc\n\t"   \
    "v_add_u32 %[cnt], 1, %[cnt]\n\t"

struct vs_rf_out {
    uint32_t lo, hi, bad, first, xm;  // first: lowest wrong slot of the lane, ~0 = none
};

// One register-file phase of one lane: x0 seeds the chain, pol is 0 or ~0.
// The write pass and the read pass are one statement, so that nothing the
// compiler schedules can land in the named registers between them.
__device__ inline vs_rf_out vs_rf_pass(uint32_t x0, uint32_t pol) {
    vs_rf_out o;
    uint32_t x, t, d, cnt;
    asm volatile(
        // write pass
        "v_mov_b32 %[x], %[x0]\n\t"
        ".irp r," VS_0_255("", ",") "\n\t"
        VS_ASM_NEXT
        "v_xor_b32 %[t], %[pol], %[x]\n\t"
        "v_accvgpr_write_b32 a\\r, %[t]\n\t"
        ".endr\n\t"
        ".irp r," VS_32_255("", ",") "\n\t"
        VS_ASM_NEXT
        "v_xor_b32 v\\r, %[pol], %[x]\n\t"
        ".endr\n\t"
        // read pass
        "v_mov_b32 %[x], %[x0]\n\t"
        "v_mov_b32 %[lo], 0\n\t"
        "v_mov_b32 %[hi], 0\n\t"
        "v_mov_b32 %[bad], 0\n\t"
        "v_mov_b32 %[xm], 0\n\t"
        "v_mov_b32 %[cnt], 0\n\t"
        "v_mov_b32 %[first], -1\n\t"
        ".irp r," VS_0_255("", ",") "\n\t"
        "v_accvgpr_read_b32 %[t], a\\r\n\t"
        VS_ASM_CHECK("%[t]")
        ".endr\n\t"
        ".irp r," VS_32_255("", ",") "\n\t"
        VS_ASM_CHECK("v\\r")
        ".endr\n\t"
        : [lo] "=&v"(o.lo), [hi] "=&v"(o.hi), [bad] "=&v"(o.bad), [first] "=&v"(o.first),
          [xm] "=&v"(o.xm), [x] "=&v"(x), [t] "=&v"(t), [d] "=&v"(d), [cnt] "=&v"(cnt)
        : [x0] "v"(x0), [pol] "v"(pol), [la] "s"(VS_LCG_A), [lb] "s"(VS_LCG_B),
          [k1] "s"(VS_FOLD_LO), [k2] "s"(VS_FOLD_HI)
        : VS_CLOBBERS);
    return o;
}

__device__ inline mt_u64 vs_fold(mt_u64 c, mt_u64 v) { return c * MS_G + v; }
__device__ inline mt_u64 vs_fold_int(mt_u64 c, int v) { return c * MS_G + (mt_u64)(long long)v; }

__device__ inline mt_u64 vs_i32_phase(mt_u64 base, mt_u64 gl) {
    const mt_u64 h0 = vs_h(base, VS_I32, 2 * gl), h1 = vs_h(base, VS_I32, 2 * gl + 1);
    uint32_t a = (uint32_t)h0, b = (uint32_t)(h0 >> 32), c = (uint32_t)h1, d = (uint32_t)(h1 >> 32);
    mt_u64 sum = 0;
    for (uint32_t k = 0; k < VS_STEPS; ++k) {
        const uint32_t t = a * b;
        const uint32_t u = __umulhi(c, d | 1u);
        const mt_u64 m = (mt_u64)a * c + (((mt_u64)d << 32) | b);
        const uint32_t e = t + u + (uint32_t)m;
        const uint32_t f = e ^ (uint32_t)(m >> 32) ^ k;
        const uint32_t g = __builtin_amdgcn_alignbit(f, e, k & 31);
        const uint32_t q = __builtin_amdgcn_perm(g, t, VS_PERM_SEL);
        sum = vs_fold(sum, ((mt_u64)q << 32) | g);
        sum = vs_fold(sum, ((mt_u64)f << 32) | e);
        a = q + 0x9E3779B9u, b = g | 1u, c = f, d = e + k;
    }
    return sum;
}

__device__ inline float vs_fma(float x, float a, float b) { return __builtin_fmaf(x, a, b); }
__device__ inline double vs_fma(double x, double a, double b) { return __builtin_fma(x, a, b); }

// f32 and f64: FP is float or double
template <typename FP>
__device__ inline mt_u64 vs_fma_phase(mt_u64 base, int p, mt_u64 gl) {
    FP x[4], a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const mt_u64 e = vs_h(base, p, 4 * gl + j);
        x[j] = (FP)((int)(e & 0xFFF) - 2048);
        a[j] = (FP)((int)((e >> 12) % 7) - 3);
        b[j] = (FP)((int)((e >> 20) % 15) - 7);
    }
    mt_u64 sum = 0;
    for (int k = 0; k < VS_STEPS; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = (int)vs_fma(x[j], a[j], b[j]);
            sum = vs_fold_int(sum, r);
            x[j] = (FP)((r & 0xFFF) - 2048);
        }
    }
    return sum;
}

__device__ inline mt_u64 vs_pk_phase(mt_u64 base, mt_u64 gl) {
    vs_f2 x[2], a[2], b[2];
    vs_h2 xh[2], ah[2], bh[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const mt_u64 e = vs_h(base, VS_PK, 8 * gl + j), eh = vs_h(base, VS_PK, 8 * gl + 4 + j);
        x[j >> 1][j & 1] = (float)((int)(e & 0xFFF) - 2048);
        a[j >> 1][j & 1] = (float)((int)((e >> 12) % 7) - 3);
        b[j >> 1][j & 1] = (float)((int)((e >> 20) % 15) - 7);
        xh[j >> 1][j & 1] = (_Float16)((int)(eh & 0x3FF) - 512);
        ah[j >> 1][j & 1] = (_Float16)((int)((eh >> 12) % 7) - 3);
        bh[j >> 1][j & 1] = (_Float16)((int)((eh >> 20) % 15) - 7);
    }
    mt_u64 sum = 0;
    for (int k = 0; k < VS_STEPS; ++k) {
        vs_f2 r[2];
        vs_h2 rh[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            r[i] = __builtin_elementwise_fma(x[i], a[i], b[i]);
            rh[i] = __builtin_elementwise_fma(xh[i], ah[i], bh[i]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = (int)r[j >> 1][j & 1];
            sum = vs_fold_int(sum, v);
            x[j >> 1][j & 1] = (float)((v & 0xFFF) - 2048);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = (int)rh[j >> 1][j & 1];
            sum = vs_fold_int(sum, v);
            xh[j >> 1][j & 1] = (_Float16)((v & 0x3FF) - 512);
        }
    }
    return sum;
}

__device__ inline uint32_t vs_rotl7(uint32_t v) { return (v << 7) | (v >> 25); }

// DPP controls: quad_perm is the four 2-bit selectors, row_ror:n 0x120 + n,
// row_mirror 0x140, row_half_mirror 0x141. Every lane is active and the row
// and bank masks are 0xF, so no lane reads an invalid source.
template <int CTRL>
__device__ inline uint32_t vs_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

__device__ inline mt_u64 vs_xlane_phase(mt_u64 base, mt_u64 gl, uint32_t l) {
    uint32_t v = (uint32_t)(vs_h(base, VS_XLANE, gl) >> 32);
    mt_u64 sum = 0;
#define VS_MOVED(expr)                    \
    do {                                  \
        v = (expr)*VS_XLANE_MUL + l;      \
        sum = vs_fold(sum, v);            \
    } while (0)
    VS_MOVED(vs_dpp<1 | (2 << 2) | (3 << 4) | (0 << 6)>(v));
    VS_MOVED(vs_dpp<0x123>(v));
    VS_MOVED(vs_dpp<0x140>(v));
    VS_MOVED(vs_dpp<0x141>(v));
    VS_MOVED((uint32_t)__builtin_amdgcn_ds_bpermute((int)(((5 * l + 3) & 63) * 4), (int)v));
    {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v ^ 0xA5A5A5A5u, false, false);
        VS_MOVED(r[0] ^ vs_rotl7(r[1]));
    }
    {
        const auto r = __builtin_amdgcn_permlane32_swap(v, v ^ 0x5A5A5A5Au, false, false);
        VS_MOVED(r[0] ^ vs_rotl7(r[1]));
    }
    VS_MOVED((uint32_t)__builtin_amdgcn_readlane((int)v, VS_BCAST_LANE));
#undef VS_MOVED
    return sum;
}

__device__ inline mt_u64 vs_trans_phase(uint32_t l) {
    mt_u64 sum = 0;
    for (uint32_t k = 0; k < VS_TRANS_STEPS; ++k) {
        const uint32_t m = ((64 * k + l) * 2654435761u) >> 9;
        const float t = __uint_as_float(0x3F800000u | m);
        sum = vs_fold(sum, __float_as_uint(__builtin_amdgcn_exp2f(t)));
        sum = vs_fold(sum, __float_as_uint(__builtin_amdgcn_logf(t)));
        sum = vs_fold(sum, __float_as_uint(__builtin_amdgcn_rcpf(t)));
        sum = vs_fold(sum, __float_as_uint(__builtin_amdgcn_rsqf(t)));
        sum = vs_fold(sum, __float_as_uint(__builtin_amdgcn_sqrtf(t)));
        sum = vs_fold(sum, __float_as_uint(__builtin_amdgcn_sinf(t - 1.5f)));
        sum = vs_fold(sum, __float_as_uint(__builtin_amdgcn_cosf(t - 1.5f)));
    }
    return sum;
}

#endif  // __gfx950__

// records: 4 * gridDim.x entries. base = seed * G (hoisted to the host);
// 1 <= iters <= VS_MAX_ITERS. Launch with VS_BLOCK threads and more than half
// of the CU's LDS as dynamic shared memory (never touched: placement only,
// as in mfma_sweep_kernel).
__global__ void __launch_bounds__(VS_BLOCK)
valu_sweep_kernel(na_valu_record* __restrict__ records, mt_u64 base, int iters) {
#if defined(__gfx950__)
    const ms_hw_where at = ms_where();
    const uint32_t l = threadIdx.x & 63;
    const mt_u64 w = (mt_u64)blockIdx.x * MS_WAVES_PER_WG + (threadIdx.x >> 6);
    const mt_u64 gl = w * 64 + l;
    mt_u64 c[VS_PHASES];

    // rf, rf_inv: one copy of the statement, run at both polarities
    uint32_t rf_bad = 0, rf_key = ~0u, rf_xor = 0;  // key = (512 p + slot) << 6 | lane
    mt_u64 rf[2];
#pragma unroll 1
    for (uint32_t p = 0; p < 2; ++p) {
        const vs_rf_out o = vs_rf_pass((uint32_t)(vs_h(base, (int)p, gl) >> 32), p ? ~0u : 0u);
        rf[p] = ((mt_u64)o.hi << 32) | o.lo;
        rf_bad += o.bad;
        rf_xor |= o.xm;
        if (o.first != ~0u) {
            const uint32_t key = ((512 * p + o.first) << 6) | l;
            if (key < rf_key) rf_key = key;
        }
    }
    c[VS_RF] = rf[0];
    c[VS_RF_INV] = rf[1];

    c[VS_I32] = vs_i32_phase(base, gl);
    c[VS_F32] = vs_fma_phase<float>(base, VS_F32, gl);
    c[VS_F64] = vs_fma_phase<double>(base, VS_F64, gl);
    c[VS_PK] = vs_pk_phase(base, gl);
    c[VS_XLANE] = vs_xlane_phase(base, gl, l);
    c[VS_TRANS] = vs_trans_phase(l);

    // stream
    vs_f2 x[VS_STREAM_PAIRS], s[VS_STREAM_PAIRS], b[VS_STREAM_PAIRS];
#pragma unroll
    for (int j = 0; j < 2 * VS_STREAM_PAIRS; ++j) {
        const mt_u64 e = vs_h(base, VS_STREAM, 2 * VS_STREAM_PAIRS * gl + j);
        x[j >> 1][j & 1] = (float)((int)(e & 0xFFF) - 2048);
        s[j >> 1][j & 1] = (e >> 12) & 1 ? -1.0f : 1.0f;
        b[j >> 1][j & 1] = (float)((int)((e >> 13) % 5) - 2);
    }
    // The stamps bracket the whole loop, go only into the record, and no
    // output is computed from them.
    const ms_clock t0 = ms_stamp();
    // Four rounds per trip, then the remainder: the loop's scalar
    // instructions take issue slots of the one wave a SIMD has. The empty asm
    // keeps the rounds from being folded (see ms_fold).
#define VS_ROUND                                                      \
    _Pragma("unroll") for (int i = 0; i < VS_STREAM_PAIRS; ++i) {     \
        asm volatile("" : "+v"(x[i]));                                \
        x[i] = __builtin_elementwise_fma(x[i], s[i], b[i]);           \
    }
    int it = 0;
    for (; it + 4 <= iters; it += 4) {
        VS_ROUND VS_ROUND VS_ROUND VS_ROUND
    }
    for (; it < iters; ++it) {
        VS_ROUND
    }
#undef VS_ROUND
    const ms_clock t1 = ms_stamp();
    {
        mt_u64 sum = 0;
#pragma unroll
        for (int j = 0; j < 2 * VS_STREAM_PAIRS; ++j) sum = vs_fold_int(sum, (int)x[j >> 1][j & 1]);
        c[VS_STREAM] = sum;
    }

    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int p = 0; p < VS_PHASES; ++p) c[p] += __shfl_xor(c[p], o);
        rf_bad += __shfl_xor(rf_bad, o);
        const uint32_t key = __shfl_xor(rf_key, o);
        if (key < rf_key) rf_key = key;
        rf_xor |= __shfl_xor(rf_xor, o);
    }
    if (l == 0) {
        na_valu_record rec;
        for (int p = 0; p < VS_PHASES; ++p) rec.checksum[p] = c[p];
        rec.wave = (uint32_t)w;
        ms_record_simd(rec, t0, t1, at);
        rec.rf_bad = rf_bad;
        rec.rf_first_slot = rf_bad ? rf_key >> 6 : ~0u;
        rec.rf_first_lane = rf_bad ? rf_key & 63 : ~0u;
        rec.rf_xor = rf_xor;
        records[w] = rec;
    }
#else
    // wrong arch: checksums no reference produces, so verification fails
    if ((threadIdx.x & 63) == 0) {
        na_valu_record rec = {};
        for (int p = 0; p < VS_PHASES; ++p) rec.checksum[p] = ~0ULL;
        records[(size_t)blockIdx.x * MS_WAVES_PER_WG + (threadIdx.x >> 6)] = rec;
    }
#endif
}
