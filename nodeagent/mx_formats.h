// OCP MX element formats for the MI355X node agent: the operand encodings of
// v_mfma_scale_f32_{16x16x128,32x32x64}_f8f6f4, their decoders, and the
// packing of a lane's 32 elements into its fragment registers. Everything
// here is __host__ __device__, so the kernels and the host references share
// one definition.
//
// Format codes are the instruction's cbsz (A) / blgp (B) values.
//
//   code  format  bits  layout     bias  specials
//   0     E4M3    8     s eeee mmm   7   S.1111.111 = NaN, no inf (OCP e4m3fn)
//   1     E5M2    8     s eeeee mm  15   IEEE-like: e = 31 is inf (m = 0) / NaN
//   2     E2M3    6     s ee mmm     1   none
//   3     E3M2    6     s eee mm     3   none
//   4     E2M1    4     s ee m       1   none
//
// All five have subnormals (e = 0: m * 2^(1 - bias - mantissa bits)).
//
// Packing: element i of a lane sits at bit i * width of the lane's fragment,
// little-endian across consecutive 32-bit registers: 8, 6 or 4 registers per
// lane for 8-, 6- and 4-bit elements, two E2M1 per byte with the even element
// in the low nibble, and an E2M3/E3M2 element may straddle two registers
// (elements 5, 10, 15, ... do). The builtin takes <8 x i32> for every format
// and reads the first 8, 6 or 4 registers of it.
//
// Scales: a lane's scale register holds four E8M0 bytes (value 2^(byte-127));
// the instruction's opsel (0..3) picks the byte, and the lanes of lane group
// g supply the scale of K block g of their row or column.
//
// What the MI355X said (single-wave MX checks, every word of D exact, with
// operands that vary in k, per-lane scales, and decoy exponents in the three
// bytes opsel does not select):
//   - the bit order above is the hardware's for E2M1, E2M3 and E3M2, on both
//     shapes, the 6-bit elements that straddle two registers included, and
//     every code of the three formats decodes as mx_decode says;
//   - opsel n selects byte n of the scale register, for n = 0..3 on A and on
//     B alike;
//   - 8-bit operands are NOT 32 consecutive k per lane: see the k maps at
//     mx_frag in mfma_frag.h. E4M3 and E5M2 bytes themselves sit at byte i.

#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

enum { MX_E4M3 = 0, MX_E5M2, MX_E2M3, MX_E3M2, MX_E2M1, MX_FORMATS };

__host__ __device__ constexpr int mx_bits(int fmt) {
    return fmt <= MX_E5M2 ? 8 : fmt == MX_E2M1 ? 4 : 6;
}
__host__ __device__ constexpr int mx_man_bits(int fmt) {
    return fmt == MX_E4M3 || fmt == MX_E2M3 ? 3 : fmt == MX_E2M1 ? 1 : 2;
}
__host__ __device__ constexpr int mx_bias(int fmt) {
    return fmt == MX_E4M3 ? 7 : fmt == MX_E5M2 ? 15 : fmt == MX_E3M2 ? 3 : 1;
}

// Value of `code` (0 <= code < 2^mx_bits(fmt)).
__host__ __device__ inline float mx_decode(int fmt, unsigned code) {
    const int man = mx_man_bits(fmt), exp_bits = mx_bits(fmt) - 1 - man;
    const unsigned m = code & ((1u << man) - 1), e = (code >> man) & ((1u << exp_bits) - 1);
    const float sign = (code >> (mx_bits(fmt) - 1)) & 1 ? -1.f : 1.f;
    if (fmt == MX_E4M3 && e == 15 && m == 7) return __builtin_nanf("");
    if (fmt == MX_E5M2 && e == 31) return m ? __builtin_nanf("") : sign * __builtin_inff();
    const int bias = mx_bias(fmt);
    return sign * (e == 0 ? ldexpf((float)m, 1 - bias - man)
                          : ldexpf((float)((1u << man) + m), (int)e - bias - man));
}

// Code of the integer v in -3..3, which every format represents exactly.
// The codes of 0, 1, 2, 3 sit in the four bytes of one constant per format,
// so with fmt known at compile time this is a shift and a select.
__host__ __device__ inline unsigned mx_encode_int(int fmt, int v) {
    const unsigned mags = fmt == MX_E4M3   ? 0x44403800u
                          : fmt == MX_E5M2 ? 0x42403C00u
                          : fmt == MX_E2M3 ? 0x14100800u
                          : fmt == MX_E3M2 ? 0x12100C00u
                                           : 0x05040200u;
    const unsigned mag = (mags >> (8 * (v < 0 ? -v : v))) & 0xFF;
    return mag | (v < 0 ? 1u << (mx_bits(fmt) - 1) : 0u);
}

// ORs element i into fragment f (zeroed beforehand): f is anything indexable
// by register, a <N x i32> vector in a kernel or a uint32_t* on the host.
// With i known at compile time the straddle test folds away.
template <typename F>
__host__ __device__ inline void mx_put(F& f, int fmt, int i, unsigned code) {
    const int width = mx_bits(fmt), bit = i * width, lo = bit & 31;
    f[bit >> 5] |= (int)(code << lo);
    if (lo + width > 32) f[(bit >> 5) + 1] |= (int)(code >> (32 - lo));
}

// A lane's scale register: E8M0 byte `e8m0` at byte `opsel`, and a decoy
// exponent 7 higher in the other three, so a wrong byte select gives a wrong
// finite result (e8m0 <= 247).
__host__ __device__ constexpr int mx_scale_word(int opsel, int e8m0) {
    return (int)((((unsigned)(e8m0 + 7) * 0x01010101u) & ~(0xFFu << (8 * opsel))) |
                 ((unsigned)e8m0 << (8 * opsel)));
}
