// Chip-wide MX quantise sweep for the MI355X node agent (included from
// agent.hip; element encodings and packing are mx_formats.h's, stamp, placement
// and record are sweep_common.h's).
//
// The MX GEMM sweep feeds v_mfma_scale_f32_16x16x128_f8f6f4 with operands a
// fill kernel wrote with integer bit tricks and with scales of 1 or 2. In
// service those operands come out of a quantiser: bf16 activations in, the
// largest magnitude of every 32 elements, an E8M0 scale from it, the elements
// through the gfx950 scaled conversions v_cvt_scalef32_pk_fp8_bf16,
// v_cvt_scalef32_pk_fp4_bf16 and v_cvt_scalef32_pk32_fp6_bf16, packed elements
// and scale bytes out in the layout the GEMM reads. This is that kernel, on
// every SIMD of the chip, every output bit checked: a conversion unit that
// rounds or saturates wrongly, or a wrong shared exponent, shows here and
// nowhere else.
//
// The operation (normative -- tests/test_nodeagent_mxquantsweep.py carries an
// independent numpy copy). src is rows x K bf16, row-major, K a multiple of 32;
// everything is dense, so it is B = rows * K / 32 blocks in a row. For format
// f of MX_E4M3 (fp8), MX_E2M3 (fp6), MX_E2M1 (fp4), block x reads elements
// 32 x .. 32 x + 31, writes 4 * mx_bits(f) bytes at dst + 4 * mx_bits(f) * x,
// element i at bit mx_bits(f) * i of them (fp8 a byte per element; fp4 two per
// byte, the even one in the low nibble; fp6 across byte and word boundaries),
// and writes byte x of scales. With emax = 8 (E4M3) or 2 (E2M3, E2M1):
//
//   amax = max |x_i|; amax == 0: scale byte 0, every element its zero code
//   otherwise e = floor(log2 amax) - emax, scale byte 127 + e, and element i
//   is x_i * 2^-e rounded to nearest even in f and saturated to the largest
//   finite magnitude of f (448, 7.5, 6); an E4M3 NaN code is never produced;
//   the sign bit of a code is the sign bit of the input, for zero results too.
//
// Contract: finite inputs that are normal or zero, and amax >= 2^-100 for a
// block that is not all zero. Outside it the result is unspecified (the
// kernel and qs_reference_block agree there all the same: the scale byte is
// max(exponent field of amax - emax, 0) and a bf16 subnormal counts as zero).
//
// What the MI355X does (tests' exhaustive case: every bf16 pattern inside the
// contract at four distances below its block's amax, every output byte
// compared; and single conversions of chosen values):
//   - the third operand is taken as an f32 of which only the exponent field
//     counts (2.0 and 3.0 scale alike), and the source is DIVIDED by that
//     power of two; the kernel passes (scale byte << 23);
//   - rounding is to nearest even, into the subnormal codes too; a result
//     that rounds to zero keeps the sign of its input, as does a zero input:
//     the rule above holds as it stands, the reference does not deviate;
//   - overflow saturates to the largest finite magnitude in E2M3 (7.5) and
//     E2M1 (6), from just above it to 1e30. In E4M3 it does NOT: 464 / 1 (the
//     tie) still gives 448, but 480 and everything above give the NaN code
//     0x7F / 0xFF. That class, elements of the block's top binade above 1.75 x
//     2^E (E that of amax, so 448 after scaling), is handled in VALU ahead of
//     the instruction: the bit patterns are clamped to that of 1.75 x 2^E,
//     two to a register (v_pk_min_i16 for the positive, v_pk_min_u16 for the
//     negative ones), which is what saturation asks for since everything in
//     448 .. 512 saturates or rounds to 448. No other class is;
//   - a scale operand of all zero bits counts as 2^-127;
//   - pk_fp8 writes source element 0 into the low byte of the half-word that
//     op_sel picks, pk_fp4 element 0 into the low nibble of the byte it
//     picks, pk32_fp6 element i at bit 6 i of its six registers: the layouts
//     above with no shuffling.
//
// Work split. 256-thread workgroups; a tile is 256 consecutive blocks (16 KiB
// of source), one block per lane; tile T = x / 256 belongs to workgroup T mod W
// (W workgroups launched) and block x to wave (x % 256) / 64 of it. The sweep
// launches 4 x CUs workgroups with the device's whole per-workgroup LDS, so a
// workgroup has its CU, and each wave a SIMD, to itself. `passes` repeats the
// workgroup's whole list of tiles; every pass rewrites the output.
//
// How a tile moves. Source: thread t loads the tile's 16-byte vectors t, t +
// 256, t + 512, t + 768 (a wave's 64 lanes 1 KiB in a row per instruction),
// for the NEXT step, into 16 registers, ahead of the current tile's
// conversion, and writes them to the other of two 16 KiB LDS stages after it.
// A lane then needs the four vectors of its own block, which in plain order
// are 64 bytes apart: eight (or sixteen) lanes of a ds_read_b128 would share
// two (or four) of the LDS's 16-byte bank groups. So vector c of tile block b
// sits at slot 4 b + (c ^ s(b)), s(b) = ((b >> 1) ^ (b >> 2)) & 3: over any 8
// consecutive b the slots of a fixed c cover all residues mod 8, over any 16
// all residues mod 16, and the writers' 8 or 16 consecutive vectors (two or
// four whole blocks) stay a permutation of the slots they covered: both sides
// conflict-free whichever of the two widths the bank period is. The lane's
// four slot addresses are loop constants.
// Output: fp4 is 16 bytes per lane at 16-byte pitch, which is already one full
// vector per lane in a row across the wave: stored straight from registers.
// fp8 is two vectors per lane: lane b writes logical vectors 2 b and 2 b + 1 of
// an 8 KiB output stage at slot 2 b + (h ^ ((b >> 2) ^ (b >> 3)) & 1) (the
// same argument for pitch 2), and after the barrier thread t stores logical
// vectors t and t + 256. fp6 is 24 bytes per lane, a vector and a half: lane b
// writes three 8-byte words at byte 24 b (24 b is 8- but not 16-byte aligned;
// at a 6-dword pitch lanes 16 apart share banks of a 32-bank LDS, two-way,
// on three instructions a tile, left as it is), and thread t stores vector t
// and, for t < 128, vector 256 + t of the 384. Two output stages alternate so
// that one barrier per step is enough: 2 x 16 KiB + 2 x 8 KiB of LDS in use.
// Scale bytes: a quad of lanes exchanges its four bytes by DPP quad_perm and
// its first lane stores the dword.
// Tails: a tile's last blocks beyond B are loaded as zeros and convert like
// any block, and are left out of stores and checksum; an fp6 tile of an odd
// number of blocks ends in half a vector, stored as 8 bytes; the last quad of
// scales, when B is no multiple of 4, is stored byte by byte.
//
// Checksum (normative). Arithmetic mod 2^64 unless said, G = MS_G, mix64 =
// mt_mix64, base = seed * G. For block x with scale byte s and output words
// w_0 .. w_{n-1} (n = mx_bits(f) little-endian dwords):
//
//   h = s; for i in 0 .. n-1: h = 33 * h + w_i           (mod 2^32)
//   weight_x = mix64(base + x) | 1
//   record 4 * g + v (wave v of workgroup g) = passes * sum weight_x * h
//     over the blocks x with (x / 256) % W == g and (x % 256) / 64 == v
//
// The kernel adds weight_x * h once per pass. `wave` of the record is 4 g + v
// and its clocks are stamped around the whole pass loop.
//
// The sweep's source (normative), element i of block x = i / 32, of E = 32 B
// elements, h = mix64(base + i):
//
//   zero if x % 64 == 63 or h % 16 == 0, otherwise
//   sign (h >> 11) & 1, mantissa (h >> 4) & 127, and exponent field
//   127 + binade_x - (h >> 32) % 11, binade_x = (mix64(base + E + x) >> 40) % 41 - 20
//
// so scale bytes range over 41 values, a block's elements over eleven binades
// (the lower ones subnormal in the 6- and 4-bit formats), a sixteenth of the
// seven-bit mantissas is a tie in E4M3, and the top binade's upper mantissas
// saturate.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mx_formats.h"
#include "sweep_common.h"

#define QS_TILE MS_BLOCK                  // blocks of a tile: one per lane
#define QS_SRC_VECS 4                     // 16-byte vectors of a block's 32 bf16
#define QS_STAGE_VECS (QS_TILE * QS_SRC_VECS)
#define QS_OUT_STAGE_VECS (QS_TILE * 2)   // the widest output, fp8: 32 bytes per block
#define QS_LDS_BYTES ((2 * QS_STAGE_VECS + 2 * QS_OUT_STAGE_VECS) * 16)
static_assert(QS_LDS_BYTES <= MS_CU_LDS_BYTES / 2, "launched with the whole allocation anyway");
static_assert(NA_MXQUANT_MAX_BLOCKS <= (1 << 24), "byte offsets of a tile stay under 2^31");

typedef unsigned qs_vec __attribute__((ext_vector_type(4)));  // one 16-byte vector

__host__ __device__ constexpr bool qs_format_ok(int fmt) {
    return fmt == MX_E4M3 || fmt == MX_E2M3 || fmt == MX_E2M1;
}
// floor(log2) of the largest finite magnitude.
__host__ __device__ constexpr int qs_emax(int fmt) { return fmt == MX_E4M3 ? 8 : 2; }
// The code of the largest finite magnitude: 448, 7.5, 6.
__host__ __device__ constexpr unsigned qs_max_code(int fmt) {
    return fmt == MX_E4M3 ? 0x7Eu : fmt == MX_E2M3 ? 0x1Fu : 0x07u;
}

// The scale byte of a block whose largest bf16 magnitude has the bits `amax`.
__host__ __device__ inline unsigned qs_scale_byte(int fmt, unsigned amax) {
    const int s = (int)(amax >> 7) - qs_emax(fmt);
    return s < 0 ? 0u : (unsigned)s;
}

// The code of the bf16 `bits` in a block of scale byte `scale`: the rules at
// the top in integer arithmetic. 128 + mantissa is the significand, te the
// biased exponent of the result in the target format.
__host__ __device__ inline unsigned qs_encode(int fmt, unsigned bits, unsigned scale) {
    const int man = mx_man_bits(fmt);
    const unsigned sign = (bits >> 15 & 1) << (mx_bits(fmt) - 1);
    const int ex = (int)(bits >> 7 & 255);
    if (ex == 0) return sign;
    const unsigned m = 128u | (bits & 127u);
    const int te = ex - (int)scale + mx_bias(fmt);
    const int drop = 7 - man + (te >= 1 ? 0 : 1 - te);  // low bits that go
    if (drop > 8) return sign;                          // under half the smallest subnormal
    const unsigned rest = m & ((1u << drop) - 1), half = 1u << (drop - 1);
    unsigned r = m >> drop;
    if (rest > half || (rest == half && (r & 1))) r++;
    // a normal's r carries the implicit one, which counts the exponent up
    const unsigned code = (te >= 1 ? (unsigned)(te - 1) << man : 0u) + r;
    return sign | (code < qs_max_code(fmt) ? code : qs_max_code(fmt));
}

// One block by the rules at the top: 32 bf16 in, mx_bits(fmt) words and the
// scale byte out. The host's quantiser and the verify's engine.
__host__ __device__ inline unsigned qs_reference_block(int fmt, const uint16_t* src,
                                                       uint32_t* words) {
    unsigned amax = 0;
    for (int i = 0; i < 32; ++i) amax = (src[i] & 0x7FFFu) > amax ? (src[i] & 0x7FFFu) : amax;
    const unsigned scale = qs_scale_byte(fmt, amax);
    for (int i = 0; i < mx_bits(fmt); ++i) words[i] = 0;
    for (int i = 0; i < 32; ++i) mx_put(words, fmt, i, qs_encode(fmt, src[i], scale));
    return scale;
}

// h of the checksum: the scale byte, then the block's words.
__host__ __device__ inline uint32_t qs_fold(uint32_t h, uint32_t word) {
    return (h << 5) + h + word;
}
__host__ __device__ inline mt_u64 qs_weight(mt_u64 base, mt_u64 x) {
    return mt_mix64(base + x) | 1;
}

// The sweep's source: the binade of block x, and element i given its block's.
__host__ __device__ inline int qs_binade(mt_u64 base, mt_u64 elems, mt_u64 x) {
    return (int)((mt_mix64(base + elems + x) >> 40) % 41) - 20;
}
__host__ __device__ inline unsigned qs_element(mt_u64 base, mt_u64 i, int binade) {
    const mt_u64 h = mt_mix64(base + i);
    if (((i >> 5) & 63) == 63 || (h & 15) == 0) return 0;
    const unsigned ex = (unsigned)(127 + binade - (int)((h >> 32) % 11));
    return (unsigned)(h >> 11 & 1) << 15 | ex << 7 | (unsigned)(h >> 4 & 127);
}

// src: `vecs` 16-byte vectors, eight elements each, of elems = 8 * vecs. One
// thread per vector.
__global__ void __launch_bounds__(MS_BLOCK)
mxquant_fill_kernel(qs_vec* __restrict__ src, mt_u64 vecs, mt_u64 base) {
#if defined(__gfx950__)
    const mt_u64 v = (mt_u64)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= vecs) return;
    const int binade = qs_binade(base, vecs * 8, v >> 2);
    qs_vec out;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        out[i] = qs_element(base, v * 8 + 2 * i, binade) |
                 qs_element(base, v * 8 + 2 * i + 1, binade) << 16;
    src[v] = out;
#endif
}

#if defined(__gfx950__)

typedef unsigned short qs_u16x2 __attribute__((ext_vector_type(2)));
typedef short qs_s16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 qs_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 qs_bf16x32 __attribute__((ext_vector_type(32)));
typedef unsigned qs_u32x6 __attribute__((ext_vector_type(6)));
typedef unsigned qs_u32x16 __attribute__((ext_vector_type(16)));

// The value of `v` in lane k of the caller's quad of lanes.
template <int K>
__device__ __forceinline__ unsigned qs_quad(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, K * 0x55, 0xF, 0xF, true);
}

// A lane's block: the 16 registers of its 32 bf16 in, mx_bits(FMT) registers
// of packed elements out, the scale byte back. amax on the bit patterns, two
// to a register (v_and, v_pk_max_u16), the exponent by shifts, then sixteen pk
// conversions (fp8, fp4) or one pk32 (fp6).
template <int FMT>
__device__ __forceinline__ unsigned qs_convert(const unsigned (&p)[16], unsigned (&out)[8]) {
    qs_u16x2 top = {0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        top = __builtin_elementwise_max(top, __builtin_bit_cast(qs_u16x2, p[i] & 0x7FFF7FFFu));
    const unsigned amax = top[0] > top[1] ? top[0] : top[1];
    const unsigned scale = qs_scale_byte(FMT, amax);
    // the instructions divide by 2^(exponent field - 127) of this; a zero
    // block (scale byte 0) divides its zeros by 2^-126
    const float by = __builtin_bit_cast(float, (scale == 0 ? 1u : scale) << 23);
    if constexpr (FMT == MX_E4M3) {
        // The class the instruction gets wrong: what rounds past 448 comes out
        // as the NaN code. 448 * 2^e is the bf16 1.75 * 2^(amax's binade), and
        // whatever lies above it in the block must become it: the positive
        // patterns by a signed minimum, which the negative ones pass, then the
        // negative ones by an unsigned minimum, which the positive ones pass.
        const unsigned most = (amax & 0x7F80u) | 0x60u;
        const qs_s16x2 above = __builtin_bit_cast(qs_s16x2, most * 0x10001u);
        const qs_u16x2 below = __builtin_bit_cast(qs_u16x2, most * 0x10001u | 0x80008000u);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            qs_bf16x2 pair[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const qs_s16x2 capped = __builtin_elementwise_min(
                    __builtin_bit_cast(qs_s16x2, p[2 * i + j]), above);
                pair[j] = __builtin_bit_cast(
                    qs_bf16x2,
                    __builtin_elementwise_min(__builtin_bit_cast(qs_u16x2, capped), below));
            }
            qs_s16x2 w = {0, 0};
            w = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(w, pair[0], by, false);
            w = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(w, pair[1], by, true);
            out[i] = __builtin_bit_cast(unsigned, w);
        }
    } else if constexpr (FMT == MX_E2M1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned w = 0;
            w = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(
                w, __builtin_bit_cast(qs_bf16x2, p[4 * i]), by, 0);
            w = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(
                w, __builtin_bit_cast(qs_bf16x2, p[4 * i + 1]), by, 1);
            w = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(
                w, __builtin_bit_cast(qs_bf16x2, p[4 * i + 2]), by, 2);
            w = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(
                w, __builtin_bit_cast(qs_bf16x2, p[4 * i + 3]), by, 3);
            out[i] = w;
        }
    } else {
        qs_u32x16 all;
#pragma unroll
        for (int i = 0; i < 16; ++i) all[i] = p[i];
        const qs_u32x6 six =
            __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(qs_bf16x32, all), by);
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = six[i];
    }
    return scale;
}

#endif  // __gfx950__

// records: 4 * gridDim.x entries. src: 4 * blocks vectors; dst: 4 *
// mx_bits(FMT) * blocks bytes, 16-byte aligned; scales: blocks bytes, 4-byte
// aligned. Launch with any number of workgroups of MS_BLOCK threads and at
// least QS_LDS_BYTES of dynamic shared memory.
template <int FMT>
__global__ void __launch_bounds__(MS_BLOCK)
mxquant_sweep_kernel(na_mfma_record* __restrict__ records, const qs_vec* __restrict__ src,
                     unsigned char* __restrict__ dst, unsigned char* __restrict__ scales,
                     uint32_t blocks, uint32_t passes, mt_u64 base) {
    const uint32_t t = threadIdx.x;
    na_mfma_record* const mine = records + (size_t)blockIdx.x * MS_WAVES_PER_WG + (t >> 6);
#if defined(__gfx950__)
    constexpr int WORDS = mx_bits(FMT);  // a block's output dwords: 8, 6, 4
    extern __shared__ qs_vec qs_lds[];
    qs_vec* const out_lds = qs_lds + 2 * QS_STAGE_VECS;
    const ms_hw_where at = ms_where();

    // this workgroup's tiles: blockIdx.x, + gridDim.x, ...; `steps` of them in all
    const uint32_t tiles = (blocks + QS_TILE - 1) / QS_TILE;
    const uint32_t own = tiles > blockIdx.x ? (tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    const uint32_t steps = own * passes;

    // source slots (see "How a tile moves"): where this thread's four staged
    // vectors go, and where its own block's four are
    const uint32_t put = ((t >> 2) << 2) | ((t & 3) ^ (((t >> 3) ^ (t >> 4)) & 3));
    const uint32_t own_swizzle = ((t >> 1) ^ (t >> 2)) & 3;
    // fp8 output slots: this lane's two, and logical vector t's
    const uint32_t out_put = (t << 1) | (((t >> 2) ^ (t >> 3)) & 1);
    const uint32_t out_get = (t & ~1u) | ((t & 1) ^ (((t >> 3) ^ (t >> 4)) & 1));

    qs_vec staged[QS_SRC_VECS];
    auto load = [&](uint32_t tile) {  // zeros past the last block
        const uint32_t vecs = min(blocks - tile * QS_TILE, (uint32_t)QS_TILE) * QS_SRC_VECS;
        const qs_vec* const g = src + (size_t)tile * QS_STAGE_VECS;
#pragma unroll
        for (int j = 0; j < QS_SRC_VECS; ++j)
            staged[j] = t + j * QS_TILE < vecs ? g[t + j * QS_TILE] : qs_vec{0, 0, 0, 0};
    };
    auto stage = [&](uint32_t s) {
#pragma unroll
        for (int j = 0; j < QS_SRC_VECS; ++j)
            qs_lds[s * QS_STAGE_VECS + put + j * QS_TILE] = staged[j];
    };

    const ms_clock t0 = ms_stamp();

    mt_u64 sum = 0;
    uint32_t tile = blockIdx.x, s = 0;
    if (steps != 0) {
        load(tile);
        stage(0);
    }
    __syncthreads();
    for (uint32_t step = 0; step < steps; ++step, s ^= 1) {
        // the next step's tile on its way (after the last: the first again, in
        // bounds, into a stage nobody reads)
        const uint32_t next = tile + gridDim.x < tiles ? tile + gridDim.x : blockIdx.x;
        load(next);

        unsigned p[16], out[8];
#pragma unroll
        for (int c = 0; c < QS_SRC_VECS; ++c) {
            const qs_vec v = qs_lds[s * QS_STAGE_VECS + ((t << 2) | (c ^ own_swizzle))];
#pragma unroll
            for (int i = 0; i < 4; ++i) p[4 * c + i] = v[i];
        }
        const unsigned scale = qs_convert<FMT>(p, out);

        const uint32_t x = tile * QS_TILE + t;  // this lane's block
        const uint32_t here = min(blocks - tile * QS_TILE, (uint32_t)QS_TILE);  // blocks of the tile
        uint32_t h = scale;
#pragma unroll
        for (int i = 0; i < WORDS; ++i) h = qs_fold(h, out[i]);
        if (t < here) sum += qs_weight(base, x) * (mt_u64)h;

        // four scale bytes to a dword, in every lane of the quad
        const unsigned quad = qs_quad<0>(scale) | qs_quad<1>(scale) << 8 |
                              qs_quad<2>(scale) << 16 | qs_quad<3>(scale) << 24;
        if ((t & 3) == 0 && t < here) {
            if (t + 3 < here) {
                *reinterpret_cast<uint32_t*>(scales + x) = quad;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 3; ++i)
                    if (t + i < here) scales[x + i] = (unsigned char)(quad >> (8 * i));
            }
        }

        qs_vec* const o = out_lds + s * QS_OUT_STAGE_VECS;
        if constexpr (FMT == MX_E4M3) {
            o[out_put] = qs_vec{out[0], out[1], out[2], out[3]};
            o[out_put ^ 1] = qs_vec{out[4], out[5], out[6], out[7]};
        } else if constexpr (FMT == MX_E2M3) {
            uint2* const o8 = reinterpret_cast<uint2*>(o) + 3 * t;
            o8[0] = uint2{out[0], out[1]};
            o8[1] = uint2{out[2], out[3]};
            o8[2] = uint2{out[4], out[5]};
        } else {
            if (t < here)
                reinterpret_cast<qs_vec*>(dst)[x] = qs_vec{out[0], out[1], out[2], out[3]};
        }
        stage(s ^ 1);
        __syncthreads();

        if constexpr (FMT == MX_E4M3) {
            qs_vec* const g = reinterpret_cast<qs_vec*>(dst) + (size_t)tile * (2 * QS_TILE);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (t + j * QS_TILE < 2 * here) g[t + j * QS_TILE] = o[out_get + j * QS_TILE];
        } else if constexpr (FMT == MX_E2M3) {
            unsigned char* const g = dst + (size_t)tile * (24 * QS_TILE);
            const uint32_t bytes = 24 * here;  // a multiple of 8
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t v = t + j * QS_TILE;
                if (16 * v + 16 <= bytes)
                    reinterpret_cast<qs_vec*>(g)[v] = o[v];
                else if (16 * v < bytes)
                    reinterpret_cast<uint2*>(g)[2 * v] = reinterpret_cast<const uint2*>(o)[2 * v];
            }
        }
        tile = next;
    }

    const ms_clock t1 = ms_stamp();

    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((t & 63) == 0) {
        na_mfma_record rec;
        rec.checksum = sum;
        rec.wave = blockIdx.x * MS_WAVES_PER_WG + (t >> 6);
        ms_record_simd(rec, t0, t1, at);
        *mine = rec;
    }
#else
    // wrong arch: a checksum no reference produces, so verification fails
    if ((t & 63) == 0) {
        na_mfma_record rec = {};
        rec.checksum = ~0ULL;
        *mine = rec;
    }
#endif
}
