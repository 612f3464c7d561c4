// Chip-wide fused attention sweep for the MI355X node agent (included from
// agent.hip; the MFMA call and its fragment maps are mfma_frag.h's bf16
// 16x16x32 trait, stamp, placement and record are sweep_common.h's).
//
// The GEMM sweeps run one matrix product per launch. Attention is the other
// hot kernel of serving, and what sets it apart is tested nowhere else: two
// chained products whose first accumulators become the second's operand
// without leaving the wave, row maxima across lanes between them, v_exp_f32
// on the critical path, ds_read_b64_tr_b16 feeding an MFMA, and a running
// rescale of live accumulators. This kernel computes
//
//   O = softmax(scale * Q K^T [+ causal mask]) V
//
// flash-attention style (S and P never touch memory), as an operation on
// caller-owned tensors and, on hashed integer operands, as a sweep in which
// every intermediate is an exact f32, so that every wave's checksum is
// recomputed by the host bit for bit.
//
// Contract. Q is bf16[heads][n_q][128], K and V are bf16[kv_heads][n_k][128],
// row-major, V not transposed; o is null or float[heads][n_q][128]. n_q is a
// multiple of 128, n_k of 64, heads of kv_heads; query head h reads KV head
// h / (heads / kv_heads). With causal = 1, key j is visible to query i iff
// j <= i + n_k - n_q (bottom-right aligned), which needs n_k >= n_q, so key 0
// is visible to every row. Softmax is in base 2: p = exp2(c s - c m) with c =
// scale_log2 > 0 and m the running row maximum of s = q . k. `reps` walks the
// visible KV tiles that many times with one online-softmax state, so l and
// the unnormalised O are `reps` times those of one walk and O / l is the same.
//
// The sweep's operands (normative -- tests/test_nodeagent_attnsweep.py carries
// an independent numpy copy). Arithmetic mod 2^64, G = MS_G, mix64 = mt_mix64,
// base = seed * G, and with H = heads, HK = kv_heads the hashed sequence is
// laid out as qbase = base, ubase = qbase + H n_q 8, ebase = ubase + HK 128,
// vbase = ebase + HK n_k 4, wbase = vbase + HK n_k 128:
//
//   Q[h][i][c]  = +1 if bit 40 + c % 16 of mix64(qbase + (h n_q + i) 8 + c / 16)
//                 is set, else -1
//   u[hk][c]    = (mix64(ubase + hk 128 + c) >> 40) % 3 - 1
//   e[hk][j][t] = mix64(ebase + (hk n_k + j) 4 + t), t = 0..3: column
//                 32 t + ((e >> 40) & 31), value -1 if bit 48 is set, else +1
//   K[hk][j][c] = u[hk][c] + (the value of e[hk][j][c / 32] if c is its column)
//   V[hk][j][c] = (mix64(vbase + (hk n_k + j) 128 + c) >> 40) % 3 - 1
//   z_c = mix64(wbase + c) | 1 (c < 128), a = mix64(wbase + 128) | 1,
//   b = mix64(wbase + 129) | 1, w_(h,i) = mix64(wbase + 130 + h n_q + i) | 1
//
// Then s_ij = q_i . u + q_i . e_j: a dense common mode up to +-128 that is the
// same for every key of a row and cancels in s - m, so that a wrong product
// bit moves a logit by at least 1 and a p by a factor of at least 2; and a
// term in {-4, -2, 0, 2, 4}, so s - m >= -8 over a row. With c = 1, p =
// 2^(s - m) is a power of two, exact in bf16; relative to any running maximum
// l and O are integer multiples of 2^-8 bounded by reps * n_k, exact in f32
// while 256 * reps * n_k < 2^24 (NA_ATTN_EXACT), and the running rescale
// multiplies by exact powers of two and by the same bound drops no bit.
// THIS RESTS ON v_exp_f32 BEING EXACT AT THE INTEGERS 0 .. -8 (and at -inf);
// docs/DESIGN.md records what the MI355X does.
//
// Checksum (normative). The wave that owns rows R of head h leaves
//
//   sum_{i in R} w_(h,i) * ( sum_c z_c * int(256 O[i][c]) + a * int(256 l_i)
//                            + b * m_i )
//
// taken from its registers before normalisation in 64-bit integer VALU; O and
// l are the unnormalised ones relative to the final row maximum, m_i = max_j
// s_ij is an integer with its common mode. The host needs no O(n_q n_k d)
// work: Vz[j] = sum_c z_c V[j][c] once per KV head, q_i . u once per row, and
// four terms per pair (i, j).
//
// Work split. One workgroup of four waves per (head, block of 128 queries);
// wave w owns the 32 rows 128 qb + 32 w .. + 31 as two blocks of 16 and leaves
// record 4 * (h * n_q / 128 + qb) + w. The KV sequence is walked in tiles of 64
// keys.
//
// Block to item. Workgroups are dealt round-robin to the 8 XCDs, each with an
// L2 of its own, so block b = 8 i + x becomes the i-th of a contiguous range of
// positions owned by XCD x (as gemmsweep.h), and position p is KV head p /
// (nqb * group), query block (p / group) % nqb, head-in-group p % group (group
// = heads / kv_heads, nqb = n_q / 128): the workgroups an XCD runs at a time
// are the heads of one GQA group at the same query block, then its next query
// blocks, and read one K and V through that XCD's L2. The record index follows
// the item, not the block.
//
// First product, S^T = K Q^T on v_mfma_f32_16x16x32_bf16: A is 16 keys, B 16
// queries. Q's B fragments (query l & 15, head columns 32 s + 8 (l >> 4) ..
// + 7) are loaded once from global memory and stay in 32 registers. An
// accumulator register r of lane l is then key 16 kb + 4 (l >> 4) + r of query
// l & 15: four consecutive keys of ONE query per lane, so the row statistics
// are per lane, and the sixteen values of a lane (four key blocks kb) reduce
// in the lane before two cross-lane steps over the four lane groups (l ^ 16 by
// ds_swizzle, l ^ 32 by ds_bpermute; DPP does not cross a row of 16). The row
// SUM needs no cross-lane step per tile: every lane group rescales by the same
// factor, so each keeps a partial l that is summed once after the loop.
//
// Second product, computed as O^T = V^T P^T (a departure from "P as the A
// operand": with P as B the output column of a lane is again query l & 15, so
// the rescale factor and 1 / l are per lane, with no transpose of statistics).
// The operand maps of A and B are the same, so the packing is as designed: a
// lane's registers of key blocks 2 t and 2 t + 1, exp2'ed and packed to bf16,
// are the eight k of its fragment for k-step t. Element i of lane group g is
// therefore key 32 t + 16 (i >> 2) + 4 g + (i & 3): the permutation of keys
// inside a k-step, which V's fragments follow. Those are head columns 16 cb +
// (l & 15) at the same eight keys, read from the row-major tile by two
// ds_read_b64_tr_b16 (i < 4 and i >= 4): in each, lane group g reads the 4 x
// 16 block of rows 32 t + 16 (i >> 2) + 4 g .. + 3, lane 4 q + p of the group
// supplying the address of 8 bytes at column 4 p of row q and lane n receiving
// column n of the four rows (builtin and lane map as ldssweep.h's tr16 phase).
// O^T is 128 x 32 per wave: register r of accumulator (cb, query block) is
// head column 16 cb + 4 (l >> 4) + r, 64 registers, stored as float4.
//
// Data movement. A tile is 64 rows of 256 bytes of K and the same of V; LDS
// holds two stages of both, 64 KiB. Thread t loads vectors t, t + 256, ... of
// the NEXT tile (sixteen consecutive lanes read one row) -- K's ahead of the
// first product, written to the other stage after it, V's ahead of softmax
// and the second product, written after them -- so 16 registers stage both,
// and one __syncthreads per tile orders this stage's writes before the next
// step's reads and this step's reads before the writes of the step after.
// All four waves run the same trip count; the loads after the last step wrap
// to tile 0 (in bounds) and land in a stage nobody reads.
//
// Swizzles. K is gemmsweep.h's XOR chunk swizzle at 16 chunks a row: a
// fragment read is ds_read_b128 by lane l of row 16 kb + (l & 15), chunk 4 s +
// (l >> 4); rows are 256 bytes apart, exactly the span of the 64 banks, so
// unswizzled the 16 lanes of one chunk index share one 16-byte bank group.
// Row r stores chunk c at c ^ (r & 15): sixteen distinct groups, all 256
// bytes. V is derived for the transposed read: one instruction reads, per
// lane group, 32 contiguous bytes (chunks 2 cb and 2 cb + 1) of four rows, 16
// rows r & 15 = 0 .. 15 over the wave, 512 bytes; unswizzled all sixteen fall
// on the same 32 bytes of banks. Row r stores chunk c at c ^ 2 (r & 7), which
// keeps a 32-byte pair together and sends pair cb to cb ^ (r & 7): any eight
// consecutive rows (a half-wave: lane groups 0-1 or 2-3) cover the 256 bytes
// once, the whole read twice, which is the minimum for 512 bytes. (Derived,
// not measured: it assumes the LDS serves a b64 read a half-wave at a time.)
// The writers' sixteen consecutive lanes cover one whole row under either.
//
// Causal. A workgroup walks only tiles with a visible pair: (128 qb + n_k -
// n_q) / 64 + 2 of them. A wave skips both products of a tile that lies
// wholly above its 32 rows' diagonal (it still moves its share of the tile and
// meets the barrier), and masks, by -inf ahead of the maximum, only in tiles
// the diagonal crosses.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "memtest.h"
#include "mfma_frag.h"
#include "nodeagent.h"
#include "sweep_common.h"

#define AS_D 128          // head dimension
#define AS_QBLOCK 128     // queries per workgroup
#define AS_WAVE_ROWS (AS_QBLOCK / MS_WAVES_PER_WG)
#define AS_TILE 64        // keys per tile
#define AS_ROW_VECS (AS_D * 2 / 16)  // 16-byte vectors per row
#define AS_TILE_VECS (AS_TILE * AS_ROW_VECS)  // one operand's tile: 16 KiB
#define AS_LDS_BYTES (2 * 2 * AS_TILE_VECS * 16)
#define AS_LOADS (AS_TILE_VECS / MS_BLOCK)  // vectors a thread moves per tile and operand
#define AS_XCDS 8
#define AS_WEIGHTS 130    // z_0 .. z_127, a, b ahead of the row weights
static_assert(AS_D == NA_ATTN_HEAD_DIM && AS_QBLOCK == NA_ATTN_Q_BLOCK && AS_TILE == NA_ATTN_K_TILE,
              "nodeagent.h tells callers otherwise");
static_assert(AS_LDS_BYTES == 64 * 1024, "two stages of K and V");

// Where the parts of the hashed sequence start (see the top).
struct as_layout {
    mt_u64 q, u, e, v, w;
};
__device__ __host__ inline as_layout as_layout_of(mt_u64 base, mt_u64 heads, mt_u64 kv_heads,
                                                  mt_u64 n_q, mt_u64 n_k) {
    as_layout at;
    at.q = base;
    at.u = at.q + heads * n_q * (AS_D / 16);
    at.e = at.u + kv_heads * AS_D;
    at.v = at.e + kv_heads * n_k * 4;
    at.w = at.v + kv_heads * n_k * AS_D;
    return at;
}

// Sixteen elements of Q: bit c % 16 set is +1.
__device__ __host__ inline unsigned as_q_bits(mt_u64 at) { return (unsigned)(mt_mix64(at) >> 40) & 0xFFFFu; }
__device__ __host__ inline int as_ternary(mt_u64 at) {
    return (int)((unsigned)(mt_mix64(at) >> 40) % 3u) - 1;
}
// e of one key and quarter: its column within the quarter and its value.
__device__ __host__ inline void as_e(mt_u64 at, int* column, int* value) {
    const mt_u64 h = mt_mix64(at);
    *column = (int)(h >> 40 & 31);
    *value = (h >> 48 & 1) ? -1 : 1;
}
__device__ __host__ inline mt_u64 as_weight(mt_u64 at) { return mt_mix64(at) | 1; }

// The position block b takes in its XCD's contiguous range (see "Block to
// item"); a bijection of 0..items-1.
__device__ __host__ inline uint32_t as_position_of_block(uint32_t b, uint32_t items) {
    const uint32_t q = items / AS_XCDS, rem = items % AS_XCDS, x = b % AS_XCDS;
    return x * q + (x < rem ? x : rem) + b / AS_XCDS;
}

// Tiles of 64 keys a workgroup of query block qb walks once.
__device__ __host__ inline uint32_t as_tiles(uint32_t qb, uint32_t nqb, uint32_t nkt, uint32_t causal) {
    return causal ? (qb * AS_QBLOCK + nkt * AS_TILE - nqb * AS_QBLOCK) / AS_TILE + 2 : nkt;
}

// The two kernels below are compiled in a translation unit of their own,
// attnsweep.hip, which defines AS_KERNELS and these launchers (arguments as the
// kernels'; the caller checks hipGetLastError). agent.hip sees the
// specification above and the launchers only.
void as_launch_fill(unsigned grid, mt_vec* q, mt_vec* k, mt_vec* v, mt_u64 q_vecs, mt_u64 kv_vecs,
                    mt_u64 n_k, as_layout at);
void as_launch_sweep(na_mfma_record* records, const mt_vec* q, const mt_vec* k, const mt_vec* v,
                     float* o, uint32_t heads, uint32_t group, uint32_t nqb, uint32_t nkt,
                     uint32_t causal, float c, uint32_t reps, mt_u64 wbase);

#ifdef AS_KERNELS

// q, k, v: q_vecs, kv_vecs and kv_vecs 16-byte vectors of eight bf16, row by
// row, n_k rows to a KV head. One thread per vector of the three together.
__global__ void __launch_bounds__(MS_BLOCK)
attn_fill_kernel(mt_vec* __restrict__ q, mt_vec* __restrict__ k, mt_vec* __restrict__ v,
                 mt_u64 q_vecs, mt_u64 kv_vecs, mt_u64 n_k, as_layout at) {
#if defined(__gfx950__)
    const mt_u64 x = (mt_u64)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (x >= q_vecs + 2 * kv_vecs) return;
    bf16x8 f;
    mt_vec* dst;
    if (x < q_vecs) {
        // vector x is columns 8 (x % 16) .. + 7 of row x / 16
        const unsigned bits = as_q_bits(at.q + (x >> 1)) >> (8 * (x & 1));
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = (__bf16)((bits >> i & 1) ? 1.0f : -1.0f);
        dst = q + x;
    } else if (x < q_vecs + kv_vecs) {
        const mt_u64 y = x - q_vecs, row = y / AS_ROW_VECS;  // row = hk * n_k + j
        const int c0 = (int)(y % AS_ROW_VECS) * 8;
        int column, value;
        as_e(at.e + row * 4 + (mt_u64)(c0 >> 5), &column, &value);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            f[i] = (__bf16)(float)(as_ternary(at.u + row / n_k * AS_D + (mt_u64)(c0 + i)) +
                                   (((c0 + i) & 31) == column ? value : 0));
        dst = k + y;
    } else {
        const mt_u64 y = x - q_vecs - kv_vecs;
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = (__bf16)(float)as_ternary(at.v + y * 8 + (mt_u64)i);
        dst = v + y;
    }
    *dst = __builtin_bit_cast(mt_vec, f);
#endif
}

#if defined(__gfx950__)

typedef short as_s16x4 __attribute__((ext_vector_type(4)));
typedef short as_s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) as_s16x4 as_lds_s16x4;

// The value of lane l ^ 16 (ds_swizzle, bit mode: and 0x1F, or 0, xor 0x10)
// and of lane l ^ 32 (ds_bpermute).
__device__ __forceinline__ float as_xor16(float v) {
    return __builtin_bit_cast(float,
                              __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));
}
__device__ __forceinline__ float as_xor32(float v) { return __shfl_xor(v, 32); }

#endif  // __gfx950__

// records: 4 * heads * nqb entries. q: heads * nqb * 128 rows, k and v: (heads
// / group) * nkt * 64 rows, of AS_ROW_VECS vectors each. o: null, or heads *
// nqb * 128 x 128 floats. c = scale_log2 > 0. at.w (where the weights start)
// is all the kernel uses of the layout. Launch with heads * nqb workgroups of
// MS_BLOCK threads and AS_LDS_BYTES of dynamic shared memory.
// Budgeted for two waves per SIMD (under 256 registers, all of them VGPRs: left
// to itself the allocator takes 208 + 100 and shuttles the accumulators through
// AGPRs), so that two workgroups, 128 of the CU's 160 KiB of LDS, share a CU and
// one's softmax runs under the other's MFMAs.
__global__ void __launch_bounds__(MS_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))
attn_sweep_kernel(na_mfma_record* __restrict__ records, const mt_vec* __restrict__ q,
                  const mt_vec* __restrict__ k, const mt_vec* __restrict__ v,
                  float* __restrict__ o, uint32_t heads, uint32_t group, uint32_t nqb,
                  uint32_t nkt, uint32_t causal, float c, uint32_t reps, mt_u64 wbase) {
    const int wave = threadIdx.x >> 6;
    const uint32_t pos = as_position_of_block(blockIdx.x, heads * nqb);
    const uint32_t hk = pos / (nqb * group), qb = pos / group % nqb, h = hk * group + pos % group;
    const uint32_t rec_index = (h * nqb + qb) * MS_WAVES_PER_WG + wave;
    na_mfma_record* const mine = records + rec_index;
#if defined(__gfx950__)
    typedef mfma_bf16_16x16x32 T;
    extern __shared__ mt_vec as_lds[];
    const ms_hw_where at = ms_where();
    const int l = threadIdx.x & 63, g = l >> 4, x = l & 15;
    const uint32_t n_q = nqb * AS_QBLOCK, off = nkt * AS_TILE - n_q;  // causal: j <= i + off
    const uint32_t qw0 = qb * AS_QBLOCK + wave * AS_WAVE_ROWS;        // the wave's first row
    const uint32_t tiles = as_tiles(qb, nqb, nkt, causal);

    // Q's fragments: block b2 of 16 rows, k-step s
    bf16x8 qf[2][4];
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
        for (int s = 0; s < 4; ++s)
            qf[b2][s] = __builtin_bit_cast(
                bf16x8, q[((size_t)h * n_q + qw0 + 16 * b2 + x) * AS_ROW_VECS + 4 * s + g]);

    // global -> LDS: vector threadIdx.x + 256 j of a tile is chunk t & 15 of row
    // (t >> 4) + 16 j
    const mt_vec* const kg = k + (size_t)hk * nkt * AS_TILE_VECS + threadIdx.x;
    const mt_vec* const vg = v + (size_t)hk * nkt * AS_TILE_VECS + threadIdx.x;
    const int lrow = threadIdx.x >> 4, chunk = threadIdx.x & 15;
    const int put_k = lrow * AS_ROW_VECS + (chunk ^ lrow);                // 16 j keeps r & 15
    const int put_v = lrow * AS_ROW_VECS + (chunk ^ (2 * (lrow & 7)));    // and r & 7
    // LDS -> K fragment (kb, s): vector (get_k ^ 4 s) + 256 kb of the tile
    const int get_k = x * AS_ROW_VECS + (g ^ x);
    // LDS -> V fragment (t, cb), half i >> 2: byte (get_v ^ 32 cb) + 256 (32 t +
    // 16 (i >> 2)) of the tile; this lane addresses row 4 g + qq, 8 bytes at
    // column 4 p of the block's 16
    const int qq = (l >> 2) & 3, p = l & 3;
    const int get_v = (4 * g + qq) * 256 + ((4 * (g & 1) + qq) << 5) + ((p >> 1) << 4) + ((p & 1) << 3);

    mt_vec staged[AS_LOADS];
    auto load = [&](const mt_vec* from, uint32_t tile) {
#pragma unroll
        for (int j = 0; j < AS_LOADS; ++j) staged[j] = from[(size_t)tile * AS_TILE_VECS + j * MS_BLOCK];
    };
    auto store = [&](int stage, int operand, int put) {
        mt_vec* const s = as_lds + (stage * 2 + operand) * AS_TILE_VECS + put;
#pragma unroll
        for (int j = 0; j < AS_LOADS; ++j) s[j * 16 * AS_ROW_VECS] = staged[j];
    };

    f32x4 acc[2][8];  // O^T: [query block][block of 16 head columns]
    float m[2], lsum[2];
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2) {
        m[b2] = -__builtin_inff();
        lsum[b2] = 0.f;
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) acc[b2][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const ms_clock t0 = ms_stamp();

    load(kg, 0);
    store(0, 0, put_k);
    load(vg, 0);
    store(0, 1, put_v);
    __syncthreads();

    const uint32_t steps = reps * tiles;
    uint32_t kt = 0, stage = 0;
    for (uint32_t step = 0; step < steps; ++step) {
        const uint32_t next = kt + 1 == tiles ? 0 : kt + 1, k0 = kt * AS_TILE;
        const mt_vec* const sk = as_lds + stage * 2 * AS_TILE_VECS;
        const char* const sv = reinterpret_cast<const char*>(sk + AS_TILE_VECS);
        // wave-uniform: some pair of the tile is visible to this wave's rows;
        // the diagonal crosses the tile
        const bool live = !causal || k0 <= qw0 + AS_WAVE_ROWS - 1 + off;
        const bool diagonal = causal && k0 + AS_TILE - 1 > qw0 + off;

        load(kg, next);
        f32x4 st[4][2];  // S^T: [key block][query block]
        if (live) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                st[kb][0] = st[kb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bf16x8 kf = __builtin_bit_cast(
                        bf16x8, sk[(get_k ^ (4 * s)) + kb * 16 * AS_ROW_VECS]);
                    st[kb][0] = T::mfma(kf, qf[0][s], st[kb][0]);
                    st[kb][1] = T::mfma(kf, qf[1][s], st[kb][1]);
                }
            }
        }
        store(stage ^ 1, 0, put_k);
        load(vg, next);

        if (live) {
            bf16x8 pf[2][2];  // P^T: [query block][k-step of 32 keys]
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) {
                if (diagonal) {
                    const uint32_t last = qw0 + 16 * b2 + x + off;  // the last visible key
#pragma unroll
                    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (k0 + 16 * kb + 4 * g + r > last) st[kb][b2][r] = -__builtin_inff();
                }
                float top = st[0][b2][0];
#pragma unroll
                for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) top = __builtin_fmaxf(top, st[kb][b2][r]);
                top = __builtin_fmaxf(top, as_xor16(top));
                top = __builtin_fmaxf(top, as_xor32(top));
                const float m_new = __builtin_fmaxf(m[b2], top);
                // the running rescale, only when some row's maximum moved
                if (__builtin_amdgcn_ballot_w64(m_new != m[b2]) != 0) {
                    const float alpha = __builtin_amdgcn_exp2f(c * (m[b2] - m_new));
                    lsum[b2] *= alpha;
#pragma unroll
                    for (int cb = 0; cb < 8; ++cb) acc[b2][cb] *= alpha;
                    m[b2] = m_new;
                }
                const float cm = c * m_new;
#pragma unroll
                for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pr =
                            __builtin_amdgcn_exp2f(__builtin_fmaf(c, st[kb][b2][r], -cm));
                        lsum[b2] += pr;
                        pf[b2][kb >> 1][4 * (kb & 1) + r] = (__bf16)pr;
                    }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int cb = 0; cb < 8; ++cb) {
                    const char* const from = sv + (get_v ^ (32 * cb)) + 256 * 32 * t;
                    const as_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (as_lds_s16x4*)(from));
                    const as_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (as_lds_s16x4*)(from + 256 * 16));
                    const bf16x8 vf = __builtin_bit_cast(
                        bf16x8, (as_s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                    acc[0][cb] = T::mfma(vf, pf[0][t], acc[0][cb]);
                    acc[1][cb] = T::mfma(vf, pf[1][t], acc[1][cb]);
                }
        }
        store(stage ^ 1, 1, put_v);
        __syncthreads();  // uniform: the same trip for all four waves
        stage ^= 1;
        kt = next;
    }

    const ms_clock t1 = ms_stamp();

    // The lane groups' partial row sums, then checksum and output. This lane
    // holds head columns 16 cb + 4 g + r of rows qw0 + 16 b2 + x.
    mt_u64 inner[2] = {0, 0};
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2) {
        lsum[b2] += as_xor16(lsum[b2]);
        lsum[b2] += as_xor32(lsum[b2]);
    }
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const mt_u64 z = as_weight(wbase + (mt_u64)(16 * cb + 4 * g + r));
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2)
                inner[b2] += z * (mt_u64)(long long)(int)(256.f * acc[b2][cb][r]);
        }
    mt_u64 sum = 0;
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2) {
        const uint32_t row = qw0 + 16 * b2 + x;
        if (g == 0)
            inner[b2] += as_weight(wbase + AS_D) * (mt_u64)(long long)(int)(256.f * lsum[b2]) +
                         as_weight(wbase + AS_D + 1) * (mt_u64)(long long)(int)m[b2];
        sum += as_weight(wbase + AS_WEIGHTS + (mt_u64)h * n_q + row) * inner[b2];
        if (o != nullptr) {
            float* const out = o + ((size_t)h * n_q + row) * AS_D + 4 * g;
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
                float4 w;
                w.x = acc[b2][cb][0] / lsum[b2];
                w.y = acc[b2][cb][1] / lsum[b2];
                w.z = acc[b2][cb][2] / lsum[b2];
                w.w = acc[b2][cb][3] / lsum[b2];
                *reinterpret_cast<float4*>(out + 16 * cb) = w;
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if (l == 0) {
        na_mfma_record rec;
        rec.checksum = sum;
        rec.wave = rec_index;
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

#endif  // AS_KERNELS
