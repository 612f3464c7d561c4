// Chip-wide MoE routing sweep for the MI355X node agent, and the three
// operations it runs on caller-owned tensors: the router (softmax weights and
// top-k), the stable sort of (token, choice) pairs into expert-major slots, and
// the weighted combine of the expert GEMM's rows back into token order
// (included from agent.hip for the host side and from attnsweep.hip, under
// AS_KERNELS, for the kernels: the translation unit without packed-f32 VALU
// forms; mix64, G and the workgroup scan are the other sweeps').
//
// moegemmsweep.h reads row_ids[slots] and offsets[experts + 1] from device
// memory. These kernels produce them there, and take the GEMM's C back to
// token order, so a whole MoE layer runs from router logits to output with no
// host step: route -> sort -> na_moe_gemm_run -> combine. The failure classes
// are their own: a cross-lane arg-max with a tie rule, LDS atomics whose result
// must not depend on order, a prefix sum over counts that exist only on the
// device, data-dependent scatter addresses, a gather-reduce bound by HBM.
//
// The problem (normative; tests/test_nodeagent_moeroutesweep.py carries an
// independent numpy copy). logits bf16[tokens][experts], 1 <= top_k <= 8 =
// NA_MOE_MAX_TOPK, top_k <= experts <= NA_MOE_MAX_EXPERTS, slots = tokens *
// top_k <= NA_MOE_MAX_ROWS.
//
// Route. Selection works on the bf16 values, never on the exponentials. Bits b
// map to the order-preserving key  b & 0x8000 ? ~b & 0xFFFF : b | 0x8000, a
// NaN of either sign to key 0, below -inf's 0x007F. A token's choices are the
// top_k largest keys, larger first, ties to the lower expert index: with
// packed = key << 8 | (255 - e) a plain maximum carries both rules. Entries
// past `experts` and entries already chosen are -1 in a signed word, under
// every real entry (whose packed value is >= 0), so whatever the logits hold
// the ids are distinct and in [0, experts). With m the largest non-NaN logit
// (0 if there is none), p_e = exp2(scale_log2 * (logit_e - m)): an f32
// subtraction, an f32 product, v_exp_f32 (__builtin_amdgcn_exp2f, as in
// attnsweep.h); a NaN logit has p = 0. denom_t is the sum of p over all experts
// (renorm = 0; lane-major, then across lanes) or over the chosen ones in the
// order chosen (renorm = 1). A row whose largest logit is +-inf gets NaN
// weights, as a softmax gives it. Outputs: topk_ids int32[tokens][top_k],
// topk_p float[tokens][top_k] unnormalised, denom float[tokens]; a routing
// weight is p / denom, and the division waits for the combine, once per token,
// as the attention sweep defers 1/l.
//
// Sort. offsets int32[experts + 1]: the exclusive prefix sums of the counts per
// expert, offsets[experts] their total; row_ids int32[slots]: expert e's slots
// hold the tokens that chose e in ascending token order (stable, hence unique:
// the host recomputes it); slot_of int32[tokens][top_k], the inverse.
//
// Combine. Y float[slots][N] (the expert GEMM's C), N a multiple of 4:
//   out[t][:] = (sum_j p[t][j] * Y[slot_of[t][j]][:]) * (1 / denom_t),
// the sum an FMA chain in the order j = 0 .. top_k-1 from 0, out float[tokens][N].
//
// Hashed operands. Arithmetic mod 2^64, base = seed * G, front(i) = mix64(base
// + i), back(i) = mix64(base - 1 - i); S = slots, T = tokens:
//   logit[t][e] = ((front(t) >> 40) % 7 - 3) - (front(T + t*experts + e) >> 40) % 9
//   weights (| 1): route id back(s), route p back(S + s), route denom back(2S + t),
//     scatter back(2S + T + s), combine token back(3S + T + t), combine row
//     back(3S + 2T + s), column back(4S + 2T + S + n)           (s = t*top_k + j)
//   Y[s][n] = a_s g_n + b_s h_n,  a = (x >> 40) % 3 - 1, b = (x >> 20) % 3 - 1
//     of x = back(4S + 2T + s); g, h the same of x = back(5S + 2T + N + n).
// With scale_log2 = 1 every p is a power of two in 2^0 .. 2^-8 (v_exp_f32 is
// exact at integer arguments: attnsweep.h), denom <= 256 a multiple of 2^-8,
// every token has ties (nine values of h over the experts), and 256 * the
// combine's sum is an integer below 2^13. The host needs O(tokens * experts +
// slots + N): 256 * sum_t[n] = A_t g_n + B_t h_n with A_t = sum_j 256 p_tj
// a_slot, so a wave's checksum is (sum_n q_n g_n) * sum_t w_t A_t + (sum_n q_n
// h_n) * sum_t w_t B_t + the row term. This is what U/V is to the GEMM sweeps.
//
// Records (na_mfma_record, indices in nodeagent.h), checksums from registers:
//   route,   wave w of block b (tokens 256 b + 64 w ..): sum over its tokens of
//            w_id * id + w_p * (int)(256 p) per choice + w_d * (int)(256 denom)
//   scatter, the same tokens: sum of w_s * (slot + 1) per choice
//   combine, wave w (tokens 8 w ..): sum_t w_t * sum_n q_n * (int)(256 sum_t[n])
//            + sum_(t,j) w_row * (row_ids[slot_of[t][j]] + 1)
// The combine's row term closes the round trip through both index arrays.
//
// Kernels. Five launches, none of which waits on another workgroup: no
// look-back, no flag in memory, no cooperative launch.
//
// moe_route_kernel<VECS>: 256 threads own 256 consecutive tokens; a token is one
// DPP row of 16 lanes, so a wave has four in hand and takes 16 trips. Lane c
// holds the packed keys of experts 8c .. 8c+7 (VECS = 1, experts <= 128) and
// 128 + 8c .. (VECS = 2): the 16 lanes read 256 contiguous bytes, 16 each. A
// row of `experts` that is no multiple of 8 is not 16-byte aligned and is read
// element by element; a vector is loaded only when it ends inside the row, so a
// row is never over-read. The row maximum and each knock-out round are four
// row_ror DPP steps (8, 4, 2, 1: a maximum may count an element twice, the
// rotation leaves every lane with the row's); the winner is knocked out by
// comparing packed values, which are unique, so no register is indexed by a
// lane-varying number; lane j keeps choice j and stores it. No LDS, no
// ds_bpermute.
//   DEPARTURE from the design this started from: the route kernel does not set
// mask bits or count. The sort is an operation on caller-owned topk_ids, which
// need not be what a route just left (the tests change one), and the scatter's
// addresses are safe only if the counts come from the SAME ids the scatter
// reads. So the count is the sort's first launch, from topk_ids; it costs a
// second read of slots * 4 bytes (1 MiB at the default shape).
//
// moe_route_count_kernel: the same blocks. Thread i takes token i's ids,
// clamped to [0, experts), and sets bit i of mask[e], a 256-bit token set per
// expert in LDS (8 KiB at 256 experts), by atomic OR: the result of an OR does
// not depend on order, which is the point. Thread e pop-counts its mask into
// block_counts[b][e], a workspace the library owns.
//
// moe_route_scan_kernel: one workgroup. Thread e walks the blocks, leaves the
// running sum in place (block_base[b][e]), and mg_scan over the experts'
// totals gives offsets.
//
// moe_route_scatter_kernel: the same blocks rebuild the masks; the rank of
// token i in expert e is the pop-count of mask[e] below bit i, slot =
// offsets[e] + block_base[b][e] + rank, row_ids[slot] = t, slot_of[t][j] =
// slot. Per (token, choice), NOT an expert-major walk of the mask bits: the walk
// would know a token's expert but not which of its choices j that was, and
// slot_of[t][j] needs j; its stores would be consecutive per THREAD, so no more
// coalesced across lanes than these, and an expert's tokens of a block have
// consecutive ranks, so the scattered stores fall in runs that L2 merges.
//
// moe_combine_kernel: one wave per 8 consecutive tokens, lane l the 16-byte
// vectors l, l + 64, .. of a row: top_k nontemporal loads, the FMA chain, one
// product, one nontemporal store. The next token's slots, weights and
// denominator are loaded before the current token's rows are waited for; the
// rows' first vectors are NOT prefetched into registers: at 8 tokens a wave the
// default shape has 8 waves on every SIMD, each with top_k * N/256 independent
// loads outstanding, which covers HBM latency without 32 more registers.
//   No block-to-XCD map: every row of Y belongs to exactly one (token, choice)
// and is read once, out is written once, so nothing of the stream is shared
// between workgroups and no L2 placement can save a byte. Only the index
// arrays (1/256 of the traffic at N = 1024) are reread.
//
// Robustness. No content of logits, topk_ids or slot_of makes a kernel read or
// write outside its arrays: ids are clamped to [0, experts) where they index
// the masks, slots to [0, slots) where they index Y and row_ids, and the
// scatter stores only below `slots`. Duplicate ids within a token in
// caller-supplied topk_ids collapse onto one mask bit (both choices get the
// same slot) and give offsets[experts] < slots, which the expert GEMM
// understands as dropped slots. Tokens past `tokens` in the last block load and
// store nothing.
//
// Error bounds of the operation on arbitrary bf16 logits (the tests assert
// them). The argument a = fl(scale * fl(x - m)) carries two f32 roundings, |a -
// exact| <= |a| 2^-23, which exp2 turns into a relative |a| 2^-23 ln 2;
// v_exp_f32 is documented to 1 ulp = 2^-23 and flushes results under 2^-126:
//   |p - exact| <= p (|a| 2^-23 ln 2 + 2 * 2^-23) + 2^-126     (one ulp spare)
//   |denom - exact| <= sum of the terms' bounds + terms * 2^-24 * denom.
// Combine: top_k roundings of the FMA chain, one of the reciprocal and one of
// the product, each 2^-24 relative to at most sum_j |p Y|:
//   |out - exact(p, denom)| <= (top_k + 2) 2^-24 (1 + 2^-20) sum_j |p Y| / denom.
//
// Compiler's result (hipcc -O3 --offload-arch=gfx950 -Xclang -target-feature
// -Xclang -packed-fp32-ops, -Rpass-analysis=kernel-resource-usage): see the
// table under MR_RESOURCES below.

#pragma once

#include "moegemmsweep.h"

#define MR_BLOCK_TOKENS MS_BLOCK   // tokens of a route, count or scatter workgroup
#define MR_MASK_WORDS (MR_BLOCK_TOKENS / 32)
#define MR_WAVE_TOKENS 8           // consecutive tokens of a combine wave
#define MR_COMBINE_TOKENS (MR_WAVE_TOKENS * MS_WAVES_PER_WG)
static_assert(MR_BLOCK_TOKENS == NA_MOE_ROUTE_BLOCK && MR_WAVE_TOKENS == NA_MOE_COMBINE_WAVE_TOKENS,
              "nodeagent.h tells callers otherwise");

// MR_RESOURCES (occupancy in waves per SIMD; 7 is the SGPRs', not the VGPRs')
//   moe_route_kernel<1>:      38 VGPRs,  83 SGPRs, LDS 0,    scratch 0, occupancy 8
//   moe_route_kernel<2>:      57 VGPRs, 106 SGPRs, LDS 0,    scratch 0, occupancy 7
//   moe_route_count_kernel:   10 VGPRs,  20 SGPRs, LDS 8192, scratch 0, occupancy 8
//   moe_route_scan_kernel:    51 VGPRs,  78 SGPRs, LDS 16,   scratch 0, occupancy 8
//   moe_route_scatter_kernel: 32 VGPRs,  55 SGPRs, LDS 8192, scratch 0, occupancy 8
//   moe_combine_kernel:       63 VGPRs, 106 SGPRs, LDS 0,    scratch 0, occupancy 7
//   moe_route_fill_kernel:    17 VGPRs,  36 SGPRs, LDS 0,    scratch 0, occupancy 8
// Measured (profiles/moe_route_sweep_mi355x.txt, 65536 tokens, 128 experts,
// top-4, N = 1024): route 34.0 us, count 4.6, scan 13.2, scatter 6.1, combine
// 251.7 us = 5333 GB/s, 0.91 of the HBM copy probe. The route is not bound by
// HBM (16 MiB in 34 us): 256 workgroups are one wave per SIMD, and a wave's 16
// trips each wait for their own load; more, smaller blocks or a load one trip
// ahead would shorten it and have not been tried.

// Where everything of a shape is in the hashed sequences (see "Hashed operands").
struct mr_layout {
    mt_u64 base;
    uint32_t tokens, experts, top_k, slots;
    __device__ __host__ mt_u64 front(mt_u64 i) const { return mt_mix64(base + i); }
    __device__ __host__ mt_u64 back(mt_u64 i) const { return mt_mix64(base - 1 - i); }
    __device__ __host__ int logit(mt_u64 t, mt_u64 e) const {
        return (int)((front(t) >> 40) % 7) - 3 -
               (int)((front((mt_u64)tokens + t * experts + e) >> 40) % 9);
    }
    __device__ __host__ mt_u64 w_id(mt_u64 s) const { return back(s) | 1; }
    __device__ __host__ mt_u64 w_p(mt_u64 s) const { return back((mt_u64)slots + s) | 1; }
    __device__ __host__ mt_u64 w_denom(mt_u64 t) const { return back(2ULL * slots + t) | 1; }
    __device__ __host__ mt_u64 w_slot(mt_u64 s) const {
        return back(2ULL * slots + tokens + s) | 1;
    }
    __device__ __host__ mt_u64 w_token(mt_u64 t) const {
        return back(3ULL * slots + tokens + t) | 1;
    }
    __device__ __host__ mt_u64 w_row(mt_u64 s) const {
        return back(3ULL * slots + 2ULL * tokens + s) | 1;
    }
    __device__ __host__ mt_u64 y_row(mt_u64 s) const { return back(4ULL * slots + 2ULL * tokens + s); }
    __device__ __host__ mt_u64 w_col(mt_u64 n) const {
        return back(5ULL * slots + 2ULL * tokens + n) | 1;
    }
    __device__ __host__ mt_u64 y_col(mt_u64 n, mt_u64 n_cols) const {
        return back(5ULL * slots + 2ULL * tokens + n_cols + n);
    }
};

// The two factors in {-1, 0, 1} that a row or a column of Y draws from x.
__device__ __host__ inline int mr_factor_a(mt_u64 x) { return (int)((x >> 40) % 3) - 1; }
__device__ __host__ inline int mr_factor_b(mt_u64 x) { return (int)((x >> 20) % 3) - 1; }

// bf16 bits to the order-preserving key; NaN of either sign to 0.
__device__ __host__ inline uint32_t mr_key(uint32_t b) {
    if ((b & 0x7FFF) > 0x7F80) return 0;
    return b & 0x8000 ? ~b & 0xFFFF : b | 0x8000;
}

// and back; key 0 gives a NaN's bits.
__device__ __host__ inline uint32_t mr_key_bits(uint32_t key) {
    if (key == 0) return 0x7FC0;
    return key & 0x8000 ? key & 0x7FFF : ~key & 0xFFFF;
}

static inline uint32_t mr_blocks(long long tokens) {
    return (uint32_t)((tokens + MR_BLOCK_TOKENS - 1) / MR_BLOCK_TOKENS);
}
static inline uint32_t mr_combine_blocks(long long tokens) {
    return (uint32_t)((tokens + MR_COMBINE_TOKENS - 1) / MR_COMBINE_TOKENS);
}

void mr_launch_fill(unsigned grid, unsigned short* logits, float* y, mr_layout at, uint32_t n_cols);
void mr_launch_route(na_mfma_record* records, const unsigned short* logits, int* topk_ids,
                     float* topk_p, float* denom, mr_layout at, float scale_log2, uint32_t renorm);
void mr_launch_sort(na_mfma_record* records, const int* topk_ids, int* block_counts, int* offsets,
                    int* row_ids, int* slot_of, mr_layout at, uint32_t wave0);
void mr_launch_combine(na_mfma_record* records, const float* y, const int* slot_of,
                       const int* row_ids, const float* topk_p, const float* denom, float* out,
                       mr_layout at, uint32_t n_cols, uint32_t wave0);

#ifdef AS_KERNELS

// One thread per logit, then one per 16-byte vector of Y (y may be null).
__global__ void __launch_bounds__(MS_BLOCK)
moe_route_fill_kernel(unsigned short* __restrict__ logits, float* __restrict__ y, mr_layout at,
                      uint32_t n_cols) {
#if defined(__gfx950__)
    const mt_u64 i = (mt_u64)blockIdx.x * MS_BLOCK + threadIdx.x;
    const mt_u64 n_logits = (mt_u64)at.tokens * at.experts;
    if (i < n_logits) {
        const float v = (float)at.logit(i / at.experts, i % at.experts);
        logits[i] = (unsigned short)(__builtin_bit_cast(uint32_t, v) >> 16);  // -11 .. 3: exact
        return;
    }
    const mt_u64 v = i - n_logits, row_vecs = n_cols / 4;
    if (y == nullptr || v >= (mt_u64)at.slots * row_vecs) return;
    const mt_u64 s = v / row_vecs, n0 = v % row_vecs * 4, xs = at.y_row(s);
    const int a = mr_factor_a(xs), b = mr_factor_b(xs);
    f32x4 out;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const mt_u64 xn = at.y_col(n0 + c, n_cols);
        out[c] = (float)(a * mr_factor_a(xn) + b * mr_factor_b(xn));
    }
    *reinterpret_cast<f32x4*>(y + v * 4) = out;
#endif
}

#if defined(__gfx950__)

// Every lane of a DPP row of 16 gets the row's maximum, or its sum: four
// rotations within the row (row_ror:8, 4, 2, 1).
template <int ROR>
__device__ inline int mr_row_ror(int v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x120 + ROR, 0xF, 0xF, false);
}
__device__ inline int mr_row_max(int v) {
    v = max(v, mr_row_ror<8>(v));
    v = max(v, mr_row_ror<4>(v));
    v = max(v, mr_row_ror<2>(v));
    return max(v, mr_row_ror<1>(v));
}
__device__ inline float mr_row_sum(float v) {
    v += __builtin_bit_cast(float, mr_row_ror<8>(__builtin_bit_cast(int, v)));
    v += __builtin_bit_cast(float, mr_row_ror<4>(__builtin_bit_cast(int, v)));
    v += __builtin_bit_cast(float, mr_row_ror<2>(__builtin_bit_cast(int, v)));
    return v + __builtin_bit_cast(float, mr_row_ror<1>(__builtin_bit_cast(int, v)));
}

__device__ inline float mr_key_value(uint32_t key) {
    return __builtin_bit_cast(float, mr_key_bits(key) << 16);
}

__device__ inline mt_u64 mr_wave_sum(mt_u64 sum) {
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    return sum;
}

// Lane 0 of the wave writes records[index], which is record wave0 + index of
// the three kernels' common numbering.
__device__ inline void mr_leave(na_mfma_record* records, uint32_t index, uint32_t wave0, mt_u64 sum,
                                ms_clock t0, ms_clock t1, ms_hw_where at) {
    sum = mr_wave_sum(sum);
    if ((threadIdx.x & 63) != 0) return;
    na_mfma_record rec;
    rec.checksum = sum;
    rec.wave = wave0 + index;
    ms_record_simd(rec, t0, t1, at);
    records[index] = rec;
}

// Sets bit i of mask[e] for the block's token i and each of its ids; the
// caller's barrier makes the masks whole. Called by all 256 threads.
__device__ inline void mr_build_masks(uint32_t* mask, const int* __restrict__ topk_ids,
                                      const mr_layout& at, int (&ids)[NA_MOE_MAX_TOPK]) {
    const uint32_t i = threadIdx.x, t = blockIdx.x * MR_BLOCK_TOKENS + i;
    for (uint32_t w = i; w < at.experts * MR_MASK_WORDS; w += MS_BLOCK) mask[w] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NA_MOE_MAX_TOPK; ++j) {
        ids[j] = 0;
        if (t < at.tokens && j < (int)at.top_k) {
            ids[j] = min(max(topk_ids[(size_t)t * at.top_k + j], 0), (int)at.experts - 1);
            atomicOr(&mask[ids[j] * MR_MASK_WORDS + (i >> 5)], 1u << (i & 31));
        }
    }
    __syncthreads();
}

#endif  // __gfx950__

// records: 4 per block of 256 tokens. Launch with mr_blocks(tokens) workgroups
// of MS_BLOCK threads. VECS: 16-byte vectors of a row a lane holds, 1 for up
// to 128 experts, 2 beyond.
template <int VECS>
__global__ void __launch_bounds__(MS_BLOCK)
moe_route_kernel(na_mfma_record* __restrict__ records, const unsigned short* __restrict__ logits,
                 int* __restrict__ topk_ids, float* __restrict__ topk_p,
                 float* __restrict__ denom, mr_layout at, float scale_log2, uint32_t renorm) {
    const uint32_t wave = threadIdx.x >> 6;
#if defined(__gfx950__)
    constexpr int KEYS = 8 * VECS;
    const ms_hw_where where = ms_where();
    const uint32_t l = threadIdx.x & 63, row = l >> 4, c = l & 15;
    const bool aligned = at.experts % 8 == 0;
    const ms_clock t0 = ms_stamp();
    mt_u64 sum = 0;
    for (uint32_t trip = 0; trip < 16; ++trip) {
        const uint32_t t = blockIdx.x * MR_BLOCK_TOKENS + wave * 64 + trip * 4 + row;
        const bool live = t < at.tokens;
        const unsigned short* const mine = logits + (size_t)(live ? t : 0) * at.experts;
        int pk[KEYS];
#pragma unroll
        for (int v = 0; v < VECS; ++v) {
            const uint32_t e0 = (v * 16 + c) * 8;
            unsigned short bits[8] = {};
            if (live && aligned && e0 + 8 <= at.experts) {
                const mt_vec got = *reinterpret_cast<const mt_vec*>(mine + e0);
                __builtin_memcpy(bits, &got, sizeof(bits));
            } else if (live) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (e0 + i < at.experts) bits[i] = mine[e0 + i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                pk[v * 8 + i] = live && e0 + i < at.experts
                                    ? (int)(mr_key(bits[i]) << 8 | (255 - (e0 + i)))
                                    : -1;
        }
        int best = pk[0];
#pragma unroll
        for (int i = 1; i < KEYS; ++i) best = max(best, pk[i]);
        best = mr_row_max(best);
        // m: the largest logit, 0 when that is a NaN (then all are) or no token
        const uint32_t top_key = best < 0 ? 0 : (uint32_t)best >> 8;
        const float m = top_key == 0 ? 0.f : mr_key_value(top_key);
        auto weight = [&](uint32_t key) {
            return key == 0 ? 0.f : __builtin_amdgcn_exp2f(scale_log2 * (mr_key_value(key) - m));
        };
        float total = 0.f;
        if (!renorm) {
#pragma unroll
            for (int i = 0; i < KEYS; ++i)
                if (pk[i] >= 0) total += weight((uint32_t)pk[i] >> 8);
            total = mr_row_sum(total);
        }
        int my_id = 0;
        float my_p = 0.f;
        for (uint32_t j = 0; j < at.top_k; ++j) {
            if (j > 0) {
                best = pk[0];
#pragma unroll
                for (int i = 1; i < KEYS; ++i) best = max(best, pk[i]);
                best = mr_row_max(best);
            }
            const int id = best < 0 ? 0 : 255 - (best & 255);
            const float p = best < 0 ? 0.f : weight((uint32_t)best >> 8);
            if (renorm) total += p;
            if (c == j) my_id = id, my_p = p;
#pragma unroll
            for (int i = 0; i < KEYS; ++i)
                if (pk[i] == best) pk[i] = -1;  // packed values are unique: the winner's lane only
        }
        if (live && c < at.top_k) {
            const size_t s = (size_t)t * at.top_k + c;
            topk_ids[s] = my_id;
            topk_p[s] = my_p;
            sum += at.w_id(s) * (mt_u64)(long long)my_id +
                   at.w_p(s) * (mt_u64)(long long)(int)(256.f * my_p);
        }
        if (live && c == 0) {
            denom[t] = total;
            sum += at.w_denom(t) * (mt_u64)(long long)(int)(256.f * total);
        }
    }
    mr_leave(records, blockIdx.x * MS_WAVES_PER_WG + wave, 0, sum, t0, ms_stamp(), where);
#else
    if ((threadIdx.x & 63) == 0) {  // wrong arch: a checksum no reference produces
        na_mfma_record rec = {};
        rec.checksum = ~0ULL;
        records[blockIdx.x * MS_WAVES_PER_WG + wave] = rec;
    }
#endif
}

// block_counts: mr_blocks(tokens) x experts. Launch as the route kernel.
__global__ void __launch_bounds__(MS_BLOCK)
moe_route_count_kernel(const int* __restrict__ topk_ids, int* __restrict__ block_counts,
                       mr_layout at) {
#if defined(__gfx950__)
    __shared__ uint32_t mask[NA_MOE_MAX_EXPERTS * MR_MASK_WORDS];
    int ids[NA_MOE_MAX_TOPK];
    mr_build_masks(mask, topk_ids, at, ids);
    const uint32_t e = threadIdx.x;
    if (e >= at.experts) return;
    int count = 0;
#pragma unroll
    for (int w = 0; w < MR_MASK_WORDS; ++w) count += __popc(mask[e * MR_MASK_WORDS + w]);
    block_counts[(size_t)blockIdx.x * at.experts + e] = count;
#endif
}

// One workgroup of MS_BLOCK threads. block_counts becomes block_base in place:
// the tokens of earlier blocks that chose the expert. offsets: experts + 1.
__global__ void __launch_bounds__(MS_BLOCK)
moe_route_scan_kernel(int* __restrict__ block_counts, int* __restrict__ offsets, mr_layout at,
                      uint32_t blocks) {
#if defined(__gfx950__)
    __shared__ uint32_t four[4];
    const uint32_t e = threadIdx.x;
    uint32_t total = 0;
    if (e < at.experts) {
        // 16 blocks' loads in flight ahead of their stores: in place, the
        // compiler may not move a load over a store by itself
        for (uint32_t b0 = 0; b0 < blocks; b0 += 16) {
            int* const at_b = block_counts + (size_t)b0 * at.experts + e;
            uint32_t count[16];
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i)
                count[i] = b0 + i < blocks ? (uint32_t)at_b[(size_t)i * at.experts] : 0;
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                if (b0 + i < blocks) at_b[(size_t)i * at.experts] = (int)total;
                total += count[i];
            }
        }
    }
    const uint32_t upto =
        mg_scan(total, four, nullptr, [](uint32_t a, uint32_t b) { return a + b; });
    if (e < at.experts) offsets[e] = (int)(upto - total);
    if (e == at.experts - 1) offsets[at.experts] = (int)upto;
#endif
}

// records: 4 per block, numbered from wave0. Launch as the route kernel, after the
// scan.
__global__ void __launch_bounds__(MS_BLOCK)
moe_route_scatter_kernel(na_mfma_record* __restrict__ records, const int* __restrict__ topk_ids,
                         const int* __restrict__ block_base, const int* __restrict__ offsets,
                         int* __restrict__ row_ids, int* __restrict__ slot_of, mr_layout at,
                         uint32_t wave0) {
    const uint32_t wave = threadIdx.x >> 6;
#if defined(__gfx950__)
    __shared__ uint32_t mask[NA_MOE_MAX_EXPERTS * MR_MASK_WORDS];
    const ms_hw_where where = ms_where();
    const ms_clock t0 = ms_stamp();
    int ids[NA_MOE_MAX_TOPK];
    mr_build_masks(mask, topk_ids, at, ids);
    const uint32_t i = threadIdx.x, t = blockIdx.x * MR_BLOCK_TOKENS + i;
    const int* const base = block_base + (size_t)blockIdx.x * at.experts;
    mt_u64 sum = 0;
#pragma unroll
    for (int j = 0; j < NA_MOE_MAX_TOPK; ++j) {
        if (t >= at.tokens || j >= (int)at.top_k) continue;
        const uint32_t* const bits = mask + ids[j] * MR_MASK_WORDS;
        uint32_t rank = __popc(bits[i >> 5] & ((1u << (i & 31)) - 1));
        for (uint32_t w = 0; w < (i >> 5); ++w) rank += __popc(bits[w]);
        const uint32_t slot = (uint32_t)offsets[ids[j]] + (uint32_t)base[ids[j]] + rank;
        const size_t s = (size_t)t * at.top_k + j;
        if (slot < at.slots) row_ids[slot] = (int)t;  // always, when count and scan ran on these ids
        slot_of[s] = (int)slot;
        sum += at.w_slot(s) * (mt_u64)(slot + 1);
    }
    mr_leave(records, blockIdx.x * MS_WAVES_PER_WG + wave, wave0, sum, t0, ms_stamp(), where);
#else
    if ((threadIdx.x & 63) == 0) {
        na_mfma_record rec = {};
        rec.checksum = ~0ULL;
        records[blockIdx.x * MS_WAVES_PER_WG + wave] = rec;
    }
#endif
}

#if defined(__gfx950__)
// What a combine wave needs of a token: uniform over the wave.
struct mr_token {
    uint32_t slot[NA_MOE_MAX_TOPK];
    float p[NA_MOE_MAX_TOPK];
    float denom;
};

__device__ inline mr_token mr_load_token(uint32_t t, const int* __restrict__ slot_of,
                                         const float* __restrict__ topk_p,
                                         const float* __restrict__ denom, const mr_layout& at) {
    mr_token k = {};
    if (t >= at.tokens) return k;
#pragma unroll
    for (int j = 0; j < NA_MOE_MAX_TOPK; ++j) {
        if (j >= (int)at.top_k) continue;
        const size_t s = (size_t)t * at.top_k + j;
        k.slot[j] = (uint32_t)min(max(slot_of[s], 0), (int)at.slots - 1);
        k.p[j] = topk_p[s];
    }
    k.denom = denom[t];
    return k;
}
#endif

// records: one per wave, 4 * mr_combine_blocks(tokens), numbered from wave0.
// Launch with mr_combine_blocks(tokens) workgroups of MS_BLOCK threads.
__global__ void __launch_bounds__(MS_BLOCK)
moe_combine_kernel(na_mfma_record* __restrict__ records, const float* __restrict__ y,
                   const int* __restrict__ slot_of, const int* __restrict__ row_ids,
                   const float* __restrict__ topk_p, const float* __restrict__ denom,
                   float* __restrict__ out, mr_layout at, uint32_t n_cols, uint32_t wave0) {
    const uint32_t wave = blockIdx.x * MS_WAVES_PER_WG + (threadIdx.x >> 6);
#if defined(__gfx950__)
    const ms_hw_where where = ms_where();
    const uint32_t l = threadIdx.x & 63, row_vecs = n_cols / 4;
    const uint32_t first = __builtin_amdgcn_readfirstlane(wave) * MR_WAVE_TOKENS;
    const ms_clock t0 = ms_stamp();
    mt_u64 sum = 0;
    mr_token next = mr_load_token(first, slot_of, topk_p, denom, at);
    for (uint32_t t = first; t < first + MR_WAVE_TOKENS && t < at.tokens; ++t) {
        const mr_token now = next;
        next = mr_load_token(t + 1 < first + MR_WAVE_TOKENS ? t + 1 : at.tokens, slot_of, topk_p,
                             denom, at);
        const float r = 1.f / now.denom;
        const mt_u64 w_t = at.w_token(t);
        if (l < at.top_k)  // lane j reads choice j's row id back
            sum += at.w_row((mt_u64)t * at.top_k + l) *
                   (mt_u64)(long long)(row_ids[min(max(slot_of[(size_t)t * at.top_k + l], 0),
                                                   (int)at.slots - 1)] + 1);
        for (uint32_t v = l; v < row_vecs; v += 64) {
            f32x4 got[NA_MOE_MAX_TOPK];
#pragma unroll
            for (int j = 0; j < NA_MOE_MAX_TOPK; ++j)
                if (j < (int)at.top_k)
                    got[j] = __builtin_nontemporal_load(
                        reinterpret_cast<const f32x4*>(y + (size_t)now.slot[j] * n_cols) + v);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NA_MOE_MAX_TOPK; ++j)
                if (j < (int)at.top_k)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(now.p[j], got[j][i], acc[i]);
            mt_u64 inner = 0;
            f32x4 scaled;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                inner += at.w_col(4 * v + i) * (mt_u64)(long long)(int)(256.f * acc[i]);
                scaled[i] = acc[i] * r;
            }
            sum += w_t * inner;
            __builtin_nontemporal_store(scaled, reinterpret_cast<f32x4*>(out + (size_t)t * n_cols) + v);
        }
    }
    mr_leave(records, wave, wave0, sum, t0, ms_stamp(), where);
#else
    if ((threadIdx.x & 63) == 0) {
        na_mfma_record rec = {};
        rec.checksum = ~0ULL;
        records[wave] = rec;
    }
#endif
}

#endif  // AS_KERNELS
