// Chip-wide decode-size MoE expert GEMM sweep for the MI355X node agent, and the
// skinny expert GEMM it runs as an operation on caller-owned tensors (included
// from agent.hip for the host side and from attnsweep.hip, under AS_KERNELS, for
// the kernel; the problem, its operands, its hashed fill, the weights p and q,
// the argument limits and the tile search are moegemmsweep.h's).
//
// moegemmsweep.h tiles 128 slots by 256 columns and assumes that the MFMAs are
// the limit. In decode a batch of 32-256 tokens routed top-4 to top-8 over 128-256
// experts leaves 1-16 slots per expert: every byte of every active expert's
// weights is read once for a handful of rows, and the limit is HBM. This kernel
// is that regime: the same operation
//
//   C[s][:] = reps * X[row_ids[s]][:] * W[e]^T   for offsets[e] <= s < offsets[e+1]
//
// on the same tensors (na_moe_gemm_fill's buffers serve both kernels unchanged),
// N a multiple of 256, K a multiple of the GEMM sweep's BK, 6 * reps * K <
// NA_GEMM_EXACT, experts <= 256. Only the tiling, the data path, the record
// numbering and the figure of merit (bytes per second) are new. Its failure
// classes are its own: a 16-row tile given the neighbouring expert's weights, a
// tail slot leaking at a 16-row granule, a CU whose direct global-to-MFMA path
// is bad while its LDS-staged path is fine.
//
// Tiles are NA_MOE_SKINNY_TILE_M = 16 slots by 256 columns and never span two
// experts. Expert e with cnt_e slots owns ceil(cnt_e / 16) * N/256 tiles; tiles
// are numbered expert-major, then column tile, then row tile: row tile FASTEST
// (mg_find_tile<16, true>). The host never reads offsets: it launches the bound
// (floor(slots / 16) + experts) * N/256 workgroups of 256 threads, and surplus
// workgroups leave four idle records and return as a whole, as in
// moegemmsweep.h. With mg_tile_of_block's contiguous range of tiles per XCD the
// 2-4 row tiles of an expert with 17-64 slots are neighbours in one XCD's range,
// start next to each other and can take the weight slab they share from that
// XCD's L2 and not a second time from HBM. That is reasoned; what the
// measurement says of it is below and in profiles/moe_skinny_sweep_mi355x.txt.
//
// Transposed product. The tile is C^T = W * X_g^T on v_mfma_f32_16x16x32 through
// ms_traits<DTYPE>: sixteen rows of W[e], which are sixteen output columns, are
// the A operand, the tile's sixteen gathered slots are B. Wave w of the four owns
// columns 64 w .. 64 w + 63 of the tile over all of K: four accumulators of
// f32x4, sixteen registers; no split-K, nothing to merge. Accumulator register r
// of block j in lane (x = l & 15, g = l >> 4) is column 64 w + 16 j + 4 g + r of
// slot x: four consecutive floats of one row of C, one 16-byte store.
//
// W never touches LDS. A dot product does not depend on a permutation of K
// applied to both operands alike (decodesweep.h's argument for K and Q), so lane
// (x, g) takes 16-byte vector 4 c + g of the k-step of ITS weight row 64 w + 16 j
// + x straight from global memory as its A fragment of sub-step c = 0, 1 (bf16:
// the natural order; E4M3: the two 8-byte halves of the vector are two MFMAs, a
// permutation of the 32 k of each, gs_frag's split) and X's B fragment is vector
// 4 c + g of slot x, the same permutation. One load instruction covers 64
// contiguous bytes of each of 16 rows, the two sub-steps a row's 128 bytes: whole
// cache lines, each byte of W requested once per tile. The address is a uniform
// base in scalar registers plus a 32-bit lane offset, as gemmsweep.h's.
//
// k-step: the GEMM sweep's 128 bytes per row (so the K limit is unchanged): 8
// vectors of W per lane, 2 MFMAs (bf16) or 4 (E4M3) per accumulator. The NEXT
// k-step's eight vectors are loaded ahead of the MFMAs of the current one and
// held in registers: two sets of 32 registers, the loop unrolled by two so that
// the sets swap by name and not by copy. The last step loads nothing and is
// peeled off the loop. A wave therefore keeps 8 KiB of W in flight and a
// workgroup 32 KiB; registers are budgeted for occupancy, not for accumulators
// (amdgpu_waves_per_eu(4, 4): four waves per SIMD, at most 128 registers), so
// four workgroups share a CU and 128 KiB of W are in flight per CU, 32 MiB on 256
// CUs: at 8 TB/s that covers 4 us of latency.
// Compiler's result (hipcc -O3 --offload-arch=gfx950 -Xclang -target-feature
// -Xclang -packed-fp32-ops, -Rpass-analysis=kernel-resource-usage):
//   moe_skinny_kernel<bf16>: 98 VGPRs, 0 AGPRs, 56 SGPRs, scratch 0, occupancy 4
//   moe_skinny_kernel<fp8>:  98 VGPRs, 0 AGPRs, 56 SGPRs, scratch 0, occupancy 4
// LDS 4096 bytes static. Four workgroups per CU by registers (LDS would allow 40).
// Measured (profiles/moe_skinny_sweep_mi355x.txt, median of five processes, the
// default sweep's decode step on 1 GiB of bf16 weights): 5199.1 GB/s, 0.88 of the
// package's HBM probe in the same processes; a pass takes 0.187 ms where
// moe_gemm_kernel takes 0.329 ms on the same tensors (1.76 x), and with uniform
// counts the 128-row kernel catches up between 32 and 48 slots per expert. The
// second row tile of an expert costs 0.46 of the first (0.282 ms at 17 slots
// everywhere against 0.192 ms at 16), not 1.0: the L2 reuse reasoned above is
// borne out in part.
//
// X through LDS, once per workgroup, shared by the four waves. A stage is the
// tile's 16 gathered rows x 128 bytes of one k-step, 2 KiB; two stages, 4 KiB:
// LDS is not what limits the workgroups per CU (the static_assert below states
// the four the registers allow). Thread t owns 8-byte half t & 1 of vector (t >> 1)
// & 7 of slab row t >> 4: it reads that row's id once per tile, clamped to [0,
// tokens), keeps one row pointer, loads its half of the next k-step FIRST in a
// step (ahead of the eight of W, so that waiting for it leaves those in flight)
// and writes it to the other stage after the step's MFMAs; one __syncthreads per
// k-step hands the stage over, with gemmsweep.h's reasoning. X is small (tokens x
// K) and lives in L2. Rows at or past the tile's valid count load the expert's LAST VALID row;
// they are masked at the C store and in the checksum, never in the K loop
// (column x of C^T depends on column x of B alone, moegemmsweep.h's rule
// transposed). So NaN in a row of X that no slot names never reaches C, and the
// K loop runs the same instructions for a tile of 1 slot and of 16.
// Layout: gemmsweep.h's chunk swizzle, row r stores vector c at position c ^ ((r
// >> 1) & 7). A B-fragment read is ds_read_b128 of row x, position (4 c + g) ^
// ((x >> 1) & 7): the sixteen lanes of one g take rows 0..15 at one vector index
// and so bank byte (x & 1) * 128 + 16 * ((4 c + g) ^ (x >> 1)), sixteen distinct
// 16-byte groups, all 256 bytes of the 64 banks: no conflict. The writer's
// thirty-two consecutive lanes (ds_write_b64) cover two whole rows, again all 256
// bytes. Derived, not measured.
//
// Safety, unchanged from moegemmsweep.h: the tile search clamps offsets to [0,
// slots] and makes them monotone, so a tile's slots are inside row_ids and its
// expert below `experts`; row ids are clamped; W is read at rows below N and
// k-steps below K / BK of that expert; C is written at the tile's valid slots
// only. No content of offsets or row_ids takes a read outside the four arrays or
// a write outside the valid slots of C.
//
// Records: 4 * tile + w for wave w, na_mfma_record, checksum
//
//   sum p_s * q_j * (uint64)(int64)C[s][j]
//
// over the wave's 64 columns and the tile's valid rows, formed in 64-bit integer
// VALU from the accumulators; placement and clocks through ms_record_simd; idle
// records as moegemmsweep.h's. `reps` repeats the K loop into the same
// accumulators, which keeps the operation's contract and its exactness test. The
// sweep itself times whole launches of reps = 1, several in its window: that is
// an HBM figure, where a repeat inside the kernel re-reads a tile's 256-row slab
// and would be a cache figure.

#pragma once

#include "moegemmsweep.h"

#define SK_TILE_M 16
#define SK_FRAGS 4  // 16-column accumulator blocks per wave: 64 columns
#define SK_STAGE_VECS (SK_TILE_M * GS_ROW_VECS)  // 2 KiB
#define SK_LDS_BYTES (2 * SK_STAGE_VECS * 16)
#define SK_WGS_PER_CU 4  // by registers: amdgpu_waves_per_eu(4, 4)
static_assert(SK_TILE_M == NA_MOE_SKINNY_TILE_M && MS_WAVES_PER_WG * SK_FRAGS * 16 == MG_TILE_N,
              "nodeagent.h tells callers otherwise; four waves of 64 columns are a tile");
static_assert(SK_WGS_PER_CU * SK_LDS_BYTES <= MS_CU_LDS_BYTES && 2 * SK_STAGE_VECS == MS_BLOCK,
              "four workgroups share a CU's LDS; a thread stages half a vector of X");

void sk_launch_sweep(int dtype, unsigned grid, na_mfma_record* records, const mt_vec* x,
                     const mt_vec* w, const int* row_ids, const int* offsets, float* c,
                     uint32_t tokens, uint32_t slots, uint32_t experts, uint32_t nt,
                     uint32_t ksteps, uint32_t reps, mt_u64 wbase);

#ifdef AS_KERNELS

// records: 4 * (slots / 16 + experts) * nt entries. x, w, row_ids, offsets, c,
// wbase: moe_gemm_kernel's, c 16-byte aligned. Launch with (slots / 16 + experts)
// * nt workgroups of MS_BLOCK threads.
template <int DTYPE>
__global__ void __launch_bounds__(MS_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4)))
moe_skinny_kernel(na_mfma_record* __restrict__ records, const mt_vec* __restrict__ x,
                  const mt_vec* __restrict__ w, const int* __restrict__ row_ids,
                  const int* __restrict__ offsets, float* __restrict__ c, uint32_t tokens,
                  uint32_t slots, uint32_t experts, uint32_t nt, uint32_t ksteps, uint32_t reps,
                  mt_u64 wbase) {
    const int wave = threadIdx.x >> 6;
#if defined(__gfx950__)
    typedef ms_traits<DTYPE> T;
    constexpr int HALVES = sizeof(mt_vec) / sizeof(typename T::frag);
    __shared__ mt_vec sk_lds[2 * SK_STAGE_VECS];
    const ms_hw_where at = ms_where();
    const int l = threadIdx.x & 63, lx = l & 15, lg = l >> 4;
    const size_t pitch = (size_t)ksteps * GS_ROW_VECS;  // vectors per operand row

    const ms_clock t0 = ms_stamp();

    // stage 1: first written at the end of the first k-step
    const mg_tile tile = mg_find_tile<SK_TILE_M, true>(
        reinterpret_cast<uint32_t*>(sk_lds + 2 * SK_STAGE_VECS) - 16, offsets, slots, experts, nt,
        blockIdx.x);
    na_mfma_record* const mine = records + (size_t)tile.index * MS_WAVES_PER_WG + wave;
    if (tile.idle) {
        if (l == 0) {
            na_mfma_record rec;
            rec.checksum = 0;
            rec.wave = tile.index * MS_WAVES_PER_WG + wave;
            ms_record_simd(rec, t0, ms_stamp(), at);
            *mine = rec;
        }
        return;
    }

    // X, global -> LDS: thread t owns 8-byte half t & 1 of vector (t >> 1) & 7 of slab
    // row t >> 4, so all 256 threads move the stage's 2 KiB and no wave branches.
    const int srow = threadIdx.x >> 4, piece = threadIdx.x & 15;
    const uint32_t row = min((uint32_t)srow, tile.valid - 1);  // tail: the last valid row
    const uint32_t id = (uint32_t)min(max(row_ids[tile.first + row], 0), (int)tokens - 1);
    const mt_u64* const gx = reinterpret_cast<const mt_u64*>(x + (size_t)id * pitch) + piece;
    mt_u64* const put = reinterpret_cast<mt_u64*>(sk_lds) + srow * 2 * GS_ROW_VECS +
                        2 * ((piece >> 1) ^ ((srow >> 1) & 7)) + (piece & 1);
    // LDS -> B fragment: vector 4 c + lg of slot lx
    const int get = lx * GS_ROW_VECS + (lg ^ ((lx >> 1) & 7));
    // W, global -> A fragments: vector 4 c + lg of row 16 j + lx of the wave's 64,
    // a uniform base plus a 32-bit lane offset (15 rows of under 2^20 vectors)
    const uint32_t uwave = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
    const mt_vec* const gw =
        w + (((size_t)tile.expert * nt + tile.tj) * MG_TILE_N + uwave * (SK_FRAGS * 16)) * pitch;
    const uint32_t lane_vec = (uint32_t)lx * (uint32_t)pitch + (uint32_t)lg;

    f32x4 acc[SK_FRAGS];
#pragma unroll
    for (int j = 0; j < SK_FRAGS; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // The K loop, `reps` times into the same accumulators, as one sequence of
    // reps * ksteps steps. A step issues the next step's loads (X's ahead of W's
    // eight), runs its MFMAs on the registers the step before loaded and on the
    // stage it filled, writes X to the other stage and meets the other waves at
    // the barrier. The last step issues nothing and is peeled off the loop: a
    // load under a condition would make the compiler wait for ALL loads in flight
    // at the join, the next step's among them. Every tile, of 1 slot or of 16,
    // runs exactly this; every branch is uniform in the workgroup.
    mt_vec wa[SK_FRAGS][2], wb[SK_FRAGS][2];
    mt_u64 xr;
    uint32_t ks = 0;  // the step being loaded
    auto issue = [&](mt_vec(&regs)[SK_FRAGS][2]) {
        xr = gx[(size_t)ks * 2 * GS_ROW_VECS];
#pragma unroll
        for (int j = 0; j < SK_FRAGS; ++j)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                regs[j][s] = (gw + ((size_t)j * 16 * pitch + (size_t)ks * GS_ROW_VECS + 4 * s))[lane_vec];
    };
    auto hand_over = [&](uint32_t stage) {  // xr to `stage`, which nobody reads before the barrier
        put[stage * 2 * SK_STAGE_VECS] = xr;
        __syncthreads();
        ks = ks + 1 == ksteps ? 0 : ks + 1;
    };
    auto compute = [&](const mt_vec(&regs)[SK_FRAGS][2], uint32_t stage) {
        const mt_vec* const s = sk_lds + stage * SK_STAGE_VECS;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const mt_vec fb = s[get ^ (sub * 4)];
#pragma unroll
            for (int h = 0; h < HALVES; ++h)
#pragma unroll
                for (int j = 0; j < SK_FRAGS; ++j)
                    acc[j] = T::mfma(gs_frag<T>(regs[j][sub], h), gs_frag<T>(fb, h), acc[j]);
        }
    };

    issue(wa);
    hand_over(0);
    const uint32_t total = reps * ksteps;
    uint32_t it = 0;
    for (; it + 2 < total; it += 2) {
        issue(wb);
        compute(wa, 0);
        hand_over(1);
        issue(wa);
        compute(wb, 1);
        hand_over(0);
    }
    if (total - it == 2) {
        issue(wb);
        compute(wa, 0);
        hand_over(1);
        compute(wb, 1);
    } else {
        compute(wa, 0);
    }

    const ms_clock t1 = ms_stamp();

    // This lane's sixteen elements are columns col0 + 16 j + r of slot first + lx.
    const uint32_t col0 = tile.tj * MG_TILE_N + wave * (SK_FRAGS * 16) + lg * 4;
    const uint32_t n_cols = nt * MG_TILE_N;
    mt_u64 sum = 0;
    if ((uint32_t)lx < tile.valid) {  // else the next expert's slot, or nobody's
        mt_u64 inner = 0;
#pragma unroll
        for (int j = 0; j < SK_FRAGS; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                inner += gs_weight(wbase + slots + col0 + j * 16 + r) *
                         (mt_u64)(long long)(int)acc[j][r];
        sum = gs_weight(wbase + tile.first + lx) * inner;
        if (c != nullptr) {
            float* const out = c + ((size_t)(tile.first + lx) * n_cols + col0);
#pragma unroll
            for (int j = 0; j < SK_FRAGS; ++j) *reinterpret_cast<f32x4*>(out + j * 16) = acc[j];
        }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (l == 0) {
        na_mfma_record rec;
        rec.checksum = sum;
        rec.wave = tile.index * MS_WAVES_PER_WG + wave;
        ms_record_simd(rec, t0, t1, at);
        *mine = rec;
    }
#else
    // wrong arch: a checksum no reference produces, so verification fails
    if ((threadIdx.x & 63) == 0) {
        na_mfma_record rec = {};
        rec.checksum = ~0ULL;
        records[(size_t)blockIdx.x * MS_WAVES_PER_WG + wave] = rec;
    }
#endif
}

#endif  // AS_KERNELS
