// Chip-wide MoE grouped GEMM sweep for the MI355X node agent, and the expert
// GEMM it runs as an operation on caller-owned tensors (included from
// agent.hip for the host side and from attnsweep.hip, under AS_KERNELS, for the
// kernels: that translation unit is built with the packed-f32 VALU forms
// turned off, which a kernel whose claim is bit-exactness does not stand on;
// hashed operands, MFMA traits, the fragment split and the chunk swizzle are
// gemmsweep.h's).
//
// The GEMM sweep multiplies contiguous rows in tiles the host lays out. The
// matrix FLOPs of a mixture-of-experts model are in the expert GEMM, which
// gathers its rows through an index array, has a ragged row count per expert
// (0, 1, 129, ...) and learns those counts from device memory. Its failure
// classes are its own: a wrong gathered address, a tail row leaking into the
// neighbouring expert, a tile given to the wrong expert's weights, a CU that
// computes dense tiles correctly and ragged ones wrongly.
//
// The problem (normative; tests/test_nodeagent_moegemmsweep.py carries an
// independent numpy copy):
//
//   C[s][:] = reps * X[row_ids[s]][:] * W[e]^T
//   for every slot s with offsets[e] <= s < offsets[e+1].
//
//   X:        [tokens][K], K-contiguous, bf16 or E4M3 bytes.
//   W:        [experts][N][K], K-contiguous, the dtype of X.
//   row_ids:  int32[slots] on the device: the routing result sorted by expert.
//             With top-k routing a token's row appears in k slots.
//   offsets:  int32[experts + 1] on the device. offsets[experts] may be below
//             `slots`: the trailing slots are dropped tokens and their rows of
//             C are never written.
//   C:        float[slots][N], optional (null pointer).
//   N a multiple of NA_MOE_TILE_N = 256; K a multiple of the GEMM sweep's BK
//   (64 elements for bf16, 128 for fp8); experts <= NA_MOE_MAX_EXPERTS = 256;
//   6 * reps * K < NA_GEMM_EXACT for the hashed operands. Only M is ragged.
//
// Tiles are NA_MOE_TILE_M = 128 slots by 256 columns and never span two
// experts. Expert e with cnt_e slots owns ceil(cnt_e / 128) * N/256 tiles;
// tiles are numbered expert-major, then row tile, then column tile. Wave (wr,
// wc) = (wave>>1, wave&1) of the tile's four holds rows 64*wr.. and columns
// 128*wc.. and leaves record 4 * tile + 2 * wr + wc, whose checksum is
//
//   sum p_s * q_j * (uint64)(int64)C[s][j]
//
// over the VALID rows of the wave's sub-tile (s below the expert's end), 0 for
// a sub-tile with no valid row. Arithmetic mod 2^64, G = MS_G, mix64 =
// mt_mix64, base = seed * G, and with gs_element's moduli 7 and 5:
//
//   X[t][k]    = ((mix64(base + t*K + k) >> 40) % 7) - 3
//   W[e][j][k] = ((mix64(base + tokens*K + (e*N + j)*K + k) >> 40) % 5) - 2
//   p_s        = mix64(base + tokens*K + experts*N*K + s) | 1
//   q_j        = mix64(base + tokens*K + experts*N*K + slots + j) | 1
//   row_ids[s] = mix64(base - 1 - s) % tokens        (duplicates are wanted)
//   offsets    = the prefix sums of the host's counts[experts]
//
// Tile list on the device. The host never reads offsets: it launches the upper
// bound (floor(slots / 128) + experts) * N/256 workgroups (sum_e ceil(cnt_e /
// 128) <= floor(sum_e cnt_e / 128) + experts), and every workgroup derives its
// tile (mg_find_tile): thread e takes expert e; a wave scan and four words of
// LDS give the running maximum of the offsets clamped to [0, slots], which
// makes them monotone on the fly: expert e is slots [m_e, max(m_e,
// offsets[e+1])), m_e = max_{i<=e} offsets[i], so ranges never overlap and
// never leave row_ids whatever offsets holds; a second scan of ceil(cnt_e /
// 128) gives every expert its first row tile and the total R; the thread whose
// range of row tiles holds the workgroup's writes (expert, first slot, valid
// rows) to LDS. A workgroup at or past R * N/256 writes four idle records
// (checksum 0, wave = its own index, placement and clocks filled in) and
// returns as a whole: the decision depends on blockIdx alone, so no barrier is
// left waiting. row_ids are clamped to [0, tokens). With that no input makes
// the kernel read outside X, W, row_ids and offsets, or write C outside the
// valid slots.
//
// Block to tile (mg_tile_of_block). Workgroups are dealt round-robin to the 8
// XCDs. The real tiles T = R * N/256 are only known on the device, and the
// surplus workgroups must not all fall to the last XCDs, so the map is over T:
// block b = 8*i + x < T is the i-th of the contiguous range of tiles XCD x
// owns, block b >= T is idle with record index b (the map is a bijection of
// 0..bound-1 for every T). Within its range an XCD walks the tile numbering
// itself: column tile fastest, then row tile, then expert. The 32 tiles it runs
// at a time are then 32 / (N/256) consecutive row tiles, mostly of ONE expert,
// times all column tiles: they share that expert's N/256 weight slabs of a
// k-step in the XCD's L2, and each gathered A slab is read by N/256 CUs.
//
// Gathered A slab. A k-step is 128 gathered rows x 128 bytes of X and 256
// contiguous rows x 128 bytes of W[e]. Thread t owns slab rows j*32 + (t>>3),
// j = 0..3: it reads their four row ids once per tile, keeps four row
// pointers, and loads 16-byte vector t&7 of each per k-step (eight consecutive
// lanes read one row's 128 bytes, as in the GEMM sweep, only that each group of
// eight has a base of its own: vector, not scalar, addressing). B's slab is the
// GEMM sweep's uniform-base load: one 64-bit base from scalar registers plus a
// 32-bit lane offset, rows j*32 + (t>>3), j = 0..7.
// Rows at or past cnt_e load the expert's last valid row. Row i of C depends
// on row i of A alone (an MFMA never mixes A rows), so a tail row can hold
// anything finite or not: masking belongs at the C store and in the checksum,
// NOT in the K loop, which runs the same instructions for a tile of 1 row and
// of 128. Consequences: NaN in a row of X that no row id names never reaches C
// (no load ever touches it); NaN in a referenced row reaches that slot's row
// of C only.
//
// LDS. Two stages of a 128-row A slab (16 KiB) and a 256-row B slab (32 KiB):
// 2 x 48 KiB = 96 KiB, with the GEMM sweep's chunk swizzle c ^ ((r>>1) & 7),
// its rule of ONE MFMA per accumulator per trip, and its split of the next
// step's loads over the two halves of the step (A's slab ahead of the first
// sub-step's MFMAs, B's ahead of the second's). The wave's 64 x 128 sub-tile is
// 4 x 8 accumulators of v_mfma_f32_16x16x32 through ms_traits<DTYPE>: 128
// accumulator registers, half the GEMM sweep's. The tile search borrows the
// last words of stage 1's B slab, which nothing writes before the barrier that
// ends the prologue.
//
// One workgroup per CU, or two? 96 KiB is over half of a CU's 160 KiB, so one.
// Two would need at most 80 KiB each: either one stage (48 KiB), which puts a
// second barrier into every k-step and the loads' latency in front of it, or a
// k-step of 64 bytes per row, which halves the MFMAs between barriers to 32 per
// wave and gives up the 128-byte row reads and the swizzle's 256-byte bank
// span. For ragged tiles a second workgroup buys nothing that is particular to
// them: a tail tile runs the same K loop as a full one (masking is in the
// epilogue), so tiles are uniform in time and there is no short tile to hide
// behind a long one; what a second workgroup would cover is the barrier and the
// LDS latency at the head of a sub-step, which the GEMM sweep's profile names
// as its own limit too. One workgroup per CU also keeps a wave alone on its
// SIMD, so a record's clocks are that SIMD's and not a neighbour's. Decided by
// this reasoning; the two-workgroup variant has not been measured.
// Compiler's result (hipcc -O3 --offload-arch=gfx950 -Xclang -target-feature
// -Xclang -packed-fp32-ops, -Rpass-analysis=kernel-resource-usage):
//   moe_gemm_kernel<bf16>: 160 VGPRs, 128 AGPRs, 56 SGPRs, scratch 0, occupancy 1
//   moe_gemm_kernel<fp8>:  160 VGPRs, 128 AGPRs, 56 SGPRs, scratch 0, occupancy 1
// (the 128 accumulators are in AGPRs and stay there through the loop). LDS
// 98304 bytes dynamic, none static: one workgroup per CU.
//
// Epilogue. Accumulator register r of tile (i, j) is row 64*wr + 16*i + (l>>4)*4
// + r and column 128*wc + 16*j + (l&15) of the tile. The checksum is formed in
// 64-bit integer VALU from the accumulators, rows at or past the tile's valid
// count left out, C is stored under the same mask, and lane 0 writes the record
// with ms_record_simd.

#pragma once

#include "gemmsweep.h"

#define MG_TILE_M 128
#define MG_TILE_N 256
#define MG_FRAGS_M 4  // 16x16 accumulator tiles per wave: 64 rows
#define MG_FRAGS_N 8  // by 128 columns
#define MG_A_VECS (MG_TILE_M * GS_ROW_VECS)  // 16 KiB
#define MG_B_VECS (MG_TILE_N * GS_ROW_VECS)  // 32 KiB
#define MG_STAGE_VECS (MG_A_VECS + MG_B_VECS)
#define MG_LDS_BYTES (2 * MG_STAGE_VECS * 16)
#define MG_A_LOADS (MG_A_VECS / MS_BLOCK)
#define MG_B_LOADS (MG_B_VECS / MS_BLOCK)
static_assert(MG_TILE_M == NA_MOE_TILE_M && MG_TILE_N == NA_MOE_TILE_N &&
                  NA_MOE_MAX_EXPERTS <= MS_BLOCK,
              "nodeagent.h tells callers otherwise; the search takes one expert per thread");
static_assert(2 * MG_LDS_BYTES > MS_CU_LDS_BYTES, "a second workgroup would fit on the CU");

// Slot s reads this row of X.
__device__ __host__ inline uint32_t mg_row_id(mt_u64 base, mt_u64 s, uint32_t tokens) {
    return (uint32_t)(mt_mix64(base - 1 - s) % tokens);
}

// The launch and record bound in row tiles of tile_m slots: see "Tile list on
// the device".
__device__ __host__ inline uint32_t mg_row_tile_bound(uint32_t slots, uint32_t experts,
                                                      uint32_t tile_m = MG_TILE_M) {
    return slots / tile_m + experts;
}

// The tile block b computes when `tiles` are real (see "Block to tile");
// b itself, an idle record's index, for b >= tiles.
__device__ __host__ inline uint32_t mg_tile_of_block(uint32_t b, uint32_t tiles) {
    if (b >= tiles) return b;
    const uint32_t q = tiles / GS_XCDS, rem = tiles % GS_XCDS, x = b % GS_XCDS;
    return x * q + (x < rem ? x : rem) + b / GS_XCDS;  // XCD x owns q (+1 if x < rem) tiles
}

void mg_launch_fill(int dtype, unsigned grid, mt_vec* x, mt_vec* w, int* row_ids, mt_u64 x_vecs,
                    mt_u64 w_vecs, uint32_t slots, uint32_t tokens, mt_u64 base);
void mg_launch_sweep(int dtype, unsigned grid, na_mfma_record* records, const mt_vec* x,
                     const mt_vec* w, const int* row_ids, const int* offsets, float* c,
                     uint32_t tokens, uint32_t slots, uint32_t experts, uint32_t nt,
                     uint32_t ksteps, uint32_t reps, mt_u64 wbase);

#ifdef AS_KERNELS

// x, w: x_vecs and w_vecs 16-byte vectors, X's elements first in the hashed
// sequence and W's behind them (gemm_fill_kernel's layout); then one thread
// per slot for row_ids.
template <int DTYPE>
__global__ void __launch_bounds__(MS_BLOCK)
moe_fill_kernel(mt_vec* __restrict__ x, mt_vec* __restrict__ w, int* __restrict__ row_ids,
                mt_u64 x_vecs, mt_u64 w_vecs, uint32_t slots, uint32_t tokens, mt_u64 base) {
#if defined(__gfx950__)
    typedef ms_traits<DTYPE> T;
    typedef typename T::frag frag;
    constexpr int FRAGS = sizeof(mt_vec) / sizeof(frag), PER_VEC = FRAGS * T::PER_LANE;
    const mt_u64 v = (mt_u64)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= x_vecs + w_vecs) {
        const mt_u64 s = v - x_vecs - w_vecs;
        if (s < slots) row_ids[s] = (int)mg_row_id(base, s, tokens);
        return;
    }
    const bool is_w = v >= x_vecs;
    frag f[FRAGS] = {};
#pragma unroll
    for (int i = 0; i < PER_VEC; ++i)
        T::set(f[i / T::PER_LANE], i % T::PER_LANE,
               gs_element(base + v * PER_VEC + i, is_w ? GS_MOD_B : GS_MOD_A));
    mt_vec out;
    __builtin_memcpy(&out, f, sizeof(out));
    if (is_w)
        w[v - x_vecs] = out;
    else
        x[v] = out;
#endif
}

#if defined(__gfx950__)

// What a workgroup computes. idle: nothing, and `index` is its record index.
struct mg_tile {
    uint32_t index;   // tile number: records 4 * index ..
    uint32_t idle;
    uint32_t expert;
    uint32_t first;   // the slot of the tile's row 0
    uint32_t valid;   // 1..TILE_M rows of it belong to the expert
    uint32_t tj;      // column tile
};

// Inclusive scan over the workgroup's 256 threads, by wave shuffles and four
// words of LDS; `total`, when not null, receives the last thread's value.
// Called by every thread; one barrier.
template <typename OP>
__device__ inline uint32_t mg_scan(uint32_t v, uint32_t* four, uint32_t* total, OP op) {
    const uint32_t l = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)v, o);
        if (l >= o) v = op(below, v);
    }
    if (l == 63) four[wave] = v;
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) v = op(four[w], v);  // `wave` is uniform in a wave
    if (total != nullptr) {
        uint32_t all = four[0];
        for (uint32_t w = 1; w < MS_WAVES_PER_WG; ++w) all = op(all, four[w]);
        *total = all;
    }
    return v;
}

// See "Tile list on the device". words: 16 words of LDS nobody else uses until
// the next barrier after the call. Every thread of the workgroup calls it and
// gets the same answer. Three barriers. TILE_M: the slots of a row tile.
// ROWS_FASTEST: within an expert the tiles are numbered column tile, then row
// tile (moeskinnysweep.h); row tile, then column tile, otherwise.
template <int TILE_M = MG_TILE_M, bool ROWS_FASTEST = false>
__device__ inline mg_tile mg_find_tile(uint32_t* words, const int* __restrict__ offsets,
                                       uint32_t slots, uint32_t experts, uint32_t nt,
                                       uint32_t block) {
    const uint32_t e = threadIdx.x;
    uint32_t lo = 0, hi = 0;
    if (e < experts) {
        lo = (uint32_t)min(max(offsets[e], 0), (int)slots);
        hi = (uint32_t)min(max(offsets[e + 1], 0), (int)slots);
    }
    const uint32_t start =
        mg_scan(lo, words, nullptr, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
    const uint32_t cnt = (hi > start ? hi : start) - start;  // 0 for threads past `experts`
    const uint32_t mine = (cnt + TILE_M - 1) / TILE_M;
    uint32_t row_tiles;
    const uint32_t upto =
        mg_scan(mine, words + 4, &row_tiles, [](uint32_t a, uint32_t b) { return a + b; });
    mg_tile t = {};
    t.index = mg_tile_of_block(block, row_tiles * nt);
    t.idle = block >= row_tiles * nt;
    if (t.idle) return t;  // uniform: depends on the block alone
    if constexpr (ROWS_FASTEST) {
        const uint32_t before = (upto - mine) * nt;  // the tiles of the experts below e
        if (before <= t.index && t.index < upto * nt) {  // exactly one thread; mine >= 1
            const uint32_t mi = (t.index - before) % mine;
            words[8] = e;
            words[9] = start + mi * TILE_M;
            words[10] = min(cnt - mi * TILE_M, (uint32_t)TILE_M);
            words[11] = (t.index - before) / mine;
        }
    } else {
        const uint32_t rt = t.index / nt;
        t.tj = t.index % nt;
        if (upto - mine <= rt && rt < upto) {  // exactly one thread
            const uint32_t mi = rt - (upto - mine);
            words[8] = e;
            words[9] = start + mi * TILE_M;
            words[10] = min(cnt - mi * TILE_M, (uint32_t)TILE_M);
        }
    }
    __syncthreads();
    t.expert = words[8];
    t.first = words[9];
    t.valid = words[10];
    if constexpr (ROWS_FASTEST) t.tj = words[11];
    return t;
}

#endif  // __gfx950__

// records: 4 * (slots / 128 + experts) * nt entries. x: tokens rows, w: experts
// * 256 * nt rows, of ksteps * GS_ROW_VECS vectors each. c: null, or slots x
// 256 * nt floats, row-major. wbase = base + tokens*K + experts*N*K (where the
// weights p start) is hoisted to the host. Launch with (slots / 128 + experts)
// * nt workgroups of MS_BLOCK threads and MG_LDS_BYTES of dynamic shared memory.
template <int DTYPE>
__global__ void __launch_bounds__(MS_BLOCK)
moe_gemm_kernel(na_mfma_record* __restrict__ records, const mt_vec* __restrict__ x,
                const mt_vec* __restrict__ w, const int* __restrict__ row_ids,
                const int* __restrict__ offsets, float* __restrict__ c, uint32_t tokens,
                uint32_t slots, uint32_t experts, uint32_t nt, uint32_t ksteps, uint32_t reps,
                mt_u64 wbase) {
    const int wave = threadIdx.x >> 6;
#if defined(__gfx950__)
    typedef ms_traits<DTYPE> T;
    constexpr int HALVES = sizeof(mt_vec) / sizeof(typename T::frag);
    extern __shared__ mt_vec mg_lds[];
    const ms_hw_where at = ms_where();
    const int l = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1;
    const size_t pitch = (size_t)ksteps * GS_ROW_VECS;  // vectors per operand row

    const ms_clock t0 = ms_stamp();

    // stage 1's B slab: first written at the end of the first k-step
    const mg_tile tile =
        mg_find_tile(reinterpret_cast<uint32_t*>(mg_lds + 2 * MG_STAGE_VECS) - 16, offsets, slots,
                     experts, nt, blockIdx.x);
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

    // global -> LDS: this thread's vector of slab row j*32 + lrow. A: a pointer
    // per gathered row; B: a uniform base plus a 32-bit lane offset.
    const int lrow = threadIdx.x >> 3, chunk = threadIdx.x & 7;
    const mt_vec* ga[MG_A_LOADS];
#pragma unroll
    for (int j = 0; j < MG_A_LOADS; ++j) {
        const uint32_t row = min((uint32_t)(j * 32 + lrow), tile.valid - 1);  // tail: a valid row
        const uint32_t id = (uint32_t)min(max(row_ids[tile.first + row], 0), (int)tokens - 1);
        ga[j] = x + ((size_t)id * pitch + chunk);
    }
    const mt_vec* const gb = w + ((size_t)tile.expert * nt + tile.tj) * MG_TILE_N * pitch;
    const uint32_t lane_vec = (uint32_t)lrow * (uint32_t)pitch + chunk;
    const int put = lrow * GS_ROW_VECS + (chunk ^ ((lrow >> 1) & 7));
    // LDS -> fragments: chunk 4*s + (l>>4) of row (l&15) of each 16-row block
    const int get = (l & 15) * GS_ROW_VECS + ((l >> 4) ^ ((l >> 1) & 7));
    const int get_a = wr * (MG_TILE_M / 2) * GS_ROW_VECS + get;
    const int get_b = MG_A_VECS + wc * (MG_TILE_N / 2) * GS_ROW_VECS + get;

    f32x4 acc[MG_FRAGS_M][MG_FRAGS_N];
#pragma unroll
    for (int i = 0; i < MG_FRAGS_M; ++i)
#pragma unroll
        for (int j = 0; j < MG_FRAGS_N; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // One operand's slab of k-step ks into registers (A uses the first four),
    // and from there into its place in a stage.
    mt_vec staged[MG_B_LOADS];
    auto load_a = [&](uint32_t ks) {
#pragma unroll
        for (int j = 0; j < MG_A_LOADS; ++j) staged[j] = ga[j][(size_t)ks * GS_ROW_VECS];
    };
    auto load_b = [&](uint32_t ks) {
#pragma unroll
        for (int j = 0; j < MG_B_LOADS; ++j)
            staged[j] = (gb + ((size_t)j * 32 * pitch + (size_t)ks * GS_ROW_VECS))[lane_vec];
    };
    auto store_a = [&](int stage) {
        mt_vec* const s = mg_lds + stage * MG_STAGE_VECS + put;
#pragma unroll
        for (int j = 0; j < MG_A_LOADS; ++j) s[j * 32 * GS_ROW_VECS] = staged[j];
    };
    auto store_b = [&](int stage) {
        mt_vec* const s = mg_lds + stage * MG_STAGE_VECS + MG_A_VECS + put;
#pragma unroll
        for (int j = 0; j < MG_B_LOADS; ++j) s[j * 32 * GS_ROW_VECS] = staged[j];
    };

    load_a(0);
    store_a(0);
    load_b(0);
    store_b(0);
    __syncthreads();

    // The K loop, `reps` times into the same accumulators: the GEMM sweep's,
    // with 4 x 8 accumulators. One trip is one sub-step (an E4M3 sub-step: one
    // of its two halves) and ONE MFMA per accumulator; the first sub-step has
    // the next step's gathered slab of A in flight and writes it to the other
    // stage, the second does the same for B. The loads of the step after the
    // last wrap to k-step 0 (in bounds) and land in a stage nobody reads. Every
    // tile, full or tail, runs exactly this.
    constexpr uint32_t PHASES = 2 * HALVES;
    const uint32_t trips = reps * ksteps * PHASES;
    uint32_t ks = ksteps == 1 ? 0 : 1, phase = 0, stage = 0;  // ks: the step being loaded
    mt_vec fa[MG_FRAGS_M], fb[MG_FRAGS_N];
    for (uint32_t it = 0; it < trips; ++it) {
        const uint32_t sub = phase / HALVES, h = phase % HALVES;
        if (h == 0) {
            if (sub == 0)
                load_a(ks);
            else
                load_b(ks);
            const mt_vec* const s = mg_lds + stage * MG_STAGE_VECS;
#pragma unroll
            for (int i = 0; i < MG_FRAGS_M; ++i) fa[i] = s[(get_a ^ (sub * 4)) + i * 16 * GS_ROW_VECS];
#pragma unroll
            for (int j = 0; j < MG_FRAGS_N; ++j) fb[j] = s[(get_b ^ (sub * 4)) + j * 16 * GS_ROW_VECS];
        }
#pragma unroll
        for (int i = 0; i < MG_FRAGS_M; ++i)
#pragma unroll
            for (int j = 0; j < MG_FRAGS_N; ++j)
                acc[i][j] = T::mfma(gs_frag<T>(fa[i], h), gs_frag<T>(fb[j], h), acc[i][j]);
        if (h == HALVES - 1) {
            if (sub == 0)
                store_a(stage ^ 1);
            else
                store_b(stage ^ 1);
        }
        if (++phase == PHASES) {  // uniform: the same trip for all four waves
            __syncthreads();
            phase = 0;
            stage ^= 1;
            ks = ks + 1 == ksteps ? 0 : ks + 1;
        }
    }

    const ms_clock t1 = ms_stamp();

    // checksum = sum over valid rows s of p_s * (sum_j q_j * C[s][j]) over this
    // lane's elements; C under the same mask
    const uint32_t row0 = wr * (MG_TILE_M / 2) + (l >> 4) * 4;  // within the tile
    const uint32_t col0 = tile.tj * MG_TILE_N + wc * (MG_TILE_N / 2) + (l & 15);
    const uint32_t n_cols = nt * MG_TILE_N;
    mt_u64 q[MG_FRAGS_N];
#pragma unroll
    for (int j = 0; j < MG_FRAGS_N; ++j) q[j] = gs_weight(wbase + slots + col0 + j * 16);
    float* const c0 =
        c == nullptr ? nullptr : c + ((size_t)(tile.first + row0) * n_cols + col0);
    mt_u64 sum = 0;
#pragma unroll
    for (int i = 0; i < MG_FRAGS_M; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t row = row0 + i * 16 + r;
            if (row >= tile.valid) continue;  // the next expert's slot, or nobody's
            mt_u64 inner = 0;
#pragma unroll
            for (int j = 0; j < MG_FRAGS_N; ++j)
                inner += q[j] * (mt_u64)(long long)(int)acc[i][j][r];
            sum += gs_weight(wbase + tile.first + row) * inner;
            if (c0 != nullptr) {
                float* const out = c0 + (size_t)(i * 16 + r) * n_cols;
#pragma unroll
                for (int j = 0; j < MG_FRAGS_N; ++j) out[j * 16] = acc[i][j][r];
            }
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
