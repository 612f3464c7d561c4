// MI355X node agent: the C ABI of libmi355x_nodeagent.so, declared once.
//
// Plain C: <stdint.h> and nothing of HIP, so that a host program over the
// verify paths, the device headers and agent.hip all read the same text.
// agent.hip defines every function below and the compiler checks each
// definition against its prototype. gpu_provisioner_amd/nodeagent.py binds
// them by the table _ABI and mirrors the structs as ctypes.Structure classes;
// tests/test_nodeagent_abi.py compiles this header with the host compiler and
// holds the two declarations against each other.

#ifndef MI355X_NODEAGENT_H
#define MI355X_NODEAGENT_H

#include <stdint.h>

#ifdef __cplusplus
#define NA_ABI_SIZE(type, bytes) static_assert(sizeof(type) == (bytes), #type " changed size")
#else
#define NA_ABI_SIZE(type, bytes) _Static_assert(sizeof(type) == (bytes), #type " changed size")
#endif

// Return codes. After any other than NA_OK, na_last_error says what happened.
#define NA_OK 0
#define NA_ERR_HIP -1
#define NA_ERR_VERIFY -2
#define NA_ERR_ARG -3

// Limits a caller sizes its buffers by. The device headers derive the values
// their kernels use themselves and assert that they are these.
#define NA_SWEEP_MAX_LISTED 8    // bad units a sweep result lists
#define NA_SWEEP_WAVES_PER_WG 4  // records per workgroup of the per-wave sweeps
#define NA_LDS_PHASES 8          // checksums of an LDS record (LS_* of ldssweep.h)
#define NA_LDS_GRANULE 4096      // an explicit lds_bytes is a multiple of this,
#define NA_LDS_MAX_BYTES (160 * 1024)  // up to the LDS of one CU
#define NA_CACHE_PHASES 7        // checksums the cache sweep uses of an LDS record (CS_* of cachesweep.h)
#define NA_CACHE_GRANULE 4096    // slice_bytes is a multiple of this,
#define NA_CACHE_MAX_BYTES (1 << 20)  // up to 1 MiB
#define NA_CACHE_TABLE_WORDS 4096     // the scalar phase's read-only table
#define NA_VALU_PHASES 9         // checksums of a VALU record (VS_* of valusweep.h)
#define NA_VALU_MAX_ITERS (((1 << 24) - 2048) / 2 - 1)  // the stream phase is exact up to here
#define NA_LOAD_GRANULE 16384    // the load sweep's slice_bytes is a multiple of this,
#define NA_LOAD_MAX_BYTES (16 << 20)  // up to 16 MiB
#define NA_GEMM_TILE 256         // the GEMM sweep's M and N are multiples of this,
#define NA_GEMM_MAX_DIM 65536    // up to this;
#define NA_GEMM_BK_BF16 64       // its K is a multiple of this for bf16,
#define NA_GEMM_BK_FP8 128       // of this for fp8 (128 bytes per row either way),
#define NA_GEMM_EXACT (1 << 24)  // and 6 * reps * K stays under this: exact f32 integers
#define NA_MXGEMM_BK_FP8 128     // the MX GEMM sweep's K is a multiple of this for fp8,
#define NA_MXGEMM_BK_FP4 256     // of this for fp4 (128 bytes per row either way),
#define NA_MXGEMM_EXACT (1 << 24)  // and 24 * reps * K stays under this: exact f32 integers
#define NA_MXQUANT_BLOCK 32      // the MX quantiser's K is a multiple of this: elements per scale,
#define NA_MXQUANT_MAX_BLOCKS (1 << 24)  // rows * K / 32 is at most this (1 GiB of bf16),
#define NA_MXQUANT_MAX_PASSES (1 << 20)  // and a launch repeats its slice at most this often
#define NA_ATTN_HEAD_DIM 128     // the attention sweep's head dimension;
#define NA_ATTN_Q_BLOCK 128      // its n_q is a multiple of this,
#define NA_ATTN_K_TILE 64        // its n_k of this,
#define NA_ATTN_MAX_HEADS 4096   // with at most this many heads
#define NA_ATTN_MAX_Q (1 << 20)  // of at most this many queries,
#define NA_ATTN_EXACT (1 << 24)  // and 256 * reps * n_k stays under this: exact f32 sums
#define NA_DECODE_HEAD_DIM 128   // the decode attention sweep's head dimension;
#define NA_DECODE_PAGE 16        // tokens in a page of its KV cache;
#define NA_DECODE_MAX_GROUP 16   // heads / kv_heads is at most this,
#define NA_DECODE_MAX_BATCH 4096     // with at most this many sequences
#define NA_DECODE_MAX_HEADS 1024     // of at most this many heads
#define NA_DECODE_MAX_PAGES (1 << 16)  // and pages in a row of the block table,
#define NA_DECODE_MAX_SPLITS 64  // at most this many workgroups share a (sequence, KV head),
#define NA_DECODE_EXACT (1 << 24)  // and 256 * reps * the longest length stays under this
#define NA_MOE_TILE_M 128        // slots in a tile of the MoE grouped GEMM sweep: a tile has one expert;
#define NA_MOE_TILE_N 256        // its N is a multiple of this (K and reps as the GEMM sweep's),
#define NA_MOE_MAX_EXPERTS 256   // with at most this many experts
#define NA_MOE_MAX_ROWS (1 << 22)  // and tokens and slots
#define NA_MOE_SKINNY_TILE_M 16  // slots in a tile of the decode-size MoE expert GEMM sweep
#define NA_MOE_MAX_TOPK 8        // choices of a token in the MoE routing sweep,
#define NA_MOE_ROUTE_BLOCK 256   // tokens of a workgroup of its route and sort (4 records),
#define NA_MOE_COMBINE_WAVE_TOKENS 8  // and of a wave of its combine (1 record)

// ---------------------------------------------------------------------------
// Records: what the sweep kernels write, one per wave or workgroup
// ---------------------------------------------------------------------------

// Matrix-core sweep (mfmasweep.h). One per wave, written by one lane.
// cycles/realtime are the deltas of s_memtime (shader clock) and
// s_memrealtime (100 MHz) around the fold loop. The load sweep (loadsweep.h)
// leaves the same record for each of its matrix waves and, with the clocks
// around the stream loop, for each of its stream waves; a wave of a role that
// is switched off leaves it all zero. The GEMM sweep (gemmsweep.h) leaves it
// for each wave of each C tile, `wave` being 4 * tile + 2 * wr + wc and the
// clocks around the K loops, and the MX GEMM sweep (mxgemmsweep.h) the same.
// The MX quantise sweep (mxquantsweep.h) leaves it for each wave of each
// workgroup, `wave` being 4 * workgroup + wave and the clocks around the passes.
// The attention sweep (attnsweep.h) leaves it for each wave of each block of
// 128 queries of each head, `wave` being 4 * (head * n_q / 128 + block) + wave
// and the clocks around the walk over the keys. The decode attention sweep
// (decodesweep.h) leaves it for each wave of each split of each (sequence, KV
// head), `wave` being 4 * ((b * kv_heads + hk) * splits + split) + wave, and
// after those one per (sequence, KV head) over the merged state, `wave` being 4
// * batch * kv_heads * splits + b * kv_heads + hk. The MoE grouped GEMM sweep
// (moegemmsweep.h) leaves it for each wave of each tile, `wave` being 4 * tile
// + 2 * wr + wc, and with checksum 0 for each wave of the workgroups beyond the
// last tile; the decode-size MoE expert GEMM sweep (moeskinnysweep.h) the same,
// `wave` being 4 * tile + wave. The MoE routing sweep (moeroutesweep.h) leaves it for each wave of
// its route, scatter and combine kernels, numbered one kernel behind the other
// as its prototypes below say.
typedef struct {
    uint64_t checksum, cycles, realtime;
    uint32_t wave, xcc, se, sh, cu, simd;
} na_mfma_record;
NA_ABI_SIZE(na_mfma_record, 48);

// LDS sweep (ldssweep.h) and cache sweep (cachesweep.h). One per workgroup
// and launch, written by one thread. The LDS sweep fills all NA_LDS_PHASES
// checksums; the cache sweep uses the first NA_CACHE_PHASES and leaves 0 in
// those its launch does not compute. cycles/realtime are the deltas of
// s_memtime (shader clock) and s_memrealtime (100 MHz) around the stream
// phase (the cache sweep's second launch: around its xread phase). bad_phase
// is an LS_* or CS_* code, 0xFFFFFFFF when bad_words is 0, and
// first_bad_offset is then UINT64_MAX; otherwise it is the LDS byte offset
// for the LDS sweep, the byte offset within the slice for the cache sweep.
typedef struct {
    uint64_t checksum[NA_LDS_PHASES];
    uint64_t bad_words, first_bad_offset, xor_mask;
    uint64_t cycles, realtime;
    uint32_t workgroup, bad_phase, xcc, se, sh, cu;
} na_lds_record;
NA_ABI_SIZE(na_lds_record, 128);

// Vector-unit sweep (valusweep.h). One per wave, written by one lane.
// cycles/realtime are the deltas of s_memtime (shader clock) and
// s_memrealtime (100 MHz) around the stream phase. The rf_* fields are the
// kernel's own comparison in the two register-file phases: rf_bad counts wrong
// (slot, lane) pairs of both, rf_first_slot is the slot of the first (rf
// before rf_inv, then lowest slot, then lowest lane) plus 512 when it was seen
// in rf_inv, rf_first_lane its lane, rf_xor the OR of got ^ want. With rf_bad
// 0 the slot and lane are 0xFFFFFFFF.
typedef struct {
    uint64_t checksum[NA_VALU_PHASES];
    uint64_t cycles, realtime;
    uint32_t wave, xcc, se, sh, cu, simd;
    uint32_t rf_bad, rf_first_slot, rf_first_lane, rf_xor;
} na_valu_record;
NA_ABI_SIZE(na_valu_record, 128);

// ---------------------------------------------------------------------------
// Results: what the verifies fill
// ---------------------------------------------------------------------------

typedef struct {
    uint64_t bytes_tested, bad_words, first_bad_offset /* UINT64_MAX = none */, xor_mask;
} na_memtest_result;
NA_ABI_SIZE(na_memtest_result, 32);

typedef struct {
    uint64_t waves, bad_waves;
    uint64_t units_seen, bad_units;  // distinct (xcc, se, sh, cu)
    uint64_t first_bad_wave;         // UINT64_MAX = none
    double clock_mhz;                // median of cycles / realtime x 100 MHz
    uint32_t first_bad_unit[5];      // xcc, se, sh, cu, simd
    uint32_t listed;                 // entries used in bad_list
    uint32_t bad_list[NA_SWEEP_MAX_LISTED][5];  // first distinct failing (xcc, se, sh, cu, simd)
} na_mfma_sweep_result;
NA_ABI_SIZE(na_mfma_sweep_result, 232);

// Of the LDS sweep and of the cache sweep.
typedef struct {
    uint64_t workgroups, bad_workgroups;
    uint64_t units_seen, bad_units;   // distinct (xcc, se, sh, cu)
    uint64_t first_bad_workgroup;     // UINT64_MAX = none
    // of the first bad workgroup, when its first failing phase compares words
    // in the kernel; otherwise 0, UINT64_MAX, 0
    uint64_t bad_words, first_bad_offset, xor_mask;
    double clock_mhz;                 // median of cycles / realtime x 100 MHz
    // stream phase, iters * lds_bytes / cycles per workgroup (slice_bytes for
    // the cache sweep): bytes per shader clock of the CU it ran on
    double median_bytes_per_clk, min_bytes_per_clk, max_bytes_per_clk;
    uint32_t first_bad_unit[4];       // xcc, se, sh, cu
    // LS_* code, NA_LDS_PHASES = the record's index; for the cache sweep a
    // CS_* code, NA_CACHE_PHASES = the record's index
    uint32_t first_bad_phase;
    uint32_t listed;                  // entries used in bad_list
    uint32_t bad_list[NA_SWEEP_MAX_LISTED][4];  // first distinct failing (xcc, se, sh, cu)
} na_lds_sweep_result;
NA_ABI_SIZE(na_lds_sweep_result, 248);

typedef struct {
    uint64_t waves, bad_waves;
    uint64_t cus_seen, simds_seen;  // distinct (xcc, se, sh, cu) and (.., simd)
    uint64_t trans_unchecked;       // 1: fewer than 3 records or no strict majority
    uint64_t trans_consensus;       // the majority's trans checksum; 0 when unchecked
    uint64_t median_cycles;         // of the stream phase
    double clock_mhz;               // median of cycles / realtime x 100 MHz
    // stream phase, FLOP per shader clock of the SIMD the wave ran on
    double median_flop_per_clk, min_flop_per_clk;
    double tflops;  // median_flop_per_clk x simds_seen x clock_mhz / 1e6
    // the first listed wave's in-kernel register-file diagnosis
    uint32_t rf_bad, rf_first_slot, rf_first_lane, rf_xor;
    uint32_t listed;  // entries used in bad_list
    // first bad waves: wave, xcc, se, sh, cu, simd, mask of failed phases
    uint32_t bad_list[NA_SWEEP_MAX_LISTED][7];
} na_valu_sweep_result;
NA_ABI_SIZE(na_valu_sweep_result, 336);

#undef NA_ABI_SIZE

// ---------------------------------------------------------------------------
// Entry points, in the order of agent.hip, where each is described
// ---------------------------------------------------------------------------

#ifdef __cplusplus
extern "C" {
#endif

const char* na_last_error(void);

// devices, bandwidth probe and one launch of its copy kernel, VALU self-test
int na_device_count(int* count);
int na_device_info(int dev, char* name, int name_len, char* arch, int arch_len,
                   long long* hbm_bytes, int* cus, int* max_clock_khz);
int na_hbm_bandwidth(int dev, long long bytes, int iters, double* gbs);
int na_copy_run(int dev, const void* src, void* dst, long long bytes, int workgroups, int threads);
int na_fma_selftest(int dev);

// single-wave MFMA checks (kinds: NA_MFMA_* of mfma_frag.h)
int na_mfma_check_run(int dev, int kind, void* out, int n_words);
int na_mfma_check_verify(int kind, const void* words, int n_words);
int na_mfma_selftest(int dev);
int na_mfma_bf16_selftest(int dev);
int na_mfma_fp8_selftest(int dev);
int na_mfma_bf16_tile_check(int dev);
int na_mfma_f16_tile_check(int dev);
int na_mfma_fp8_tile_check(int dev);
int na_mfma_i8_tile_check(int dev);
int na_mfma_bf16_tile32_check(int dev);
int na_mfma_mx_tile_check(int dev);

// single-wave MX checks (formats: MX_* of mx_formats.h, kinds: NA_MX_* of mfma_frag.h)
int na_mx_decode(int fmt, int code, float* value);
int na_mx_pack(int fmt, const int* codes, int n, uint32_t* words, int n_words);
int na_mx_check_run(int dev, int kind, void* out, int n_words);
int na_mx_check_verify(int kind, const void* words, int n_words);
int na_mx_checks(int dev);

// LDS self-test, SDMA and peer-to-peer probes
int na_lds_selftest(int dev, long long* bytes_tested);
int na_sdma_bandwidth(int dev, long long bytes, int iters, double* gbs);
int na_p2p_matrix(int n, int* out /* n*n */);
int na_p2p_bandwidth(int src, int dst, long long bytes, int iters, double* gbs);

// HBM data-integrity test
int na_mem_info(int dev, long long* free_bytes, long long* total_bytes);
int na_memtest_fill(int dev, void* dptr, long long bytes, unsigned long long seed, int invert);
int na_memtest_verify(int dev, void* dptr, long long bytes, unsigned long long seed, int invert,
                      int flip, na_memtest_result* out);
int na_hbm_memtest_passes(int dev, long long bytes, int rounds, unsigned long long seed,
                          na_memtest_result* out, double* gbs, double* pass_gbs);
int na_hbm_memtest(int dev, long long bytes, int rounds, unsigned long long seed,
                   na_memtest_result* out, double* gbs);

// chip-wide matrix-core sweep: dtype 0 = bf16, 1 = fp8
int na_mfma_sweep_expected(unsigned long long seed, unsigned long long wave, int outer,
                           uint64_t* checksum);
int na_mfma_sweep_run(int dev, int dtype, int workgroups, int outer, unsigned long long seed,
                      na_mfma_record* out, long long n_out, double* ms);
int na_mfma_sweep_verify(const na_mfma_record* recs, long long n, int outer,
                         unsigned long long seed, na_mfma_sweep_result* res);
int na_mfma_sweep(int dev, int dtype, int workgroups, int outer, unsigned long long seed,
                  na_mfma_sweep_result* res, double* tflops);

// chip-wide MX sweep: format 0 = fp4, 1 = fp6
int na_mx_sweep_expected(unsigned long long seed, unsigned long long wave, int outer,
                         uint64_t* checksum);
int na_mx_sweep_run(int dev, int format, int workgroups, int outer, unsigned long long seed,
                    na_mfma_record* out, long long n_out, double* ms);
int na_mx_sweep_verify(const na_mfma_record* recs, long long n, int outer,
                       unsigned long long seed, na_mfma_sweep_result* res);
int na_mx_sweep(int dev, int format, int workgroups, int outer, unsigned long long seed,
                na_mfma_sweep_result* res, double* tflops);

// chip-wide LDS sweep
int na_lds_sweep_allocation(int dev, long long* bytes);
int na_lds_sweep_expected(unsigned long long seed, unsigned long long workgroup,
                          long long lds_bytes, int iters, uint64_t* checksums, int n);
int na_lds_sweep_run(int dev, int workgroups, long long lds_bytes, int iters,
                     unsigned long long seed, na_lds_record* out, long long n_out, double* ms);
int na_lds_sweep_verify(const na_lds_record* recs, long long n, long long lds_bytes, int iters,
                        unsigned long long seed, na_lds_sweep_result* res);
int na_lds_sweep(int dev, int workgroups, long long lds_bytes, int iters,
                 unsigned long long seed, na_lds_sweep_result* res, double* gbs);

// chip-wide cache sweep: records 0..workgroups-1 are the first launch's,
// workgroups..2*workgroups-1 the second's
int na_cache_sweep_expected(unsigned long long seed, unsigned long long workgroup,
                            unsigned long long workgroups, long long slice_bytes, int iters,
                            uint64_t* checksums, int n);
int na_cache_sweep_run(int dev, int workgroups, long long slice_bytes, int iters,
                       unsigned long long seed, na_lds_record* out, long long n_out, double* ms);
int na_cache_sweep_verify(const na_lds_record* recs, long long n, long long slice_bytes, int iters,
                          unsigned long long seed, na_lds_sweep_result* res);
int na_cache_sweep(int dev, int workgroups, long long slice_bytes, int iters,
                   unsigned long long seed, na_lds_sweep_result* res, double* gbs);

// chip-wide vector-unit sweep
int na_valu_sweep_xlane_table(int move, int* out, int n);
int na_valu_sweep_slots(void);
int na_valu_sweep_expected(unsigned long long seed, unsigned long long wave, int iters,
                           uint64_t* checksums);
int na_valu_sweep_run(int dev, int workgroups, int iters, unsigned long long seed,
                      na_valu_record* out, long long n_out, double* ms);
int na_valu_sweep_verify(const na_valu_record* recs, long long n, int iters,
                         unsigned long long seed, na_valu_sweep_result* res);
int na_valu_sweep(int dev, int workgroups, int iters, unsigned long long seed,
                  na_valu_sweep_result* res);

// chip-wide load sweep (matrix cores, LDS and HBM at once): dtype 0 = bf16,
// 1 = fp8; outer 0 switches the matrix waves off, passes 0 the stream waves;
// records and results are the matrix-core sweep's, one set per role
int na_load_sweep_stream_expected(unsigned long long seed, unsigned long long workgroup,
                                  long long slice_bytes, int passes, uint64_t* checksums, int n);
int na_load_sweep_run(int dev, int dtype, int workgroups, int outer, void* region,
                      long long slice_bytes, int passes, unsigned long long seed,
                      na_mfma_record* matrix, na_mfma_record* stream, long long n_out,
                      na_memtest_result* mem, double* ms);
int na_load_sweep_verify(const na_mfma_record* matrix, const na_mfma_record* stream, long long n,
                         int outer, long long slice_bytes, int passes, unsigned long long seed,
                         na_mfma_sweep_result* matrix_res, na_mfma_sweep_result* stream_res);
int na_load_sweep(int dev, int dtype, int workgroups, int outer, long long slice_bytes,
                  int passes, unsigned long long seed, na_mfma_sweep_result* matrix_res,
                  na_mfma_sweep_result* stream_res, na_memtest_result* mem,
                  double* tflops, double* gbs, double* overlap);

// chip-wide GEMM sweep, C = reps * A * B^T through HBM, L2 and LDS: dtype 0 =
// bf16, 1 = fp8; a is m x k, b n_cols x k, both K-contiguous in that dtype, c
// null or m x n_cols floats; records and results are the matrix-core sweep's,
// record 4 * tile + 2 * wr + wc for the wave of the 128 x 128 sub-tile (wr, wc)
// of tile ti * (n_cols / 256) + tj
int na_gemm_sweep_fill(int dev, int dtype, void* a, void* b, long long m, long long n_cols,
                       long long k, unsigned long long seed);
int na_gemm_sweep_expected(unsigned long long seed, long long m, long long n_cols, long long k,
                           int reps, uint64_t* checksums, long long n_out);
int na_gemm_sweep_run(int dev, int dtype, const void* a, const void* b, void* c, long long m,
                      long long n_cols, long long k, int reps, unsigned long long seed,
                      na_mfma_record* out, long long n_out, double* ms);
int na_gemm_sweep_verify(const na_mfma_record* recs, long long n, long long m, long long n_cols,
                         long long k, int reps, unsigned long long seed,
                         na_mfma_sweep_result* res);
int na_gemm_sweep(int dev, int dtype, long long m, long long n_cols, long long k, int reps,
                  unsigned long long seed, na_mfma_sweep_result* res, double* tflops);

// chip-wide block-scaled MX GEMM sweep, C = reps * (2^ea a) * (2^eb b)^T on
// v_mfma_scale_f32_16x16x128_f8f6f4: format 0 = fp8 (MX_E4M3, a byte per
// element), 4 = fp4 (MX_E2M1, two per byte, even k in the low nibble); a is m x
// k, b n_cols x k, K-contiguous, sa and sb their E8M0 scales, uint8[rows][k/32];
// shapes, records and results as the GEMM sweep's
int na_mxgemm_sweep_fill(int dev, int format, void* a, void* b, void* sa, void* sb, long long m,
                         long long n_cols, long long k, unsigned long long seed);
int na_mxgemm_sweep_expected(unsigned long long seed, long long m, long long n_cols, long long k,
                             int reps, uint64_t* checksums, long long n_out);
int na_mxgemm_sweep_run(int dev, int format, const void* a, const void* b, const void* sa,
                        const void* sb, void* c, long long m, long long n_cols, long long k,
                        int reps, unsigned long long seed, na_mfma_record* out, long long n_out,
                        double* ms);
int na_mxgemm_sweep_verify(const na_mfma_record* recs, long long n, long long m, long long n_cols,
                           long long k, int reps, unsigned long long seed,
                           na_mfma_sweep_result* res);
int na_mxgemm_sweep(int dev, int format, long long m, long long n_cols, long long k, int reps,
                    unsigned long long seed, na_mfma_sweep_result* res, double* tflops);

// chip-wide MX quantise sweep, and the OCP MX quantiser it runs as an operation
// on caller-owned tensors: format 0 = fp8 (MX_E4M3), 2 = fp6 (MX_E2M3), 4 = fp4
// (MX_E2M1); src is rows x k bf16, K-contiguous, k a multiple of 32; dst the
// packed elements (fp8 a byte each, fp4 two per byte with the even k in the low
// nibble, fp6 element i of a block at bit 6 i of its 24 bytes), scales
// uint8[rows][k/32] of E8M0 bytes; rules, layout and checksum in mxquantsweep.h;
// records and results are the matrix-core sweep's, record 4 * workgroup + wave
int na_mxquant_reference(int format, const void* src, long long rows, long long k, void* dst,
                         void* scales);
int na_mxquant_fill(int dev, void* src, long long rows, long long k, unsigned long long seed);
int na_mxquant_expected(int format, unsigned long long seed, long long rows, long long k,
                        int workgroups, int passes, uint64_t* checksums, long long n_out);
int na_mxquant_run(int dev, int format, const void* src, void* dst, void* scales, long long rows,
                   long long k, int workgroups, int passes, unsigned long long seed,
                   na_mfma_record* records, long long n_out, double* ms);
int na_mxquant_verify(const na_mfma_record* recs, long long n, int format, long long rows,
                      long long k, int workgroups, int passes, unsigned long long seed,
                      na_mfma_sweep_result* res);
int na_mxquant_sweep(int dev, int format, int workgroups, int passes, unsigned long long seed,
                     na_mfma_sweep_result* res, double* gelems);

// chip-wide fused attention sweep, and the attention it runs as an operation on
// caller-owned tensors: o = softmax(scale q k^T [+ causal mask]) v in base 2,
// p = exp2(scale_log2 * (s - max s)); q is bf16[heads][n_q][128], k and v
// bf16[kv_heads][n_k][128], row-major, o null or float[heads][n_q][128]; n_q a
// multiple of 128, n_k of 64, heads of kv_heads (query head h reads KV head h /
// (heads / kv_heads)); causal 1 shows key j to query i iff j <= i + n_k - n_q and
// needs n_k >= n_q; reps walks the keys that often into one softmax state;
// operands, layout and checksum in attnsweep.h; records and results are the
// matrix-core sweep's, record 4 * (head * n_q / 128 + block) + wave
int na_attn_sweep_fill(int dev, void* q, void* k, void* v, int heads, int kv_heads, long long n_q,
                       long long n_k, unsigned long long seed);
int na_attn_sweep_expected(unsigned long long seed, int heads, int kv_heads, long long n_q,
                           long long n_k, int causal, int reps, uint64_t* checksums,
                           long long n_out);
int na_attn_run(int dev, const void* q, const void* k, const void* v, void* o, int heads,
                int kv_heads, long long n_q, long long n_k, int causal, float scale_log2, int reps,
                unsigned long long seed, na_mfma_record* records, long long n_out, double* ms);
int na_attn_sweep_verify(const na_mfma_record* recs, long long n, int heads, int kv_heads,
                         long long n_q, long long n_k, int causal, int reps,
                         unsigned long long seed, na_mfma_sweep_result* res);
int na_attn_sweep(int dev, int heads, int kv_heads, long long n_q, long long n_k, int causal,
                  int reps, unsigned long long seed, na_mfma_sweep_result* res, double* tflops);

// chip-wide paged decode attention sweep, and the decode attention it runs as
// an operation on caller-owned tensors: one query token per sequence against a
// KV cache in pages of 16 tokens. q is bf16[batch][heads][128], k_cache and
// v_cache bf16[num_pages][kv_heads][16][128], block_table int32[batch][max_pages]
// and seq_lens int32[batch] in device memory (each length 1 .. 16 * max_pages), o
// null or float[batch][heads][128]; heads a multiple of kv_heads with heads /
// kv_heads <= 16; splits workgroups share one (sequence, KV head); reps and
// scale_log2 as na_attn_run's; `lens` is the host's copy of the lengths;
// operands, paging and checksums in decodesweep.h; batch * kv_heads * (4 * splits
// + 1) records, results are the matrix-core sweep's. na_decode_splits gives the
// splits that na_decode_sweep takes for splits = 0.
int na_decode_splits(int dev, int batch, int kv_heads, int max_pages, int* splits);
int na_decode_sweep_fill(int dev, void* q, void* k_cache, void* v_cache, void* block_table,
                         void* seq_lens, int batch, int heads, int kv_heads, int max_pages,
                         const int* lens, unsigned long long seed);
int na_decode_sweep_expected(unsigned long long seed, int batch, int heads, int kv_heads,
                             int max_pages, const int* lens, int splits, int reps,
                             uint64_t* checksums, long long n_out);
int na_decode_run(int dev, const void* q, const void* k_cache, const void* v_cache,
                  const void* block_table, const void* seq_lens, void* o, int batch, int heads,
                  int kv_heads, int max_pages, long long num_pages, int splits, float scale_log2,
                  int reps, unsigned long long seed, na_mfma_record* records, long long n_out,
                  double* ms);
int na_decode_sweep_verify(const na_mfma_record* recs, long long n, int batch, int heads,
                           int kv_heads, int max_pages, const int* lens, int splits, int reps,
                           unsigned long long seed, na_mfma_sweep_result* res);
int na_decode_sweep(int dev, int batch, int heads, int kv_heads, int max_pages, int splits,
                    int reps, unsigned long long seed, na_mfma_sweep_result* res, double* gbps);

// chip-wide MoE grouped GEMM sweep, and the expert GEMM it runs as an operation
// on caller-owned tensors: C[s] = reps * X[row_ids[s]] * W[e]^T for the slots s
// of expert e, offsets[e] <= s < offsets[e+1]. dtype 0 = bf16, 1 = fp8; x is
// tokens x k and w experts x n_cols x k, K-contiguous in that dtype, row_ids
// int32[slots] and offsets int32[experts + 1] in device memory, c null or slots
// x n_cols floats (rows from offsets[experts] on are never written); n_cols a
// multiple of 256, k and reps as the GEMM sweep's; `counts` is the host's copy
// of the slots per expert, their sum at most `slots`. Tiles of 128 slots x 256
// columns are found on the device, so a launch has na_moe_gemm_tiles' `bound`
// workgroups, (slots / 128 + experts) * n_cols / 256, and leaves 4 * bound
// records: 4 * tile + 2 * wr + wc for the wave of the 64 x 128 sub-tile (wr,
// wc) of a tile, tiles numbered by expert, row tile, column tile, and idle
// records behind them. Operands and checksums in moegemmsweep.h; results are
// the matrix-core sweep's. 0 = the default for na_moe_gemm_sweep's shape and
// reps, its counts are hashed from the seed.
int na_moe_gemm_tiles(long long slots, int experts, long long n_cols, long long* bound);
int na_moe_gemm_fill(int dev, int dtype, void* x, void* w, void* row_ids, void* offsets,
                     long long tokens, long long slots, int experts, long long n_cols, long long k,
                     const int* counts, unsigned long long seed);
int na_moe_gemm_expected(unsigned long long seed, long long tokens, long long slots, int experts,
                         long long n_cols, long long k, const int* counts, int reps,
                         uint64_t* checksums, long long n_out);
int na_moe_gemm_run(int dev, int dtype, const void* x, const void* w, const void* row_ids,
                    const void* offsets, void* c, long long tokens, long long slots, int experts,
                    long long n_cols, long long k, int reps, unsigned long long seed,
                    na_mfma_record* out, long long n_out, double* ms);
int na_moe_gemm_verify(const na_mfma_record* recs, long long n, long long tokens, long long slots,
                       int experts, long long n_cols, long long k, const int* counts, int reps,
                       unsigned long long seed, na_mfma_sweep_result* res);
int na_moe_gemm_sweep(int dev, int dtype, long long tokens, long long slots, int experts,
                      long long n_cols, long long k, int reps, unsigned long long seed,
                      na_mfma_sweep_result* res, double* tflops);

// chip-wide decode-size MoE expert GEMM sweep, and the skinny expert GEMM it
// runs as an operation: the problem, the tensors, the dtypes and the limits of
// na_moe_gemm_* above (na_moe_gemm_fill fills for both; c here 16-byte aligned),
// for 1-16 slots per expert, where the expert weights stream from HBM straight
// into the matrix cores. Tiles of 16 slots x 256 columns are found on the
// device: na_moe_skinny_tiles' `bound` is (slots / 16 + experts) * n_cols / 256
// workgroups, and a launch leaves 4 * bound records: 4 * tile + w for wave w,
// which owns columns 64 w .. 64 w + 63 of the tile, tiles numbered by expert,
// column tile, row tile (row tile fastest), and idle records behind them.
// Specification in moeskinnysweep.h. 0 = the default for na_moe_skinny_sweep's
// shape (a decode step: 160 tokens top-8 on 128 experts of n_cols 2048, k 2048,
// counts of 0-16 and a few of 17-40 hashed from the seed) and reps (1); *gbps
// counts the bytes of W of the experts that have a slot, the gathered rows of X
// and the rows of C written, per second, over several launches in one window.
int na_moe_skinny_tiles(long long slots, int experts, long long n_cols, long long* bound);
int na_moe_skinny_expected(unsigned long long seed, long long tokens, long long slots, int experts,
                           long long n_cols, long long k, const int* counts, int reps,
                           uint64_t* checksums, long long n_out);
int na_moe_skinny_run(int dev, int dtype, const void* x, const void* w, const void* row_ids,
                      const void* offsets, void* c, long long tokens, long long slots, int experts,
                      long long n_cols, long long k, int reps, unsigned long long seed,
                      na_mfma_record* out, long long n_out, double* ms);
int na_moe_skinny_verify(const na_mfma_record* recs, long long n, long long tokens,
                         long long slots, int experts, long long n_cols, long long k,
                         const int* counts, int reps, unsigned long long seed,
                         na_mfma_sweep_result* res);
int na_moe_skinny_sweep(int dev, int dtype, long long tokens, long long slots, int experts,
                        long long n_cols, long long k, int reps, unsigned long long seed,
                        na_mfma_sweep_result* res, double* gbps);

// chip-wide MoE routing sweep, and the three operations it runs on caller-owned
// tensors around the expert GEMM above (specification, operands and checksums
// in moeroutesweep.h). Route: logits bf16 tokens x experts -> topk_ids int32 and
// topk_p float (unnormalised exp2(scale_log2 (logit - max))) tokens x top_k,
// denom float[tokens] (the sum of p over all experts, or over the chosen ones
// with renorm 1). Sort: topk_ids -> offsets int32[experts + 1], row_ids
// int32[tokens * top_k] (what na_moe_gemm_run reads) and slot_of int32 tokens x
// top_k. Combine: out_rows[t] = (sum_j topk_p[t][j] * y[slot_of[t][j]]) * (1 /
// denom[t]), y float tokens * top_k x n_cols, n_cols a multiple of 4. top_k in
// 1..8, top_k <= experts <= 256, tokens * top_k <= NA_MOE_MAX_ROWS. Records,
// with B = ceil(tokens / 256): the route's are 0 .. 4B-1, wave w of block b at 4b
// + w over tokens 256b + 64w ..; the scatter's 4B .. 8B-1 over the same tokens;
// the combine's from 8B, one per wave of 8 tokens, 4 * ceil(tokens / 32) of
// them. na_moe_route_run, na_moe_sort_run and na_moe_combine_run each take room
// for their own kernel's records; `expected` and `verify` take all, one behind
// the other. Results are the matrix-core sweep's. 0 = the default for
// na_moe_route_sweep's shape and reps.
int na_moe_route_fill(int dev, void* logits, void* y, long long tokens, int experts, int top_k,
                      long long n_cols, unsigned long long seed);
int na_moe_route_expected(unsigned long long seed, long long tokens, int experts, int top_k,
                          long long n_cols, int renorm, uint64_t* checksums, long long n_out);
int na_moe_route_run(int dev, const void* logits, void* topk_ids, void* topk_p, void* denom,
                     long long tokens, int experts, int top_k, float scale_log2, int renorm,
                     unsigned long long seed, na_mfma_record* out, long long n_out, double* ms);
int na_moe_sort_run(int dev, const void* topk_ids, void* offsets, void* row_ids, void* slot_of,
                    long long tokens, int experts, int top_k, unsigned long long seed,
                    na_mfma_record* out, long long n_out, double* ms);
int na_moe_combine_run(int dev, const void* y, const void* slot_of, const void* row_ids,
                       const void* topk_p, const void* denom, void* out_rows, long long tokens,
                       int top_k, long long n_cols, unsigned long long seed, na_mfma_record* out,
                       long long n_out, double* ms);
int na_moe_route_verify(const na_mfma_record* recs, long long n, long long tokens, int experts,
                        int top_k, long long n_cols, int renorm, unsigned long long seed,
                        na_mfma_sweep_result* res);
int na_moe_route_sweep(int dev, long long tokens, int experts, int top_k, long long n_cols,
                       int reps, unsigned long long seed, na_mfma_sweep_result* res, double* mtoks,
                       double* gbps);

#ifdef __cplusplus
}
#endif

#endif  // MI355X_NODEAGENT_H
