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

// ---------------------------------------------------------------------------
// Records: what the sweep kernels write, one per wave or workgroup
// ---------------------------------------------------------------------------

// Matrix-core sweep (mfmasweep.h). One per wave, written by one lane.
// cycles/realtime are the deltas of s_memtime (shader clock) and
// s_memrealtime (100 MHz) around the fold loop. The load sweep (loadsweep.h)
// leaves the same record for each of its matrix waves and, with the clocks
// around the stream loop, for each of its stream waves; a wave of a role that
// is switched off leaves it all zero.
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

#ifdef __cplusplus
}
#endif

#endif  // MI355X_NODEAGENT_H
