// MI355X node agent — on-node GPU health validation for provisioned nodes.
//
// The MI355X-native analogue of what the reference left to AKS's NVIDIA
// node-image health machinery: before a freshly provisioned 8×MI355X node is
// trusted (and as the node.health controller's on-node evidence), this agent
// validates the GPU stack end to end: device discovery (gfx950 arch, 288 GB
// HBM3E), an HBM bandwidth self-test (float4 streaming copy; healthy nodes
// reach ~6 TB/s of the 8 TB/s peak; like the SDMA and peer probes it moves
// the memtest pattern and verifies what arrived), an opt-in HBM data-integrity test
// (pattern fill / verify+invert / verify, memtest.h), a VALU FMA correctness
// check, single-wave MFMA checks of every matrix-core datatype and geometry
// the ML workloads live on (one kernel template over the operand traits of
// mfma_frag.h, run and verified by na_mfma_check_run / _verify), an opt-in
// chip-wide matrix-core sweep (one wave per SIMD of every CU, mfmasweep.h),
// opt-in single-wave checks and the same sweep on the block-scaled MX
// instructions in fp4/fp6/bf6/bf8 (na_mx_*, formats in mx_formats.h; both
// families of single-wave checks are rows of one table type with one
// argument check, run and verify: check_run / check_verify), an
// opt-in chip-wide LDS sweep (every LDS access path on every CU, ldssweep.h),
// an opt-in chip-wide cache sweep (L1, L2, write-through, global atomics,
// scalar cache and the cross-XCD read path from every CU, cachesweep.h),
// an opt-in chip-wide vector-unit sweep (register file and VALU of every
// SIMD, valusweep.h), an opt-in chip-wide load sweep (the matrix-core
// sweep's chain, an LDS round trip and an HBM stream on every CU in the same
// cycles, loadsweep.h), and the xGMI peer-to-peer link matrix. The
// chip-wide sweeps share their device-side stamp and placement record
// (sweep_common.h) and their host side ("Shared host side of the chip-wide
// sweeps" below): a further sweep starts from those.
//
// Built for gfx950 only (hipcc --offload-arch=gfx950); exposed as a C ABI
// (nodeagent.h: return codes, limits, record and result structs, one
// prototype per entry point) consumed by gpu_provisioner_amd/nodeagent.py
// (ctypes) both as a CLI and in the k8s DaemonSet health probe.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "memtest.h"
#include "mfma_frag.h"
#include "nodeagent.h"
#include "sweep_common.h"

static char na_last_error_buf[512];

extern "C" const char* na_last_error() { return na_last_error_buf; }

// Every error report: the message into na_last_error, `rc` back.
__attribute__((format(printf, 2, 3))) static int na_error(int rc, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(na_last_error_buf, sizeof(na_last_error_buf), fmt, ap);
    va_end(ap);
    return rc;
}

#define arg_error(...) na_error(NA_ERR_ARG, __VA_ARGS__)

#define HIP_CHECK(expr)                                                                  \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess)                                                            \
            return na_error(NA_ERR_HIP, "%s at %s:%d", hipGetErrorString(_e), __FILE__,  \
                            __LINE__);                                                   \
    } while (0)

// ---------------------------------------------------------------------------
// HIP resources: HIP_CHECK returns from the middle of a function, so whatever
// an entry point allocates is held by one of these and released on every path
// ---------------------------------------------------------------------------

// n elements of device memory. `dev` >= 0 is made current before the free
// (na_p2p_bandwidth holds a buffer on each of two devices).
template <typename T>
struct dev_buf {
    T* p = nullptr;
    int dev = -1;
    dev_buf() = default;
    explicit dev_buf(int d) : dev(d) {}
    dev_buf(dev_buf&& o) noexcept : p(o.p), dev(o.dev) { o.p = nullptr; }
    ~dev_buf() {
        if (p == nullptr) return;
        if (dev >= 0) (void)hipSetDevice(dev);
        (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n * sizeof(T)); }
};

template <int N>
struct dev_events {
    hipEvent_t e[N] = {};  // created by the caller, one HIP_CHECK each
    ~dev_events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

struct dev_stream {
    hipStream_t s = nullptr;
    ~dev_stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

// Streaming float4 copy: the canonical HBM bandwidth probe. Winning shape
// from two on-device variant sweeps (nodeagent/bw_sweep.hip + /tmp round 2,
// MI355X): each workgroup owns ONE CONTIGUOUS slice (consecutive
// iterations stay in the same DRAM window — grid-stride loses ~15%),
// nontemporal dwordx4 (streaming policy, no L2/LC pollution), and FOUR
// independent loads in flight per thread before the stores. Measured
// 6233 GB/s at 16384 WGs x 1024 threads — 99% of the ≈6.3 TB/s this chip
// sustains on read+write streams.
//
// Supported arguments (na_copy_run checks them; tests/
// test_nodeagent_copyprobes.py runs the edges against data): src and dst
// 16-byte aligned and not overlapping (__restrict__ and nontemporal accesses
// make an overlap undefined), n >= 1 vectors of 16 bytes, any grid of 1..65535
// workgroups and any block of 64..1024 threads in whole waves. Workgroup g
// copies vectors [g * per, min((g + 1) * per, n)), per = ceil(n / gridDim.x);
// with n small against the grid the last workgroups start at or past n and
// copy nothing. Neither n nor per needs to be a multiple of anything.
typedef float f4v __attribute__((ext_vector_type(4)));  // raw vector: nt-builtin compatible

// The shape na_hbm_bandwidth times, and what 0 means to na_copy_run: the
// sweep winner, 16384 WGs × 1024 threads (the 4-deep unroll is the kernel's).
static const int COPY_WORKGROUPS = 16384, COPY_THREADS = 1024;

__global__ void copy_f4_kernel(const float4* __restrict__ src_, float4* __restrict__ dst_,
                               size_t n) {
    const f4v* __restrict__ src = reinterpret_cast<const f4v*>(src_);
    f4v* __restrict__ dst = reinterpret_cast<f4v*>(dst_);
    size_t per = (n + gridDim.x - 1) / gridDim.x;
    size_t lo = blockIdx.x * per;
    size_t hi = lo + per < n ? lo + per : n;
    size_t bd = blockDim.x;
    size_t i = lo + threadIdx.x;
    for (; i + 3 * bd < hi; i += 4 * bd) {
        f4v a = __builtin_nontemporal_load(&src[i]);
        f4v b = __builtin_nontemporal_load(&src[i + bd]);
        f4v c = __builtin_nontemporal_load(&src[i + 2 * bd]);
        f4v e = __builtin_nontemporal_load(&src[i + 3 * bd]);
        __builtin_nontemporal_store(a, &dst[i]);
        __builtin_nontemporal_store(b, &dst[i + bd]);
        __builtin_nontemporal_store(c, &dst[i + 2 * bd]);
        __builtin_nontemporal_store(e, &dst[i + 3 * bd]);
    }
    for (; i < hi; i += bd)
        __builtin_nontemporal_store(__builtin_nontemporal_load(&src[i]), &dst[i]);
}

// VALU self-test: dependent FMA chain with a closed-form result.
__global__ void fma_selftest_kernel(float* __restrict__ out, int iters) {
    int lane = threadIdx.x;
    float x = 1.0f;
    float a = 0.5f, b = 0.25f;
    for (int i = 0; i < iters; ++i) x = fmaf(x, a, b);  // x -> x/2 + 1/4, fixpoint 0.5
    out[blockIdx.x * blockDim.x + lane] = x;
}

// Single-wave MFMA checks: one wave issues the MFMA of operand traits T
// (mfma_frag.h) on the operands of generator GEN and stores its accumulator
// registers as 32-bit words.
//
// uniform_operands: A = alpha = 1.5 and B = beta = 2.0 everywhere (exact in
// f32, bf16 and E4M3: bytes 0x3C and 0x40), C = 0, two MFMAs so that
// D = A*B + C chains through the accumulator. Every output element is
// 2*K*alpha*beta regardless of fragment layout, so the check is
// layout-independent and still exercises the input muxes, the matrix pipe
// and the accumulator file. Register r of lane l goes to out[l*4 + r].
//
// tile_operands: D[MN x MN] = A[MN x K]·B[K x MN] from one MFMA on
// ASYMMETRIC integer-valued data, stored row-major and checked against an
// exact host reference; it fails if the per-lane fragment mapping is wrong
// anywhere. Small integers keep both sides exact in every format and
// summation order. k is taken modulo 64, which only the K = 128 MX kind
// notices.
__device__ __host__ inline int tile_a(int i, int k) { return (i * 31 + k * 7) % 7 - 3; }
__device__ __host__ inline int tile_b(int k, int j) { return (k * 13 + j * 3) % 5 - 2; }

__device__ inline void uniform_fill(float& a, float& b) { a = 1.5f, b = 2.0f; }
__device__ inline void uniform_fill(bf16x8& a, bf16x8& b) {
    for (int i = 0; i < 8; ++i) a[i] = (__bf16)1.5f, b[i] = (__bf16)2.0f;
}
__device__ inline void uniform_fill(long& a, long& b) {
    a = 0x3C3C3C3C3C3C3C3CLL, b = 0x4040404040404040LL;
}

struct uniform_operands {
    enum { UNIFORM = 1, CHAIN = 2 };
    template <typename T>
    static __device__ void fill(typename T::frag& a, typename T::frag& b, int) {
        uniform_fill(a, b);
    }
    template <typename T>
    static __device__ int index(int l, int r) {
        return l * 4 + r;
    }
};

struct tile_operands {
    enum { UNIFORM = 0, CHAIN = 1 };
    template <typename T>
    static __device__ void fill(typename T::frag& a, typename T::frag& b, int l) {
        const int rc = l % T::MN, k0 = (l / T::MN) * T::PER_LANE;
#pragma unroll
        for (int i = 0; i < T::PER_LANE; ++i) {
            T::set(a, i, tile_a(rc, (k0 + i) % 64));
            T::set(b, i, tile_b((k0 + i) % 64, rc));
        }
    }
    template <typename T>
    static __device__ int index(int l, int r) {
        return T::d_row(l, r) * T::MN + l % T::MN;
    }
};

// MX kinds (the mfma_mxs_* traits; formulas normative, and carried as an
// independent numpy copy by tests/test_nodeagent_mxchecks.py). Unlike
// tile_a, both operands vary in k, so an error in how K is laid out across
// lanes or packed inside a fragment changes D; blk = k / 32 is the scale
// block, and every D is a multiple of 1/4 below 2^13, exact in any order.
__device__ __host__ inline int mx_tile_a(int i, int k) {
    return (i * 5 + k * 3 + (k >> 4)) % 7 - 3;
}
__device__ __host__ inline int mx_tile_b(int k, int j) {
    return (k * 2 + j * 3 + (k >> 5)) % 5 - 2;
}
__device__ __host__ inline int mx_tile_ea(int i, int blk) { return (i + 2 * blk) % 4 - 1; }
__device__ __host__ inline int mx_tile_eb(int blk, int j) { return (j * 3 + blk) % 3 - 1; }

// mx_tile_operands: D = sum_blk 2^(ea+eb) sum_{k in blk} a(i,k) b(k,j), the
// scales as E8M0 bytes 127 + e.
struct mx_tile_operands : tile_operands {
    template <typename T>
    static __device__ void fill(mx_frag& a, mx_frag& b, int l) {
        const int rc = l % T::MN, g = l / T::MN;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            T::set_a(a, i, mx_encode_int(T::FMT_A, mx_tile_a(rc, T::k_a(g, i))));
            T::set_b(b, i, mx_encode_int(T::FMT_B, mx_tile_b(T::k_b(g, i), rc)));
        }
        T::scale_a(a, 127 + mx_tile_ea(rc, g));
        T::scale_b(b, 127 + mx_tile_eb(g, rc));
    }
};

// mx_code_operands (16x16x128, B in E2M1): A[i][k] is code (i*37 + k*11) % n
// of A's format, n its number of codes; B[k][j] = 1.0 where k % 16 == j, else
// 0; scales 1.0. D[i][j] = sum_{m<8} decode(code(i, j + 16m)) pushes every
// code through A's decoder (11 is odd, so a row's 128 k cover all n codes).
__device__ __host__ inline unsigned mx_code_a(int fmt, int i, int k) {
    return (unsigned)(i * 37 + k * 11) % (1u << mx_bits(fmt));
}

struct mx_code_operands : tile_operands {
    template <typename T>
    static __device__ void fill(mx_frag& a, mx_frag& b, int l) {
        const int rc = l % 16, g = l / 16;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            T::set_a(a, i, mx_code_a(T::FMT_A, rc, T::k_a(g, i)));
            T::set_b(b, i, T::k_b(g, i) % 16 == rc ? mx_encode_int(MX_E2M1, 1) : 0u);
        }
        T::scale_a(a, 127);
        T::scale_b(b, 127);
    }
};

// out: T::MN * T::MN words. Launch with one wave (64 threads): MFMA is a
// per-wave instruction. scale_a reaches the fp8-only MX kind of mfma_frag.h;
// the mfma_mxs_* traits carry their scales in the fragments.
template <typename T, typename GEN>
__global__ void mfma_check_kernel(void* __restrict__ out_, int scale_a) {
    typename T::word* __restrict__ out = static_cast<typename T::word*>(out_);
#if defined(__gfx950__)
    const int l = threadIdx.x;
    typename T::frag a{}, b{};
    GEN::template fill<T>(a, b, l);
    typename T::acc acc{};
    for (int n = 0; n < GEN::CHAIN; ++n) acc = T::mfma(a, b, acc, scale_a);
#pragma unroll
    for (int r = 0; r < (int)(sizeof(acc) / sizeof(typename T::word)); ++r)
        out[GEN::template index<T>(l, r)] = acc[r];
#else
    out[threadIdx.x] = -1;  // wrong arch: fail verification
#endif
}

// LDS self-test: fill the whole per-WG allocation with a position-dependent
// pattern, barrier, read back through a bank-swizzled index. Exercises the
// LDS array + crossbar across all CUs (one WG per CU's worth of a big grid).
__global__ void lds_selftest_kernel(unsigned* __restrict__ fails, size_t words) {
    extern __shared__ unsigned lds[];
    unsigned t = threadIdx.x, n = blockDim.x;
    for (size_t i = t; i < words; i += n)
        lds[i] = (unsigned)(i * 2654435761u) ^ (blockIdx.x * 97u);
    __syncthreads();
    unsigned bad = 0;
    for (size_t i = t; i < words; i += n) {
        // swizzle: XOR within a 64-dword bank row so every lane group hits
        // addresses written by other lanes (crossbar coverage)
        size_t j = (i & ~(size_t)63) | ((i ^ 37) & 63);
        if (j < words && lds[j] != ((unsigned)(j * 2654435761u) ^ (blockIdx.x * 97u))) bad++;
    }
    if (bad) atomicAdd(fails, bad);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" int na_device_count(int* count) {
    HIP_CHECK(hipGetDeviceCount(count));
    return NA_OK;
}

extern "C" int na_device_info(int dev, char* name, int name_len, char* arch, int arch_len,
                              long long* hbm_bytes, int* cus, int* max_clock_khz) {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    std::snprintf(name, name_len, "%s", prop.name);
    std::snprintf(arch, arch_len, "%s", prop.gcnArchName);
    *hbm_bytes = (long long)prop.totalGlobalMem;
    *cus = prop.multiProcessorCount;
    *max_clock_khz = prop.clockRate;
    return NA_OK;
}

// The second of a bandwidth probe's two buffers: n elements, a failure
// reported by the runtime's message alone.
template <typename T>
static int alloc_second(dev_buf<T>& buf, size_t n) {
    hipError_t e = buf.alloc(n);
    return e == hipSuccess ? NA_OK : na_error(NA_ERR_HIP, "%s", hipGetErrorString(e));
}

// The timed loop of the bandwidth probes: op() once as warm-up, then `iters`
// times between two events on `stream`; *ms is the time between the events.
// The null stream synchronises the device after the warm-up, any other
// stream itself. An event of `t` the caller has not created is created after
// the warm-up.
template <typename OP>
static int timed_loop(hipStream_t stream, int iters, dev_events<2>& t, float* ms, OP op) {
    HIP_CHECK(op());
    HIP_CHECK(stream ? hipStreamSynchronize(stream) : hipDeviceSynchronize());
    for (hipEvent_t& e : t.e)
        if (!e) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(t.e[0], stream));
    for (int i = 0; i < iters; ++i) HIP_CHECK(op());
    HIP_CHECK(hipEventRecord(t.e[1], stream));
    HIP_CHECK(hipEventSynchronize(t.e[1]));
    HIP_CHECK(hipEventElapsedTime(ms, t.e[0], t.e[1]));
    return NA_OK;
}

// What the three bandwidth probes check before any HIP call.
static int bw_check_args(const char* fn, long long bytes, int iters, const double* gbs) {
    if (bytes < 16 || iters < 1 || gbs == nullptr)
        return arg_error("%s: need bytes >= 16 (got %lld), iters >= 1 (got %d) and a result "
                         "pointer (gbs %p)",
                         fn, bytes, iters, (const void*)gbs);
    return NA_OK;
}

// The data a bandwidth probe moves and the check that it arrived. prime()
// fills the first `nvec` 16-byte vectors of `src` with the memtest pattern
// (memtest.h; seed COPY_PROBE_SEED, vector index from 0) on src_dev and those
// of `dst` with its complement on dst_dev: memory from hipMalloc may hold the
// pattern from an earlier run, and a copy that writes nothing must leave
// every word wrong, not right. verify() compares `dst` with the pattern on
// dst_dev and reports any mismatch as NA_ERR_VERIFY under `name`, with the two
// devices when they differ. Both synchronise, and both belong outside the
// probe's timed window. They leave dst_dev current. Defined with the memtest
// further down, whose launch and accumulator they use.
struct copy_probe {
    const char* name;
    int src_dev, dst_dev;
    void *src, *dst;
    size_t nvec;
    int prime() const;
    int verify() const;
};

// One launch of the probe's kernel; 0 workgroups or threads are the probe's own.
static void copy_launch(const void* src, void* dst, size_t nvec, int workgroups, int threads) {
    dim3 grid(workgroups ? workgroups : COPY_WORKGROUPS), block(threads ? threads : COPY_THREADS);
    copy_f4_kernel<<<grid, block>>>(static_cast<const float4*>(src), static_cast<float4*>(dst),
                                    nvec);
}

// `bytes` is rounded down to a multiple of 16: that many are copied, verified
// and counted in *gbs.
extern "C" int na_hbm_bandwidth(int dev, long long bytes, int iters, double* gbs) {
    int rc = bw_check_args("na_hbm_bandwidth", bytes, iters, gbs);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipSetDevice(dev));
    size_t n = (size_t)bytes / sizeof(float4);
    dev_buf<float4> src, dst;
    HIP_CHECK(src.alloc(n));
    rc = alloc_second(dst, n);
    if (rc != NA_OK) return rc;
    const copy_probe probe = {"hbm bandwidth", dev, dev, src.p, dst.p, n};
    rc = probe.prime();
    if (rc != NA_OK) return rc;
    dev_events<2> t;
    for (hipEvent_t& e : t.e) HIP_CHECK(hipEventCreate(&e));
    float ms = 0.f;
    rc = timed_loop(nullptr, iters, t, &ms, [&] {
        copy_launch(src.p, dst.p, n, 0, 0);
        return hipSuccess;  // the launches go unqueried, so nothing sits between two of them
    });
    if (rc != NA_OK) return rc;
    // read + write
    *gbs = (2.0 * (double)(n * sizeof(float4)) * iters) / (ms * 1e6);
    return probe.verify();
}

// One launch of copy_f4_kernel on caller-owned device memory, synchronised
// before returning: the kernel na_hbm_bandwidth times, at any shape, so that
// a test can look at what it moved. workgroups == 0 and threads == 0 are the
// probe's own 16384 and 1024. Argument errors (the kernel's supported range,
// above it) are detected before any HIP call.
extern "C" int na_copy_run(int dev, const void* src, void* dst, long long bytes, int workgroups,
                           int threads) {
    const char* fn = "na_copy_run";
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    if (src == nullptr || dst == nullptr || ((s | d) & 15) != 0)
        return arg_error("%s: src %p and dst %p must be non-null and 16-byte aligned", fn, src,
                         dst);
    if (bytes <= 0 || (bytes & 15) != 0)
        return arg_error("%s: bytes (%lld) must be a positive multiple of 16", fn, bytes);
    if (threads != 0 && (threads < 64 || threads > 1024 || threads % 64 != 0))
        return arg_error("%s: threads (%d) must be 0 (the probe's %d) or a multiple of 64 in "
                         "64..1024",
                         fn, threads, COPY_THREADS);
    if (workgroups < 0 || workgroups > 65535)
        return arg_error("%s: workgroups (%d) must be in 0..65535, 0 being the probe's %d", fn,
                         workgroups, COPY_WORKGROUPS);
    if ((s < d ? d - s : s - d) < (uintptr_t)bytes)
        return arg_error("%s: src %p and dst %p overlap over bytes (%lld); the kernel takes "
                         "disjoint ranges only",
                         fn, src, dst, bytes);
    HIP_CHECK(hipSetDevice(dev));
    copy_launch(src, dst, (size_t)bytes / 16, workgroups, threads);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    return NA_OK;
}

extern "C" int na_fma_selftest(int dev) {
    HIP_CHECK(hipSetDevice(dev));
    const int blocks = 1024, threads = 256, iters = 256;
    dev_buf<float> out;
    HIP_CHECK(out.alloc((size_t)blocks * threads));
    fma_selftest_kernel<<<dim3(blocks), dim3(threads)>>>(out.p, iters);
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> host((size_t)blocks * threads);
    HIP_CHECK(hipMemcpy(host.data(), out.p, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < blocks * threads; ++i) {
        // fixpoint of x -> x/2 + 1/4 is 0.5; 256 iterations converge exactly
        if (host[i] != 0.5f)
            return na_error(NA_ERR_VERIFY, "fma selftest: lane %d got %g want 0.5", i, host[i]);
    }
    return NA_OK;
}

// How a single-wave check's wanted D[i][j] comes about.
enum check_want {
    WANT_UNIFORM,   // the constant 2*K*alpha*beta (alpha*beta = 3)
    WANT_TILE,      // `mult` times the integer product of tile_a and tile_b
    WANT_MX_TILE,   // the block-scaled sum of mx_tile_operands
    WANT_MX_CODES,  // the code-point sum of mx_code_operands over format `code_fmt`
};

// One row per kind of the single-wave checks, of both families: the NA_MFMA_*
// kinds and the NA_MX_* kinds of mfma_frag.h. `label` opens the failure
// message. The words are int32 for the i8 kind (`is_int`), float32 otherwise.
struct wave_check {
    const char* label;
    void (*kernel)(void*, int);
    int mn, k, scale_a;
    bool is_int;
    check_want want;
    int mult, code_fmt;
    int words() const { return mn * mn; }  // 64 lanes x 4 registers for the uniform kinds too
};

template <typename T, typename GEN>
static wave_check check_row(const char* label, check_want want, int scale_a = 0, int mult = 1,
                            int code_fmt = -1) {
    return {label, mfma_check_kernel<T, GEN>, T::MN, T::K, scale_a,
            std::is_same<typename T::word, int>::value, want, mult, code_fmt};
}
template <typename T>
static wave_check mx_tile_row(const char* label) {
    return check_row<T, mx_tile_operands>(label, WANT_MX_TILE);
}
template <int FMT, int OA, int OB>
static wave_check mx_code_row(const char* label) {
    typedef mfma_mxs_16x16x128<FMT, MX_E2M1, OA, OB> T;
    return check_row<T, mx_code_operands>(label, WANT_MX_CODES, 0, 1, FMT);
}

// In the order of the NA_MFMA_* codes. D of the two MX kinds is `mult` times
// the unscaled product.
static const wave_check mfma_checks[NA_MFMA_KINDS] = {
    check_row<mfma_f32_16x16x4, uniform_operands>("mfma selftest", WANT_UNIFORM),
    check_row<mfma_bf16_16x16x32, uniform_operands>("mfma-bf16 selftest", WANT_UNIFORM),
    check_row<mfma_fp8_16x16x32, uniform_operands>("mfma-fp8 selftest", WANT_UNIFORM),
    check_row<mfma_bf16_16x16x32, tile_operands>("mfma bf16 tile", WANT_TILE),
    check_row<mfma_f16_16x16x32, tile_operands>("mfma f16 tile", WANT_TILE),
    check_row<mfma_fp8_16x16x32, tile_operands>("mfma fp8 tile", WANT_TILE),
    check_row<mfma_i8_16x16x64, tile_operands>("mfma i8 tile", WANT_TILE),
    check_row<mfma_bf16_32x32x16, tile_operands>("mfma bf16 32x32 tile", WANT_TILE),
    check_row<mfma_mx_16x16x128, tile_operands>("mfma mx tile (scale 1x)", WANT_TILE, 0x7F, 1),
    check_row<mfma_mx_16x16x128, tile_operands>("mfma mx tile (scale 2x)", WANT_TILE, 0x80, 2),
};

// In the order of the NA_MX_* codes. Between them the kinds select every byte
// of the scale register on each side.
static const wave_check mx_checks[NA_MX_KINDS] = {
    mx_tile_row<mfma_mxs_16x16x128<MX_E2M1, MX_E2M1, 1, 2>>("mx fp4 tile"),
    mx_tile_row<mfma_mxs_16x16x128<MX_E2M3, MX_E2M3, 2, 3>>("mx fp6 tile"),
    mx_tile_row<mfma_mxs_16x16x128<MX_E3M2, MX_E3M2, 3, 0>>("mx bf6 tile"),
    mx_tile_row<mfma_mxs_16x16x128<MX_E5M2, MX_E5M2, 0, 1>>("mx bf8 tile"),
    mx_tile_row<mfma_mxs_16x16x128<MX_E4M3, MX_E2M1, 2, 1>>("mx fp8 x fp4 tile"),
    mx_tile_row<mfma_mxs_32x32x64<MX_E2M1, MX_E2M1, 3, 2>>("mx fp4 32x32 tile"),
    mx_code_row<MX_E2M1, 1, 3>("mx fp4 codes"),
    mx_code_row<MX_E2M3, 3, 1>("mx fp6 codes"),
    mx_code_row<MX_E3M2, 2, 2>("mx bf6 codes"),
};

// A family's table; `prefix` opens its argument errors.
struct check_family {
    const char* prefix;
    const wave_check* rows;
    int kinds;
};
static const check_family mfma_family = {"na_mfma_check", mfma_checks, NA_MFMA_KINDS};
static const check_family mx_family = {"na_mx_check", mx_checks, NA_MX_KINDS};

// Every value is a small integer or a multiple of 1/4 below 2^13: exact in
// float, and every partial sum with it.
static float check_want_at(const wave_check& c, int i, int j) {
    float want = 0.f;
    switch (c.want) {
        case WANT_UNIFORM: return (float)(2 * c.k * 3);
        case WANT_TILE: {
            int dot = 0;
            for (int k = 0; k < c.k; ++k) dot += tile_a(i, k % 64) * tile_b(k % 64, j);
            return (float)(dot * c.mult);
        }
        case WANT_MX_TILE:
            for (int blk = 0; blk < c.k / 32; ++blk) {
                int dot = 0;
                for (int k = blk * 32; k < blk * 32 + 32; ++k)
                    dot += mx_tile_a(i, k) * mx_tile_b(k, j);
                want += std::ldexp((float)dot, mx_tile_ea(i, blk) + mx_tile_eb(blk, j));
            }
            return want;
        case WANT_MX_CODES:
            for (int m = 0; m < c.k / 16; ++m)
                want += mx_decode(c.code_fmt, mx_code_a(c.code_fmt, i, j + 16 * m));
            return want;
    }
    return want;
}

static const wave_check* check_args(const check_family& fam, const char* fn, int kind,
                                    const void* words, int n_words) {
    if (kind >= 0 && kind < fam.kinds && words != nullptr && n_words >= fam.rows[kind].words())
        return &fam.rows[kind];
    arg_error("%s_%s: need kind in 0..%d (got %d) and room for its 256 words, 1024 for the 32x32 "
              "tile (words %p, n_words %d)",
              fam.prefix, fn, fam.kinds - 1, kind, words, n_words);
    return nullptr;
}

// Launches the one wave of `kind` and copies its raw 32-bit words back.
// Argument errors are detected before any HIP call.
static int check_run(const check_family& fam, int dev, int kind, void* out, int n_words) {
    const wave_check* c = check_args(fam, "run", kind, out, n_words);
    if (c == nullptr) return NA_ERR_ARG;
    HIP_CHECK(hipSetDevice(dev));
    dev_buf<uint32_t> d;
    HIP_CHECK(d.alloc((size_t)c->words()));
    c->kernel<<<dim3(1), dim3(64)>>>(d.p, c->scale_a);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, d.p, (size_t)c->words() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NA_OK;
}

// Pure host code: compares the words of `kind` by value against the exact
// reference. The first mismatch is named in na_last_error.
static int check_verify(const check_family& fam, int kind, const void* words, int n_words) {
    const wave_check* c = check_args(fam, "verify", kind, words, n_words);
    if (c == nullptr) return NA_ERR_ARG;
    const float* f = static_cast<const float*>(words);
    const int* w = static_cast<const int*>(words);
    for (int e = 0; e < c->words(); ++e) {
        const int i = e / c->mn, j = e % c->mn;
        const float want = check_want_at(*c, i, j);
        if (c->is_int ? w[e] == (int)want : f[e] == want) continue;
        if (c->want == WANT_UNIFORM)
            return na_error(NA_ERR_VERIFY, "%s: elem %d got %g want %g", c->label, e, f[e], want);
        if (c->is_int)
            return na_error(NA_ERR_VERIFY, "%s: D[%d][%d] got %d want %d", c->label, i, j, w[e],
                            (int)want);
        return na_error(NA_ERR_VERIFY, "%s: D[%d][%d] got %g want %g", c->label, i, j, f[e], want);
    }
    return NA_OK;
}

static int check_one(const check_family& fam, int dev, int kind) {
    uint32_t words[1024];
    int rc = check_run(fam, dev, kind, words, 1024);
    return rc != NA_OK ? rc : check_verify(fam, kind, words, 1024);
}

// The words of an NA_MFMA_* kind are int32 for the i8 kind, float32 otherwise.
extern "C" int na_mfma_check_run(int dev, int kind, void* out, int n_words) {
    return check_run(mfma_family, dev, kind, out, n_words);
}
extern "C" int na_mfma_check_verify(int kind, const void* words, int n_words) {
    return check_verify(mfma_family, kind, words, n_words);
}
static int mfma_check_one(int dev, int kind) { return check_one(mfma_family, dev, kind); }

extern "C" int na_mfma_selftest(int dev) { return mfma_check_one(dev, NA_MFMA_F32_UNIFORM); }
extern "C" int na_mfma_bf16_selftest(int dev) { return mfma_check_one(dev, NA_MFMA_BF16_UNIFORM); }
extern "C" int na_mfma_fp8_selftest(int dev) { return mfma_check_one(dev, NA_MFMA_FP8_UNIFORM); }
extern "C" int na_mfma_bf16_tile_check(int dev) { return mfma_check_one(dev, NA_MFMA_BF16_TILE); }
extern "C" int na_mfma_f16_tile_check(int dev) { return mfma_check_one(dev, NA_MFMA_F16_TILE); }
extern "C" int na_mfma_fp8_tile_check(int dev) { return mfma_check_one(dev, NA_MFMA_FP8_TILE); }
extern "C" int na_mfma_i8_tile_check(int dev) { return mfma_check_one(dev, NA_MFMA_I8_TILE); }
extern "C" int na_mfma_bf16_tile32_check(int dev) {
    return mfma_check_one(dev, NA_MFMA_BF16_TILE32);
}
// Two checks in one: layout at scale 1.0, then scale semantics — E8M0
// exponent 128 on A doubles the result.
extern "C" int na_mfma_mx_tile_check(int dev) {
    int rc = mfma_check_one(dev, NA_MFMA_MX_TILE);
    return rc != NA_OK ? rc : mfma_check_one(dev, NA_MFMA_MX_TILE_X2);
}

// ---------------------------------------------------------------------------
// Single-wave MX checks: every operand format, the per-lane scales and the
// scale byte select of the f8f6f4 instructions (traits in mfma_frag.h)
// ---------------------------------------------------------------------------

// Pure host code, for tests of the encodings and the packing.
extern "C" int na_mx_decode(int fmt, int code, float* value) {
    if (fmt < 0 || fmt >= MX_FORMATS || code < 0 || code >= 1 << mx_bits(fmt) ||
        value == nullptr)
        return arg_error("na_mx_decode: need fmt in 0..%d (got %d), a code of its width (got %d) "
                         "and a result pointer",
                         MX_FORMATS - 1, fmt, code);
    *value = mx_decode(fmt, (unsigned)code);
    return NA_OK;
}

// n codes (a multiple of 32: whole fragments) packed as a lane's fragment
// registers are, fragment after fragment; words receives n * width / 32.
extern "C" int na_mx_pack(int fmt, const int* codes, int n, uint32_t* words, int n_words) {
    bool ok = fmt >= 0 && fmt < MX_FORMATS && codes != nullptr && words != nullptr && n > 0 &&
              n % 32 == 0 && (long long)n_words * 32 >= (long long)n * mx_bits(fmt);
    for (int i = 0; ok && i < n; ++i) ok = codes[i] >= 0 && codes[i] < 1 << mx_bits(fmt);
    if (!ok)
        return arg_error("na_mx_pack: need fmt in 0..%d (got %d), n a positive multiple of 32 "
                         "(got %d) of codes of that width, and room for n * width / 32 words "
                         "(codes %p, words %p, n_words %d)",
                         MX_FORMATS - 1, fmt, n, (const void*)codes, (void*)words, n_words);
    const int regs = mx_bits(fmt);  // 32 elements of `width` bits fill `width` registers
    std::memset(words, 0, (size_t)(n / 32) * regs * sizeof(uint32_t));
    for (int i = 0; i < n; ++i) {
        uint32_t* frag = words + (i / 32) * regs;
        mx_put(frag, fmt, i % 32, (unsigned)codes[i]);
    }
    return NA_OK;
}

// As na_mfma_check_run / na_mfma_check_verify, on the NA_MX_* kinds: every
// word is a float32.
extern "C" int na_mx_check_run(int dev, int kind, void* out, int n_words) {
    return check_run(mx_family, dev, kind, out, n_words);
}
extern "C" int na_mx_check_verify(int kind, const void* words, int n_words) {
    return check_verify(mx_family, kind, words, n_words);
}

// Every kind in turn, stopping at the first that fails.
extern "C" int na_mx_checks(int dev) {
    for (int kind = 0; kind < NA_MX_KINDS; ++kind) {
        int rc = check_one(mx_family, dev, kind);
        if (rc != NA_OK) return rc;
    }
    return NA_OK;
}

// The device's whole per-workgroup LDS allocation (160 KiB/CU on gfx950, minus
// any runtime-reserved slice reported via sharedMemPerBlock): what
// na_lds_selftest tests and the dynamic LDS the sweep kernels are launched
// with. It is more than half of the CU's LDS, so one workgroup per CU.
static int sweep_lds_bytes(int dev, size_t* bytes) {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    *bytes = std::min<size_t>(prop.sharedMemPerBlock, MS_CU_LDS_BYTES);
    return NA_OK;
}

extern "C" int na_lds_selftest(int dev, long long* bytes_tested) {
    HIP_CHECK(hipSetDevice(dev));
    size_t lds_bytes = 0;
    int rc = sweep_lds_bytes(dev, &lds_bytes);
    if (rc != NA_OK) return rc;
    size_t words = lds_bytes / sizeof(unsigned);
    dev_buf<unsigned> fails;
    HIP_CHECK(fails.alloc(1));
    HIP_CHECK(hipMemset(fails.p, 0, sizeof(unsigned)));
    // 2048 WGs: every CU's LDS array gets exercised multiple times
    lds_selftest_kernel<<<dim3(2048), dim3(256), lds_bytes>>>(fails.p, words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return na_error(NA_ERR_HIP, "lds launch: %s", hipGetErrorString(e));
    HIP_CHECK(hipDeviceSynchronize());
    unsigned bad = 0;
    HIP_CHECK(hipMemcpy(&bad, fails.p, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (bytes_tested) *bytes_tested = (long long)lds_bytes;
    if (bad)
        return na_error(NA_ERR_VERIFY, "lds selftest: %u mismatched words across %zu-byte LDS", bad,
                        lds_bytes);
    return NA_OK;
}

extern "C" int na_sdma_bandwidth(int dev, long long bytes, int iters, double* gbs) {
    // device-to-device copy through hipMemcpyAsync: the runtime routes
    // large D2D copies through the SDMA engines — the same hardware RCCL
    // leans on for xGMI peer traffic. A sick SDMA engine shows up here
    // before any collective does. All of `bytes` is copied and counted; the
    // verified part is `bytes` rounded down to a multiple of 16.
    int rc = bw_check_args("na_sdma_bandwidth", bytes, iters, gbs);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipSetDevice(dev));
    dev_buf<char> src, dst;
    HIP_CHECK(src.alloc((size_t)bytes));
    rc = alloc_second(dst, (size_t)bytes);
    if (rc != NA_OK) return rc;
    const copy_probe probe = {"sdma bandwidth", dev, dev, src.p, dst.p, (size_t)bytes / 16};
    rc = probe.prime();
    if (rc != NA_OK) return rc;
    dev_stream stream;
    HIP_CHECK(hipStreamCreate(&stream.s));
    dev_events<2> t;  // created by timed_loop
    float ms = 0.f;
    rc = timed_loop(stream.s, iters, t, &ms, [&] {
        return hipMemcpyAsync(dst.p, src.p, (size_t)bytes, hipMemcpyDeviceToDevice, stream.s);
    });
    if (rc != NA_OK) return rc;
    *gbs = (2.0 * (double)bytes * iters) / (ms * 1e6);  // read + write
    return probe.verify();
}

extern "C" int na_p2p_matrix(int n, int* out /* n*n */) {
    if (n < 1 || out == nullptr)
        return arg_error("na_p2p_matrix: need n >= 1 (got %d) and a result pointer (out %p)", n,
                         (void*)out);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            if (i == j) {
                out[i * n + j] = 1;
                continue;
            }
            int can = 0;
            HIP_CHECK(hipDeviceCanAccessPeer(&can, i, j));
            out[i * n + j] = can;
        }
    }
    return NA_OK;
}

// Returns with `src` current on every path once it has been made so: sbuf is
// destroyed last, and each buffer is freed with its own device current. The
// pattern is filled on `src` and verified on `dst`, each by its own device.
// All of `bytes` is copied and counted; the verified part is `bytes` rounded
// down to a multiple of 16.
extern "C" int na_p2p_bandwidth(int src, int dst, long long bytes, int iters, double* gbs) {
    int rc = bw_check_args("na_p2p_bandwidth", bytes, iters, gbs);
    if (rc != NA_OK) return rc;
    if (src < 0 || dst < 0 || src == dst)
        return arg_error("na_p2p_bandwidth: need two different devices, neither negative (got src "
                         "%d, dst %d)",
                         src, dst);
    HIP_CHECK(hipSetDevice(src));
    dev_buf<char> sbuf(src), dbuf(dst);
    HIP_CHECK(sbuf.alloc((size_t)bytes));
    HIP_CHECK(hipSetDevice(dst));
    rc = alloc_second(dbuf, (size_t)bytes);
    if (rc != NA_OK) return rc;
    const copy_probe probe = {"p2p bandwidth", src, dst, sbuf.p, dbuf.p, (size_t)bytes / 16};
    rc = probe.prime();
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipSetDevice(src));
    dev_events<2> t;
    for (hipEvent_t& ev : t.e) HIP_CHECK(hipEventCreate(&ev));
    float ms = 0.f;
    rc = timed_loop(nullptr, iters, t, &ms, [&] {
        return hipMemcpyPeer(dbuf.p, dst, sbuf.p, src, (size_t)bytes);
    });
    if (rc != NA_OK) return rc;
    *gbs = ((double)bytes * iters) / (ms * 1e6);
    return probe.verify();
}

// ---------------------------------------------------------------------------
// HBM data-integrity test (kernels in memtest.h)
// ---------------------------------------------------------------------------
//
// The bandwidth probes above move this section's pattern and verify their
// destination once, after the timed loop (copy_probe, defined below): that
// catches a copy that drops, misplaces or damages data, on buffers of the
// probe's size and at one polarity. This is the test of the memory itself.
// One round is fill(seed+r) → verify+invert → verify(inverted): every cell is
// read back at both polarities, and because the pattern is a bijection of
// the vector index an aliased address line is a mismatch too. Phases are
// separate launches over the whole region, so read-back never comes from a
// register. HBM ECC silently corrects single-bit cell errors; what shows up
// here is what ECC does not fix — uncorrected/multi-bit corruption,
// addressing faults and data-path faults.

extern "C" int na_mem_info(int dev, long long* free_bytes, long long* total_bytes) {
    HIP_CHECK(hipSetDevice(dev));
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (free_bytes) *free_bytes = (long long)free_b;
    if (total_bytes) *total_bytes = (long long)total_b;
    return NA_OK;
}

// One launch covers at most 1 GiB (16384 workgroups — the copy probe's
// measured grid); larger regions take several launches. na_hbm_memtest
// allocates in chunks of the same size.
static const size_t MT_MAX_LAUNCH_VECS = (size_t)1 << 26;

static int mt_launch(int mode, void* dptr, size_t nvec, mt_u64 v0, mt_u64 seed, int invert,
                     mt_accum* d_acc) {
    const mt_u64 base = seed * 0x9E3779B97F4A7C15ULL;
    const mt_u64 inv = invert ? ~0ULL : 0ULL;
    // indexed by the MT_* mode
    static void (*const kernels[3])(mt_vec*, size_t, mt_u64, mt_u64, mt_u64, mt_accum*) = {
        memtest_kernel<MT_FILL>, memtest_kernel<MT_VERIFY>, memtest_kernel<MT_VERIFY_FLIP>};
    for (size_t off = 0; off < nvec; off += MT_MAX_LAUNCH_VECS) {
        size_t n = nvec - off < MT_MAX_LAUNCH_VECS ? nvec - off : MT_MAX_LAUNCH_VECS;
        mt_vec* p = reinterpret_cast<mt_vec*>(dptr) + off;
        dim3 grid((unsigned)((n + MT_TILE - 1) / MT_TILE)), block(MT_BLOCK);
        kernels[mode]<<<grid, block>>>(p, n, v0 + off, base, inv, d_acc);
        HIP_CHECK(hipGetLastError());
    }
    return NA_OK;
}

// Device-side accumulator.
struct mt_dev_accum {
    dev_buf<mt_accum> d;
    int init() {
        HIP_CHECK(d.alloc(1));
        mt_accum zero = {0, UINT64_MAX, 0};
        HIP_CHECK(hipMemcpy(d.p, &zero, sizeof(zero), hipMemcpyHostToDevice));
        return NA_OK;
    }
    int read(uint64_t bytes, na_memtest_result* out) {
        mt_accum h;
        HIP_CHECK(hipMemcpy(&h, d.p, sizeof(h), hipMemcpyDeviceToHost));
        out->bytes_tested = bytes;
        out->bad_words = h.bad_words;
        out->first_bad_offset = h.first_bad_offset;
        out->xor_mask = h.xor_mask;
        return NA_OK;
    }
};

static int mt_check_args(const char* fn, const void* dptr, long long bytes) {
    if (dptr == nullptr || ((uintptr_t)dptr & 15) != 0 || bytes <= 0 || (bytes & 15) != 0)
        return arg_error("%s: pointer %p must be 16-byte aligned and bytes (%lld) a positive "
                         "multiple of 16",
                         fn, dptr, bytes);
    return NA_OK;
}

// `what` opens the message: the memtest, or a bandwidth probe.
static int mt_verdict(const char* what, const na_memtest_result* r) {
    if (r->bad_words == 0) return NA_OK;
    return na_error(NA_ERR_VERIFY,
                    "%s: %llu bad 64-bit words in %llu bytes, first at offset 0x%llx, "
                    "failing bits 0x%016llx",
                    what, (unsigned long long)r->bad_words, (unsigned long long)r->bytes_tested,
                    (unsigned long long)r->first_bad_offset, (unsigned long long)r->xor_mask);
}

// The bandwidth probes' data (copy_probe, declared with them). The seed is
// "MI355XBW", fixed: a probe's two buffers live for one call.
static const mt_u64 COPY_PROBE_SEED = 0x4D49333535584257ULL;

int copy_probe::prime() const {
    HIP_CHECK(hipSetDevice(src_dev));
    int rc = mt_launch(MT_FILL, src, nvec, 0, COPY_PROBE_SEED, 0, nullptr);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipSetDevice(dst_dev));
    rc = mt_launch(MT_FILL, dst, nvec, 0, COPY_PROBE_SEED, 1, nullptr);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipDeviceSynchronize());
    return NA_OK;
}

int copy_probe::verify() const {
    HIP_CHECK(hipSetDevice(dst_dev));
    mt_dev_accum acc;
    acc.d.dev = dst_dev;
    int rc = acc.init();
    if (rc != NA_OK) return rc;
    rc = mt_launch(MT_VERIFY, dst, nvec, 0, COPY_PROBE_SEED, 0, acc.d.p);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipDeviceSynchronize());
    na_memtest_result res;
    rc = acc.read((uint64_t)nvec * 16, &res);
    if (rc != NA_OK) return rc;
    char what[64];
    if (src_dev == dst_dev)
        std::snprintf(what, sizeof(what), "%s", name);
    else
        std::snprintf(what, sizeof(what), "%s %d->%d", name, src_dev, dst_dev);
    return mt_verdict(what, &res);
}

// Pointer-level calls on caller-owned device memory (16-byte aligned,
// bytes a positive multiple of 16). Both synchronise before returning.
extern "C" int na_memtest_fill(int dev, void* dptr, long long bytes, unsigned long long seed,
                               int invert) {
    int rc = mt_check_args("na_memtest_fill", dptr, bytes);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipSetDevice(dev));
    rc = mt_launch(MT_FILL, dptr, (size_t)bytes / 16, 0, seed, invert, nullptr);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipDeviceSynchronize());
    return NA_OK;
}

// flip != 0: also store the complement of the expected pattern (the region
// then holds the pattern for !invert). Returns NA_ERR_VERIFY when any word
// mismatched; *out is filled either way.
extern "C" int na_memtest_verify(int dev, void* dptr, long long bytes, unsigned long long seed,
                                 int invert, int flip, na_memtest_result* out) {
    int rc = mt_check_args("na_memtest_verify", dptr, bytes);
    if (rc != NA_OK) return rc;
    if (out == nullptr) return arg_error("na_memtest_verify: out must not be null");
    HIP_CHECK(hipSetDevice(dev));
    mt_dev_accum acc;
    rc = acc.init();
    if (rc != NA_OK) return rc;
    rc = mt_launch(flip ? MT_VERIFY_FLIP : MT_VERIFY, dptr, (size_t)bytes / 16, 0, seed, invert,
                   acc.d.p);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipDeviceSynchronize());
    rc = acc.read((uint64_t)bytes, out);
    if (rc != NA_OK) return rc;
    return mt_verdict("hbm memtest", out);
}

// Whole test on a region the agent allocates itself, in chunks of at most
// 1 GiB so no huge contiguous allocation is needed. pass_gbs (optional,
// 3 doubles) receives GB/s of the fill, verify+invert and verify passes;
// *gbs the aggregate over all passes (4x the region per round), HIP-event
// timed. `bytes` is rounded down to a multiple of 16.
extern "C" int na_hbm_memtest_passes(int dev, long long bytes, int rounds,
                                     unsigned long long seed, na_memtest_result* out,
                                     double* gbs, double* pass_gbs) {
    bytes &= ~15LL;
    if (bytes < 16 || rounds < 1 || out == nullptr)
        return arg_error("na_hbm_memtest: need bytes >= 16 (got %lld), rounds >= 1 (got %d) and a "
                         "result pointer",
                         bytes, rounds);
    HIP_CHECK(hipSetDevice(dev));
    const size_t nvec = (size_t)bytes / 16;
    std::vector<dev_buf<mt_vec>> chunks;
    std::vector<size_t> chunk_vecs;
    for (size_t off = 0; off < nvec; off += MT_MAX_LAUNCH_VECS) {
        size_t n = nvec - off < MT_MAX_LAUNCH_VECS ? nvec - off : MT_MAX_LAUNCH_VECS;
        chunks.emplace_back();
        hipError_t e = chunks.back().alloc(n);
        if (e != hipSuccess) {
            (void)hipGetLastError();  // consumed here, not by a later check
            return na_error(NA_ERR_HIP,
                            "hbm memtest: allocation failed after %zu of %lld bytes: %s", off * 16,
                            bytes, hipGetErrorString(e));
        }
        chunk_vecs.push_back(n);
    }
    mt_dev_accum acc;
    int rc = acc.init();
    if (rc != NA_OK) return rc;
    dev_events<4> ev;
    for (hipEvent_t& e : ev.e) HIP_CHECK(hipEventCreate(&e));

    // each phase sweeps the WHOLE region before the next starts, so by the
    // time a chunk is read back the rest of the region has gone through the
    // caches in between
    static const int phase_mode[3] = {MT_FILL, MT_VERIFY_FLIP, MT_VERIFY};
    static const int phase_invert[3] = {0, 0, 1};
    double phase_ms[3] = {0.0, 0.0, 0.0};
    for (int r = 0; r < rounds; ++r) {
        HIP_CHECK(hipEventRecord(ev.e[0]));
        for (int ph = 0; ph < 3; ++ph) {
            size_t off = 0;
            for (size_t c = 0; c < chunks.size(); ++c) {
                rc = mt_launch(phase_mode[ph], chunks[c].p, chunk_vecs[c], off, seed + (mt_u64)r,
                               phase_invert[ph], acc.d.p);
                if (rc != NA_OK) return rc;
                off += chunk_vecs[c];
            }
            HIP_CHECK(hipEventRecord(ev.e[ph + 1]));
        }
        HIP_CHECK(hipEventSynchronize(ev.e[3]));
        for (int ph = 0; ph < 3; ++ph) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, ev.e[ph], ev.e[ph + 1]));
            phase_ms[ph] += ms;
        }
    }
    HIP_CHECK(hipDeviceSynchronize());
    rc = acc.read((uint64_t)bytes, out);
    if (rc != NA_OK) return rc;
    // bytes moved per round: fill writes 1x, verify+invert reads and writes
    // (2x), verify reads 1x
    static const double phase_traffic[3] = {1.0, 2.0, 1.0};
    double total_ms = 0.0;
    for (int ph = 0; ph < 3; ++ph) {
        total_ms += phase_ms[ph];
        if (pass_gbs)
            pass_gbs[ph] = phase_traffic[ph] * (double)bytes * rounds / (phase_ms[ph] * 1e6);
    }
    if (gbs) *gbs = 4.0 * (double)bytes * rounds / (total_ms * 1e6);
    return mt_verdict("hbm memtest", out);
}

extern "C" int na_hbm_memtest(int dev, long long bytes, int rounds, unsigned long long seed,
                              na_memtest_result* out, double* gbs) {
    return na_hbm_memtest_passes(dev, bytes, rounds, seed, out, gbs, nullptr);
}

// ---------------------------------------------------------------------------
// Shared host side of the chip-wide sweeps (device side: sweep_common.h)
// ---------------------------------------------------------------------------
//
// Each sweep below (matrix cores, LDS, caches, vector unit) is a kernel that leaves
// one record per wave or workgroup, a *_run that launches it once (the cache
// sweep: its two kernels, one after the other), a pure-host
// *_verify that recomputes every record's checksums, and an entry point that
// runs twice and verifies. A sweep owns its reference, its verdict rules, its
// messages and its argument checks; the launch (sweep_launch), the defaults
// and the warm-up (sweep_defaults, sweep_twice) and the bookkeeping over the
// records (sweep_census, median_of) are here, for the next sweep too. The
// LDS size they launch with (sweep_lds_bytes) is further up, with
// na_lds_selftest, which tests the same allocation.

// What 0 means to the whole-sweep entry points: four workgroups per CU, and
// the sweep's default count of folds, passes or rounds.
static int sweep_defaults(int dev, int* workgroups, int* iters, int default_iters) {
    if (*iters == 0) *iters = default_iters;
    if (*workgroups == 0) {
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        *workgroups = 4 * prop.multiProcessorCount;
    }
    return NA_OK;
}

// One HIP-event timed launch on `dev`: launch(records) starts the kernel on n
// device records, which come back in out. A record its wave or workgroup
// never wrote stays 0xFF, carries no valid index and fails the verify.
template <typename R, typename LAUNCH>
static int sweep_launch(int dev, size_t n, R* out, double* ms, LAUNCH launch) {
    HIP_CHECK(hipSetDevice(dev));
    dev_buf<R> d;
    HIP_CHECK(d.alloc(n));
    HIP_CHECK(hipMemset(d.p, 0xFF, n * sizeof(R)));
    dev_events<2> ev;
    for (hipEvent_t& e : ev.e) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(ev.e[0]));
    launch(d.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[1]));
    HIP_CHECK(hipEventSynchronize(ev.e[1]));
    float elapsed = 0.f;
    HIP_CHECK(hipEventElapsedTime(&elapsed, ev.e[0], ev.e[1]));
    HIP_CHECK(hipMemcpy(out, d.p, n * sizeof(R), hipMemcpyDeviceToHost));
    if (ms) *ms = (double)elapsed;
    return NA_OK;
}

// run() twice: the first is the untimed warm-up, the second leaves its
// records and its time.
template <typename RUN>
static int sweep_twice(RUN run) {
    int rc = run();
    return rc != NA_OK ? rc : run();
}

// 0 for none.
template <typename T>
static T median_of(std::vector<T>& v) {
    if (v.empty()) return 0;
    std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
    return v[v.size() / 2];
}

// Who took part and who failed, over any of the sweeps' records. A unit is
// (xcc, se, sh, cu, simd), simd 0 for the records that are per CU.
struct sweep_census {
    std::vector<bool> cu_seen, simd_seen, cu_bad;
    std::vector<double> mhz;  // cycles / realtime x 100 MHz, per record
    uint64_t cus_seen = 0, simds_seen = 0, bad_cus = 0;
    uint32_t first_bad[5] = {}, listed = 0;  // the first bad unit; 0s for none
    uint32_t bad_list[NA_SWEEP_MAX_LISTED][5] = {};  // the first distinct bad units

    sweep_census() : cu_seen(1 << 11), simd_seen(1 << 13), cu_bad(1 << 11) {}

    template <typename R>
    void see(const R& r, uint32_t simd = 0) {
        const uint32_t key = ms_cu_key(r), simd_key = key << 2 | (simd & 3);
        if (!cu_seen[key]) cu_seen[key] = true, cus_seen++;
        if (!simd_seen[simd_key]) simd_seen[simd_key] = true, simds_seen++;
        if (r.realtime) mhz.push_back((double)r.cycles / (double)r.realtime * 100.0);
    }

    template <typename R>
    void mark_bad(const R& r, uint32_t simd = 0) {
        const uint32_t key = ms_cu_key(r), unit[5] = {r.xcc, r.se, r.sh, r.cu, simd};
        if (!cu_bad[key]) cu_bad[key] = true, bad_cus++;
        if (listed == 0) std::memcpy(first_bad, unit, sizeof(unit));
        bool known = false;
        for (uint32_t k = 0; k < listed && !known; ++k)
            known = std::memcmp(bad_list[k], unit, sizeof(unit)) == 0;
        if (!known && listed < NA_SWEEP_MAX_LISTED)
            std::memcpy(bad_list[listed++], unit, sizeof(unit));
    }

    // The leading W fields of the first bad unit and of the listed ones, into
    // a result struct's arrays.
    template <int W>
    void bad_units(uint32_t (&first)[W], uint32_t (&list)[NA_SWEEP_MAX_LISTED][W],
                   uint32_t* n) const {
        *n = listed;
        std::memcpy(first, first_bad, sizeof(first));
        for (uint32_t k = 0; k < listed; ++k) std::memcpy(list[k], bad_list[k], sizeof(first));
    }

    double clock_mhz() { return median_of(mhz); }
};

// ---------------------------------------------------------------------------
// Chip-wide matrix-core sweep (kernel in mfmasweep.h)
// ---------------------------------------------------------------------------
//
// Every MFMA check above is one wave: one SIMD of one CU. The sweep runs one
// wave per SIMD on every CU, each through `outer` folds of 64 MFMAs on its
// own integer data, and the host recomputes every wave's checksum exactly, so
// a bad matrix core is named by (XCC, SE, SH, CU, SIMD). The timed launch
// also yields sustained TFLOP/s and the in-kernel clock. The figure comes
// from small-integer operands held in registers, which clock higher than a
// random-data GEMM: it is a health floor, not a GEMM benchmark.

#include "mfmasweep.h"

#define NA_MFMA_MAX_WORKGROUPS (1 << 20)
#define NA_MFMA_MAX_OUTER (1 << 22)  // ~2 s per resident wave: keeps a typo from hanging the node
// 8192 folds x 64 MFMAs x 16 cycles is ~3.5 ms per workgroup at 2.4 GHz, and
// the default grid puts four workgroups on each CU in turn: ~14 ms by
// arithmetic, 15.4 ms (bf16) / 16.1 ms (fp8) measured
// (profiles/mfma_sweep_mi355x.txt) — past the 10 ms from which the
// in-kernel clock estimate is reliable.
#define NA_MFMA_DEFAULT_OUTER 8192

// S(n) = sum_{j<n} q^j mod 2^64 by binary expansion of n.
static uint64_t ms_geometric_sum(uint64_t q, uint64_t n) {
    uint64_t s = 0, qk = 1;  // s = S(k), qk = q^k for the bits of n consumed so far
    for (int bit = 63; bit >= 0; --bit) {
        s *= 1 + qk;
        qk *= qk;
        if ((n >> bit) & 1) {
            s = s * q + 1;
            qk *= q;
        }
    }
    return s;
}

// sum over the wave's 64 lanes of P = d0 G^3 + d1 G^2 + d2 G + d3, where
// d_i = D[(l>>4)*4+i][l&15] and D = (sum_t A_t)(sum_t B_t) over k_len.
static uint64_t ms_wave_p_sum(uint64_t base, uint64_t wave, int k_len) {
    int sa[16][MS_MAX_K], sb[16][MS_MAX_K];
    for (int r = 0; r < 16; ++r) {
        for (int k = 0; k < k_len; ++k) {
            sa[r][k] = sb[r][k] = 0;
            for (int t = 0; t < MS_FRAGS; ++t) {
                sa[r][k] += ms_value(base, wave, 0, t, r, k, k_len);
                sb[r][k] += ms_value(base, wave, 1, t, r, k, k_len);
            }
        }
    }
    uint64_t sum = 0;
    for (int l = 0; l < 64; ++l) {
        uint64_t p = 0;
        for (int i = 0; i < 4; ++i) {
            int row = (l >> 4) * 4 + i, col = l & 15, d = 0;
            for (int k = 0; k < k_len; ++k) d += sa[row][k] * sb[col][k];
            p = p * MS_G + (uint64_t)(int64_t)d;
        }
        sum += p;
    }
    return sum;
}

// The sweep comes in two families that share everything below: the
// na_mfma_sweep* entry points on the non-scaled K = 32 instructions and the
// na_mx_sweep* ones on the block-scaled K = 128 instruction. A family's
// public code c (dtype or format, 0 or 1) is kernel variant `first` + c.
struct ms_family {
    const char* prefix;  // opens the argument errors
    const char* label;   // opens the verdict
    const char* codes;   // the two public codes, for the argument error
    int first, k_len;
};
static const ms_family ms_mfma = {"na_mfma_sweep", "mfma sweep", "dtype 0 (bf16) or 1 (fp8)",
                                  MS_BF16, 32};
static const ms_family ms_mx = {"na_mx_sweep", "mx sweep", "format 0 (fp4) or 1 (fp6)", MS_FP4,
                                MS_MAX_K};

// Pure host code. All folds produce the same D, so the per-lane recurrence
// c = c G + d_i collapses to c = P S(outer), S(n) = sum_{j<n} G^{4j}, and the
// wave checksum to S(outer) * sum_l P_l.
static int ms_expected(const ms_family& fam, unsigned long long seed, unsigned long long wave,
                       int outer, uint64_t* checksum) {
    if (outer < 1 || checksum == nullptr)
        return arg_error("%s_expected: need outer >= 1 (got %d) and a result pointer", fam.prefix,
                         outer);
    const uint64_t g2 = MS_G * MS_G;
    *checksum = ms_geometric_sum(g2 * g2, (uint64_t)outer) *
                ms_wave_p_sum(seed * MS_G, wave, fam.k_len);
    return NA_OK;
}

// One launch of `workgroups` x 4 waves, HIP-event timed; out receives the
// 4 * workgroups records. Argument errors are detected before any HIP call.
static int ms_run(const ms_family& fam, int dev, int code, int workgroups, int outer,
                  unsigned long long seed, na_mfma_record* out, long long n_out, double* ms) {
    if ((code != 0 && code != 1) || workgroups < 1 || workgroups > NA_MFMA_MAX_WORKGROUPS ||
        outer < 1 || outer > NA_MFMA_MAX_OUTER || out == nullptr ||
        n_out < (long long)workgroups * MS_WAVES_PER_WG)
        return arg_error("%s_run: need %s (got %d), workgroups in 1..%d (got %d), outer in 1..%d "
                         "(got %d) and room for 4 records per workgroup (out %p, n_out %lld)",
                         fam.prefix, fam.codes, code, NA_MFMA_MAX_WORKGROUPS, workgroups,
                         NA_MFMA_MAX_OUTER, outer, (void*)out, n_out);
    size_t lds_bytes = 0;
    int rc = sweep_lds_bytes(dev, &lds_bytes);
    if (rc != NA_OK) return rc;
    static void (*const kernels[MS_DTYPES])(na_mfma_record*, mt_u64, int) = {
        mfma_sweep_kernel<MS_BF16>, mfma_sweep_kernel<MS_FP8>, mfma_sweep_kernel<MS_FP4>,
        mfma_sweep_kernel<MS_FP6>};
    const size_t n = (size_t)workgroups * MS_WAVES_PER_WG;
    return sweep_launch(dev, n, out, ms, [&](na_mfma_record* records) {
        kernels[fam.first + code]<<<dim3((unsigned)workgroups), dim3(MS_BLOCK), lds_bytes>>>(
            records, seed * MS_G, outer);
    });
}

// The verdict over n per-wave records, for the two matrix-core families and
// for each role of the load sweep: record i is wave i and want(i) its
// checksum. A wave is bad when its checksum is not that or it does not carry
// its own index; the waves of a role that did not run (`ran` false: the load
// sweep's, when switched off) are bad unless their records are all zero, and
// are left out of the census. Fills *res.
template <typename WANT>
static void ms_tally(const na_mfma_record* recs, long long n, bool ran, na_mfma_sweep_result* res,
                     WANT want) {
    static const na_mfma_record none = {};
    std::memset(res, 0, sizeof(*res));
    res->waves = (uint64_t)n;
    res->first_bad_wave = UINT64_MAX;
    sweep_census census;
    for (long long i = 0; i < n; ++i) {
        const na_mfma_record& r = recs[i];
        if (ran) census.see(r, r.simd);
        if (ran ? r.checksum == want(i) && r.wave == (uint64_t)i
                : std::memcmp(&r, &none, sizeof(r)) == 0)
            continue;
        res->bad_waves++;
        if (res->first_bad_wave == UINT64_MAX) res->first_bad_wave = (uint64_t)i;
        census.mark_bad(r, r.simd);
    }
    res->units_seen = census.cus_seen;
    res->bad_units = census.bad_cus;
    res->clock_mhz = census.clock_mhz();
    census.bad_units(res->first_bad_unit, res->bad_list, &res->listed);
}

// Pure host code: record i is wave i. A wave is bad when its checksum is
// not the expected one or it does not carry its own index. Returns
// NA_ERR_VERIFY on any bad wave; *res is filled either way.
static int ms_verify(const ms_family& fam, const na_mfma_record* recs, long long n, int outer,
                     unsigned long long seed, na_mfma_sweep_result* res) {
    if (recs == nullptr || n < 1 || outer < 1 || res == nullptr)
        return arg_error("%s_verify: need records, n >= 1 (got %lld), outer >= 1 (got %d) and a "
                         "result pointer",
                         fam.prefix, n, outer);
    const uint64_t base = seed * MS_G, g2 = MS_G * MS_G;
    const uint64_t s = ms_geometric_sum(g2 * g2, (uint64_t)outer);
    ms_tally(recs, n, true, res, [&](long long i) {
        return s * ms_wave_p_sum(base, (uint64_t)i, fam.k_len);
    });
    if (res->bad_waves == 0) return NA_OK;
    const uint32_t* u = res->first_bad_unit;
    return na_error(NA_ERR_VERIFY,
                    "%s: %llu of %llu waves wrong on %llu CU(s), first wave %llu on "
                    "xcc%u.se%u.sh%u.cu%u.simd%u",
                    fam.label, (unsigned long long)res->bad_waves, (unsigned long long)res->waves,
                    (unsigned long long)res->bad_units, (unsigned long long)res->first_bad_wave,
                    u[0], u[1], u[2], u[3], u[4]);
}

// Whole sweep: one untimed warm-up launch, the timed launch, the verify.
// workgroups 0 = 4 per CU, outer 0 = NA_MFMA_DEFAULT_OUTER. *tflops counts
// 64 MFMAs of 512 K FLOP (16384, or 65536 for the MX family) per wave and
// fold over the event time.
static int ms_sweep(const ms_family& fam, int dev, int code, int workgroups, int outer,
                    unsigned long long seed, na_mfma_sweep_result* res, double* tflops) {
    if (res == nullptr || workgroups < 0 || workgroups > NA_MFMA_MAX_WORKGROUPS || outer < 0)
        return arg_error("%s: need workgroups in 0..%d (got %d), outer >= 0 (got %d) and a result "
                         "pointer",
                         fam.prefix, NA_MFMA_MAX_WORKGROUPS, workgroups, outer);
    int rc = sweep_defaults(dev, &workgroups, &outer, NA_MFMA_DEFAULT_OUTER);
    if (rc != NA_OK) return rc;
    std::vector<na_mfma_record> recs((size_t)workgroups * MS_WAVES_PER_WG);
    double ms = 0.0;
    rc = sweep_twice([&] {
        return ms_run(fam, dev, code, workgroups, outer, seed, recs.data(),
                      (long long)recs.size(), &ms);
    });
    if (rc != NA_OK) return rc;
    if (tflops)
        *tflops = (double)recs.size() * outer * MS_MFMA_PER_FOLD * MS_FLOP_PER_MFMA_K * fam.k_len /
                  (ms * 1e9);
    return ms_verify(fam, recs.data(), (long long)recs.size(), outer, seed, res);
}

extern "C" int na_mfma_sweep_expected(unsigned long long seed, unsigned long long wave, int outer,
                                      uint64_t* checksum) {
    return ms_expected(ms_mfma, seed, wave, outer, checksum);
}
extern "C" int na_mfma_sweep_run(int dev, int dtype, int workgroups, int outer,
                                 unsigned long long seed, na_mfma_record* out, long long n_out,
                                 double* ms) {
    return ms_run(ms_mfma, dev, dtype, workgroups, outer, seed, out, n_out, ms);
}
extern "C" int na_mfma_sweep_verify(const na_mfma_record* recs, long long n, int outer,
                                    unsigned long long seed, na_mfma_sweep_result* res) {
    return ms_verify(ms_mfma, recs, n, outer, seed, res);
}
extern "C" int na_mfma_sweep(int dev, int dtype, int workgroups, int outer,
                             unsigned long long seed, na_mfma_sweep_result* res, double* tflops) {
    return ms_sweep(ms_mfma, dev, dtype, workgroups, outer, seed, res, tflops);
}

// The same four on v_mfma_scale_f32_16x16x128_f8f6f4 at scales of 1.0:
// format 0 = fp4 (E2M1), 1 = fp6 (E2M3), and 65536 FLOP per MFMA. Both
// formats give the same checksums.
extern "C" int na_mx_sweep_expected(unsigned long long seed, unsigned long long wave, int outer,
                                    uint64_t* checksum) {
    return ms_expected(ms_mx, seed, wave, outer, checksum);
}
extern "C" int na_mx_sweep_run(int dev, int format, int workgroups, int outer,
                               unsigned long long seed, na_mfma_record* out, long long n_out,
                               double* ms) {
    return ms_run(ms_mx, dev, format, workgroups, outer, seed, out, n_out, ms);
}
extern "C" int na_mx_sweep_verify(const na_mfma_record* recs, long long n, int outer,
                                  unsigned long long seed, na_mfma_sweep_result* res) {
    return ms_verify(ms_mx, recs, n, outer, seed, res);
}
extern "C" int na_mx_sweep(int dev, int format, int workgroups, int outer,
                           unsigned long long seed, na_mfma_sweep_result* res, double* tflops) {
    return ms_sweep(ms_mx, dev, format, workgroups, outer, seed, res, tflops);
}

// ---------------------------------------------------------------------------
// Chip-wide LDS sweep (kernel and specification in ldssweep.h)
// ---------------------------------------------------------------------------
//
// na_lds_selftest above says "N mismatched words" of 32-bit accesses. The
// sweep runs one workgroup at a time on every CU through every LDS access
// path (32/128-bit, LDS-DMA at three widths, transposed read, atomics) and a
// timed read stream, and the host recomputes each workgroup's phase checksums
// exactly, so a bad LDS is named by (XCC, SE, SH, CU) and phase.

#include "ldssweep.h"

#define NA_LDS_MAX_WORKGROUPS (1 << 20)
// A pass over 160 KiB is 640 clocks at the LDS's 256 B/clk, 0.27 us at
// 2.4 GHz: 2^22 passes hold a CU for ~1.1 s at full rate, ~2 s at the half
// rate a sick CU might run at — NA_MFMA_MAX_OUTER's bound, which keeps a typo
// from hanging the node.
#define NA_LDS_MAX_ITERS (1 << 22)
// 12288 passes x 0.27 us is 3.3 ms per workgroup at full rate, and the
// default grid puts four workgroups on each CU in turn: at least 13 ms by
// arithmetic; measured 17.4 ms of stream phase per CU in an 18.3 ms launch
// (profiles/lds_sweep_mi355x.txt: the loop reaches 195 B/clk) — past the
// 10 ms from which the in-kernel clock estimate is reliable (see
// NA_MFMA_DEFAULT_OUTER).
#define NA_LDS_DEFAULT_ITERS 12288

static const char* const ls_phase_names[LS_PHASES] = {"b32",   "b128", "dma16",  "dma4",
                                                      "dma12", "tr16", "atomic", "stream"};

// Per 1 KiB chunk of each pattern, the sums the checksums are linear in.
// They do not depend on the workgroup, whose rotation only selects which
// chunk's sums enter at which step: computed once per (seed, lds_bytes), they
// make the reference of a workgroup a few hundred multiplications.
struct ls_sums {
    uint32_t C;
    std::vector<uint64_t> s32[2], lo[2], hi[2];  // b32 and b128 at both polarities
    std::vector<uint64_t> dma_lo, dma_hi, dma_w2, dma_w3, tr, atomic;
    uint64_t stream_total;

    static void words(uint64_t base, int pat, uint32_t pol, uint32_t chunk, uint32_t* w) {
        for (uint32_t i = 0; i < LS_CHUNK_WORDS; ++i)
            w[i] = ls_pat(base, pat, chunk * LS_CHUNK_WORDS + i) ^ pol;
    }
    static uint64_t sum32(const uint32_t* w) {
        uint64_t s = 0;
        for (uint32_t i = 0; i < LS_CHUNK_WORDS; ++i) s += w[i];
        return s;
    }
    static void sum128(const uint32_t* w, uint64_t* lo, uint64_t* hi) {
        *lo = *hi = 0;
        for (uint32_t i = 0; i < LS_CHUNK_WORDS; i += 4) {
            *lo += (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
            *hi += (uint64_t)w[i + 2] | ((uint64_t)w[i + 3] << 32);
        }
    }

    ls_sums(uint64_t base, uint32_t lds_bytes) : C(lds_bytes / 1024), stream_total(0) {
        uint32_t w[LS_CHUNK_WORDS];
        for (int p = 0; p < 2; ++p) s32[p].resize(C), lo[p].resize(C), hi[p].resize(C);
        dma_lo.resize(C), dma_hi.resize(C), dma_w2.resize(C), dma_w3.resize(C);
        tr.resize(C), atomic.resize(C);
        for (uint32_t c = 0; c < C; ++c) {
            for (int p = 0; p < 2; ++p) {
                words(base, LS_PAT_B32, p ? ~0u : 0u, c, w);
                s32[p][c] = sum32(w);
                words(base, LS_PAT_B128, p ? ~0u : 0u, c, w);
                sum128(w, &lo[p][c], &hi[p][c]);
            }
            words(base, LS_PAT_DMA, 0, c, w);
            sum128(w, &dma_lo[c], &dma_hi[c]);
            dma_w2[c] = dma_w3[c] = 0;
            for (uint32_t i = 0; i < LS_CHUNK_WORDS; i += 4) dma_w2[c] += w[i + 2], dma_w3[c] += w[i + 3];
            // a tile is 32 words, row q its words 8q..8q+7; column i of row
            // q lands in bits 16q.. of lane i's value
            words(base, LS_PAT_TR16, 0, c, w);
            tr[c] = 0;
            for (uint32_t i = 0; i < LS_CHUNK_WORDS; ++i)
                tr[c] += ((uint64_t)(w[i] & 0xFFFF) + (uint64_t)(w[i] >> 16)) << (16 * ((i >> 3) & 3));
            words(base, LS_PAT_ATOMIC, 0, c, w);
            atomic[c] = 0;
            for (uint32_t i = 0; i < LS_CHUNK_WORDS; ++i) atomic[c] += (uint32_t)(w[i] + (w[i] >> 16));
            words(base, LS_PAT_STREAM, 0, c, w);
            uint64_t l, h;
            sum128(w, &l, &h);
            stream_total += l + h;
        }
    }

    // What 256 threads folding c = c*G + value leave in sum: Horner over the
    // per-step sums of the values.
    static void fold(uint64_t& c, uint64_t step_sum) { c = c * MS_G + step_sum; }

    void fold32(uint64_t& c, const std::vector<uint64_t>& s, uint32_t rot, uint32_t chunks) const {
        for (uint32_t k = 0; k < chunks; ++k) fold(c, s[(k + rot) % C]);
    }
    void fold128(uint64_t& c, const std::vector<uint64_t>& l, const std::vector<uint64_t>& h,
                 uint32_t rot) const {
        for (uint32_t k = 0; k < C / 4; ++k) {
            uint64_t sl = 0, sh = 0;
            for (uint32_t m = 0; m < 4; ++m) sl += l[(4 * k + m + rot) % C], sh += h[(4 * k + m + rot) % C];
            fold(c, sl);
            fold(c, sh);
        }
    }

    void expected(uint64_t workgroup, int iters, uint64_t* out) const {
        const uint32_t rot = (uint32_t)(workgroup % C);
        for (int p = 0; p < LS_PHASES; ++p) out[p] = 0;
        for (int p = 0; p < 2; ++p) fold32(out[LS_B32], s32[p], rot, C);
        for (int p = 0; p < 2; ++p) fold128(out[LS_B128], lo[p], hi[p], rot);
        fold128(out[LS_DMA16], dma_lo, dma_hi, rot);
        fold128(out[LS_DMA4], dma_lo, dma_hi, (rot + 1) % C);
        // dma12 renews three words of every vector; the fourth is still dma4's
        for (uint32_t k = 0; k < C / 4; ++k) {
            uint64_t sl = 0, sh = 0;
            for (uint32_t m = 0; m < 4; ++m) {
                const uint32_t c12 = (4 * k + m + rot + 2) % C, c4 = (4 * k + m + rot + 1) % C;
                sl += dma_lo[c12];
                sh += dma_w2[c12] + (dma_w3[c4] << 32);
            }
            fold(out[LS_DMA12], sl);
            fold(out[LS_DMA12], sh);
        }
        for (uint32_t k = 0; k < C / 2; ++k)
            fold(out[LS_TR16], tr[(2 * k + rot) % C] + tr[(2 * k + 1 + rot) % C]);
        fold32(out[LS_ATOMIC], atomic, rot, C);
        out[LS_STREAM] = (uint64_t)iters * stream_total;
    }
};

static bool ls_bytes_ok(long long lds_bytes) {
    return lds_bytes >= LS_GRANULE && lds_bytes <= LS_MAX_BYTES && lds_bytes % LS_GRANULE == 0;
}

// The per-workgroup LDS allocation the sweep launches with and, at
// lds_bytes 0, tests: sharedMemPerBlock, capped at 160 KiB and rounded down
// to the sweep's granule.
extern "C" int na_lds_sweep_allocation(int dev, long long* bytes) {
    if (bytes == nullptr) return arg_error("na_lds_sweep_allocation: need a result pointer");
    size_t alloc = 0;
    int rc = sweep_lds_bytes(dev, &alloc);
    if (rc == NA_OK) *bytes = (long long)(alloc / LS_GRANULE * LS_GRANULE);
    return rc;
}

// Pure host code: the LS_PHASES checksums of one workgroup, in the order of
// the LS_* codes. lds_bytes is explicit here (a multiple of 4096 in
// 4096..160 KiB); n is the room in `checksums`.
extern "C" int na_lds_sweep_expected(unsigned long long seed, unsigned long long workgroup,
                                     long long lds_bytes, int iters, uint64_t* checksums, int n) {
    if (!ls_bytes_ok(lds_bytes) || iters < 1 || checksums == nullptr || n < LS_PHASES)
        return arg_error("na_lds_sweep_expected: need lds_bytes a multiple of %d in %d..%d (got "
                         "%lld), iters >= 1 (got %d) and room for %d checksums (n %d)",
                         LS_GRANULE, LS_GRANULE, LS_MAX_BYTES, lds_bytes, iters, LS_PHASES, n);
    ls_sums(seed * MS_G, (uint32_t)lds_bytes).expected(workgroup, iters, checksums);
    return NA_OK;
}

// One launch of `workgroups` workgroups, HIP-event timed; out receives one
// record per workgroup. lds_bytes 0 = the whole allocation. Argument errors
// are detected before any HIP call.
extern "C" int na_lds_sweep_run(int dev, int workgroups, long long lds_bytes, int iters,
                                unsigned long long seed, na_lds_record* out, long long n_out,
                                double* ms) {
    if (workgroups < 1 || workgroups > NA_LDS_MAX_WORKGROUPS ||
        (lds_bytes != 0 && !ls_bytes_ok(lds_bytes)) || iters < 1 || iters > NA_LDS_MAX_ITERS ||
        out == nullptr || n_out < (long long)workgroups)
        return arg_error("na_lds_sweep_run: need workgroups in 1..%d (got %d), lds_bytes 0 or a "
                         "multiple of %d up to %d (got %lld), iters in 1..%d (got %d) and room "
                         "for a record per workgroup (out %p, n_out %lld)",
                         NA_LDS_MAX_WORKGROUPS, workgroups, LS_GRANULE, LS_MAX_BYTES, lds_bytes,
                         NA_LDS_MAX_ITERS, iters, (void*)out, n_out);
    HIP_CHECK(hipSetDevice(dev));  // for the upload below, ahead of sweep_launch
    long long alloc = 0;
    int rc = na_lds_sweep_allocation(dev, &alloc);
    if (rc != NA_OK) return rc;
    if (lds_bytes == 0) lds_bytes = alloc;
    if (lds_bytes > alloc || alloc < LS_GRANULE)
        return arg_error("na_lds_sweep_run: lds_bytes %lld exceeds the device's %lld-byte "
                         "per-workgroup LDS allocation",
                         lds_bytes, alloc);
    // the dma phases' source: pattern LS_PAT_DMA
    const uint32_t W = (uint32_t)lds_bytes / 4;
    const mt_u64 base = seed * MS_G;
    std::vector<uint32_t> pattern(W);
    for (uint32_t j = 0; j < W; ++j) pattern[j] = ls_pat(base, LS_PAT_DMA, j);
    dev_buf<uint32_t> src;
    HIP_CHECK(src.alloc(pattern.size()));
    HIP_CHECK(hipMemcpy(src.p, pattern.data(), pattern.size() * sizeof(uint32_t),
                        hipMemcpyHostToDevice));
    return sweep_launch(dev, (size_t)workgroups, out, ms, [&](na_lds_record* records) {
        // the whole allocation whatever lds_bytes is: one workgroup per CU
        lds_sweep_kernel<<<dim3((unsigned)workgroups), dim3(LS_BLOCK), (size_t)alloc>>>(
            records, src.p, base, (uint32_t)lds_bytes, iters);
    });
}

// Pure host code: record i is workgroup i. A workgroup is bad when a phase
// checksum is not the expected one, when it does not carry its own index, or
// when its in-kernel count of bad words is not zero. Returns NA_ERR_VERIFY on
// any bad workgroup; *res is filled either way.
extern "C" int na_lds_sweep_verify(const na_lds_record* recs, long long n, long long lds_bytes,
                                   int iters, unsigned long long seed, na_lds_sweep_result* res) {
    if (recs == nullptr || n < 1 || !ls_bytes_ok(lds_bytes) || iters < 1 || res == nullptr)
        return arg_error("na_lds_sweep_verify: need records, n >= 1 (got %lld), lds_bytes a "
                         "multiple of %d in %d..%d (got %lld), iters >= 1 (got %d) and a result "
                         "pointer",
                         n, LS_GRANULE, LS_GRANULE, LS_MAX_BYTES, lds_bytes, iters);
    std::memset(res, 0, sizeof(*res));
    res->workgroups = (uint64_t)n;
    res->first_bad_workgroup = res->first_bad_offset = UINT64_MAX;
    res->first_bad_phase = ~0u;
    const ls_sums sums(seed * MS_G, (uint32_t)lds_bytes);
    // every C-th workgroup shares a rotation, hence its checksums
    std::vector<uint64_t> want((size_t)sums.C * LS_PHASES);
    for (uint32_t r = 0; r < sums.C; ++r) sums.expected(r, iters, &want[(size_t)r * LS_PHASES]);
    sweep_census census;
    std::vector<double> rate;
    for (long long i = 0; i < n; ++i) {
        const na_lds_record& r = recs[i];
        census.see(r);
        if (r.cycles) rate.push_back((double)iters * (double)lds_bytes / (double)r.cycles);
        const uint64_t* w = &want[(size_t)(i % sums.C) * LS_PHASES];
        uint32_t phase = 0;
        while (phase < LS_PHASES && r.checksum[phase] == w[phase]) ++phase;
        if (phase == LS_PHASES && r.bad_words != 0)
            phase = r.bad_phase < LS_PHASES ? r.bad_phase : (uint32_t)LS_B32;
        if (phase == LS_PHASES && r.workgroup == (uint64_t)i) continue;
        // `phase` failed; LS_PHASES: the record is only in the wrong place
        res->bad_workgroups++;
        census.mark_bad(r);
        if (res->first_bad_workgroup == UINT64_MAX) {
            res->first_bad_workgroup = (uint64_t)i;
            res->first_bad_phase = phase;
            if (r.bad_words != 0 && r.bad_phase == phase) {
                res->bad_words = r.bad_words;
                res->first_bad_offset = r.first_bad_offset;
                res->xor_mask = r.xor_mask;
            }
        }
    }
    res->units_seen = census.cus_seen;
    res->bad_units = census.bad_cus;
    res->clock_mhz = census.clock_mhz();
    census.bad_units(res->first_bad_unit, res->bad_list, &res->listed);
    if (!rate.empty()) {
        res->min_bytes_per_clk = *std::min_element(rate.begin(), rate.end());
        res->max_bytes_per_clk = *std::max_element(rate.begin(), rate.end());
    }
    res->median_bytes_per_clk = median_of(rate);
    if (res->bad_workgroups == 0) return NA_OK;
    const uint32_t* u = res->first_bad_unit;
    char where[128] = "";
    if (res->first_bad_offset != UINT64_MAX)
        std::snprintf(where, sizeof(where),
                      ", %llu bad words, first at LDS offset 0x%llx (bank %llu), failing bits "
                      "0x%08llx",
                      (unsigned long long)res->bad_words,
                      (unsigned long long)res->first_bad_offset,
                      (unsigned long long)(res->first_bad_offset / 4 % 64),
                      (unsigned long long)res->xor_mask);
    return na_error(
        NA_ERR_VERIFY,
        "lds sweep: %llu of %llu workgroups wrong on %llu CU(s), first workgroup %llu in phase %s "
        "on xcc%u.se%u.sh%u.cu%u%s",
        (unsigned long long)res->bad_workgroups, (unsigned long long)res->workgroups,
        (unsigned long long)res->bad_units, (unsigned long long)res->first_bad_workgroup,
        res->first_bad_phase < LS_PHASES ? ls_phase_names[res->first_bad_phase] : "index", u[0],
        u[1], u[2], u[3], where);
}

// Whole sweep: one untimed warm-up launch, the timed launch, the verify.
// workgroups 0 = 4 per CU, lds_bytes 0 = the whole allocation, iters 0 =
// NA_LDS_DEFAULT_ITERS. *gbs is the chip-wide rate of the stream phase from
// the in-kernel stamps alone, not the launch's event time (which includes
// the other phases):
//   gbs = median_bytes_per_clk x units_seen x clock_mhz / 1000
// i.e. the median CU's bytes per shader clock, on every CU that took part, at
// the median measured clock.
extern "C" int na_lds_sweep(int dev, int workgroups, long long lds_bytes, int iters,
                            unsigned long long seed, na_lds_sweep_result* res, double* gbs) {
    if (res == nullptr || workgroups < 0 || workgroups > NA_LDS_MAX_WORKGROUPS ||
        (lds_bytes != 0 && !ls_bytes_ok(lds_bytes)) || iters < 0 || iters > NA_LDS_MAX_ITERS)
        return arg_error("na_lds_sweep: need workgroups in 0..%d (got %d), lds_bytes 0 or a "
                         "multiple of %d up to %d (got %lld), iters in 0..%d (got %d) and a "
                         "result pointer",
                         NA_LDS_MAX_WORKGROUPS, workgroups, LS_GRANULE, LS_MAX_BYTES, lds_bytes,
                         NA_LDS_MAX_ITERS, iters);
    int rc = sweep_defaults(dev, &workgroups, &iters, NA_LDS_DEFAULT_ITERS);
    if (rc == NA_OK && lds_bytes == 0) rc = na_lds_sweep_allocation(dev, &lds_bytes);
    if (rc != NA_OK) return rc;
    std::vector<na_lds_record> recs((size_t)workgroups);
    rc = sweep_twice([&] {
        return na_lds_sweep_run(dev, workgroups, lds_bytes, iters, seed, recs.data(),
                                (long long)recs.size(), nullptr);
    });
    if (rc != NA_OK) return rc;
    rc = na_lds_sweep_verify(recs.data(), (long long)recs.size(), lds_bytes, iters, seed, res);
    if (gbs && (rc == NA_OK || rc == NA_ERR_VERIFY))
        *gbs = res->median_bytes_per_clk * (double)res->units_seen * res->clock_mhz / 1000.0;
    return rc;
}

// ---------------------------------------------------------------------------
// Chip-wide cache sweep (kernels and specification in cachesweep.h)
// ---------------------------------------------------------------------------
//
// The HBM memtest streams past the caches and the other sweeps stay inside a
// CU. This one gives every workgroup a slice of device memory small enough to
// stay in cache and runs it, one workgroup at a time on every CU, through the
// L1, the L2, write-through and refill, global atomics, the scalar data cache
// and a timed read stream from the L2; a second launch reads each slice from
// another workgroup, normally on another XCD. The host recomputes each
// workgroup's phase checksums exactly, so a bad cache is named by (XCC, SE,
// SH, CU) and phase. Records and result are the LDS sweep's structs.

#include "cachesweep.h"

// 64 KiB per workgroup: with the 32 CUs of an XCD holding one workgroup each
// that is 2 MiB live per XCD, half of its L2, and twice a CU's L1.
#define NA_CACHE_DEFAULT_BYTES (64 * 1024)
#define NA_CACHE_MAX_TOTAL_BYTES (1LL << 32)
// A pass over the 64 KiB slice, eight sc1 loads in flight per thread, takes
// about 1.2 us per workgroup (measured: 23 B/clk and CU, latency-bound), and
// the default grid puts four workgroups on each CU in turn: a launch pair
// measured 0.7 ms + 5.1 us per pass, so 3072 passes make it about 16 ms, the
// other sweeps' length (profiles/cache_sweep_mi355x.txt) and past the 10 ms
// from which the in-kernel clock estimate is reliable (see
// NA_MFMA_DEFAULT_OUTER).
#define NA_CACHE_DEFAULT_ITERS 3072

static const char* const cs_phase_names[CS_PHASES] = {"l1",     "l2",     "wt",   "atomic",
                                                      "scalar", "stream", "xread"};

static bool cs_bytes_ok(long long slice_bytes) {
    return slice_bytes >= CS_GRANULE && slice_bytes <= CS_MAX_BYTES &&
           slice_bytes % CS_GRANULE == 0;
}

// The reference of one (seed, slice_bytes). The checksums are linear in the
// sums, over the 256 threads, of what each step reads: 256 threads folding
// c = c*G + value leave in their sum the Horner form over the per-step sums.
struct cs_ref {
    uint64_t base;
    uint32_t W, steps;
    uint64_t table_fold[CS_TABLE_STARTS];  // a wave's fold of the table, per start

    cs_ref(uint64_t base_, uint32_t slice_bytes)
        : base(base_), W(slice_bytes / 4), steps(slice_bytes / CS_GRANULE) {
        std::vector<uint32_t> table(CS_TABLE_WORDS);
        for (uint32_t j = 0; j < CS_TABLE_WORDS; ++j) table[j] = cs_pat(base, CS_SCALAR, j);
        for (uint32_t s = 0; s < CS_TABLE_STARTS; ++s) {
            uint64_t c = 0;
            for (uint32_t j = 0; j < CS_TABLE_WORDS; ++j)
                c = c * MS_G + table[(256 * s + j) % CS_TABLE_WORDS];
            table_fold[s] = c;
        }
    }

    // The sums of lo and of hi over the 256 vectors of each of the leading n
    // steps of the slice that starts at global word g0, under pattern pat,
    // each word through f.
    template <typename F>
    void step_sums(int pat, uint64_t g0, uint32_t n, F f, std::vector<uint64_t>& lo,
                   std::vector<uint64_t>& hi) const {
        lo.assign(n, 0), hi.assign(n, 0);
        for (uint32_t k = 0; k < n; ++k)
            for (uint32_t u = 0; u < 256; ++u) {
                const uint64_t g = g0 + 4 * (uint64_t)(256 * k + u);
                const uint64_t w0 = f(cs_pat(base, pat, g)), w1 = f(cs_pat(base, pat, g + 1)),
                               w2 = f(cs_pat(base, pat, g + 2)), w3 = f(cs_pat(base, pat, g + 3));
                lo[k] += w0 | (w1 << 32);
                hi[k] += w2 | (w3 << 32);
            }
    }

    // One pass over the steps; inverted: every word complemented, and the sum
    // of 256 values ~x = -1 - x is -256 - their sum.
    static void fold_pass(uint64_t& c, const std::vector<uint64_t>& lo,
                          const std::vector<uint64_t>& hi, bool inverted) {
        for (size_t k = 0; k < lo.size(); ++k) {
            c = c * MS_G + (inverted ? 0 - 256 - lo[k] : lo[k]);
            c = c * MS_G + (inverted ? 0 - 256 - hi[k] : hi[k]);
        }
    }

    // The CS_PHASES checksums of workgroup w of `workgroups`, both launches'.
    void expected(uint64_t w, uint64_t workgroups, int iters, uint64_t* out) const {
        const auto plain = [](uint32_t x) { return x; };
        const uint64_t g0 = w * W;
        std::vector<uint64_t> lo, hi;
        for (int p = 0; p < CS_PHASES; ++p) out[p] = 0;
        step_sums(CS_L1, g0, std::min<uint32_t>(steps, CS_L1_BYTES / CS_GRANULE), plain, lo, hi);
        for (int pol = 0; pol < 2; ++pol)
            for (int pass = 0; pass < CS_L1_PASSES; ++pass) fold_pass(out[CS_L1], lo, hi, pol);
        step_sums(CS_L2, g0, steps, plain, lo, hi);
        for (int pol = 0; pol < 2; ++pol)
            for (int pass = 0; pass < CS_L2_PASSES; ++pass) fold_pass(out[CS_L2], lo, hi, pol);
        step_sums(CS_WT, g0, steps, plain, lo, hi);
        for (int pol = 0; pol < 2; ++pol) fold_pass(out[CS_WT], lo, hi, pol);
        step_sums(CS_ATOMIC, g0, steps, [](uint32_t a) { return (uint32_t)(a + (a >> 16)); }, lo,
                  hi);
        fold_pass(out[CS_ATOMIC], lo, hi, false);
        for (uint64_t v = 0; v < MS_WAVES_PER_WG; ++v)
            out[CS_SCALAR] += table_fold[(w + v) % CS_TABLE_STARTS];
        step_sums(CS_STREAM, g0, steps, plain, lo, hi);
        uint64_t total = 0;
        for (uint32_t k = 0; k < steps; ++k) total += lo[k] + hi[k];
        out[CS_STREAM] = (uint64_t)iters * total;
        // xread: the pattern-5 image of the neighbour's slice
        step_sums(CS_STREAM, (w + 1) % workgroups * W, steps, plain, lo, hi);
        fold_pass(out[CS_XREAD], lo, hi, false);
    }
};

// Pure host code: the CS_PHASES checksums of workgroup `workgroup` of
// `workgroups`, in the order of the CS_* codes: l1..stream are what its
// record of the first launch carries, xread what its record of the second
// does. n is the room in `checksums`.
extern "C" int na_cache_sweep_expected(unsigned long long seed, unsigned long long workgroup,
                                       unsigned long long workgroups, long long slice_bytes,
                                       int iters, uint64_t* checksums, int n) {
    if (!cs_bytes_ok(slice_bytes) || iters < 1 || workgroups < 1 || workgroup >= workgroups ||
        checksums == nullptr || n < CS_PHASES)
        return arg_error("na_cache_sweep_expected: need slice_bytes a multiple of %d in %d..%d "
                         "(got %lld), iters >= 1 (got %d), workgroup %llu below workgroups %llu "
                         "and room for %d checksums (n %d)",
                         CS_GRANULE, CS_GRANULE, CS_MAX_BYTES, slice_bytes, iters, workgroup,
                         workgroups, CS_PHASES, n);
    cs_ref(seed * MS_G, (uint32_t)slice_bytes).expected(workgroup, workgroups, iters, checksums);
    return NA_OK;
}

// Both launches of `workgroups` workgroups on one stream, HIP-event timed as
// a pair; out receives the first launch's records, then the second's.
// Argument errors are detected before any HIP call.
extern "C" int na_cache_sweep_run(int dev, int workgroups, long long slice_bytes, int iters,
                                  unsigned long long seed, na_lds_record* out, long long n_out,
                                  double* ms) {
    if (workgroups < 1 || workgroups > NA_LDS_MAX_WORKGROUPS || !cs_bytes_ok(slice_bytes) ||
        workgroups * slice_bytes > NA_CACHE_MAX_TOTAL_BYTES || iters < 1 ||
        iters > NA_LDS_MAX_ITERS || out == nullptr || n_out < 2 * (long long)workgroups)
        return arg_error("na_cache_sweep_run: need workgroups in 1..%d (got %d), slice_bytes a "
                         "multiple of %d up to %d (got %lld), at most %lld bytes in all, iters in "
                         "1..%d (got %d) and room for two records per workgroup (out %p, n_out "
                         "%lld)",
                         NA_LDS_MAX_WORKGROUPS, workgroups, CS_GRANULE, CS_MAX_BYTES, slice_bytes,
                         NA_CACHE_MAX_TOTAL_BYTES, NA_LDS_MAX_ITERS, iters, (void*)out, n_out);
    HIP_CHECK(hipSetDevice(dev));  // for the buffers below, ahead of sweep_launch
    size_t alloc = 0;
    int rc = sweep_lds_bytes(dev, &alloc);
    if (rc != NA_OK) return rc;
    const mt_u64 base = seed * MS_G;
    std::vector<uint32_t> pattern(CS_TABLE_WORDS);
    for (uint32_t j = 0; j < CS_TABLE_WORDS; ++j) pattern[j] = cs_pat(base, CS_SCALAR, j);
    dev_buf<uint32_t> table;
    HIP_CHECK(table.alloc(pattern.size()));
    HIP_CHECK(hipMemcpy(table.p, pattern.data(), pattern.size() * sizeof(uint32_t),
                        hipMemcpyHostToDevice));
    dev_buf<unsigned char> mem;
    HIP_CHECK(mem.alloc((size_t)workgroups * (size_t)slice_bytes));
    return sweep_launch(dev, 2 * (size_t)workgroups, out, ms, [&](na_lds_record* records) {
        // the whole LDS allocation: one workgroup per CU. The second launch
        // follows the first on the same (null) stream.
        const dim3 grid((unsigned)workgroups), block(CS_BLOCK);
        cache_sweep_kernel<<<grid, block, alloc>>>(records, mem.p, table.p, base,
                                                   (uint32_t)slice_bytes, iters);
        cache_xread_kernel<<<grid, block, alloc>>>(records + workgroups, mem.p, base,
                                                   (uint32_t)slice_bytes);
    });
}

// Pure host code: n records, record i being workgroup i mod (n/2) of launch
// i / (n/2). A record is bad when a checksum of its launch is not the
// expected one, when a checksum its launch does not compute is not 0 (the
// failing phase is that slot's; the unused eighth counts as the index), when
// it does not carry its own index, or when its in-kernel count of bad words
// is not zero. bad_workgroups counts the workgroups with a bad record in
// either launch. The census, the clock and the rates come from the first
// launch, whose stamps bracket the stream phase. Returns NA_ERR_VERIFY on any
// bad record; *res is filled either way.
extern "C" int na_cache_sweep_verify(const na_lds_record* recs, long long n,
                                     long long slice_bytes, int iters, unsigned long long seed,
                                     na_lds_sweep_result* res) {
    if (recs == nullptr || n < 2 || n % 2 != 0 || !cs_bytes_ok(slice_bytes) || iters < 1 ||
        res == nullptr)
        return arg_error("na_cache_sweep_verify: need records, an even n >= 2 (got %lld), "
                         "slice_bytes a multiple of %d in %d..%d (got %lld), iters >= 1 (got %d) "
                         "and a result pointer",
                         n, CS_GRANULE, CS_GRANULE, CS_MAX_BYTES, slice_bytes, iters);
    const long long wgs = n / 2;
    std::memset(res, 0, sizeof(*res));
    res->workgroups = (uint64_t)wgs;
    res->first_bad_workgroup = res->first_bad_offset = UINT64_MAX;
    res->first_bad_phase = ~0u;
    const cs_ref ref(seed * MS_G, (uint32_t)slice_bytes);
    sweep_census census;
    std::vector<double> rate;
    std::vector<bool> wg_bad((size_t)wgs);
    // the bad records of the phases an XCD's L2 serves: their XCC when they
    // share one (-1: none yet, -2: several), and their CUs
    int l2_xcc = -1;
    std::vector<uint32_t> l2_cus;
    long long first_bad_record = -1;
    // a workgroup's checksums serve its records of both launches
    std::vector<uint64_t> want((size_t)wgs * CS_PHASES);
    for (long long i = 0; i < n; ++i) {
        const na_lds_record& r = recs[i];
        const long long w = i % wgs;
        const bool second = i >= wgs;
        const uint64_t* wants = &want[(size_t)w * CS_PHASES];
        if (!second) {
            ref.expected((uint64_t)w, (uint64_t)wgs, iters, &want[(size_t)w * CS_PHASES]);
            census.see(r);
            if (r.cycles) rate.push_back((double)iters * (double)slice_bytes / (double)r.cycles);
        }
        // `phase` is the one that failed; CS_PHASES: the record is malformed
        // or only in the wrong place
        uint32_t phase = CS_PHASES;
        bool bad = false;
        for (uint32_t p = 0; p < NA_LDS_PHASES && !bad; ++p) {
            const bool computed = p < CS_PHASES && (p == CS_XREAD) == second;
            if (r.checksum[p] != (computed ? wants[p] : 0))
                bad = true, phase = std::min<uint32_t>(p, CS_PHASES);
        }
        if (!bad && r.bad_words != 0) {
            bad = true;
            phase = second ? (uint32_t)CS_XREAD
                           : r.bad_phase < CS_XREAD ? r.bad_phase : (uint32_t)CS_L1;
        }
        if (!bad && r.workgroup != (uint64_t)w) bad = true;  // phase stays CS_PHASES: the index
        if (!bad) continue;
        if (!wg_bad[(size_t)w]) wg_bad[(size_t)w] = true, res->bad_workgroups++;
        census.mark_bad(r);
        if (phase == CS_L2 || phase == CS_WT || phase == CS_ATOMIC || phase == CS_STREAM ||
            phase == CS_XREAD) {
            l2_xcc = l2_xcc == -1 || l2_xcc == (int)r.xcc ? (int)r.xcc : -2;
            const uint32_t key = ms_cu_key(r);
            if (std::find(l2_cus.begin(), l2_cus.end(), key) == l2_cus.end()) l2_cus.push_back(key);
        }
        if (first_bad_record < 0) {
            first_bad_record = i;
            res->first_bad_workgroup = (uint64_t)w;
            res->first_bad_phase = phase;
            if (r.bad_words != 0 && r.bad_phase == phase) {
                res->bad_words = r.bad_words;
                res->first_bad_offset = r.first_bad_offset;
                res->xor_mask = r.xor_mask;
            }
        }
    }
    res->units_seen = census.cus_seen;
    res->bad_units = census.bad_cus;
    res->clock_mhz = census.clock_mhz();
    census.bad_units(res->first_bad_unit, res->bad_list, &res->listed);
    if (!rate.empty()) {
        res->min_bytes_per_clk = *std::min_element(rate.begin(), rate.end());
        res->max_bytes_per_clk = *std::max_element(rate.begin(), rate.end());
    }
    res->median_bytes_per_clk = median_of(rate);
    if (first_bad_record < 0) return NA_OK;
    const uint32_t* u = res->first_bad_unit;
    char where[128] = "", writer[96] = "", l2[96] = "";
    if (res->first_bad_offset != UINT64_MAX)
        std::snprintf(where, sizeof(where),
                      ", %llu bad words, first at slice offset 0x%llx, failing bits 0x%08llx",
                      (unsigned long long)res->bad_words,
                      (unsigned long long)res->first_bad_offset,
                      (unsigned long long)res->xor_mask);
    if (res->first_bad_phase == CS_XREAD) {
        // who wrote what the first bad workgroup read
        const uint64_t from = (res->first_bad_workgroup + 1) % (uint64_t)wgs;
        const na_lds_record& a = recs[from];
        std::snprintf(writer, sizeof(writer), "; its slice was written by workgroup %llu on "
                      "xcc%u.se%u.sh%u.cu%u",
                      (unsigned long long)from, a.xcc, a.se, a.sh, a.cu);
    }
    if (l2_xcc >= 0 && l2_cus.size() >= 2)
        std::snprintf(l2, sizeof(l2), "; the %zu CUs that failed in a phase the L2 serves are all on "
                      "xcc%d: suspect its L2", l2_cus.size(), l2_xcc);
    return na_error(
        NA_ERR_VERIFY,
        "cache sweep: %llu of %llu workgroups wrong on %llu CU(s), first workgroup %llu in "
        "phase %s on xcc%u.se%u.sh%u.cu%u%s%s%s",
        (unsigned long long)res->bad_workgroups, (unsigned long long)res->workgroups,
        (unsigned long long)res->bad_units, (unsigned long long)res->first_bad_workgroup,
        res->first_bad_phase < CS_PHASES ? cs_phase_names[res->first_bad_phase] : "index", u[0],
        u[1], u[2], u[3], where, writer, l2);
}

// Whole sweep: one untimed warm-up pair of launches, the timed pair, the
// verify. workgroups 0 = 4 per CU, slice_bytes 0 = NA_CACHE_DEFAULT_BYTES,
// iters 0 = NA_CACHE_DEFAULT_ITERS. *gbs is the chip-wide rate of the stream
// phase from the in-kernel stamps alone, as na_lds_sweep computes its figure:
//   gbs = median_bytes_per_clk x units_seen x clock_mhz / 1000
extern "C" int na_cache_sweep(int dev, int workgroups, long long slice_bytes, int iters,
                              unsigned long long seed, na_lds_sweep_result* res, double* gbs) {
    if (res == nullptr || workgroups < 0 || workgroups > NA_LDS_MAX_WORKGROUPS ||
        (slice_bytes != 0 && !cs_bytes_ok(slice_bytes)) ||
        workgroups * slice_bytes > NA_CACHE_MAX_TOTAL_BYTES || iters < 0 ||
        iters > NA_LDS_MAX_ITERS)
        return arg_error("na_cache_sweep: need workgroups in 0..%d (got %d), slice_bytes 0 or a "
                         "multiple of %d up to %d (got %lld), at most %lld bytes in all, iters in "
                         "0..%d (got %d) and a result pointer",
                         NA_LDS_MAX_WORKGROUPS, workgroups, CS_GRANULE, CS_MAX_BYTES, slice_bytes,
                         NA_CACHE_MAX_TOTAL_BYTES, NA_LDS_MAX_ITERS, iters);
    int rc = sweep_defaults(dev, &workgroups, &iters, NA_CACHE_DEFAULT_ITERS);
    if (rc != NA_OK) return rc;
    if (slice_bytes == 0) slice_bytes = NA_CACHE_DEFAULT_BYTES;
    std::vector<na_lds_record> recs(2 * (size_t)workgroups);
    rc = sweep_twice([&] {
        return na_cache_sweep_run(dev, workgroups, slice_bytes, iters, seed, recs.data(),
                                  (long long)recs.size(), nullptr);
    });
    if (rc != NA_OK) return rc;
    rc = na_cache_sweep_verify(recs.data(), (long long)recs.size(), slice_bytes, iters, seed, res);
    if (gbs && (rc == NA_OK || rc == NA_ERR_VERIFY))
        *gbs = res->median_bytes_per_clk * (double)res->units_seen * res->clock_mhz / 1000.0;
    return rc;
}

// ---------------------------------------------------------------------------
// Chip-wide vector-unit sweep (kernel and specification in valusweep.h)
// ---------------------------------------------------------------------------
//
// na_fma_selftest above is one short f32 chain whose mismatches go into one
// counter. The sweep runs one wave per SIMD on every CU through a
// register-file pattern at both polarities, integer, f32, f64, packed,
// cross-lane and transcendental chains and a timed packed-f32 stream, and the
// host recomputes every exact checksum, so a bad SIMD is named by (XCC, SE,
// SH, CU, SIMD) and phase. The transcendental phase has no exact reference:
// there the records are compared with each other.

#include "valusweep.h"

#define NA_VALU_MAX_WORKGROUPS (1 << 20)
// Bits of a listed wave's phase mask above the VS_PHASES checksum bits: the
// record does not carry its own index (a missing or duplicated wave), or the
// four waves of its workgroup do not sit on four SIMDs of one CU.
#define NA_VALU_BAD_INDEX (1u << VS_PHASES)
#define NA_VALU_BAD_PLACEMENT (1u << (VS_PHASES + 1))
// 131072 rounds x 16 v_pk_fma_f32 at the measured 5 clocks per instruction is
// 10.5 M clocks per workgroup, ~4.5 ms, and the default grid puts four
// workgroups on each CU in turn: 18.8 ms per launch measured
// (profiles/valu_sweep_mi355x.txt) — past the 10 ms from which the in-kernel
// clock estimate is reliable (see NA_MFMA_DEFAULT_OUTER).
#define NA_VALU_DEFAULT_ITERS 131072

static const char* const vs_phase_names[VS_PHASES + 2] = {
    "rf", "rf_inv", "i32", "f32", "f64", "pk", "xlane", "trans", "stream", "index", "placement"};

// Source slot of destination slot i under cross-lane move n of the xlane
// phase. Single-operand moves have 64 slots (the lanes); the two swaps have
// 128: A's lanes, then B's.
static int vs_xlane_source(int n, int i) {
    const int l = i & 63;
    switch (n) {
        case 0: return (l & ~3) | ((l + 1) & 3);
        case 1: return (l & ~15) | ((l - 3) & 15);
        case 2: return l ^ 15;
        case 3: return l ^ 7;
        case 4: return (5 * l + 3) & 63;
        case 5:
        case 6: {
            const int half = n == 5 ? 16 : 32;
            if (i < 64) return l & half ? 64 + l - half : l;  // A': B's row below, or A
            return l & half ? i : l + half;                   // B': B, or A's row above
        }
        default: return VS_BCAST_LANE;
    }
}
static int vs_xlane_slots(int n) { return n == 5 || n == 6 ? 128 : 64; }

// Pure host code: the source table of move n (see vs_xlane_source).
extern "C" int na_valu_sweep_xlane_table(int move, int* out, int n) {
    if (move < 0 || move >= VS_XLANE_MOVES || out == nullptr || n < vs_xlane_slots(move))
        return arg_error("na_valu_sweep_xlane_table: need move in 0..%d (got %d) and room for its "
                         "slots (out %p, n %d)",
                         VS_XLANE_MOVES - 1, move, (void*)out, n);
    for (int i = 0; i < vs_xlane_slots(move); ++i) out[i] = vs_xlane_source(move, i);
    return vs_xlane_slots(move);
}

static inline uint64_t vs_hfold(uint64_t c, uint64_t v) { return c * MS_G + v; }
static inline uint64_t vs_hfold_int(uint64_t c, int v) { return c * MS_G + (uint64_t)(int64_t)v; }

// x = fma(x, a, b) chains on exact small integers, in integer arithmetic:
// `n` chains from h(p, first + j), x kept to `mask` + 1 values around 0.
static void vs_chain_init(uint64_t base, int p, uint64_t first, int n, int mask, int* x, int* a,
                          int* b) {
    for (int j = 0; j < n; ++j) {
        const uint64_t e = vs_h(base, p, first + j);
        x[j] = (int)(e & mask) - (mask + 1) / 2;
        a[j] = (int)((e >> 12) % 7) - 3;
        b[j] = (int)((e >> 20) % 15) - 7;
    }
}
static inline int vs_chain_step(uint64_t& c, int x, int a, int b, int mask) {
    const int r = x * a + b;
    c = vs_hfold_int(c, r);
    return (r & mask) - (mask + 1) / 2;
}

// The VS_PHASES checksums of wave `wave` (trans: 0).
static void vs_expected(uint64_t base, uint64_t wave, int iters, uint64_t* out) {
    for (int p = 0; p < VS_PHASES; ++p) out[p] = 0;
    uint32_t xl[64];
    uint64_t xc[64];
    for (uint32_t l = 0; l < 64; ++l) {
        const uint64_t gl = wave * 64 + l;
        for (int p = VS_RF; p <= VS_RF_INV; ++p) {
            const uint32_t pol = p == VS_RF ? 0u : ~0u;
            uint32_t x = (uint32_t)(vs_h(base, p, gl) >> 32), lo = 0, hi = 0;
            for (int s = 0; s < VS_SLOTS; ++s) {
                x = x * VS_LCG_A + VS_LCG_B;
                lo = lo * VS_FOLD_LO + (x ^ pol);
                hi = hi * VS_FOLD_HI + (x ^ pol);
            }
            out[p] += ((uint64_t)hi << 32) | lo;
        }
        {
            const uint64_t h0 = vs_h(base, VS_I32, 2 * gl), h1 = vs_h(base, VS_I32, 2 * gl + 1);
            uint32_t a = (uint32_t)h0, b = (uint32_t)(h0 >> 32), c = (uint32_t)h1,
                     d = (uint32_t)(h1 >> 32);
            uint64_t sum = 0;
            for (uint32_t k = 0; k < VS_STEPS; ++k) {
                const uint32_t t = a * b;
                const uint32_t u = (uint32_t)(((uint64_t)c * (d | 1u)) >> 32);
                const uint64_t m = (uint64_t)a * c + (((uint64_t)d << 32) | b);
                const uint32_t e = t + u + (uint32_t)m;
                const uint32_t f = e ^ (uint32_t)(m >> 32) ^ k;
                const uint32_t g = (uint32_t)((((uint64_t)f << 32) | e) >> (k & 31));
                const uint64_t gt = ((uint64_t)g << 32) | t;
                uint32_t q = 0;
                for (int i = 0; i < 4; ++i)
                    q |= (uint32_t)((gt >> (8 * ((VS_PERM_SEL >> (8 * i)) & 7))) & 0xFF) << (8 * i);
                sum = vs_hfold(sum, ((uint64_t)q << 32) | g);
                sum = vs_hfold(sum, ((uint64_t)f << 32) | e);
                a = q + 0x9E3779B9u, b = g | 1u, c = f, d = e + k;
            }
            out[VS_I32] += sum;
        }
        for (int p = VS_F32; p <= VS_F64; ++p) {
            int x[4], a[4], b[4];
            vs_chain_init(base, p, 4 * gl, 4, 0xFFF, x, a, b);
            uint64_t sum = 0;
            for (int k = 0; k < VS_STEPS; ++k)
                for (int j = 0; j < 4; ++j) x[j] = vs_chain_step(sum, x[j], a[j], b[j], 0xFFF);
            out[p] += sum;
        }
        {
            int x[8], a[8], b[8];
            vs_chain_init(base, VS_PK, 8 * gl, 4, 0xFFF, x, a, b);
            vs_chain_init(base, VS_PK, 8 * gl + 4, 4, 0x3FF, x + 4, a + 4, b + 4);
            uint64_t sum = 0;
            for (int k = 0; k < VS_STEPS; ++k)
                for (int j = 0; j < 8; ++j)
                    x[j] = vs_chain_step(sum, x[j], a[j], b[j], j < 4 ? 0xFFF : 0x3FF);
            out[VS_PK] += sum;
        }
        {
            uint64_t sum = 0;
            for (int j = 0; j < 2 * VS_STREAM_PAIRS; ++j) {
                const uint64_t e = vs_h(base, VS_STREAM, 2 * VS_STREAM_PAIRS * gl + j);
                const int x = (int)(e & 0xFFF) - 2048, b = (int)((e >> 13) % 5) - 2;
                const bool neg = (e >> 12) & 1;
                sum = vs_hfold_int(sum, !neg ? x + iters * b : (iters & 1) ? b - x : x);
            }
            out[VS_STREAM] += sum;
        }
        xl[l] = (uint32_t)(vs_h(base, VS_XLANE, gl) >> 32);
        xc[l] = 0;
    }
    // xlane: the whole wave at once
    for (int n = 0; n < VS_XLANE_MOVES; ++n) {
        uint32_t src[128], moved[128];
        const uint32_t other = n == 5 ? 0xA5A5A5A5u : 0x5A5A5A5Au;
        for (int l = 0; l < 64; ++l) src[l] = xl[l], src[64 + l] = xl[l] ^ other;
        const int slots = vs_xlane_slots(n);
        for (int i = 0; i < slots; ++i) moved[i] = src[vs_xlane_source(n, i)];
        for (uint32_t l = 0; l < 64; ++l) {
            uint32_t v = moved[l];
            if (slots == 128) v ^= (moved[64 + l] << 7) | (moved[64 + l] >> 25);
            xl[l] = v * VS_XLANE_MUL + l;
            xc[l] = vs_hfold(xc[l], xl[l]);
        }
    }
    for (int l = 0; l < 64; ++l) out[VS_XLANE] += xc[l];
}

// R of the register-file phases: a0..a255 and v32..v255.
extern "C" int na_valu_sweep_slots() { return VS_SLOTS; }

// Pure host code: the VS_PHASES checksums of one wave, in the order of the
// VS_* codes; the trans entry, which has no host reference, is 0.
extern "C" int na_valu_sweep_expected(unsigned long long seed, unsigned long long wave, int iters,
                                      uint64_t* checksums) {
    if (iters < 1 || iters > VS_MAX_ITERS || checksums == nullptr)
        return arg_error("na_valu_sweep_expected: need iters in 1..%d, the bound to which the "
                         "stream phase is exact (got %d), and room for %d checksums",
                         VS_MAX_ITERS, iters, VS_PHASES);
    vs_expected(seed * MS_G, wave, iters, checksums);
    return NA_OK;
}

// One launch of `workgroups` x 4 waves, HIP-event timed; out receives the
// 4 * workgroups records. Argument errors are detected before any HIP call.
extern "C" int na_valu_sweep_run(int dev, int workgroups, int iters, unsigned long long seed,
                                 na_valu_record* out, long long n_out, double* ms) {
    if (workgroups < 1 || workgroups > NA_VALU_MAX_WORKGROUPS || iters < 1 ||
        iters > VS_MAX_ITERS || out == nullptr ||
        n_out < (long long)workgroups * MS_WAVES_PER_WG)
        return arg_error("na_valu_sweep_run: need workgroups in 1..%d (got %d), iters in 1..%d, "
                         "the bound to which the stream phase is exact (got %d), and room for 4 "
                         "records per workgroup (out %p, n_out %lld)",
                         NA_VALU_MAX_WORKGROUPS, workgroups, VS_MAX_ITERS, iters, (void*)out,
                         n_out);
    size_t lds_bytes = 0;
    int rc = sweep_lds_bytes(dev, &lds_bytes);
    if (rc != NA_OK) return rc;
    const size_t n = (size_t)workgroups * MS_WAVES_PER_WG;
    return sweep_launch(dev, n, out, ms, [&](na_valu_record* records) {
        valu_sweep_kernel<<<dim3((unsigned)workgroups), dim3(VS_BLOCK), lds_bytes>>>(
            records, seed * MS_G, iters);
    });
}

// Pure host code: record i is wave i. A wave is bad when an exact phase
// checksum is not the expected one, when its in-kernel register-file count is
// not zero, when its trans checksum is not the strict majority's (with fewer
// than 3 records or no strict majority the phase is left unchecked, which is
// no failure), when it does not carry its own index, or when its workgroup's
// four waves are not on four distinct SIMDs of one CU. Returns NA_ERR_VERIFY
// on any bad wave; *res is filled either way.
extern "C" int na_valu_sweep_verify(const na_valu_record* recs, long long n, int iters,
                                    unsigned long long seed, na_valu_sweep_result* res) {
    if (recs == nullptr || n < 1 || iters < 1 || iters > VS_MAX_ITERS || res == nullptr)
        return arg_error("na_valu_sweep_verify: need records, n >= 1 (got %lld), iters in 1..%d "
                         "(got %d) and a result pointer",
                         n, VS_MAX_ITERS, iters);
    std::memset(res, 0, sizeof(*res));
    res->waves = (uint64_t)n;
    res->rf_first_slot = res->rf_first_lane = ~0u;
    const uint64_t base = seed * MS_G;

    // trans: the strict majority by the Boyer-Moore vote, then a count
    res->trans_unchecked = 1;
    if (n >= 3) {
        uint64_t cand = 0;
        long long votes = 0, count = 0;
        for (long long i = 0; i < n; ++i) {
            if (votes == 0) cand = recs[i].checksum[VS_TRANS];
            votes += recs[i].checksum[VS_TRANS] == cand ? 1 : -1;
        }
        for (long long i = 0; i < n; ++i) count += recs[i].checksum[VS_TRANS] == cand;
        if (2 * count > n) {
            res->trans_unchecked = 0;
            res->trans_consensus = cand;
        }
    }

    std::vector<uint32_t> mask((size_t)n, 0);
    sweep_census census;
    std::vector<double> rate;
    std::vector<uint64_t> cycles;
    for (long long i = 0; i < n; ++i) {
        const na_valu_record& r = recs[i];
        census.see(r, r.simd);
        if (r.cycles) {
            rate.push_back((double)iters * VS_FLOP_PER_ITER / (double)r.cycles);
            cycles.push_back(r.cycles);
        }
        uint64_t want[VS_PHASES];
        vs_expected(base, (uint64_t)i, iters, want);
        for (int p = 0; p < VS_PHASES; ++p)
            if (p != VS_TRANS && r.checksum[p] != want[p]) mask[i] |= 1u << p;
        if (r.rf_bad != 0 && !(mask[i] & (1u << VS_RF | 1u << VS_RF_INV)))
            mask[i] |= 1u << (r.rf_first_slot != ~0u && r.rf_first_slot >= 512 ? VS_RF_INV : VS_RF);
        if (!res->trans_unchecked && r.checksum[VS_TRANS] != res->trans_consensus)
            mask[i] |= 1u << VS_TRANS;
        if (r.wave != (uint64_t)i) mask[i] |= NA_VALU_BAD_INDEX;
    }
    for (long long g = 0; g + MS_WAVES_PER_WG <= n; g += MS_WAVES_PER_WG) {
        unsigned simds = 0;
        bool one_cu = true;
        for (int k = 0; k < MS_WAVES_PER_WG; ++k) {
            simds |= 1u << (recs[g + k].simd & 3);
            one_cu = one_cu && ms_cu_key(recs[g + k]) == ms_cu_key(recs[g]);
        }
        if (simds != 15u || !one_cu)
            for (int k = 0; k < MS_WAVES_PER_WG; ++k) mask[g + k] |= NA_VALU_BAD_PLACEMENT;
    }
    for (long long i = 0; i < n; ++i) {
        if (mask[i] == 0) continue;
        const na_valu_record& r = recs[i];
        if (res->bad_waves++ == 0 && (mask[i] & (1u << VS_RF | 1u << VS_RF_INV)) && r.rf_bad) {
            res->rf_bad = r.rf_bad;
            res->rf_first_slot = r.rf_first_slot;
            res->rf_first_lane = r.rf_first_lane;
            res->rf_xor = r.rf_xor;
        }
        if (res->listed < NA_SWEEP_MAX_LISTED) {
            const uint32_t row[7] = {(uint32_t)i, r.xcc, r.se, r.sh, r.cu, r.simd, mask[i]};
            std::memcpy(res->bad_list[res->listed++], row, sizeof(row));
        }
    }
    res->cus_seen = census.cus_seen;
    res->simds_seen = census.simds_seen;
    res->clock_mhz = census.clock_mhz();
    if (!rate.empty()) res->min_flop_per_clk = *std::min_element(rate.begin(), rate.end());
    res->median_flop_per_clk = median_of(rate);
    res->median_cycles = median_of(cycles);
    res->tflops = res->median_flop_per_clk * (double)res->simds_seen * res->clock_mhz / 1e6;
    if (res->bad_waves == 0) return NA_OK;
    const uint32_t* u = res->bad_list[0];
    char phases[96] = "";
    for (int p = 0, at = 0; p < VS_PHASES + 2; ++p)
        if (u[6] >> p & 1)
            at += std::snprintf(phases + at, sizeof(phases) - at, "%s%s", at ? "," : "",
                                vs_phase_names[p]);
    char where[128] = "";
    if (res->rf_bad) {
        const uint32_t slot = res->rf_first_slot & 511;
        std::snprintf(where, sizeof(where),
                      ", %u wrong registers, first %c%u lane %u, failing bits 0x%08x", res->rf_bad,
                      slot < 256 ? 'a' : 'v', slot < 256 ? slot : slot - 256 + VS_FIRST_VGPR,
                      res->rf_first_lane, res->rf_xor);
    }
    return na_error(NA_ERR_VERIFY,
                    "valu sweep: %llu of %llu waves wrong, first wave %u in phase %s on "
                    "xcc%u.se%u.sh%u.cu%u.simd%u%s",
                    (unsigned long long)res->bad_waves, (unsigned long long)res->waves, u[0],
                    phases, u[1], u[2], u[3], u[4], u[5], where);
}

// Whole sweep: one untimed warm-up launch, the timed launch, the verify.
// workgroups 0 = 4 per CU, iters 0 = NA_VALU_DEFAULT_ITERS. res->tflops is
// the chip-wide rate of the stream phase from the in-kernel stamps alone,
// not the launch's event time (which includes the other phases): the median
// SIMD's FLOP per shader clock, on every SIMD that took part, at the median
// measured clock.
extern "C" int na_valu_sweep(int dev, int workgroups, int iters, unsigned long long seed,
                             na_valu_sweep_result* res) {
    if (res == nullptr || workgroups < 0 || workgroups > NA_VALU_MAX_WORKGROUPS || iters < 0 ||
        iters > VS_MAX_ITERS)
        return arg_error("na_valu_sweep: need workgroups in 0..%d (got %d), iters in 0..%d (got "
                         "%d) and a result pointer",
                         NA_VALU_MAX_WORKGROUPS, workgroups, VS_MAX_ITERS, iters);
    int rc = sweep_defaults(dev, &workgroups, &iters, NA_VALU_DEFAULT_ITERS);
    if (rc != NA_OK) return rc;
    std::vector<na_valu_record> recs((size_t)workgroups * MS_WAVES_PER_WG);
    rc = sweep_twice([&] {
        return na_valu_sweep_run(dev, workgroups, iters, seed, recs.data(),
                                 (long long)recs.size(), nullptr);
    });
    if (rc != NA_OK) return rc;
    return na_valu_sweep_verify(recs.data(), (long long)recs.size(), iters, seed, res);
}

// ---------------------------------------------------------------------------
// Chip-wide load sweep (kernel and specification in loadsweep.h)
// ---------------------------------------------------------------------------
//
// Every sweep above tests its unit with the rest of the chip idle, and the
// memtest streams HBM with no MFMA in flight. A part that is marginal on
// power delivery or timing passes all of them and miscomputes in service,
// where matrix cores, LDS and HBM are busy in the same cycles. This sweep
// runs one workgroup of eight waves per CU at a time: four on the
// matrix-core sweep's MFMA chain, four streaming a slice of pattern-filled
// device memory through LDS and comparing every word. The host recomputes
// every wave's checksum exactly, so a wave that is wrong under load is named
// by role and (XCC, SE, SH, CU, SIMD); the in-kernel clocks give the rates
// both roles reach together and the clock the chip holds under that load.
// Records and results are the matrix-core sweep's structs, one set per role;
// the in-kernel comparison reports through the memtest's.

#include "loadsweep.h"

// 16 GiB per workgroup at the longest slice: about a second of a CU's share
// of HBM, NA_MFMA_MAX_OUTER's kind of bound against a typo.
#define NA_LOAD_MAX_PASSES 1024
#define NA_LOAD_DEFAULT_BYTES (4 << 20)
// Chosen on the MI355X so that both roles of a workgroup take about the same
// time: 8192 folds are the matrix-core sweep's, and 19 passes over 4 MiB take
// the stream waves as long beside them (about 5 ms per workgroup, overlap
// 0.98; the default grid puts four workgroups on each CU in turn: 21.8 ms per
// launch measured, profiles/load_sweep_mi355x.txt) — the range of the other
// sweeps, and past the 10 ms from which the in-kernel clock estimate is
// reliable (see NA_MFMA_DEFAULT_OUTER).
#define NA_LOAD_DEFAULT_OUTER 8192
#define NA_LOAD_DEFAULT_PASSES 19

static bool ld_bytes_ok(long long slice_bytes) {
    return slice_bytes >= LD_GRANULE && slice_bytes <= LD_MAX_BYTES &&
           slice_bytes % LD_GRANULE == 0;
}

// What dtype, workgroups, outer and passes must satisfy in _run; `lo` is 0
// where the whole-sweep entry point takes 0 as "the default".
static bool ld_shape_ok(int dtype, int workgroups, int outer, int passes, int lo) {
    return (dtype == 0 || dtype == 1) && workgroups >= lo &&
           workgroups <= NA_MFMA_MAX_WORKGROUPS && outer >= 0 && outer <= NA_MFMA_MAX_OUTER &&
           passes >= 0 && passes <= NA_LOAD_MAX_PASSES;
}

// The sums of ld_term over the vectors of workgroup `workgroup`'s slice that
// each of its four stream waves reads in one pass.
static void ld_stream_sums(uint64_t base, uint64_t workgroup, uint64_t vecs, uint64_t* sums) {
    for (int q = 0; q < MS_WAVES_PER_WG; ++q) sums[q] = 0;
    const uint64_t v0 = workgroup * vecs;
    for (uint64_t i = 0; i < vecs; ++i) {
        const mt_vec w = mt_pattern(v0 + i, base, 0);
        sums[(i >> 6) & (MS_WAVES_PER_WG - 1)] += ld_term(w.x, w.y);
    }
}

// Pure host code: the checksums of the four stream waves of one workgroup
// after `passes` passes over its slice. n is the room in `checksums`.
extern "C" int na_load_sweep_stream_expected(unsigned long long seed, unsigned long long workgroup,
                                             long long slice_bytes, int passes,
                                             uint64_t* checksums, int n) {
    if (!ld_bytes_ok(slice_bytes) || passes < 1 || passes > NA_LOAD_MAX_PASSES ||
        checksums == nullptr || n < MS_WAVES_PER_WG)
        return arg_error("na_load_sweep_stream_expected: need slice_bytes a multiple of %d in "
                         "%d..%d (got %lld), passes in 1..%d (got %d) and room for %d checksums "
                         "(n %d)",
                         LD_GRANULE, LD_GRANULE, LD_MAX_BYTES, slice_bytes, NA_LOAD_MAX_PASSES,
                         passes, MS_WAVES_PER_WG, n);
    ld_stream_sums(seed * MS_G, workgroup, (uint64_t)slice_bytes / 16, checksums);
    for (int q = 0; q < MS_WAVES_PER_WG; ++q) checksums[q] *= (uint64_t)passes;
    return NA_OK;
}

// One launch of `workgroups` x 8 waves on a caller-owned device region of
// workgroups * slice_bytes bytes that holds the memtest pattern of `seed`
// (na_memtest_fill, invert 0), HIP-event timed; matrix and stream receive the
// 4 * workgroups records of their role, *mem what the stream waves' own
// comparison saw. Returns NA_ERR_VERIFY when that saw a mismatch; the records
// and *mem are filled either way. Argument errors are detected before any HIP
// call.
extern "C" int na_load_sweep_run(int dev, int dtype, int workgroups, int outer, void* region,
                                 long long slice_bytes, int passes, unsigned long long seed,
                                 na_mfma_record* matrix, na_mfma_record* stream, long long n_out,
                                 na_memtest_result* mem, double* ms) {
    if (!ld_shape_ok(dtype, workgroups, outer, passes, 1) || !ld_bytes_ok(slice_bytes))
        return arg_error("na_load_sweep_run: need dtype 0 (bf16) or 1 (fp8) (got %d), workgroups "
                         "in 1..%d (got %d), outer in 0..%d (got %d), slice_bytes a multiple of %d "
                         "up to %d (got %lld) and passes in 0..%d (got %d)",
                         dtype, NA_MFMA_MAX_WORKGROUPS, workgroups, NA_MFMA_MAX_OUTER, outer,
                         LD_GRANULE, LD_MAX_BYTES, slice_bytes, NA_LOAD_MAX_PASSES, passes);
    if (outer == 0 && passes == 0)
        return arg_error("na_load_sweep_run: outer and passes are both 0: no role to run");
    if (region == nullptr || ((uintptr_t)region & 15) != 0 || matrix == nullptr ||
        stream == nullptr || mem == nullptr || n_out < (long long)workgroups * MS_WAVES_PER_WG)
        return arg_error("na_load_sweep_run: need a 16-byte aligned region (%p), room for 4 "
                         "records per workgroup and role (matrix %p, stream %p, n_out %lld) and a "
                         "memtest result pointer (mem %p)",
                         region, (void*)matrix, (void*)stream, n_out, (void*)mem);
    HIP_CHECK(hipSetDevice(dev));  // for the accumulator below, ahead of sweep_launch
    size_t lds_bytes = 0;
    int rc = sweep_lds_bytes(dev, &lds_bytes);
    if (rc != NA_OK) return rc;
    if (lds_bytes < LD_LDS_BYTES)
        return arg_error("na_load_sweep_run: the device's %zu-byte per-workgroup LDS allocation "
                         "is under the %d bytes the stream waves use",
                         lds_bytes, LD_LDS_BYTES);
    mt_dev_accum acc;
    rc = acc.init();
    if (rc != NA_OK) return rc;
    static void (*const kernels[2])(na_mfma_record*, na_mfma_record*, const mt_vec*, mt_u64, int,
                                    uint32_t, int, mt_accum*) = {load_sweep_kernel<MS_BF16>,
                                                                 load_sweep_kernel<MS_FP8>};
    // one device array, the matrix records ahead of the stream records
    const size_t n = (size_t)workgroups * MS_WAVES_PER_WG;
    std::vector<na_mfma_record> both(2 * n);
    rc = sweep_launch(dev, 2 * n, both.data(), ms, [&](na_mfma_record* records) {
        kernels[dtype]<<<dim3((unsigned)workgroups), dim3(LD_BLOCK), lds_bytes>>>(
            records, records + n, static_cast<const mt_vec*>(region), seed * MS_G, outer,
            (uint32_t)(slice_bytes / LD_GRANULE), passes, acc.d.p);
    });
    if (rc != NA_OK) return rc;
    std::copy(both.begin(), both.begin() + n, matrix);
    std::copy(both.begin() + n, both.end(), stream);
    rc = acc.read(passes ? (uint64_t)workgroups * (uint64_t)slice_bytes : 0, mem);
    if (rc != NA_OK) return rc;
    return mt_verdict("load sweep", mem);
}

// Pure host code: n records per role, record i being wave i of its role
// (workgroup i / 4). The rules are the matrix-core sweep's (ms_tally), per
// role; the records of a role that is off (outer 0, passes 0) must be all
// zero. Returns NA_ERR_VERIFY on any bad wave; both results are filled either
// way.
extern "C" int na_load_sweep_verify(const na_mfma_record* matrix, const na_mfma_record* stream,
                                    long long n, int outer, long long slice_bytes, int passes,
                                    unsigned long long seed, na_mfma_sweep_result* matrix_res,
                                    na_mfma_sweep_result* stream_res) {
    if (matrix == nullptr || stream == nullptr || n < MS_WAVES_PER_WG ||
        n % MS_WAVES_PER_WG != 0 || !ld_shape_ok(0, 1, outer, passes, 1) ||
        !ld_bytes_ok(slice_bytes) || matrix_res == nullptr || stream_res == nullptr)
        return arg_error("na_load_sweep_verify: need the records of both roles, n a positive "
                         "multiple of 4 (got %lld), outer in 0..%d (got %d), slice_bytes a multiple "
                         "of %d up to %d (got %lld), passes in 0..%d (got %d) and two result "
                         "pointers",
                         n, NA_MFMA_MAX_OUTER, outer, LD_GRANULE, LD_MAX_BYTES, slice_bytes,
                         NA_LOAD_MAX_PASSES, passes);
    if (outer == 0 && passes == 0)
        return arg_error("na_load_sweep_verify: outer and passes are both 0: no role ran");
    const uint64_t base = seed * MS_G;
    ms_tally(matrix, n, outer != 0, matrix_res, [&](long long i) {
        uint64_t want = 0;
        (void)ms_expected(ms_mfma, seed, (uint64_t)i, outer, &want);  // outer >= 1 here
        return want;
    });
    uint64_t sums[MS_WAVES_PER_WG] = {};
    ms_tally(stream, n, passes != 0, stream_res, [&](long long i) {
        if (i % MS_WAVES_PER_WG == 0)  // the records come in order: once per workgroup
            ld_stream_sums(base, (uint64_t)i / MS_WAVES_PER_WG, (uint64_t)slice_bytes / 16, sums);
        return (uint64_t)passes * sums[i % MS_WAVES_PER_WG];
    });
    if (matrix_res->bad_waves == 0 && stream_res->bad_waves == 0) return NA_OK;
    const bool first_is_matrix = matrix_res->bad_waves != 0;
    const na_mfma_sweep_result* first = first_is_matrix ? matrix_res : stream_res;
    const uint32_t* u = first->first_bad_unit;
    return na_error(NA_ERR_VERIFY,
                    "load sweep: %llu of %llu matrix waves and %llu of %llu stream waves wrong "
                    "under combined load on %llu and %llu CU(s), first %s wave %llu on "
                    "xcc%u.se%u.sh%u.cu%u.simd%u",
                    (unsigned long long)matrix_res->bad_waves,
                    (unsigned long long)matrix_res->waves,
                    (unsigned long long)stream_res->bad_waves,
                    (unsigned long long)stream_res->waves,
                    (unsigned long long)matrix_res->bad_units,
                    (unsigned long long)stream_res->bad_units,
                    first_is_matrix ? "matrix" : "stream",
                    (unsigned long long)first->first_bad_wave, u[0], u[1], u[2], u[3], u[4]);
}

// The chip-wide rate of one role from the in-kernel stamps alone, as the VALU
// and cache sweeps compute theirs: the median wave's work per shader clock,
// on the four waves of that role on every CU that took part, at the median
// measured clock. `work` is one wave's, `per_mhz` scales work x MHz to the
// unit reported.
static double ld_rate(const na_mfma_record* recs, size_t n, double work,
                      const na_mfma_sweep_result* res, double per_mhz) {
    std::vector<double> rate;
    for (size_t i = 0; i < n; ++i)
        if (recs[i].cycles) rate.push_back(work / (double)recs[i].cycles);
    return median_of(rate) * MS_WAVES_PER_WG * (double)res->units_seen * res->clock_mhz / per_mhz;
}

// Whole sweep on a region the agent allocates and fills itself: one untimed
// warm-up launch, the timed launch, the verify. 0 = default for workgroups
// (4 per CU), outer, slice_bytes and passes, so both roles run; the roles
// alone are reached through na_load_sweep_run. *tflops and *gbs are the
// rates the two roles reach together (ld_rate), matrix_res->clock_mhz the
// clock under that load, *overlap the median over the workgroups of
// min(Tm, Ts) / max(Tm, Ts), Tm and Ts being the longest realtime among the
// workgroup's matrix waves and among its stream waves. A region over half of
// the free device memory, or one that cannot be allocated, is NA_ERR_ARG.
extern "C" int na_load_sweep(int dev, int dtype, int workgroups, int outer, long long slice_bytes,
                             int passes, unsigned long long seed,
                             na_mfma_sweep_result* matrix_res, na_mfma_sweep_result* stream_res,
                             na_memtest_result* mem, double* tflops, double* gbs,
                             double* overlap) {
    if (!ld_shape_ok(dtype, workgroups, outer, passes, 0) ||
        (slice_bytes != 0 && !ld_bytes_ok(slice_bytes)) || matrix_res == nullptr ||
        stream_res == nullptr || mem == nullptr)
        return arg_error("na_load_sweep: need dtype 0 (bf16) or 1 (fp8) (got %d), workgroups in "
                         "0..%d (got %d), outer in 0..%d (got %d), slice_bytes 0 or a multiple of "
                         "%d up to %d (got %lld), passes in 0..%d (got %d) and three result "
                         "pointers",
                         dtype, NA_MFMA_MAX_WORKGROUPS, workgroups, NA_MFMA_MAX_OUTER, outer,
                         LD_GRANULE, LD_MAX_BYTES, slice_bytes, NA_LOAD_MAX_PASSES, passes);
    int rc = sweep_defaults(dev, &workgroups, &outer, NA_LOAD_DEFAULT_OUTER);
    if (rc != NA_OK) return rc;
    if (passes == 0) passes = NA_LOAD_DEFAULT_PASSES;
    if (slice_bytes == 0) slice_bytes = NA_LOAD_DEFAULT_BYTES;
    HIP_CHECK(hipSetDevice(dev));
    const size_t bytes = (size_t)workgroups * (size_t)slice_bytes;
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    dev_buf<unsigned char> region;
    if (bytes > free_b / 2 || region.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();  // consumed here, not by a later check
        return arg_error("na_load_sweep: the region of %zu bytes (%d workgroups x %lld) does not "
                         "fit: %zu bytes of device memory are free and the sweep takes at most "
                         "half",
                         bytes, workgroups, slice_bytes, free_b);
    }
    rc = mt_launch(MT_FILL, region.p, bytes / 16, 0, seed, 0, nullptr);
    if (rc != NA_OK) return rc;
    HIP_CHECK(hipDeviceSynchronize());
    const size_t n = (size_t)workgroups * MS_WAVES_PER_WG;
    std::vector<na_mfma_record> matrix(n), stream(n);
    rc = sweep_twice([&] {
        int run = na_load_sweep_run(dev, dtype, workgroups, outer, region.p, slice_bytes, passes,
                                    seed, matrix.data(), stream.data(), (long long)n, mem,
                                    nullptr);
        return run == NA_ERR_VERIFY ? NA_OK : run;  // bad words: judged below, with the records
    });
    if (rc != NA_OK) return rc;
    rc = na_load_sweep_verify(matrix.data(), stream.data(), (long long)n, outer, slice_bytes,
                              passes, seed, matrix_res, stream_res);
    if (rc != NA_OK && rc != NA_ERR_VERIFY) return rc;
    if (tflops)
        *tflops = ld_rate(matrix.data(), n,
                          (double)outer * MS_MFMA_PER_FOLD * MS_FLOP_PER_MFMA_K * ms_mfma.k_len,
                          matrix_res, 1e6);
    if (gbs)
        *gbs = ld_rate(stream.data(), n, (double)passes * (double)slice_bytes / MS_WAVES_PER_WG,
                       stream_res, 1e3);
    if (overlap) {
        std::vector<double> ratio;
        for (size_t g = 0; g < n; g += MS_WAVES_PER_WG) {
            uint64_t tm = 0, ts = 0;
            for (int k = 0; k < MS_WAVES_PER_WG; ++k) {
                tm = std::max<uint64_t>(tm, matrix[g + k].realtime);
                ts = std::max<uint64_t>(ts, stream[g + k].realtime);
            }
            if (tm && ts) ratio.push_back((double)std::min(tm, ts) / (double)std::max(tm, ts));
        }
        *overlap = median_of(ratio);
    }
    return rc != NA_OK ? rc : mt_verdict("load sweep", mem);
}
