// loadgen_lib.cpp — host-side C API around the CDNA4 load kernels.
//
// MI355X-native replacement for the reference's load workload machinery
// (reference: cuda-test-deployment.yaml:18-19 runs 5000 sequential CUDA
// `vectorAdd` *processes*; README.md:115 doubles the load with a second
// loop). Here the same load shapes are produced from one resident process:
//   * lg_vector_add_loop(): N launches of the vectorAdd kernel with a host
//     sync between launches — reproduces the reference's partial-utilization
//     shape (launch/driver overhead dominates) without 5000 process forks.
//   * lg_gemm_burn(): duty-cycled MFMA bf16 GEMM bursts targeting a given
//     GPU-busy percentage — the high/tunable load the scale-up experiments
//     need (reference has no equivalent).
//   * lg_gemm_fp8_*/lg_gemm_mxfp4_*(): the same bench/burn/verify entries
//     over the fp8 (E4M3) and MXFP4 (E2M1 + E8M0 block scale) MFMA kernels.
//   * lg_decode_mxfp4_*(): the decode half of an inference pod — a skinny-M
//     (1..64 rows) MXFP4 GEMM streaming a ring of weight matrices from HBM
//     (gemm_mxfp4_decode.hip): busy% high, matrix cores idle, bandwidth-bound.
//   * lg_*_verify(): run one kernel on caller-provided host data so tests
//     can check numerics against a plain fp32 reference.
//
// Exposed as a plain C ABI: consumed by loadgen_main.cpp (CLI) and by
// mi355x_gpu_hpa/loadgen (ctypes).

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "mxfp4_host.h"

extern "C" __global__ void vector_add_f32(const float*, const float*, float*, int);
extern "C" __global__ void vector_add_f32x4(const float4*, const float4*, float4*, int);
extern "C" __global__ void triad_f32x4(const float4*, const float4*, float4*, float,
                                       long);
extern "C" __global__ void gemm_bf16_tn(const unsigned short*, const unsigned short*,
                                        float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_linear(const unsigned short*,
                                               const unsigned short*, float*, int,
                                               int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d21(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d20(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d19(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d18(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d9e(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d9w(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d6(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d14(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d9(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d9nr(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d2(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d7(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d8(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_w32(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_soft(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d5(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d4(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256_d1(const unsigned short*, const unsigned short*, float*, int, int, int, int);
extern "C" __global__ void gemm_bf16_tn_256(const unsigned short*,
                                            const unsigned short*, float*, int,
                                            int, int, int);
extern "C" __global__ void gemm_fp8_tn_256(const unsigned char*,
                                           const unsigned char*, float*, int,
                                           int, int, int);
extern "C" __global__ void gemm_fp8_tn_256_db(const unsigned char*,
                                              const unsigned char*, float*, int,
                                              int, int, int);
extern "C" __global__ void gemm_fp8_tn_256_nr(const unsigned char*,
                                              const unsigned char*, float*, int,
                                              int, int, int);
extern "C" __global__ void gemm_mxfp4_tn_256(const unsigned char*,
                                             const unsigned char*, const int*,
                                             const int*, float*, int, int, int,
                                             int);
#define LG_DECODE_KERNEL(NAME)                                                \
    extern "C" __global__ void NAME(const unsigned char*, const int*,        \
                                    const unsigned char*, const int*, float*, \
                                    int, int, int, int, int)
LG_DECODE_KERNEL(decode_mxfp4_m16);
LG_DECODE_KERNEL(decode_mxfp4_m32);
LG_DECODE_KERNEL(decode_mxfp4_m48);
LG_DECODE_KERNEL(decode_mxfp4_m64);
#undef LG_DECODE_KERNEL
extern "C" __global__ void decode_mxfp4_reduce(const float4*, float4*, long,
                                               int);

#define LG_CHECK(expr)                                                        \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) {                                               \
            std::snprintf(g_last_error, sizeof(g_last_error), "%s:%d %s: %s", \
                          __FILE__, __LINE__, #expr, hipGetErrorString(_e));  \
            return -1;                                                        \
        }                                                                     \
    } while (0)

static char g_last_error[512] = "";

static inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

static inline unsigned short f32_to_bf16(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    // round-to-nearest-even
    uint32_t lsb = (u >> 16) & 1;
    u += 0x7fffu + lsb;
    return (unsigned short)(u >> 16);
}

extern "C" {

const char* lg_last_error() { return g_last_error; }

int lg_device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------------------
// vectorAdd
// ---------------------------------------------------------------------------

// One allocation + `iters` kernel launches (sync per launch, like one
// process-per-launch in the reference but without exec overhead).
// Returns 0 on success; *ms_out = total wall ms over the launches.
int lg_vector_add_loop(int device, int n, int iters, double* ms_out)
{
    LG_CHECK(hipSetDevice(device));
    float *a, *b, *c;
    size_t bytes = (size_t)n * 4;
    LG_CHECK(hipMalloc(&a, bytes));
    LG_CHECK(hipMalloc(&b, bytes));
    LG_CHECK(hipMalloc(&c, bytes));
    std::vector<float> h(n);
    for (int i = 0; i < n; ++i) h[i] = (float)((i * 2654435761u) % 1000) * 1e-3f;
    LG_CHECK(hipMemcpy(a, h.data(), bytes, hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(b, h.data(), bytes, hipMemcpyHostToDevice));

    int threads = 256;
    int blocks = (n + threads - 1) / threads;
    if (blocks > 4096) blocks = 4096; // grid-stride covers the rest
    double t0 = now_ms();
    for (int i = 0; i < iters; ++i) {
        hipLaunchKernelGGL(vector_add_f32, dim3(blocks), dim3(threads), 0, 0, a, b, c, n);
        LG_CHECK(hipDeviceSynchronize());
    }
    double t1 = now_ms();
    if (ms_out) *ms_out = t1 - t0;
    LG_CHECK(hipFree(a));
    LG_CHECK(hipFree(b));
    LG_CHECK(hipFree(c));
    return 0;
}

// Numerics entry: c_out[i] = a[i] + b[i] computed on the GPU.
int lg_vector_add_verify(int device, const float* a_h, const float* b_h, float* c_out, int n)
{
    LG_CHECK(hipSetDevice(device));
    float *a, *b, *c;
    size_t bytes = (size_t)n * 4;
    LG_CHECK(hipMalloc(&a, bytes));
    LG_CHECK(hipMalloc(&b, bytes));
    LG_CHECK(hipMalloc(&c, bytes));
    LG_CHECK(hipMemcpy(a, a_h, bytes, hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(b, b_h, bytes, hipMemcpyHostToDevice));
    int threads = 256;
    if (n % 4 == 0) {
        int n4 = n / 4;
        int blocks = (n4 + threads - 1) / threads;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(vector_add_f32x4, dim3(blocks), dim3(threads), 0, 0,
                           (const float4*)a, (const float4*)b, (float4*)c, n4);
    } else {
        int blocks = (n + threads - 1) / threads;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(vector_add_f32, dim3(blocks), dim3(threads), 0, 0, a, b, c, n);
    }
    LG_CHECK(hipDeviceSynchronize());
    LG_CHECK(hipMemcpy(c_out, c, bytes, hipMemcpyDeviceToHost));
    LG_CHECK(hipFree(a));
    LG_CHECK(hipFree(b));
    LG_CHECK(hipFree(c));
    return 0;
}

// ---------------------------------------------------------------------------
// MFMA bf16 GEMM
// ---------------------------------------------------------------------------

struct GemmBufs {
    unsigned short* a = nullptr;
    unsigned short* bt = nullptr;
    float* c = nullptr;
    int m = 0, n = 0, k = 0;
};

static int gemm_alloc(GemmBufs& g, int m, int n, int k, bool fill_random)
{
    LG_CHECK(hipMalloc(&g.a, (size_t)m * k * 2));
    LG_CHECK(hipMalloc(&g.bt, (size_t)n * k * 2));
    LG_CHECK(hipMalloc(&g.c, (size_t)m * n * 4));
    g.m = m; g.n = n; g.k = k;
    if (fill_random) {
        // Random-ish bf16 in [-1, 1): DVFS-honest load (zero-filled operands
        // clock higher and overstate TF/s — playbook §5.4 rule 25).
        size_t na = (size_t)m * k, nb = (size_t)n * k;
        std::vector<unsigned short> h(na > nb ? na : nb);
        uint32_t s = 0x12345678u;
        for (size_t i = 0; i < h.size(); ++i) {
            s = s * 1664525u + 1013904223u;
            float f = ((s >> 8) & 0xffff) / 32768.0f - 1.0f;
            h[i] = f32_to_bf16(f);
        }
        LG_CHECK(hipMemcpy(g.a, h.data(), na * 2, hipMemcpyHostToDevice));
        LG_CHECK(hipMemcpy(g.bt, h.data(), nb * 2, hipMemcpyHostToDevice));
    }
    return 0;
}

static void gemm_free(GemmBufs& g)
{
    (void)hipFree(g.a); (void)hipFree(g.bt); (void)hipFree(g.c);
    g = GemmBufs{};
}

// variant: 0 = 128^2 linear LDS, 1 = 128^2 swizzled, 2 = 256^2 8-phase.
static int gemm_launch(const GemmBufs& g, hipStream_t stream, int variant = 1)
{
    if (variant == 13) {  // d14: 1024-thread CTA, 4 waves/SIMD
        int n_tiles = (g.m / 256) * (g.n / 256);
        int blocks = n_tiles < 2048 ? n_tiles : 2048;
        int tiles_per_cta = (n_tiles + blocks - 1) / blocks;
        hipLaunchKernelGGL(gemm_bf16_tn_256_d14, dim3(blocks), dim3(1024), 0,
                           stream, g.a, g.bt, g.c, g.m, g.n, g.k, tiles_per_cta);
        return 0;
    }
    if (variant >= 2) {
        int n_tiles = (g.m / 256) * (g.n / 256);
        int blocks = n_tiles < 2048 ? n_tiles : 2048;
        int tiles_per_cta = (n_tiles + blocks - 1) / blocks;
        // product auto-select: at huge grids (>2048 tiles, 16k-class
        // shapes) the 3-deep-B d18 wins by ~16% (DMA latency under heavy
        // memory-system load); at <=8192-class shapes d9 ties or wins.
        if (variant == 2 && n_tiles > 2048) variant = 17;
        if (variant == 19 || variant == 20) {  // d20/d21: 256-thread CTA,
            hipLaunchKernelGGL(                    // 1 wave/SIMD, AGPR acc
                variant == 19 ? gemm_bf16_tn_256_d20 : gemm_bf16_tn_256_d21,
                dim3(blocks), dim3(256), 0, stream, g.a, g.bt, g.c, g.m,
                g.n, g.k, tiles_per_cta);
            return 0;
        }
        hipLaunchKernelGGL(variant == 3 ? gemm_bf16_tn_256_d1 : variant == 4 ? gemm_bf16_tn_256_d4 : variant == 5 ? gemm_bf16_tn_256_d5 : variant == 6 ? gemm_bf16_tn_256_d2 : variant == 7 ? gemm_bf16_tn_256_d7 : variant == 8 ? gemm_bf16_tn_256_d8 : variant == 9 ? gemm_bf16_tn_256_w32 : variant == 10 ? gemm_bf16_tn_256_soft : variant == 11 ? gemm_bf16_tn_256_d9 : variant == 12 ? gemm_bf16_tn_256_d9nr : variant == 14 ? gemm_bf16_tn_256_d6 : variant == 15 ? gemm_bf16_tn_256_d9w : variant == 16 ? gemm_bf16_tn_256_d9e : variant == 17 ? gemm_bf16_tn_256_d18 : variant == 18 ? gemm_bf16_tn_256_d19 : gemm_bf16_tn_256, dim3(blocks), dim3(512), 0, stream,
                           g.a, g.bt, g.c, g.m, g.n, g.k, tiles_per_cta);
        return 0;
    }
    int n_tiles = (g.m / 128) * (g.n / 128);
    int blocks = n_tiles < 2048 ? n_tiles : 2048;
    int tiles_per_cta = (n_tiles + blocks - 1) / blocks;
    if (variant == 0)
        hipLaunchKernelGGL(gemm_bf16_tn_linear, dim3(blocks), dim3(256), 0, stream,
                           g.a, g.bt, g.c, g.m, g.n, g.k, tiles_per_cta);
    else
        hipLaunchKernelGGL(gemm_bf16_tn, dim3(blocks), dim3(256), 0, stream,
                           g.a, g.bt, g.c, g.m, g.n, g.k, tiles_per_cta);
    return 0;
}

static bool gemm_dims_ok(int m, int n, int k, int variant)
{
    int mt = variant >= 2 ? 256 : 128;
    if (m % mt || n % mt || k % 64) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "gemm dims must be multiples of %d/%d/64", mt, mt);
        return false;
    }
    return true;
}

// Timed GEMM: `iters` back-to-back launches after `warmup` untimed ones.
// *ms_out = mean ms per GEMM, *tflops_out = 2*M*N*K / time.
// variant: 1 = st_16x32-swizzled LDS (default), 0 = linear LDS (A/B ref).
// 256-tile kernels need >=128 CTAs to fill the 256-CU chip; below that the
// 128-tile kernel wins (4x the CTAs). Perf entry points auto-select; the
// verify entry points do NOT (tests must exercise the exact kernel asked).
static int gemm_effective_variant(int m, int n, int variant)
{
    if (variant >= 2 && (m / 256) * (n / 256) < 128 && m % 128 == 0 &&
        n % 128 == 0)
        return 1;
    return variant;
}

int lg_gemm_bf16_bench_variant(int device, int m, int n, int k, int warmup,
                               int iters, int variant, double* ms_out,
                               double* tflops_out)
{
    if (!gemm_dims_ok(m, n, k, variant)) return -1;
    variant = gemm_effective_variant(m, n, variant);
    LG_CHECK(hipSetDevice(device));
    GemmBufs g;
    if (gemm_alloc(g, m, n, k, true)) return -1;
    for (int i = 0; i < warmup; ++i) gemm_launch(g, 0, variant);
    LG_CHECK(hipDeviceSynchronize());
    double t0 = now_ms();
    for (int i = 0; i < iters; ++i) gemm_launch(g, 0, variant);
    LG_CHECK(hipDeviceSynchronize());
    double t1 = now_ms();
    double ms = (t1 - t0) / iters;
    if (ms_out) *ms_out = ms;
    if (tflops_out) *tflops_out = 2.0 * m * n * k / (ms * 1e-3) / 1e12;
    gemm_free(g);
    return 0;
}

int lg_gemm_bf16_bench(int device, int m, int n, int k, int warmup, int iters,
                       double* ms_out, double* tflops_out)
{
    return lg_gemm_bf16_bench_variant(device, m, n, k, warmup, iters, 1, ms_out,
                                      tflops_out);
}

// Numerics entry: C f32 = A bf16 @ B^T bf16 on caller data (A row-major
// [m][k] as f32 -> converted; Bt row-major [n][k]).
// variant: 1 = swizzled (product kernel), 0 = linear LDS.
int lg_gemm_bf16_verify_variant(int device, const float* a_h, const float* bt_h,
                                float* c_out, int m, int n, int k, int variant)
{
    if (!gemm_dims_ok(m, n, k, variant)) return -1;
    LG_CHECK(hipSetDevice(device));
    GemmBufs g;
    if (gemm_alloc(g, m, n, k, false)) return -1;
    std::vector<unsigned short> tmp((size_t)m * k);
    for (size_t i = 0; i < tmp.size(); ++i) tmp[i] = f32_to_bf16(a_h[i]);
    LG_CHECK(hipMemcpy(g.a, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    tmp.resize((size_t)n * k);
    for (size_t i = 0; i < tmp.size(); ++i) tmp[i] = f32_to_bf16(bt_h[i]);
    LG_CHECK(hipMemcpy(g.bt, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    gemm_launch(g, 0, variant);
    LG_CHECK(hipDeviceSynchronize());
    LG_CHECK(hipGetLastError());
    LG_CHECK(hipMemcpy(c_out, g.c, (size_t)m * n * 4, hipMemcpyDeviceToHost));
    gemm_free(g);
    return 0;
}

int lg_gemm_bf16_verify(int device, const float* a_h, const float* bt_h,
                        float* c_out, int m, int n, int k)
{
    return lg_gemm_bf16_verify_variant(device, a_h, bt_h, c_out, m, n, k, 1);
}

// Streaming-triad bandwidth burn: duty-cycled HBM traffic at
// `target_util_pct` of wall time; `gb` working set (3 buffers summing to
// ~gb GiB). Returns achieved GB/s over the busy bursts in *gbps_out.
// The bandwidth-axis load for the multi-metric HPA (config 5).
int lg_bw_burn(int device, double target_util_pct, double seconds, double gb,
               double period_ms, volatile int* stop_flag, double* gbps_out)
{
    if (gb <= 0) gb = 6.0;
    if (period_ms <= 0) period_ms = 100.0;
    if (target_util_pct < 0) target_util_pct = 0;
    if (target_util_pct > 100) target_util_pct = 100;
    LG_CHECK(hipSetDevice(device));
    long n4 = (long)(gb * (1ull << 30) / 3.0 / 16.0);
    float4 *a, *b, *c;
    LG_CHECK(hipMalloc(&a, n4 * 16));
    LG_CHECK(hipMalloc(&b, n4 * 16));
    LG_CHECK(hipMalloc(&c, n4 * 16));
    LG_CHECK(hipMemset(a, 0x3f, n4 * 16));
    LG_CHECK(hipMemset(b, 0x3e, n4 * 16));
    int blocks = 8192;
    double busy_ms_total = 0, bytes_total = 0;
    double t_end = now_ms() + seconds * 1e3;
    while (now_ms() < t_end) {
        if (stop_flag && *stop_flag) break;
        double period_start = now_ms();
        double busy_until = period_start + period_ms * target_util_pct / 100.0;
        while (now_ms() < busy_until) {
            double t0 = now_ms();
            hipLaunchKernelGGL(triad_f32x4, dim3(blocks), dim3(256), 0, 0, a, b,
                               c, 1.5f, n4);
            LG_CHECK(hipDeviceSynchronize());
            busy_ms_total += now_ms() - t0;
            bytes_total += 3.0 * n4 * 16;
        }
        double rest = period_start + period_ms - now_ms();
        if (rest > 0)
            std::this_thread::sleep_for(
                std::chrono::duration<double, std::milli>(rest));
    }
    if (gbps_out)
        *gbps_out = busy_ms_total > 0 ? bytes_total / (busy_ms_total * 1e-3) / 1e9
                                      : 0;
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(c);
    return 0;
}

} // extern "C"

// Shared closed-loop duty engine: runs `launch4()` (4 queued kernel
// launches + sync, hipEvent-measured) in busy bursts of duty*period and
// trims the duty fraction by the measured GPU-active fraction per actual
// period. Used by the bf16, fp8 and mxfp4 burn entries.
template <typename LaunchFn>
static int duty_burn_loop(double target_util_pct, double seconds,
                          double period_ms, volatile int* stop_flag,
                          LaunchFn&& launch4)
{
    hipEvent_t ev0, ev1;
    LG_CHECK(hipEventCreate(&ev0));
    LG_CHECK(hipEventCreate(&ev1));
    double duty = target_util_pct / 100.0;
    const double duty_lo = duty > 0.25 ? duty - 0.25 : 0.0;
    const double duty_hi = duty + 0.25 < 1.0 ? duty + 0.25 : 1.0;
    const double kI = 0.004;
    double ema = -1;
    double t_end = now_ms() + seconds * 1e3;
    while (now_ms() < t_end) {
        if (stop_flag && *stop_flag) break;
        double period_start = now_ms();
        double busy_until = period_start + period_ms * duty;
        float active_ms = 0;
        while (now_ms() < busy_until) {
            LG_CHECK(hipEventRecord(ev0, 0));
            launch4();
            LG_CHECK(hipEventRecord(ev1, 0));
            LG_CHECK(hipDeviceSynchronize());
            float dt = 0;
            LG_CHECK(hipEventElapsedTime(&dt, ev0, ev1));
            active_ms += dt;
        }
        if (target_util_pct > 0 && target_util_pct < 100) {
            double actual_ms = now_ms() - period_start;
            if (actual_ms < period_ms) actual_ms = period_ms;
            double active_pct = active_ms / actual_ms * 100.0;
            ema = ema < 0 ? active_pct : 0.7 * ema + 0.3 * active_pct;
            duty += kI * (target_util_pct - ema);
            if (duty < duty_lo) duty = duty_lo;
            if (duty > duty_hi) duty = duty_hi;
        }
        double rest = period_start + period_ms - now_ms();
        if (rest > 0)
            std::this_thread::sleep_for(
                std::chrono::duration<double, std::milli>(rest));
    }
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    return 0;
}

extern "C" {

// Duty-cycled GEMM burn: aim at `target_util_pct` GPU-busy for `seconds`.
// Duty cycle over a `period_ms` window: run GEMM launches for duty*period,
// sleep the rest. Two mechanisms close the gap between wall-clock duty and
// the GRBM busy% that rocm-smi/the exporter report (round 1 measured an
// open-loop undershoot of ~0.72x: launch+sync gaps inside a "busy" burst
// are GPU-idle wall time):
//   * launches are BATCHED (4 queued back-to-back per sync) so intra-burst
//     gaps mostly vanish;
//   * the duty fraction is CLOSED-LOOP on the measured GPU-active time per
//     period (hipEvent elapsed time — the kernel-resident time GRBM
//     counts) over the period's ACTUAL length, trimmed with bounded
//     integral action. A sysfs gpu_busy_percent blend was tried and
//     removed: the controller reads right after a burst, so that sample
//     is busy-biased and settled ~8pp low (profiles/duty_closed_loop.md).
// Round-1 verdict item 8: the open-loop burn needed a +/-25pp test band;
// closed-loop targets +/-10pp.
// stop_flag: optional; polled between periods (set non-zero to stop early).
int lg_gemm_burn(int device, double target_util_pct, double seconds,
                 int m, int n, int k, double period_ms, volatile int* stop_flag)
{
    if (m <= 0) m = 4096;
    if (n <= 0) n = 4096;
    if (k <= 0) k = 4096;
    if (period_ms <= 0) period_ms = 100.0;
    const int burn_variant = gemm_effective_variant(m, n, 2);
    if (target_util_pct < 0) target_util_pct = 0;
    if (target_util_pct > 100) target_util_pct = 100;
    LG_CHECK(hipSetDevice(device));
    GemmBufs g;
    if (gemm_alloc(g, m, n, k, true)) return -1;
    // one calibration launch so the first period isn't all compile/warmup
    gemm_launch(g, 0, burn_variant);
    LG_CHECK(hipDeviceSynchronize());
    int rc = duty_burn_loop(target_util_pct, seconds, period_ms, stop_flag,
                            [&] {
                                for (int b = 0; b < 4; ++b)
                                    gemm_launch(g, 0, burn_variant);
                            });
    gemm_free(g);
    return rc;
}

} // extern "C"

// ---------------------------------------------------------------------------
// FP8 (E4M3) MFMA GEMM — the CDNA4 2x-peak datatype (gemm_fp8_256.hip)
// ---------------------------------------------------------------------------

// f32 -> OCP E4M3 (saturating, round-to-nearest-even via the FPU's default
// rounding). Max finite 448; subnormal step 2^-9.
static unsigned char f32_to_fp8_e4m3(float f)
{
    if (f != f) return 0x7f;  // NaN
    unsigned char sign = f < 0 ? 0x80 : 0;
    float af = f < 0 ? -f : f;
    if (af > 448.f) return sign | 0x7e;  // saturate to max finite
    int ef;
    float m = std::frexp(af, &ef);  // af = m * 2^ef, m in [0.5, 1)
    int k = ef - 1;                 // af = (2m) * 2^k, 2m in [1, 2)
    if (af == 0.f || k < -20) return sign;  // below half the min subnormal
    if (k < -6) {  // subnormal band: units of 2^-9, codes 1..8
        int q = (int)std::nearbyint(af * 512.f);
        if (q == 0) return sign;
        return (unsigned char)(sign | q);  // q==8 lands on min normal 0x08
    }
    int q = (int)std::nearbyint(std::ldexp(af, 3 - k));  // in [8, 16]
    if (q == 16) {
        ++k;
        q = 8;
        if (k > 8) return sign | 0x7e;
    }
    return (unsigned char)(sign | ((k + 7) << 3) | (q - 8));
}

static float fp8_e4m3_to_f32(unsigned char v)
{
    int sign = v >> 7;
    int exp = (v >> 3) & 0xf;
    int man = v & 7;
    float r;
    if (exp == 0)
        r = man * (1.f / 512.f);
    else if (exp == 15 && man == 7)
        r = __builtin_nanf("");
    else
        r = (1.f + man / 8.f) * std::ldexp(1.f, exp - 7);
    return sign ? -r : r;
}

struct Fp8GemmBufs {
    unsigned char* a = nullptr;
    unsigned char* bt = nullptr;
    float* c = nullptr;
    int m = 0, n = 0, k = 0;
};

static int fp8_gemm_alloc(Fp8GemmBufs& g, int m, int n, int k, bool fill_random)
{
    LG_CHECK(hipMalloc(&g.a, (size_t)m * k));
    LG_CHECK(hipMalloc(&g.bt, (size_t)n * k));
    LG_CHECK(hipMalloc(&g.c, (size_t)m * n * 4));
    g.m = m; g.n = n; g.k = k;
    if (fill_random) {
        // random fp8 in [-1, 1): DVFS-honest load (playbook rule 25)
        size_t na = (size_t)m * k, nb = (size_t)n * k;
        std::vector<unsigned char> h(na > nb ? na : nb);
        uint32_t st = 0x2468ace1u;
        for (size_t i = 0; i < h.size(); ++i) {
            st = st * 1664525u + 1013904223u;
            float f = ((st >> 8) & 0xffff) / 32768.0f - 1.0f;
            h[i] = f32_to_fp8_e4m3(f);
        }
        LG_CHECK(hipMemcpy(g.a, h.data(), na, hipMemcpyHostToDevice));
        LG_CHECK(hipMemcpy(g.bt, h.data(), nb, hipMemcpyHostToDevice));
    }
    return 0;
}

static void fp8_gemm_free(Fp8GemmBufs& g)
{
    (void)hipFree(g.a); (void)hipFree(g.bt); (void)hipFree(g.c);
    g = Fp8GemmBufs{};
}

static int fp8_gemm_launch(const Fp8GemmBufs& g, hipStream_t stream, int raster)
{
    int n_tiles = (g.m / 256) * (g.n / 256);
    int blocks = n_tiles < 2048 ? n_tiles : 2048;
    int tiles_per_cta = (n_tiles + blocks - 1) / blocks;
    // raster: 1 = product (4x4 super-tile), 0 = linear, 2 = deep-B rotation
    hipLaunchKernelGGL(raster == 2   ? gemm_fp8_tn_256_db
                       : raster == 1 ? gemm_fp8_tn_256
                                     : gemm_fp8_tn_256_nr,
                       dim3(blocks), dim3(512), 0, stream, g.a, g.bt, g.c,
                       g.m, g.n, g.k, tiles_per_cta);
    return 0;
}

extern "C" {

// Timed fp8 GEMM: mean ms + TF/s over `iters` launches. raster: 4x4
// super-tile rasterization on (1, the product config) or off (0).
int lg_gemm_fp8_bench(int device, int m, int n, int k, int warmup, int iters,
                      int raster, double* ms_out, double* tflops_out)
{
    if (m % 256 || n % 256 || k % 128) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "fp8 gemm dims must be multiples of 256/256/128");
        return -1;
    }
    LG_CHECK(hipSetDevice(device));
    Fp8GemmBufs g;
    if (fp8_gemm_alloc(g, m, n, k, true)) return -1;
    for (int i = 0; i < warmup; ++i) fp8_gemm_launch(g, 0, raster);
    LG_CHECK(hipDeviceSynchronize());
    double t0 = now_ms();
    for (int i = 0; i < iters; ++i) fp8_gemm_launch(g, 0, raster);
    LG_CHECK(hipDeviceSynchronize());
    double t1 = now_ms();
    double ms = (t1 - t0) / iters;
    if (ms_out) *ms_out = ms;
    if (tflops_out) *tflops_out = 2.0 * m * n * k / (ms * 1e-3) / 1e12;
    fp8_gemm_free(g);
    return 0;
}

// Numerics entry: quantizes the f32 inputs to E4M3, runs the kernel, and
// writes C plus the DEQUANTIZED inputs (aq/btq, f32) back so the caller
// can compute the exact reference matmul on what the GPU actually saw.
int lg_gemm_fp8_verify(int device, const float* a_h, const float* bt_h,
                       float* c_out, float* aq_out, float* btq_out,
                       int m, int n, int k)
{
    if (m % 256 || n % 256 || k % 128) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "fp8 gemm dims must be multiples of 256/256/128");
        return -1;
    }
    LG_CHECK(hipSetDevice(device));
    Fp8GemmBufs g;
    if (fp8_gemm_alloc(g, m, n, k, false)) return -1;
    std::vector<unsigned char> q((size_t)m * k);
    for (size_t i = 0; i < q.size(); ++i) {
        q[i] = f32_to_fp8_e4m3(a_h[i]);
        if (aq_out) aq_out[i] = fp8_e4m3_to_f32(q[i]);
    }
    LG_CHECK(hipMemcpy(g.a, q.data(), q.size(), hipMemcpyHostToDevice));
    q.resize((size_t)n * k);
    for (size_t i = 0; i < q.size(); ++i) {
        q[i] = f32_to_fp8_e4m3(bt_h[i]);
        if (btq_out) btq_out[i] = fp8_e4m3_to_f32(q[i]);
    }
    LG_CHECK(hipMemcpy(g.bt, q.data(), q.size(), hipMemcpyHostToDevice));
    fp8_gemm_launch(g, 0, 1);
    LG_CHECK(hipDeviceSynchronize());
    LG_CHECK(hipMemcpy(c_out, g.c, (size_t)m * n * 4, hipMemcpyDeviceToHost));
    fp8_gemm_free(g);
    return 0;
}

// variant form: raster 0/1/2 selects the kernel (2 = deep-B rotation).
int lg_gemm_fp8_verify_variant(int device, const float* a_h, const float* bt_h,
                               float* c_out, float* aq_out, float* btq_out,
                               int m, int n, int k, int raster)
{
    if (m % 256 || n % 256 || k % 128) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "fp8 gemm dims must be multiples of 256/256/128");
        return -1;
    }
    LG_CHECK(hipSetDevice(device));
    Fp8GemmBufs g;
    if (fp8_gemm_alloc(g, m, n, k, false)) return -1;
    std::vector<unsigned char> q((size_t)m * k);
    for (size_t i = 0; i < q.size(); ++i) {
        q[i] = f32_to_fp8_e4m3(a_h[i]);
        if (aq_out) aq_out[i] = fp8_e4m3_to_f32(q[i]);
    }
    LG_CHECK(hipMemcpy(g.a, q.data(), q.size(), hipMemcpyHostToDevice));
    q.resize((size_t)n * k);
    for (size_t i = 0; i < q.size(); ++i) {
        q[i] = f32_to_fp8_e4m3(bt_h[i]);
        if (btq_out) btq_out[i] = fp8_e4m3_to_f32(q[i]);
    }
    LG_CHECK(hipMemcpy(g.bt, q.data(), q.size(), hipMemcpyHostToDevice));
    fp8_gemm_launch(g, 0, raster);
    LG_CHECK(hipDeviceSynchronize());
    LG_CHECK(hipMemcpy(c_out, g.c, (size_t)m * n * 4, hipMemcpyDeviceToHost));
    fp8_gemm_free(g);
    return 0;
}

// fp8 (E4M3) variant of the burn: same closed-loop duty engine over the
// fp8 MFMA kernel — the 2x-peak datatype's power/clock profile as a load.
int lg_gemm_fp8_burn(int device, double target_util_pct, double seconds,
                     int m, int n, int k, double period_ms,
                     volatile int* stop_flag)
{
    if (m <= 0) m = 4096;
    if (n <= 0) n = 4096;
    if (k <= 0) k = 4096;
    if (period_ms <= 0) period_ms = 100.0;
    if (m % 256 || n % 256 || k % 128) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "fp8 gemm dims must be multiples of 256/256/128");
        return -1;
    }
    if (target_util_pct < 0) target_util_pct = 0;
    if (target_util_pct > 100) target_util_pct = 100;
    LG_CHECK(hipSetDevice(device));
    Fp8GemmBufs g;
    if (fp8_gemm_alloc(g, m, n, k, true)) return -1;
    fp8_gemm_launch(g, 0, 1);
    LG_CHECK(hipDeviceSynchronize());
    int rc = duty_burn_loop(target_util_pct, seconds, period_ms, stop_flag,
                            [&] {
                                for (int b = 0; b < 4; ++b)
                                    fp8_gemm_launch(g, 0, 1);
                            });
    fp8_gemm_free(g);
    return rc;
}

} // extern "C"


// ---------------------------------------------------------------------------
// MXFP4 (E2M1 + E8M0 block scale) MFMA GEMM — the CDNA4 4x-peak datatype
// (gemm_mxfp4_256.hip). Public operand format and quantizer: mxfp4_host.h.
// ---------------------------------------------------------------------------

struct Mxfp4GemmBufs {
    unsigned char* a = nullptr;   // [m][k/2]
    unsigned char* bt = nullptr;  // [n][k/2]
    int* sa = nullptr;            // [m/64][k/128][64], mxfp4::shuffle_scales
    int* sb = nullptr;            // [n/64][k/128][64]
    float* c = nullptr;
    int m = 0, n = 0, k = 0;
};

static bool mxfp4_dims_ok(int m, int n, int k)
{
    if (m <= 0 || n <= 0 || k <= 0 || m % 256 || n % 256 || k % 256) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "mxfp4 gemm dims must be positive multiples of "
                      "256/256/256");
        return false;
    }
    return true;
}

static int mxfp4_gemm_alloc(Mxfp4GemmBufs& g, int m, int n, int k,
                            bool fill_random)
{
    const size_t na = (size_t)m * k / 2, nb = (size_t)n * k / 2;
    const size_t nsa = (size_t)m * k / 32, nsb = (size_t)n * k / 32;
    LG_CHECK(hipMalloc(&g.a, na));
    LG_CHECK(hipMalloc(&g.bt, nb));
    LG_CHECK(hipMalloc(&g.sa, nsa));
    LG_CHECK(hipMalloc(&g.sb, nsb));
    LG_CHECK(hipMalloc(&g.c, (size_t)m * n * 4));
    g.m = m; g.n = n; g.k = k;
    if (fill_random) {
        // random E2M1 codes (every byte is a valid pair) and scale bytes in
        // 125..129, never zeros: DVFS-honest load (playbook rule 25)
        std::vector<unsigned char> h(na > nb ? na : nb);
        uint32_t st = 0x1357bdf1u;
        for (size_t i = 0; i < h.size(); ++i) {
            st = st * 1664525u + 1013904223u;
            h[i] = (unsigned char)(st >> 16);
        }
        LG_CHECK(hipMemcpy(g.a, h.data(), na, hipMemcpyHostToDevice));
        LG_CHECK(hipMemcpy(g.bt, h.data(), nb, hipMemcpyHostToDevice));
        h.resize(nsa > nsb ? nsa : nsb);
        for (size_t i = 0; i < h.size(); ++i) {
            st = st * 1664525u + 1013904223u;
            h[i] = (unsigned char)(125 + (st >> 16) % 5);
        }
        LG_CHECK(hipMemcpy(g.sa, h.data(), nsa, hipMemcpyHostToDevice));
        LG_CHECK(hipMemcpy(g.sb, h.data(), nsb, hipMemcpyHostToDevice));
    }
    return 0;
}

static void mxfp4_gemm_free(Mxfp4GemmBufs& g)
{
    (void)hipFree(g.a); (void)hipFree(g.bt); (void)hipFree(g.sa);
    (void)hipFree(g.sb); (void)hipFree(g.c);
    g = Mxfp4GemmBufs{};
}

// max_ctas > 0 caps the grid (each CTA then loops over several tiles).
static int mxfp4_gemm_launch(const Mxfp4GemmBufs& g, hipStream_t stream,
                             int max_ctas = 0)
{
    int n_tiles = (g.m / 256) * (g.n / 256);
    int blocks = n_tiles < 2048 ? n_tiles : 2048;
    if (max_ctas > 0 && blocks > max_ctas) blocks = max_ctas;
    int tiles_per_cta = (n_tiles + blocks - 1) / blocks;
    hipLaunchKernelGGL(gemm_mxfp4_tn_256, dim3(blocks), dim3(512), 0, stream,
                       g.a, g.bt, g.sa, g.sb, g.c, g.m, g.n, g.k,
                       tiles_per_cta);
    return 0;
}

// Quantize one f32 operand, upload elements + device-layout scales, and
// hand back the dequantized values.
static int mxfp4_upload_operand(const float* x_h, int rows, int k,
                                unsigned char* elems_d, int* scales_d,
                                float* deq_out)
{
    std::vector<unsigned char> packed((size_t)rows * k / 2);
    std::vector<unsigned char> scales((size_t)rows * k / 32);
    if (mxfp4::quantize(x_h, rows, k, packed.data(), scales.data(), deq_out,
                        g_last_error, sizeof(g_last_error)))
        return -1;
    std::vector<unsigned char> shuffled(scales.size());
    mxfp4::shuffle_scales(scales.data(), rows, k, shuffled.data());
    LG_CHECK(hipMemcpy(elems_d, packed.data(), packed.size(),
                       hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(scales_d, shuffled.data(), shuffled.size(),
                       hipMemcpyHostToDevice));
    return 0;
}

extern "C" {

// Timed MXFP4 GEMM: mean ms + TF/s (2*M*N*K) over `iters` launches.
int lg_gemm_mxfp4_bench(int device, int m, int n, int k, int warmup, int iters,
                        double* ms_out, double* tflops_out)
{
    if (!mxfp4_dims_ok(m, n, k)) return -1;
    LG_CHECK(hipSetDevice(device));
    Mxfp4GemmBufs g;
    if (mxfp4_gemm_alloc(g, m, n, k, true)) return -1;
    for (int i = 0; i < warmup; ++i) mxfp4_gemm_launch(g, 0);
    LG_CHECK(hipDeviceSynchronize());
    double t0 = now_ms();
    for (int i = 0; i < iters; ++i) mxfp4_gemm_launch(g, 0);
    LG_CHECK(hipDeviceSynchronize());
    double t1 = now_ms();
    double ms = (t1 - t0) / iters;
    if (ms_out) *ms_out = ms;
    if (tflops_out) *tflops_out = 2.0 * m * n * k / (ms * 1e-3) / 1e12;
    mxfp4_gemm_free(g);
    return 0;
}

// Numerics entry: quantizes the f32 inputs to MXFP4 with the shared host
// quantizer, runs the kernel, and writes C plus the DEQUANTIZED inputs
// (aq/btq, f32) back so the caller can compute the exact reference on what
// the GPU actually multiplied. max_ctas > 0 caps the grid so a small shape
// exercises the tiles-per-CTA loop; 0 = the normal grid.
int lg_gemm_mxfp4_verify(int device, const float* a_h, const float* bt_h,
                         float* c_out, float* aq_out, float* btq_out,
                         int m, int n, int k, int max_ctas)
{
    if (!mxfp4_dims_ok(m, n, k)) return -1;
    LG_CHECK(hipSetDevice(device));
    Mxfp4GemmBufs g;
    if (mxfp4_gemm_alloc(g, m, n, k, false)) return -1;
    int rc = mxfp4_upload_operand(a_h, m, k, g.a, g.sa, aq_out);
    if (!rc) rc = mxfp4_upload_operand(bt_h, n, k, g.bt, g.sb, btq_out);
    if (rc) {
        mxfp4_gemm_free(g);
        return -1;
    }
    mxfp4_gemm_launch(g, 0, max_ctas);
    LG_CHECK(hipDeviceSynchronize());
    LG_CHECK(hipGetLastError());
    LG_CHECK(hipMemcpy(c_out, g.c, (size_t)m * n * 4, hipMemcpyDeviceToHost));
    mxfp4_gemm_free(g);
    return 0;
}

// MXFP4 variant of the burn: same closed-loop duty engine over the
// block-scaled fp4 MFMA kernel — the load shape of an MXFP4 serving pod.
int lg_gemm_mxfp4_burn(int device, double target_util_pct, double seconds,
                       int m, int n, int k, double period_ms,
                       volatile int* stop_flag)
{
    if (m <= 0) m = 4096;
    if (n <= 0) n = 4096;
    if (k <= 0) k = 4096;
    if (period_ms <= 0) period_ms = 100.0;
    if (!mxfp4_dims_ok(m, n, k)) return -1;
    if (target_util_pct < 0) target_util_pct = 0;
    if (target_util_pct > 100) target_util_pct = 100;
    LG_CHECK(hipSetDevice(device));
    Mxfp4GemmBufs g;
    if (mxfp4_gemm_alloc(g, m, n, k, true)) return -1;
    mxfp4_gemm_launch(g, 0);
    LG_CHECK(hipDeviceSynchronize());
    int rc = duty_burn_loop(target_util_pct, seconds, period_ms, stop_flag,
                            [&] {
                                for (int b = 0; b < 4; ++b)
                                    mxfp4_gemm_launch(g, 0);
                            });
    mxfp4_gemm_free(g);
    return rc;
}

} // extern "C"


// ---------------------------------------------------------------------------
// Decode-phase MXFP4 weight streaming (gemm_mxfp4_decode.hip): a skinny-M
// a4w4 GEMM over a ring of `layers` weight matrices W[L][N][K] and one
// activation block X[M][K], 1 <= M <= 64. Memory-bound by design: each
// weight byte is read once per step.
// ---------------------------------------------------------------------------

struct DecodeBufs {
    unsigned char* x = nullptr;  // [mp][k/2], mp = m rounded up to 16
    int* sx = nullptr;           // [k/128][64], one 64-row group
    unsigned char* w = nullptr;  // [layers][n][k/2]
    int* sw = nullptr;           // [layers*n/64][k/128][64]
    float* c = nullptr;          // [layers][m][n]
    float* part = nullptr;       // [k_splits][layers][m][n] if k_splits > 1
    int m = 0, mp = 0, n = 0, k = 0, layers = 0, k_splits = 1;
};

static bool decode_dims_ok(int m, int n, int k, int layers, int k_splits)
{
    if (m < 1 || m > 64 || n <= 0 || n % 64 || k <= 0 || k % 128 ||
        layers < 1) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "mxfp4 decode needs 1 <= m <= 64, n a positive "
                      "multiple of 64, k of 128, layers >= 1");
        return false;
    }
    if (k_splits < 0 || (k_splits > 0 && (k / 128) % k_splits)) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "mxfp4 decode: k_splits %d must divide k/128 = %d",
                      k_splits, k / 128);
        return false;
    }
    return true;
}

// Product heuristic: a CTA is one (layer, 64-row group, K slice). Split K
// across CTAs until the grid reaches two CTAs per CU (the chip has 256),
// as long as a slice keeps at least 8 k-steps (two per wave).
static int decode_pick_k_splits(int n, int k, int layers)
{
    const long ctas = (long)layers * (n / 64);
    const int ksteps = k / 128;
    int s = 1;
    while (ctas * s < 512 && ksteps % (s * 2) == 0 && ksteps / (s * 2) >= 8)
        s *= 2;
    return s;
}

static void decode_free(DecodeBufs& d)
{
    (void)hipFree(d.x); (void)hipFree(d.sx); (void)hipFree(d.w);
    (void)hipFree(d.sw); (void)hipFree(d.c); (void)hipFree(d.part);
    d = DecodeBufs{};
}

// k_splits: 0 = heuristic. Dimensions must have passed decode_dims_ok.
static int decode_alloc(DecodeBufs& d, int m, int n, int k, int layers,
                        int k_splits)
{
    d.m = m; d.mp = (m + 15) / 16 * 16; d.n = n; d.k = k; d.layers = layers;
    d.k_splits = k_splits > 0 ? k_splits : decode_pick_k_splits(n, k, layers);
    const size_t c_bytes = (size_t)layers * m * n * 4;
    LG_CHECK(hipMalloc(&d.x, (size_t)d.mp * k / 2));
    LG_CHECK(hipMalloc(&d.sx, (size_t)64 * k / 32));
    LG_CHECK(hipMalloc(&d.w, (size_t)layers * n * k / 2));
    LG_CHECK(hipMalloc(&d.sw, (size_t)layers * n * k / 32));
    LG_CHECK(hipMalloc(&d.c, c_bytes));
    if (d.k_splits > 1) LG_CHECK(hipMalloc(&d.part, c_bytes * d.k_splits));
    return 0;
}

// One decode step: every layer of the ring against X. One launch for the
// ring, plus the ordered slice sum when K is split across CTAs. Verify,
// bench and burn all run this function.
static void decode_step(const DecodeBufs& d, hipStream_t stream)
{
    const int blocks = d.layers * (d.n / 64) * d.k_splits;
    float* out = d.k_splits > 1 ? d.part : d.c;
    auto kern = d.mp == 16   ? decode_mxfp4_m16
                : d.mp == 32 ? decode_mxfp4_m32
                : d.mp == 48 ? decode_mxfp4_m48
                             : decode_mxfp4_m64;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, stream, d.x, d.sx,
                       d.w, d.sw, out, d.m, d.n, d.k, d.layers, d.k_splits);
    if (d.k_splits > 1) {
        const long n4 = (long)d.layers * d.m * d.n / 4;
        long rb = (n4 + 255) / 256;
        if (rb > 2048) rb = 2048;
        hipLaunchKernelGGL(decode_mxfp4_reduce, dim3((int)rb), dim3(256), 0,
                           stream, (const float4*)d.part, (float4*)d.c, n4,
                           d.k_splits);
    }
}

static double decode_weight_bytes(const DecodeBufs& d)
{
    return (double)d.layers * ((double)d.n * d.k / 2 + (double)d.n * d.k / 32);
}

// Random codes and scale bytes 125..129 (DVFS-honest, as mxfp4_gemm_alloc).
// One layer is generated on the host and replicated on the device.
static int decode_fill_random(DecodeBufs& d)
{
    const size_t wl = (size_t)d.n * d.k / 2, swl = (size_t)d.n * d.k / 32;
    const size_t xb = (size_t)d.mp * d.k / 2, sxb = (size_t)64 * d.k / 32;
    std::vector<unsigned char> h(wl > xb ? wl : xb);
    uint32_t st = 0x0decade1u;
    for (size_t i = 0; i < h.size(); ++i) {
        st = st * 1664525u + 1013904223u;
        h[i] = (unsigned char)(st >> 16);
    }
    LG_CHECK(hipMemcpy(d.w, h.data(), wl, hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(d.x, h.data(), xb, hipMemcpyHostToDevice));
    h.resize(swl > sxb ? swl : sxb);
    for (size_t i = 0; i < h.size(); ++i) {
        st = st * 1664525u + 1013904223u;
        h[i] = (unsigned char)(125 + (st >> 16) % 5);
    }
    LG_CHECK(hipMemcpy(d.sw, h.data(), swl, hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(d.sx, h.data(), sxb, hipMemcpyHostToDevice));
    for (int l = 1; l < d.layers; ++l) {
        LG_CHECK(hipMemcpy(d.w + l * wl, d.w, wl, hipMemcpyDeviceToDevice));
        LG_CHECK(hipMemcpy((unsigned char*)d.sw + l * swl, d.sw, swl,
                           hipMemcpyDeviceToDevice));
    }
    return 0;
}

static void decode_defaults(int& m, int& n, int& k, int& layers)
{
    if (m <= 0) m = 16;
    if (n <= 0) n = 8192;
    if (k <= 0) k = 8192;
    if (layers <= 0) layers = 16;
}

extern "C" {

// Numerics entry: x_h[m][k] and w_h[layers][n][k] (f32) are quantized with
// the shared host quantizer; writes c_out[layers][m][n] and the
// DEQUANTIZED operands xq_out/wq_out (same convention as
// lg_gemm_mxfp4_verify). k_splits: 0 = the product heuristic, > 0 forces
// that many K slices across CTAs (must divide k/128) so a small shape
// reaches every combine path.
int lg_decode_mxfp4_verify(int device, const float* x_h, const float* w_h,
                           float* c_out, float* xq_out, float* wq_out, int m,
                           int n, int k, int layers, int k_splits)
{
    if (!decode_dims_ok(m, n, k, layers, k_splits)) return -1;
    LG_CHECK(hipSetDevice(device));
    const long wrows = (long)layers * n;
    const int kb = k / 32;
    // X: elements padded to mp rows with zero codes, scales to one 64-row
    // group with byte 127
    const int mp = (m + 15) / 16 * 16;
    std::vector<unsigned char> xe((size_t)mp * k / 2, 0);
    std::vector<unsigned char> xs((size_t)64 * kb, 127);
    std::vector<unsigned char> xsh(xs.size());
    if (mxfp4::quantize(x_h, m, k, xe.data(), xs.data(), xq_out, g_last_error,
                        sizeof(g_last_error)))
        return -1;
    mxfp4::shuffle_scales(xs.data(), 64, k, xsh.data());
    std::vector<unsigned char> we((size_t)wrows * k / 2);
    std::vector<unsigned char> ws((size_t)wrows * kb);
    std::vector<unsigned char> wsh(ws.size());
    if (mxfp4::quantize(w_h, wrows, k, we.data(), ws.data(), wq_out,
                        g_last_error, sizeof(g_last_error)))
        return -1;
    mxfp4::shuffle_scales(ws.data(), (int)wrows, k, wsh.data());

    DecodeBufs d;
    int rc = decode_alloc(d, m, n, k, layers, k_splits);
    auto up = [&](void* dst, const std::vector<unsigned char>& src) {
        LG_CHECK(hipMemcpy(dst, src.data(), src.size(), hipMemcpyHostToDevice));
        return 0;
    };
    if (!rc) rc = up(d.x, xe);
    if (!rc) rc = up(d.sx, xsh);
    if (!rc) rc = up(d.w, we);
    if (!rc) rc = up(d.sw, wsh);
    auto run = [&] {
        decode_step(d, 0);
        LG_CHECK(hipDeviceSynchronize());
        LG_CHECK(hipGetLastError());
        LG_CHECK(hipMemcpy(c_out, d.c, (size_t)layers * m * n * 4,
                           hipMemcpyDeviceToHost));
        return 0;
    };
    if (!rc) rc = run();
    decode_free(d);
    return rc;
}

// Timed decode steps: mean ms per step (one pass over the ring) and the
// weight stream rate, layers * (N*K/2 + N*K/32) bytes / step time, GB/s.
int lg_decode_mxfp4_bench(int device, int m, int n, int k, int layers,
                          int warmup, int iters, double* ms_per_step_out,
                          double* weight_gbps_out)
{
    decode_defaults(m, n, k, layers);
    if (iters < 1) iters = 1;
    if (!decode_dims_ok(m, n, k, layers, 0)) return -1;
    LG_CHECK(hipSetDevice(device));
    DecodeBufs d;
    auto run = [&] {
        if (decode_alloc(d, m, n, k, layers, 0)) return -1;
        if (decode_fill_random(d)) return -1;
        for (int i = 0; i < warmup; ++i) decode_step(d, 0);
        LG_CHECK(hipDeviceSynchronize());
        double t0 = now_ms();
        for (int i = 0; i < iters; ++i) decode_step(d, 0);
        LG_CHECK(hipDeviceSynchronize());
        double ms = (now_ms() - t0) / iters;
        LG_CHECK(hipGetLastError());
        if (ms_per_step_out) *ms_per_step_out = ms;
        if (weight_gbps_out)
            *weight_gbps_out = decode_weight_bytes(d) / (ms * 1e-3) / 1e9;
        return 0;
    };
    int rc = run();
    decode_free(d);
    return rc;
}

// Decode burn: the shared closed-loop duty engine over decode steps — the
// load shape of a small-batch MXFP4 serving pod (busy%, bandwidth-bound).
// *weight_gbps_out: weight bytes streamed / GPU-active time of the bursts.
int lg_decode_mxfp4_burn(int device, double target_util_pct, double seconds,
                         int m, int n, int k, int layers, double period_ms,
                         volatile int* stop_flag, double* weight_gbps_out)
{
    decode_defaults(m, n, k, layers);
    if (period_ms <= 0) period_ms = 100.0;
    if (!decode_dims_ok(m, n, k, layers, 0)) return -1;
    if (target_util_pct < 0) target_util_pct = 0;
    if (target_util_pct > 100) target_util_pct = 100;
    LG_CHECK(hipSetDevice(device));
    DecodeBufs d;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double active_ms = 0, steps = 0;
    auto run = [&] {
        if (decode_alloc(d, m, n, k, layers, 0)) return -1;
        if (decode_fill_random(d)) return -1;
        LG_CHECK(hipEventCreate(&e0));
        LG_CHECK(hipEventCreate(&e1));
        // calibration step: sizes the burst so that a busy slice of the
        // default 100 ms period holds several launches
        LG_CHECK(hipEventRecord(e0, 0));
        decode_step(d, 0);
        LG_CHECK(hipEventRecord(e1, 0));
        LG_CHECK(hipDeviceSynchronize());
        float step_ms = 0;
        LG_CHECK(hipEventElapsedTime(&step_ms, e0, e1));
        int per_burst = step_ms > 0 ? (int)(2.0f / step_ms) : 4;
        if (per_burst < 4) per_burst = 4;
        if (per_burst > 64) per_burst = 64;
        // rate: each burst is bracketed by events of its own, read back
        // at the next burst (the engine has synchronised by then), so the
        // engine itself stays as it is
        bool pending = false;
        int rc = duty_burn_loop(
            target_util_pct, seconds, period_ms, stop_flag, [&] {
                float dt = 0;
                if (pending &&
                    hipEventElapsedTime(&dt, e0, e1) == hipSuccess) {
                    active_ms += dt;
                    steps += per_burst;
                }
                (void)hipEventRecord(e0, 0);
                for (int b = 0; b < per_burst; ++b) decode_step(d, 0);
                (void)hipEventRecord(e1, 0);
                pending = true;
            });
        if (rc) return rc;
        LG_CHECK(hipDeviceSynchronize());
        if (pending) {
            float dt = 0;
            LG_CHECK(hipEventElapsedTime(&dt, e0, e1));
            active_ms += dt;
            steps += per_burst;
        }
        LG_CHECK(hipGetLastError());
        return 0;
    };
    int rc = run();
    if (weight_gbps_out)
        *weight_gbps_out =
            active_ms > 0
                ? steps * decode_weight_bytes(d) / (active_ms * 1e-3) / 1e9
                : 0;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    decode_free(d);
    return rc;
}

} // extern "C"
