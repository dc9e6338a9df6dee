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
//   * lg_attn_decode_*(): the other half of a decode pod's HBM traffic —
//     single-token attention over a contiguous bf16 KV cache with ragged
//     sequence lengths and grouped-query heads (attn_decode.hip); its bytes
//     per step grow with batch and context.
//   * lg_*_verify(): run one kernel on caller-provided host data so tests
//     can check numerics against a plain fp32 reference.
//
// The C ABI is declared and documented in loadgen_api.h: consumed by
// loadgen_main.cpp (CLI) and by mi355x_gpu_hpa/loadgen (ctypes).
//
// Every device buffer and event is owned by a DevBuf / DevEvent, so the
// early return inside LG_CHECK releases what the entry had allocated: this
// library lives in a resident process that runs for days.

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "loadgen_api.h"
#include "mxfp4_host.h"

extern "C" __global__ void vector_add_f32(const float*, const float*, float*, int);
extern "C" __global__ void vector_add_f32x4(const float4*, const float4*, float4*, int);
extern "C" __global__ void triad_f32x4(const float4*, const float4*, float4*, float,
                                       long);
#define LG_BF16_KERNEL(NAME)                                                  \
    extern "C" __global__ void NAME(const unsigned short*,                    \
                                    const unsigned short*, float*, int, int,  \
                                    int, int)
LG_BF16_KERNEL(gemm_bf16_tn);
LG_BF16_KERNEL(gemm_bf16_tn_linear);
LG_BF16_KERNEL(gemm_bf16_tn_256);
LG_BF16_KERNEL(gemm_bf16_tn_256_d1);
LG_BF16_KERNEL(gemm_bf16_tn_256_d2);
LG_BF16_KERNEL(gemm_bf16_tn_256_d4);
LG_BF16_KERNEL(gemm_bf16_tn_256_d5);
LG_BF16_KERNEL(gemm_bf16_tn_256_d6);
LG_BF16_KERNEL(gemm_bf16_tn_256_d7);
LG_BF16_KERNEL(gemm_bf16_tn_256_d8);
LG_BF16_KERNEL(gemm_bf16_tn_256_d9);
LG_BF16_KERNEL(gemm_bf16_tn_256_d9e);
LG_BF16_KERNEL(gemm_bf16_tn_256_d9nr);
LG_BF16_KERNEL(gemm_bf16_tn_256_d9w);
LG_BF16_KERNEL(gemm_bf16_tn_256_d14);
LG_BF16_KERNEL(gemm_bf16_tn_256_d18);
LG_BF16_KERNEL(gemm_bf16_tn_256_d19);
LG_BF16_KERNEL(gemm_bf16_tn_256_d20);
LG_BF16_KERNEL(gemm_bf16_tn_256_d21);
LG_BF16_KERNEL(gemm_bf16_tn_256_soft);
LG_BF16_KERNEL(gemm_bf16_tn_256_w32);
#undef LG_BF16_KERNEL
#define LG_FP8_KERNEL(NAME)                                                   \
    extern "C" __global__ void NAME(const unsigned char*,                     \
                                    const unsigned char*, float*, int, int,   \
                                    int, int)
LG_FP8_KERNEL(gemm_fp8_tn_256);
LG_FP8_KERNEL(gemm_fp8_tn_256_db);
LG_FP8_KERNEL(gemm_fp8_tn_256_nr);
#undef LG_FP8_KERNEL
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
extern "C" __global__ void attn_decode_bf16(
    const unsigned short*, const unsigned short*, const unsigned short*,
    const int*, float*, float*, float*, float*, float*, int, int, int, int, int,
    int, float);
extern "C" __global__ void attn_decode_merge(const float*, const float*,
                                             const float*, float*, float*, int);

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

// ---------------------------------------------------------------------------
// Shared host machinery
// ---------------------------------------------------------------------------

// Move-only owner of one device allocation: hipFree on scope exit.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    operator T*() const { return p; }
};

// The same for a hipEvent_t.
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(DevEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() { if (e) (void)hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }
    operator hipEvent_t() const { return e; }
};

// Operand fill for bench and burn: one LCG stream per entry family, never
// zeros — DVFS-honest load (zero-filled operands clock higher and overstate
// TF/s — playbook §5.4 rule 25). Operand content moves clocks and power, so
// the seeds and the byte formulas below are part of what a measurement
// means: they stay as they are.
static inline uint32_t lcg_next(uint32_t& st)
{
    return st = st * 1664525u + 1013904223u;
}
static inline float lcg_unit(uint32_t& st)  // in [-1, 1)
{
    return ((lcg_next(st) >> 8) & 0xffff) / 32768.0f - 1.0f;
}
template <typename T, typename Gen>
static void lcg_fill(std::vector<T>& h, uint32_t& st, Gen gen)
{
    for (T& v : h) v = gen(st);
}

// Fill two operands (a: na elements, b: nb) from one host image of the
// longer one, so both start with the same values.
template <typename T, typename Gen>
static int fill_pair(T* a, size_t na, T* b, size_t nb, uint32_t& st, Gen gen)
{
    std::vector<T> h(na > nb ? na : nb);
    lcg_fill(h, st, gen);
    LG_CHECK(hipMemcpy(a, h.data(), na * sizeof(T), hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(b, h.data(), nb * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// MXFP4 operands: random E2M1 codes (every byte is a valid pair), then, on
// the same stream, scale bytes in 125..129.
static int fill_mxfp4_pair(uint32_t seed, unsigned char* ea, size_t nea,
                           unsigned char* eb, size_t neb, int* sa, size_t nsa,
                           int* sb, size_t nsb)
{
    uint32_t st = seed;
    if (fill_pair(ea, nea, eb, neb, st, [](uint32_t& s) {
            return (unsigned char)(lcg_next(s) >> 16);
        }))
        return -1;
    return fill_pair((unsigned char*)sa, nsa, (unsigned char*)sb, nsb, st,
                     [](uint32_t& s) {
                         return (unsigned char)(125 + (lcg_next(s) >> 16) % 5);
                     });
}

// Grid of a tiled GEMM: one CTA per output tile up to 2048 CTAs (or
// max_ctas, if > 0), each looping over tiles_per_cta tiles.
struct TileGrid {
    int blocks, tiles_per_cta;
};
static TileGrid tile_grid(int m, int n, int tile, int max_ctas = 0)
{
    const int n_tiles = (m / tile) * (n / tile);
    int blocks = n_tiles < 2048 ? n_tiles : 2048;
    if (max_ctas > 0 && blocks > max_ctas) blocks = max_ctas;
    return {blocks, (n_tiles + blocks - 1) / blocks};
}

// Bench loop: `warmup` untimed launches, then the mean wall ms of `iters`
// back-to-back ones.
template <typename LaunchFn>
static int timed_launches(int warmup, int iters, LaunchFn&& launch,
                          double* ms_out)
{
    for (int i = 0; i < warmup; ++i) launch();
    LG_CHECK(hipDeviceSynchronize());
    double t0 = now_ms();
    for (int i = 0; i < iters; ++i) launch();
    LG_CHECK(hipDeviceSynchronize());
    *ms_out = (now_ms() - t0) / iters;
    return 0;
}

static void report_gemm(int m, int n, int k, double ms, double* ms_out,
                        double* tflops_out)
{
    if (ms_out) *ms_out = ms;
    if (tflops_out) *tflops_out = 2.0 * m * n * k / (ms * 1e-3) / 1e12;
}

// Verify tail: launch, wait, surface a launch or execution error, copy the
// result back.
template <typename LaunchFn>
static int run_and_fetch(LaunchFn&& launch, float* c_out, const float* c_dev,
                         size_t bytes)
{
    launch();
    LG_CHECK(hipDeviceSynchronize());
    LG_CHECK(hipGetLastError());
    LG_CHECK(hipMemcpy(c_out, c_dev, bytes, hipMemcpyDeviceToHost));
    return 0;
}

static void burn_args(double& target_util_pct, double& period_ms)
{
    if (period_ms <= 0) period_ms = 100.0;
    if (target_util_pct < 0) target_util_pct = 0;
    if (target_util_pct > 100) target_util_pct = 100;
}

static void gemm_burn_dims(int& m, int& n, int& k)
{
    if (m <= 0) m = 4096;
    if (n <= 0) n = 4096;
    if (k <= 0) k = 4096;
}

// Shared closed-loop duty engine: runs `launch4()` (4 queued kernel
// launches + sync, hipEvent-measured) in busy bursts of duty*period and
// trims the duty fraction by the measured GPU-active fraction per actual
// period. Used by the bf16, fp8, mxfp4 and decode burn entries.
template <typename LaunchFn>
static int duty_burn_loop(double target_util_pct, double seconds,
                          double period_ms, volatile int* stop_flag,
                          LaunchFn&& launch4)
{
    DevEvent ev0, ev1;
    LG_CHECK(ev0.create());
    LG_CHECK(ev1.create());
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
    return 0;
}

// GEMM burn body shared by bf16, fp8 and mxfp4: one calibration launch so
// the first period isn't all compile/warmup, then bursts of 4 launches.
template <typename LaunchFn>
static int gemm_burn(double target_util_pct, double seconds, double period_ms,
                     volatile int* stop_flag, LaunchFn&& launch)
{
    launch();
    LG_CHECK(hipDeviceSynchronize());
    return duty_burn_loop(target_util_pct, seconds, period_ms, stop_flag, [&] {
        for (int b = 0; b < 4; ++b) launch();
    });
}

// Burn body shared by the step-shaped loads (decode, attention): the
// closed-loop duty engine over bursts of `step()` launches, plus the
// GPU-active time of the bursts and the number of steps in them, from which
// the caller derives its byte rate.
template <typename StepFn>
static int step_burn(double target_util_pct, double seconds, double period_ms,
                     volatile int* stop_flag, StepFn&& step, double& active_ms,
                     double& steps)
{
    DevEvent e0, e1;
    LG_CHECK(e0.create());
    LG_CHECK(e1.create());
    // calibration step: sizes the burst so that a busy slice of the
    // default 100 ms period holds several launches
    LG_CHECK(hipEventRecord(e0, 0));
    step();
    LG_CHECK(hipEventRecord(e1, 0));
    LG_CHECK(hipDeviceSynchronize());
    float step_ms = 0;
    LG_CHECK(hipEventElapsedTime(&step_ms, e0, e1));
    int per_burst = step_ms > 0 ? (int)(2.0f / step_ms) : 4;
    if (per_burst < 4) per_burst = 4;
    if (per_burst > 64) per_burst = 64;
    // rate: each burst is bracketed by events of its own, read back at the
    // next burst (the engine has synchronised by then), so the engine
    // itself stays as it is
    active_ms = 0;
    steps = 0;
    bool pending = false;
    if (duty_burn_loop(target_util_pct, seconds, period_ms, stop_flag, [&] {
            float dt = 0;
            if (pending && hipEventElapsedTime(&dt, e0, e1) == hipSuccess) {
                active_ms += dt;
                steps += per_burst;
            }
            (void)hipEventRecord(e0, 0);
            for (int b = 0; b < per_burst; ++b) step();
            (void)hipEventRecord(e1, 0);
            pending = true;
        }))
        return -1;
    LG_CHECK(hipDeviceSynchronize());
    if (pending) {
        float dt = 0;
        LG_CHECK(hipEventElapsedTime(&dt, e0, e1));
        active_ms += dt;
        steps += per_burst;
    }
    LG_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// vectorAdd and the streaming triad
// ---------------------------------------------------------------------------

static int vec_blocks(int n, int threads)
{
    int blocks = (n + threads - 1) / threads;
    return blocks > 4096 ? 4096 : blocks;  // grid-stride covers the rest
}

// One allocation + `iters` kernel launches (sync per launch, like one
// process-per-launch in the reference but without exec overhead).
int lg_vector_add_loop(int device, int n, int iters, double* ms_out)
{
    LG_CHECK(hipSetDevice(device));
    DevBuf<float> a, b, c;
    size_t bytes = (size_t)n * 4;
    LG_CHECK(a.alloc(bytes));
    LG_CHECK(b.alloc(bytes));
    LG_CHECK(c.alloc(bytes));
    std::vector<float> h(n);
    for (int i = 0; i < n; ++i) h[i] = (float)((i * 2654435761u) % 1000) * 1e-3f;
    LG_CHECK(hipMemcpy(a, h.data(), bytes, hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(b, h.data(), bytes, hipMemcpyHostToDevice));

    const int threads = 256, blocks = vec_blocks(n, threads);
    double t0 = now_ms();
    for (int i = 0; i < iters; ++i) {
        hipLaunchKernelGGL(vector_add_f32, dim3(blocks), dim3(threads), 0, 0,
                           a.p, b.p, c.p, n);
        LG_CHECK(hipDeviceSynchronize());
    }
    if (ms_out) *ms_out = now_ms() - t0;
    return 0;
}

// Numerics entry: c_out[i] = a[i] + b[i] computed on the GPU.
int lg_vector_add_verify(int device, const float* a_h, const float* b_h, float* c_out, int n)
{
    LG_CHECK(hipSetDevice(device));
    DevBuf<float> a, b, c;
    size_t bytes = (size_t)n * 4;
    LG_CHECK(a.alloc(bytes));
    LG_CHECK(b.alloc(bytes));
    LG_CHECK(c.alloc(bytes));
    LG_CHECK(hipMemcpy(a, a_h, bytes, hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(b, b_h, bytes, hipMemcpyHostToDevice));
    const int threads = 256;
    return run_and_fetch(
        [&] {
            if (n % 4 == 0)
                hipLaunchKernelGGL(vector_add_f32x4,
                                   dim3(vec_blocks(n / 4, threads)),
                                   dim3(threads), 0, 0, (const float4*)a.p,
                                   (const float4*)b.p, (float4*)c.p, n / 4);
            else
                hipLaunchKernelGGL(vector_add_f32, dim3(vec_blocks(n, threads)),
                                   dim3(threads), 0, 0, a.p, b.p, c.p, n);
        },
        c_out, c, bytes);
}

// Streaming-triad bandwidth burn: duty-cycled HBM traffic at
// `target_util_pct` of wall time; `gb` working set (3 buffers summing to
// ~gb GiB). The bandwidth-axis load for the multi-metric HPA (config 5).
int lg_bw_burn(int device, double target_util_pct, double seconds, double gb,
               double period_ms, volatile int* stop_flag, double* gbps_out)
{
    if (gb <= 0) gb = 6.0;
    burn_args(target_util_pct, period_ms);
    LG_CHECK(hipSetDevice(device));
    long n4 = (long)(gb * (1ull << 30) / 3.0 / 16.0);
    DevBuf<float4> a, b, c;
    LG_CHECK(a.alloc(n4 * 16));
    LG_CHECK(b.alloc(n4 * 16));
    LG_CHECK(c.alloc(n4 * 16));
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
            hipLaunchKernelGGL(triad_f32x4, dim3(blocks), dim3(256), 0, 0,
                               (const float4*)a.p, (const float4*)b.p, c.p,
                               1.5f, n4);
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
    return 0;
}

// ---------------------------------------------------------------------------
// MFMA bf16 GEMM
// ---------------------------------------------------------------------------

// The bf16 kernel variants, numbered as the *_variant entries and
// tools/gemm_ab_gpu.py number them (profiles/gemm_bf16_256_ladder.md has
// the measurements). Selection rules, unchanged since the variants were
// added one by one:
//   * variant 2 is the product entry: it runs d18 (17) above 2048 tiles
//     (16k-class shapes: the 3-deep-B d18 wins by ~16% there, DMA latency
//     under heavy memory-system load) and d9 otherwise;
//   * bench and burn fall back to the 128^2 kernel (1) below 128 tiles of
//     256^2: 256-tile kernels need >= 128 CTAs to fill the 256-CU chip.
//     Verify never does: tests must exercise the exact kernel asked for;
//   * a number that is not in the table runs the 256^2 product kernel if it
//     is >= 2, and the 128^2 swizzled kernel otherwise.
using Bf16Kernel = void (*)(const unsigned short*, const unsigned short*,
                            float*, int, int, int, int);
struct Bf16Variant {
    int variant;
    Bf16Kernel kernel;
    int threads, tile;
};
static const Bf16Variant kBf16Variants[] = {
    {0, gemm_bf16_tn_linear, 256, 128},     // 128^2, linear LDS (A/B ref)
    {1, gemm_bf16_tn, 256, 128},            // 128^2, st_16x32-swizzled LDS
    {2, gemm_bf16_tn_256, 512, 256},        // product: d9 (d18 when huge)
    {3, gemm_bf16_tn_256_d1, 512, 256},     // depth-1 full drain
    {4, gemm_bf16_tn_256_d4, 512, 256},     // quadrant phases, all B held
    {5, gemm_bf16_tn_256_d5, 512, 256},     // latency-balanced d2
    {6, gemm_bf16_tn_256_d2, 512, 256},     // half per phase, one B0 ahead
    {7, gemm_bf16_tn_256_d7, 512, 256},     // d6 with 5 barriers per K-tile
    {8, gemm_bf16_tn_256_d8, 512, 256},     // d6 without the raster
    {9, gemm_bf16_tn_256_w32, 512, 256},    // d6 on 32x32x16 MFMA tiles
    {10, gemm_bf16_tn_256_soft, 512, 256},  // d6 with explicit lgkm drains
    {11, gemm_bf16_tn_256_d9, 512, 256},    // one barrier per K-tile
    {12, gemm_bf16_tn_256_d9nr, 512, 256},  // d9 without the raster
    {13, gemm_bf16_tn_256_d14, 1024, 256},  // 16 waves, 4 waves/SIMD
    {14, gemm_bf16_tn_256_d6, 512, 256},    // round-1 product (A/B baseline)
    {15, gemm_bf16_tn_256_d9w, 512, 256},   // d9 + wide epilogue
    {16, gemm_bf16_tn_256_d9e, 512, 256},   // d9, all stages at q0
    {17, gemm_bf16_tn_256_d18, 512, 256},   // d9 + 3-deep B rotation
    {18, gemm_bf16_tn_256_d19, 512, 256},   // d18 + pipelined A reads
    {19, gemm_bf16_tn_256_d20, 256, 256},   // 4 waves, 1 wave/SIMD, AGPR acc
    {20, gemm_bf16_tn_256_d21, 256, 256},   // d20 + deep B + A prefetch
};

static const Bf16Variant& bf16_variant(int variant)
{
    for (const Bf16Variant& v : kBf16Variants)
        if (v.variant == variant) return v;
    return kBf16Variants[variant >= 2 ? 2 : 1];
}

struct GemmBufs {
    DevBuf<unsigned short> a, bt;
    DevBuf<float> c;
    int m = 0, n = 0, k = 0;
};

static int gemm_alloc(GemmBufs& g, int m, int n, int k, bool fill_random)
{
    const size_t na = (size_t)m * k, nb = (size_t)n * k;
    LG_CHECK(g.a.alloc(na * 2));
    LG_CHECK(g.bt.alloc(nb * 2));
    LG_CHECK(g.c.alloc((size_t)m * n * 4));
    g.m = m; g.n = n; g.k = k;
    if (!fill_random) return 0;
    uint32_t st = 0x12345678u;  // random-ish bf16 in [-1, 1)
    return fill_pair(g.a.p, na, g.bt.p, nb, st,
                     [](uint32_t& s) { return f32_to_bf16(lcg_unit(s)); });
}

static void gemm_launch(const GemmBufs& g, hipStream_t stream, int variant)
{
    if (variant == 2 && (g.m / 256) * (g.n / 256) > 2048) variant = 17;
    const Bf16Variant& v = bf16_variant(variant);
    const TileGrid grid = tile_grid(g.m, g.n, v.tile);
    hipLaunchKernelGGL(v.kernel, dim3(grid.blocks), dim3(v.threads), 0, stream,
                       g.a.p, g.bt.p, g.c.p, g.m, g.n, g.k,
                       grid.tiles_per_cta);
}

static bool gemm_dims_ok(int m, int n, int k, int variant)
{
    const int mt = bf16_variant(variant).tile;
    if (m % mt || n % mt || k % 64) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "gemm dims must be multiples of %d/%d/64", mt, mt);
        return false;
    }
    return true;
}

// Bench and burn only (see the selection rules above).
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
    double ms;
    if (timed_launches(warmup, iters, [&] { gemm_launch(g, 0, variant); }, &ms))
        return -1;
    report_gemm(m, n, k, ms, ms_out, tflops_out);
    return 0;
}

int lg_gemm_bf16_bench(int device, int m, int n, int k, int warmup, int iters,
                       double* ms_out, double* tflops_out)
{
    return lg_gemm_bf16_bench_variant(device, m, n, k, warmup, iters, 1, ms_out,
                                      tflops_out);
}

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
    return run_and_fetch([&] { gemm_launch(g, 0, variant); }, c_out, g.c,
                         (size_t)m * n * 4);
}

int lg_gemm_bf16_verify(int device, const float* a_h, const float* bt_h,
                        float* c_out, int m, int n, int k)
{
    return lg_gemm_bf16_verify_variant(device, a_h, bt_h, c_out, m, n, k, 1);
}

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
int lg_gemm_burn(int device, double target_util_pct, double seconds,
                 int m, int n, int k, double period_ms, volatile int* stop_flag)
{
    gemm_burn_dims(m, n, k);
    burn_args(target_util_pct, period_ms);
    const int burn_variant = gemm_effective_variant(m, n, 2);
    LG_CHECK(hipSetDevice(device));
    GemmBufs g;
    if (gemm_alloc(g, m, n, k, true)) return -1;
    return gemm_burn(target_util_pct, seconds, period_ms, stop_flag,
                     [&] { gemm_launch(g, 0, burn_variant); });
}

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
    (void)std::frexp(af, &ef);      // af = m * 2^ef, m in [0.5, 1)
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
    DevBuf<unsigned char> a, bt;
    DevBuf<float> c;
    int m = 0, n = 0, k = 0;
};

static bool fp8_dims_ok(int m, int n, int k)
{
    if (m % 256 || n % 256 || k % 128) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "fp8 gemm dims must be multiples of 256/256/128");
        return false;
    }
    return true;
}

static int fp8_gemm_alloc(Fp8GemmBufs& g, int m, int n, int k, bool fill_random)
{
    const size_t na = (size_t)m * k, nb = (size_t)n * k;
    LG_CHECK(g.a.alloc(na));
    LG_CHECK(g.bt.alloc(nb));
    LG_CHECK(g.c.alloc((size_t)m * n * 4));
    g.m = m; g.n = n; g.k = k;
    if (!fill_random) return 0;
    uint32_t st = 0x2468ace1u;  // random fp8 in [-1, 1)
    return fill_pair(g.a.p, na, g.bt.p, nb, st,
                     [](uint32_t& s) { return f32_to_fp8_e4m3(lcg_unit(s)); });
}

// raster: 1 = product (4x4 super-tile), 0 = linear, 2 = deep-B rotation
static void fp8_gemm_launch(const Fp8GemmBufs& g, hipStream_t stream, int raster)
{
    const TileGrid grid = tile_grid(g.m, g.n, 256);
    hipLaunchKernelGGL(raster == 2   ? gemm_fp8_tn_256_db
                       : raster == 1 ? gemm_fp8_tn_256
                                     : gemm_fp8_tn_256_nr,
                       dim3(grid.blocks), dim3(512), 0, stream, g.a.p, g.bt.p,
                       g.c.p, g.m, g.n, g.k, grid.tiles_per_cta);
}

// Quantize one f32 operand to E4M3, upload it, hand back what it dequantizes
// to.
static int fp8_upload_operand(const float* x_h, size_t count,
                              unsigned char* x_d, float* deq_out)
{
    std::vector<unsigned char> q(count);
    for (size_t i = 0; i < count; ++i) {
        q[i] = f32_to_fp8_e4m3(x_h[i]);
        if (deq_out) deq_out[i] = fp8_e4m3_to_f32(q[i]);
    }
    LG_CHECK(hipMemcpy(x_d, q.data(), count, hipMemcpyHostToDevice));
    return 0;
}

int lg_gemm_fp8_bench(int device, int m, int n, int k, int warmup, int iters,
                      int raster, double* ms_out, double* tflops_out)
{
    if (!fp8_dims_ok(m, n, k)) return -1;
    LG_CHECK(hipSetDevice(device));
    Fp8GemmBufs g;
    if (fp8_gemm_alloc(g, m, n, k, true)) return -1;
    double ms;
    if (timed_launches(warmup, iters, [&] { fp8_gemm_launch(g, 0, raster); },
                       &ms))
        return -1;
    report_gemm(m, n, k, ms, ms_out, tflops_out);
    return 0;
}

int lg_gemm_fp8_verify_variant(int device, const float* a_h, const float* bt_h,
                               float* c_out, float* aq_out, float* btq_out,
                               int m, int n, int k, int raster)
{
    if (!fp8_dims_ok(m, n, k)) return -1;
    LG_CHECK(hipSetDevice(device));
    Fp8GemmBufs g;
    if (fp8_gemm_alloc(g, m, n, k, false)) return -1;
    if (fp8_upload_operand(a_h, (size_t)m * k, g.a, aq_out)) return -1;
    if (fp8_upload_operand(bt_h, (size_t)n * k, g.bt, btq_out)) return -1;
    return run_and_fetch([&] { fp8_gemm_launch(g, 0, raster); }, c_out, g.c,
                         (size_t)m * n * 4);
}

int lg_gemm_fp8_verify(int device, const float* a_h, const float* bt_h,
                       float* c_out, float* aq_out, float* btq_out,
                       int m, int n, int k)
{
    return lg_gemm_fp8_verify_variant(device, a_h, bt_h, c_out, aq_out,
                                      btq_out, m, n, k, 1);
}

// fp8 (E4M3) variant of the burn: same closed-loop duty engine over the
// fp8 MFMA kernel — the 2x-peak datatype's power/clock profile as a load.
int lg_gemm_fp8_burn(int device, double target_util_pct, double seconds,
                     int m, int n, int k, double period_ms,
                     volatile int* stop_flag)
{
    gemm_burn_dims(m, n, k);
    burn_args(target_util_pct, period_ms);
    if (!fp8_dims_ok(m, n, k)) return -1;
    LG_CHECK(hipSetDevice(device));
    Fp8GemmBufs g;
    if (fp8_gemm_alloc(g, m, n, k, true)) return -1;
    return gemm_burn(target_util_pct, seconds, period_ms, stop_flag,
                     [&] { fp8_gemm_launch(g, 0, 1); });
}

// ---------------------------------------------------------------------------
// MXFP4 (E2M1 + E8M0 block scale) MFMA GEMM — the CDNA4 4x-peak datatype
// (gemm_mxfp4_256.hip). Public operand format and quantizer: mxfp4_host.h.
// ---------------------------------------------------------------------------

struct Mxfp4GemmBufs {
    DevBuf<unsigned char> a;   // [m][k/2]
    DevBuf<unsigned char> bt;  // [n][k/2]
    DevBuf<int> sa;            // [m/64][k/128][64], mxfp4::shuffle_scales
    DevBuf<int> sb;            // [n/64][k/128][64]
    DevBuf<float> c;
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
    LG_CHECK(g.a.alloc(na));
    LG_CHECK(g.bt.alloc(nb));
    LG_CHECK(g.sa.alloc(nsa));
    LG_CHECK(g.sb.alloc(nsb));
    LG_CHECK(g.c.alloc((size_t)m * n * 4));
    g.m = m; g.n = n; g.k = k;
    if (!fill_random) return 0;
    return fill_mxfp4_pair(0x1357bdf1u, g.a, na, g.bt, nb, g.sa, nsa, g.sb,
                           nsb);
}

// max_ctas > 0 caps the grid (each CTA then loops over several tiles).
static void mxfp4_gemm_launch(const Mxfp4GemmBufs& g, hipStream_t stream,
                              int max_ctas = 0)
{
    const TileGrid grid = tile_grid(g.m, g.n, 256, max_ctas);
    hipLaunchKernelGGL(gemm_mxfp4_tn_256, dim3(grid.blocks), dim3(512), 0,
                       stream, g.a.p, g.bt.p, g.sa.p, g.sb.p, g.c.p, g.m, g.n,
                       g.k, grid.tiles_per_cta);
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

int lg_gemm_mxfp4_bench(int device, int m, int n, int k, int warmup, int iters,
                        double* ms_out, double* tflops_out)
{
    if (!mxfp4_dims_ok(m, n, k)) return -1;
    LG_CHECK(hipSetDevice(device));
    Mxfp4GemmBufs g;
    if (mxfp4_gemm_alloc(g, m, n, k, true)) return -1;
    double ms;
    if (timed_launches(warmup, iters, [&] { mxfp4_gemm_launch(g, 0); }, &ms))
        return -1;
    report_gemm(m, n, k, ms, ms_out, tflops_out);
    return 0;
}

int lg_gemm_mxfp4_verify(int device, const float* a_h, const float* bt_h,
                         float* c_out, float* aq_out, float* btq_out,
                         int m, int n, int k, int max_ctas)
{
    if (!mxfp4_dims_ok(m, n, k)) return -1;
    LG_CHECK(hipSetDevice(device));
    Mxfp4GemmBufs g;
    if (mxfp4_gemm_alloc(g, m, n, k, false)) return -1;
    if (mxfp4_upload_operand(a_h, m, k, g.a, g.sa, aq_out)) return -1;
    if (mxfp4_upload_operand(bt_h, n, k, g.bt, g.sb, btq_out)) return -1;
    return run_and_fetch([&] { mxfp4_gemm_launch(g, 0, max_ctas); }, c_out,
                         g.c, (size_t)m * n * 4);
}

// MXFP4 variant of the burn: same closed-loop duty engine over the
// block-scaled fp4 MFMA kernel — the load shape of an MXFP4 serving pod.
int lg_gemm_mxfp4_burn(int device, double target_util_pct, double seconds,
                       int m, int n, int k, double period_ms,
                       volatile int* stop_flag)
{
    gemm_burn_dims(m, n, k);
    burn_args(target_util_pct, period_ms);
    if (!mxfp4_dims_ok(m, n, k)) return -1;
    LG_CHECK(hipSetDevice(device));
    Mxfp4GemmBufs g;
    if (mxfp4_gemm_alloc(g, m, n, k, true)) return -1;
    return gemm_burn(target_util_pct, seconds, period_ms, stop_flag,
                     [&] { mxfp4_gemm_launch(g, 0); });
}

// ---------------------------------------------------------------------------
// Decode-phase MXFP4 weight streaming (gemm_mxfp4_decode.hip): a skinny-M
// a4w4 GEMM over a ring of `layers` weight matrices W[L][N][K] and one
// activation block X[M][K], 1 <= M <= 64. Memory-bound by design: each
// weight byte is read once per step.
// ---------------------------------------------------------------------------

struct DecodeBufs {
    DevBuf<unsigned char> x;  // [mp][k/2], mp = m rounded up to 16
    DevBuf<int> sx;           // [k/128][64], one 64-row group
    DevBuf<unsigned char> w;  // [layers][n][k/2]
    DevBuf<int> sw;           // [layers*n/64][k/128][64]
    DevBuf<float> c;          // [layers][m][n]
    DevBuf<float> part;       // [k_splits][layers][m][n] if k_splits > 1
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

// k_splits: 0 = heuristic. Dimensions must have passed decode_dims_ok.
static int decode_alloc(DecodeBufs& d, int m, int n, int k, int layers,
                        int k_splits)
{
    d.m = m; d.mp = (m + 15) / 16 * 16; d.n = n; d.k = k; d.layers = layers;
    d.k_splits = k_splits > 0 ? k_splits : decode_pick_k_splits(n, k, layers);
    const size_t c_bytes = (size_t)layers * m * n * 4;
    LG_CHECK(d.x.alloc((size_t)d.mp * k / 2));
    LG_CHECK(d.sx.alloc((size_t)64 * k / 32));
    LG_CHECK(d.w.alloc((size_t)layers * n * k / 2));
    LG_CHECK(d.sw.alloc((size_t)layers * n * k / 32));
    LG_CHECK(d.c.alloc(c_bytes));
    if (d.k_splits > 1) LG_CHECK(d.part.alloc(c_bytes * d.k_splits));
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
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, stream, d.x.p, d.sx.p,
                       d.w.p, d.sw.p, out, d.m, d.n, d.k, d.layers,
                       d.k_splits);
    if (d.k_splits > 1) {
        const long n4 = (long)d.layers * d.m * d.n / 4;
        long rb = (n4 + 255) / 256;
        if (rb > 2048) rb = 2048;
        hipLaunchKernelGGL(decode_mxfp4_reduce, dim3((int)rb), dim3(256), 0,
                           stream, (const float4*)d.part.p, (float4*)d.c.p, n4,
                           d.k_splits);
    }
}

static double decode_weight_bytes(const DecodeBufs& d)
{
    return (double)d.layers * ((double)d.n * d.k / 2 + (double)d.n * d.k / 32);
}

// Random codes and scale bytes (as mxfp4_gemm_alloc). One layer is
// generated on the host and replicated on the device.
static int decode_fill_random(DecodeBufs& d)
{
    const size_t wl = (size_t)d.n * d.k / 2, swl = (size_t)d.n * d.k / 32;
    const size_t xb = (size_t)d.mp * d.k / 2, sxb = (size_t)64 * d.k / 32;
    if (fill_mxfp4_pair(0x0decade1u, d.w, wl, d.x, xb, d.sw, swl, d.sx, sxb))
        return -1;
    for (int l = 1; l < d.layers; ++l) {
        LG_CHECK(hipMemcpy(d.w + l * wl, d.w, wl, hipMemcpyDeviceToDevice));
        LG_CHECK(hipMemcpy((unsigned char*)d.sw.p + l * swl, d.sw, swl,
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
    if (decode_alloc(d, m, n, k, layers, k_splits)) return -1;
    auto up = [&](void* dst, const std::vector<unsigned char>& src) {
        LG_CHECK(hipMemcpy(dst, src.data(), src.size(), hipMemcpyHostToDevice));
        return 0;
    };
    if (up(d.x, xe) || up(d.sx, xsh) || up(d.w, we) || up(d.sw, wsh))
        return -1;
    return run_and_fetch([&] { decode_step(d, 0); }, c_out, d.c,
                         (size_t)layers * m * n * 4);
}

int lg_decode_mxfp4_bench(int device, int m, int n, int k, int layers,
                          int warmup, int iters, double* ms_per_step_out,
                          double* weight_gbps_out)
{
    decode_defaults(m, n, k, layers);
    if (iters < 1) iters = 1;
    if (!decode_dims_ok(m, n, k, layers, 0)) return -1;
    LG_CHECK(hipSetDevice(device));
    DecodeBufs d;
    if (decode_alloc(d, m, n, k, layers, 0)) return -1;
    if (decode_fill_random(d)) return -1;
    double ms;
    if (timed_launches(warmup, iters, [&] { decode_step(d, 0); }, &ms))
        return -1;
    LG_CHECK(hipGetLastError());
    if (ms_per_step_out) *ms_per_step_out = ms;
    if (weight_gbps_out)
        *weight_gbps_out = decode_weight_bytes(d) / (ms * 1e-3) / 1e9;
    return 0;
}

// Decode burn: the shared closed-loop duty engine over decode steps — the
// load shape of a small-batch MXFP4 serving pod (busy%, bandwidth-bound).
int lg_decode_mxfp4_burn(int device, double target_util_pct, double seconds,
                         int m, int n, int k, int layers, double period_ms,
                         volatile int* stop_flag, double* weight_gbps_out)
{
    if (weight_gbps_out) *weight_gbps_out = 0;
    decode_defaults(m, n, k, layers);
    burn_args(target_util_pct, period_ms);
    if (!decode_dims_ok(m, n, k, layers, 0)) return -1;
    LG_CHECK(hipSetDevice(device));
    DecodeBufs d;
    if (decode_alloc(d, m, n, k, layers, 0)) return -1;
    if (decode_fill_random(d)) return -1;
    double active_ms = 0, steps = 0;
    if (step_burn(target_util_pct, seconds, period_ms, stop_flag,
                  [&] { decode_step(d, 0); }, active_ms, steps))
        return -1;
    if (weight_gbps_out && active_ms > 0)
        *weight_gbps_out =
            steps * decode_weight_bytes(d) / (active_ms * 1e-3) / 1e9;
    return 0;
}

// ---------------------------------------------------------------------------
// Decode attention over a contiguous bf16 KV cache (attn_decode.hip):
// q [B][Hq][128] against one K and one V slab of Lmax positions per
// (sequence, kv head), ragged seq_lens, G = Hq / Hkv query heads per kv
// head. Memory-bound by design: each cached key and value is read once per
// step.
// ---------------------------------------------------------------------------

struct AttnBufs {
    DevBuf<unsigned short> q;   // [batch][hq][128]
    DevBuf<unsigned short> k;   // [batch][hkv][lmax][128]
    DevBuf<unsigned short> vp;  // [batch][hkv][blocks][128][32], private
    DevBuf<int> lens;           // [batch]
    DevBuf<float> o;            // [batch][hq][128]
    DevBuf<float> lse;          // [batch][hq]
    DevBuf<float> ws;           // kv_splits > 1: acc, then m, then l
    int batch = 0, hq = 0, hkv = 0, lmax = 0, blocks = 0, kv_splits = 1;
    int blocks_per_split = 0;
    float scale_log2e = 0;
    size_t rows() const { return (size_t)batch * hq; }
    size_t k_slab() const { return (size_t)lmax * 128; }     // elements
    size_t v_slab() const { return (size_t)blocks * 4096; }  // elements
};

// Every argument the device code turns into an address is checked here,
// before any device call. seq_lens may be null (bench, burn: all = lmax).
static bool attn_dims_ok(int batch, int hq, int hkv, int lmax, int d,
                         int kv_splits, const int* seq_lens)
{
    const char* why = nullptr;
    if (d != 128) why = "head dimension must be 128";
    else if (batch < 1 || hq < 1 || hkv < 1 || lmax < 1)
        why = "batch, heads and context must be >= 1";
    else if (hq % hkv) why = "q heads must be a multiple of kv heads";
    else if (hq / hkv > 16) why = "at most 16 q heads per kv head";
    else if (kv_splits < 0 || kv_splits > (lmax + 31) / 32)
        why = "kv_splits must be in 0..ceil(lmax/32)";
    if (why) {
        std::snprintf(g_last_error, sizeof(g_last_error),
                      "attn decode: %s (batch %d, hq %d, hkv %d, lmax %d, "
                      "d %d, kv_splits %d)",
                      why, batch, hq, hkv, lmax, d, kv_splits);
        return false;
    }
    for (int b = 0; seq_lens && b < batch; ++b)
        if (seq_lens[b] < 1 || seq_lens[b] > lmax) {
            std::snprintf(g_last_error, sizeof(g_last_error),
                          "attn decode: seq_lens[%d] = %d outside 1..%d", b,
                          seq_lens[b], lmax);
            return false;
        }
    return true;
}

// Product heuristic: a CTA is one (sequence, kv head, KV split). Split the
// context across CTAs until the grid reaches two CTAs per CU (the chip has
// 256), as long as a split keeps at least 256 positions.
static int attn_pick_kv_splits(int batch, int hkv, int lmax)
{
    const long ctas = (long)batch * hkv;
    int s = 1;
    while (ctas * s < 512 && lmax / (s * 2) >= 256) s *= 2;
    return s;
}

// kv_splits: 0 = heuristic. Dimensions must have passed attn_dims_ok.
static int attn_alloc(AttnBufs& a, int batch, int hq, int hkv, int lmax,
                      int kv_splits, double scale)
{
    a.batch = batch; a.hq = hq; a.hkv = hkv; a.lmax = lmax;
    a.blocks = (lmax + 31) / 32;
    a.kv_splits =
        kv_splits > 0 ? kv_splits : attn_pick_kv_splits(batch, hkv, lmax);
    a.blocks_per_split = (a.blocks + a.kv_splits - 1) / a.kv_splits;
    if (scale <= 0) scale = 1.0 / std::sqrt(128.0);
    a.scale_log2e = (float)(scale * 1.4426950408889634);
    const size_t slabs = (size_t)batch * hkv;
    LG_CHECK(a.q.alloc(a.rows() * 128 * 2));
    LG_CHECK(a.k.alloc(slabs * a.k_slab() * 2));
    LG_CHECK(a.vp.alloc(slabs * a.v_slab() * 2));
    LG_CHECK(a.lens.alloc((size_t)batch * 4));
    LG_CHECK(a.o.alloc(a.rows() * 128 * 4));
    LG_CHECK(a.lse.alloc(a.rows() * 4));
    if (a.kv_splits > 1)
        LG_CHECK(a.ws.alloc((size_t)a.kv_splits * a.rows() * 130 * 4));
    return 0;
}

// One decode-attention step: one launch over (sequence, kv head, split),
// plus the ordered merge when the context is split across CTAs. Verify,
// bench and burn all run this function.
static void attn_step(const AttnBufs& a, hipStream_t stream)
{
    const size_t part = (size_t)a.kv_splits * a.rows();
    float* ws_acc = a.ws;
    float* ws_m = a.kv_splits > 1 ? ws_acc + part * 128 : nullptr;
    float* ws_l = a.kv_splits > 1 ? ws_m + part : nullptr;
    hipLaunchKernelGGL(attn_decode_bf16,
                       dim3(a.batch * a.hkv * a.kv_splits), dim3(256), 0,
                       stream, a.q.p, a.k.p, a.vp.p, a.lens.p, a.o.p, a.lse.p,
                       ws_acc, ws_m, ws_l, a.batch, a.hq, a.hkv, a.lmax,
                       a.blocks_per_split, a.kv_splits, a.scale_log2e);
    if (a.kv_splits > 1)
        hipLaunchKernelGGL(attn_decode_merge, dim3((int)a.rows()), dim3(128),
                           0, stream, ws_acc, ws_m, ws_l, a.o.p, a.lse.p,
                           a.kv_splits);
}

// Public V slab [lmax][128] f32 -> the kernel's private layout
// [blocks][128][32] bf16 (attn_decode.hip): position p of a 32-block sits
// at 8*((p%16)/4) + 4*(p/16) + p%4. Padding past lmax is zero.
static void attn_pack_v(const float* v, int lmax, unsigned short* out)
{
    const int blocks = (lmax + 31) / 32;
    std::memset(out, 0, (size_t)blocks * 4096 * 2);
    for (int pos = 0; pos < lmax; ++pos) {
        const int p = pos & 31;
        const int idx = 8 * ((p & 15) >> 2) + 4 * (p >> 4) + (p & 3);
        unsigned short* dst = out + (size_t)(pos >> 5) * 4096 + idx;
        for (int d = 0; d < 128; ++d)
            dst[d * 32] = f32_to_bf16(v[(size_t)pos * 128 + d]);
    }
}

// Bench and burn: every sequence is lmax long. One (sequence, kv head)
// slab of K and of V (filled in the private layout directly: it is a
// permutation of random values) is generated and replicated on the device.
static int attn_fill_random(AttnBufs& a)
{
    uint32_t st = 0xa77e11d1u;
    auto gen = [](uint32_t& s) { return f32_to_bf16(lcg_unit(s)); };
    std::vector<unsigned short> h(a.rows() * 128);
    lcg_fill(h, st, gen);
    LG_CHECK(hipMemcpy(a.q, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    if (fill_pair(a.k.p, a.k_slab(), a.vp.p, a.v_slab(), st, gen)) return -1;
    const size_t slabs = (size_t)a.batch * a.hkv;
    for (size_t s = 1; s < slabs; ++s) {
        LG_CHECK(hipMemcpy(a.k + s * a.k_slab(), a.k, a.k_slab() * 2,
                           hipMemcpyDeviceToDevice));
        LG_CHECK(hipMemcpy(a.vp + s * a.v_slab(), a.vp, a.v_slab() * 2,
                           hipMemcpyDeviceToDevice));
    }
    const std::vector<int> lens(a.batch, a.lmax);
    LG_CHECK(hipMemcpy(a.lens, lens.data(), lens.size() * 4,
                       hipMemcpyHostToDevice));
    return 0;
}

// K and V bytes read per step when every sequence is ctx long.
static double attn_kv_bytes(const AttnBufs& a)
{
    return (double)a.batch * a.hkv * a.lmax * 2 * 128 * 2;
}

int lg_attn_decode_verify(int device, const float* q_h, const float* k_h,
                          const float* v_h, const int* seq_lens, float* o_out,
                          float* lse_out, int batch, int hq, int hkv, int lmax,
                          int d, int kv_splits, double scale)
{
    if (!attn_dims_ok(batch, hq, hkv, lmax, d, kv_splits, seq_lens)) return -1;
    LG_CHECK(hipSetDevice(device));
    AttnBufs a;
    if (attn_alloc(a, batch, hq, hkv, lmax, kv_splits, scale)) return -1;
    const size_t slabs = (size_t)batch * hkv;
    std::vector<unsigned short> tmp(a.rows() * 128);
    for (size_t i = 0; i < tmp.size(); ++i) tmp[i] = f32_to_bf16(q_h[i]);
    LG_CHECK(hipMemcpy(a.q, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    tmp.resize(slabs * a.k_slab());
    for (size_t i = 0; i < tmp.size(); ++i) tmp[i] = f32_to_bf16(k_h[i]);
    LG_CHECK(hipMemcpy(a.k, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    tmp.resize(slabs * a.v_slab());
    for (size_t s = 0; s < slabs; ++s)
        attn_pack_v(v_h + s * a.k_slab(), lmax, tmp.data() + s * a.v_slab());
    LG_CHECK(hipMemcpy(a.vp, tmp.data(), tmp.size() * 2,
                       hipMemcpyHostToDevice));
    LG_CHECK(hipMemcpy(a.lens, seq_lens, (size_t)batch * 4,
                       hipMemcpyHostToDevice));
    if (run_and_fetch([&] { attn_step(a, 0); }, o_out, a.o,
                      a.rows() * 128 * 4))
        return -1;
    LG_CHECK(hipMemcpy(lse_out, a.lse, a.rows() * 4, hipMemcpyDeviceToHost));
    return 0;
}

int lg_attn_decode_bench_splits(int device, int batch, int hq, int hkv, int ctx,
                                int d, int kv_splits, int warmup, int iters,
                                double* ms_per_step_out, double* kv_gbps_out)
{
    if (iters < 1) iters = 1;
    if (!attn_dims_ok(batch, hq, hkv, ctx, d, kv_splits, nullptr)) return -1;
    LG_CHECK(hipSetDevice(device));
    AttnBufs a;
    if (attn_alloc(a, batch, hq, hkv, ctx, kv_splits, 0)) return -1;
    if (attn_fill_random(a)) return -1;
    double ms;
    if (timed_launches(warmup, iters, [&] { attn_step(a, 0); }, &ms))
        return -1;
    LG_CHECK(hipGetLastError());
    if (ms_per_step_out) *ms_per_step_out = ms;
    if (kv_gbps_out) *kv_gbps_out = attn_kv_bytes(a) / (ms * 1e-3) / 1e9;
    return 0;
}

int lg_attn_decode_bench(int device, int batch, int hq, int hkv, int ctx, int d,
                         int warmup, int iters, double* ms_per_step_out,
                         double* kv_gbps_out)
{
    return lg_attn_decode_bench_splits(device, batch, hq, hkv, ctx, d, 0,
                                       warmup, iters, ms_per_step_out,
                                       kv_gbps_out);
}

// Attention burn: the shared closed-loop duty engine over attention steps —
// the KV-cache side of a decode pod (busy%, bandwidth-bound, bytes per step
// set by batch and context).
int lg_attn_decode_burn(int device, double target_util_pct, double seconds,
                        int batch, int hq, int hkv, int ctx, int d,
                        double period_ms, volatile int* stop_flag,
                        double* kv_gbps_out)
{
    if (kv_gbps_out) *kv_gbps_out = 0;
    burn_args(target_util_pct, period_ms);
    if (!attn_dims_ok(batch, hq, hkv, ctx, d, 0, nullptr)) return -1;
    LG_CHECK(hipSetDevice(device));
    AttnBufs a;
    if (attn_alloc(a, batch, hq, hkv, ctx, 0, 0)) return -1;
    if (attn_fill_random(a)) return -1;
    double active_ms = 0, steps = 0;
    if (step_burn(target_util_pct, seconds, period_ms, stop_flag,
                  [&] { attn_step(a, 0); }, active_ms, steps))
        return -1;
    if (kv_gbps_out && active_ms > 0)
        *kv_gbps_out = steps * attn_kv_bytes(a) / (active_ms * 1e-3) / 1e9;
    return 0;
}

const char* lg_last_error() { return g_last_error; }

int lg_device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
