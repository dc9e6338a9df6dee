// loadgen_api.h — the C ABI of libmi355x_loadgen.so.
//
// Included by loadgen_lib.cpp (which defines these) and loadgen_main.cpp
// (which calls them), so a signature drift is a compile error. The ctypes
// bindings in mi355x_gpu_hpa/loadgen mirror this file by hand.
//
// Every entry returns 0 on success and -1 on error; lg_last_error() then
// names the failing call. Burn entries: target_util_pct is clamped to
// 0..100, period_ms <= 0 means 100 ms, dimensions <= 0 mean the entry's
// default, stop_flag is optional and polled between periods.

#pragma once

#ifdef __cplusplus
extern "C" {
#endif

const char* lg_last_error();
int lg_device_count();

// vectorAdd: `iters` launches with a host sync each; *ms_out = total ms.
int lg_vector_add_loop(int device, int n, int iters, double* ms_out);
int lg_vector_add_verify(int device, const float* a_h, const float* b_h,
                         float* c_out, int n);

// bf16 GEMM, C f32 = A @ Bt^T. `variant` selects the kernel (the table in
// loadgen_lib.cpp); the plain entries use variant 1. Bench: mean ms per
// GEMM and 2*M*N*K / time. Verify: caller data (f32, converted to bf16).
int lg_gemm_bf16_bench(int device, int m, int n, int k, int warmup, int iters,
                       double* ms_out, double* tflops_out);
int lg_gemm_bf16_bench_variant(int device, int m, int n, int k, int warmup,
                               int iters, int variant, double* ms_out,
                               double* tflops_out);
int lg_gemm_bf16_verify(int device, const float* a_h, const float* bt_h,
                        float* c_out, int m, int n, int k);
int lg_gemm_bf16_verify_variant(int device, const float* a_h,
                                const float* bt_h, float* c_out, int m, int n,
                                int k, int variant);
int lg_gemm_burn(int device, double target_util_pct, double seconds, int m,
                 int n, int k, double period_ms, volatile int* stop_flag);

// Streaming-triad HBM burn over ~gb GiB; *gbps_out = GB/s over the bursts.
int lg_bw_burn(int device, double target_util_pct, double seconds, double gb,
               double period_ms, volatile int* stop_flag, double* gbps_out);

// fp8 (E4M3) GEMM. raster: 1 = product (4x4 super-tile), 0 = linear,
// 2 = deep-B rotation. Verify quantizes the f32 inputs and also writes the
// DEQUANTIZED inputs (aq/btq) so the caller can compute the exact reference
// on what the GPU multiplied; the plain verify is raster 1.
int lg_gemm_fp8_bench(int device, int m, int n, int k, int warmup, int iters,
                      int raster, double* ms_out, double* tflops_out);
int lg_gemm_fp8_verify(int device, const float* a_h, const float* bt_h,
                       float* c_out, float* aq_out, float* btq_out, int m,
                       int n, int k);
int lg_gemm_fp8_verify_variant(int device, const float* a_h, const float* bt_h,
                               float* c_out, float* aq_out, float* btq_out,
                               int m, int n, int k, int raster);
int lg_gemm_fp8_burn(int device, double target_util_pct, double seconds, int m,
                     int n, int k, double period_ms, volatile int* stop_flag);

// MXFP4 GEMM (format and quantizer: mxfp4_host.h). Verify as for fp8;
// max_ctas > 0 caps the grid so a small shape runs the tiles-per-CTA loop.
int lg_gemm_mxfp4_bench(int device, int m, int n, int k, int warmup, int iters,
                        double* ms_out, double* tflops_out);
int lg_gemm_mxfp4_verify(int device, const float* a_h, const float* bt_h,
                         float* c_out, float* aq_out, float* btq_out, int m,
                         int n, int k, int max_ctas);
int lg_gemm_mxfp4_burn(int device, double target_util_pct, double seconds,
                       int m, int n, int k, double period_ms,
                       volatile int* stop_flag);

// Decode-phase MXFP4 weight streaming: x_h[m][k], w_h[layers][n][k] ->
// c_out[layers][m][n], 1 <= m <= 64. k_splits: 0 = the product heuristic,
// > 0 forces that many K slices across CTAs (must divide k/128). Bench:
// mean ms per step (one pass over the ring) and the weight stream rate,
// layers * (N*K/2 + N*K/32) bytes / step time. Burn: weight bytes streamed
// / GPU-active time of the bursts.
int lg_decode_mxfp4_verify(int device, const float* x_h, const float* w_h,
                           float* c_out, float* xq_out, float* wq_out, int m,
                           int n, int k, int layers, int k_splits);
int lg_decode_mxfp4_bench(int device, int m, int n, int k, int layers,
                          int warmup, int iters, double* ms_per_step_out,
                          double* weight_gbps_out);
int lg_decode_mxfp4_burn(int device, double target_util_pct, double seconds,
                         int m, int n, int k, int layers, double period_ms,
                         volatile int* stop_flag, double* weight_gbps_out);

// Decode attention over a contiguous bf16 KV cache: q_h[batch][hq][d],
// k_h and v_h [batch][hkv][lmax][d], seq_lens[batch] in 1..lmax ->
// o_out[batch][hq][d], lse_out[batch][hq] (natural log). d must be 128, hq
// a multiple of hkv with at most 16 q heads per kv head; inputs are f32,
// converted to bf16. kv_splits: 0 = the product heuristic, > 0 forces that
// many splits of the context across CTAs (<= ceil(lmax/32)). scale <= 0
// means 1/sqrt(d). These entries have no dimension defaults: a dimension
// below 1 is an error, like every other bad argument, before any device
// call. Bench and burn: every sequence is ctx long; kv_gbps is
// batch*hkv*ctx*2*d*2 bytes / step time (burn: / GPU-active time of the
// bursts).
int lg_attn_decode_verify(int device, const float* q_h, const float* k_h,
                          const float* v_h, const int* seq_lens, float* o_out,
                          float* lse_out, int batch, int hq, int hkv, int lmax,
                          int d, int kv_splits, double scale);
int lg_attn_decode_bench(int device, int batch, int hq, int hkv, int ctx, int d,
                         int warmup, int iters, double* ms_per_step_out,
                         double* kv_gbps_out);
// The bench with kv_splits forced (> 0) instead of the heuristic (0).
int lg_attn_decode_bench_splits(int device, int batch, int hq, int hkv, int ctx,
                                int d, int kv_splits, int warmup, int iters,
                                double* ms_per_step_out, double* kv_gbps_out);
int lg_attn_decode_burn(int device, double target_util_pct, double seconds,
                        int batch, int hq, int hkv, int ctx, int d,
                        double period_ms, volatile int* stop_flag,
                        double* kv_gbps_out);

#ifdef __cplusplus
}
#endif
