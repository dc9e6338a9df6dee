// loadgen_main.cpp — `mi355x-loadgen` CLI.
//
// The container entrypoint for the autoscaled workload pods (replacement for
// the reference's `for (( c=1; c<=5000; c++ )); do ./vectorAdd; done`,
// cuda-test-deployment.yaml:19). Modes:
//
//   mi355x-loadgen vectoradd [--n 50000] [--iters 5000] [--device 0]
//       the reference's load shape: tiny kernel, launch-bound, a few % util
//   mi355x-loadgen gemm [--m/--n-dim/--k 4096] [--iters 50] [--device 0]
//       one timed MFMA bf16 GEMM burst; prints ms + TFLOP/s
//   mi355x-loadgen fp8gemm [--m/--n-dim/--k 8192] [--iters 10] [--no-raster]
//       one timed fp8 (E4M3) MFMA GEMM burst
//   mi355x-loadgen fp4gemm [--m/--n-dim/--k 8192] [--iters 10]
//       one timed MXFP4 (E2M1 + E8M0 block scale) MFMA GEMM burst
//   mi355x-loadgen burn --util 80 [--seconds 60] [--device 0] [--fp8|--fp4]
//       duty-cycled GEMM load at a target busy%% (tunable HPA-test load);
//       --fp8 / --fp4 burn with the E4M3 / MXFP4 kernel instead of bf16
//   mi355x-loadgen decode [--batch 16] [--n-dim 8192] [--k 8192]
//                         [--layers 16] [--iters 10]
//       timed decode steps: a skinny-M MXFP4 GEMM streaming a ring of
//       weight matrices; prints ms per step, weight GB/s, ring footprint
//   mi355x-loadgen decodeburn --util 80 [--seconds 60] [--batch 16]
//                         [--n-dim 8192] [--k 8192] [--layers 16]
//       duty-cycled decode load (busy%% high, HBM-bandwidth-bound): the
//       load shape of a small-batch MXFP4 serving pod
//   mi355x-loadgen attn [--batch 32] [--q-heads 64] [--kv-heads 8]
//                       [--ctx 8192] [--iters 10]
//       timed decode-attention steps over a contiguous bf16 KV cache (head
//       dimension 128); prints ms per step, KV GB/s, cache footprint
//   mi355x-loadgen attnburn --util 80 [--seconds 60] [--batch 32]
//                       [--q-heads 64] [--kv-heads 8] [--ctx 8192]
//       duty-cycled decode-attention load: the KV-cache side of a decode
//       pod, HBM bytes per step set by batch and context
//   mi355x-loadgen bwburn --util 80 [--seconds 60] [--gb 6]
//       duty-cycled streaming-triad HBM load
//
// Exit code 0 on success, 1 on usage error, 2 on HIP error.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "loadgen_api.h"

static double argd(int argc, char** argv, const char* flag, double dflt)
{
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], flag)) return std::atof(argv[i + 1]);
    return dflt;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr,
                     "usage: mi355x-loadgen {vectoradd|gemm|fp8gemm|fp4gemm|burn|decode|decodeburn|attn|attnburn|bwburn|devices} [flags]\n");
        return 1;
    }
    std::string mode = argv[1];
    int device = (int)argd(argc, argv, "--device", 0);

    if (mode == "devices") {
        std::printf("%d\n", lg_device_count());
        return 0;
    }
    if (mode == "vectoradd") {
        int n = (int)argd(argc, argv, "--n", 50000);
        int iters = (int)argd(argc, argv, "--iters", 5000);
        double ms = 0;
        if (lg_vector_add_loop(device, n, iters, &ms)) {
            std::fprintf(stderr, "error: %s\n", lg_last_error());
            return 2;
        }
        std::printf("vectoradd n=%d iters=%d total_ms=%.1f ms_per_iter=%.3f\n",
                    n, iters, ms, ms / iters);
        return 0;
    }
    if (mode == "gemm") {
        int m = (int)argd(argc, argv, "--m", 4096);
        int n = (int)argd(argc, argv, "--n-dim", 4096);
        int k = (int)argd(argc, argv, "--k", 4096);
        int iters = (int)argd(argc, argv, "--iters", 50);
        int warmup = (int)argd(argc, argv, "--warmup", 5);
        int variant = 1;
        for (int i = 1; i < argc; ++i) {
            if (!std::strcmp(argv[i], "--linear")) variant = 0;
            if (!std::strcmp(argv[i], "--v256")) variant = 2;
        }
        int vflag = (int)argd(argc, argv, "--variant", -1);
        if (vflag >= 0) variant = vflag;
        double ms = 0, tf = 0;
        if (lg_gemm_bf16_bench_variant(device, m, n, k, warmup, iters, variant,
                                       &ms, &tf)) {
            std::fprintf(stderr, "error: %s\n", lg_last_error());
            return 2;
        }
        char vname[16] = "";
        if (variant == 0) std::snprintf(vname, sizeof(vname), "_linear");
        else if (variant >= 2) std::snprintf(vname, sizeof(vname), "_v%d", variant);
        std::printf("gemm_bf16%s %dx%dx%d ms=%.3f tflops=%.1f\n",
                    vname, m, n, k, ms, tf);
        return 0;
    }
    if (mode == "fp8gemm") {
        int m = (int)argd(argc, argv, "--m", 8192);
        int n = (int)argd(argc, argv, "--n-dim", 8192);
        int k = (int)argd(argc, argv, "--k", 8192);
        int iters = (int)argd(argc, argv, "--iters", 10);
        int warmup = (int)argd(argc, argv, "--warmup", 2);
        int raster = 1;
        for (int i = 1; i < argc; ++i)
            if (!std::strcmp(argv[i], "--no-raster")) raster = 0;
        double ms = 0, tf = 0;
        if (lg_gemm_fp8_bench(device, m, n, k, warmup, iters, raster, &ms,
                              &tf)) {
            std::fprintf(stderr, "error: %s\n", lg_last_error());
            return 2;
        }
        std::printf("gemm_fp8 %dx%dx%d ms=%.3f tflops=%.1f\n", m, n, k, ms, tf);
        return 0;
    }
    if (mode == "fp4gemm") {
        int m = (int)argd(argc, argv, "--m", 8192);
        int n = (int)argd(argc, argv, "--n-dim", 8192);
        int k = (int)argd(argc, argv, "--k", 8192);
        int iters = (int)argd(argc, argv, "--iters", 10);
        int warmup = (int)argd(argc, argv, "--warmup", 2);
        double ms = 0, tf = 0;
        if (lg_gemm_mxfp4_bench(device, m, n, k, warmup, iters, &ms, &tf)) {
            std::fprintf(stderr, "error: %s\n", lg_last_error());
            return 2;
        }
        std::printf("gemm_mxfp4 %dx%dx%d ms=%.3f tflops=%.1f\n", m, n, k, ms,
                    tf);
        return 0;
    }
    if (mode == "burn") {
        double util = argd(argc, argv, "--util", 80.0);
        double seconds = argd(argc, argv, "--seconds", 60.0);
        int m = (int)argd(argc, argv, "--m", 4096);
        int n = (int)argd(argc, argv, "--n-dim", 4096);
        int k = (int)argd(argc, argv, "--k", 4096);
        double period = argd(argc, argv, "--period-ms", 100.0);
        bool fp8 = false, fp4 = false;
        for (int i = 1; i < argc; ++i) {
            if (!std::strcmp(argv[i], "--fp8")) fp8 = true;
            if (!std::strcmp(argv[i], "--fp4")) fp4 = true;
        }
        if (fp8 && fp4) {
            std::fprintf(stderr, "burn: --fp8 and --fp4 are exclusive\n");
            return 1;
        }
        int rc = fp4   ? lg_gemm_mxfp4_burn(device, util, seconds, m, n, k,
                                            period, nullptr)
                 : fp8 ? lg_gemm_fp8_burn(device, util, seconds, m, n, k,
                                          period, nullptr)
                       : lg_gemm_burn(device, util, seconds, m, n, k, period,
                                      nullptr);
        if (rc) {
            std::fprintf(stderr, "error: %s\n", lg_last_error());
            return 2;
        }
        return 0;
    }
    if (mode == "decode" || mode == "decodeburn") {
        int m = (int)argd(argc, argv, "--batch", 16);
        int n = (int)argd(argc, argv, "--n-dim", 8192);
        int k = (int)argd(argc, argv, "--k", 8192);
        int layers = (int)argd(argc, argv, "--layers", 16);
        double ms = 0, gbps = 0;
        int rc;
        if (mode == "decode") {
            int iters = (int)argd(argc, argv, "--iters", 10);
            int warmup = (int)argd(argc, argv, "--warmup", 2);
            rc = lg_decode_mxfp4_bench(device, m, n, k, layers, warmup, iters,
                                       &ms, &gbps);
        } else {
            double util = argd(argc, argv, "--util", 80.0);
            double seconds = argd(argc, argv, "--seconds", 60.0);
            double period = argd(argc, argv, "--period-ms", 100.0);
            rc = lg_decode_mxfp4_burn(device, util, seconds, m, n, k, layers,
                                      period, nullptr, &gbps);
        }
        if (rc) {
            std::fprintf(stderr, "error: %s\n", lg_last_error());
            return 2;
        }
        const double ring_mib =
            (double)layers * ((double)n * k / 2 + (double)n * k / 32) /
            (1 << 20);
        if (mode == "decode")
            std::printf("decode_mxfp4 batch=%d %dx%d layers=%d ms_per_step=%.3f "
                        "weight_gbps=%.0f ring_mib=%.0f\n",
                        m, n, k, layers, ms, gbps, ring_mib);
        else
            std::printf("decodeburn batch=%d %dx%d layers=%d weight_gbps=%.0f "
                        "during bursts ring_mib=%.0f\n",
                        m, n, k, layers, gbps, ring_mib);
        if (ring_mib < 512)
            std::printf("note: a %.0f MiB ring is below 512 MiB and stays in "
                        "the 256 MiB Infinity Cache in part or whole; this is "
                        "not an HBM reading\n",
                        ring_mib);
        return 0;
    }
    if (mode == "attn" || mode == "attnburn") {
        int batch = (int)argd(argc, argv, "--batch", 32);
        int hq = (int)argd(argc, argv, "--q-heads", 64);
        int hkv = (int)argd(argc, argv, "--kv-heads", 8);
        int ctx = (int)argd(argc, argv, "--ctx", 8192);
        const int d = 128;
        double ms = 0, gbps = 0;
        int rc;
        if (mode == "attn") {
            int iters = (int)argd(argc, argv, "--iters", 10);
            int warmup = (int)argd(argc, argv, "--warmup", 2);
            rc = lg_attn_decode_bench(device, batch, hq, hkv, ctx, d, warmup,
                                      iters, &ms, &gbps);
        } else {
            double util = argd(argc, argv, "--util", 80.0);
            double seconds = argd(argc, argv, "--seconds", 60.0);
            double period = argd(argc, argv, "--period-ms", 100.0);
            rc = lg_attn_decode_burn(device, util, seconds, batch, hq, hkv,
                                     ctx, d, period, nullptr, &gbps);
        }
        if (rc) {
            std::fprintf(stderr, "error: %s\n", lg_last_error());
            return 2;
        }
        const double cache_mib =
            (double)batch * hkv * ctx * 2 * d * 2 / (1 << 20);
        if (mode == "attn")
            std::printf("attn_decode batch=%d q_heads=%d kv_heads=%d ctx=%d "
                        "ms_per_step=%.3f kv_gbps=%.0f cache_mib=%.0f\n",
                        batch, hq, hkv, ctx, ms, gbps, cache_mib);
        else
            std::printf("attnburn batch=%d q_heads=%d kv_heads=%d ctx=%d "
                        "kv_gbps=%.0f during bursts cache_mib=%.0f\n",
                        batch, hq, hkv, ctx, gbps, cache_mib);
        if (cache_mib < 512)
            std::printf("note: a %.0f MiB cache is below 512 MiB and stays in "
                        "the 256 MiB Infinity Cache in part or whole; this is "
                        "not an HBM reading\n",
                        cache_mib);
        return 0;
    }
    if (mode == "bwburn") {
        double util = argd(argc, argv, "--util", 80.0);
        double seconds = argd(argc, argv, "--seconds", 60.0);
        double gb = argd(argc, argv, "--gb", 6.0);
        double period = argd(argc, argv, "--period-ms", 100.0);
        double gbps = 0;
        if (lg_bw_burn(device, util, seconds, gb, period, nullptr, &gbps)) {
            std::fprintf(stderr, "error: %s\n", lg_last_error());
            return 2;
        }
        std::printf("bwburn util=%.0f%% achieved=%.0f GB/s during bursts\n",
                    util, gbps);
        return 0;
    }
    std::fprintf(stderr, "unknown mode '%s'\n", mode.c_str());
    return 1;
}
