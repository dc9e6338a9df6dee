// mxfp4_host.h — OCP MX FP4 (E2M1 elements + E8M0 block scales) on the host.
//
// Header-only, plain C++ (no HIP): shared by the load-generator library
// (loadgen_lib.cpp), the host-only C API (mxfp4_capi.cpp) and the
// sanitizer self-test (mxfp4_selftest.cpp).
//
// Public data format (what callers see; fixed):
//   elements  [rows][k/2] bytes, element 2i in bits 3:0, element 2i+1 in
//             bits 7:4. An E2M1 code is sign (bit 3), 2 exponent bits, 1
//             mantissa bit; magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}.
//   scales    [rows][k/32] bytes, E8M0: value 2^(byte-127). 255 (NaN) is
//             never produced.
// Quantizer (OCP MX v1.0, per 32-element block of a row):
//   e = floor(log2(amax)) - 2, clamped to [-127, 127]; each element is
//   x / 2^e rounded to nearest, ties to the even code, saturating at +-6.
//   An all-zero block gives scale byte 127 and all codes 0. A value that
//   rounds to zero is stored as code 0 (never the negative-zero code 8).
//   Non-finite input is an error, not an encoding.
//
// The device-side scale layout (shuffle_scales) is private to the kernels in
// gemm_mxfp4_256.hip and gemm_mxfp4_decode.hip and may change; the public
// format does not.

#ifndef MI355X_MXFP4_HOST_H
#define MI355X_MXFP4_HOST_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace mxfp4 {

constexpr int kBlock = 32;  // elements per E8M0 scale

// Magnitude of an E2M1 code's low three bits.
inline float e2m1_magnitude(unsigned code)
{
    static const float mag[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    return mag[code & 7];
}

inline float e2m1_value(unsigned code)
{
    float v = e2m1_magnitude(code);
    return (code & 8) ? -v : v;
}

// |v| (already divided by the block scale) -> magnitude code 0..7.
// Midpoints go to the even code; anything above 5 saturates to 6.
inline unsigned e2m1_encode_magnitude(double av)
{
    if (av <= 0.25) return 0;
    if (av < 0.75) return 1;
    if (av <= 1.25) return 2;
    if (av < 1.75) return 3;
    if (av <= 2.5) return 4;
    if (av < 3.5) return 5;
    if (av <= 5.0) return 6;
    return 7;
}

// Shared block exponent from floor(log2(amax)): minus the E2M1 maximum's
// exponent (2), clamped to what an E8M0 byte 0..254 can say.
inline int block_exponent(int floor_log2_amax)
{
    int e = floor_log2_amax - 2;
    if (e < -127) e = -127;
    if (e > 127) e = 127;
    return e;
}

// Quantize x[rows][k] (k % 32 == 0). Writes packed[rows][k/2],
// scales[rows][k/32] and, if deq != nullptr, the dequantized values
// deq[rows][k]. Returns 0, or -1 with a message in err (if given).
inline int quantize(const float* x, long rows, int k, unsigned char* packed,
                    unsigned char* scales, float* deq, char* err = nullptr,
                    size_t errlen = 0)
{
    if (rows < 0 || k <= 0 || k % kBlock) {
        if (err)
            std::snprintf(err, errlen,
                          "mxfp4 quantize: k must be a positive multiple of %d",
                          kBlock);
        return -1;
    }
    const long nblocks = rows * (long)(k / kBlock);
    for (long b = 0; b < nblocks; ++b) {
        const float* xb = x + b * kBlock;
        float amax = 0.f;
        for (int i = 0; i < kBlock; ++i) {
            if (!std::isfinite(xb[i])) {
                if (err)
                    std::snprintf(err, errlen,
                                  "mxfp4 quantize: non-finite input at "
                                  "element %ld",
                                  b * kBlock + i);
                return -1;
            }
            float a = std::fabs(xb[i]);
            if (a > amax) amax = a;
        }
        int e = 0;
        if (amax > 0.f) {
            int ex;
            (void)std::frexp(amax, &ex);  // amax = m * 2^ex, m in [0.5, 1)
            e = block_exponent(ex - 1);
        }
        scales[b] = (unsigned char)(e + 127);
        unsigned char* pb = packed + b * (kBlock / 2);
        for (int i = 0; i < kBlock; i += 2) {
            unsigned c[2];
            for (int j = 0; j < 2; ++j) {
                // exact in double: |e| <= 127 and f32 spans 2^-149..2^128
                double v = std::ldexp((double)xb[i + j], -e);
                unsigned m = e2m1_encode_magnitude(std::fabs(v));
                c[j] = (m && v < 0) ? (m | 8) : m;
                if (deq) deq[b * kBlock + i + j] = std::ldexp(e2m1_value(c[j]), e);
            }
            pb[i / 2] = (unsigned char)(c[0] | (c[1] << 4));
        }
    }
    return 0;
}

inline void dequantize(const unsigned char* packed, const unsigned char* scales,
                       long rows, int k, float* out)
{
    const long n = rows * (long)k;
    for (long i = 0; i < n; ++i) {
        unsigned byte = packed[i >> 1];
        unsigned code = (i & 1) ? (byte >> 4) : (byte & 15);
        out[i] = std::ldexp(e2m1_value(code), (int)scales[i / kBlock] - 127);
    }
}

// Device scale layout for gemm_mxfp4_tn_256 and the decode kernels
// (rows % 64 == 0, k % 128 == 0):
// one dword per lane carries the scale bytes of four 16-row MFMA fragments
// for one 128-wide k-step, so the instruction's byte select picks the
// fragment. out[g][s][lane][j] = scales[g*64 + j*16 + (lane & 15)]
//                                      [s*4 + (lane >> 4)]
// with g = row / 64, s = k / 128, lane 0..63, j 0..3.
inline void shuffle_scales(const unsigned char* scales, int rows, int k,
                           unsigned char* out)
{
    const int ksteps = k / 128, kblocks = k / kBlock;
    for (int g = 0; g < rows / 64; ++g)
        for (int s = 0; s < ksteps; ++s)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j)
                    out[(((size_t)g * ksteps + s) * 64 + lane) * 4 + j] =
                        scales[(size_t)(g * 64 + j * 16 + (lane & 15)) * kblocks +
                               s * 4 + (lane >> 4)];
}

}  // namespace mxfp4

#endif  // MI355X_MXFP4_HOST_H
