// mxfp4_selftest.cpp — stand-alone check of mxfp4_host.h, meant to be built
// with -fsanitize=address,undefined (make mxfp4-selftest). Every buffer is
// heap-allocated at its exact size so an overrun is caught. Exits non-zero
// on the first mismatch; prints nothing on success.

#include "mxfp4_host.h"

#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <vector>

static int g_fail = 0;

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__,     \
                         __LINE__, #cond);                                   \
            ++g_fail;                                                        \
        }                                                                    \
    } while (0)

struct Q {
    std::vector<unsigned char> packed, scales;
    std::vector<float> deq;
    int rc;
};

static Q quant(const std::vector<float>& x, int rows, int k)
{
    Q q;
    q.packed.assign((size_t)rows * k / 2, 0xAA);
    q.scales.assign((size_t)rows * k / 32, 0xAA);
    q.deq.assign((size_t)rows * k, -1.f);
    q.rc = mxfp4::quantize(x.data(), rows, k, q.packed.data(), q.scales.data(),
                           q.deq.data());
    return q;
}

static unsigned code_at(const Q& q, size_t i)
{
    unsigned b = q.packed[i / 2];
    return (i & 1) ? (b >> 4) : (b & 15);
}

static bool same_bits(float a, float b) { return !std::memcmp(&a, &b, 4); }

int main()
{
    // every code, in element order (pins the nibble order), scale 2^3
    {
        std::vector<float> x(32, 0.f);
        for (unsigned c = 0; c < 16; ++c) x[c] = mxfp4::e2m1_value(c) * 8.f;
        Q q = quant(x, 1, 32);
        EXPECT(q.rc == 0);
        EXPECT(q.scales[0] == 127 + 3);
        for (unsigned c = 0; c < 16; ++c) {
            unsigned want = (c == 8) ? 0 : c;  // -0 is stored as +0
            EXPECT(code_at(q, c) == want);
            EXPECT(q.deq[c] == x[c]);
        }
        EXPECT((q.packed[0] & 15) == 0 && (q.packed[0] >> 4) == 1);
        EXPECT(q.packed[3] == (6u | (7u << 4)));
    }
    // ties go to the even code, both signs, at scales 2^-5, 1, 2^9
    {
        const float tie[7] = {0.25f, 0.75f, 1.25f, 1.75f, 2.5f, 3.5f, 5.f};
        const unsigned want[7] = {0, 2, 2, 4, 4, 6, 6};
        const int exps[3] = {-5, 0, 9};
        for (int ei = 0; ei < 3; ++ei) {
            float s = std::ldexp(1.f, exps[ei]);
            std::vector<float> x(32, 0.f);
            x[0] = 6.f * s;  // anchors e = exps[ei]
            for (int t = 0; t < 7; ++t) {
                x[1 + t] = tie[t] * s;
                x[8 + t] = -tie[t] * s;
            }
            x[15] = std::nextafter(0.25f, 1.f) * s;  // just above a tie
            x[16] = std::nextafter(5.f, 6.f) * s;
            Q q = quant(x, 1, 32);
            EXPECT(q.rc == 0);
            EXPECT(q.scales[0] == 127 + exps[ei]);
            for (int t = 0; t < 7; ++t) {
                EXPECT(code_at(q, 1 + t) == want[t]);
                EXPECT(code_at(q, 8 + t) == (want[t] ? (want[t] | 8) : 0));
            }
            EXPECT(code_at(q, 15) == 1);
            EXPECT(code_at(q, 16) == 7);
        }
    }
    // saturation: (6, 8) * 2^e all land on 6
    {
        std::vector<float> x(32, 0.f);
        x[0] = 7.9f;
        x[1] = -7.f;
        x[2] = 6.5f;
        x[3] = 4.f;
        Q q = quant(x, 1, 32);
        EXPECT(q.rc == 0 && q.scales[0] == 127);
        EXPECT(code_at(q, 0) == 7 && code_at(q, 1) == 15 && code_at(q, 2) == 7);
        EXPECT(q.deq[0] == 6.f && q.deq[1] == -6.f && q.deq[3] == 4.f);
    }
    // zero blocks (both zero signs) next to a live block
    {
        std::vector<float> x(96, 0.f);
        for (int i = 0; i < 32; ++i) x[i] = (i & 1) ? -0.f : 0.f;
        x[40] = 1.f;
        Q q = quant(x, 1, 96);
        EXPECT(q.rc == 0);
        EXPECT(q.scales[0] == 127 && q.scales[2] == 127);
        EXPECT(q.scales[1] == 127 - 2);
        for (int i = 0; i < 16; ++i) EXPECT(q.packed[i] == 0 && q.packed[32 + i] == 0);
        for (int i = 0; i < 32; ++i) EXPECT(same_bits(q.deq[i], 0.f));
        EXPECT(code_at(q, 40) == 6 && q.deq[40] == 1.f);
    }
    // low scale clamp: floor(log2(amax)) - 2 < -127
    {
        std::vector<float> x(64, 0.f);
        x[0] = std::ldexp(1.f, -127);    // subnormal
        x[1] = std::ldexp(1.f, -149);    // smallest subnormal
        x[32] = std::ldexp(1.5f, -126);  // e would be -128
        x[33] = -std::ldexp(1.f, -128);
        Q q = quant(x, 1, 64);
        EXPECT(q.rc == 0);
        EXPECT(q.scales[0] == 0 && q.scales[1] == 0);
        EXPECT(code_at(q, 0) == 2 && same_bits(q.deq[0], x[0]));
        EXPECT(code_at(q, 1) == 0 && same_bits(q.deq[1], 0.f));
        EXPECT(code_at(q, 32) == 5 && same_bits(q.deq[32], x[32]));
        EXPECT(code_at(q, 33) == 9 && same_bits(q.deq[33], x[33]));
    }
    // high end: the largest finite f32 gives e = 125 (byte 252); the upper
    // clamp itself is only reachable through block_exponent()
    {
        std::vector<float> x(32, 0.f);
        x[0] = FLT_MAX;
        x[1] = -std::ldexp(1.f, 127);
        Q q = quant(x, 1, 32);
        EXPECT(q.rc == 0 && q.scales[0] == 252);
        EXPECT(code_at(q, 0) == 7 && q.deq[0] == std::ldexp(6.f, 125));
        EXPECT(code_at(q, 1) == 14 && q.deq[1] == x[1]);
        EXPECT(mxfp4::block_exponent(127) == 125);
        EXPECT(mxfp4::block_exponent(200) == 127);
        EXPECT(mxfp4::block_exponent(-126) == -127);
        EXPECT(mxfp4::block_exponent(-400) == -127);
    }
    // rows*k = 288 (a multiple of 32 and of nothing larger): round trips
    {
        const int rows = 3, k = 96;
        std::vector<float> x((size_t)rows * k);
        unsigned st = 12345u;
        for (size_t i = 0; i < x.size(); ++i) {
            st = st * 1664525u + 1013904223u;
            float u = ((st >> 8) & 0xffff) / 32768.f - 1.f;
            x[i] = std::ldexp(u, (int)((st >> 26) % 13) - 6);
        }
        Q q = quant(x, rows, k);
        EXPECT(q.rc == 0);
        std::vector<float> back(x.size(), -1.f);
        mxfp4::dequantize(q.packed.data(), q.scales.data(), rows, k, back.data());
        for (size_t i = 0; i < x.size(); ++i) EXPECT(same_bits(back[i], q.deq[i]));
        for (size_t b = 0; b < x.size() / 32; ++b) {
            float amax = 0;
            for (int i = 0; i < 32; ++i) amax = std::fmax(amax, std::fabs(x[b * 32 + i]));
            for (int i = 0; i < 32; ++i)
                EXPECT(std::fabs(q.deq[b * 32 + i] - x[b * 32 + i]) <= amax / 4);
        }
        // a dequantized tensor whose block maximum is a power-of-two times
        // 4 or 6 re-quantizes to itself
        std::vector<float> y(64, 0.f);
        for (int i = 0; i < 64; ++i) y[i] = mxfp4::e2m1_value((i * 7) & 15) * 0.5f;
        y[0] = 6.f * 0.5f;
        y[32] = -4.f * 0.5f;
        Q q2 = quant(y, 2, 32);
        EXPECT(q2.rc == 0);
        for (int i = 0; i < 64; ++i) EXPECT(q2.deq[i] == y[i]);
    }
    // errors: non-finite input, bad k; deq may be null
    {
        std::vector<float> x(32, 1.f);
        std::vector<unsigned char> p(16), s(1);
        char err[128] = "";
        x[31] = INFINITY;
        EXPECT(mxfp4::quantize(x.data(), 1, 32, p.data(), s.data(), nullptr, err,
                               sizeof(err)) == -1);
        EXPECT(std::strstr(err, "non-finite") != nullptr);
        x[31] = NAN;
        EXPECT(mxfp4::quantize(x.data(), 1, 32, p.data(), s.data(), nullptr) == -1);
        x[31] = 1.f;
        EXPECT(mxfp4::quantize(x.data(), 1, 32, p.data(), s.data(), nullptr) == 0);
        EXPECT(mxfp4::quantize(x.data(), 2, 16, p.data(), s.data(), nullptr) == -1);
    }
    // device scale shuffle is a permutation with the documented index map
    {
        const int rows = 128, k = 256, kb = k / 32;
        std::vector<unsigned char> sc((size_t)rows * kb), out(sc.size(), 0);
        for (size_t i = 0; i < sc.size(); ++i) sc[i] = (unsigned char)(i * 37 + 11);
        mxfp4::shuffle_scales(sc.data(), rows, k, out.data());
        for (int g = 0; g < rows / 64; ++g)
            for (int s = 0; s < k / 128; ++s)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j)
                        EXPECT(out[(((size_t)g * (k / 128) + s) * 64 + lane) * 4 + j] ==
                               sc[(size_t)(g * 64 + j * 16 + (lane & 15)) * kb + s * 4 +
                                  (lane >> 4)]);
        long sum_in = 0, sum_out = 0;
        for (size_t i = 0; i < sc.size(); ++i) {
            sum_in += sc[i];
            sum_out += out[i];
        }
        EXPECT(sum_in == sum_out);
    }
    return g_fail ? 1 : 0;
}
