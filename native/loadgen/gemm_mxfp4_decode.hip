// gemm_mxfp4_decode.hip — decode-phase (skinny-M) MXFP4 weight-streaming
// GEMM for MI355X (gfx950).
//
// C[L][M][N] f32 = dq(X)[M][K] @ dq(W[L])[N][K]^T for a ring of L weight
// matrices and ONE activation block X, 1 <= M <= 64, N % 64 == 0,
// K % 128 == 0. Both operands are MXFP4 (a4w4) in the public format of
// mxfp4_host.h; the matrix core takes them exactly as gemm_mxfp4_256.hip
// does: v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz:4 blgp:4, lane l holds
// row l&15, k 32*(l>>4)..+31 of the 128-wide step as 16 contiguous bytes,
// and the lane's E8M0 byte applies to exactly that block.
//
// The shape is memory-bound: every W byte is used once by one wave, so W
// goes straight from global memory into VGPRs with 16-B loads (a lane's
// load is one OCP block of one W row; no LDS round trip, no repack).
//
//   * One launch covers the whole ring: CTA = (layer, 64-row N group,
//     K slice), 256 threads. At the default ring that is 2048 CTAs.
//   * A wave owns all four 16-row W fragments of the group for its k-steps
//     and multiplies each against every X fragment (MF = ceil(M/16), a
//     template parameter), so an X fragment fetched once (L2-resident) is
//     used four times.
//   * The four waves of a CTA split the CTA's K slice into contiguous
//     quarters. A wave walks its quarter two k-steps at a time (the two
//     64-B halves of each W row's 128-B line together), with the next
//     pair's loads issued before the current pair's MFMAs: 8 KiB of W in
//     flight per wave at all times.
//   * Combine: the waves leave their accumulators in LDS and wave w sums
//     W-fragment w over waves 0..3 in that fixed order. With k_splits > 1
//     (few layers / small N: not enough CTAs to fill the chip) each K
//     slice writes its partial C to a workspace and decode_mxfp4_reduce
//     adds the slices in index order. No float atomics anywhere: results
//     are bit-identical from run to run.
//
// Scales are 1/16 of the traffic and use the 64-row-group layout of
// mxfp4::shuffle_scales for both operands: one dword per lane and k-step
// carries the bytes of four 16-row fragments, op_sel picks the fragment.
// X scales are padded to one 64-row group on the host (byte 127); X
// elements are padded to MF*16 rows with zero codes. Rows >= M are never
// stored.

#include "gemm_tile.h"

static __device__ __forceinline__ f32x4 mfma_mxfp4_d(i32x4 a4, i32x4 b4,
                                                     f32x4 c, int oa, int sa,
                                                     int ob, int sb)
{
    // fp4 operands live in elements 0..3 only (4 VGPRs)
    const i32x8 a = {a4[0], a4[1], a4[2], a4[3], 0, 0, 0, 0};
    const i32x8 b = {b4[0], b4[1], b4[2], b4[3], 0, 0, 0, 0};
    return mfma_mxfp4(a, b, c, oa, sa, ob, sb);
}

// Operands of two consecutive k-steps for one wave.
template <int MF>
struct DecodePair {
    i32x4 w[2][4];   // W fragments (16 rows each) of the 64-row group
    i32x4 x[2][MF];  // X fragments
    int sw[2];       // W scale dword: byte j = fragment j
    int sx[2];       // X scale dword: byte i = fragment i
};

template <int MF>
static __device__ __forceinline__ void decode_body(
    const unsigned char* __restrict__ X,   // [MF*16][K/2] packed E2M1
    const int* __restrict__ SX,            // [K/128][64] shuffled E8M0
    const unsigned char* __restrict__ W,   // [layers][N][K/2] packed E2M1
    const int* __restrict__ SW,            // [layers*N/64][K/128][64]
    float* __restrict__ out,  // k_splits == 1: C[layers][M][N];
                              // else partials [k_splits][layers][M][N]
    int M, int N, int K, int layers, int k_splits)
{
    __shared__ f32x4 red[4][MF * 4][64];

    const int tid = threadIdx.x;
    // wave-uniform in an SGPR, so the k-range tests below are scalar
    // branches and not exec-masked regions
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int groups = N >> 6;
    const int kSteps = K >> 7;
    const long KB = K >> 1;  // operand bytes per row

    int id = blockIdx.x;
    const int ks = id % k_splits;
    id /= k_splits;
    const int g = id % groups;
    const int layer = id / groups;

    // this CTA's K slice, and this wave's contiguous quarter of it
    const int S = kSteps / k_splits;
    const int sb = ks * S + (S * w) / 4;
    const int se = ks * S + (S * (w + 1)) / 4;

    const long lane_off = (long)(lane & 15) * KB + (lane >> 4) * 16;
    const unsigned char* wp = W + ((long)layer * N + g * 64) * KB + lane_off;
    const unsigned char* xp = X + lane_off;
    const int* swp = SW + ((long)layer * groups + g) * kSteps * 64 + lane;
    const int* sxp = SX + lane;

    // Loads k-steps s and s+1. full: both steps are known to be in the
    // wave's range; otherwise a second step past it is clamped onto s (in
    // bounds, its values are not used).
    auto load_pair = [&](DecodePair<MF>& p, int s, bool full) {
        const long s1 = (full || s + 1 < se) ? s + 1 : s;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long st = t ? s1 : s;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                p.w[t][j] = *(const i32x4*)(wp + j * 16 * KB + st * 64);
            p.sw[t] = swp[st * 64];
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long st = t ? s1 : s;
#pragma unroll
            for (int i = 0; i < MF; ++i)
                p.x[t][i] = *(const i32x4*)(xp + i * 16 * KB + st * 64);
            p.sx[t] = sxp[st * 64];
        }
    };

    // written out: zero_acc() here changes the generated code
    // (profiles/loadgen_refactor.md)
    f32x4 acc[MF][4];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // A = X (rows m), B = W (cols n)
    auto mma_pair = [&](const DecodePair<MF>& p, int s, bool full) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (t == 0 || full || s + 1 < se) {
#pragma unroll
                for (int i = 0; i < MF; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = mfma_mxfp4_d(p.x[t][i], p.w[t][j],
                                                 acc[i][j], i, p.sx[t], j,
                                                 p.sw[t]);
            }
        }
    };

    if (sb < se) {
        DecodePair<MF> p0, p1;
        int s = sb;
        load_pair(p0, s, false);
        // Steady state has no branch around a load, so the compiler's
        // counted vmcnt leaves the whole next pair in flight behind the
        // current pair's MFMAs (a load under a branch makes it wait for
        // everything at the join).
        while (s + 5 < se) {  // steps s..s+5 exist: three full pairs
            load_pair(p1, s + 2, true);
            mma_pair(p0, s, true);
            load_pair(p0, s + 4, true);
            mma_pair(p1, s + 2, true);
            s += 4;
        }
        // 1..5 steps left, p0 holds s (and s+1)
        if (s + 2 < se) {
            load_pair(p1, s + 2, false);
            mma_pair(p0, s, true);
            if (s + 4 < se) load_pair(p0, s + 4, false);
            mma_pair(p1, s + 2, false);
            if (s + 4 < se) mma_pair(p0, s + 4, false);
        } else {
            mma_pair(p0, s, false);
        }
    }

    // in-CTA split-K combine, fixed order
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[w][i * 4 + j][lane] = acc[i][j];
    __syncthreads();

    float* dst = out + ((long)ks * layers + layer) * M * (long)N;
    const int col = g * 64 + w * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        f32x4 v = red[0][i * 4 + w][lane];
        v += red[1][i * 4 + w][lane];
        v += red[2][i * 4 + w][lane];
        v += red[3][i * 4 + w][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i * 16 + (lane >> 4) * 4 + r;
            if (row < M) dst[(long)row * N + col] = v[r];
        }
    }
}

#define DECODE_KERNEL(NAME, MF)                                               \
    extern "C" __global__ void __launch_bounds__(256) NAME(                   \
        const unsigned char* __restrict__ X, const int* __restrict__ SX,     \
        const unsigned char* __restrict__ W, const int* __restrict__ SW,     \
        float* __restrict__ out, int M, int N, int K, int layers,            \
        int k_splits)                                                         \
    {                                                                         \
        decode_body<MF>(X, SX, W, SW, out, M, N, K, layers, k_splits);        \
    }

DECODE_KERNEL(decode_mxfp4_m16, 1)
DECODE_KERNEL(decode_mxfp4_m32, 2)
DECODE_KERNEL(decode_mxfp4_m48, 3)
DECODE_KERNEL(decode_mxfp4_m64, 4)
#undef DECODE_KERNEL

// Second pass for k_splits > 1: C = P[0] + P[1] + ... in index order.
// n4 = layers*M*N/4 float4s per slice.
extern "C" __global__ void __launch_bounds__(256) decode_mxfp4_reduce(
    const float4* __restrict__ P, float4* __restrict__ C, long n4,
    int k_splits)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (long)gridDim.x * blockDim.x) {
        float4 v = P[i];
        for (int s = 1; s < k_splits; ++s) {
            const float4 p = P[s * n4 + i];
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        C[i] = v;
    }
}
