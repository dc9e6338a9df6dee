// attn_decode.hip — single-token (decode) attention over a contiguous bf16
// KV cache for MI355X (gfx950), head dimension D = 128.
//
//   s_i = scale * q . k_i  (i < seq_lens[b]),  p = softmax(s),
//   o   = sum_i p_i v_i,   lse = ln sum_i exp(s_i)
//
// for q [B][Hq][D], one slab of keys and values per (sequence, kv head),
// ragged seq_lens[B] (1 <= len <= Lmax) and grouped-query heads: query head
// h reads kv head h / G, G = Hq / Hkv <= 16. Operands are bf16, all
// accumulation is f32, o [B][Hq][D] and lse [B][Hq] are f32.
//
// The shape is memory-bound: every K and V byte is used once by one wave,
// so both go straight from global memory into VGPRs with 16-B loads (no LDS
// staging), and the next 32 positions' loads are issued before the current
// 32 positions' MFMAs, as gemm_mxfp4_decode.hip does for W.
//
// Both products run on v_mfma_f32_16x16x32_bf16, in the orientation that
// keeps P on its lane:
//
//   * S^T = K . Q^T. A = 16 key rows (lane l: position p0 + l%16, d =
//     32*ks + 8*(l/16) .. +7, one 16-B load of the row-major K slab),
//     B = the G query rows of the kv head as one 16-column fragment,
//     zero-padded. The result has query l%16 on the lane and positions
//     p0 + 4*(l/16) + r in registers r = 0..3.
//   * O^T = V^T . P^T. Two 16-position tiles give a lane the 8 bf16 values
//     of one 32-deep k-step of P^T as the B operand, with no lane movement.
//     The k order inside the step is therefore permuted: lane group
//     g = l/16, element j is position 4g + j of tile 0 for j < 4 and
//     4g + j - 4 of tile 1 for j >= 4. V^T (A operand, rows = 16 values of
//     d) must present the same order, 8 positions contiguous per lane.
//
// Device-side layouts:
//
//   K   [B][Hkv][Lmax][128] bf16, row-major (the public layout).
//   VP  [B][Hkv][ceil(Lmax/32)][128][32] bf16, PRIVATE: per block of 32
//       positions and per d, the 32 positions in MFMA k order, i.e.
//       position p of the block sits at index
//           8 * ((p % 16) / 4) + 4 * (p / 16) + p % 4.
//       One wave-instruction then reads 1 KiB contiguous (16 d x 64 B).
//       Positions past Lmax in the last block are padding. The host repacks
//       the public [Lmax][128] slab (attn_pack_v in loadgen_lib.cpp).
//
// No address is formed from a position >= seq_lens[b]: a K row index is
// clamped to len - 1, and a V block is only touched if its first position
// is < len. In the block that straddles the end the clamped positions'
// scores are SELECTED to -inf (p is exactly 0) and their V elements are
// masked to +0 before the product, since stale cache slots may hold NaN and
// 0 * NaN is NaN.
//
// Work split, no float atomics, results bit-identical from run to run:
//
//   * CTA = (sequence, kv head, KV split), 256 threads. Split bounds are
//     multiples of 32 positions and the same for every sequence; a short
//     sequence leaves later splits empty.
//   * The four waves take contiguous quarters of the split's 32-position
//     blocks (clipped to len); each keeps running (m, l, acc) with
//     online-softmax rescaling in the exp2 domain (scale * log2(e) is
//     folded into the score). l stays a per-lane partial sum until the end:
//     the lanes of one query share m, so only the max crosses lanes per
//     block (xor 16, xor 32).
//   * The waves leave (m, l, acc) in LDS and merge in wave order. An empty
//     wave has m = -inf, l = 0: its weight is exp2(m - M') with M' = M, or 0
//     if M itself is -inf, so -inf - (-inf) is never evaluated.
//   * kv_splits > 1: the CTA writes its merged, unnormalised (m, l, acc) to
//     a workspace and attn_decode_merge combines the splits in split order
//     by the same rule.

#include "gemm_tile.h"

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16v2;

#define ATTN_NEG_INF (-__builtin_inff())
#define ATTN_LN2 0.69314718055994530942f
// A weight below 2^-60 of the running maximum's is set to exactly 0: a
// probability, and the rescale factor of what a wave has accumulated.
// Fewer than 2^31 positions can be dropped this way, together less than
// 2^-29 of the leading weight: below f32 resolution in o and in l. It keeps
// such addends out of the P.V MFMA, which does not round them to nearest:
// with them, an exactly representable o = 64 came back as 64 - 2^-18
// (profiles/attn_decode.md).
#define ATTN_P_FLUSH_LOG2 (-60.f)

// two f32 -> packed bf16 (round to nearest even), a in the low half
static __device__ __forceinline__ int pack_bf16(float a, float b)
{
    const f32x2 f = {a, b};
    return __builtin_bit_cast(int, __builtin_convertvector(f, bf16v2));
}

// Operands of one block of 32 positions for one wave.
struct AttnBlock {
    bf16x8 k[2][4];  // two 16-position tiles x four 32-deep d steps
    i32x4 v[8];      // eight 16-row d fragments of V^T, 32 positions deep
};

extern "C" __global__ void __launch_bounds__(256) attn_decode_bf16(
    const unsigned short* __restrict__ Q,   // [B][Hq][128]
    const unsigned short* __restrict__ K,   // [B][Hkv][Lmax][128]
    const unsigned short* __restrict__ VP,  // [B][Hkv][ceil(Lmax/32)][128][32]
    const int* __restrict__ seq_lens,       // [B]
    float* __restrict__ O,                  // [B][Hq][128]
    float* __restrict__ LSE,                // [B][Hq]
    float* __restrict__ ws_acc,             // [splits][B][Hq][128]
    float* __restrict__ ws_m,               // [splits][B][Hq]
    float* __restrict__ ws_l,               // [splits][B][Hq]
    int B, int Hq, int Hkv, int Lmax,
    int blocks_per_split, int splits, float scale_log2e)
{
    __shared__ f32x4 red[4][8][64];
    __shared__ float red_m[4][64];
    __shared__ float red_l[4][64];

    const int tid = threadIdx.x;
    // wave-uniform in an SGPR: the block-range tests are scalar branches
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int r16 = lane & 15;
    const int g = lane >> 4;
    const int G = Hq / Hkv;

    int id = blockIdx.x;
    const int split = id % splits;
    id /= splits;
    const int h = id % Hkv;
    const int b = id / Hkv;

    const int len = seq_lens[b];
    // this CTA's 32-position blocks, clipped to the sequence, and this
    // wave's contiguous quarter of them
    const int blk0 = split * blocks_per_split;
    int blk1 = blk0 + blocks_per_split;
    const int seq_blocks = (len + 31) >> 5;
    if (blk1 > seq_blocks) blk1 = seq_blocks;
    const int nb = blk1 > blk0 ? blk1 - blk0 : 0;
    const int bb = blk0 + (nb * w) / 4;
    const int be = blk0 + (nb * (w + 1)) / 4;

    const long slab = (long)b * Hkv + h;
    const unsigned short* kp = K + slab * Lmax * 128 + g * 8;
    const unsigned short* vp =
        VP + slab * ((Lmax + 31) >> 5) * 4096 + r16 * 32 + g * 8;

    // B operand of S^T: query column r16 of this kv head, zero past G
    bf16x8 qf[4];
    {
        const int qi = r16 < G ? r16 : G - 1;
        const unsigned short* qp =
            Q + ((long)b * Hq + h * G + qi) * 128 + g * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = *(const bf16x8*)(qp + ks * 32);
            if (r16 >= G) qf[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
    }

    // Loads block blk (its first position is < len). A key row past the
    // end is clamped onto len - 1: in bounds, its score is not used.
    auto load_block = [&](AttnBlock& t, int blk) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            int pos = blk * 32 + tt * 16 + r16;
            pos = pos < len ? pos : len - 1;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                t.k[tt][ks] =
                    *(const bf16x8*)(kp + (long)pos * 128 + ks * 32);
        }
#pragma unroll
        for (int db = 0; db < 8; ++db)
            t.v[db] = *(const i32x4*)(vp + (long)blk * 4096 + db * 512);
    };

    float m = ATTN_NEG_INF;  // running max of the lane's query (log2 domain)
    float l = 0.f;           // the lane's partial sum of p
    f32x4 acc[8];            // O^T: d = 16*db + 4*g + r, query r16
#pragma unroll
    for (int db = 0; db < 8; ++db) acc[db] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // full: all 32 positions of the block are < len.
    auto compute_block = [&](const AttnBlock& t, int blk, bool full) {
        f32x4 s[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            s[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    t.k[tt][ks], qf[ks], s[tt], 0, 0, 0);
        }
        // element j of the P fragment: tile j/4, register j%4
        float x[8];
        const int pos0 = blk * 32 + g * 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j] = s[j >> 2][j & 3] * scale_log2e;
            if (!full && pos0 + (j >> 2) * 16 + (j & 3) >= len)
                x[j] = ATTN_NEG_INF;
        }
        float mx = x[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) mx = fmaxf(mx, x[j]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        // the block's first position is valid, so mx and m_new are finite
        const float m_new = fmaxf(m, mx);
        // the same flush for what the wave has accumulated so far: it
        // enters the P.V MFMA as the C operand
        const float dm = m - m_new;
        const float alpha =
            dm < ATTN_P_FLUSH_LOG2 ? 0.f : __builtin_amdgcn_exp2f(dm);
        m = m_new;
        float p[8], ps = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float dx = x[j] - m_new;
            p[j] = dx < ATTN_P_FLUSH_LOG2 ? 0.f : __builtin_amdgcn_exp2f(dx);
            ps += p[j];
        }
        l = l * alpha + ps;
        const i32x4 pw = {pack_bf16(p[0], p[1]), pack_bf16(p[2], p[3]),
                          pack_bf16(p[4], p[5]), pack_bf16(p[6], p[7])};
        const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
        // V elements of positions >= len go to +0 (dword wd holds elements
        // 2*wd and 2*wd + 1)
        i32x4 keep = {-1, -1, -1, -1};
        if (!full) {
#pragma unroll
            for (int wd = 0; wd < 4; ++wd) {
                const int pa = pos0 + (wd >> 1) * 16 + (wd & 1) * 2;
                keep[wd] = (pa < len ? 0xffff : 0) |
                           (pa + 1 < len ? (int)0xffff0000 : 0);
            }
        }
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            const i32x4 vv = full ? t.v[db] : (t.v[db] & keep);
            acc[db] *= alpha;
            acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8, vv), pf, acc[db], 0, 0, 0);
        }
    };

    if (bb < be) {
        AttnBlock t0, t1;
        int i = bb;
        load_block(t0, i);
        // Steady state has no branch around a load, so the compiler's
        // counted vmcnt leaves the whole next block in flight behind the
        // current block's MFMAs. Only a wave's last block can straddle the
        // end of the sequence.
        while (i + 2 < be) {  // blocks i, i+1, i+2 exist
            load_block(t1, i + 1);
            compute_block(t0, i, true);
            load_block(t0, i + 2);
            compute_block(t1, i + 1, true);
            i += 2;
        }
        // one or two blocks left, t0 holds i
        if (i + 1 < be) {
            load_block(t1, i + 1);
            compute_block(t0, i, true);
            compute_block(t1, i + 1, false);
        } else {
            compute_block(t0, i, false);
        }
    }

    // the lane groups of one query hold disjoint positions
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);

    // in-CTA merge, wave order
#pragma unroll
    for (int db = 0; db < 8; ++db) red[w][db][lane] = acc[db];
    red_m[w][lane] = m;
    red_l[w][lane] = l;
    __syncthreads();

    float M = ATTN_NEG_INF;
#pragma unroll
    for (int i = 0; i < 4; ++i) M = fmaxf(M, red_m[i][lane]);
    const float Mf = M == ATTN_NEG_INF ? 0.f : M;  // finite
    float wgt[4], L = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        wgt[i] = __builtin_amdgcn_exp2f(red_m[i][lane] - Mf);
        L += wgt[i] * red_l[i][lane];
    }
    // wave w finishes d fragments 2w and 2w + 1
    const int hq = h * G + r16;
    const long row = (long)b * Hq + hq;
    const long prow = (long)split * B * Hq + row;
#pragma unroll
    for (int dd = 0; dd < 2; ++dd) {
        const int db = 2 * w + dd;
        f32x4 a = wgt[0] * red[0][db][lane];
        a += wgt[1] * red[1][db][lane];
        a += wgt[2] * red[2][db][lane];
        a += wgt[3] * red[3][db][lane];
        if (r16 < G) {
            const int d = db * 16 + g * 4;
            if (splits == 1)
                *(f32x4*)(O + row * 128 + d) = a / L;
            else
                *(f32x4*)(ws_acc + prow * 128 + d) = a;
        }
    }
    if (w == 0 && g == 0 && r16 < G) {
        if (splits == 1) {
            LSE[row] = (M + log2f(L)) * ATTN_LN2;
        } else {
            ws_m[prow] = M;
            ws_l[prow] = L;
        }
    }
}

// Second pass for kv_splits > 1: one CTA per (sequence, query head), thread
// = d. Combines the splits' (m, l, acc) in split order; split 0 is never
// empty, so M is finite and L > 0.
extern "C" __global__ void __launch_bounds__(128) attn_decode_merge(
    const float* __restrict__ ws_acc, const float* __restrict__ ws_m,
    const float* __restrict__ ws_l, float* __restrict__ O,
    float* __restrict__ LSE, int splits)
{
    const long row = blockIdx.x, rows = gridDim.x;
    const int d = threadIdx.x;
    float M = ATTN_NEG_INF;
    for (int s = 0; s < splits; ++s) M = fmaxf(M, ws_m[s * rows + row]);
    const float Mf = M == ATTN_NEG_INF ? 0.f : M;
    float L = 0.f, a = 0.f;
    for (int s = 0; s < splits; ++s) {
        const float wgt = __builtin_amdgcn_exp2f(ws_m[s * rows + row] - Mf);
        L += wgt * ws_l[s * rows + row];
        a += wgt * ws_acc[(s * rows + row) * 128 + d];
    }
    O[row * 128 + d] = a / L;
    if (d == 0) LSE[row] = (M + log2f(L)) * ATTN_LN2;
}
