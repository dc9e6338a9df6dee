// gemm_mxfp4_256.hip — 256x256-tile MXFP4 (E2M1 + E8M0 block scale) MFMA
// GEMM for MI355X (gfx950).
//
// CDNA4's block-scaled fp4 dense peak is 4x bf16 (~10 PF/s). The matrix
// core takes it through v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz:4
// blgp:4: K=128 per instruction, 16 operand bytes (32 E2M1 nibbles) per
// lane in 4 VGPRs, and one E8M0 scale byte per lane and operand. Lane l
// holds row l&15, k 32*(l>>4)..+31 of the 128-wide step; its scale byte
// applies to exactly that (row, 32-block), which is the OCP MX block.
//
// Schedule and LDS machinery are the fp8 kernel's (gemm_fp8_256.hip):
// 256x256 CTA tile, 512 threads as a 2x4 wave grid, one barrier per K-tile,
// global_load_lds width 16 into 16-KiB half-tile images with 128-B rows,
// XCD remap and 4x4 super-tile raster. A 128-B row is now 256 fp4
// elements, so a K-tile covers K=256 = two MFMA k-steps, and a fragment is
// ONE ds_read_b128 per k-step at row*128 + step*64 + (lane>>4)*16.
//
// LDS swizzle: ds_read_b128 is served in four 16-lane groups, each holding
// 16 distinct fragment rows and two adjacent 16-B k-chunks (c, c^1). A
// 256-B bank row is two image rows, so the 16-B slot of (row, chunk) is
// (row&1)*8 + chunk. XOR-ing the chunk with (row>>1)&7 spreads each group
// over all 16 slots: conflict-free. As always with global_load_lds the
// LDS image stays lane-linear and the XOR moves to the source address.
//
// Scales: the host pre-shuffles them (mxfp4::shuffle_scales) so that one
// dword per lane carries the scale bytes of four 16-row fragments for one
// k-step; the instruction's byte select (op_sel 0..3) picks the fragment
// with no VALU work. Per wave and K-tile that is 4 dwords for A and 2 for
// B, loaded one K-tile ahead into registers and retired by the same
// boundary vmcnt(0) as the tile DMAs.
//
// C[M][N] f32 = dq(A)[M][K] @ dq(Bt)[N][K]^T; M,N % 256 == 0, K % 256 == 0.
// A, Bt: [rows][K/2] bytes, element 2i in the low nibble.

#include "gemm_tile.h"

#define F4_HALF_BYTES 16384   // [128][256] fp4 image, 128-B rows

extern "C" __global__ void __launch_bounds__(512, 2) gemm_mxfp4_tn_256(
    const unsigned char* __restrict__ A,   // [M][K/2] packed E2M1
    const unsigned char* __restrict__ Bt,  // [N][K/2] packed E2M1
    const int* __restrict__ SA,            // [M/64][K/128][64] shuffled E8M0
    const int* __restrict__ SB,            // [N/64][K/128][64] shuffled E8M0
    float* __restrict__ C,                 // [M][N] f32
    int M, int N, int K, int tiles_per_cta)
{
    __shared__ unsigned char lds[8 * F4_HALF_BYTES];

    const int tid = threadIdx.x;
    const int w = tid >> 6;
    const int lane = tid & 63;
    const int wr = w >> 2;  // 0..1: A half this wave consumes
    const int wc = w & 3;   // 0..3: B cols wc*64..+64

    const int n_tiles_n = N / 256;
    const int n_tiles_m = M / 256;
    const int n_tiles = n_tiles_m * n_tiles_n;
    const int KB = K >> 1;       // operand bytes per row
    const int kTiles = K / 256;
    const int kSteps = K / 128;  // scale dwords per lane and 64-row group

    const int nwg = gridDim.x;
    const int wgid = xcd_remap(blockIdx.x, nwg);

    // glds source mapping: piece p = w*2+it fills image bytes
    // p*1024 + lane*16 (rows p*8..p*8+7); the lane fetches the 16 B that
    // the swizzle places there.
    long src_off[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int logical = swz_f4((w * 2 + it) * 1024 + lane * 16);
        src_off[it] = (long)(logical >> 7) * KB + (logical & 127);
    }

    // fragment read byte offset: one 16-B k-chunk per lane group (lane>>4)
    auto frag_off = [&](int row_in_half, int step) {
        return swz_f4(row_in_half * 128 + step * 64 + (lane >> 4) * 16);
    };

    const bool super4 = (n_tiles_n % 4 == 0) && (n_tiles_m % 4 == 0);

    for (int t = 0; t < tiles_per_cta; ++t) {
        const int tile = wgid + t * nwg;
        if (tile >= n_tiles) return;
        int tm, tn;
        tile_coords(tile, n_tiles_n, super4, tm, tn);
        const long row0 = (long)tm * 256;
        const long col0 = (long)tn * 256;

        // zeroing and the final store are written out: zero_acc() and
        // store_acc() here change the generated code
        // (profiles/loadgen_refactor.md)
        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

        // slot layout: [buf][A0 A1 B0 B1] x2
        auto stage = [&](int kt, int h, int buf) {
            if (kt >= kTiles) kt = kTiles - 1;  // tail clamp (benign restage)
            const unsigned char* src =
                ((h < 2) ? A + (row0 + h * 128) * (long)KB
                         : Bt + (col0 + (h - 2) * 128) * (long)KB) +
                (long)kt * 128;
            unsigned char* dst = &lds[(buf * 4 + h) * F4_HALF_BYTES];
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int p = w * 2 + it;
                glds16(src + src_off[it], dst + p * 1024);
            }
        };

        // this wave's scale dwords: A rows row0+wr*128.. are 64-row groups
        // ga, ga+1 (fragments 0-3, 4-7); B cols col0+wc*64.. are group gb.
        const int* sa_ptr =
            SA + ((row0 + wr * 128) >> 6) * (long)kSteps * 64 + lane;
        const int* sb_ptr =
            SB + ((col0 + wc * 64) >> 6) * (long)kSteps * 64 + lane;
        // index [step*2 + group] for A, [step] for B
        auto load_scales = [&](int kt, int* sa, int* sb) {
            if (kt >= kTiles) kt = kTiles - 1;  // tail clamp (unused values)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const long ks = (long)(kt * 2 + s) * 64;
                sa[s * 2 + 0] = sa_ptr[ks];
                sa[s * 2 + 1] = sa_ptr[(long)kSteps * 64 + ks];
                sb[s] = sb_ptr[ks];
            }
        };

        // The compiler cannot see the hand-written vmcnt(0) below, so it
        // would wait for the scale registers at their first MFMA, behind
        // the next tile's freshly issued DMAs, and drain the pipeline
        // there. Touching them right after the boundary wait moves its
        // own wait to that (already satisfied) point.
        auto retire_scales = [](int* sa, int* sb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(sa[i]));
            asm volatile("" : "+v"(sb[0]));
            asm volatile("" : "+v"(sb[1]));
        };

        int sa_cur[4], sb_cur[2], sa_nxt[4], sb_nxt[2];

        stage(0, 0, 0);
        stage(0, 1, 0);
        stage(0, 2, 0);
        stage(0, 3, 0);
        load_scales(0, sa_cur, sb_cur);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        retire_scales(sa_cur, sb_cur);
        __builtin_amdgcn_s_barrier();

        i32x8 afrag[2];
        i32x8 bfrag[4];

        // fp4 operands live in elements 0..3 only (4 VGPRs)
        auto read_frag = [&](const unsigned char* base, int row_in_half,
                             int step) {
            i32x4 lo = *(const i32x4*)(base + frag_off(row_in_half, step));
            i32x8 r = {lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
            return r;
        };

        for (int kt = 0; kt < kTiles; ++kt) {
            const int buf = kt & 1;
            const unsigned char* la = &lds[(buf * 4 + wr) * F4_HALF_BYTES];
            const unsigned char* lb =
                &lds[(buf * 4 + 2 + (wc >> 1)) * F4_HALF_BYTES];
            const int bcol0 = (wc & 1) * 64;

#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int mbase = q * 2;
#pragma unroll
                    for (int m = 0; m < 2; ++m)
                        afrag[m] = read_frag(
                            la, (mbase + m) * 16 + (lane & 15), s);
                    if (q == 0) {
#pragma unroll
                        for (int n = 0; n < 4; ++n)
                            bfrag[n] = read_frag(
                                lb, bcol0 + n * 16 + (lane & 15), s);
                    }

                    // next tile's DMAs and scales: every slot of buf^1 is
                    // dead since the previous boundary barrier
                    if (s == 0) {
                        if (q == 0) {
                            load_scales(kt + 1, sa_nxt, sb_nxt);
                            stage(kt + 1, 0, buf ^ 1);
                            stage(kt + 1, 1, buf ^ 1);
                        } else if (q == 1) {
                            stage(kt + 1, 2, buf ^ 1);
                        } else if (q == 2) {
                            stage(kt + 1, 3, buf ^ 1);
                        }
                    }

                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int n = 0; n < 4; ++n)
                            // fragment mbase+m = group (q>>1), byte
                            // (q&1)*2+m of the A scale dword; n-fragment n
                            // = byte n of the B scale dword
                            acc[mbase + m][n] = mfma_mxfp4(
                                afrag[m], bfrag[n], acc[mbase + m][n],
                                (q & 1) * 2 + m, sa_cur[s * 2 + (q >> 1)],
                                n, sb_cur[s]);
                    __builtin_amdgcn_s_setprio(0);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            retire_scales(sa_nxt, sb_nxt);
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int i = 0; i < 4; ++i) sa_cur[i] = sa_nxt[i];
            sb_cur[0] = sb_nxt[0];
            sb_cur[1] = sb_nxt[1];
        }

#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long row = row0 + wr * 128 + i * 16 + (lane >> 4) * 4 + r;
                    const long col = col0 + wc * 64 + j * 16 + (lane & 15);
                    C[row * (long)N + col] = acc[i][j][r];
                }
            }
        }
        __syncthreads();
    }
}
