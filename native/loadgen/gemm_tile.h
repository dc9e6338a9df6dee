// gemm_tile.h — tile machinery shared by the GEMM load kernels (gfx950).
//
// Helpers and typedefs only: no kernels, no __shared__. Everything is
// __forceinline__, and a kernel moves onto a helper only where that leaves
// its ISA unchanged: tools/kernel_isa_diff.py compares two source trees
// kernel by kernel. hipcc's schedule is sensitive to how the same
// arithmetic reaches it, so a few bodies keep a loop written out (the
// per-wave store in the AGPR/spilling schedules, the two-piece glds loop of
// the stage lambdas); profiles/loadgen_refactor.md lists them and why.

#pragma once

#include <hip/hip_runtime.h>

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(8))) unsigned short bf16x8;

// XCD-aware bijective remap of the block index: block b runs on XCD b % 8,
// so consecutive remapped ids land on one XCD and its L2 sees contiguous
// tiles. The q/r form handles grids that are no multiple of 8. This is the
// only copy of the formula in device code; tests/test_xcd_remap.py is its
// executable specification (bijectivity, per-XCD contiguity).
static __device__ __forceinline__ int xcd_remap(int wgid, int nwg)
{
    int q = nwg >> 3, r = nwg & 7;
    int xcd = wgid & 7, pos = wgid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// Tile index -> tile coordinates. super4: 4x4 super-tile rasterization — an
// XCD's consecutive tiles cover a 4x4 block of the tile grid, so 4 A-panels
// x 4 B-panels are re-read from L2/L3 instead of HBM (fetch ~4x lower per
// block); the caller enables it only where both tile counts divide by 4.
// Otherwise the linear row-major raster.
static __device__ __forceinline__ void tile_coords(int tile, int n_tiles_n,
                                                   bool super4, int& tm,
                                                   int& tn)
{
    if (super4) {
        const int sb = tile >> 4, wi = tile & 15;
        const int sbn = n_tiles_n >> 2;
        tm = (sb / sbn) * 4 + (wi >> 2);
        tn = (sb % sbn) * 4 + (wi & 3);
    } else {
        tm = tile / n_tiles_n;
        tn = tile % n_tiles_n;
    }
}

// 16 B per lane straight from global memory into LDS (no VGPR round trip):
// the wave's 64 lanes fill dst + lane*16, dst wave-uniform.
static __device__ __forceinline__ void glds16(const void* src, void* dst)
{
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)dst, 16, 0, 0);
}

// st_16x32 LDS swizzle on a byte offset within an operand image of 128-B
// rows (subtile = 1024 B = 8 rows): the bf16 and fp8 fragment reads take
// TWO adjacent 16-B chunks per lane group, and flipping bit 5 by bit 9
// spreads a 16-lane group from 8-way to 4-way on a bank pair. glds writes
// lane-linear, so the same XOR is applied to the per-lane global source.
static __device__ __forceinline__ int swz_st16x32(int byte_off)
{
    return byte_off ^ (((byte_off >> 9) & 1) << 5);
}

// MXFP4 swizzle. A different function on purpose: an fp4 fragment is ONE
// ds_read_b128 per k-step, served in 16-lane groups that hold 16 distinct
// rows and two adjacent chunks, so the 16-B chunk index is XOR-ed with
// (row >> 1) & 7 to spread a group over all 16 slots of a 256-B bank row
// (derivation: gemm_mxfp4_256.hip).
static __device__ __forceinline__ int swz_f4(int byte_off)
{
    return byte_off ^ (((byte_off >> 8) & 7) << 4);
}

template <int R, int S>
static __device__ __forceinline__ void zero_acc(f32x4 (&acc)[R][S])
{
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < S; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// Per-wave f32 store: wave (wr, wc) of the CTA's wave grid owns the R*16 x
// S*16 sub-tile (128x64 for acc[8][4]) of the C tile at (row0, col0), as
// R x S accumulator fragments of 16x16. Lane l, register r of a fragment
// holds row (l/16)*4 + r, col l%16 — coalesced by 16-lane row groups.
template <int R, int S>
static __device__ __forceinline__ void store_acc(float* C, int N, long row0,
                                                 long col0, int wr, int wc,
                                                 int lane,
                                                 const f32x4 (&acc)[R][S])
{
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int j = 0; j < S; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row =
                    row0 + wr * (R * 16) + i * 16 + (lane >> 4) * 4 + r;
                const long col = col0 + wc * (S * 16) + j * 16 + (lane & 15);
                C[row * (long)N + col] = acc[i][j][r];
            }
        }
    }
}

// Block-scaled fp4 MFMA (cbsz:4 blgp:4) with run-time-looking scale byte
// selects. The selects must be literal constants for the builtin; after
// unrolling, oa/ob are constants and the switch folds away.
#define GEMM_TILE_F4_MFMA(OA, OB)                                             \
    case (OA) * 4 + (OB):                                                     \
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(              \
            a, b, c, 4, 4, OA, sa, OB, sb)
static __device__ __forceinline__ f32x4 mfma_mxfp4(i32x8 a, i32x8 b, f32x4 c,
                                                   int oa, int sa, int ob,
                                                   int sb)
{
    switch (oa * 4 + ob) {
        GEMM_TILE_F4_MFMA(0, 0); GEMM_TILE_F4_MFMA(0, 1);
        GEMM_TILE_F4_MFMA(0, 2); GEMM_TILE_F4_MFMA(0, 3);
        GEMM_TILE_F4_MFMA(1, 0); GEMM_TILE_F4_MFMA(1, 1);
        GEMM_TILE_F4_MFMA(1, 2); GEMM_TILE_F4_MFMA(1, 3);
        GEMM_TILE_F4_MFMA(2, 0); GEMM_TILE_F4_MFMA(2, 1);
        GEMM_TILE_F4_MFMA(2, 2); GEMM_TILE_F4_MFMA(2, 3);
        GEMM_TILE_F4_MFMA(3, 0); GEMM_TILE_F4_MFMA(3, 1);
        GEMM_TILE_F4_MFMA(3, 2);
        default:
            return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                a, b, c, 4, 4, 3, sa, 3, sb);
    }
}
#undef GEMM_TILE_F4_MFMA
