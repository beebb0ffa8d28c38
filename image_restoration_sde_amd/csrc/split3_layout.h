// The three-piece operand layout of gemm_split3i_kernel (gemm_split.hip) and its writers (wino.hip, split_triples_kernel).
//
// An f32 matrix [rows][K] (K a multiple of 32) becomes three bf16 planes (round to nearest even, every residual exact in f32), interleaved per
// ROW PAIR and 32-k block:
//     [row / 2][k / 32][row % 2][plane 0..2][k % 32]            2 x 3 x 64 B = 384 bytes = three whole 128-byte lines per block
// so the 16 rows x 192 bytes a stage's LDS-DMA group fetches are 8 blocks of whole lines (a single row's 192 bytes would start on a half line every
// second row).  A component holds split3_rows(rows) rows (rows rounded up to even; the pad row of an odd matrix is never read: the kernel clamps
// its row index to rows - 1) = split3_comp_elems(rows, K) unsigned shorts, 6 bytes per f32 element.
// The kernel's load ring (profiles/split3_ring.md) cuts a K-step's stage by tile ROWS (24 KB units of 16-row groups), never inside a block: every LDS-DMA
// wave-load still fetches whole 384-byte blocks, so the ring needed no 16-k re-layout of the blocks and every writer stores what it stored before.
#pragma once
#include <cstddef>

namespace irsde {

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IRSDE_S3_HD __host__ __device__
#else
#define IRSDE_S3_HD
#endif

IRSDE_S3_HD inline size_t split3_rows(size_t rows) { return (rows + 1) & ~(size_t)1; }
IRSDE_S3_HD inline size_t split3_comp_elems(size_t rows, size_t K) { return split3_rows(rows) * K * 3; }
// index (in unsigned shorts, inside one component) of plane `p` of element (row, k); nkb = K / 32
IRSDE_S3_HD inline size_t split3_index(size_t row, size_t k, int p, size_t nkb) {
    return ((row >> 1) * nkb + (k >> 5)) * 192 + (row & 1) * 96 + (size_t)p * 32 + (k & 31);
}

#undef IRSDE_S3_HD

}  // namespace irsde
