// The train tile's gradient phase dC[16 candidates][16 KB columns] += G^T[16][32 rows] . Q[32 rows][16 KB] of one wave and one
// 64-row chunk, on the bf16 matrix cores from three bf16 planes per operand (arithmetic: csrc/okge_dq_split.h) -- the form
// fused_tile64_kernel (okge_train64.hip) runs at the instances tile_grad_split() names, in place of eight fp32 sub-steps.  In a
// header so that tools/ubench/mfma_bf16_split.hip, part (c), times exactly the loop the kernel runs; results:
// profiles/tile_grad_split.md.
//
// A operand.  After the loss epilogue lane (c, s) of wave (blk, h) holds g4[rg][i] = G[row 32h + 16rg + 4s + i][candidate 16blk + c]:
// 8 batch rows of one candidate, which IS an A operand of v_mfma_f32_16x16x32_bf16 with k = 4rg + i in k-group s.  The
// contraction index may be permuted freely as long as both operands use the same permutation, so G needs no transpose and no LDS:
// one split3 of 8 floats per lane and chunk.
//
// B operand: the query planes of a chunk, made once per step outside the tile kernel, in the image the phase reads:
// [half h][plane hi|mid|lo][k-group s][slot 0 .. 16 KB - 1] cells of 8 bf16; element 4rg + i of cell (h, s, slot) is batch row
// 32h + 16rg + 4s + i -- the row set lane (., s) holds in g4.  Lane (c, s) reads slot 16 kb + c of row s with one ds_read_b128
// per plane and block; a cell row is a multiple of 256 B, so a ds_read_b128 lane group (which mixes two s) covers 16 distinct
// 16-byte bank slots: conflict-free.  Slot 16 kb + c holds the column the tile's accumulator dc[kb] holds in lane c
// (query_plane_slot).  A chunk is one contiguous block of CHUNK_CELLS cells, so staging is a flat copy: PIECES pieces of 1 KiB,
// one global_load_lds_dwordx4 each, dealt to the eight waves.
//
// The planes are a pure function of the fp32 query block: whoever produces that block (encode_queries_kernel in the step, the
// caller of okge_train_tiles otherwise) has write_query_row_planes run over every row of the padded batch, so rows past B and
// columns past d are zero planes on every call -- G is not zero on padding rows, and a stale cell there would reach dE.
#pragma once
#include "okge_dq_split.h"

namespace okge {

// slot of query column k in a cell row: dc[kb] of lane c is column 64 (kb / 4) + 4 c + kb % 4 up to the last whole group of
// four blocks and column 16 kb + c behind it (the fp32 loop's ds_read_b128 order, which the write-back is written for)
__host__ __device__ constexpr int query_plane_slot(int k, int KB) { return k < 64 * (KB / 4) ? 16 * (4 * (k >> 6) + (k & 3)) + ((k & 63) >> 2) : k; }

// Batch row b of the padded batch, fp32 folded query row q (nullptr: a zero row; columns past d count as zero) -> its 2-byte
// element of every cell of its k-group.  All threads of the workgroup take part; rows share cells, never bytes.
__device__ __forceinline__ void write_query_row_planes(const float *q, int d, int KB, int b, __bf16 *planes)
{
    const int D16 = 16 * KB, r = b & 63, h = r >> 5, s = (r >> 2) & 3, e = 4 * ((r >> 4) & 1) + (r & 3);
    __bf16 *dst = planes + ((size_t)(b >> 6) * (24 * D16) + (size_t)(12 * h + s) * D16) * 8 + e;
    for (int k = threadIdx.x; k < D16; k += blockDim.x) {
        const Split1 p = split1((q && k < d) ? q[k] : 0.f);
        __bf16 *cell = dst + 8 * query_plane_slot(k, KB);
        cell[0] = p.hi;
        cell[32 * D16] = p.mid;
        cell[64 * D16] = p.lo;
    }
}

template <int KB>
struct TileGradSplit {
    static constexpr int D16 = 16 * KB;
    static constexpr int PLANE_CELLS = 4 * D16;               // [s][slot]
    static constexpr int HALF_CELLS = 3 * PLANE_CELLS;
    static constexpr int CHUNK_CELLS = 2 * HALF_CELLS;
    static constexpr int PIECES = CHUNK_CELLS / 64;           // 1 KiB each
    static_assert(CHUNK_CELLS % 64 == 0, "whole 1 KiB pieces");

    __device__ static Planes a_planes(const v4f (&g4)[2])
    {
        const float x[8] = {g4[0][0], g4[0][1], g4[0][2], g4[0][3], g4[1][0], g4[1][1], g4[1][2], g4[1][3]};
        return split3(x);
    }

    // wave w's pieces of one chunk, global -> LDS; the caller waits for vmcnt(0) (a barrier does) before anybody reads them
    __device__ static void copy_chunk(const v8bf *src, v8bf *dst, int w, int lane)
    {
        typedef __attribute__((address_space(1))) const void *gptr;
        typedef __attribute__((address_space(3))) void *lptr;
#pragma unroll
        for (int p = 0; p < (PIECES + 7) / 8; ++p) {
            const int piece = 8 * p + w;
            if (piece < PIECES)
                __builtin_amdgcn_global_load_lds((gptr)(src + 64 * piece + lane), (lptr)(dst + 64 * piece), 16, 0, 0);
        }
    }

    // FOLD: the five corrections of a block are chained from zero and meet the main sum by one fp32 add per chunk (no registers
    // of their own beyond the block in flight); otherwise they have an accumulator of their own, corr[KB], added once by the caller
    template <bool FOLD>
    __device__ static void product(v4f (&dc)[KB], v4f (&corr)[FOLD ? 1 : KB], const Planes &a, const v8bf *chunk, int h, int lane)
    {
        const int c = lane & 15, s = lane >> 4;
        const v8bf *bi = chunk + h * HALF_CELLS + s * D16 + c;
        Planes b;
        b.hi = bi[0]; b.mid = bi[PLANE_CELLS]; b.lo = bi[2 * PLANE_CELLS];
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            Planes nb = b;
            if (kb + 1 < KB) {                                // the reads stay one block ahead of their MFMAs
                nb.hi = bi[16 * (kb + 1)]; nb.mid = bi[16 * (kb + 1) + PLANE_CELLS]; nb.lo = bi[16 * (kb + 1) + 2 * PLANE_CELLS];
            }
            v4f t = FOLD ? (v4f){0.f, 0.f, 0.f, 0.f} : corr[FOLD ? 0 : kb];
            t = mfma_bf16(a.lo, b.hi, t);                     // smallest first, as DqSplit::product
            t = mfma_bf16(a.hi, b.lo, t);
            t = mfma_bf16(a.mid, b.mid, t);
            t = mfma_bf16(a.mid, b.hi, t);
            t = mfma_bf16(a.hi, b.mid, t);
            dc[kb] = mfma_bf16(a.hi, b.hi, dc[kb]);
            if (FOLD) dc[kb] += t;
            else corr[FOLD ? 0 : kb] = t;
            b = nb;
            if (kb + 1 < KB) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
        }
    }
};

}  // namespace okge
