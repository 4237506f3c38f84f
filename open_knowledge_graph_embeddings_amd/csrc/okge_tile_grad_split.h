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
// [half h][plane hi|mid|lo][k-group s][position 0 .. 16 KB - 1] cells of 8 bf16; cell (h, s, slot) holds the batch rows
// 32h + 16rg + 4s + i -- the row set lane (., s) holds in g4 -- of one column.  Lane (c, s) reads slot 16 kb + c of row s with
// one ds_read_b128 per plane and block; a cell row is a multiple of 256 B, so a ds_read_b128 lane group (which mixes two s of
// one pair 2 (s / 2), 2 (s / 2) + 1) covers 16 distinct 16-byte bank slots: conflict-free.  Slot 16 kb + c holds the column the
// tile's accumulator dc[kb] holds in lane c (query_plane_slot).  A chunk is one contiguous block of CHUNK_CELLS cells, so staging
// is a flat copy: PIECES pieces of 1 KiB, one global_load_lds_dwordx4 each, dealt to the eight waves.
//
// Two swizzles, both a function of the cell row s alone, make the SAME image serve the score phase's transposed reads
// (TileScoreSplit below) without bank conflicts.  (1) Slot `slot` of row s sits at position slot ^ 8 (s / 2)
// (query_plane_pos): rows 0, 1 and rows 2, 3 of a column are 128 B apart in bank space -- every cell row starts on bank 0,
// so without it the four rows of a column share their banks.  The gradient phase reads position (16 kb + c) ^ 8 (s / 2): the
// same 16 cells per lane group.  (2) Batch row 32h + 16rg + 4s + i is element 4 (rg ^ (s & 1)) + i of its cell
// (query_plane_elem): odd rows carry their two 8-byte halves swapped, so the 32 lanes of a transposed read -- which all want
// the same rg -- use both halves of the 16 cells they touch.  The gradient phase's contraction index is permuted within a
// k-group, which is free as long as the A operand follows: a_planes swaps g4[0] and g4[1] on odd s.
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

// where slot `slot` of cell row s sits in the row, and which element of its cell batch row 32h + 16rg + 4s + i is
__host__ __device__ constexpr int query_plane_pos(int slot, int s) { return slot ^ ((s >> 1) << 3); }
__host__ __device__ constexpr int query_plane_elem(int rg, int i, int s) { return 4 * (rg ^ (s & 1)) + i; }

// Batch row b of the padded batch, fp32 folded query row q (nullptr: a zero row; columns past d count as zero) -> its 2-byte
// element of every cell of its k-group.  All threads of the workgroup take part; rows share cells, never bytes.
__device__ __forceinline__ void write_query_row_planes(const float *q, int d, int KB, int b, __bf16 *planes)
{
    const int D16 = 16 * KB, r = b & 63, h = r >> 5, s = (r >> 2) & 3, e = query_plane_elem((r >> 4) & 1, r & 3, s);
    __bf16 *dst = planes + ((size_t)(b >> 6) * (24 * D16) + (size_t)(12 * h + s) * D16) * 8 + e;
    for (int k = threadIdx.x; k < D16; k += blockDim.x) {
        const Split1 p = split1((q && k < d) ? q[k] : 0.f);
        __bf16 *cell = dst + 8 * query_plane_pos(query_plane_slot(k, KB), s);
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

    // lane (., s): element query_plane_elem(rg, i, s) is g4[rg][i]
    __device__ static Planes a_planes(const v4f (&g4)[2], int s)
    {
        const v4f lo = (s & 1) ? g4[1] : g4[0], hi = (s & 1) ? g4[0] : g4[1];
        const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return split3(x);
    }

    // wave w's pieces of one chunk (rounds P0 .. P1 - 1 of the (PIECES + 7) / 8 in which the pieces are dealt to the eight waves),
    // global -> LDS; the caller waits for vmcnt(0) (a barrier does) before anybody reads them
    template <int P0 = 0, int P1 = (PIECES + 7) / 8>
    __device__ static void copy_chunk(const v8bf *src, v8bf *dst, int w, int lane)
    {
        typedef __attribute__((address_space(1))) const void *gptr;
        typedef __attribute__((address_space(3))) void *lptr;
#pragma unroll
        for (int p = P0; p < P1; ++p) {
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
        const v8bf *bi = chunk + h * HALF_CELLS + s * D16 + query_plane_pos(c, s);
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

// The train tile's score phase X[16 rows][16 candidates] = Q[rows][columns] . C[candidates][columns]^T of one wave (blk, h) and
// one 64-row chunk -- the two blocks rg = 0, 1 of rows 32h + 16rg .. + 15 against the candidates 16blk .. + 15 -- from the SAME
// plane image, in place of 4 KB v_mfma_f32_16x16x4_f32 per block on an fp32 copy of the chunk.  The contraction runs over
// columns, the image holds batch rows along a cell: the A operand is read transposed, with ds_read_b64_tr_b16.
//
// Steps.  t = 0 .. KB/2 - 1: one v_mfma_f32_16x16x32_bf16 per plane product over the 32 columns 32t .. 32t + 31; odd KB: one
// v_mfma_f32_16x16x16_bf16 over the last 16.  Six products per step and block in two chains, as DqSplit::product: hi.hi into x,
// the five corrections smallest first into a chain of their own that runs through all steps and meets x once, at the end.
//
// Contraction order (both operands follow col()): element e = 4j + q of k-group g (lanes 16g .. 16g + 15) is column
//   32t + 16 (g & 1) + 4q + 2 (g >> 1) + j   of a K = 32 step,      32 (KB/2) + 8 (g >> 1) + 4 (g & 1) + q   of the K = 16 step.
//
// A operand.  One ds_read_b64_tr_b16 takes, per 16-lane group, four 8-byte pieces for each of four columns and hands lane i the
// 16-bit element i of the four columns.  Lane 4q + p of group g addresses, for read j of step t, the half rg of cell (h, p,
// slot of column col(t, g, 4j + q)): bytes 8 (rg ^ (p & 1)) .. + 7 of the cell at position query_plane_pos(slot, p) of cell row p
// -- the batch rows 32h + 16rg + 4p .. + 3 of that column.  Lane i = 4 (i / 4) + i % 4 of the group then holds batch row
// 32h + 16rg + i at columns col(t, g, 4j + 0 .. 3): two reads make the 8 elements of the K = 32 operand, one the 4 of K = 16.
// Banks ((byte / 4) % 64, counted per 32-lane half = two groups g, g + 1 of one g >> 1): the slot of col() has
// (slot & 7) = 4 (g & 1) + q and (slot & 8) the same in all lanes of the half, so with position = slot ^ 8 (p >> 1) and the
// half 8 (rg ^ (p & 1)) the 32 lanes take 32 different 8-byte bank pairs: conflict-free (enumerated over every read of a chunk
// in tests/test_tile_score_split.py; on the unswizzled image every read is 4-way).  All addresses are multiples of 8.
// EXEC must be all ones at the reads: score() is called by whole waves only.
//
// B operand: the lane's candidate row 16blk + c, split once per tile into three planes in the order above and kept in
// registers: 12 (KB/2) + 6 VGPRs.
template <int KB>
struct TileScoreSplit {
    using T = TileGradSplit<KB>;
    static constexpr int STEPS = KB / 2;
    static constexpr bool TAIL = KB & 1;
    // (instantiable at any KB, so that a kernel template can name BOp; load_b and score are for the KB below)
    static constexpr bool FITS = 32 * STEPS == 64 * (KB / 4) && TAIL;    // whole steps cover the permuted slots, the K = 16 step the last block
    typedef short v4s __attribute__((ext_vector_type(4)));

    __host__ __device__ static constexpr int col(int t, int g, int e)
    {
        return t < STEPS ? 32 * t + 16 * (g & 1) + 4 * (e & 3) + 2 * (g >> 1) + (e >> 2) : 32 * STEPS + 8 * (g >> 1) + 4 * (g & 1) + (e & 3);
    }

    struct BOp { Planes b[STEPS]; v4s thi, tmid, tlo; };

    // crow: the lane's masked candidate row (fp32, 16 KB columns, zeros past d), g = lane >> 4
    __device__ static void load_b(BOp &o, const float *crow, int g)
    {
        static_assert(FITS, "KB = 13");
        const float *base = crow + 16 * (g & 1) + 2 * (g >> 1);
#pragma unroll
        for (int t = 0; t < STEPS; ++t) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = base[32 * t + 4 * (e & 3) + (e >> 2)];
            o.b[t] = split3(x);
        }
        const v4f tl = *reinterpret_cast<const v4f *>(crow + 32 * STEPS + 8 * (g >> 1) + 4 * (g & 1));
        typedef __bf16 v4bf __attribute__((ext_vector_type(4)));
        v4bf hi, mid, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const Split1 v = split1(tl[e]);
            hi[e] = v.hi; mid[e] = v.mid; lo[e] = v.lo;
        }
        o.thi = __builtin_bit_cast(v4s, hi); o.tmid = __builtin_bit_cast(v4s, mid); o.tlo = __builtin_bit_cast(v4s, lo);
    }

    // byte offset in the chunk image of the piece lane `lane` addresses: step t (STEPS: the K = 16 step), read j, plane pl, block rg
    __host__ __device__ static constexpr int a_offset(int h, int lane, int t, int j, int pl, int rg)
    {
        const int p = lane & 3, q = (lane >> 2) & 3, g = lane >> 4;
        return 16 * (h * T::HALF_CELLS + pl * T::PLANE_CELLS + p * T::D16 + query_plane_pos(query_plane_slot(col(t, g, 4 * j + q), KB), p)) +
               8 * (rg ^ (p & 1));
    }

    __device__ static v4s read_tr(const char *p)
    {
        typedef __attribute__((address_space(3))) v4s *lptr;
        return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)p);
    }

    // x[rg] = the score block of rows 32h + 16rg + 4s + i (element i of lane (c, s)), candidates 16blk + c
    __device__ static void score(v4f (&x)[2], const BOp &o, const v8bf *chunk, int h, int lane)
    {
        static_assert(FITS, "KB = 13");
        const char *img = reinterpret_cast<const char *>(chunk);
        // what of a_offset depends on the lane: four bases for the whole steps (t & 1, rg), two for the K = 16 step; the rest
        // (t >> 1, j, plane) is the same in all lanes and goes into the reads' offset fields
        const char *base[2][2], *tbase[2];
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) {
            base[0][rg] = img + a_offset(h, lane, 0, 0, 0, rg);
            base[1][rg] = img + a_offset(h, lane, 1, 0, 0, rg) - 16 * query_plane_slot(32, KB);
            tbase[rg] = img + a_offset(h, lane, STEPS, 0, 0, rg);
        }
        auto load = [&](int t, Planes (&a)[2]) {
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) {
                const char *p = base[t & 1][rg] + 16 * query_plane_slot(32 * t, KB);
                v4s r[3][2];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                    for (int j = 0; j < 2; ++j) r[pl][j] = read_tr(p + 16 * (pl * T::PLANE_CELLS + 16 * j));
                a[rg].hi = __builtin_bit_cast(v8bf, __builtin_shufflevector(r[0][0], r[0][1], 0, 1, 2, 3, 4, 5, 6, 7));
                a[rg].mid = __builtin_bit_cast(v8bf, __builtin_shufflevector(r[1][0], r[1][1], 0, 1, 2, 3, 4, 5, 6, 7));
                a[rg].lo = __builtin_bit_cast(v8bf, __builtin_shufflevector(r[2][0], r[2][1], 0, 1, 2, 3, 4, 5, 6, 7));
            }
        };
        v4f tc[2];
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) x[rg] = tc[rg] = (v4f){0.f, 0.f, 0.f, 0.f};
        Planes a[2];
        load(0, a);
        __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
#pragma unroll
        for (int t = 0; t < STEPS; ++t) {
            Planes na[2] = {a[0], a[1]};
            v4s ta[2][3];
            if (t + 1 < STEPS) {                              // the reads stay one step ahead of their MFMAs
                load(t + 1, na);
            } else {
#pragma unroll
                for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) ta[rg][pl] = read_tr(tbase[rg] + 16 * pl * T::PLANE_CELLS);
            }
            const Planes &b = o.b[t];
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) tc[rg] = mfma_bf16(a[rg].lo, b.hi, tc[rg]);     // smallest first, as DqSplit::product
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) tc[rg] = mfma_bf16(a[rg].hi, b.lo, tc[rg]);
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) tc[rg] = mfma_bf16(a[rg].mid, b.mid, tc[rg]);
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) tc[rg] = mfma_bf16(a[rg].mid, b.hi, tc[rg]);
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) tc[rg] = mfma_bf16(a[rg].hi, b.mid, tc[rg]);
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) x[rg] = mfma_bf16(a[rg].hi, b.hi, x[rg]);
            if (t + 1 < STEPS) __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
            else __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
            if (t + 1 < STEPS) {
                a[0] = na[0]; a[1] = na[1];
            } else {
#pragma unroll
                for (int rg = 0; rg < 2; ++rg) {
                    v4f c5 = tc[rg];
                    c5 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ta[rg][2], o.thi, c5, 0, 0, 0);
                    c5 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ta[rg][0], o.tlo, c5, 0, 0, 0);
                    c5 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ta[rg][1], o.tmid, c5, 0, 0, 0);
                    c5 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ta[rg][1], o.thi, c5, 0, 0, 0);
                    c5 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ta[rg][0], o.tmid, c5, 0, 0, 0);
                    tc[rg] = c5;
                    x[rg] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ta[rg][0], o.thi, x[rg], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) x[rg] += tc[rg];
    }
};

}  // namespace okge
