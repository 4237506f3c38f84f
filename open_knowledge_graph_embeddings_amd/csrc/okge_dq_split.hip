// dq8s_kernel<KB>: dQ = G . C for slot sizes up to 208 (KB = 4, 8, 13), fp32 emulated on the bf16 matrix cores from three
// bf16 planes per operand (arithmetic, LDS image and wave roles: okge_dq_split.h; measurements: profiles/dq_split_ablation.md).
// Same contract as the fp32-MFMA kernel it replaced (dq8_kernel, retired): DqArgs, (Bpad / 64) x nsplit workgroups of 512
// threads, workgroup = 64 batch rows x a contiguous run of 64-candidate chunks -> one [64][16 KB] slab block, written or (with
// `accumulate`) added to; no atomics, fixed summation order, so two runs give identical bits.
//
// Loop: 32-candidate sub-chunks (two per chunk), two LDS buffers, ONE barrier per sub-chunk: sub-chunk i + 1 -- the candidate
// planes as the tile kernel wrote them, G^T split here -- is parked in the second buffer while sub-chunk i is being multiplied.  Two register sets per staging thread keep the
// loads of sub-chunks i + 2 and i + 3 in flight (a sub-chunk is multiplied in well under a load latency).  Of a SIMD's two
// waves the one with w < 4 parks before its MFMAs and the other one after: they take turns at the matrix core.
#include "okge_dq_split.h"
#include "okge_kernels.h"

namespace okge {

template <int KB>
__global__ __launch_bounds__(512, 2) void dq8s_kernel(const DqArgs a)
{
    using S = DqSplit<KB>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v8bf *lds = reinterpret_cast<v8bf *>(smem);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int h = w >> 2, blk0 = S::wave_blk0(h, w & 3), nblk = S::wave_nblk(h, w & 3);
    const int split = blockIdx.x % a.nsplit, bblk = blockIdx.x / a.nsplit;
    const int nJ = a.Bpad / BC;
    const int nchunks = (a.N + NT - 1) / NT;
    const int sc_lo = 2 * (int)((int64_t)split * nchunks / a.nsplit);          // whole 64-candidate chunks, as sub-chunks
    const int sc_hi = 2 * (int)((int64_t)(split + 1) * nchunks / a.nsplit);

    v4f acc[2][S::NBW], corr[2][S::NBW];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int nb = 0; nb < S::NBW; ++nb) acc[r][nb] = corr[r][nb] = (v4f){0.f, 0.f, 0.f, 0.f};

    typename S::Stage st[2];                          // sub-chunk sc_lo + i travels in set i & 1 and is parked in buffer i & 1
    auto step = [&](int sc, int buf, typename S::Stage &nxt) {
        __syncthreads();                              // sub-chunk sc is parked; the other buffer's readers (sc - 1) are done
        const bool more = sc + 1 < sc_hi;
        if (w < 4 && more) {
            S::park(nxt, lds + (buf ^ 1) * S::BUF_CELLS, tid);
            if (sc + 3 < sc_hi) S::prefetch(nxt, a.G, a.Cplanes, sc + 3, bblk, nJ, tid);
        }
        S::product(acc, corr, lds + buf * S::BUF_CELLS, h, blk0, nblk, lane);
        if (w >= 4 && more) {
            S::park(nxt, lds + (buf ^ 1) * S::BUF_CELLS, tid);
            if (sc + 3 < sc_hi) S::prefetch(nxt, a.G, a.Cplanes, sc + 3, bblk, nJ, tid);
        }
    };
    if (sc_lo < sc_hi) {                              // (sc_hi - sc_lo is even)
        S::prefetch(st[0], a.G, a.Cplanes, sc_lo, bblk, nJ, tid);
        S::prefetch(st[1], a.G, a.Cplanes, sc_lo + 1, bblk, nJ, tid);
        S::park(st[0], lds, tid);
        if (sc_lo + 2 < sc_hi) S::prefetch(st[0], a.G, a.Cplanes, sc_lo + 2, bblk, nJ, tid);
    }
    for (int sc = sc_lo; sc < sc_hi; sc += 2) {
        step(sc, 0, st[1]);
        step(sc + 1, 1, st[0]);
    }
    __syncthreads();                                  // the buffers are free: they take the fp32 output image [64][LDO]

    // acc + corrections -> natural (row, column) through LDS -> coalesced slab rows
    float *out = reinterpret_cast<float *>(smem);
    const int c = lane & 15, s = lane >> 4;
#pragma unroll
    for (int nb = 0; nb < S::NBW; ++nb) {
        if (nb < nblk) {
            const int col = S::slot_to_col(16 * (blk0 + nb) + c);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i)           // G slot 32 h + 16 r + 4 s + i holds batch row 4 (4 s + i) + 2 h + r
                    out[(4 * (4 * s + i) + 2 * h + r) * S::LDO + col] = acc[r][nb][i] + corr[r][nb][i];
        }
    }
    __syncthreads();
    for (int f = tid; f < 64 * S::NQ; f += 512) {
        const int row = f / S::NQ, q = f % S::NQ;
        float *dst = a.slab + ((size_t)split * a.Bpad + bblk * BC + row) * a.ldq + 4 * q;
        v4f v = *reinterpret_cast<const v4f *>(out + row * S::LDO + 4 * q);
        if (a.accumulate) v += *reinterpret_cast<const v4f *>(dst);
        *reinterpret_cast<v4f *>(dst) = v;
    }
}

template <int KB>
static hipError_t launch_dq8s_t(const DqArgs &a, int grid_x, hipStream_t st)
{
    return launch_with_lds<dq8s_kernel<KB>>(dim3(grid_x), dim3(512), DqSplit<KB>::LDS_BYTES, st, a);
}

hipError_t launch_dq8s(const DqArgs &a, int grid_x, hipStream_t st)
{
    switch (a.KB) {
        case 4:  return launch_dq8s_t<4>(a, grid_x, st);
        case 8:  return launch_dq8s_t<8>(a, grid_x, st);
        case 13: return launch_dq8s_t<13>(a, grid_x, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace okge
