// Device code shared by the chain-rule kernels behind the tile kernels (prefix_backward_vec_kernel in okge_misc.hip, the
// data-bias scorers' kernels in okge_bias.hip): float4 arithmetic and THE order in which the dQ slabs are summed -- every
// kernel that turns the dQ slabs into prefix gradients sums them through dq_quad_sum, so they agree bit for bit.
#pragma once
#include "okge_device.h"

namespace okge {

__device__ __forceinline__ float4 f4mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 f4fma(float4 a, float4 b, float4 c)
{
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 f4neg(float4 a) { return make_float4(-a.x, -a.y, -a.z, -a.w); }
__device__ __forceinline__ void atomic_add4(float *p, float4 v)
{
    atomicAdd(p, v.x); atomicAdd(p + 1, v.y); atomicAdd(p + 2, v.z); atomicAdd(p + 3, v.w);
}

// Component sq of the float4 that the lead lane (sq == 0) of a 4-lane column group holds; every lane of the group must call it.
// The group then adds p[sq] += component, one column per lane, so that the 64 lanes of a wave whose groups stand on consecutive
// column quads add 64 consecutive floats: one 256-byte global_atomic_add_f32 in place of four with 16 lanes, 16 bytes apart,
// each (float atomics execute at the memory side one 64-byte request at a time: four full requests, not sixteen quarter-filled).
__device__ __forceinline__ float quad_lead_component(float4 v, int sq)
{
    const float x = dpp_mov<0x00>(v.x), y = dpp_mov<0x00>(v.y), z = dpp_mov<0x00>(v.z), w = dpp_mov<0x00>(v.w);
    return sq == 0 ? x : sq == 1 ? y : sq == 2 ? z : w;
}

// deterministic sum of the per-workgroup loss partials by ONE workgroup (the order depends on its size)
__device__ __forceinline__ void loss_reduce_block(const double *__restrict__ partials, int n, double *__restrict__ out)
{
    __shared__ double red[4];
    const int nw = blockDim.x >> 6;
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) v += partials[i];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < nw; ++i) t += red[i];
        out[0] = t;
    }
}

// Columns k .. k+3 of one batch row's dQ, summed over the split-K slabs by the four lanes of a column group: lane sq adds the
// slabs s_lo .. s_hi-1 of its quarter (NB loads in flight at a time), then the quarters are combined.  Every lane of the quad
// must call it (inactive ones contribute zeros); all four return the sum.
template <int NB>
__device__ __forceinline__ float4 dq_quad_sum(const float *__restrict__ sl, size_t split_stride, int s_lo, int s_hi, int k, bool active)
{
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        int sidx = s_lo;
        if (NB > 1)
            for (; sidx + NB <= s_hi; sidx += NB) {
                float4 v[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) v[u] = *reinterpret_cast<const float4 *>(sl + (sidx + u) * split_stride + k);
#pragma unroll
                for (int u = 0; u < NB; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
            }
        for (; sidx < s_hi; ++sidx) {
            const float4 v = *reinterpret_cast<const float4 *>(sl + sidx * split_stride + k);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    // the four lanes of a column group are a DPP quad: xor 1, xor 2 as quad permutes (a ds_bpermute shuffle each
    // would cost ~60 cycles on this latency-bound path)
    acc.x += dpp_mov<0xB1>(acc.x); acc.y += dpp_mov<0xB1>(acc.y); acc.z += dpp_mov<0xB1>(acc.z); acc.w += dpp_mov<0xB1>(acc.w);
    acc.x += dpp_mov<0x4E>(acc.x); acc.y += dpp_mov<0x4E>(acc.y); acc.z += dpp_mov<0x4E>(acc.z); acc.w += dpp_mov<0x4E>(acc.w);
    return acc;
}

}  // namespace okge
