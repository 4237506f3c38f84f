// The N3 regulariser of the lookup models as the reference spells it (`l2_reg`, model.py:444-453, :471-479): every _encode call
// in training mode adds  c * sum |x|^3  over the rows it returns, x = the row AFTER its dropouts, and the Trainer
// backpropagates (loss + hook) / normalizer (trainer.py:217-221).  With x = m s e (m the keep flag, s the mask scale, e the
// stored element):
//     value       c * sum |x|^3                                (double, one partial per workgroup, fixed order)
//     d / d e     3 c x |x| m s / normalizer                   (fp32; zero at x == 0, never NaN)
// Kernel of okge_n3_forward_backward:
//   n3_kernel   workgroups [0, cand_wgs): candidate rows -- read through cand_table_row, masked with the bits the tile kernels
//               draw (drop_keep8 keyed by candidate position, column / 8, stream, step; or the explicit keep mask), value and
//               gradient multiplied by the number of passes the reference encodes the block in;
//               workgroups [cand_wgs, ..): the B prefix entity rows, then the B prefix relation rows, each with its own
//               stream's mask by row position.
//               The gradient is ADDED: plain read-modify-write where one lane owns the element (a candidate range, a list the
//               caller vouches for, distinct prefix rows, occurrence rows), float atomics where an id may repeat.  A prefix
//               entity is usually a candidate too: where the candidate rows are read-modify-written and the prefix rows added
//               atomically the two parts run as two launches, so that the plain update never meets an atomic one.
// Memory-bound and elementwise: one item = one 8-column octet of a row (the unit of a mask draw), two float4 accesses when
// d % 4 == 0, single floats otherwise.  The work a workgroup takes and the order it sums in depend on (B, N, d) alone
// (plan_n3), so the value is bit-reproducible.
#include <hip/hip_runtime.h>

#include "okge_kernels.h"
#include "okge_plan.h"
#include "okge_tile.h"

// Every product is rounded before it is added (hipcc contracts a * b + c into one fma by default, __fmul_rn included): the
// read-modify-write paths must add the very fp32 number the atomic paths hand to the memory system, or a row-sparse step and
// a dense step of the same batch would part in the last bit.
#pragma clang fp contract(off)

namespace okge {

namespace {

// one element: x = keep ? e s : 0; returns the gradient term x |x| ks and adds |x|^3 to acc
__device__ __forceinline__ float n3_elem(float e, bool keep, float s, float ks, double &acc)
{
    const float x = keep ? __fmul_rn(e, s) : 0.f;
    const float ax = fabsf(x);
    const double a = (double)ax;
    acc += a * a * a;
    return __fmul_rn(__fmul_rn(x, ax), ks);
}

template <bool ATOMIC>
__device__ __forceinline__ void n3_add(float *p, float g)
{
    if (ATOMIC) {
        if (g != 0.f) atomicAdd(p, g);
    } else {
        *p += g;
    }
}

// the items of rows [r0, r1) of one part; row(r, src, dst, dr, pos) resolves a row
template <bool ATOMIC, class Row>
__device__ __forceinline__ double n3_rows(const N3Args &a, int r0, int r1, double kd, Row row)
{
    const int d = a.d, items = (r1 - r0) * a.n_oct;
    double acc = 0.0;
    for (int it = threadIdx.x; it < items; it += N3_THREADS) {
        const int rr = it / a.n_oct, o = it - rr * a.n_oct;
        const float *src;
        float *dst;
        const DropDev *dr;
        uint32_t pos;
        if (!row(r0 + rr, o == 0, src, dst, dr, pos)) continue;
        const int k0 = 8 * o;
        const float s = dr->scale, ks = (float)(kd * (double)s);
        if (a.vec) {
            // (d % 4 == 0: an octet is one or two whole float4; both are requested before the mask arithmetic)
            const bool two = k0 + 4 < d;
            const float4 e0 = *reinterpret_cast<const float4 *>(src + k0);
            const float4 e1 = two ? *reinterpret_cast<const float4 *>(src + k0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            const uint32_t bits = dr->enabled ? drop_keep8(*dr, pos, o, d, drop_step(*dr)) : 0xFFu;
            float4 g0, g1;
            g0.x = n3_elem(e0.x, bits & 1u, s, ks, acc);  g0.y = n3_elem(e0.y, bits & 2u, s, ks, acc);
            g0.z = n3_elem(e0.z, bits & 4u, s, ks, acc);  g0.w = n3_elem(e0.w, bits & 8u, s, ks, acc);
            g1.x = n3_elem(e1.x, bits & 16u, s, ks, acc); g1.y = n3_elem(e1.y, bits & 32u, s, ks, acc);
            g1.z = n3_elem(e1.z, bits & 64u, s, ks, acc); g1.w = n3_elem(e1.w, bits & 128u, s, ks, acc);
            if (a.loss_only) continue;
            if (ATOMIC) {
                n3_add<true>(dst + k0, g0.x); n3_add<true>(dst + k0 + 1, g0.y); n3_add<true>(dst + k0 + 2, g0.z); n3_add<true>(dst + k0 + 3, g0.w);
                if (two) { n3_add<true>(dst + k0 + 4, g1.x); n3_add<true>(dst + k0 + 5, g1.y); n3_add<true>(dst + k0 + 6, g1.z); n3_add<true>(dst + k0 + 7, g1.w); }
            } else {
                // (the gradient rows are requested here: requesting them beside the table rows, with the mask from the wide Philox,
                //  took 76 registers for 62 and 0.16 ms for 0.12 at the S-FB shape, d = 2048)
                float4 *p0 = reinterpret_cast<float4 *>(dst + k0);
                float4 t0 = *p0;
                t0.x += g0.x; t0.y += g0.y; t0.z += g0.z; t0.w += g0.w;
                *p0 = t0;
                if (two) {
                    float4 *p1 = reinterpret_cast<float4 *>(dst + k0 + 4);
                    float4 t1 = *p1;
                    t1.x += g1.x; t1.y += g1.y; t1.z += g1.z; t1.w += g1.w;
                    *p1 = t1;
                }
            }
        } else {
            const uint32_t bits = dr->enabled ? drop_keep8(*dr, pos, o, d, drop_step(*dr)) : 0xFFu;
            for (int e = 0; e < 8 && k0 + e < d; ++e) {
                const float g = n3_elem(src[k0 + e], (bits >> e) & 1u, s, ks, acc);
                if (!a.loss_only) n3_add<ATOMIC>(dst + k0 + e, g);
            }
        }
    }
    return acc;
}

template <bool ATOMIC>
__device__ __forceinline__ double n3_cand(const N3Args &a, int wg)
{
    const int r0 = wg * a.rows_per_wg, r1 = min(a.N, r0 + a.rows_per_wg);
    return n3_rows<ATOMIC>(a, r0, r1, a.grad_cand, [&](int n, bool lead, const float *&src, float *&dst, const DropDev *&dr, uint32_t &pos) {
        const int64_t cid = cand_table_row(a.cand_ids, a.cand_first, n, a.n_ent, lead ? a.p.id_err : nullptr);
        src = a.E + cid * a.d;
        dst = a.dE + (a.row_grads ? (int64_t)n : cid) * a.d;
        dr = &a.drop_c;
        pos = (uint32_t)n;
        return true;
    });
}

template <bool ATOMIC>
__device__ __forceinline__ double n3_prefix(const N3Args &a, int wg)
{
    const int B = a.p.n_po + a.p.n_sp;
    const int r0 = wg * a.rows_per_wg, r1 = min(2 * B, r0 + a.rows_per_wg);
    return n3_rows<ATOMIC>(a, r0, r1, a.grad_prefix, [&](int r, bool lead, const float *&src, float *&dst, const DropDev *&dr, uint32_t &pos) {
        const bool rel = r >= B;
        const int b = rel ? r - B : r;
        const bool sp = b >= a.p.n_po;
        const int i = sp ? b - a.p.n_po : b;
        int *err = lead ? a.p.id_err : nullptr;
        pos = (uint32_t)i;
        if (rel) {
            const int64_t id = checked_row(sp ? a.p.sp_rel[i] : a.p.po_rel[i], a.p.n_rel, err);
            src = a.R + id * a.d;
            dst = a.dR + (a.row_grads ? (int64_t)b : id) * a.d;
            dr = sp ? &a.p.drop_sp_rel : &a.p.drop_po_rel;
        } else {
            const int64_t id = checked_row(sp ? a.p.sp_subj[i] : a.p.po_obj[i], a.n_ent, err);
            src = a.E + id * a.d;
            dst = a.dE + (a.row_grads ? (int64_t)a.N + b : id) * a.d;
            dr = sp ? &a.p.drop_sp_ent : &a.p.drop_po_ent;
        }
        return true;
    });
}

__global__ __launch_bounds__(N3_THREADS) void n3_kernel(const N3Args a)
{
    __shared__ double red[N3_THREADS / WAVE];
    const int wg = a.wg0 + (int)blockIdx.x;
    const bool cand = wg < a.cand_wgs;
    double acc;
    if (cand) acc = a.cand_atomic ? n3_cand<true>(a, wg) : n3_cand<false>(a, wg);
    else acc = a.prefix_atomic ? n3_prefix<true>(a, wg - a.cand_wgs) : n3_prefix<false>(a, wg - a.cand_wgs);
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < N3_THREADS / WAVE; ++i) t += red[i];
        a.partial[wg] = t * (cand ? a.value_cand : a.value_prefix);
    }
}

}  // namespace

// workgroups [wg0, wg0 + n_wgs) of the call's cand_wgs + prefix_wgs
hipError_t launch_n3(const N3Args &a0, int wg0, int n_wgs, hipStream_t st)
{
    if (n_wgs <= 0) return hipSuccess;
    N3Args a = a0;
    a.wg0 = wg0;
    hipLaunchKernelGGL(n3_kernel, dim3(n_wgs), dim3(N3_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace okge
