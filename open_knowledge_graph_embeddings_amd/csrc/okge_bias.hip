// Chain rule of the data-bias scorers (DataBiasOnlyRelationScorer / DataBiasOnlyEntityScorer, openkge/model.py:281-350) behind
// the tile kernels (gfx950).  The query row of these scorers is ONE masked row, copied -- the relation's (bias_relation) or the
// prefix entity's (bias_entity) --, so
//   gradient of the used slot   = dQ * that slot's dropout mask
//   gradient of the other slot  = nothing: its row is STORED as zeros where rows are stored (distinct prefix rows, the
//                                 segmented path's row buffers: nobody clears those) and left alone where they are accumulated.
// Kernels of their own instead of branches in prefix_backward_kernel / prefix_backward_vec_kernel (okge_misc.hip): a third
// scorer branch there cost the existing kernels scalar-register spills and, at 8 slab loads in flight, scratch.  The dQ slabs
// are summed by the shared dq_quad_sum (okge_prefix_device.h) and the scalar kernel's loop is prefix_backward_kernel's, so a
// bias scorer agrees bit for bit with DistMult on an all-ones unused operand.
#include <algorithm>

#include "okge_device.h"
#include "okge_kernels.h"
#include "okge_eval_device.h"
#include "okge_prefix_device.h"

namespace okge {
namespace {

// any slot size: one workgroup per batch row, one column per thread and step (launch twin: prefix_backward_kernel)
__global__ __launch_bounds__(128) void bias_prefix_backward_kernel(int d, int scorer, const PrefixDev p, const float *__restrict__ slab,
                                                                   int nsplit, int Bpad, int ldq, int have_ent_rows,
                                                                   float *__restrict__ dE, float *__restrict__ dR, int distinct)
{
    const int b = blockIdx.x;
    const RowSrc rs = row_source(p, b);
    if (!have_ent_rows && !rs.owned) return;
    const bool use_e = scorer == SC_BIAS_ENTITY;
    const DropDev &du = use_e ? (rs.sp ? p.drop_sp_ent : p.drop_po_ent) : (rs.sp ? p.drop_sp_rel : p.drop_po_rel);
    float *ge = dE + (rs.owned ? rs.ent : 0) * d, *gr = dR + rs.rel * d;
    float *used = use_e ? ge : gr, *other = use_e ? gr : ge;
    const bool write_used = !use_e || rs.owned, zero_other = distinct && (use_e || rs.owned);
    const size_t split_stride = (size_t)Bpad * ldq;
    const float *sl = slab + (size_t)b * ldq;
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        float dq = 0.f;
        for (int sidx = 0; sidx < nsplit; ++sidx) dq += sl[sidx * split_stride + k];
        const float g = dq * drop_mult1(du, rs.pos, k, d);
        if (write_used) {
            if (distinct) used[k] = g;
            else atomicAdd(used + k, g);
        }
        if (zero_other) other[k] = 0.f;
    }
}

// d % 4 == 0: lane = (column group, split quarter) as in prefix_backward_vec_kernel; workgroup blockIdx.x == B_rows sums the
// loss partials, blockIdx.y is the 128-column chunk of the row
template <int NB>
__global__ __launch_bounds__(128) void bias_prefix_backward_vec_kernel(int d, int scorer, const PrefixDev p,
                                                                       const float *__restrict__ slab, int nsplit, int Bpad, int ldq,
                                                                       int have_ent_rows, float *__restrict__ dE, float *__restrict__ dR,
                                                                       const double *__restrict__ loss_partials, int n_partials,
                                                                       double *__restrict__ loss_out, float *__restrict__ dr_rows,
                                                                       float *__restrict__ de_rows, int distinct, int B_rows)
{
    if ((int)blockIdx.x >= B_rows) {
        if ((int)blockIdx.x == B_rows && blockIdx.y == 0 && loss_partials) loss_reduce_block(loss_partials, n_partials, loss_out);
        return;
    }
    const int b = blockIdx.x, grp = threadIdx.x >> 2, sq = threadIdx.x & 3;
    const RowSrc rs = row_source(p, b);
    if (!have_ent_rows && !rs.owned) return;
    const bool use_e = scorer == SC_BIAS_ENTITY;
    const DropDev &du = use_e ? (rs.sp ? p.drop_sp_ent : p.drop_po_ent) : (rs.sp ? p.drop_sp_rel : p.drop_po_rel);
    float *ge = de_rows ? de_rows + (size_t)b * ldq : dE + (rs.owned ? rs.ent : 0) * d;
    float *gr = dr_rows ? dr_rows + (size_t)b * ldq : dR + rs.rel * d;
    const bool store_e = de_rows || distinct, store_r = dr_rows || distinct;
    float *used = use_e ? ge : gr, *other = use_e ? gr : ge;
    const bool store_used = use_e ? store_e : store_r, write_used = !use_e || rs.owned;
    const bool zero_other = use_e ? store_r : (store_e && rs.owned);
    const size_t split_stride = (size_t)Bpad * ldq;
    const float *sl = slab + (size_t)b * ldq;
    const int s_lo = (nsplit * sq) >> 2, s_hi = (nsplit * (sq + 1)) >> 2;
    for (int k0 = 128 * blockIdx.y; k0 < d; k0 += 128 * gridDim.y) {
        const int k = k0 + 4 * grp;
        const bool act = k < d, lead = act && sq == 0;
        // the keep nibble of the chain-rule lane's four columns, requested before the slab sums
        uint32_t nib = 15u;
        if (du.enabled && lead) nib = (drop_keep8(du, rs.pos, k >> 3, d) >> (k & 4)) & 15u;
        const float4 dq = dq_quad_sum<NB>(sl, split_stride, s_lo, s_hi, act ? k : 0, act);
        if (!lead) continue;
        float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
        if (du.enabled) apply_keep4(m, nib, du.scale);
        const float4 g = f4mul(dq, m);
        if (write_used) {
            if (store_used) *reinterpret_cast<float4 *>(used + k) = g;
            else atomic_add4(used + k, g);
        }
        if (zero_other) *reinterpret_cast<float4 *>(other + k) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

}  // namespace

hipError_t launch_bias_prefix_rows(int d, int scorer, const PrefixDev &p, const float *slab,
                                   int nsplit, int Bpad, int ldq, const float *ent_rows, float *dE, float *dR,
                                   const double *loss_partials, int n_partials, double *loss_out, float *dr_rows, float *de_rows,
                                   int distinct, hipStream_t st)
{
    const int B = p.n_po + p.n_sp;
    if (B <= 0) return hipSuccess;
    if (!sc_is_bias(scorer)) return hipErrorInvalidValue;
    const int have_ent_rows = ent_rows != nullptr;
    if (d % 4 == 0) {
        const int chunks = std::min(8, (d + 127) / 128);
        if (nsplit >= 8)
            hipLaunchKernelGGL(bias_prefix_backward_vec_kernel<8>, dim3(B + 1, chunks), dim3(128), 0, st, d, scorer, p, slab, nsplit, Bpad,
                               ldq, have_ent_rows, dE, dR, loss_partials, n_partials, loss_out, dr_rows, de_rows, distinct, B);
        else
            hipLaunchKernelGGL(bias_prefix_backward_vec_kernel<1>, dim3(B + 1, chunks), dim3(128), 0, st, d, scorer, p, slab, nsplit, Bpad,
                               ldq, have_ent_rows, dE, dR, loss_partials, n_partials, loss_out, dr_rows, de_rows, distinct, B);
    } else {
        if (dr_rows || de_rows) return hipErrorInvalidValue;      // (row buffers are float4 rows)
        hipLaunchKernelGGL(bias_prefix_backward_kernel, dim3(B), dim3(128), 0, st, d, scorer, p, slab, nsplit, Bpad, ldq, have_ent_rows,
                           dE, dR, distinct);
    }
    return hipGetLastError();
}

}  // namespace okge
