// The Adam element update (torch.optim.Adam with amsgrad = False, maximize = False and coupled L2 weight decay:
// _single_tensor_adam's non-capturable branch; the optimizer OptimRegime is born with, utils/optim.py:29, and the one a config's
// `optimizer: Adam` selects, utils/optim.py:143-145), stated once for every kernel that applies it:
//     g' = g + wd * p                              (ABSENT at wd == 0, not multiplied by zero: see adagrad1_rows' note on
//                                                   fmaf(0, p, g) in okge_adagrad_device.h)
//     m += (g' - m) * (1 - beta1)                  (exp_avg.lerp_)
//     v  = v * beta2 + (1 - beta2) * g' * g'       (exp_avg_sq.mul_().addcmul_())
//     p -= c1 * (m / (sqrt(v) / c2 + eps))         c1 = lr / (1 - beta1^t),  c2 = sqrt(1 - beta2^t)
// and the row-sparse one (torch.optim._functional.sparse_adam on a coalesced row; no weight-decay term):
//     m += (g - m) * (1 - beta1);  v += (g * g - v) * (1 - beta2);  p -= step * (m / (sqrt(v) + eps))
//     step = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
// At most one rounding per written operation (where the compiler contracts a multiply into the subtraction that follows, one
// rounding fewer: tests/adam_reference.py's caps hold either way); correctly rounded sqrtf and division.  c1, c2 and step depend
// on the step count t alone: adam_prologue_kernel forms them in double once per call and leaves them, rounded to fp32 once, in
// the tensor's device state.
#pragma once
#include "okge_device.h"

namespace okge {

// device state of one Adam tensor: int32[4] = { t (steps taken), bits of c1, bits of c2, bits of the sparse step size }
constexpr int ADAM_T = 0, ADAM_C1 = 1, ADAM_C2 = 2, ADAM_STEP = 3;

// what does not depend on t, formed on the host once per call: 1 - beta in double from the fp32 beta, rounded to fp32 once
struct AdamHyper { float omb1, beta2, omb2, eps, wd; };
inline AdamHyper adam_hyper(float beta1, float beta2, float eps, float wd)
{
    return AdamHyper{(float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2), eps, wd};
}

__device__ __forceinline__ void adam_moments1(float gj, float &m, float &v, const AdamHyper &h)
{
    m = fmaf(gj - m, h.omb1, m);
    v = fmaf(v, h.beta2, (h.omb2 * gj) * gj);
}

template <bool WD>
__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, float c1, float c2, const AdamHyper &h)
{
    const float gj = WD ? fmaf(h.wd, p, g) : g;
    adam_moments1(gj, m, v, h);
    p = p - c1 * (m / (sqrtf(v) / c2 + h.eps));
}

template <bool WD>
__device__ __forceinline__ void adam4(float4 &pv, const float4 &gv, float4 &mv, float4 &vv, float c1, float c2, const AdamHyper &h)
{
    float *pp = &pv.x, *mm = &mv.x, *vs = &vv.x;
    const float *gg = &gv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) adam1<WD>(pp[j], gg[j], mm[j], vs[j], c1, c2, h);
}

__device__ __forceinline__ void adam1_rows(float &p, float g, float &m, float &v, float step, const AdamHyper &h)
{
    m = fmaf(g - m, h.omb1, m);
    v = fmaf(g * g - v, h.omb2, v);
    p = p - step * (m / (sqrtf(v) + h.eps));
}

}  // namespace okge
