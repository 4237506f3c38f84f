// The dense Adam sweep (gfx950) and the prologue both Adam entry points share; the element update itself is okge_adam_device.h's.
//   adam_prologue_kernel   one workgroup: t += 1 per tensor, and c1 / c2 / the sparse step size of that t, formed in double
//   adam2_kernel           one or two tensors per launch over ONE dense sweep (+ zero_grad)      torch.optim.Adam / _single_tensor_adam
// The step count lives on the device (as counters[0] = T of okge_adagrad_lazy does): a captured HIP graph replays the
// increment with the sweep, nothing is read back, and the launches are fixed by the n alone.
#include <algorithm>
#include <cstring>

#include "okge_kernels.h"
#include "okge_adam_device.h"

namespace okge {

// lane k owns tensor k (a state two tensors share advances once: the launcher hands it over once)
__global__ __launch_bounds__(64) void adam_prologue_kernel(const AdamStates st, float lr, float beta1, float beta2)
{
    const int k = threadIdx.x;
    if (k >= st.n) return;
    int32_t *s = st.state[k];
    const int t = s[ADAM_T] + 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    s[ADAM_T] = t;
    s[ADAM_C1] = __float_as_int((float)((double)lr / bc1));
    s[ADAM_C2] = __float_as_int((float)sqrt(bc2));
    s[ADAM_STEP] = __float_as_int((float)((double)lr * sqrt(bc2) / bc1));
}

// The shape of adagrad_sweep (okge_optim.hip): 16-byte accesses over n >> 2 quads in a grid-stride loop, the n & 3 tail element by
// element.  Every element moves every step -- m and v decay whatever the gradient is -- so the stores are unconditional: the
// store-only-what-changed trick of adagrad_commit4 does not carry over (only the gradient clear stays conditional on a gradient
// that is not clear already, which leaves the same bits).
template <bool WD>
__device__ __forceinline__ void adam_sweep(const AdamSeg sg, const AdamHyper h, bool zero_grad, int64_t first, int64_t stride)
{
    if (sg.n <= 0) return;
    const float c1 = __int_as_float(sg.state[ADAM_C1]), c2 = __int_as_float(sg.state[ADAM_C2]);
    const int64_t n4 = sg.n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(sg.p), *g4 = reinterpret_cast<float4 *>(sg.g);
    float4 *m4 = reinterpret_cast<float4 *>(sg.m), *v4 = reinterpret_cast<float4 *>(sg.v);
    for (int64_t i = first; i < n4; i += stride) {
        float4 pv = p4[i], gv = g4[i], mv = m4[i], vv = v4[i];
        adam4<WD>(pv, gv, mv, vv, c1, c2, h);
        p4[i] = pv;
        m4[i] = mv;
        v4[i] = vv;
        if (zero_grad && ((__float_as_uint(gv.x) | __float_as_uint(gv.y) | __float_as_uint(gv.z) | __float_as_uint(gv.w)) != 0u))
            g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (first < (sg.n & 3)) {
        const int64_t i = (n4 << 2) + first;
        adam1<WD>(sg.p[i], sg.g[i], sg.m[i], sg.v[i], c1, c2, h);
        if (zero_grad) sg.g[i] = 0.f;
    }
}

__global__ __launch_bounds__(256) void adam2_kernel(const AdamSeg a, const AdamSeg b, const AdamHyper h, int zero_grad)
{
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    // zero_grad: 0 none, 1 both, 2 second tensor only
    if (h.wd != 0.f) {
        adam_sweep<true>(a, h, zero_grad == 1, first, stride);
        adam_sweep<true>(b, h, zero_grad != 0, first, stride);
    } else {
        adam_sweep<false>(a, h, zero_grad == 1, first, stride);
        adam_sweep<false>(b, h, zero_grad != 0, first, stride);
    }
}

hipError_t launch_adam_prologue(int32_t *const *states, int n_states, float lr, float beta1, float beta2, hipStream_t st)
{
    AdamStates a;
    std::memset(&a, 0, sizeof(a));
    for (int k = 0; k < n_states && a.n < ADAM_MAX_SEGS; ++k) {
        bool seen = false;
        for (int j = 0; j < a.n; ++j) seen = seen || a.state[j] == states[k];
        if (!seen) a.state[a.n++] = states[k];
    }
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_prologue_kernel, dim3(1), dim3(64), 0, st, a, lr, beta1, beta2);
    return hipGetLastError();
}

// the grid cap of the Adagrad launchers: 16384 workgroups of 256 threads, one float4 per thread and pass
hipError_t launch_adam2(const AdamSeg &a, const AdamSeg &b, float beta1, float beta2, float eps, float wd, int zero_grad, hipStream_t st)
{
    const int64_t n4 = (std::max(a.n, b.n) + 3) / 4;
    if (n4 <= 0) return hipSuccess;
    const int blocks = (int)std::min((int64_t)16384, (n4 + 255) / 256);
    hipLaunchKernelGGL(adam2_kernel, dim3(blocks), dim3(256), 0, st, a, b, adam_hyper(beta1, beta2, eps, wd), zero_grad);
    return hipGetLastError();
}

}  // namespace okge
