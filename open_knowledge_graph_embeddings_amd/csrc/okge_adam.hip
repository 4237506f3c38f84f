// The dense Adam sweep (gfx950) and the prologue both Adam entry points share; the element update itself is okge_adam_device.h's.
//   adam_prologue_kernel   one workgroup: t += 1 per tensor, and c1 / c2 / the sparse step size of that t, formed in double
//   adam2_kernel           one or two tensors per launch over ONE dense sweep (+ zero_grad)      torch.optim.Adam / _single_tensor_adam
//   adam_multi_kernel      up to four tensors per launch, a tensor optionally with a touched-row byte map (okge_adam_multi)
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

// The sweep over a tensor with a touched-row byte map (the contract of adagrad_sweep's, okge_optim.hip): a row whose byte differs
// from the stamp holds an all-zero gradient, which is neither read nor cleared -- the row runs through adam4 with g = 0, the bits
// of the dense update on a zero gradient (m and v decay, p moves).  Rows are whole quads (row_len % 4 == 0), so there is no tail.
// U iterations side by side, for the reason given there: the map byte decides whether the gradient is loaded at all.
template <int U, bool WD>
__device__ __forceinline__ void adam_sweep_map(const AdamSegM sg, const AdamHyper h, int64_t first, int64_t stride)
{
    if (sg.n <= 0) return;
    const float c1 = __int_as_float(sg.state[ADAM_C1]), c2 = __int_as_float(sg.state[ADAM_C2]);
    const int64_t n4 = sg.n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(sg.p), *g4 = reinterpret_cast<float4 *>(sg.g);
    float4 *m4 = reinterpret_cast<float4 *>(sg.m), *v4 = reinterpret_cast<float4 *>(sg.v);
    const uint32_t row4 = (uint32_t)(sg.row_len >> 2);
    const int shift = (row4 & (row4 - 1)) == 0 ? 31 - __clz(row4) : -1;
    const uint8_t stamp = (uint8_t)sg.stamp;
    for (int64_t i0 = first; i0 < n4; i0 += U * stride) {
        bool ok[U], live[U];
        float4 pv[U], gv[U], mv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {                            // the U map bytes first, no branch between the loads
            const int64_t i = min(i0 + u * stride, n4 - 1);
            ok[u] = i0 + u * stride < n4;
            const int64_t row = shift >= 0 ? i >> shift : (i >> 32 ? i / row4 : (int64_t)((uint32_t)i / row4));
            live[u] = sg.touched[row] == stamp;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            live[u] = live[u] && ok[u];
            pv[u] = gv[u] = mv[u] = vv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok[u]) { pv[u] = p4[i]; mv[u] = m4[i]; vv[u] = v4[i]; }
            if (live[u]) gv[u] = g4[i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            const int64_t i = i0 + u * stride;
            const float4 g_in = gv[u];
            adam4<WD>(pv[u], g_in, mv[u], vv[u], c1, c2, h);
            p4[i] = pv[u];
            m4[i] = mv[u];
            v4[i] = vv[u];
            if (live[u] && ((__float_as_uint(g_in.x) | __float_as_uint(g_in.y) | __float_as_uint(g_in.z) | __float_as_uint(g_in.w)) != 0u))
                g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

struct AdamSegsDev { AdamSegM s[ADAM_MULTI_MAX_SEGS]; int n; };
// (four streams of 16 bytes per iteration against adagrad_sweep's three: the compiler's figures are 97 registers / 4 waves per SIMD
//  at two iterations side by side, 163 / 3 at four)
constexpr int ADAM_MAP_UNROLL = 2;

template <bool WD>
__device__ __forceinline__ void adam_multi_body(const AdamSegsDev &segs, const AdamHyper h, int64_t first, int64_t stride)
{
    // (one copy of each sweep, the segment picked at run time: unrolled over the four segments the kernel holds eight sweeps
    //  and spills scalar registers)
#pragma unroll 1
    for (int k = 0; k < segs.n; ++k) {
        const AdamSegM &sg = segs.s[k];
        if (sg.touched) adam_sweep_map<ADAM_MAP_UNROLL, WD>(sg, h, first, stride);
        else adam_sweep<WD>(AdamSeg{sg.p, sg.g, sg.m, sg.v, sg.state, sg.n}, h, true, first, stride);
    }
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamSegsDev segs, const AdamHyper h)
{
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (h.wd != 0.f) adam_multi_body<true>(segs, h, first, stride);
    else adam_multi_body<false>(segs, h, first, stride);
}

hipError_t launch_adam_prologue(int32_t *const *states, int n_states, float lr, float beta1, float beta2, hipStream_t st)
{
    AdamStates a;
    std::memset(&a, 0, sizeof(a));
    for (int k = 0; k < n_states && a.n < ADAM_MULTI_MAX_SEGS; ++k) {
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

hipError_t launch_adam_multi(const AdamSegM *segs, int n_segs, float beta1, float beta2, float eps, float wd, hipStream_t st)
{
    if (n_segs <= 0) return hipSuccess;
    if (n_segs > ADAM_MULTI_MAX_SEGS) return hipErrorInvalidValue;
    AdamSegsDev a;
    std::memset(&a, 0, sizeof(a));
    a.n = n_segs;
    int64_t n4 = 0;
    for (int k = 0; k < n_segs; ++k) {
        a.s[k] = segs[k];
        n4 = std::max(n4, (segs[k].n + 3) / 4);
    }
    if (n4 <= 0) return hipSuccess;
    const int blocks = (int)std::min((int64_t)16384, (n4 + 255) / 256);
    hipLaunchKernelGGL(adam_multi_kernel, dim3(blocks), dim3(256), 0, st, a, adam_hyper(beta1, beta2, eps, wd));
    return hipGetLastError();
}

}  // namespace okge
