// The dense optimizer, clipping and scaling kernels (gfx950); the element update itself is okge_adagrad_device.h's.
//   adagrad_kernel, adagrad2_kernel, adagrad_multi_kernel   one / two / up to four tensors per launch, entry points over ONE
//                                                           dense sweep (+ zero_grad)        utils/optim.py:139-160 / torch.optim.Adagrad
//   adagrad_lazy_kernel                                     the weight-decay-only updates of rows no batch names, deferred
//   sqnorm_partial_kernel, clip_coef_kernel                 clip_grad_norm_'s coefficient     trainer.py:236-240
//   sqnorm_multi_kernel, scale_multi_kernel                 the same over up to eight tensors, touched-row maps honoured
//   scale_kernel, rescale2_kernel                          x *= a device scalar
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "okge_kernels.h"
#include "okge_adagrad_device.h"

namespace okge {

// The dense sweep over one tensor, optionally with a touched-row byte map: a row whose byte differs from the segment's stamp
// holds an all-zero gradient by contract (the pooling backward stamps every row it writes, okge_pool.hip pass 4), so its
// gradient is neither read nor cleared -- such rows still run through the arithmetic (the reference's wd * p reaches ALL rows)
// on p and sum alone.  The stamp is never erased: the caller moves to another stamp after every update (a stale byte that
// meets its stamp again 255 updates later only costs the read of a gradient row that is zero).
// (U iterations of the grid-stride loop side by side: the map byte decides whether the gradient is loaded at all, so one
//  iteration is TWO dependent round trips -- run one at a time the sweep was latency-bound, slower than the map-less one)
template <int U, bool MAP>
__device__ __forceinline__ void adagrad_sweep(const AdagradSegM sg, float lr, float wd, float eps, int64_t first, int64_t stride)
{
    const int64_t n4 = sg.n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(sg.p), *g4 = reinterpret_cast<float4 *>(sg.g), *s4 = reinterpret_cast<float4 *>(sg.s);
    const uint32_t row4 = MAP ? (uint32_t)(sg.row_len >> 2) : 1u;
    const int shift = (row4 & (row4 - 1)) == 0 ? 31 - __clz(row4) : -1;
    const uint8_t stamp = (uint8_t)sg.stamp;
    for (int64_t i0 = first; i0 < n4; i0 += U * stride) {
        bool ok[U], live[U];
        float4 pv[U], sv[U], gv[U];
        uint8_t mb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {                            // the U map bytes first, no branch between the loads
            const int64_t i = min(i0 + u * stride, n4 - 1);
            ok[u] = i0 + u * stride < n4;
            mb[u] = stamp;
            if (MAP) mb[u] = sg.touched[shift >= 0 ? (uint32_t)i >> shift : (uint32_t)i / row4];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) live[u] = ok[u] && mb[u] == stamp;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            pv[u] = sv[u] = gv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok[u]) { pv[u] = p4[i]; sv[u] = s4[i]; }
            if (live[u]) gv[u] = g4[i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            const int64_t i = i0 + u * stride;
            const float4 p_old = pv[u], s_old = sv[u];
            adagrad4(pv[u], gv[u], sv[u], lr, wd, eps);
            adagrad_commit4(p4, s4, g4, i, pv[u], p_old, sv[u], s_old, gv[u], live[u] && sg.zero_grad);
        }
    }
    if (first < (sg.n & 3)) {                                    // (tail: only tensors without a map have one)
        const int64_t i = (n4 << 2) + first;
        adagrad1(sg.p[i], sg.g[i], sg.s[i], lr, wd, eps, sg.zero_grad);
    }
}

__device__ __forceinline__ AdagradSegM dense_seg(float *p, float *g, float *s, int64_t n, int zero_grad)
{
    return AdagradSegM{p, g, s, n, nullptr, 0, 0, zero_grad};
}

__global__ __launch_bounds__(256) void adagrad_kernel(float *__restrict__ p, float *__restrict__ g,
                                                      float *__restrict__ sum, int64_t n, float lr, float wd,
                                                      float eps, int zero_grad)
{
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    adagrad_sweep<1, false>(dense_seg(p, g, sum, n, zero_grad), lr, wd, eps, first, stride);
}

struct AdagradSeg { float *p, *g, *s; int64_t n; };     // (adagrad2_kernel's argument block, as it has always been laid out)

__global__ __launch_bounds__(256) void adagrad2_kernel(const AdagradSeg a, const AdagradSeg b, float lr, float wd,
                                                       float eps, int zero_grad)
{
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    // zero_grad: 0 none, 1 both, 2 second tensor only
    adagrad_sweep<1, false>(dense_seg(a.p, a.g, a.s, a.n, zero_grad == 1), lr, wd, eps, first, stride);
    adagrad_sweep<1, false>(dense_seg(b.p, b.g, b.s, b.n, zero_grad != 0), lr, wd, eps, first, stride);
}

// Up to four tensors in one launch (token tables + batch-norm parameters of a token-pooled step: one launch instead of two)
struct AdagradSegsDev { AdagradSegM s[ADAGRAD_MAX_SEGS]; int n; };

__global__ __launch_bounds__(256) void adagrad_multi_kernel(const AdagradSegsDev segs, float lr, float wd, float eps)
{
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
#pragma unroll
    for (int k = 0; k < ADAGRAD_MAX_SEGS; ++k)
        if (k < segs.n) {
            if (segs.s[k].touched) adagrad_sweep<4, true>(segs.s[k], lr, wd, eps, first, stride);
            else adagrad_sweep<1, false>(segs.s[k], lr, wd, eps, first, stride);
        }
}

// ---- okge_adagrad_lazy: the weight-decay-only updates of rows no batch names, deferred ------------------------------------
// The reference's Adagrad reaches every row of a table every step (weight_decay 1e-10 makes every gradient row non-zero,
// utils/optim.py:139-160): at BASELINE configs[4] 85 % of the token rows are read, moved by their own decay term and written
// back per step -- 1 GB of HBM traffic, 175 us of a 0.78 ms step.  Such a row's update depends on (p, sum) of that row alone,
// so it can be applied LATER, all pending steps at once in registers, as long as it has happened before anything reads the row:
//   row_steps[r]   number of optimizer steps row r has seen; counters[0] = T, the steps taken
//   STEP           rows the backward stamped: their T - row_steps[r] pending decay steps, then this step with the gradient;
//                  rows with r % window == T % window: their T + 1 - row_steps[r] pending decay steps; T += 1 (last workgroup)
//   catch-up       (okge_pool.hip, before the pooling forward) brings the rows the batch's tokens name to T
//   FLUSH          every row to T (before anything else reads the tables: evaluation, checkpoints, the host)
// Per step the sweep touches the stamped rows and 1 / window of the others: the traffic falls by ~window, the arithmetic
// (correctly rounded sqrt and division per element and pending step) stays and becomes the bound.  Same operations in the
// same order per element as the eager sweep: the tables are bit-identical after a FLUSH (tests/test_token_pooled.py).
struct LazySegsDev { LazySeg s[ADAGRAD_MAX_SEGS]; int n; int64_t batch0[ADAGRAD_MAX_SEGS + 1]; };

constexpr int LAZY_BATCH = 16;         // rows per wave and turn: many short turns hide the rows' load latency

__device__ __forceinline__ void adagrad_lazy_body(const LazySegsDev &segs, int32_t *counters, int window, int mode, float lr, float wd,
                                                  float eps, int lazy_batch)
{
    const int T = counters[0], target = mode == LAZY_STEP ? T + 1 : T;
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const int phase = T % window;
    // tensors with a row_steps array: batches of LAZY_BATCH rows, one per wave at a time; lane = row while the batch's bytes
    // and counters are read, lane = column quad while a row is updated
    for (int64_t b = gw; b < segs.batch0[segs.n]; b += nw) {
        int k = 0;
        while (b >= segs.batch0[k + 1]) ++k;
        const LazySeg &sg = segs.s[k];
        const int64_t r = (b - segs.batch0[k]) * lazy_batch + (lane & (lazy_batch - 1));
        const bool in = lane < lazy_batch && r < sg.rows;
        const int up = in ? sg.steps[r] : target;
        const bool stamped = mode == LAZY_STEP && in && sg.touched && sg.touched[r] == (uint8_t)sg.stamp;
        const bool due = in && (mode == LAZY_FLUSH || (int)((uint32_t)r % (uint32_t)window) == phase);      // (rows < 2^31: okge_api_optim.hip)
        const bool need = stamped || (due && up < target);
        lazy_rows(__ballot(need), r, max(0, (stamped ? T : target) - up), stamped, sg.p, sg.s, sg.g, sg.row_len, lane, lr, wd, eps);
        if (need) {
            sg.steps[r] = target;
            if (stamped) sg.touched[r] = 0;              // the map is clean again: a stamp never has to move on
        }
    }
    // plain dense tensors (batch-norm parameters): every element every step
    if (mode == LAZY_STEP) {
        const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
        for (int k = 0; k < segs.n; ++k) {
            const LazySeg &sg = segs.s[k];
            if (sg.steps) continue;
            const int64_t n = sg.rows * sg.row_len;
            for (int64_t i = first; i < n; i += stride) adagrad1(sg.p[i], sg.g[i], sg.s[i], lr, wd, eps, true);
        }
        // every workgroup has read T by the time the last one arrives here
        __shared__ int last;
        __syncthreads();
        if (threadIdx.x == 0) last = atomicAdd(&counters[1], 1) == (int)gridDim.x - 1;
        __syncthreads();
        if (last && threadIdx.x == 0) { counters[1] = 0; counters[0] = T + 1; }
    }
}

// 93 registers = 5 waves per SIMD.  Budgets of 80 / 64 registers (6 / 8 waves) spill inside the replay loops: 85 / 130 us against
// 70 us at configs[4] (profiles/round4_ablation.md section 6)
__global__ __launch_bounds__(256, 5) void adagrad_lazy_kernel(const LazySegsDev segs, int32_t *counters, int window, int mode, float lr,
                                                           float wd, float eps, int lazy_batch)
{
    adagrad_lazy_body(segs, counters, window, mode, lr, wd, eps, lazy_batch);
}

__global__ __launch_bounds__(256) void scale_kernel(float *__restrict__ x, int64_t n, const float *__restrict__ alpha)
{
    const float a = *alpha;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] *= a;
}

// The drop-in path's gradients come out of the fused step already multiplied by `applied` = the 1 / normalizer the reference
// Trainer is known to divide by (trainer.py:221); autograd later hands over the factor it really used (*alpha).  Both
// tensors in one launch, and nothing but the scalar is read when the two agree (the normal case): x *= alpha / applied.
__global__ __launch_bounds__(256) void rescale2_kernel(float *__restrict__ x0, int64_t n0, float *__restrict__ x1, int64_t n1,
                                                       const float *__restrict__ alpha, float applied)
{
    const float r = *alpha / applied;
    if (r == 1.0f) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n0; i += stride) x0[i] *= r;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n1; i += stride) x1[i] *= r;
}

// ---- gradient clipping (trainer.py:236-240: torch.nn.utils.clip_grad_norm_) ----------------------------------------------------
__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float *__restrict__ g0, int64_t n0, const float *__restrict__ g1,
                                                             int64_t n1, double *__restrict__ partial)
{
    __shared__ double red[4];
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = first; i < n0; i += stride) acc += (double)g0[i] * (double)g0[i];
    for (int64_t i = first; i < n1; i += stride) acc += (double)g1[i] * (double)g1[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void clip_coef_kernel(const double *__restrict__ partial, int n, float max_norm,
                                                        float *__restrict__ coef, double *__restrict__ norm_out)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partial[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(red[0] + red[1] + red[2] + red[3]);        // torch keeps the norm in fp32
        const float c = max_norm / (total + 1e-6f);
        coef[0] = c < 1.f ? c : 1.f;
        if (norm_out) norm_out[0] = (double)total;
    }
}

// ---- okge_clip_grad_norm_multi: the same over up to eight tensors, a tensor optionally with a touched-row byte map -------------
// One walk for the sum and the scaling: thread `first` of the grid owns the quads first, first + stride, ... of every tensor
// (elements 4q .. 4q + 3, in that order) and, below n & 3, one tail element.  Which thread sees which element is fixed by the
// sizes and the grid, so with a fixed grid the partial sums -- and the norm -- come out bit-identical from run to run, whether a
// quad is read as one 16-byte access (base 16-byte aligned) or as four floats.  With a map, a row whose byte differs from the
// stamp is skipped whole (zeros by the maps' contract: neither read nor written); rows are whole quads, there is no tail.
struct GradSegsDev { GradSeg s[CLIP_MAX_SEGS]; int n; };

template <typename F>
__device__ __forceinline__ void grad_walk(const GradSeg &sg, int64_t first, int64_t stride, F &&f)
{
    const int64_t n4 = sg.n >> 2;
    const bool vec = (reinterpret_cast<uintptr_t>(sg.g) & 15) == 0;
    const uint32_t row4 = sg.touched ? (uint32_t)(sg.row_len >> 2) : 1u;
    const uint8_t stamp = (uint8_t)sg.stamp;
    for (int64_t i = first; i < n4; i += stride) {
        if (sg.touched && sg.touched[i >> 32 ? i / row4 : (int64_t)((uint32_t)i / row4)] != stamp) continue;
        float *x = sg.g + (i << 2);
        if (vec) {
            float4 v = *reinterpret_cast<float4 *>(x);
            if (f(v.x, v.y, v.z, v.w)) *reinterpret_cast<float4 *>(x) = v;
        } else if (f(x[0], x[1], x[2], x[3])) {
            // (f wrote through the references)
        }
    }
    if (first < (sg.n & 3)) {
        float pad0 = 0.f, pad1 = 0.f, pad2 = 0.f;
        f(sg.g[(n4 << 2) + first], pad0, pad1, pad2);
    }
}

__global__ __launch_bounds__(256) void sqnorm_multi_kernel(const GradSegsDev segs, double *__restrict__ partial)
{
    __shared__ double red[4];
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < segs.n; ++k)
        grad_walk(segs.s[k], first, stride, [&acc](float &a, float &b, float &c, float &d) {
            acc += (double)a * (double)a;
            acc += (double)b * (double)b;
            acc += (double)c * (double)c;
            acc += (double)d * (double)d;
            return false;
        });
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void scale_multi_kernel(const GradSegsDev segs, const float *__restrict__ coef)
{
    const float c = *coef;
    if (c == 1.0f) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < segs.n; ++k)
        grad_walk(segs.s[k], first, stride, [c](float &a, float &b, float &d, float &e) {
            a *= c; b *= c; d *= c; e *= c;
            return true;
        });
}

// ---- launchers -----------------------------------------------------------------------------------------
hipError_t launch_adagrad(float *p, float *g, float *sum, int64_t n, float lr, float wd, float eps, int zero_grad,
                          hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int64_t n4 = (n + 3) / 4;
    const int blocks = (int)min((int64_t)16384, (n4 + 255) / 256);
    hipLaunchKernelGGL(adagrad_kernel, dim3(blocks), dim3(256), 0, st, p, g, sum, n, lr, wd, eps, zero_grad);
    return hipGetLastError();
}

hipError_t launch_adagrad2(float *p0, float *g0, float *s0, int64_t n0, float *p1, float *g1, float *s1, int64_t n1,
                           float lr, float wd, float eps, int zero_grad, hipStream_t st)
{
    const int64_t n4 = (std::max(n0, n1) + 3) / 4;
    if (n4 <= 0) return hipSuccess;
    const int blocks = (int)std::min((int64_t)16384, (n4 + 255) / 256);
    const AdagradSeg a{p0, g0, s0, n0}, b{p1, g1, s1, n1};
    hipLaunchKernelGGL(adagrad2_kernel, dim3(blocks), dim3(256), 0, st, a, b, lr, wd, eps, zero_grad);
    return hipGetLastError();
}

hipError_t launch_adagrad_multi(const AdagradSegM *segs, int n_segs, float lr, float wd, float eps, hipStream_t st)
{
    if (n_segs <= 0) return hipSuccess;
    if (n_segs > ADAGRAD_MAX_SEGS) return hipErrorInvalidValue;
    AdagradSegsDev a;
    std::memset(&a, 0, sizeof(a));
    a.n = n_segs;
    int64_t n4 = 0;
    for (int k = 0; k < n_segs; ++k) {
        a.s[k] = segs[k];
        n4 = std::max(n4, (segs[k].n + 3) / 4);
    }
    if (n4 <= 0) return hipSuccess;
    const int blocks = (int)std::min((int64_t)16384, (n4 + 255) / 256);
    hipLaunchKernelGGL(adagrad_multi_kernel, dim3(blocks), dim3(256), 0, st, a, lr, wd, eps);
    return hipGetLastError();
}

hipError_t launch_adagrad_lazy(const LazySeg *segs, int n_segs, int32_t *counters, int window, int mode, float lr, float wd,
                               float eps, hipStream_t st)
{
    if (n_segs <= 0) return hipSuccess;
    if (n_segs > ADAGRAD_MAX_SEGS || window < 1 || !counters) return hipErrorInvalidValue;
    LazySegsDev a;
    std::memset(&a, 0, sizeof(a));
    a.n = n_segs;
    static const int lazy_batch_env = getenv("OKGE_LAZY_BATCH") ? atoi(getenv("OKGE_LAZY_BATCH")) : LAZY_BATCH;
    const int lazy_batch = (lazy_batch_env == 8 || lazy_batch_env == 32 || lazy_batch_env == 64) ? lazy_batch_env : LAZY_BATCH;
    for (int k = 0; k < n_segs; ++k) {
        a.s[k] = segs[k];
        a.batch0[k + 1] = a.batch0[k] + (segs[k].steps ? (segs[k].rows + lazy_batch - 1) / lazy_batch : 0);
    }
    // (every wave resident: 5 per SIMD; a wave takes batch after batch)
    const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>((a.batch0[n_segs] + 3) / 4, 256 * 5));
    hipLaunchKernelGGL(adagrad_lazy_kernel, dim3((unsigned)wgs), dim3(256), 0, st, a, counters, window, mode, lr, wd, eps, lazy_batch);
    return hipGetLastError();
}

hipError_t launch_scale(float *x, int64_t n, const float *alpha_dev, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::min((int64_t)4096, (n + 255) / 256);
    hipLaunchKernelGGL(scale_kernel, dim3(blocks), dim3(256), 0, st, x, n, alpha_dev);
    return hipGetLastError();
}

hipError_t launch_rescale2(float *x0, int64_t n0, float *x1, int64_t n1, const float *alpha_dev, float applied, hipStream_t st)
{
    const int64_t n = std::max(n0, n1);
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::min((int64_t)2048, (n + 255) / 256);
    hipLaunchKernelGGL(rescale2_kernel, dim3(blocks), dim3(256), 0, st, x0, n0, x1, n1, alpha_dev, applied);
    return hipGetLastError();
}

hipError_t launch_clip_coef(const float *g0, int64_t n0, const float *g1, int64_t n1, float max_norm, double *partial,
                            int n_partial, float *coef_dev, double *norm_dev, hipStream_t st)
{
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(n_partial), dim3(256), 0, st, g0, n0, g1, n1, partial);
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, st, partial, n_partial, max_norm, coef_dev, norm_dev);
    return hipGetLastError();
}

hipError_t launch_clip_multi(const GradSeg *segs, int n_segs, float max_norm, double *partial, int n_partial, float *coef_dev,
                             double *norm_dev, hipStream_t st)
{
    if (n_segs <= 0 || n_segs > CLIP_MAX_SEGS) return hipErrorInvalidValue;
    GradSegsDev a;
    std::memset(&a, 0, sizeof(a));
    a.n = n_segs;
    int64_t n4 = 0;
    for (int k = 0; k < n_segs; ++k) {
        a.s[k] = segs[k];
        n4 = std::max(n4, (segs[k].n + 3) / 4);
    }
    hipLaunchKernelGGL(sqnorm_multi_kernel, dim3(n_partial), dim3(256), 0, st, a, partial);
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, st, partial, n_partial, max_norm, coef_dev, norm_dev);
    const int blocks = (int)std::max<int64_t>(1, std::min((int64_t)4096, (n4 + 255) / 256));
    hipLaunchKernelGGL(scale_multi_kernel, dim3(blocks), dim3(256), 0, st, a, coef_dev);
    return hipGetLastError();
}

}  // namespace okge
