// Microbenchmark for the three-plane bf16 dQ kernel (csrc/okge_dq_split.{h,hip}); results: profiles/dq_split_ablation.md.
//  (a) How does v_mfma_f32_16x16x32_bf16 round?  Every A row is ak[0..31] and every B column is bk[0..31], so each output
//      element is C + sum_k ak[k] bk[k] whatever the lane <-> k map; operands are chosen so that round-to-nearest, truncation,
//      product-by-product accumulation and a wider internal sum give different fp32 bits.  Printed as hex.
//  (b) Cycles per 32-candidate sub-chunk of the kernel's own loop at KB = 13, one 512-thread workgroup per CU:
//      bare MFMAs on register operands / operands read from LDS (DqSplit::product) / product + park + barrier (the kernel's
//      loop without its global loads) in its two forms: BEFORE the tile kernel wrote the candidate planes -- every fp32
//      candidate row and G^T split here, the retired staging kept below as OldStage / park_split_all -- and as it is NOW --
//      candidate cells copied, G^T split on four waves (DqSplit::park).  The matrix-core floor is 78 MFMAs per SIMD x 16
//      cycles = 1248.
//  (c) The train tile's gradient phase dC += G^T . Q per 64-row chunk at KB = 13 (csrc/okge_tile_grad_split.h), 256 workgroups of 8 waves, one
//      barrier per chunk: the fp32 loop fused_tile64_kernel runs today (104 v_mfma_f32_16x16x4_f32 per wave, operands read from
//      the fp32 chunk in LDS) against the three-plane form (one split3 of the lane's 8 G values, 78 v_mfma_f32_16x16x32_bf16, B
//      cells read from the plane image) with the corrections folded per chunk or in an accumulator of their own, each without
//      and with the next chunk's planes copied global -> LDS beside it.  Floors per SIMD (two waves): 2 x 3328 cycles fp32,
//      2 x 1248 bf16; the LDS reads of the bf16 form are 8 waves x 39 KiB per chunk.
//  (d) The train tile's score phase X = Q . C^T per 64-row chunk at KB = 13 and both phases together: the fp32 loop
//      fused_tile64_kernel ran (a frozen copy: 2 x 50 v_mfma_f32_16x16x4_f32 per wave from an fp32 chunk in LDS, the candidate
//      operand in registers, the short last round of slot sizes 193 .. 200) against TileScoreSplit::score (72
//      v_mfma_f32_16x16x32_bf16 + 12 v_mfma_f32_16x16x16_bf16 per wave, the query operand read transposed from the plane
//      image), and score + gradient phase per chunk from two plane buffers with the next chunk's copy beside them and one
//      barrier per chunk -- the loop the kernel runs now, without its loss epilogue.  The gate of profiles/tile_score_split.md
//      compares the last against the sum of the fp32 score loop and part (c)'s "folded + copy" gradient loop of the same run.
// Build: hipcc -O3 --offload-arch=gfx950 -std=c++17 -o mfma_bf16_split.bin mfma_bf16_split.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../open_knowledge_graph_embeddings_amd/csrc/okge_dq_split.h"
#include "../../open_knowledge_graph_embeddings_amd/csrc/okge_tile_grad_split.h"
using namespace okge;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)

// ---- (a) ------------------------------------------------------------------------------------------------------------
struct Probe { const char *what; float c; float ak[32], bk[32]; };

__global__ __launch_bounds__(64) void probe_kernel(const float *ak, const float *bk, const float *c0, float *out, int n)
{
    const int lane = threadIdx.x, kg = lane >> 4;
    for (int p = 0; p < n; ++p) {
        v8bf a, b;
        for (int j = 0; j < 8; ++j) { a[j] = (__bf16)ak[32 * p + 8 * kg + j]; b[j] = (__bf16)bk[32 * p + 8 * kg + j]; }
        v4f c = (v4f){c0[p], c0[p], c0[p], c0[p]};
        c = mfma_bf16(a, b, c);
        if (lane == 0) out[p] = c[0];
        if (lane == 37) out[n + p] = c[3];            // another element of the tile: must be the same number
    }
}

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

// ---- (b) ------------------------------------------------------------------------------------------------------------
// the staging dq8s_kernel had while the masked candidate rows reached it in fp32: threads 0 .. 4 NQ - 1 hold 8 candidates x one
// float4 of the rows, wave 6 the same of the G^T block; everything is split when it is parked
struct OldStage { v4f v[8]; };
template <int KB>
__device__ void park_split_all(const OldStage &st, v8bf *buf, int tid)
{
    using S = DqSplit<KB>;
    constexpr int C_TASKS = 4 * S::NQ, G_TID0 = 384;
    v8bf *dst;
    int stride, plane;
    if (tid < C_TASKS) {
        dst = buf + (tid / S::NQ) * S::NS + tid % S::NQ; stride = S::NQ; plane = S::C_CELLS;
    } else if (tid >= G_TID0 && tid < G_TID0 + 64) {
        dst = buf + 3 * S::C_CELLS + ((tid - G_TID0) >> 4) * 64 + (tid & 15); stride = 16; plane = S::G_CELLS;
    } else {
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = st.v[k][j];
        const Planes p = split3(x);
        dst[j * stride] = p.hi;
        dst[j * stride + plane] = p.mid;
        dst[j * stride + 2 * plane] = p.lo;
    }
}

// variant not kept: candidate cells copied as now, G^T still split by wave 6 alone (one float4 x 8 candidates per thread)
template <int KB>
__device__ void park_copy_g_wave6(const typename DqSplit<KB>::Stage &st, const OldStage &g, v8bf *buf, int tid)
{
    using S = DqSplit<KB>;
#pragma unroll
    for (int i = 0; i < S::C_COPY; ++i)
        if (i * S::THREADS + tid < S::C_BLOCK) buf[i * S::THREADS + tid] = st.c[i];
    if (tid >= 384 && tid < 448) park_split_all<KB>(g, buf, tid);
}

template <int MODE>
__global__ __launch_bounds__(512, 2) void loop_kernel(const float *src, float *out, unsigned long long *cyc, int iters)
{
    using S = DqSplit<13>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v8bf *lds = reinterpret_cast<v8bf *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int h = w >> 2, blk0 = S::wave_blk0(h, w & 3), nblk = S::wave_nblk(h, w & 3);
    v4f acc[2][S::NBW], corr[2][S::NBW];
    for (int r = 0; r < 2; ++r)
        for (int nb = 0; nb < S::NBW; ++nb) acc[r][nb] = corr[r][nb] = (v4f){0.f, 0.f, 0.f, 0.f};
    OldStage old;
    for (int k = 0; k < 8; ++k) old.v[k] = *reinterpret_cast<const v4f *>(src + (size_t)(tid * 8 + k) * 4);
    typename S::Stage st;                             // any finite bf16 cells / floats will do
    for (int i = 0; i < S::C_COPY; ++i) {
        float x[8];
        for (int k = 0; k < 8; ++k) x[k] = old.v[k][i & 3] + (float)i;
        st.c[i] = split3(x).hi;
    }
    for (int k = 0; k < 8; ++k) st.g[k] = old.v[k][0];
    S::park(st, lds, tid);
    S::park(st, lds + S::BUF_CELLS, tid);
    __syncthreads();
    Planes ra, rb;
    ra.hi = lds[lane]; ra.mid = lds[lane + 64]; ra.lo = lds[lane + 128];
    rb.hi = lds[lane + 192]; rb.mid = lds[lane + 256]; rb.lo = lds[lane + 320];
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        const int buf = it & 1;
        if (MODE == 0) {
#pragma unroll
            for (int nb = 0; nb < S::NBW; ++nb)
                if (nb < nblk)
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        v4f s = corr[r][nb];
                        s = mfma_bf16(ra.lo, rb.hi, s); s = mfma_bf16(ra.hi, rb.lo, s); s = mfma_bf16(ra.mid, rb.mid, s);
                        s = mfma_bf16(ra.mid, rb.hi, s); s = mfma_bf16(ra.hi, rb.mid, s);
                        corr[r][nb] = s;
                        acc[r][nb] = mfma_bf16(ra.hi, rb.hi, acc[r][nb]);
                    }
        } else if (MODE == 1) {
            S::product(acc, corr, lds + buf * S::BUF_CELLS, h, blk0, nblk, lane);
        } else if (MODE == 2) {
            __syncthreads();
            // the staged values change every iteration (as they do in the kernel), so the split cannot be hoisted out of the loop
            for (int k = 0; k < 8; ++k) old.v[k] += (v4f){1e-3f, 1e-3f, 1e-3f, 1e-3f};
            if (w < 4) park_split_all<13>(old, lds + (buf ^ 1) * S::BUF_CELLS, tid);
            S::product(acc, corr, lds + buf * S::BUF_CELLS, h, blk0, nblk, lane);
            if (w >= 4) park_split_all<13>(old, lds + (buf ^ 1) * S::BUF_CELLS, tid);
        } else if (MODE == 4) {
            __syncthreads();
            for (int k = 0; k < 8; ++k) old.v[k] += (v4f){1e-3f, 1e-3f, 1e-3f, 1e-3f};
            if (w < 4) park_copy_g_wave6<13>(st, old, lds + (buf ^ 1) * S::BUF_CELLS, tid);
            S::product(acc, corr, lds + buf * S::BUF_CELLS, h, blk0, nblk, lane);
            if (w >= 4) park_copy_g_wave6<13>(st, old, lds + (buf ^ 1) * S::BUF_CELLS, tid);
        } else {
            __syncthreads();
            for (int k = 0; k < 8; ++k) st.g[k] += 1e-3f;
            if (w < 4) S::park(st, lds + (buf ^ 1) * S::BUF_CELLS, tid);
            S::product(acc, corr, lds + buf * S::BUF_CELLS, h, blk0, nblk, lane);
            if (w >= 4) S::park(st, lds + (buf ^ 1) * S::BUF_CELLS, tid);
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0.f;
    for (int r = 0; r < 2; ++r)
        for (int nb = 0; nb < S::NBW; ++nb) for (int i = 0; i < 4; ++i) s += acc[r][nb][i] + corr[r][nb][i];
    out[blockIdx.x * 512 + tid] = s;
    if (lane == 0) cyc[blockIdx.x * 8 + w] = t1 - t0;
}

template <int MODE>
static int run_loop(const char *name, const float *src, float *out, unsigned long long *cyc, int blocks, int iters)
{
    auto k = loop_kernel<MODE>;
    const size_t shmem = DqSplit<13>::LDS_BYTES;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(512), shmem, 0, src, out, cyc, iters);   // warm-up
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(512), shmem, 0, src, out, cyc, iters);
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> hc(blocks * 8);
    CK(hipMemcpy(hc.data(), cyc, hc.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long mx = 0; double mean = 0;
    for (auto c : hc) { mx = c > mx ? c : mx; mean += (double)c / hc.size(); }
    // s_memtime ticks at a fixed 100 MHz-class clock on this part, so the event time is the trustworthy figure; both are printed
    const double flop = 12.0 * 64 * 208 * 32 * (double)iters * blocks;
    printf("%-44s %8.3f ms  %7.1f ns/sub-chunk  %6.1f TFLOP/s executed (bf16)   s_memtime ticks/iter: mean %.1f max %.1f\n", name, ms,
           ms * 1e6 / iters, flop / (ms * 1e-3) * 1e-12, mean / iters, (double)mx / iters);
    return 0;
}

// ---- (c) ------------------------------------------------------------------------------------------------------------
// MODE 0: the fp32 loop (a frozen copy, see below); 1 / 2: three planes, corrections folded / in their own accumulator; 3 / 4: the same with the next
// chunk's planes copied beside the product.  Every mode declares the same LDS (two plane chunks), so one workgroup per CU.
template <int MODE>
__global__ __launch_bounds__(512, 2) void grad_phase_kernel(const float *src, const v8bf *planes, float *out, unsigned long long *cyc, int iters)
{
    constexpr int KB = 13, KQ = KB / 4, KR = KB % 4, LDK = lds_ld(16 * KB);
    constexpr bool FOLD = MODE == 1 || MODE == 3, COPY = MODE >= 3;
    using T = TileGradSplit<KB>;
    static_assert(64 * LDK * 4 <= T::CHUNK_CELLS * 16, "the fp32 chunk fits the first plane buffer");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v8bf *lds = reinterpret_cast<v8bf *>(smem);           // two plane chunks; the fp32 loop reads the first as [64][LDK] floats
    const float *Qs = reinterpret_cast<const float *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, s = lane >> 4, h = w >> 2;
    // any finite numbers will do: floats of magnitude < 1 for the fp32 loop, bf16 cells for the plane loops
    if (MODE == 0) {
        for (int i = tid; i < 64 * LDK; i += 512) reinterpret_cast<float *>(smem)[i] = src[i & 16383];
    } else {
        for (int i = tid; i < 2 * T::CHUNK_CELLS; i += 512) {
            float x[8];
            for (int k = 0; k < 8; ++k) x[k] = src[(8 * i + k) & 16383];
            lds[i] = split3(x).hi;
        }
    }
    v4f g4[2];
    for (int rg = 0; rg < 2; ++rg) g4[rg] = *reinterpret_cast<const v4f *>(src + 8 * tid + 4 * rg) * 1e-3f;
    v4f dc[KB], corr[FOLD || MODE == 0 ? 1 : KB];
    for (int kb = 0; kb < KB; ++kb) dc[kb] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (auto &v : corr) v = (v4f){0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        __syncthreads();
        // G changes every chunk, as in the kernel: the split cannot be hoisted out of the loop
        for (int rg = 0; rg < 2; ++rg) g4[rg] += (v4f){1e-6f, 2e-6f, 3e-6f, 4e-6f};
        if constexpr (MODE == 0) {
            const float *qb = Qs + (32 * h + 4 * s) * LDK;
            v4f pb[KQ];
            float pr[KR];
#pragma unroll
            for (int kq = 0; kq < KQ; ++kq) pb[kq] = *reinterpret_cast<const v4f *>(qb + 64 * kq + 4 * c);
#pragma unroll
            for (int r = 0; r < KR; ++r) pr[r] = qb[64 * KQ + 16 * r + c];
#pragma unroll
            // a FROZEN COPY of the fp32 loop fused_tile64_kernel ran at KB = 13 before this form (okge_train64.hip, "dC += G^T . Q",
            // as it still stands there for the other instances): the baseline of the comparison, not shared code -- an edit of
            // the kernel's fp32 loop does not reach it
            for (int u = 0; u < 8; ++u) {
                const float av = g4[u >> 2][u & 3];
                v4f nb[KQ];
                float nr[KR];
                if (u + 1 < 8) {
                    const float *brow = qb + (16 * ((u + 1) >> 2) + ((u + 1) & 3)) * LDK;
#pragma unroll
                    for (int kq = 0; kq < KQ; ++kq) nb[kq] = *reinterpret_cast<const v4f *>(brow + 64 * kq + 4 * c);
#pragma unroll
                    for (int r = 0; r < KR; ++r) nr[r] = brow[64 * KQ + 16 * r + c];
                }
#pragma unroll
                for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
                    for (int e = 0; e < 4; ++e) dc[4 * kq + e] = mfma16(av, pb[kq][e], dc[4 * kq + e]);
#pragma unroll
                for (int r = 0; r < KR; ++r) dc[4 * KQ + r] = mfma16(av, pr[r], dc[4 * KQ + r]);
                if (u + 1 < 8) {
#pragma unroll
                    for (int kq = 0; kq < KQ; ++kq) pb[kq] = nb[kq];
#pragma unroll
                    for (int r = 0; r < KR; ++r) pr[r] = nr[r];
                    __builtin_amdgcn_sched_group_barrier(0x100, KQ + KR, 1);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, KB, 1);
            }
        } else {
            const int buf = COPY ? it & 1 : 0;
            if (COPY) T::copy_chunk(planes + (size_t)(it & 7) * T::CHUNK_CELLS, lds + (buf ^ 1) * T::CHUNK_CELLS, w, lane);
            const Planes a = T::a_planes(g4, s);
            T::template product<FOLD>(dc, corr, a, lds + buf * T::CHUNK_CELLS, h, lane);
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float sum = 0.f;
    for (int kb = 0; kb < KB; ++kb) for (int i = 0; i < 4; ++i) sum += dc[kb][i];
    for (auto &v : corr) for (int i = 0; i < 4; ++i) sum += v[i];
    out[blockIdx.x * 512 + tid] = sum;
    if (lane == 0) cyc[blockIdx.x * 8 + w] = t1 - t0;
}

template <int MODE>
static int run_phase(const char *name, const float *src, const v8bf *planes, float *out, unsigned long long *cyc, int blocks, int iters)
{
    auto k = grad_phase_kernel<MODE>;
    const size_t shmem = (size_t)2 * TileGradSplit<13>::CHUNK_CELLS * 16;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(512), shmem, 0, src, planes, out, cyc, iters);   // warm-up
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(512), shmem, 0, src, planes, out, cyc, iters);
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> hc(blocks * 8);
    CK(hipMemcpy(hc.data(), cyc, hc.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long mx = 0; double mean = 0;
    for (auto v : hc) { mx = v > mx ? v : mx; mean += (double)v / hc.size(); }
    printf("%-58s %8.3f ms  %7.1f ns/chunk   s_memtime ticks/chunk: mean %.1f max %.1f\n", name, ms, ms * 1e6 / iters, mean / iters,
           (double)mx / iters);
    return 0;
}

// ---- (d) ------------------------------------------------------------------------------------------------------------
// MODE 0: the fp32 score loop (frozen copy); 1: the plane score loop; 2: score + gradient phase + the next chunk's copy issued
// in front of the score phase; 3: the copy issued between the phases (where the kernel has its VALU-only loss epilogue); 4: half
// of it in front, half between
template <int MODE>
__global__ __launch_bounds__(512, 2) void score_phase_kernel(const float *src, const v8bf *planes, float *out, unsigned long long *cyc, int iters)
{
    constexpr int KB = 13, LDK = lds_ld(16 * KB);
    using T = TileGradSplit<KB>;
    using S = TileScoreSplit<KB>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v8bf *lds = reinterpret_cast<v8bf *>(smem);           // two plane chunks; the fp32 loop reads the first as [64][LDK] floats
    const float *Qc = reinterpret_cast<const float *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, s = lane >> 4, h = w >> 2;
    if (MODE == 0) {
        for (int i = tid; i < 64 * LDK; i += 512) reinterpret_cast<float *>(smem)[i] = src[i & 16383];
    } else {
        for (int i = tid; i < 2 * T::CHUNK_CELLS; i += 512) {
            float x[8];
            for (int k = 0; k < 8; ++k) x[k] = src[(8 * i + k) & 16383];
            lds[i] = split3(x).hi;
        }
    }
    v4f breg[KB];
    typename S::BOp bop;
    if (MODE == 0) {
        for (int r = 0; r < KB; ++r) breg[r] = *reinterpret_cast<const v4f *>(src + ((16 * tid + 4 * r) & 16383));
    } else {
        S::load_b(bop, src + ((212 * tid) & 8191), s);
    }
    v4f dc[KB], none[1];
    for (int kb = 0; kb < KB; ++kb) dc[kb] = (v4f){0.f, 0.f, 0.f, 0.f};
    v4f xsum = (v4f){0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        if (MODE >= 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (MODE == 0) {
            // a FROZEN COPY of the fp32 score loop fused_tile64_kernel<13, ., true> ran before TileScoreSplit: the baseline of the
            // comparison, not shared code
            v4f x0 = (v4f){0.f, 0.f, 0.f, 0.f}, x1 = (v4f){0.f, 0.f, 0.f, 0.f};
            const float *qa0 = Qc + (32 * h + c) * LDK + 4 * s;
            const float *qa1 = qa0 + 16 * LDK;
            v4f a00 = *reinterpret_cast<const v4f *>(qa0), a01 = *reinterpret_cast<const v4f *>(qa1);
            v4f b0v = breg[0];
            v4f a10 = *reinterpret_cast<const v4f *>(qa0 + 16), a11 = *reinterpret_cast<const v4f *>(qa1 + 16), b1v = breg[1];
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
            for (int r = 0; r < KB; ++r) {
                v4f a20 = a10, a21 = a11, b2v = b1v;
                const bool short_next = r + 2 == KB - 1;
                if (r + 2 < KB) {
                    if (short_next) {
                        const float *q0 = Qc + (32 * h + c) * LDK + 16 * (KB - 1) + s, *q1 = q0 + 16 * LDK;
                        a20[0] = q0[0]; a20[1] = q0[4];
                        a21[0] = q1[0]; a21[1] = q1[4];
                    } else {
                        a20 = *reinterpret_cast<const v4f *>(qa0 + 16 * (r + 2));
                        a21 = *reinterpret_cast<const v4f *>(qa1 + 16 * (r + 2));
                    }
                    b2v = breg[r + 2 < KB ? r + 2 : 0];
                }
                const int nj = r == KB - 1 ? 2 : 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < nj) {
                        x0 = mfma16(a00[j], b0v[j], x0);
                        x1 = mfma16(a01[j], b0v[j], x1);
                    }
                }
                a00 = a10; a01 = a11; b0v = b1v;
                a10 = a20; a11 = a21; b1v = b2v;
                if (short_next) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                else __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                if (nj == 2) __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                else __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
            }
            xsum += x0 + x1;
        } else {
            const int buf = MODE >= 2 ? it & 1 : 0;
            const v8bf *csrc = planes + (size_t)(it & 7) * T::CHUNK_CELLS;
            v8bf *cdst = lds + (buf ^ 1) * T::CHUNK_CELLS;
            if (MODE == 2) T::copy_chunk(csrc, cdst, w, lane);
            if (MODE == 4) T::template copy_chunk<0, 5>(csrc, cdst, w, lane);
            v4f x[2];
            S::score(x, bop, lds + buf * T::CHUNK_CELLS, h, lane);
            xsum += x[0] + x[1];
            if (MODE == 3) T::copy_chunk(csrc, cdst, w, lane);
            if (MODE == 4) T::template copy_chunk<5>(csrc, cdst, w, lane);
            if (MODE >= 2) {
                // G is a function of the scores, as in the kernel: the gradient phase cannot start before the score phase ends
                const v4f g4[2] = {x[0] * 1e-3f, x[1] * 1e-3f};
                T::template product<true>(dc, none, T::a_planes(g4, s), lds + buf * T::CHUNK_CELLS, h, lane);
            }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float sum = xsum[0] + xsum[1] + xsum[2] + xsum[3];
    for (int kb = 0; kb < KB; ++kb) for (int i = 0; i < 4; ++i) sum += dc[kb][i];
    out[blockIdx.x * 512 + tid] = sum;
    if (lane == 0) cyc[blockIdx.x * 8 + w] = t1 - t0;
}

template <int MODE>
static int run_score(const char *name, const float *src, const v8bf *planes, float *out, unsigned long long *cyc, int blocks, int iters, double *ns)
{
    auto k = score_phase_kernel<MODE>;
    const size_t shmem = (size_t)2 * TileGradSplit<13>::CHUNK_CELLS * 16;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(512), shmem, 0, src, planes, out, cyc, iters);   // warm-up
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(512), shmem, 0, src, planes, out, cyc, iters);
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    *ns = ms * 1e6 / iters;
    printf("%-58s %8.3f ms  %7.1f ns/chunk\n", name, ms, *ns);
    return 0;
}

int main()
{
    // (a)
    std::vector<Probe> P;
    auto add = [&](const char *what, float c) { Probe p{}; p.what = what; p.c = c; P.push_back(p); return &P.back(); };
    const float u = ldexpf(1.f, -24);                 // half an ulp of 1.0
    Probe *p;
    p = add("C=1 + one product 1.0*2^-24 (tie)          RN-even 3f800000  trunc 3f800000", 1.f); p->ak[0] = 1.f; p->bk[0] = u;
    p = add("C=1 + one product 1.5*2^-24                RN 3f800001  trunc 3f800000", 1.f); p->ak[0] = 1.5f; p->bk[0] = u;
    p = add("C=1 + one product 3*2^-24 (tie)            RN-even 3f800002  trunc 3f800001", 1.f); p->ak[0] = 3.f; p->bk[0] = u;
    p = add("C=1 + two products 0.75*2^-24              summed-then-RN 3f800001  one-by-one-RN 3f800000  trunc 3f800000", 1.f);
    p->ak[0] = p->ak[9] = 0.75f; p->bk[0] = p->bk[9] = u;
    p = add("C=1 + 32 products of 2^-25                 wide sum 3f800008  one-by-one (any rounding) 3f800000", 1.f);
    for (int k = 0; k < 32; ++k) { p->ak[k] = 1.f; p->bk[k] = ldexpf(1.f, -25); }
    p = add("C=1 - one product 2^-26                    RN 3f800000  trunc-to-zero/floor 3f7fffff", 1.f); p->ak[0] = -1.f; p->bk[0] = ldexpf(1.f, -26);
    p = add("C=-1 + one product 2^-26                   RN bf800000  to-zero bf7fffff  floor bf800000", -1.f); p->ak[0] = 1.f; p->bk[0] = ldexpf(1.f, -26);
    p = add("C=0, products 1.0 and 1.5*2^-24            RN 3f800001  trunc 3f800000", 0.f); p->ak[0] = 1.f; p->bk[0] = 1.f; p->ak[20] = 1.5f; p->bk[20] = u;
    p = add("C=0, products 2^10, -2^10, 2^-20           exact 35800000  (0 = the small product fell off the internal sum)", 0.f);
    p->ak[0] = 1024.f; p->bk[0] = 1.f; p->ak[1] = -1024.f; p->bk[1] = 1.f; p->ak[2] = 1.f; p->bk[2] = ldexpf(1.f, -20);
    p = add("C=0, products 2^10, -2^10, 2^-40           exact 2b800000", 0.f);
    p->ak[0] = 1024.f; p->bk[0] = 1.f; p->ak[1] = -1024.f; p->bk[1] = 1.f; p->ak[2] = 1.f; p->bk[2] = ldexpf(1.f, -40);
    p = add("C=2^10, products -2^10, 2^-20              exact 35800000", 1024.f); p->ak[0] = -1024.f; p->bk[0] = 1.f; p->ak[2] = 1.f; p->bk[2] = ldexpf(1.f, -20);
    p = add("C=0, one product 1e-19 * 1 (normal bf16)   kept: 2008xxxx-ish, flushed: 00000000", 0.f); p->ak[0] = 1e-19f; p->bk[0] = 1.f;
    p = add("C=0, one product 1e-19 * 1e-19             (1e-38, a normal fp32 just above the subnormals)", 0.f); p->ak[0] = 1e-19f; p->bk[0] = 1e-19f;
    p = add("C=0, one product 2^-70 * 2^-70 = 2^-140    subnormal result kept 00000200, flushed 00000000", 0.f); p->ak[0] = ldexpf(1.f, -70); p->bk[0] = ldexpf(1.f, -70);
    p = add("C=0, one product 2^-130 * 2^10             subnormal bf16 input kept 03800000 (2^-120), flushed 00000000", 0.f); p->ak[0] = ldexpf(1.f, -130); p->bk[0] = 1024.f;
    p = add("C=2^-130 (subnormal) + 0                   kept 00080000, flushed 00000000", ldexpf(1.f, -130));
    const int n = (int)P.size();
    std::vector<float> hak(32 * n), hbk(32 * n), hc(n), hout(2 * n);
    for (int i = 0; i < n; ++i) { memcpy(&hak[32 * i], P[i].ak, 128); memcpy(&hbk[32 * i], P[i].bk, 128); hc[i] = P[i].c; }
    float *dak, *dbk, *dc, *dout;
    CK(hipMalloc(&dak, 128 * n)); CK(hipMalloc(&dbk, 128 * n)); CK(hipMalloc(&dc, 4 * n)); CK(hipMalloc(&dout, 8 * n));
    CK(hipMemcpy(dak, hak.data(), 128 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dbk, hbk.data(), 128 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, hc.data(), 4 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(64), 0, 0, dak, dbk, dc, dout, n);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(hout.data(), dout, 8 * n, hipMemcpyDeviceToHost));
    printf("== (a) v_mfma_f32_16x16x32_bf16 rounding probes: got (lane 0 elt 0 / lane 37 elt 3)\n");
    for (int i = 0; i < n; ++i) printf("  %08x / %08x  % .9e   %s\n", bits(hout[i]), bits(hout[n + i]), hout[i], P[i].what);

    // (b)
    const int blocks = 256, iters = 4000;
    std::vector<float> hs(512 * 32);
    unsigned x = 12345u;
    for (auto &v : hs) { x = x * 1664525u + 1013904223u; v = ((int)(x >> 8) - (1 << 23)) * (1.f / (1 << 23)); }
    float *src, *out; unsigned long long *cyc;
    CK(hipMalloc(&src, hs.size() * 4)); CK(hipMalloc(&out, 4 * 512 * blocks)); CK(hipMalloc(&cyc, 8 * 8 * blocks));
    CK(hipMemcpy(src, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    printf("== (b) KB = 13 loop, %d workgroups x 512 threads, %d sub-chunks each; floor 1248 cycles per sub-chunk and SIMD\n", blocks, iters);
    if (run_loop<0>("bare MFMAs, register operands", src, out, cyc, blocks, iters)) return 1;
    if (run_loop<1>("operands from LDS (product)", src, out, cyc, blocks, iters)) return 1;
    if (run_loop<2>("before: product + split of C and G^T + park", src, out, cyc, blocks, iters)) return 1;
    if (run_loop<3>("now: product + C cells copied, G^T split by 4 waves", src, out, cyc, blocks, iters)) return 1;
    if (run_loop<4>("not kept: C cells copied, G^T split by wave 6", src, out, cyc, blocks, iters)) return 1;

    // (c)
    using T = TileGradSplit<13>;
    std::vector<v8bf> hp((size_t)8 * T::CHUNK_CELLS);
    for (size_t i = 0; i < hp.size(); ++i)
        for (int k = 0; k < 8; ++k) hp[i][k] = (__bf16)hs[(8 * i + k) & 16383];
    v8bf *planes;
    CK(hipMalloc(&planes, hp.size() * sizeof(v8bf)));
    CK(hipMemcpy(planes, hp.data(), hp.size() * sizeof(v8bf), hipMemcpyHostToDevice));
    printf("== (c) KB = 13 gradient phase of the train tile, %d workgroups x 512 threads, %d chunks each, one barrier per chunk\n", blocks, iters);
    if (run_phase<0>("before: fp32, 104 MFMAs per wave", src, planes, out, cyc, blocks, iters)) return 1;
    if (run_phase<1>("three planes, corrections folded per chunk", src, planes, out, cyc, blocks, iters)) return 1;
    if (run_phase<2>("three planes, corrections in their own accumulator", src, planes, out, cyc, blocks, iters)) return 1;
    if (run_phase<3>("folded + next chunk's planes copied beside it", src, planes, out, cyc, blocks, iters)) return 1;
    if (run_phase<4>("own accumulator + next chunk's planes copied beside it", src, planes, out, cyc, blocks, iters)) return 1;

    // (d)
    printf("== (d) KB = 13 score phase of the train tile and both phases together, %d workgroups x 512 threads, %d chunks each\n", blocks, iters);
    double ns_fp32 = 0, ns_planes = 0, ns_both = 0, ns_grad = 0;
    if (run_score<0>("before: fp32 score loop, 2 x 50 MFMAs per wave", src, planes, out, cyc, blocks, iters, &ns_fp32)) return 1;
    if (run_score<1>("three planes, transposed reads: 84 MFMAs per wave", src, planes, out, cyc, blocks, iters, &ns_planes)) return 1;
    double ns_mid = 0, ns_halves = 0;
    if (run_score<2>("score + gradient phase, copy issued in front", src, planes, out, cyc, blocks, iters, &ns_both)) return 1;
    if (run_score<3>("score + gradient phase, copy issued between the phases", src, planes, out, cyc, blocks, iters, &ns_mid)) return 1;
    if (run_score<4>("score + gradient phase, copy half in front, half between", src, planes, out, cyc, blocks, iters, &ns_halves)) return 1;

    {   // the gradient loop of the kernel before, once more in this part's own run order
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        auto k = grad_phase_kernel<3>;
        const size_t shmem = (size_t)2 * T::CHUNK_CELLS * 16;
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(k, dim3(blocks), dim3(512), shmem, 0, src, planes, out, cyc, iters);
        CK(hipEventRecord(e1));
        CK(hipDeviceSynchronize());
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        ns_grad = ms * 1e6 / iters;
    }
    const double bar = 0.75 * (ns_fp32 + ns_grad);
    printf("gate: 0.75 x (fp32 score %.1f + folded gradient with copy %.1f) = %.1f ns/chunk; copy in front %.1f (%.3f), between %.1f (%.3f), "
           "halves %.1f (%.3f) of the sum -- single samples, compare several runs\n", ns_fp32, ns_grad, bar, ns_both,
           ns_both / (ns_fp32 + ns_grad), ns_mid, ns_mid / (ns_fp32 + ns_grad), ns_halves, ns_halves / (ns_fp32 + ns_grad));
    return 0;
}
