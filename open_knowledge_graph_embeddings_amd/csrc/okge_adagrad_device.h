// The Adagrad element update (utils/optim.py:139-160 / torch.optim.Adagrad), stated once for every kernel that applies it:
//     g += wd * p;  s += g * g;  p -= lr * g / (sqrt(s) + eps)
// bit-identical across the eager sweeps (okge_optim.hip), the deferred replay (lazy_rows: okge_optim.hip, okge_pool.hip,
// okge_sparse.hip) and the row-sparse update (okge_sparse.hip).  Included by those three units only.
#pragma once
#include "okge_device.h"

namespace okge {

__device__ __forceinline__ bool bits_differ(const float4 &a, const float4 &b)
{
    return ((__float_as_uint(a.x) ^ __float_as_uint(b.x)) | (__float_as_uint(a.y) ^ __float_as_uint(b.y)) |
            (__float_as_uint(a.z) ^ __float_as_uint(b.z)) | (__float_as_uint(a.w) ^ __float_as_uint(b.w))) != 0u;
}

__device__ __forceinline__ bool any_bits(const float4 &v)
{
    return (__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z) | __float_as_uint(v.w)) != 0u;
}

__device__ __forceinline__ void adagrad4(float4 &pv, const float4 &gv, float4 &sv, float lr, float wd, float eps)
{
    float *pp = &pv.x, *ss = &sv.x;
    const float *gg = &gv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float gj = fmaf(wd, pp[j], gg[j]);
        ss[j] = fmaf(gj, gj, ss[j]);
        pp[j] = pp[j] - lr * (gj / (sqrtf(ss[j]) + eps));
    }
}

// the scalar twin, in place on one element (the < 4 elements behind a tensor's last float4; tensors swept element by element)
__device__ __forceinline__ void adagrad1(float &p, float &g, float &s, float lr, float wd, float eps, bool zero_grad)
{
    const float gj = fmaf(wd, p, g);
    s = fmaf(gj, gj, s);
    p = p - lr * (gj / (sqrtf(s) + eps));
    if (zero_grad) g = 0.f;
}

// The row-sparse update (torch's sparse Adagrad: no weight decay).  NOT adagrad1 at wd = 0: fmaf(0, p, g) is not g for
// g = -0.0f (it gives +0.0f) or for a non-finite p (it gives NaN) -- the decay term is absent here, not multiplied by zero.
__device__ __forceinline__ void adagrad1_rows(float &p, float g, float &s, float lr, float eps)
{
    s = fmaf(g, g, s);
    p = p - lr * (g / (sqrtf(s) + eps));
}

// Store only what changed.  A row no gradient reached still moves by the weight-decay term (the reference applies wd = 1e-10
// to ALL rows) -- but once its accumulator has seen a real gradient, that term is below half an ulp of both the accumulator and
// the parameter and the update returns the old bits: such rows (most token rows of a token-pooled step, the entities outside a
// sampled candidate list) then cost three read streams instead of three reads + two writes.  Likewise `clear` (zero_grad) clears
// only a gradient that is not clear already: one store stream less for the same rows, a sixth of the HBM-bound sweep.  Memory
// ends up bit-identical to the unconditional stores.
// Element i of p4 / s4 / g4; pv / sv: the updated values, p_old / s_old / gv: what was loaded.
__device__ __forceinline__ void adagrad_commit4(float4 *p4, float4 *s4, float4 *g4, size_t i, const float4 &pv, const float4 &p_old,
                                                const float4 &sv, const float4 &s_old, const float4 &gv, bool clear)
{
    if (bits_differ(pv, p_old)) p4[i] = pv;
    if (bits_differ(sv, s_old)) s4[i] = sv;
    if (clear && any_bits(gv)) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- decay-only steps on operands known to be ordinary numbers --------------------------------------------------------------
// The compiler's correctly rounded `sqrtf` and `/` spend a third of their instructions on operands that cannot occur here
// (denormal / huge / zero / infinite: `v_div_scale` x2 + `v_div_fixup`, the 2^32 scaling and class test around `v_sqrt_f32`), and
// none of their fix-up arithmetic is packed.  The replay of deferred steps is bound by exactly this arithmetic, so it
// runs the SAME sequences -- `v_sqrt_f32` + the two neighbour tests; `v_rcp_f32` + the Newton step on the reciprocal + two
// residual corrections of the quotient -- on two elements at a time (`v_pk_fma_f32`), without the branches for operands outside
//     sqrt:  2^-96 <= x < inf                    (below: scaled by 2^32 first;  v_cmp_gt 0x0f800000 in the generic code)
//     a / b: a, b != 0, b and 1/b and a/b normal, exponent(a) - exponent(b) < 96, |a| >= 2^-103      (V_DIV_SCALE_F32 leaves
//            both operands as they are and VCC = 0; V_DIV_FMAS_F32 is then a plain fma and V_DIV_FIXUP_F32 returns its operand)
// Inside that range the result is the generic one bit for bit (the same instructions on the same values);
// tests/test_token_pooled.py::test_fast_decay_arithmetic_is_the_generic_one compares the two over twelve orders of magnitude.
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v fma2(f2v a, f2v b, f2v c) { return __builtin_elementwise_fma(a, b, c); }

__device__ __forceinline__ f2v sqrt_rn_ordinary2(f2v x)
{
    f2v y, dn, up;
    y.x = __builtin_amdgcn_sqrtf(x.x);
    y.y = __builtin_amdgcn_sqrtf(x.y);
    dn.x = __int_as_float(__float_as_int(y.x) - 1);
    dn.y = __int_as_float(__float_as_int(y.y) - 1);
    up.x = __int_as_float(__float_as_int(y.x) + 1);
    up.y = __int_as_float(__float_as_int(y.y) + 1);
    const f2v e_dn = fma2(-dn, y, x), e_up = fma2(-up, y, x);
    f2v r;
    r.x = 0.f >= e_dn.x ? dn.x : y.x;
    r.y = 0.f >= e_dn.y ? dn.y : y.y;
    r.x = 0.f < e_up.x ? up.x : r.x;
    r.y = 0.f < e_up.y ? up.y : r.y;
    return r;
}

__device__ __forceinline__ f2v div_rn_ordinary2(f2v a, f2v b)
{
    f2v r0;
    r0.x = __builtin_amdgcn_rcpf(b.x);
    r0.y = __builtin_amdgcn_rcpf(b.y);
    const f2v one = {1.f, 1.f};
    const f2v r = fma2(fma2(-b, r0, one), r0, r0);
    f2v q = a * r;
    q = fma2(fma2(-b, q, a), r, q);
    q = fma2(fma2(-b, q, a), r, q);
    return q;
}

// may `n` decay-only steps from (p, s) take the sequences above?  Bounds with room for n <= 64 steps of drift (|p| moves by at
// most lr * wd / eps <= 1/16 of itself per step, s grows by g^2 <= 2^20 per step); the parameters' own ranges are checked once
__device__ __forceinline__ bool decay_params_ordinary(float lr, float wd, float eps)
{
    return wd >= 0x1p-40f && wd <= 0x1p-10f && eps >= 0x1p-40f && eps <= 1.f && lr > 0.f && lr <= 16.f && lr * wd <= 0x1p-4f * eps;
}
__device__ __forceinline__ bool decay_operands_ordinary(const float4 &pv, const float4 &sv)
{
    const float *pp = &pv.x, *ss = &sv.x;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j)          // (unsigned compares of the bit patterns: one subtract + one compare per bound pair)
        ok = ok && (__float_as_uint(fabsf(pp[j])) - 0x26800000u) <= (0x49800000u - 0x26800000u)      // 2^-50 <= |p| <= 2^20
                && (__float_as_uint(ss[j]) - 0x0f800000u) <= (0x53800000u - 0x0f800000u);              // 2^-96 <= s <= 2^40
    return ok;
}

__device__ __forceinline__ void decay_step4_ordinary(float4 &pv, float4 &sv, float lr, float wd, float eps)
{
    const f2v wd2 = {wd, wd}, eps2 = {eps, eps}, nlr2 = {-lr, -lr}, zero2 = {0.f, 0.f};
    f2v p01 = {pv.x, pv.y}, p23 = {pv.z, pv.w}, s01 = {sv.x, sv.y}, s23 = {sv.z, sv.w};
    const f2v g01 = fma2(wd2, p01, zero2), g23 = fma2(wd2, p23, zero2);
    s01 = fma2(g01, g01, s01);
    s23 = fma2(g23, g23, s23);
    p01 = fma2(nlr2, div_rn_ordinary2(g01, sqrt_rn_ordinary2(s01) + eps2), p01);
    p23 = fma2(nlr2, div_rn_ordinary2(g23, sqrt_rn_ordinary2(s23) + eps2), p23);
    pv = make_float4(p01.x, p01.y, p23.x, p23.y);
    sv = make_float4(s01.x, s01.y, s23.x, s23.y);
}

// `n` consecutive updates of a row no gradient reached (g = 0: the weight-decay term alone, okge_adagrad_lazy): the same
// arithmetic as n sweeps, one after the other.  If the first step returns the bits it was given on every active lane of the wave
// (warm accumulators: wd * p is below half an ulp of both), all later ones do too and are skipped.  `ordinary` (wave-uniform):
// every active lane's operands allow the short sequences above.
__device__ __forceinline__ void decay_replay4(float4 &pv, float4 &sv, int n, float lr, float wd, float eps)
{
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n <= 0) return;
    const bool ordinary = n <= 64 && decay_params_ordinary(lr, wd, eps) && !__any(!decay_operands_ordinary(pv, sv));
    const float4 p0 = pv, s0 = sv;
    if (ordinary) decay_step4_ordinary(pv, sv, lr, wd, eps);
    else adagrad4(pv, zero, sv, lr, wd, eps);
    if (!__any(bits_differ(pv, p0) || bits_differ(sv, s0))) return;      // (checked once: a row that moves keeps moving)
    if (ordinary) {
        for (int i = 1; i < n; ++i) decay_step4_ordinary(pv, sv, lr, wd, eps);
    } else {
        for (int i = 1; i < n; ++i) adagrad4(pv, zero, sv, lr, wd, eps);
    }
}

// The rows a wave owes work on, one after the other with the NEXT row's loads in flight while the current one is replayed
// (a row is a dependent chain: counters -> row loads -> up to `window` correctly rounded sqrt / div steps -> stores; one row at a
// time left the wave waiting on HBM for most of its life).  Lane-held description of the wave's 64 candidate rows: `mask` (bit j:
// lane j's row needs work), row index, pending decay-only steps, and whether the step with the gradient follows.  Rows of up to
// 256 floats (lane = column quad); longer rows go through the plain column loop.
__device__ __forceinline__ void lazy_rows(uint64_t mask, int64_t row, int n_decay, bool with_grad, float *__restrict__ p,
                                          float *__restrict__ s, float *__restrict__ g, int row_len, int lane, float lr, float wd,
                                          float eps)
{
    const int row4 = row_len >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(p), *s4 = reinterpret_cast<float4 *>(s), *g4 = reinterpret_cast<float4 *>(g);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row4 > 64) {
        while (mask) {
            const int j = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            const size_t base = (size_t)__shfl(row, j) * row4;
            const int n = __shfl(n_decay, j);
            const bool wg = __shfl((int)with_grad, j) != 0;
            for (int c = lane; c < row4; c += 64) {
                const size_t i = base + c;
                float4 pv = p4[i], sv = s4[i], gv = wg ? g4[i] : zero;
                const float4 p0 = pv, s0 = sv;
                decay_replay4(pv, sv, n, lr, wd, eps);
                if (wg) adagrad4(pv, gv, sv, lr, wd, eps);
                adagrad_commit4(p4, s4, g4, i, pv, p0, sv, s0, gv, wg);
            }
        }
        return;
    }
    const bool act = lane < row4;
    int j = mask ? __ffsll((unsigned long long)mask) - 1 : -1;
    if (j >= 0) mask &= mask - 1;
    size_t base = 0;
    int n = 0;
    bool wg = false;
    float4 pv = zero, sv = zero, gv = zero;
    if (j >= 0) {
        base = (size_t)__shfl(row, j) * row4 + lane;
        n = __shfl(n_decay, j);
        wg = __shfl((int)with_grad, j) != 0;
        if (act) { pv = p4[base]; sv = s4[base]; if (wg) gv = g4[base]; }
    }
    while (j >= 0) {
        const int jn = mask ? __ffsll((unsigned long long)mask) - 1 : -1;
        if (jn >= 0) mask &= mask - 1;
        size_t base_n = 0;
        int n_n = 0;
        bool wg_n = false;
        float4 pn = zero, sn = zero, gn = zero;
        if (jn >= 0) {                                   // the next row's loads leave before this row's arithmetic starts
            base_n = (size_t)__shfl(row, jn) * row4 + lane;
            n_n = __shfl(n_decay, jn);
            wg_n = __shfl((int)with_grad, jn) != 0;
            if (act) { pn = p4[base_n]; sn = s4[base_n]; if (wg_n) gn = g4[base_n]; }
        }
        if (act) {
            const float4 p0 = pv, s0 = sv;
            decay_replay4(pv, sv, n, lr, wd, eps);
            if (wg) adagrad4(pv, gv, sv, lr, wd, eps);
            adagrad_commit4(p4, s4, g4, base, pv, p0, sv, s0, gv, wg);
        }
        j = jn; base = base_n; n = n_n; wg = wg_n; pv = pn; sv = sn; gv = gn;
    }
}

}  // namespace okge
