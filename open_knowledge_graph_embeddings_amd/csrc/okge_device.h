// Device-side helpers shared by the gfx950 kernels of the open-KGE hot path.
// gfx950 only: 64-wide wavefronts, v_mfma_f32_16x16x4_f32 (exact fp32 matrix FMA), 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "okge_consts.h"      // NT, BC, lds_ld, ...

namespace okge {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));   // one 16-byte cell of a bf16 plane (okge_dq_split.h)

constexpr int WAVE = 64;

// ---- dropout description as the kernels see it (host fills it from okge_dropout) -----------------
struct DropDev {
    const uint8_t *keep;   // explicit keep mask [rows][d] or nullptr
    float          scale;  // 1/(1-p)   (1 when disabled)
    uint32_t       thr;    // keep <=> 16-bit philox number >= thr (= floor(p * 65536))
    uint32_t       k0, k1; // philox key = seed
    uint32_t       stream, step;
    int32_t        enabled;
    const uint32_t *step_dev;   // device-resident step counter (graph replay) or nullptr
};

__device__ __forceinline__ uint32_t drop_step(const DropDev &dr) { return dr.step_dev ? *dr.step_dev : dr.step; }

// ---- Philox4x32-10 (Salmon et al. 2011), Random123 known-answer vectors in tests/ -------------------
// WIDE: one 32 x 32 -> 64 multiply per product (v_mad_u64_u32) instead of a v_mul_hi / v_mul_lo pair -- the integer
// multiplies are quarter-rate and set the cost of a round; same numbers.  (The tile kernels use it; hipcc 7.2 fails to
// select instructions for some of the small kernels of okge_misc.hip with it, so it is opt-in.)
template <bool WIDE = false>
__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        if (WIDE) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
            hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
            hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        } else {
            hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
            hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        }
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// Keep flags (bit e = column 8*o8 + e) of eight consecutive columns of row `row_pos` of a gathered block with
// `d` columns.  One Philox call yields 8 uniform 16-bit numbers: word e>>1, low half for even e, high half
// for odd e; keep <=> u16 >= thr (thr = floor(p * 65536)).  Columns >= d report "drop".
// (`step` = drop_step(dr), fetched once by the caller: with a device-resident counter it is a load, and a load between a
//  kernel's gather and its mask arithmetic makes the arithmetic wait for the gather -- vmcnt retires in order)
template <bool WIDE = false>
__device__ __forceinline__ uint32_t drop_keep8(const DropDev &dr, uint32_t row_pos, int o8, int d, uint32_t step)
{
    uint32_t bits = 0;
    if (dr.keep) {
        const uint8_t *kp = dr.keep + (size_t)row_pos * d + 8 * o8;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (8 * o8 + e < d && kp[e]) bits |= 1u << e;
        return bits;
    }
    const uint4 u = philox4x32_10<WIDE>(row_pos, (uint32_t)o8, dr.stream, step, dr.k0, dr.k1);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t u16 = (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
        if (u16 >= dr.thr && 8 * o8 + e < d) bits |= 1u << e;
    }
    return bits;
}

__device__ __forceinline__ uint32_t drop_keep8(const DropDev &dr, uint32_t row_pos, int o8, int d)
{
    return drop_keep8(dr, row_pos, o8, d, drop_step(dr));
}

__device__ __forceinline__ float drop_mult1(const DropDev &dr, uint32_t row_pos, int k, int d)
{
    if (!dr.enabled) return 1.f;
    if (dr.keep) return dr.keep[(size_t)row_pos * d + k] ? dr.scale : 0.f;
    const uint4 u = philox4x32_10(row_pos, (uint32_t)(k >> 3), dr.stream, drop_step(dr), dr.k0, dr.k1);
    const int e = k & 7;
    const uint32_t w = (e >> 1) == 0 ? u.x : (e >> 1) == 1 ? u.y : (e >> 1) == 2 ? u.z : u.w;
    return ((w >> (16 * (e & 1))) & 0xFFFFu) >= dr.thr ? dr.scale : 0.f;
}

// v *= (keep ? scale : 0) for the 4 columns selected by bits (nibble already shifted down)
__device__ __forceinline__ void apply_keep4(float4 &v, uint32_t nibble, float scale)
{
    v.x *= (nibble & 1u) ? scale : 0.f;
    v.y *= (nibble & 2u) ? scale : 0.f;
    v.z *= (nibble & 4u) ? scale : 0.f;
    v.w *= (nibble & 8u) ? scale : 0.f;
}

// D(16x16) += A(16x4) * B(4x16), exact fp32.  Lane l supplies A[l&15][l>>4] and B[l>>4][l&15];
// result register i of lane l is D[4*(l>>4)+i][l&15].
__device__ __forceinline__ v4f mfma16(float a, float b, v4f c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Ids live in device memory and are trusted for speed, but never for safety: a row index outside its table is replaced
// by row 0 (the padding row every table has) and counted in a device word the host reads lazily (okge_id_errors).
__device__ __forceinline__ int64_t checked_row(int64_t id, int64_t n_rows, int *err)
{
    if ((uint64_t)id >= (uint64_t)n_rows) {
        if (err) atomicAdd(err, 1);
        return 0;
    }
    return id;
}

// Reductions over the 16 lanes of a DPP row (lanes 16s .. 16s+15) with DPP moves instead of ds_bpermute shuffles: quad
// swaps (xor 1, xor 2), then row_half_mirror and row_mirror -- after the quad steps all four lanes of a quad agree, so
// the mirrors pair every quad with the one it still misses.  All 16 lanes end up with the result.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_max(float v)
{
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    return v;
}
__device__ __forceinline__ float row16_sum(float v)
{
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int lower_bound_i32(const int32_t *__restrict__ a, int n, int key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace okge
