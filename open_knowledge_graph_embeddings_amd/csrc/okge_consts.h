// Tile constants shared by the kernels, their launchers and the host-side planner (okge_plan.h).  No HIP header: this file
// compiles as plain C++.
#pragma once

namespace okge {

constexpr int NT = 64;             // candidate rows per tile
constexpr int BC = 64;             // batch rows per chunk
// 16-byte cells of the three bf16 planes of one 64-candidate tile of D16 columns (layout: okge_dq_split.h)
constexpr int plane_cells_per_tile(int D16) { return 3 * NT * D16 / 8; }
// the instances of fused_tile64_kernel whose gradient product dC = G^T . Q runs on the bf16 matrix cores, from three bf16 planes
// of Q made once per step (okge_tile_grad_split.h)
constexpr bool tile_grad_split(int KB) { return KB == 13; }

// Padded leading dimension (floats) of an LDS tile whose rows hold D16 floats: D16 + 4 = 4 * odd, so
// (a) ds_read_b128 of 16 different rows at one column lands on 16 different 16-byte slots and
// (b) ds_read_b32 of rows r and r+4 at 16 consecutive columns lands on disjoint bank halves.
#ifdef __HIPCC__
__host__ __device__
#endif
constexpr int lds_ld(int D16) { return D16 + 4; }

}  // namespace okge
