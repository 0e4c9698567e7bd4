// grid_pairs.h -- what the searches of ball_grid.hip, three_nn_grid.hip and knn.hip share: a PAIR of clouds per batch
// element, the reference cloud counting-sorted into the uniform grid of grid_common.h (cell side h) and the query cloud
// sorted along a Morton curve, so that the lanes of a wave walk neighbouring cells.
//   pair_layout        the workspace of such a pair
//   pair_build_launch  the one kernel that builds it (grid_pairs.hip)
#pragma once
#include "grid_common.h"

namespace pp {

// byte offsets into the workspace; every region starts 256-byte aligned
struct PairLayout {
  size_t sets, cell_start, sorted, qsorted, total;
};
__host__ __device__ inline PairLayout pair_layout(int B, int n_ref, int n_query) {
  PairLayout L;
  L.sets = 0;  // GridSet [2B]: the sets of the reference clouds, then the (unused) sets of the query sort
  L.cell_start = ((size_t)64 * 2 * B + 255) / 256 * 256;                                    // u32 [B][kGridCells + 1]
  L.sorted = L.cell_start + ((size_t)4 * (kGridCells + 1) * B + 255) / 256 * 256;           // f4 [B][n_ref]: x, y, z, index
  L.qsorted = L.sorted + ((size_t)16 * B * n_ref + 255) / 256 * 256;                        // f4 [B][n_query], likewise
  L.total = L.qsorted + (size_t)16 * B * n_query;
  return L;
}

// Builds both halves of every batch element's pair into ws (pair_layout(B, n_ref, n_query).total bytes): one launch.
// 0 on success, otherwise the hipError_t of the launch or of raising the kernel's LDS limit.
int pair_build_launch(const float* ref, const float* query, unsigned char* ws, int B, int n_ref, int n_query,
                      hipStream_t s);

}  // namespace pp
