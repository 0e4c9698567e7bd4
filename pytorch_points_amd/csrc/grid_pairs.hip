// grid_pairs.hip -- the build of grid_pairs.h's workspace, for ball_grid.hip, three_nn_grid.hip and knn.hip: every
// batch element's reference cloud into its grid, its query cloud into Morton order, in one launch.
#include "grid_pairs.h"

namespace {

using pp::kBuildSlabs;
using pp::kBuildThreads;
using pp::kGridCells;

// workgroups [0, S*B): slab s of the reference cloud of batch element b into its grid; [S*B, 2*S*B): slab s of the
// queries of batch element b into Morton order (S = kBuildSlabs)
template <bool VEC>
__global__ __launch_bounds__(kBuildThreads) void pair_build_kernel(const float* __restrict__ ref,
                                                                   const float* __restrict__ query,
                                                                   unsigned char* __restrict__ ws, int B, int n_ref,
                                                                   int n_query) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_cnt[];
  const pp::PairLayout L = pp::pair_layout(B, n_ref, n_query);
  // both sets of a batch element are built on the XCD that will search it (the query kernels' batch ->
  // XCD mapping): virtual order (batch, cloud | queries, slab)
  const int V = pp::xcd_virtual_block(blockIdx.x, (2 * B * kBuildSlabs + 7) / 8);
  if (V >= 2 * B * kBuildSlabs) return;
  const int slab = V % kBuildSlabs;
  const int set = ((V / kBuildSlabs) & 1) * B + V / (2 * kBuildSlabs);
  pp::GridSet* gs = reinterpret_cast<pp::GridSet*>(ws + L.sets) + set;
  if (set >= B) {
    const int b = set - B;
    pp::grid_build_set<true, VEC>(query + (size_t)b * n_query * 3, n_query, gs, nullptr,
                                  reinterpret_cast<pp::f4*>(ws + L.qsorted) + (size_t)b * n_query, nullptr, s_cnt,
                                  nullptr, nullptr, slab, kBuildSlabs);
    return;
  }
  const int b = set;
  pp::grid_build_set_plain<VEC>(ref + (size_t)b * n_ref * 3, n_ref, gs,
                                reinterpret_cast<unsigned*>(ws + L.cell_start) + (size_t)b * (kGridCells + 1),
                                reinterpret_cast<pp::f4*>(ws + L.sorted) + (size_t)b * n_ref, s_cnt, slab, kBuildSlabs);
}

}  // namespace

int pp::pair_build_launch(const float* ref, const float* query, unsigned char* ws, int B, int n_ref, int n_query,
                          hipStream_t s) {
  const size_t lds = grid_build_lds_bytes(kBuildSlabs) > grid_build_fast_lds_bytes() ? grid_build_lds_bytes(kBuildSlabs)
                                                                                     : grid_build_fast_lds_bytes();
  // (two kernels: with both load paths inlined into one the register allocator spills -- grid_common.h)
  static DeviceFlags lds_ok, lds_ok_vec;
  const bool vec = clouds_vec_aligned(ref, n_ref, B) && clouds_vec_aligned(query, n_query, B);
  const hipError_t e = vec ? allow_big_lds(pair_build_kernel<true>, (int)lds, lds_ok_vec)
                           : allow_big_lds(pair_build_kernel<false>, (int)lds, lds_ok);
  if (e != hipSuccess) return (int)e;
  (vec ? pair_build_kernel<true> : pair_build_kernel<false>)<<<dim3(8 * ((2 * B * kBuildSlabs + 7) / 8)),
                                                               dim3(kBuildThreads), lds, s>>>(ref, query, ws, B, n_ref,
                                                                                               n_query);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}
