// mesh_common.h -- what the topology builds of mesh_edges.hip and mesh_dihedral.hip share (bucket_lists.h itself knows
// nothing of meshes).
#pragma once
#include "bucket_lists.h"

namespace pp {

// the index words in use: u32 positions and codes within a batch element, int32 starts, 31-bit grids; `starts` for a
// build that writes every batch element's (N+1)-word start table
inline bool mesh_build_ok(int Bt, int N, long long items, bool starts) {
  return Bt >= 0 && N >= 0 && items >= 0 && (long long)Bt * items <= 0x7fffffffLL &&
         (long long)Bt * ((long long)N + (starts ? 1 : 0)) <= 0x7fffffffLL;
}

// Half-edge h = 3*f + j of faces (Bt,F,3), f the face number over the whole batch, joins corners j and (j+1) mod 3:
// its batch element and its vertex pair as (min, max).  One with a vertex outside [0, N) is only ever compared.
struct MeshHalfEdge {
  long long b, mn, mx;
  bool in_range;
};
__device__ __forceinline__ MeshHalfEdge mesh_half_edge(const long long* __restrict__ faces, long long h, int F, int N) {
  const long long f = h / 3;
  const int j = (int)(h - f * 3);
  const long long p = faces[f * 3 + j], q = faces[f * 3 + (j == 2 ? 0 : j + 1)];
  MeshHalfEdge e;
  e.b = h / (3LL * F);
  e.mn = p < q ? p : q;
  e.mx = p < q ? q : p;
  e.in_range = !(p < 0 || p >= N || q < 0 || q >= N);
  return e;
}

}  // namespace pp
