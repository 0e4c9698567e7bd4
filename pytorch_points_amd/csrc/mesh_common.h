// mesh_common.h -- what the topology builds of mesh_edges.hip and mesh_dihedral.hip share (bucket_lists.h itself knows
// nothing of meshes), and the three-vector arithmetic of the step kernels of mesh_dihedral.hip and mesh_normals.hip.
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

// ---- three-vectors of the step kernels (mesh_dihedral.hip, mesh_normals.hip) ------------------------------------------
struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 md_load(const float* __restrict__ vb, long long i) {
  return {vb[i * 3], vb[i * 3 + 1], vb[i * 3 + 2]};
}
__device__ __forceinline__ V3 md_sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// a*b - c*d within 1.5 ulp (Kahan): the rounding error of c*d is recovered by one fma and added back
__device__ __forceinline__ float md_dop(float a, float b, float c, float d) {
  const float w = c * d;
  const float e = __builtin_fmaf(-c, d, w);
  const float f = __builtin_fmaf(a, b, -w);
  return f + e;
}
__device__ __forceinline__ V3 md_cross(V3 a, V3 b) {
  return {md_dop(a.y, b.z, a.z, b.y), md_dop(a.z, b.x, a.x, b.z), md_dop(a.x, b.y, a.y, b.x)};
}
__device__ __forceinline__ float md_dot(V3 a, V3 b) {
  return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));   // symmetric in a and b
}

}  // namespace pp
