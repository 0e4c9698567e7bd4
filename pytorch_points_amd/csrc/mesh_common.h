// mesh_common.h -- the one device layer of the six mesh files (mesh_edges.hip, mesh_dihedral.hip, mesh_normals.hip,
// mesh_sample.hip, mesh_distance.hip, mesh_winding.hip); bucket_lists.h itself knows nothing of meshes.  mesh_pair.h,
// beside it, is the pair function that the last two share.
//   sizes       mesh_build_ok (the builds' index words), mesh_sizes_ok (the steps' launches)
//   rows        mesh_half_edge, mesh_face (a face's three indices and whether all are in range), mesh_row (b, i, tb of
//               a (b,vertex) lane), mesh_slice (its clipped slice of a (N+1)-word start table)
//   V3          v3_*: the three-vector arithmetic of the step kernels, every operation rounded as written; the two dot
//               products are two functions because the tests compare their bits
//   item lists  mesh_item_lists: the bucket -> item lists of a call (the samples of a face, the faces of a point)
#pragma once
#include "bucket_lists.h"

namespace pp {

// the index words in use: u32 positions and codes within a batch element, int32 starts, 31-bit grids; `starts` for a
// build that writes every batch element's (N+1)-word start table
inline bool mesh_build_ok(int Bt, int N, long long items, bool starts) {
  return Bt >= 0 && N >= 0 && items >= 0 && (long long)Bt * items <= 0x7fffffffLL &&
         (long long)Bt * ((long long)N + (starts ? 1 : 0)) <= 0x7fffffffLL;
}

// the sizes a step entry checks: the (b,vertex), (b,face) and (b,item) rows of a launch, and the slot codes 3f + c,
// fit 31 bits; S is the entry's third count (samples, points), 0 where it has none
inline bool mesh_sizes_ok(int B, int N, int F, int S = 0) {
  return B >= 0 && N >= 0 && F >= 0 && S >= 0 && (long long)B * N <= 0x7fffffffLL && (long long)B * F <= 0x7fffffffLL &&
         (long long)B * S <= 0x7fffffffLL && 3LL * F <= 0x7fffffffLL;
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

// Face f of batch element b of faces (Bt,F,3), Bt = 1 when shared: its three indices, and whether all lie in [0, N).
// The caller has f in [0, F); an index out of range is only ever compared.
struct MeshFace {
  long long i0, i1, i2;
  bool in_range;
};
__device__ __forceinline__ MeshFace mesh_face(const long long* __restrict__ faces, long long b, long long f, int F,
                                              int N, int shared) {
  const long long* __restrict__ row = faces + ((shared ? 0 : b * F) + f) * 3;
  MeshFace t;
  t.i0 = row[0], t.i1 = row[1], t.i2 = row[2];
  t.in_range = !(t.i0 < 0 || t.i0 >= N || t.i1 < 0 || t.i1 >= N || t.i2 < 0 || t.i2 >= N);
  return t;
}

// Row r = b*N + i of a one-lane-per-(b,vertex) kernel, and tb, the batch element of its topology tables
struct MeshRow {
  long long b, i, tb;
};
__device__ __forceinline__ MeshRow mesh_row(long long r, int N, int shared) {
  MeshRow w;
  w.b = r / N;
  w.i = r - w.b * N;
  w.tb = shared ? 0 : w.b;
  return w;
}

// The slice [q0, q1) of row w in a (Bt,N+1) start table over lists of X entries per batch element, CLIPPED to the
// list, with the batch element's (next, prev) pairs and slot codes.  `codes` may be NULL; a caller without pairs passes
// NULL for `nbr` and does not touch s.nbr (a null test here, and likewise a second form without `nbr`, changes the
// registers of kernels that are otherwise the same).  The gathers over an edge incidence (me_sqrlen_backward_kernel,
// md_backward_kernel) and me_laplacian_apply_kernel read st[0], st[1] as they are and do not come through here.
struct MeshSlice {
  const int2* nbr;
  const unsigned* codes;
  int q0, q1;
};
__device__ __forceinline__ MeshSlice mesh_slice(const int* __restrict__ start, const int* __restrict__ nbr,
                                                const unsigned* __restrict__ codes, const MeshRow& w, int N,
                                                long long X) {
  const int* __restrict__ st = start + (size_t)w.tb * ((size_t)N + 1) + w.i;
  MeshSlice s;
  s.nbr = reinterpret_cast<const int2*>(nbr) + (size_t)w.tb * (size_t)X;
  s.codes = codes ? codes + (size_t)w.tb * (size_t)X : nullptr;
  const int a = st[0], b = st[1];
  s.q0 = a < 0 ? 0 : a;
  s.q1 = (long long)b > X ? (int)X : b;
  return s;
}

// ---- three-vectors -------------------------------------------------------------------------------------------------
// The library is built with -ffp-contract=off: every product, sum and quotient below is rounded on its own, and an fma
// is one only where it is written.
struct V3 {
  float x, y, z;
};
// (to pass a zero on; an accumulator starts from the written-out triple, which keeps its loop's packed instructions)
__device__ __forceinline__ V3 v3_zero() { return {0.0f, 0.0f, 0.0f}; }
__device__ __forceinline__ V3 v3_nan() { return {quiet_nan(), quiet_nan(), quiet_nan()}; }
__device__ __forceinline__ V3 v3_load(const float* __restrict__ p, long long i) {
  return {p[i * 3], p[i * 3 + 1], p[i * 3 + 2]};
}
__device__ __forceinline__ void v3_store(float* __restrict__ p, long long i, V3 v) {
  p[i * 3] = v.x;
  p[i * 3 + 1] = v.y;
  p[i * 3 + 2] = v.z;
}
__device__ __forceinline__ V3 v3_sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// a + b: `acc = v3_add(acc, term)` is the ordered sum of the gathers
__device__ __forceinline__ V3 v3_add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 v3_scale(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 v3_div(V3 a, float d) { return {a.x / d, a.y / d, a.z / d}; }
// fma(s, a, b) per component, one rounding each
__device__ __forceinline__ V3 v3_fma(float s, V3 a, V3 b) {
  return {__builtin_fmaf(s, a.x, b.x), __builtin_fmaf(s, a.y, b.y), __builtin_fmaf(s, a.z, b.z)};
}
// (w0 a + w1 b) + w2 c: three products and two sums per component
__device__ __forceinline__ V3 v3_weighted(float w0, V3 a, float w1, V3 b, float w2, V3 c) {
  return v3_add(v3_add(v3_scale(w0, a), v3_scale(w1, b)), v3_scale(w2, c));
}
// a*b - c*d within 1.5 ulp (Kahan): the rounding error of c*d is recovered by one fma and added back
__device__ __forceinline__ float v3_dop(float a, float b, float c, float d) {
  const float w = c * d;
  const float e = __builtin_fmaf(-c, d, w);
  const float f = __builtin_fmaf(a, b, -w);
  return f + e;
}
__device__ __forceinline__ V3 v3_cross(V3 a, V3 b) {
  return {v3_dop(a.y, b.z, a.z, b.y), v3_dop(a.z, b.x, a.x, b.z), v3_dop(a.x, b.y, a.y, b.x)};
}
// The two dot products differ in their last bits and are not interchangeable.
// fma(az, bz, fma(ay, by, ax*bx)): one product and two fused steps, three roundings (the dihedral chain, the
// projections of mesh_normals.hip); symmetric in a and b
__device__ __forceinline__ float v3_dot_fused(V3 a, V3 b) {
  return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));
}
// (ax bx + ay by) + az bz: three products and two sums, five roundings (torch's sum of products: the lengths of
// mesh_normals.hip and the cotangent, every dot product and residual of mesh_distance.hip)
__device__ __forceinline__ float v3_dot_rounded(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// sqrtf of the five-rounding square
__device__ __forceinline__ float v3_len(V3 a) { return sqrtf(v3_dot_rounded(a, a)); }

// ---- item lists ----------------------------------------------------------------------------------------------------
// Item x of batch element b (S per element) belongs to bucket item[b,x] of K.  FILL = false: the buckets' sizes;
// FILL = true: the lists.  An item whose bucket is outside [0, K) is only compared and takes no part.
template <bool FILL>
__global__ __launch_bounds__(kBucketThreads) void mesh_item_lists_kernel(const long long* __restrict__ item,
                                                                         unsigned* __restrict__ cursor,
                                                                         unsigned* __restrict__ entries,
                                                                         long long total, int K, int S) {
  const long long x = (long long)blockIdx.x * kBucketThreads + threadIdx.x;
  if (x >= total) return;
  const long long k = item[x];
  if (k < 0 || k >= K) return;
  const long long b = x / S;
  bucket_put<FILL>(cursor, entries, b, K, (long long)S, (size_t)k, (unsigned)(x - b * S));
}

// the sorted lists of item (B,S) over B*K buckets, in the scratch ws laid out by L = bucket_layout(B, K, S, false)
inline int mesh_item_lists(const long long* item, int B, int K, int S, const BucketLayout& L, unsigned char* ws,
                           hipStream_t s) {
  unsigned* cursor = reinterpret_cast<unsigned*>(ws + L.cursor);
  unsigned* entries = reinterpret_cast<unsigned*>(ws + L.entries);
  const long long total = (long long)B * S;
  return bucket_build(ws, L, entries, nullptr, B, K, S, true, s, [&](bool fill) {
    const dim3 grid(blocks(total, kBucketThreads)), block(kBucketThreads);
    if (fill)
      mesh_item_lists_kernel<true><<<grid, block, 0, s>>>(item, cursor, entries, total, K, S);
    else
      mesh_item_lists_kernel<false><<<grid, block, 0, s>>>(item, cursor, entries, total, K, S);
  });
}

}  // namespace pp
