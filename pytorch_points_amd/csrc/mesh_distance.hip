// mesh_distance.hip -- the exact squared distance between a point cloud and a triangle mesh, in both directions, by
// walking every (point, triangle) pair.  The seventh mesh operator; contract in DESIGN.md "Point-to-mesh distances".
//
//   records      one lane per (b, face): the face's corners a, b, c, its edges ab = b - a and ac = c - a and a validity
//                word, 16 floats, so that the pair loops gather nothing and check no index
//   point->face  one lane per point, a workgroup within one batch element; the records come through LDS in tiles of
//                kPdFaceTile, in ascending order; the record of a step is the same for every lane (an LDS broadcast)
//   face->point  one lane per face with its record in registers; the points of the batch element come through LDS in
//                tiles of kPdPointTile, in ascending order
//   Both keep (best, index, weights) from (+inf, -1, NaN) and take a pair where d < best: the lowest index among equal
//   distances, never a NaN, never a face with a vertex index outside [0, N).
//   backward     one lane per item: r = p - q with q interpolated again, (2 g) r and its negative; for face->point the
//                point -> face lists of the call (pp::mesh_item_lists: buckets the B*P points, items the faces,
//                sorted) and per point the sum of its faces' vectors in ascending order.  The vertices' gradient is
//                pp_mesh_sample_backward_f32's on the negated vectors.
//
// pd_pair is the one pair function: Ericson's region walk with every operation rounded on its own, in the operation
// order of mesh_distance.distance_composition, which it equals to the bit.
//
// No floating-point atomics: every output word is written once and the bits are the same on every run.  An index of
// `faces` outside [0, N), and in the backward a face outside [0, F) or a point outside [0, P), are only compared,
// never used as an address.
#include "mesh_common.h"   // pp::mesh_face, mesh_item_lists, mesh_sizes_ok, V3 and v3_*; pp::blocks, pp::quiet_nan
#include "mesh_pair.h"     // pp::PdTri, PdPair, pd_pair, pd_unpack (shared with mesh_winding.hip)

namespace {

using namespace pp;   // mesh_common.h's rows, three-vectors and item lists; every dot product is v3_dot_rounded

constexpr int kPdThreads = 256;
constexpr int kPdRecord = 16;         // floats of a face record: a, b, c, ab, ac, valid
constexpr int kPdFaceTile = 256;      // records in LDS: 16 KB
constexpr int kPdPointTile = 1024;    // points in LDS: 12 KB

// ---- records --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPdThreads) void pd_records_kernel(const float* __restrict__ vertices,
                                                                const long long* __restrict__ faces,
                                                                float4* __restrict__ records, long long rows, int N,
                                                                int F, int shared) {
  const long long x = (long long)blockIdx.x * kPdThreads + threadIdx.x;
  if (x >= rows) return;
  const long long b = x / F;
  const MeshFace t = mesh_face(faces, b, x - b * F, F, N, shared);
  float4 w0 = {0.0f, 0.0f, 0.0f, 0.0f}, w1 = w0, w2 = w0, w3 = w0;
  if (t.in_range) {
    const float* __restrict__ vb = vertices + (size_t)b * N * 3;
    const V3 a = v3_load(vb, t.i0), c1 = v3_load(vb, t.i1), c2 = v3_load(vb, t.i2);
    const V3 ab = v3_sub(c1, a), ac = v3_sub(c2, a);
    w0 = {a.x, a.y, a.z, c1.x};
    w1 = {c1.y, c1.z, c2.x, c2.y};
    w2 = {c2.z, ab.x, ab.y, ab.z};
    w3 = {ac.x, ac.y, ac.z, 1.0f};
  }
  float4* __restrict__ out = records + (size_t)x * (kPdRecord / 4);
  out[0] = w0;
  out[1] = w1;
  out[2] = w2;
  out[3] = w3;
}

// ---- forward --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pd_store(float* __restrict__ dist, long long* __restrict__ index,
                                         float* __restrict__ bary, size_t x, float best, int arg, float w0, float w1,
                                         float w2) {
  dist[x] = arg < 0 ? pp::quiet_nan() : best;
  index[x] = arg;
  v3_store(bary, x, {w0, w1, w2});
}

__global__ __launch_bounds__(kPdThreads) void pd_point_face_kernel(const float* __restrict__ points,
                                                                   const float4* __restrict__ records,
                                                                   float* __restrict__ dist,
                                                                   long long* __restrict__ face,
                                                                   float* __restrict__ bary, int P, int F,
                                                                   int blocks_per_element) {
  __shared__ float4 s_rec[kPdFaceTile * (kPdRecord / 4)];
  const int t = threadIdx.x;
  const long long b = blockIdx.x / blocks_per_element;
  const long long i = (long long)(blockIdx.x - (unsigned)b * blocks_per_element) * kPdThreads + t;
  const bool live = i < P;
  V3 p = {0.0f, 0.0f, 0.0f};
  if (live) p = v3_load(points + (size_t)b * P * 3, i);
  const float4* __restrict__ rb = records + (size_t)b * F * (kPdRecord / 4);
  float best = __builtin_inff();
  int arg = -1;
  float w0 = pp::quiet_nan(), w1 = w0, w2 = w0;
  for (int f0 = 0; f0 < F; f0 += kPdFaceTile) {
    const int n = F - f0 < kPdFaceTile ? F - f0 : kPdFaceTile;
    __syncthreads();   // the previous tile's readers are done
    for (int k = t; k < n * (kPdRecord / 4); k += kPdThreads) s_rec[k] = rb[(size_t)f0 * (kPdRecord / 4) + k];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const float4 q3 = s_rec[j * 4 + 3];
      if (q3.w == 0.0f) continue;   // (the whole workgroup) a face with a vertex index out of range
      const PdTri tri = pd_unpack(s_rec[j * 4], s_rec[j * 4 + 1], s_rec[j * 4 + 2], q3);
      const PdPair r = pd_pair(p, tri);
      if (r.d < best) {
        best = r.d;
        arg = f0 + j;
        w0 = r.w0, w1 = r.w1, w2 = r.w2;
      }
    }
  }
  if (live) pd_store(dist, face, bary, (size_t)b * P + i, best, arg, w0, w1, w2);
}

__global__ __launch_bounds__(kPdThreads) void pd_face_point_kernel(const float* __restrict__ points,
                                                                   const float4* __restrict__ records,
                                                                   float* __restrict__ dist,
                                                                   long long* __restrict__ point,
                                                                   float* __restrict__ bary, int P, int F,
                                                                   int blocks_per_element) {
  __shared__ float s_pt[kPdPointTile * 3];
  const int t = threadIdx.x;
  const long long b = blockIdx.x / blocks_per_element;
  const long long f = (long long)(blockIdx.x - (unsigned)b * blocks_per_element) * kPdThreads + t;
  const bool live = f < F;
  float4 q0 = {0.0f, 0.0f, 0.0f, 0.0f}, q1 = q0, q2 = q0, q3 = q0;
  if (live) {
    const float4* __restrict__ rec = records + ((size_t)b * F + f) * (kPdRecord / 4);
    q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
  }
  const PdTri tri = pd_unpack(q0, q1, q2, q3);
  const bool valid = q3.w != 0.0f;
  const float* __restrict__ pb = points + (size_t)b * P * 3;
  float best = __builtin_inff();
  int arg = -1;
  float w0 = pp::quiet_nan(), w1 = w0, w2 = w0;
  for (int p0 = 0; p0 < P; p0 += kPdPointTile) {
    const int n = P - p0 < kPdPointTile ? P - p0 : kPdPointTile;
    __syncthreads();   // the previous tile's readers are done
    for (int k = t; k < n * 3; k += kPdThreads) s_pt[k] = pb[(size_t)p0 * 3 + k];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const V3 p = {s_pt[j * 3], s_pt[j * 3 + 1], s_pt[j * 3 + 2]};
      const PdPair r = pd_pair(p, tri);
      if (valid && r.d < best) {
        best = r.d;
        arg = p0 + j;
        w0 = r.w0, w1 = r.w1, w2 = r.w2;
      }
    }
  }
  if (live) pd_store(dist, point, bary, (size_t)b * F + f, best, arg, w0, w1, w2);
}

// ---- backward -------------------------------------------------------------------------------------------------------
// Item s of batch element b pairs the face item_face[b,s] (NULL: s) with the point item_point[b,s] (NULL: s) at the
// weights bary[b,s]: vec = (2 g) (p - q), neg = -vec, face_out = the face, each may be NULL.  An item whose face or
// point is out of range, or whose face holds a vertex index out of range, gives +0 and face_out = -1.
__global__ __launch_bounds__(kPdThreads) void pd_backward_kernel(
    const float* __restrict__ points, const float* __restrict__ vertices, const long long* __restrict__ faces,
    const long long* __restrict__ item_face, const long long* __restrict__ item_point, const float* __restrict__ bary,
    const float* __restrict__ g, float* __restrict__ vec, float* __restrict__ neg, long long* __restrict__ face_out,
    long long total, int N, int F, int P, int S, int shared) {
  const long long x = (long long)blockIdx.x * kPdThreads + threadIdx.x;
  if (x >= total) return;
  const long long b = x / S;
  const long long f = item_face ? item_face[x] : x - b * S;
  const long long i = item_point ? item_point[x] : x - b * S;
  bool ok = f >= 0 && f < F && i >= 0 && i < P;
  long long i0 = 0, i1 = 0, i2 = 0;
  if (ok) {   // (the face row and the stores are written out: pp::mesh_face and v3_store change this kernel's code)
    const long long* __restrict__ row = faces + ((shared ? 0 : b * F) + f) * 3;
    i0 = row[0], i1 = row[1], i2 = row[2];
    ok = !(i0 < 0 || i0 >= N || i1 < 0 || i1 >= N || i2 < 0 || i2 >= N);
  }
  V3 out = {0.0f, 0.0f, 0.0f}, opp = out;
  if (ok) {
    const float* __restrict__ vb = vertices + (size_t)b * N * 3;
    const V3 a = v3_load(vb, i0), c1 = v3_load(vb, i1), c2 = v3_load(vb, i2);
    const V3 p = v3_load(points + (size_t)b * P * 3, i);
    const float w0 = bary[x * 3], w1 = bary[x * 3 + 1], w2 = bary[x * 3 + 2];
    const float rx = p.x - ((w0 * a.x + w1 * c1.x) + w2 * c2.x);
    const float ry = p.y - ((w0 * a.y + w1 * c1.y) + w2 * c2.y);
    const float rz = p.z - ((w0 * a.z + w1 * c1.z) + w2 * c2.z);
    const float s2 = 2.0f * g[x];
    out = {s2 * rx, s2 * ry, s2 * rz};
    opp = {-out.x, -out.y, -out.z};
  }
  if (vec) {
    vec[x * 3] = out.x;
    vec[x * 3 + 1] = out.y;
    vec[x * 3 + 2] = out.z;
  }
  if (neg) {
    neg[x * 3] = opp.x;
    neg[x * 3 + 1] = opp.y;
    neg[x * 3 + 2] = opp.z;
  }
  if (face_out) face_out[x] = ok ? f : -1;
}

// one lane per (b, point): the sum of vec over the point's sorted face list, plain fp32 additions from +0
__global__ __launch_bounds__(kPdThreads) void pd_point_sums_kernel(const unsigned* __restrict__ start,
                                                                   const unsigned* __restrict__ cursor,
                                                                   const unsigned* __restrict__ entries,
                                                                   const float* __restrict__ vec,
                                                                   float* __restrict__ grad_points, long long rows,
                                                                   int F, int P) {
  const long long i = (long long)blockIdx.x * kPdThreads + threadIdx.x;
  if (i >= rows) return;
  const long long b = i / P;
  const unsigned s0 = start[i], n = cursor[i] - s0;
  const unsigned* __restrict__ list = entries + (size_t)b * F + s0;
  const float* __restrict__ vb = vec + (size_t)b * F * 3;
  V3 acc = {0.0f, 0.0f, 0.0f};
  for (unsigned q = 0; q < n; ++q) {
    const unsigned e = list[q];
    V3 term = v3_nan();
    if (e < (unsigned)F) term = v3_load(vb, e);
    acc = v3_add(acc, term);
  }
  v3_store(grad_points, i, acc);
}

}  // namespace

extern "C" int pp_mesh_distance_records_f32(const float* vertices, const long long* faces, float* records, int B, int N,
                                            int F, int shared_topology, void* stream) {
  if (!pp::mesh_sizes_ok(B, N, F, 0)) return PP_EINVAL;
  if (B == 0 || N == 0 || F == 0) return PP_OK;
  if (!vertices || !faces || !records || ((uintptr_t)records & 15u)) return PP_EINVAL;
  const long long rows = (long long)B * F;
  pd_records_kernel<<<dim3(pp::blocks(rows, kPdThreads)), dim3(kPdThreads), 0, (hipStream_t)stream>>>(
      vertices, faces, reinterpret_cast<float4*>(records), rows, N, F, shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_point_face_forward_f32(const float* points, const float* records, float* dist, long long* face,
                                              float* bary, int B, int P, int F, void* stream) {
  if (!pp::mesh_sizes_ok(B, 0, F, P)) return PP_EINVAL;
  if (B == 0 || P == 0 || F == 0) return PP_OK;
  if (!points || !records || !dist || !face || !bary || ((uintptr_t)records & 15u)) return PP_EINVAL;
  const int per_element = (int)pp::blocks(P, kPdThreads);
  if ((long long)B * per_element > 0x7fffffffLL) return PP_EINVAL;
  pd_point_face_kernel<<<dim3((unsigned)(B * per_element)), dim3(kPdThreads), 0, (hipStream_t)stream>>>(
      points, reinterpret_cast<const float4*>(records), dist, face, bary, P, F, per_element);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_face_point_forward_f32(const float* points, const float* records, float* dist, long long* point,
                                              float* bary, int B, int P, int F, void* stream) {
  if (!pp::mesh_sizes_ok(B, 0, F, P)) return PP_EINVAL;
  if (B == 0 || P == 0 || F == 0) return PP_OK;
  if (!points || !records || !dist || !point || !bary || ((uintptr_t)records & 15u)) return PP_EINVAL;
  const int per_element = (int)pp::blocks(F, kPdThreads);
  if ((long long)B * per_element > 0x7fffffffLL) return PP_EINVAL;
  pd_face_point_kernel<<<dim3((unsigned)(B * per_element)), dim3(kPdThreads), 0, (hipStream_t)stream>>>(
      points, reinterpret_cast<const float4*>(records), dist, point, bary, P, F, per_element);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_distance_backward_f32(const float* points, const float* vertices, const long long* faces,
                                             const long long* item_face, const long long* item_point,
                                             const float* bary, const float* grad_dist, float* vec, float* neg,
                                             long long* face_out, float* grad_points, int B, int N, int F, int P,
                                             int shared_topology, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  if (!pp::mesh_sizes_ok(B, N, F, P)) return PP_EINVAL;
  if (B == 0 || N == 0 || F == 0 || P == 0) return PP_OK;
  if (!points || !vertices || !faces || !bary || !grad_dist || (item_face != nullptr) == (item_point != nullptr))
    return PP_EINVAL;
  if (grad_points && (!item_point || !vec || vec == grad_points)) return PP_EINVAL;
  if (!vec && !neg) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int S = item_face ? P : F;   // one item per point, or one per face
  const long long total = (long long)B * S;
  pd_backward_kernel<<<dim3(pp::blocks(total, kPdThreads)), dim3(kPdThreads), 0, s>>>(
      points, vertices, faces, item_face, item_point, bary, grad_dist, vec, neg, face_out, total, N, F, P, S,
      shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  if (!grad_points) return PP_OK;
  const pp::BucketLayout L = pp::bucket_layout(B, P, F, false);
  unsigned char* ws = (unsigned char*)workspace;
  if (!ws || workspace_bytes < L.total) return PP_EINVAL;
  const int rc = pp::mesh_item_lists(item_point, B, P, F, L, ws, s);   // (a face whose point is out of range: no part)
  if (rc != PP_OK) return rc;
  const long long rows = (long long)B * P;
  pd_point_sums_kernel<<<dim3(pp::blocks(rows, kPdThreads)), dim3(kPdThreads), 0, s>>>(
      reinterpret_cast<const unsigned*>(ws + L.start), reinterpret_cast<const unsigned*>(ws + L.cursor),
      reinterpret_cast<const unsigned*>(ws + L.entries), vec, grad_points, rows, F, P);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}
