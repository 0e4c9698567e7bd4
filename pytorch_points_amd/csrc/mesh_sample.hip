// mesh_sample.hip -- area-weighted sampling of points on a triangle mesh's surface and the re-evaluation of a sample
// set on a deformed mesh, on the corner lists of mesh_edges.hip and the list chain of bucket_lists.h.  The sixth mesh
// operator; contract in DESIGN.md "Mesh surface sampling".
//
//   cdf        one workgroup per batch element: cdf[b,f] = the fp64 inclusive prefix sum of the fp32 areas[b,:], in
//              chunks of kBucketScanThreads with a fixed association (lanes of a wave, then the waves, then the chunks)
//   forward    one lane per sample, a workgroup within one batch element.  CHOOSE: target = double(u1) * cdf[F-1],
//              face = the first f with cdf[f] > target: the top levels of the search run over a strided sample of the
//              CDF in LDS (every ceil(F/4096)-th entry, at most 32 KB), the last ones over global memory; then
//              su = sqrtf(u2), w = (1 - su, su (1 - u3), su u3).  Otherwise face and w are the caller's.
//              points_d = (w0 p0_d + w1 p1_d) + w2 p2_d, every operation rounded on its own; normals = the face's.
//   backward   the face -> sample lists of this call (pp::mesh_item_lists: buckets the B*F faces, items the samples,
//              sorted), then
//              stage 1, per face: gC[f][c] = sum over its samples in ascending order of w_c g_points, and
//                       gN[f] = sum of g_normals, plain fp32 additions from +0 by one lane; a list beyond kBucketLong
//                       (the chain's own list of long buckets) by a whole workgroup: lane t adds the entries t, t+T, ...
//                       in order, then a fixed tree over the lanes of a wave and the waves in order
//              stage 2, per vertex: the sum of gC over its sorted corner slice (the slot code 3f + c is gC's row),
//                       plus the result of pp_mesh_face_normals_backward_f32 on gN.
//
// No floating-point atomics: every output word is written once and the bits are the same on every run.
//
// An index of `faces` outside [0, N), a caller's `face` outside [0, F) and a slot code that names no face are only
// compared, never used as an address: the sample's point is NaN, and in the backward the sample (or the whole face
// with such a vertex) adds nothing.
#include "mesh_common.h"   // pp::mesh_face, mesh_row, mesh_slice, mesh_item_lists, mesh_sizes_ok, V3 and v3_*

namespace {

using namespace pp;   // mesh_common.h's rows, three-vectors and item lists; bucket_lists.h

constexpr int kMsThreads = 256;
constexpr int kMsForwardThreads = 1024;   // samples of a workgroup: they share one staged CDF
constexpr int kMsStaged = 4096;           // CDF entries in LDS: 32 KB
constexpr int kMsLongThreads = 512;

// ---- cdf ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(pp::kBucketScanThreads) void ms_cdf_kernel(const float* __restrict__ areas,
                                                                        double* __restrict__ cdf, int F) {
  __shared__ double s_wave[pp::kBucketScanThreads / 64];
  const int t = threadIdx.x;
  const float* __restrict__ ar = areas + (size_t)blockIdx.x * F;
  double* __restrict__ out = cdf + (size_t)blockIdx.x * F;
  double carry = 0.0;
  for (int i0 = 0; i0 < F; i0 += pp::kBucketScanThreads) {
    const int i = i0 + t;
    double incl = i < F ? (double)ar[i] : 0.0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double o = __shfl_up(incl, off);
      if ((t & 63) >= off) incl += o;
    }
    __syncthreads();   // the previous chunk's readers of s_wave are done
    if ((t & 63) == 63) s_wave[t >> 6] = incl;
    __syncthreads();
    double before = 0.0, all = 0.0;
    for (int w = 0; w < pp::kBucketScanThreads / 64; ++w) {
      const double s = s_wave[w];
      if (w < (t >> 6)) before += s;
      all += s;
    }
    if (i < F) out[i] = carry + (before + incl);
    carry += all;
  }
}

// ---- forward --------------------------------------------------------------------------------------------------------
// CHOOSE: face and weights from cdf and u (u_stride floats per sample: u1, and with points u2, u3); else from face_in
// and bary_in.  points, normals (with face_normals), face_out and bary_out may be NULL.
template <bool CHOOSE>
__global__ __launch_bounds__(kMsForwardThreads) void ms_forward_kernel(
    const float* __restrict__ vertices, const long long* __restrict__ faces, const double* __restrict__ cdf,
    const float* __restrict__ u, int u_stride, const long long* __restrict__ face_in,
    const float* __restrict__ bary_in, const float* __restrict__ face_normals, long long* __restrict__ face_out,
    float* __restrict__ bary_out, float* __restrict__ points, float* __restrict__ normals, int N, int F, int S,
    int blocks_per_element, int shared) {
  __shared__ double s_cdf[CHOOSE ? kMsStaged : 1];
  const int t = threadIdx.x;
  const long long b = blockIdx.x / blocks_per_element;
  const long long s = (long long)(blockIdx.x - (unsigned)b * blocks_per_element) * kMsForwardThreads + t;
  const int stride = (F + kMsStaged - 1) / kMsStaged;      // F >= 1
  const int staged = (F + stride - 1) / stride;            // <= kMsStaged; entry i is the last of [i*stride, (i+1)*stride)
  const double* __restrict__ cb = CHOOSE ? cdf + (size_t)b * F : nullptr;
  if (CHOOSE) {
    for (int i = t; i < staged; i += kMsForwardThreads) {
      const long long last = (long long)(i + 1) * stride;
      s_cdf[i] = cb[(last < F ? last : F) - 1];
    }
    __syncthreads();
  }
  if (s >= S) return;
  const size_t x = (size_t)b * S + s;
  long long f;
  V3 w;
  if (CHOOSE) {
    const double total = s_cdf[staged - 1];                // cdf[b, F-1]
    f = -1;
    w = v3_nan();
    if (total > 0.0 && total < __builtin_inf()) {
      const float* __restrict__ us = u + x * u_stride;
      const double target = (double)us[0] * total;
      int lo = 0, hi = staged;                             // the first staged entry beyond target
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_cdf[mid] > target) hi = mid; else lo = mid + 1;
      }
      if (lo < staged) {                                   // (else target >= total: u1 outside [0,1))
        int a = lo * stride;
        long long e = (long long)(lo + 1) * stride;
        int z = (int)(e < F ? e : F) - 1;                  // cdf[z] > target is known
        while (a < z) {
          const int mid = (a + z) >> 1;
          if (cb[mid] > target) z = mid; else a = mid + 1;
        }
        f = a;
        if (u_stride >= 3) {
          const float su = sqrtf(us[1]);
          w = {1.0f - su, su * (1.0f - us[2]), su * us[2]};
        }
      }
    }
    if (face_out) face_out[x] = f;
    if (bary_out) v3_store(bary_out, x, w);
  } else {
    f = face_in[x];
    w = v3_load(bary_in, x);
  }
  if (!points) return;
  MeshFace tri = {0, 0, 0, false};
  if (f >= 0 && f < F) tri = mesh_face(faces, b, f, F, N, shared);
  if (!tri.in_range) {
    v3_store(points, x, v3_nan());
    if (normals) v3_store(normals, x, v3_nan());
    return;
  }
  const float* __restrict__ vb = vertices + (size_t)b * N * 3;
  v3_store(points, x, v3_weighted(w.x, v3_load(vb, tri.i0), w.y, v3_load(vb, tri.i1), w.z, v3_load(vb, tri.i2)));
  if (normals) v3_store(normals, x, v3_load(face_normals, b * F + f));
}

// ---- backward -------------------------------------------------------------------------------------------------------
// the sums of one face over the entries q = first, first + step, ... < n of its list
struct MsSums {
  float c[9], n[3];
};
template <bool POINTS, bool NORMALS>
__device__ __forceinline__ MsSums ms_list_sums(const unsigned* __restrict__ list, unsigned first, unsigned step,
                                               unsigned n, const float* __restrict__ bary,
                                               const float* __restrict__ gp, const float* __restrict__ gn,
                                               size_t base) {
  MsSums a;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.c[k] = 0.0f;
  a.n[0] = a.n[1] = a.n[2] = 0.0f;
  for (unsigned q = first; q < n; q += step) {
    const size_t x = (base + list[q]) * 3;
    if (POINTS) {
      const float g0 = gp[x], g1 = gp[x + 1], g2 = gp[x + 2];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float w = bary[x + c];
        a.c[c * 3] += w * g0;
        a.c[c * 3 + 1] += w * g1;
        a.c[c * 3 + 2] += w * g2;
      }
    }
    if (NORMALS) {
      a.n[0] += gn[x];
      a.n[1] += gn[x + 1];
      a.n[2] += gn[x + 2];
    }
  }
  return a;
}

template <bool POINTS, bool NORMALS>
__device__ __forceinline__ void ms_store_sums(const MsSums& a, float* __restrict__ gC, float* __restrict__ gN,
                                              size_t i) {
  if (POINTS) {
#pragma unroll
    for (int k = 0; k < 9; ++k) gC[i * 9 + k] = a.c[k];
  }
  if (NORMALS) v3_store(gN, i, {a.n[0], a.n[1], a.n[2]});
}

// stage 1: one lane per (b, face); a list beyond kBucketLong is left to ms_face_sums_long_kernel
template <bool POINTS, bool NORMALS>
__global__ __launch_bounds__(kMsThreads) void ms_face_sums_kernel(
    const long long* __restrict__ faces, const unsigned* __restrict__ start, const unsigned* __restrict__ cursor,
    const unsigned* __restrict__ entries, const float* __restrict__ bary, const float* __restrict__ gp,
    const float* __restrict__ gn, float* __restrict__ gC, float* __restrict__ gN, long long rows, int N, int F, int S,
    int shared) {
  const long long i = (long long)blockIdx.x * kMsThreads + threadIdx.x;
  if (i >= rows) return;
  const long long b = i / F;
  const unsigned s0 = start[i];
  unsigned n = cursor[i] - s0;
  if (!mesh_face(faces, b, i - b * F, F, N, shared).in_range)
    n = 0;   // adds nothing
  else if (n > (unsigned)pp::kBucketLong)
    return;
  const MsSums a = ms_list_sums<POINTS, NORMALS>(entries + (size_t)b * S + s0, 0u, 1u, n, bary, gp, gn, (size_t)b * S);
  ms_store_sums<POINTS, NORMALS>(a, gC, gN, (size_t)i);
}

// stage 1, long lists: a workgroup per list of bucket_sort_kernel's longlist
template <bool POINTS, bool NORMALS>
__global__ __launch_bounds__(kMsLongThreads) void ms_face_sums_long_kernel(
    const long long* __restrict__ faces, const unsigned* __restrict__ start, const unsigned* __restrict__ cursor,
    const unsigned* __restrict__ entries, const unsigned* __restrict__ nlong, const unsigned* __restrict__ longlist,
    const float* __restrict__ bary, const float* __restrict__ gp, const float* __restrict__ gn,
    float* __restrict__ gC, float* __restrict__ gN, int N, int F, int S, int shared) {
  constexpr int kWaves = kMsLongThreads / 64;
  __shared__ float s_part[kWaves][12];
  const int t = threadIdx.x;
  const unsigned count = *nlong;
  for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
    const unsigned i = longlist[q];
    const long long b = i / (unsigned)F;
    if (!mesh_face(faces, b, (long long)i - b * F, F, N, shared).in_range) continue;   // (the whole workgroup)
    const unsigned s0 = start[i], n = cursor[i] - s0;
    const MsSums a = ms_list_sums<POINTS, NORMALS>(entries + (size_t)b * S + s0, (unsigned)t, (unsigned)kMsLongThreads,
                                                   n, bary, gp, gn, (size_t)b * S);
    float v[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = a.c[k];
    v[9] = a.n[0], v[10] = a.n[1], v[11] = a.n[2];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    }
    __syncthreads();   // the previous list's reader is done
    if ((t & 63) == 0) {
#pragma unroll
      for (int k = 0; k < 12; ++k) s_part[t >> 6][k] = v[k];
    }
    __syncthreads();
    if (t == 0) {
      MsSums r;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        float acc = s_part[0][k];
        for (int w = 1; w < kWaves; ++w) acc += s_part[w][k];
        if (k < 9) r.c[k] = acc; else r.n[k - 9] = acc;
      }
      ms_store_sums<POINTS, NORMALS>(r, gC, gN, (size_t)i);
    }
  }
}

// stage 2: grad_i = sum over the vertex's slots of gC[slot code] (+ extra_i)
__global__ __launch_bounds__(kMsThreads) void ms_vertex_gather_kernel(const int* __restrict__ start,
                                                                      const unsigned* __restrict__ codes,
                                                                      const float* __restrict__ gC,
                                                                      const float* __restrict__ extra,
                                                                      float* __restrict__ grad, long long rows, int N,
                                                                      int F, int shared) {
  const long long r = (long long)blockIdx.x * kMsThreads + threadIdx.x;
  if (r >= rows) return;
  const long long X = 3LL * F;
  const MeshRow w = mesh_row(r, N, shared);
  const MeshSlice s = mesh_slice(start, nullptr, codes, w, N, X);
  const float* __restrict__ gb = gC + (size_t)w.b * (size_t)X * 3;
  V3 acc = {0.0f, 0.0f, 0.0f};
  for (int q = s.q0; q < s.q1; ++q) {
    const unsigned code = s.codes[q];
    V3 term = v3_nan();
    if (code < (unsigned)X) term = v3_load(gb, code);
    acc = v3_add(acc, term);
  }
  if (extra) acc = v3_add(acc, v3_load(extra, r));
  v3_store(grad, r, acc);
}

template <bool POINTS, bool NORMALS>
int ms_face_sums(const long long* faces, unsigned char* ws, const pp::BucketLayout& L, const float* bary,
                 const float* gp, const float* gn, float* gC, float* gN, int B, int N, int F, int S, int shared,
                 hipStream_t s) {
  const unsigned* start = reinterpret_cast<const unsigned*>(ws + L.start);
  const unsigned* cursor = reinterpret_cast<const unsigned*>(ws + L.cursor);
  const unsigned* entries = reinterpret_cast<const unsigned*>(ws + L.entries);
  const long long rows = (long long)B * F;
  ms_face_sums_kernel<POINTS, NORMALS><<<dim3(pp::blocks(rows, kMsThreads)), dim3(kMsThreads), 0, s>>>(
      faces, start, cursor, entries, bary, gp, gn, gC, gN, rows, N, F, S, shared);
  PP_RETURN_IF_LAUNCH_FAILED();
  ms_face_sums_long_kernel<POINTS, NORMALS><<<dim3(pp::kBucketSortBlocks), dim3(kMsLongThreads), 0, s>>>(
      faces, start, cursor, entries, reinterpret_cast<const unsigned*>(ws + L.nlong),
      reinterpret_cast<const unsigned*>(ws + L.longlist), bary, gp, gn, gC, gN, N, F, S, shared);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

}  // namespace

extern "C" int pp_mesh_sample_cdf_f32(const float* areas, double* cdf, int B, int F, void* stream) {
  if (B < 0 || F < 0 || (long long)B * F > 0x7fffffffLL) return PP_EINVAL;
  if (B == 0 || F == 0) return PP_OK;
  if (!areas || !cdf) return PP_EINVAL;
  ms_cdf_kernel<<<dim3((unsigned)B), dim3(pp::kBucketScanThreads), 0, (hipStream_t)stream>>>(areas, cdf, F);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_sample_forward_f32(const float* vertices, const long long* faces, const double* cdf,
                                          const float* u, int u_stride, const long long* face_in,
                                          const float* bary_in, const float* face_normals, long long* face_out,
                                          float* bary_out, float* points, float* normals, int B, int N, int F, int S,
                                          int shared_topology, void* stream) {
  if (!pp::mesh_sizes_ok(B, N, F, S)) return PP_EINVAL;
  if (B == 0 || F == 0 || S == 0 || (points && N == 0)) return PP_OK;
  const bool choose = cdf != nullptr;
  if (choose ? (!u || (u_stride != 1 && u_stride != 3) || face_in || bary_in) : (!face_in || !bary_in || !points))
    return PP_EINVAL;
  if (points && (!vertices || !faces || (choose && u_stride != 3))) return PP_EINVAL;
  if (!points && !face_out) return PP_EINVAL;
  if (normals && (!face_normals || !points)) return PP_EINVAL;
  const int per_element = (int)pp::blocks(S, kMsForwardThreads);
  if ((long long)B * per_element > 0x7fffffffLL) return PP_EINVAL;
  const dim3 grid((unsigned)(B * per_element)), block(kMsForwardThreads);
  hipStream_t s = (hipStream_t)stream;
  const int sh = shared_topology != 0;
  if (choose)
    ms_forward_kernel<true><<<grid, block, 0, s>>>(vertices, faces, cdf, u, u_stride, nullptr, nullptr, face_normals,
                                                   face_out, bary_out, points, normals, N, F, S, per_element, sh);
  else
    ms_forward_kernel<false><<<grid, block, 0, s>>>(vertices, faces, nullptr, nullptr, 0, face_in, bary_in,
                                                    face_normals, nullptr, nullptr, points, normals, N, F, S,
                                                    per_element, sh);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_sample_backward_f32(const float* vertices, const long long* faces, const int* start,
                                           const int* nbr, const unsigned* codes, const long long* face,
                                           const float* bary, const float* grad_points, const float* grad_normals,
                                           float* scratch, float* grad_vertices, int B, int N, int F, int S,
                                           int shared_topology, void* workspace, size_t workspace_bytes,
                                           void* stream) {
  if (!pp::mesh_sizes_ok(B, N, F, S)) return PP_EINVAL;
  if (B == 0 || N == 0 || F == 0 || S == 0) return PP_OK;
  if (!vertices || !faces || !start || !nbr || !codes || !face || !bary || !scratch || !grad_vertices ||
      (!grad_points && !grad_normals) || scratch == grad_vertices)
    return PP_EINVAL;
  const pp::BucketLayout L = pp::bucket_layout(B, F, S, false);
  unsigned char* ws = (unsigned char*)workspace;
  if (!ws || workspace_bytes < L.total) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int sh = shared_topology != 0;
  int rc = pp::mesh_item_lists(face, B, F, S, L, ws, s);   // a sample whose face is out of range takes no part
  if (rc != PP_OK) return rc;
  // scratch: gC (B,F,3,3) | gN (B,F,3) | the normals' gradient of the vertices (B,N,3); the last two with grad_normals
  float* gC = scratch;
  float* gN = scratch + (size_t)B * F * 9;
  float* extra = gN + (size_t)B * F * 3;
  if (grad_points && grad_normals)
    rc = ms_face_sums<true, true>(faces, ws, L, bary, grad_points, grad_normals, gC, gN, B, N, F, S, sh, s);
  else if (grad_points)
    rc = ms_face_sums<true, false>(faces, ws, L, bary, grad_points, nullptr, gC, nullptr, B, N, F, S, sh, s);
  else
    rc = ms_face_sums<false, true>(faces, ws, L, bary, nullptr, grad_normals, nullptr, gN, B, N, F, S, sh, s);
  if (rc != PP_OK) return rc;
  if (grad_normals) {
    rc = pp_mesh_face_normals_backward_f32(vertices, start, nbr, codes, gN, nullptr, grad_points ? extra : grad_vertices,
                                           B, N, F, shared_topology, stream);
    if (rc != PP_OK || !grad_points) return rc;
  }
  const long long rows = (long long)B * N;
  ms_vertex_gather_kernel<<<dim3(pp::blocks(rows, kMsThreads)), dim3(kMsThreads), 0, s>>>(
      start, codes, gC, grad_normals ? extra : nullptr, grad_vertices, rows, N, F, sh);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}
