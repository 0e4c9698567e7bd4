// mesh_normals.hip -- the unit normals and areas of a triangle mesh's faces (reference geo_operations.py:529-559
// compute_face_normals_and_areas) and the unit normals of its vertices, on the corner lists of mesh_edges.hip
// (pp_mesh_corner_incidence: per vertex the ascending slots 3f + c with (next, prev) beside each).  The fifth mesh
// operator on the pattern of mesh_dihedral.hip: nothing is built here, a step is one launch (the vertex backward two),
// every backward is a gather.
//
//   face forward     one thread per (b,f), p_k = vertices[b, faces[f,k]]:  c = (p1-p0) x (p2-p1),
//                    len = sqrtf((cx*cx + cy*cy) + cz*cz), area = len * 0.5f, normal = c / max(len, 1e-12f)
//   face backward    one thread per (b,vertex) over its slots in order: the slot 3f + c names the face and which of
//                    its corners the vertex is, (next, prev) the other two, so p0, p1, p2 are rebuilt without reading
//                    `faces` and the forward chain is evaluated again.  With u = c / len,
//                    G = (g_n - u (u.g_n)) / len + (g_a * 0.5f) u   and the slot adds  (v_next - v_prev) x G:
//                    c = p0 x p1 + p1 x p2 + p2 x p0, so d(G.c)/dv_i = (v_next - v_prev) x G.
//   vertex forward   one thread per (b,vertex):  S = sum over the slots of w(c_slot), c_slot = (v_next - v_i) x
//                    (v_prev - v_i) (the face's c, whichever corner it is taken at); weighting 0 ("area") w(c) = c,
//                    1 ("uniform") w(c) = c / max(|c|, 1e-12f);  out = S / max(|S|, 1e-12f)
//   vertex backward  (a) per vertex S again and h = (g - n (n.g)) / |S| with n = S / |S| into a (B,N,3) scratch;
//                    (b) per vertex over its slots H = h_i + h_next + h_prev -- every corner of a face adds the same
//                    w(c) to its own vertex -- for "uniform" H <- (H - u (u.H)) / |c|, and the slot adds
//                    (v_next - v_prev) x H.
//
// A face with len <= 1e-12f (and a vertex with |S| <= 1e-12f) passes no gradient: F.normalize's and sqrt's backward
// give 1e12 or NaN there.  The same rule as the dihedral backward's.
//
// Sums are plain fp32 additions from +0 in slot order; a*b - c*d is Kahan's difference of products (mesh_common.h).
// No floating-point atomics: every output word is written once and the bits are the same on every run.
//
// An index outside [0, n_vertices) is never used as an address: a neighbour the build stored as -1 (or any value out
// of range in a hand-made list), a face index out of range and a slot code that names no face are only compared, and
// the lane's results are NaN.  A slice is clipped to the list.
#include "mesh_common.h"   // pp::mesh_face, mesh_row, mesh_slice, mesh_sizes_ok, V3 and v3_*; pp::blocks, pp::quiet_nan

namespace {

using namespace pp;   // mesh_common.h's rows and three-vectors

constexpr int kMnThreads = 256;
constexpr float kMnEps = 1e-12f;   // F.normalize's eps

// (g - u (u.g)) / len: what reaches c through c / len
__device__ __forceinline__ V3 mn_project(V3 g, V3 u, float len) {
  return v3_div(v3_fma(-v3_dot_fused(u, g), u, g), len);
}
__device__ __forceinline__ bool mn_in_range(int2 jk, int N) { return jk.x >= 0 && jk.x < N && jk.y >= 0 && jk.y < N; }

// ---- faces --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMnThreads) void mn_face_forward_kernel(const float* __restrict__ vertices,
                                                                     const long long* __restrict__ faces,
                                                                     float* __restrict__ normals,
                                                                     float* __restrict__ areas, long long total, int N,
                                                                     int F, int shared) {
  const long long x = (long long)blockIdx.x * kMnThreads + threadIdx.x;
  if (x >= total) return;
  const long long b = x / F;
  const MeshFace t = mesh_face(faces, b, x - b * F, F, N, shared);
  if (!t.in_range) {
    v3_store(normals, x, v3_nan());
    areas[x] = quiet_nan();
    return;
  }
  const float* __restrict__ vb = vertices + (size_t)b * N * 3;
  const V3 p0 = v3_load(vb, t.i0), p1 = v3_load(vb, t.i1), p2 = v3_load(vb, t.i2);
  const V3 c = v3_cross(v3_sub(p1, p0), v3_sub(p2, p1));
  const float len = v3_len(c);
  areas[x] = len * 0.5f;
  v3_store(normals, x, v3_div(c, len > kMnEps ? len : kMnEps));
}

__global__ __launch_bounds__(kMnThreads) void mn_face_backward_kernel(
    const float* __restrict__ vertices, const int* __restrict__ start, const int* __restrict__ nbr,
    const unsigned* __restrict__ codes, const float* __restrict__ grad_normals, const float* __restrict__ grad_areas,
    float* __restrict__ grad, long long rows, int N, int F, int shared) {
  const long long r = (long long)blockIdx.x * kMnThreads + threadIdx.x;
  if (r >= rows) return;
  const MeshRow w = mesh_row(r, N, shared);
  const float* __restrict__ vb = vertices + (size_t)w.b * N * 3;
  const MeshSlice s = mesh_slice(start, nbr, codes, w, N, 3LL * F);
  const V3 pi = v3_load(vb, w.i);
  V3 acc = {0.0f, 0.0f, 0.0f};
  for (int q = s.q0; q < s.q1; ++q) {
    const int2 jk = s.nbr[q];
    const unsigned code = s.codes[q];
    const unsigned f = code / 3u, c = code - f * 3u;
    V3 term;
    if (f >= (unsigned)F || !mn_in_range(jk, N)) {
      term = v3_nan();
    } else {
      const V3 pn = v3_load(vb, jk.x), pv = v3_load(vb, jk.y);
      // the vertex is corner c: p_c = v_i, p_(c+1)%3 = next, p_(c+2)%3 = prev
      const V3 p0 = c == 0 ? pi : (c == 1 ? pv : pn);
      const V3 p1 = c == 0 ? pn : (c == 1 ? pi : pv);
      const V3 p2 = c == 0 ? pv : (c == 1 ? pn : pi);
      const V3 cr = v3_cross(v3_sub(p1, p0), v3_sub(p2, p1));
      const float len = v3_len(cr);
      if (len <= kMnEps) {
        term = v3_zero();
      } else {
        const V3 u = v3_div(cr, len);
        const size_t face = (size_t)w.b * F + f;
        V3 G = {0.0f, 0.0f, 0.0f};
        if (grad_normals) G = mn_project(v3_load(grad_normals, (long long)face), u, len);
        if (grad_areas) G = v3_fma(grad_areas[face] * 0.5f, u, G);
        term = v3_cross(v3_sub(pn, pv), G);
      }
    }
    acc = v3_add(acc, term);
  }
  v3_store(grad, r, acc);
}

// ---- vertices -----------------------------------------------------------------------------------------------------
// S of vertex i: the weighted sum over its slots, NaN where a neighbour is out of range
template <int WEIGHTING>
__device__ __forceinline__ V3 mn_vertex_sum(const float* __restrict__ vb, const MeshSlice& s, V3 pi, int N) {
  V3 S = {0.0f, 0.0f, 0.0f};
  for (int q = s.q0; q < s.q1; ++q) {
    const int2 jk = s.nbr[q];
    V3 w;
    if (!mn_in_range(jk, N)) {
      w = v3_nan();
    } else {
      w = v3_cross(v3_sub(v3_load(vb, jk.x), pi), v3_sub(v3_load(vb, jk.y), pi));
      if (WEIGHTING == 1) {
        const float len = v3_len(w);
        w = v3_div(w, len > kMnEps ? len : kMnEps);
      }
    }
    S = v3_add(S, w);
  }
  return S;
}

template <int WEIGHTING>
__global__ __launch_bounds__(kMnThreads) void mn_vertex_forward_kernel(const float* __restrict__ vertices,
                                                                       const int* __restrict__ start,
                                                                       const int* __restrict__ nbr,
                                                                       float* __restrict__ out, long long rows, int N,
                                                                       int F, int shared) {
  const long long r = (long long)blockIdx.x * kMnThreads + threadIdx.x;
  if (r >= rows) return;
  const MeshRow w = mesh_row(r, N, shared);
  const float* __restrict__ vb = vertices + (size_t)w.b * N * 3;
  const MeshSlice s = mesh_slice(start, nbr, nullptr, w, N, 3LL * F);
  const V3 S = mn_vertex_sum<WEIGHTING>(vb, s, v3_load(vb, w.i), N);
  const float len = v3_len(S);
  v3_store(out, r, v3_div(S, len > kMnEps ? len : kMnEps));
}

// (a) h_i = (g_i - n_i (n_i.g_i)) / |S_i|, 0 where |S_i| <= 1e-12f
template <int WEIGHTING>
__global__ __launch_bounds__(kMnThreads) void mn_vertex_h_kernel(const float* __restrict__ vertices,
                                                                 const int* __restrict__ start,
                                                                 const int* __restrict__ nbr,
                                                                 const float* __restrict__ grad_out,
                                                                 float* __restrict__ h, long long rows, int N, int F,
                                                                 int shared) {
  const long long r = (long long)blockIdx.x * kMnThreads + threadIdx.x;
  if (r >= rows) return;
  const MeshRow w = mesh_row(r, N, shared);
  const float* __restrict__ vb = vertices + (size_t)w.b * N * 3;
  const MeshSlice s = mesh_slice(start, nbr, nullptr, w, N, 3LL * F);
  const V3 S = mn_vertex_sum<WEIGHTING>(vb, s, v3_load(vb, w.i), N);
  const float len = v3_len(S);
  V3 out = {0.0f, 0.0f, 0.0f};
  if (!(len <= kMnEps)) out = mn_project(v3_load(grad_out, r), v3_div(S, len), len);   // (a NaN sum stays NaN)
  v3_store(h, r, out);
}

// (b) grad_i = sum over the slots of (v_next - v_prev) x H
template <int WEIGHTING>
__global__ __launch_bounds__(kMnThreads) void mn_vertex_backward_kernel(const float* __restrict__ vertices,
                                                                        const int* __restrict__ start,
                                                                        const int* __restrict__ nbr,
                                                                        const float* __restrict__ h,
                                                                        float* __restrict__ grad, long long rows, int N,
                                                                        int F, int shared) {
  const long long r = (long long)blockIdx.x * kMnThreads + threadIdx.x;
  if (r >= rows) return;
  const MeshRow w = mesh_row(r, N, shared);
  const float* __restrict__ vb = vertices + (size_t)w.b * N * 3;
  const float* __restrict__ hb = h + (size_t)w.b * N * 3;
  const MeshSlice s = mesh_slice(start, nbr, nullptr, w, N, 3LL * F);
  const V3 pi = v3_load(vb, w.i), hi = v3_load(hb, w.i);
  V3 acc = {0.0f, 0.0f, 0.0f};
  for (int q = s.q0; q < s.q1; ++q) {
    const int2 jk = s.nbr[q];
    V3 term;
    if (!mn_in_range(jk, N)) {
      term = v3_nan();
    } else {
      const V3 pn = v3_load(vb, jk.x), pv = v3_load(vb, jk.y);
      const V3 hn = v3_load(hb, jk.x), hv = v3_load(hb, jk.y);
      V3 H = v3_add(v3_add(hi, hn), hv);
      if (WEIGHTING == 1) {
        const V3 cr = v3_cross(v3_sub(pn, pi), v3_sub(pv, pi));
        const float len = v3_len(cr);
        if (len <= kMnEps)
          H = v3_zero();
        else
          H = mn_project(H, v3_div(cr, len), len);
      }
      term = v3_cross(v3_sub(pn, pv), H);
    }
    acc = v3_add(acc, term);
  }
  v3_store(grad, r, acc);
}

}  // namespace

extern "C" int pp_mesh_face_normals_forward_f32(const float* vertices, const long long* faces, float* normals,
                                                float* areas, int B, int N, int F, int shared_topology, void* stream) {
  if (!pp::mesh_sizes_ok(B, N, F)) return PP_EINVAL;
  if (B == 0 || N == 0 || F == 0) return PP_OK;
  if (!vertices || !faces || !normals || !areas) return PP_EINVAL;
  const long long total = (long long)B * F;
  mn_face_forward_kernel<<<dim3(pp::blocks(total, kMnThreads)), dim3(kMnThreads), 0, (hipStream_t)stream>>>(
      vertices, faces, normals, areas, total, N, F, shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_face_normals_backward_f32(const float* vertices, const int* start, const int* nbr,
                                                 const unsigned* codes, const float* grad_normals,
                                                 const float* grad_areas, float* grad_vertices, int B, int N, int F,
                                                 int shared_topology, void* stream) {
  if (!pp::mesh_sizes_ok(B, N, F)) return PP_EINVAL;
  if (B == 0 || N == 0 || F == 0) return PP_OK;
  if (!vertices || !start || !nbr || !codes || !grad_vertices) return PP_EINVAL;
  const long long rows = (long long)B * N;
  mn_face_backward_kernel<<<dim3(pp::blocks(rows, kMnThreads)), dim3(kMnThreads), 0, (hipStream_t)stream>>>(
      vertices, start, nbr, codes, grad_normals, grad_areas, grad_vertices, rows, N, F, shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_vertex_normals_forward_f32(const float* vertices, const int* start, const int* nbr, float* out,
                                                  int B, int N, int F, int weighting, int shared_topology,
                                                  void* stream) {
  if (!pp::mesh_sizes_ok(B, N, F) || weighting < 0 || weighting > 1) return PP_EINVAL;
  if (B == 0 || N == 0 || F == 0) return PP_OK;
  if (!vertices || !start || !nbr || !out) return PP_EINVAL;
  const long long rows = (long long)B * N;
  const dim3 grid(pp::blocks(rows, kMnThreads)), block(kMnThreads);
  hipStream_t s = (hipStream_t)stream;
  const int sh = shared_topology != 0;
  if (weighting == 0)
    mn_vertex_forward_kernel<0><<<grid, block, 0, s>>>(vertices, start, nbr, out, rows, N, F, sh);
  else
    mn_vertex_forward_kernel<1><<<grid, block, 0, s>>>(vertices, start, nbr, out, rows, N, F, sh);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_vertex_normals_backward_f32(const float* vertices, const int* start, const int* nbr,
                                                   const float* grad_out, float* scratch, float* grad_vertices, int B,
                                                   int N, int F, int weighting, int shared_topology, void* stream) {
  if (!pp::mesh_sizes_ok(B, N, F) || weighting < 0 || weighting > 1) return PP_EINVAL;
  if (B == 0 || N == 0 || F == 0) return PP_OK;
  if (!vertices || !start || !nbr || !grad_out || !scratch || !grad_vertices || scratch == grad_vertices)
    return PP_EINVAL;
  const long long rows = (long long)B * N;
  const dim3 grid(pp::blocks(rows, kMnThreads)), block(kMnThreads);
  hipStream_t s = (hipStream_t)stream;
  const int sh = shared_topology != 0;
  if (weighting == 0)
    mn_vertex_h_kernel<0><<<grid, block, 0, s>>>(vertices, start, nbr, grad_out, scratch, rows, N, F, sh);
  else
    mn_vertex_h_kernel<1><<<grid, block, 0, s>>>(vertices, start, nbr, grad_out, scratch, rows, N, F, sh);
  PP_RETURN_IF_LAUNCH_FAILED();
  if (weighting == 0)
    mn_vertex_backward_kernel<0><<<grid, block, 0, s>>>(vertices, start, nbr, scratch, grad_vertices, rows, N, F, sh);
  else
    mn_vertex_backward_kernel<1><<<grid, block, 0, s>>>(vertices, start, nbr, scratch, grad_vertices, rows, N, F, sh);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}
