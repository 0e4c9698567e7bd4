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
#include "mesh_common.h"   // pp::V3, md_load, md_sub, md_cross, md_dot; pp::blocks, pp::quiet_nan

namespace {

using pp::V3;
using pp::md_cross;
using pp::md_dot;
using pp::md_load;
using pp::md_sub;

constexpr int kMnThreads = 256;
constexpr float kMnEps = 1e-12f;   // F.normalize's eps

__device__ __forceinline__ float mn_len(V3 c) { return sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z); }
__device__ __forceinline__ V3 mn_div(V3 c, float d) { return {c.x / d, c.y / d, c.z / d}; }
__device__ __forceinline__ V3 mn_nan() { return {pp::quiet_nan(), pp::quiet_nan(), pp::quiet_nan()}; }
__device__ __forceinline__ void mn_store(float* __restrict__ p, V3 v) {
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
}
// (g - u (u.g)) / len: what reaches c through c / len
__device__ __forceinline__ V3 mn_project(V3 g, V3 u, float len) {
  const float t = md_dot(u, g);
  return {__builtin_fmaf(-t, u.x, g.x) / len, __builtin_fmaf(-t, u.y, g.y) / len, __builtin_fmaf(-t, u.z, g.z) / len};
}

// the slice of vertex i and the tables of its batch element
struct MnSlice {
  const int2* nb;
  const unsigned* cd;
  int q0, q1;
};
__device__ __forceinline__ MnSlice mn_slice(const int* __restrict__ start, const int* __restrict__ nbr,
                                            const unsigned* __restrict__ codes, long long tb, long long i, int N,
                                            long long X) {
  const int* __restrict__ st = start + (size_t)tb * ((size_t)N + 1) + i;
  MnSlice s;
  s.nb = reinterpret_cast<const int2*>(nbr) + (size_t)tb * (size_t)X;
  s.cd = codes ? codes + (size_t)tb * (size_t)X : nullptr;
  const int a = st[0], b = st[1];
  s.q0 = a < 0 ? 0 : a;
  s.q1 = (long long)b > X ? (int)X : b;
  return s;
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
  const long long* __restrict__ row = faces + (shared ? x - b * F : x) * 3;
  const long long i0 = row[0], i1 = row[1], i2 = row[2];
  if (i0 < 0 || i0 >= N || i1 < 0 || i1 >= N || i2 < 0 || i2 >= N) {
    mn_store(normals + x * 3, mn_nan());
    areas[x] = pp::quiet_nan();
    return;
  }
  const float* __restrict__ vb = vertices + (size_t)b * N * 3;
  const V3 p0 = md_load(vb, i0), p1 = md_load(vb, i1), p2 = md_load(vb, i2);
  const V3 c = md_cross(md_sub(p1, p0), md_sub(p2, p1));
  const float len = mn_len(c);
  areas[x] = len * 0.5f;
  mn_store(normals + x * 3, mn_div(c, len > kMnEps ? len : kMnEps));
}

__global__ __launch_bounds__(kMnThreads) void mn_face_backward_kernel(
    const float* __restrict__ vertices, const int* __restrict__ start, const int* __restrict__ nbr,
    const unsigned* __restrict__ codes, const float* __restrict__ grad_normals, const float* __restrict__ grad_areas,
    float* __restrict__ grad, long long rows, int N, int F, int shared) {
  const long long r = (long long)blockIdx.x * kMnThreads + threadIdx.x;
  if (r >= rows) return;
  const long long b = r / N;
  const long long i = r - b * N;
  const float* __restrict__ vb = vertices + (size_t)b * N * 3;
  const MnSlice s = mn_slice(start, nbr, codes, shared ? 0 : b, i, N, 3LL * F);
  const V3 pi = md_load(vb, i);
  V3 acc = {0.0f, 0.0f, 0.0f};
  for (int q = s.q0; q < s.q1; ++q) {
    const int2 jk = s.nb[q];
    const unsigned code = s.cd[q];
    const unsigned f = code / 3u, c = code - f * 3u;
    V3 term;
    if (f >= (unsigned)F || !mn_in_range(jk, N)) {
      term = mn_nan();
    } else {
      const V3 pn = md_load(vb, jk.x), pv = md_load(vb, jk.y);
      // the vertex is corner c: p_c = v_i, p_(c+1)%3 = next, p_(c+2)%3 = prev
      const V3 p0 = c == 0 ? pi : (c == 1 ? pv : pn);
      const V3 p1 = c == 0 ? pn : (c == 1 ? pi : pv);
      const V3 p2 = c == 0 ? pv : (c == 1 ? pn : pi);
      const V3 cr = md_cross(md_sub(p1, p0), md_sub(p2, p1));
      const float len = mn_len(cr);
      if (len <= kMnEps) {
        term = {0.0f, 0.0f, 0.0f};
      } else {
        const V3 u = mn_div(cr, len);
        const size_t face = (size_t)b * F + f;
        V3 G = {0.0f, 0.0f, 0.0f};
        if (grad_normals) G = mn_project(md_load(grad_normals, (long long)face), u, len);
        if (grad_areas) {
          const float h = grad_areas[face] * 0.5f;
          G = {__builtin_fmaf(h, u.x, G.x), __builtin_fmaf(h, u.y, G.y), __builtin_fmaf(h, u.z, G.z)};
        }
        term = md_cross(md_sub(pn, pv), G);
      }
    }
    acc = {acc.x + term.x, acc.y + term.y, acc.z + term.z};
  }
  mn_store(grad + r * 3, acc);
}

// ---- vertices -----------------------------------------------------------------------------------------------------
// S of vertex i: the weighted sum over its slots, NaN where a neighbour is out of range
template <int WEIGHTING>
__device__ __forceinline__ V3 mn_vertex_sum(const float* __restrict__ vb, const MnSlice& s, V3 pi, int N) {
  V3 S = {0.0f, 0.0f, 0.0f};
  for (int q = s.q0; q < s.q1; ++q) {
    const int2 jk = s.nb[q];
    V3 w;
    if (!mn_in_range(jk, N)) {
      w = mn_nan();
    } else {
      w = md_cross(md_sub(md_load(vb, jk.x), pi), md_sub(md_load(vb, jk.y), pi));
      if (WEIGHTING == 1) {
        const float len = mn_len(w);
        w = mn_div(w, len > kMnEps ? len : kMnEps);
      }
    }
    S = {S.x + w.x, S.y + w.y, S.z + w.z};
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
  const long long b = r / N;
  const long long i = r - b * N;
  const float* __restrict__ vb = vertices + (size_t)b * N * 3;
  const MnSlice s = mn_slice(start, nbr, nullptr, shared ? 0 : b, i, N, 3LL * F);
  const V3 S = mn_vertex_sum<WEIGHTING>(vb, s, md_load(vb, i), N);
  const float len = mn_len(S);
  mn_store(out + r * 3, mn_div(S, len > kMnEps ? len : kMnEps));
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
  const long long b = r / N;
  const long long i = r - b * N;
  const float* __restrict__ vb = vertices + (size_t)b * N * 3;
  const MnSlice s = mn_slice(start, nbr, nullptr, shared ? 0 : b, i, N, 3LL * F);
  const V3 S = mn_vertex_sum<WEIGHTING>(vb, s, md_load(vb, i), N);
  const float len = mn_len(S);
  V3 out = {0.0f, 0.0f, 0.0f};
  if (!(len <= kMnEps)) out = mn_project(md_load(grad_out, r), mn_div(S, len), len);   // (a NaN sum stays NaN)
  mn_store(h + r * 3, out);
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
  const long long b = r / N;
  const long long i = r - b * N;
  const float* __restrict__ vb = vertices + (size_t)b * N * 3;
  const float* __restrict__ hb = h + (size_t)b * N * 3;
  const MnSlice s = mn_slice(start, nbr, nullptr, shared ? 0 : b, i, N, 3LL * F);
  const V3 pi = md_load(vb, i), hi = md_load(hb, i);
  V3 acc = {0.0f, 0.0f, 0.0f};
  for (int q = s.q0; q < s.q1; ++q) {
    const int2 jk = s.nb[q];
    V3 term;
    if (!mn_in_range(jk, N)) {
      term = mn_nan();
    } else {
      const V3 pn = md_load(vb, jk.x), pv = md_load(vb, jk.y);
      const V3 hn = md_load(hb, jk.x), hv = md_load(hb, jk.y);
      V3 H = {(hi.x + hn.x) + hv.x, (hi.y + hn.y) + hv.y, (hi.z + hn.z) + hv.z};
      if (WEIGHTING == 1) {
        const V3 cr = md_cross(md_sub(pn, pi), md_sub(pv, pi));
        const float len = mn_len(cr);
        if (len <= kMnEps)
          H = {0.0f, 0.0f, 0.0f};
        else
          H = mn_project(H, mn_div(cr, len), len);
      }
      term = md_cross(md_sub(pn, pv), H);
    }
    acc = {acc.x + term.x, acc.y + term.y, acc.z + term.z};
  }
  mn_store(grad + r * 3, acc);
}

// the sizes every entry checks: the rows and the faces of a launch, and the slot codes, fit 31 bits
bool mn_sizes_ok(int B, int N, int F) {
  return B >= 0 && N >= 0 && F >= 0 && (long long)B * N <= 0x7fffffffLL && (long long)B * F <= 0x7fffffffLL &&
         3LL * F <= 0x7fffffffLL;
}

}  // namespace

extern "C" int pp_mesh_face_normals_forward_f32(const float* vertices, const long long* faces, float* normals,
                                                float* areas, int B, int N, int F, int shared_topology, void* stream) {
  if (!mn_sizes_ok(B, N, F)) return PP_EINVAL;
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
  if (!mn_sizes_ok(B, N, F)) return PP_EINVAL;
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
  if (!mn_sizes_ok(B, N, F) || weighting < 0 || weighting > 1) return PP_EINVAL;
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
  if (!mn_sizes_ok(B, N, F) || weighting < 0 || weighting > 1) return PP_EINVAL;
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
