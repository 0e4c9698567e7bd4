// mesh_dihedral.hip -- the face-to-face angle across a mesh edge (reference geo_operations.py:603-619 get_normals,
// :775-789 dihedral_angle) and the (E,4) "edge points" table it works on (reference utils/geometry_utils.py:242-341
// build_gemm / get_edge_points / get_side_points, a Python loop over the faces with a dict).  The fourth mesh operator
// on the pattern of mesh_edges.hip: the topology is built once, a step is two launches, the backward is a gather.
//
//   edge points    faces (Bt,F,3), the unique edges (Bt,Ecap,2) and their counts -> edge_points (Bt,Ecap,4): row e is
//                  [a, c, w0, w1], (a,c) the edge, w0 / w1 the corner opposite the edge in the incident half-edge with
//                  the lowest / highest number 3f + j; a boundary edge has w1 == w0; rows from count[b] on are -1.
//                  One thread per half-edge finds its edge by binary search and updates three integer words of the
//                  edge's own row (atomicMin, atomicMax, a count); one thread per edge decodes them.  Min and max do
//                  not depend on the order the atomics are served in, so nothing is sorted.
//   incidence      edge_points (Bt,Ecap,4), counts -> per vertex the ascending list of 4*e + slot: mesh_edges.hip's
//                  incidence build with four columns (pp_mesh_edge_points_incidence is defined there)
//   forward        one thread per (b,e):  na = (p2-p0) x (p1-p0), nb = (p3-p1) x (p0-p1), each divided by
//                  max(|n|, 1e-12); d = clamp(na.nb, -1+1e-6, 1-1e-6); out = pi - acos(d); 0 in the padding rows
//   backward       a GATHER, one thread per (b,vertex): from +0 over the vertex's list in order, the edge's chain
//                  evaluated again from its four vertices and that slot's term added with plain fp32 additions.
//                  No floating-point atomics, no per-edge gradient tensor, one form only.
//
// The evaluation order of a row is canonical: the two ends are taken in ascending vertex number and so are the two
// wings.  Swapping columns 0 and 1 flips both normals, swapping columns 2 and 3 trades them (and flips both), so the
// angle does not change, and with the canonical order not a bit of it changes either: any table made the reference's
// way (whose column order follows the face traversal) gives the same bits for the same edge.
//
// The cross and dot products are evaluated with fused multiply-adds written out (Kahan's difference of products), not
// by contraction: the cancellation in a*b - c*d is where a sliver face loses its digits.
//
// An index outside [0, n_vertices) is never used as an address: the builds compare it and leave out what it belongs
// to, the forward writes NaN for such an edge and the backward adds NaN for it.
#include "mesh_common.h"   // pp::mesh_half_edge, mesh_build_ok, mesh_row, V3 and v3_*; pp::blocks, pp::quiet_nan

namespace {

constexpr int kMdThreads = 256;
constexpr float kMdEps = 1e-12f;                          // F.normalize's eps
constexpr float kMdLo = (float)(-1.0 + 1e-6);             // torch's clamp bounds: the double, rounded to fp32
constexpr float kMdHi = (float)(1.0 - 1e-6);
constexpr float kMdPi = 3.14159265358979323846f;

// ---- edge points --------------------------------------------------------------------------------------------------
// The three words of an edge live in the edge's own output row (32 bytes) until the decode overwrites it.
__global__ __launch_bounds__(kMdThreads) void md_words_init_kernel(long long* __restrict__ edge_points,
                                                                   const int* __restrict__ counts, long long total,
                                                                   int Ecap) {
  const long long x = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (x >= total) return;
  const long long b = x / Ecap;
  if (x - b * Ecap >= counts[b]) return;
  edge_points[x * 4] = 0xffffffffLL;   // u32 word 0: the lowest half-edge number; word 1: the highest
  edge_points[x * 4 + 1] = 0;          // u32 word 2: how many
}

// One thread per half-edge (b, f, j) joining corners j and (j+1) mod 3.  One with an index outside [0, N) takes no
// part (pp_mesh_unique_edges has flagged it), nor does one whose pair is not in the list.
__global__ __launch_bounds__(kMdThreads) void md_half_edges_kernel(const long long* __restrict__ faces,
                                                                   const long long* __restrict__ edges,
                                                                   const int* __restrict__ counts,
                                                                   long long* __restrict__ edge_points,
                                                                   long long total, int F, int Ecap, int N) {
  const long long h = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (h >= total) return;
  const pp::MeshHalfEdge he = pp::mesh_half_edge(faces, h, F, N);
  if (!he.in_range) return;
  const long long b = he.b, mn = he.mn, mx = he.mx;
  const long long* __restrict__ eb = edges + b * Ecap * 2;
  int count = counts[b];
  count = count < 0 ? 0 : (count > Ecap ? Ecap : count);
  int lo = 0, hi = count;             // the first row that is not below (mn, mx)
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const long long a = eb[2 * (size_t)mid], c = eb[2 * (size_t)mid + 1];
    if (a < mn || (a == mn && c < mx))
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo >= count || eb[2 * (size_t)lo] != mn || eb[2 * (size_t)lo + 1] != mx) return;
  unsigned* w = reinterpret_cast<unsigned*>(edge_points + (b * Ecap + lo) * 4);
  const unsigned code = (unsigned)(h - b * 3LL * F);   // 3*f + j within the batch element
  atomicMin(w, code);
  atomicMax(w + 1, code);
  atomicAdd(w + 2, 1u);
}

// One thread per edge row: its words -> [a, c, w0, w1]; more than two half-edges set the batch element's flag.  An
// edge that no half-edge found (a list that is not the faces' own) gets the wings -1.
__global__ __launch_bounds__(kMdThreads) void md_decode_kernel(const long long* __restrict__ faces,
                                                               const long long* __restrict__ edges,
                                                               const int* __restrict__ counts,
                                                               long long* __restrict__ edge_points,
                                                               int* __restrict__ nonmanifold, long long total, int F,
                                                               int Ecap) {
  const long long x = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (x >= total) return;
  const long long b = x / Ecap;
  long long* row = edge_points + x * 4;
  if (x - b * Ecap >= counts[b]) {
    row[0] = row[1] = row[2] = row[3] = -1;
    return;
  }
  const unsigned long long lohi = (unsigned long long)row[0];
  const unsigned lowest = (unsigned)lohi, highest = (unsigned)(lohi >> 32), many = (unsigned)row[1];
  long long w0 = -1, w1 = -1;
  if (many > 0) {
    const long long* __restrict__ fb = faces + b * 3LL * F;
    const unsigned f0 = lowest / 3u, j0 = lowest - f0 * 3u, f1 = highest / 3u, j1 = highest - f1 * 3u;
    w0 = fb[(size_t)f0 * 3 + (j0 == 0 ? 2 : j0 - 1)];   // corner (j + 2) mod 3 is opposite half-edge j
    w1 = fb[(size_t)f1 * 3 + (j1 == 0 ? 2 : j1 - 1)];
  }
  if (many > 2) atomicOr(nonmanifold + b, 1);
  row[0] = edges[2 * x];
  row[1] = edges[2 * x + 1];
  row[2] = w0;
  row[3] = w1;
}

// ---- the chain ----------------------------------------------------------------------------------------------------
using namespace pp;   // mesh_common.h: V3 and v3_*; every dot product of the chain is v3_dot_fused

// a row in canonical order (ends ascending, wings ascending) and what became of the caller's slots
struct MdRow {
  long long i0, i1, i2, i3;
  bool swap01, swap23, in_range;
};
__device__ __forceinline__ MdRow md_row(const long long* __restrict__ row, int N) {
  const long long c0 = row[0], c1 = row[1], c2 = row[2], c3 = row[3];
  MdRow r;
  r.swap01 = c0 > c1;
  r.swap23 = c2 > c3;
  r.i0 = r.swap01 ? c1 : c0;
  r.i1 = r.swap01 ? c0 : c1;
  r.i2 = r.swap23 ? c3 : c2;
  r.i3 = r.swap23 ? c2 : c3;
  r.in_range = r.i0 >= 0 && r.i1 < N && r.i2 >= 0 && r.i3 < N;   // the smaller of each pair from below, the larger from above
  return r;
}

// the forward's values of one row, and what the backward needs beside them
struct MdChain {
  V3 u, w, s, t;        // p1-p0, p2-p0, p3-p1, p0-p1
  V3 ua, ub;            // the unit normals
  float la, lb, d_raw;  // |na|, |nb|, the dot before the clamp
};
__device__ __forceinline__ MdChain md_chain(const float* __restrict__ vb, const MdRow& r) {
  const V3 p0 = v3_load(vb, r.i0), p1 = v3_load(vb, r.i1), p2 = v3_load(vb, r.i2), p3 = v3_load(vb, r.i3);
  MdChain c;
  c.u = v3_sub(p1, p0);
  c.w = v3_sub(p2, p0);
  c.s = v3_sub(p3, p1);
  c.t = v3_sub(p0, p1);
  const V3 na = v3_cross(c.w, c.u), nb = v3_cross(c.s, c.t);
  c.la = sqrtf(v3_dot_fused(na, na));
  c.lb = sqrtf(v3_dot_fused(nb, nb));
  c.ua = v3_div(na, c.la > kMdEps ? c.la : kMdEps);
  c.ub = v3_div(nb, c.lb > kMdEps ? c.lb : kMdEps);
  c.d_raw = v3_dot_fused(c.ua, c.ub);
  return c;
}
__device__ __forceinline__ float md_clamp(float d) {
  // torch.clamp: NaN stays NaN
  return d < kMdLo ? kMdLo : (d > kMdHi ? kMdHi : d);
}

// one thread per (b, e)
__global__ __launch_bounds__(kMdThreads) void md_forward_kernel(const float* __restrict__ vertices,
                                                                const long long* __restrict__ edge_points,
                                                                const int* __restrict__ counts,
                                                                float* __restrict__ out, long long total, int N,
                                                                int Ecap, int shared) {
  const long long x = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (x >= total) return;
  const long long b = x / Ecap;
  const long long e = x - b * Ecap;
  const long long tb = shared ? 0 : b;
  if (e >= counts[tb]) {
    out[x] = 0.0f;
    return;
  }
  const MdRow r = md_row(edge_points + (tb * Ecap + e) * 4, N);
  if (!r.in_range) {
    out[x] = quiet_nan();
    return;
  }
  const MdChain c = md_chain(vertices + (size_t)b * N * 3, r);
  out[x] = kMdPi - acosf(md_clamp(c.d_raw));
}

// One thread per (b, vertex); its list in order, however long it is.  With g = grad_out[b,e] / sqrt(1 - d^2) where
// the dot lies inside the closed clamp interval (0 outside it, and 0 for an edge with a normal of length <= 1e-12):
//   ga = g (ub - d ua) / |na|,  gb = g (ua - d ub) / |nb|          (the gradients of the two normals)
//   slot 0: gb x s - (u x ga + ga x w)    slot 1: ga x w - (t x gb + gb x s)    slot 2: u x ga    slot 3: t x gb
__global__ __launch_bounds__(kMdThreads) void md_backward_kernel(
    const float* __restrict__ vertices, const long long* __restrict__ edge_points, const int* __restrict__ inc_start,
    const unsigned* __restrict__ inc_entries, const float* __restrict__ grad_out, float* __restrict__ grad,
    long long rows, int N, int Ecap, int shared) {
  const long long i = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (i >= rows) return;
  const MeshRow w = mesh_row(i, N, shared);
  const float* __restrict__ vb = vertices + (size_t)w.b * N * 3;
  const long long* __restrict__ eb = edge_points + (size_t)w.tb * Ecap * 4;
  const unsigned* __restrict__ list = inc_entries + (size_t)w.tb * Ecap * 4;
  const float* __restrict__ gb_ = grad_out + (size_t)w.b * Ecap;
  const int* __restrict__ st = inc_start + (size_t)w.tb * ((size_t)N + 1) + w.i;   // (read as it is, not clipped)
  V3 acc = {0.0f, 0.0f, 0.0f};
  for (int q = st[0], q1 = st[1]; q < q1; ++q) {
    const unsigned code = list[q];
    const unsigned e = code >> 2;
    unsigned slot = code & 3u;
    if (e >= (unsigned)Ecap) continue;   // (a list that is not this table's own)
    const MdRow r = md_row(eb + (size_t)e * 4, N);
    V3 term;
    if (!r.in_range) {
      term = v3_nan();
    } else {
      if (slot < 2u ? r.swap01 : r.swap23) slot ^= 1u;   // the caller's slot in canonical order
      const MdChain c = md_chain(vb, r);
      const float d = md_clamp(c.d_raw);
      float fa = 0.0f, fb = 0.0f;
      if (c.d_raw >= kMdLo && c.d_raw <= kMdHi && c.la > kMdEps && c.lb > kMdEps) {
        const float g = gb_[e] / sqrtf((1.0f - d) * (1.0f + d));
        fa = g / c.la;
        fb = g / c.lb;
      }
      const V3 ga = v3_scale(fa, v3_fma(-d, c.ua, c.ub)), gb = v3_scale(fb, v3_fma(-d, c.ub, c.ua));
      if (slot == 2u) {
        term = v3_cross(c.u, ga);
      } else if (slot == 3u) {
        term = v3_cross(c.t, gb);
      } else {
        const V3 uga = v3_cross(c.u, ga), gaw = v3_cross(ga, c.w), tgb = v3_cross(c.t, gb), gbs = v3_cross(gb, c.s);
        term = slot == 0u ? v3_sub(gbs, v3_add(uga, gaw)) : v3_sub(gaw, v3_add(tgb, gbs));
      }
    }
    acc = v3_add(acc, term);
  }
  v3_store(grad, i, acc);
}

}  // namespace

extern "C" int pp_mesh_edge_points(const long long* faces, const long long* edges, const int* counts,
                                   long long* edge_points, int* nonmanifold, int Bt, int F, int Ecap, int n_vertices,
                                   void* stream) {
  const long long H = 3LL * (F > 0 ? F : 0);
  if (F < 0 || Ecap < 0 || !pp::mesh_build_ok(Bt, n_vertices, H, true) ||
      !pp::mesh_build_ok(Bt, n_vertices, 4LL * Ecap, true))
    return PP_EINVAL;
  if (Bt == 0 || Ecap == 0) return PP_OK;
  if (!edges || !counts || !edge_points || !nonmanifold || (F > 0 && !faces)) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long rows = (long long)Bt * Ecap;
  const dim3 block(kMdThreads), row_grid(pp::blocks(rows, kMdThreads));
  md_words_init_kernel<<<row_grid, block, 0, s>>>(edge_points, counts, rows, Ecap);
  PP_RETURN_IF_LAUNCH_FAILED();
  if (F > 0) {
    const long long total = (long long)Bt * H;
    md_half_edges_kernel<<<dim3(pp::blocks(total, kMdThreads)), block, 0, s>>>(faces, edges, counts, edge_points, total,
                                                                               F, Ecap, n_vertices);
    PP_RETURN_IF_LAUNCH_FAILED();
  }
  md_decode_kernel<<<row_grid, block, 0, s>>>(faces, edges, counts, edge_points, nonmanifold, rows, F, Ecap);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_dihedral_forward_f32(const float* vertices, const long long* edge_points, const int* counts,
                                            float* out, int B, int N, int Ecap, int shared_topology, void* stream) {
  if (B < 0 || N < 0 || Ecap < 0 || (long long)B * Ecap > 0x7fffffffLL || (long long)B * N > 0x7fffffffLL)
    return PP_EINVAL;
  if (B == 0 || Ecap == 0) return PP_OK;
  if (!edge_points || !counts || !out || (N > 0 && !vertices)) return PP_EINVAL;
  const long long total = (long long)B * Ecap;
  md_forward_kernel<<<dim3(pp::blocks(total, kMdThreads)), dim3(kMdThreads), 0, (hipStream_t)stream>>>(
      vertices, edge_points, counts, out, total, N, Ecap, shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_dihedral_backward_f32(const float* vertices, const long long* edge_points, const int* start,
                                             const unsigned* entries, const float* grad_out, float* grad_vertices,
                                             int B, int N, int Ecap, int shared_topology, void* stream) {
  if (B < 0 || N < 0 || Ecap < 0 || (long long)B * N > 0x7fffffffLL || 4LL * Ecap > 0x7fffffffLL) return PP_EINVAL;
  if (B == 0 || N == 0) return PP_OK;
  if (!vertices || !start || !grad_vertices || (Ecap > 0 && (!edge_points || !entries || !grad_out))) return PP_EINVAL;
  const long long rows = (long long)B * N;
  md_backward_kernel<<<dim3(pp::blocks(rows, kMdThreads)), dim3(kMdThreads), 0, (hipStream_t)stream>>>(
      vertices, edge_points, start, entries, grad_out, grad_vertices, rows, N, Ecap, shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}
