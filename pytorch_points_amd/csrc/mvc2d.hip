// mvc2d.hip -- mean value coordinates of 2-D query points with respect to a closed polygon (Floater, "Mean value
// coordinates", 2003; Hormann and Floater 2006 for the boundary rules), forward and backward, fp32 and fp64.
// Contract: DESIGN.md "Mean value coordinates, 2-D" (reference network/geo_operations.py:459-526).
//
// Layout: one workgroup = one wave = 64 queries of one batch element, one query per lane.  The wave walks the polygon
// in order, so a vertex is a wave-uniform load; the pair (vertex i, vertex i+1) is evaluated in fp64 registers for
// either data type, and what pair i-1 left (its t and its on-edge flag) is carried in registers.  Inputs are
// channel-first, points (B,2,N) and polygon (B,2,M); rows are (B,M,N) with N contiguous, so the wave's access to the
// row element of one vertex is one coalesced segment.  Any M: nothing per vertex is kept on chip.
//
// Forward: two walks.  The first finds what the row rules need before anything final can be written (any on-edge
// pair, any on-vertex distance, the sums); the second evaluates every pair again and writes each output element once.
//
// Backward: every pair is evaluated again and differentiated by hand.  dL/dpoints is summed in two registers per lane;
// a vertex's dL/dpolygon is summed over the wave in a fixed order and stored by one lane into the workgroup's slice of
// the workspace, and a second kernel adds the slices of a batch element in workgroup order.  No floating-point atomics:
// every output is reproducible bit for bit, and a query's forward row does not depend on the other queries.
#include <math.h>

#include "cage_common.h"

using namespace pp::cage;

namespace {

// code bits of a query row (kept for the backward)
constexpr int kZeroSum = 1, kOnEdge = 2, kOnVertex = 4, kNonFinite = 8;
constexpr double kAreaEps = 1e-5;    // |A_i| <= this: pair i contributes no t_i; with D_i < 0 the query is on edge i
constexpr double kVertexEps = 1e-8;  // r_i < this: the query is on vertex i
constexpr double kTiny = 1e-10;      // the reference's guard added to every denominator

// |(x, y)| with the rounding sequence of torch's 2-norm over a dimension of two (x*x rounded, then one fused
// multiply-add): the reference's r_i bit for bit.  One rounding of r_i r_{i+1} matters: far from the polygon
// r_i r_{i+1} - D_i keeps few of its digits
__device__ __forceinline__ double norm2(double x, double y) { return sqrt(__builtin_fma(y, y, x * x)); }

// vertex i as query n sees it: p the vertex itself (wave-uniform), s = p - q and r = |s|
struct Vtx {
  double px, py, x, y, r;
};

template <typename T>
__device__ __forceinline__ Vtx load_vtx(const T* __restrict__ px, const T* __restrict__ py, int i, double qx,
                                        double qy) {
  Vtx v;
  v.px = (double)px[i];
  v.py = (double)py[i];
  v.x = v.px - qx;
  v.y = v.py - qy;
  v.r = norm2(v.x, v.y);
  return v;
}

// pair i = (vertex i, vertex i+1): A the signed triangle area, D the dot product, t = (r r' - D) / (A + 1e-10) where
// |A| > 1e-5 (else 0), edge = the query lies on the segment
struct Pair {
  double A, D, t;
  bool big, edge;
};

__device__ __forceinline__ Pair eval_pair(const Vtx& a, const Vtx& b) {
  Pair p;
  p.A = (a.x * b.y - a.y * b.x) / 2.0;
  p.D = a.x * b.x + a.y * b.y;
  const double mag = fabs(p.A);
  p.big = mag > kAreaEps;
  p.edge = mag <= kAreaEps && p.D < 0.0;
  p.t = p.big ? (b.r * a.r - p.D) / (p.A + kTiny) : 0.0;
  return p;
}

__device__ __forceinline__ double edge_length(const Vtx& a, const Vtx& b) {
  const double ex = a.px - b.px, ey = a.py - b.py;
  return norm2(ex, ey);
}

// f(i, a, b, pr, prev) for i = 0 .. M-1 in order: a = vertex i, b = vertex i+1 (cyclic), pr = pair i, prev = pair i-1
template <typename T, typename F>
__device__ __forceinline__ void walk(const T* __restrict__ px, const T* __restrict__ py, int M, double qx, double qy,
                                     F f) {
  Vtx a = load_vtx(px, py, M - 1, qx, qy);
  Vtx b = load_vtx(px, py, 0, qx, qy);
  Pair prev = eval_pair(a, b);
  for (int i = 0; i < M; ++i) {
    a = b;
    b = load_vtx(px, py, i + 1 == M ? 0 : i + 1, qx, qy);
    const Pair pr = eval_pair(a, b);
    f(i, a, b, pr, prev);
    prev = pr;
  }
}

template <typename T>
__global__ __launch_bounds__(kWave) void mvc2d_forward_kernel(const T* __restrict__ points,
                                                              const T* __restrict__ polygon, T* __restrict__ phi,
                                                              T* __restrict__ wout, T* __restrict__ sums,
                                                              int* __restrict__ codes, int N, int M, int tiles) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int n = tile * kWave + lane;
  const bool live = n < N;
  const int nn = live ? n : N - 1;
  const T* pts = points + (long long)b * 2 * N;
  const double qx = (double)pts[nn], qy = (double)pts[(long long)N + nn];
  const T* px = polygon + (long long)b * 2 * M;
  const T* py = px + M;

  // walk 1: the flags and the sums.  sn: the plain row; sp: the on-edge values (the reference's row sum S' at that
  // point); sk: those of them that the later rule (1 - S' at the edge's far vertex) does not overwrite
  double sn = 0.0, sp = 0.0, sk = 0.0;
  int n_edge = 0, n_vertex = 0;
  bool bad = false;
  walk(px, py, M, qx, qy, [&](int, const Vtx& a, const Vtx& b2, const Pair& pr, const Pair& prev) {
    sn += (prev.t + pr.t) / (a.r + kTiny);
    if (pr.edge) {
      const double e = 1.0 - a.r / (edge_length(a, b2) + kTiny);
      sp += e;
      sk += prev.edge ? 0.0 : e;
      ++n_edge;
    }
    n_vertex += a.r < kVertexEps ? 1 : 0;
    bad = bad || !(fabs(a.x) < INFINITY && fabs(a.y) < INFINITY);
  });
  const bool on_vertex = n_vertex > 0, on_edge = n_edge > 0;
  const double far_value = 1.0 - sp;
  double S = on_vertex ? (double)n_vertex : (on_edge ? sk + (double)n_edge * far_value : sn);
  int code = (on_edge ? kOnEdge : 0) | (on_vertex ? kOnVertex : 0);
  if (S == 0.0) {
    S = 1.0;
    code |= kZeroSum;
  }
  if (bad) {
    code |= kNonFinite;
    S = __builtin_nan("");
  }
  if (live) {
    sums[(long long)b * N + n] = (T)S;
    codes[(long long)b * N + n] = code;
  }

  // walk 2: every pair again; each output element is written once
  T* out = phi + (long long)b * M * N + nn;
  T* raw = wout ? wout + (long long)b * M * N + nn : nullptr;
  walk(px, py, M, qx, qy, [&](int i, const Vtx& a, const Vtx& b2, const Pair& pr, const Pair& prev) {
    double e = 0.0;
    if (pr.edge) e = 1.0 - a.r / (edge_length(a, b2) + kTiny);
    const double plain = (prev.t + pr.t) / (a.r + kTiny);
    const double on_e = prev.edge ? far_value : e;
    const double on_v = a.r < kVertexEps ? 1.0 : 0.0;
    double w = on_vertex ? on_v : (on_edge ? on_e : plain);
    w = bad ? __builtin_nan("") : w;
    if (live) {
      out[(long long)i * N] = (T)(w / S);
      if (raw) raw[(long long)i * N] = (T)w;
    }
  });
}

// sum over the wave in a fixed order; every lane returns the same bits
__device__ __forceinline__ float wave_sum(float v) { return pp::wave_reduce_dpp<true>(v); }
__device__ __forceinline__ double wave_sum(double v) {
  double x[1] = {v};
  pp::cage::wave_sum(x);
  return x[0];
}

template <typename T>
__global__ __launch_bounds__(kWave) void mvc2d_backward_kernel(
    const T* __restrict__ points, const T* __restrict__ polygon, const T* __restrict__ phi,
    const T* __restrict__ sums, const int* __restrict__ codes, const T* __restrict__ gphi, const T* __restrict__ gw,
    T* __restrict__ gpoints, T* __restrict__ part, int N, int M, int tiles) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int n = tile * kWave + lane;
  const bool live = n < N;
  const int nn = live ? n : N - 1;
  const T* pts = points + (long long)b * 2 * N;
  const double qx = (double)pts[nn], qy = (double)pts[(long long)N + nn];
  const T* px = polygon + (long long)b * 2 * M;
  const T* py = px + M;
  const int code = codes[(long long)b * N + nn];
  // rows overridden to constants (on a vertex, non-finite): no gradient
  const bool dead = !live || (code & (kOnVertex | kNonFinite)) != 0;
  const bool replaced = (code & kZeroSum) != 0;
  const bool edge_row = !dead && (code & kOnEdge) != 0;
  const bool plain_row = !dead && (code & kOnEdge) == 0;
  const T* g = gphi + (long long)b * M * N + nn;
  const T* ph = phi + (long long)b * M * N + nn;
  const T* gr = gw ? gw + (long long)b * M * N + nn : nullptr;

  // d(w / S)/dw: (G_k - sum_j G_j phi_j) / S; with S replaced by 1 (a zero row sum) it is G_k
  double dot = 0.0;
  for (int i = 0; i < M; ++i) dot += (double)g[(long long)i * N] * (double)ph[(long long)i * N];
  const double shift = replaced ? 0.0 : dot;
  const double inv_s = replaced ? 1.0 : 1.0 / (double)sums[(long long)b * N + nn];
  auto cotangent = [&](int i) {   // dL/dw_i of the row before the division
    double v = ((double)g[(long long)i * N] - shift) * inv_s;
    if (gr) v += (double)gr[(long long)i * N];
    return dead ? 0.0 : v;
  };

  // a row on an edge: w_i = 1 - S' at the far vertex of every on-edge pair, so dL/dS' = -(the sum of their cotangents)
  const bool wave_edge = __ballot(edge_row) != 0ull;
  double d_sp = 0.0;
  if (wave_edge) {
    double acc = 0.0;
    walk(px, py, M, qx, qy, [&](int i, const Vtx&, const Vtx&, const Pair&, const Pair& prev) {
      acc += prev.edge ? cotangent(i) : 0.0;
    });
    d_sp = edge_row ? -acc : 0.0;
  }

  T* dv = part + ((long long)b * tiles + tile) * M * 2;
  double gqx = 0.0, gqy = 0.0;                 // dL/dq = -sum_i dL/ds_i
  double csx = 0.0, csy = 0.0;                 // what pair i-1 gives to s_i
  double cpx = 0.0, cpy = 0.0;                 // what edge i-1's length gives to p_i
  double w_cur = cotangent(0);
  walk(px, py, M, qx, qy, [&](int i, const Vtx& a, const Vtx& b2, const Pair& pr, const Pair& prev) {
    const double w_next = cotangent(i + 1 == M ? 0 : i + 1);
    const double den0 = a.r + kTiny, den1 = b2.r + kTiny;
    double ir0 = 1.0 / (a.r > 0.0 ? a.r : 1.0), ir1 = 1.0 / (b2.r > 0.0 ? b2.r : 1.0);
    ir0 = a.r > 0.0 ? ir0 : 0.0;               // a norm at 0 has derivative 0
    ir1 = b2.r > 0.0 ? ir1 : 0.0;
    // the plain row: w_i = (t_{i-1} + t_i) / (r_i + 1e-10), t_i = (r_i r_{i+1} - D_i) / (A_i + 1e-10) where |A_i| > 1e-5
    const double gt = plain_row && pr.big ? w_cur / den0 + w_next / den1 : 0.0;
    const double ia = 1.0 / (pr.big ? pr.A + kTiny : 1.0);
    const double gd = -gt * ia;                          // dL/dD_i
    const double ha = -gt * pr.t * ia * 0.5;             // dL/dA_i / 2
    const double wi = (prev.t + pr.t) / den0;
    double gr0 = gt * b2.r * ia + (plain_row ? -w_cur * wi / den0 : 0.0);   // dL/dr_i from pair i and from w_i
    const double gr1 = gt * a.r * ia;                    // dL/dr_{i+1} from pair i
    double px0 = 0.0, py0 = 0.0;                         // dL/dp_i through the length of edge i
    if (wave_edge) {
      // the on-edge row: e_i = 1 - r_i / (|p_i - p_{i+1}| + 1e-10) where pair i is on-edge, kept unless pair i-1 is too
      const double ge = edge_row && pr.edge ? d_sp + (prev.edge ? 0.0 : w_cur) : 0.0;
      const double ex = a.px - b2.px, ey = a.py - b2.py;
      const double len = norm2(ex, ey);
      const double il = 1.0 / (len + kTiny);
      gr0 += -ge * il;
      double ill = 1.0 / (len > 0.0 ? len : 1.0);
      ill = len > 0.0 ? ill : 0.0;
      const double gl = ge * a.r * il * il * ill;        // dL/dlen / len
      px0 = gl * ex;
      py0 = gl * ey;
    }
    double sx = csx + gd * b2.x + ha * b2.y + gr0 * a.x * ir0;   // dL/ds_i, complete
    double sy = csy + gd * b2.y - ha * b2.x + gr0 * a.y * ir0;
    sx = dead ? 0.0 : sx;
    sy = dead ? 0.0 : sy;
    double vx = sx + cpx + px0, vy = sy + cpy + py0;             // dL/dp_i of this query
    vx = dead ? 0.0 : vx;
    vy = dead ? 0.0 : vy;
    gqx -= sx;
    gqy -= sy;
    const T rx = wave_sum((T)vx), ry = wave_sum((T)vy);
    if (lane == 0) {
      dv[(long long)i * 2] = rx;
      dv[(long long)i * 2 + 1] = ry;
    }
    csx = gd * a.x - ha * a.y + gr1 * b2.x * ir1;
    csy = gd * a.y + ha * a.x + gr1 * b2.y * ir1;
    cpx = -px0;
    cpy = -py0;
    w_cur = w_next;
  });
  // pair M-1 closes the polygon: what it gives to vertex 0 is added to the slice's entry by the lane that wrote it
  csx = dead ? 0.0 : csx;
  csy = dead ? 0.0 : csy;
  const double tx = dead ? 0.0 : csx + cpx, ty = dead ? 0.0 : csy + cpy;
  gqx -= csx;
  gqy -= csy;
  const T rx = wave_sum((T)tx), ry = wave_sum((T)ty);
  if (lane == 0) {
    dv[0] += rx;
    dv[1] += ry;
  }
  if (live) {
    T* go = gpoints + (long long)b * 2 * N;
    go[n] = (T)gqx;
    go[(long long)N + n] = (T)gqy;
  }
}

// dL/dpolygon (B,2,M) = the workgroups' slices (M,2) of batch element b, added in workgroup order
template <typename T>
__global__ void mvc2d_reduce_kernel(const T* __restrict__ part, T* __restrict__ gpolygon, long long total, int M,
                                    int tiles) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long long b = idx / (2LL * M);
  const long long rem = idx - b * 2LL * M;
  const int a = (int)(rem / M);
  const int i = (int)(rem - (long long)a * M);
  T s = T(0);
  for (int t = 0; t < tiles; ++t) s += part[((b * tiles + t) * M + i) * 2 + a];
  gpolygon[idx] = s;
}

template <typename T>
int forward(const T* points, const T* polygon, T* phi, T* w, T* sums, int* codes, int B, int N, int M, void* stream) {
  if (bad_sizes(B, N, M, 0)) return PP_EINVAL;
  if (B == 0 || N == 0 || M == 0) return PP_OK;
  if (!points || !polygon || !phi || !sums || !codes) return PP_EINVAL;
  const int tiles = tiles_of(N);
  if ((long long)B * tiles > INT_MAX) return PP_EINVAL;
  mvc2d_forward_kernel<T><<<dim3((unsigned)(B * tiles)), dim3(kWave), 0, (hipStream_t)stream>>>(
      points, polygon, phi, w, sums, codes, N, M, tiles);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

template <typename T>
int backward(const T* points, const T* polygon, const T* phi, const T* sums, const int* codes, const T* gphi,
             const T* gw, T* gpoints, T* gpolygon, int B, int N, int M, void* ws, size_t ws_bytes, void* stream) {
  if (bad_sizes(B, N, M, 0)) return PP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (B == 0 || (N == 0 && M == 0)) return PP_OK;
  if (N == 0) {                                      // no query: the polygon's gradient is zero
    if (!gpolygon) return PP_EINVAL;
    return (int)pp::fill_bytes(gpolygon, 0, (size_t)B * 2 * M * sizeof(T), st);
  }
  if (M == 0) {                                      // no vertex: the points' gradient is zero
    if (!gpoints) return PP_EINVAL;
    return (int)pp::fill_bytes(gpoints, 0, (size_t)B * 2 * N * sizeof(T), st);
  }
  if (!points || !polygon || !phi || !sums || !codes || !gphi || !gpoints || !gpolygon) return PP_EINVAL;
  const int tiles = tiles_of(N);
  if ((long long)B * tiles > INT_MAX) return PP_EINVAL;
  if (!ws || ws_bytes < workspace_bytes(B, N, M, 2, (int)sizeof(T))) return PP_EINVAL;
  T* part = (T*)ws;
  mvc2d_backward_kernel<T><<<dim3((unsigned)(B * tiles)), dim3(kWave), 0, st>>>(points, polygon, phi, sums, codes,
                                                                                 gphi, gw, gpoints, part, N, M, tiles);
  PP_RETURN_IF_LAUNCH_FAILED();
  const long long total = (long long)B * 2 * M;
  mvc2d_reduce_kernel<T><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(part, gpolygon, total, M, tiles);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

}  // namespace

extern "C" size_t pp_mvc2d_workspace_bytes(int B, int N, int M, int elem_bytes) {
  if (elem_bytes != 4 && elem_bytes != 8) return 0;
  return workspace_bytes(B, N, M, 2, elem_bytes);
}

extern "C" int pp_mvc2d_forward_f32(const float* points, const float* polygon, float* phi, float* w, float* sums,
                                    int* codes, int B, int N, int M, void* stream) {
  return forward<float>(points, polygon, phi, w, sums, codes, B, N, M, stream);
}

extern "C" int pp_mvc2d_forward_f64(const double* points, const double* polygon, double* phi, double* w, double* sums,
                                    int* codes, int B, int N, int M, void* stream) {
  return forward<double>(points, polygon, phi, w, sums, codes, B, N, M, stream);
}

extern "C" int pp_mvc2d_backward_f32(const float* points, const float* polygon, const float* phi, const float* sums,
                                     const int* codes, const float* grad_phi, const float* grad_w, float* grad_points,
                                     float* grad_polygon, int B, int N, int M, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return backward<float>(points, polygon, phi, sums, codes, grad_phi, grad_w, grad_points, grad_polygon, B, N, M,
                         workspace, workspace_bytes, stream);
}

extern "C" int pp_mvc2d_backward_f64(const double* points, const double* polygon, const double* phi,
                                     const double* sums, const int* codes, const double* grad_phi,
                                     const double* grad_w, double* grad_points, double* grad_polygon, int B, int N,
                                     int M, void* workspace, size_t workspace_bytes, void* stream) {
  return backward<double>(points, polygon, phi, sums, codes, grad_phi, grad_w, grad_points, grad_polygon, B, N, M,
                          workspace, workspace_bytes, stream);
}
