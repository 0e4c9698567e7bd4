// green2d.hip -- Green coordinates of 2-D query points with respect to a closed polygonal cage given as directed edges
// (Lipman, Levin and Cohen-Or, "Green Coordinates", 2008, the closed form of Algorithm 1), forward and backward, fp32
// and fp64.  Contract: DESIGN.md "Green coordinates, 2-D" (the reference declares green_coordinates_2D and leaves it
// empty, network/geo_operations.py:622).
//
// Layout (as green.hip): one workgroup = one wave = 64 queries of one batch element, one query per lane; the wave walks
// the edges in order, so an edge's indices and endpoints are wave-uniform loads.  Every (query, edge) pair is evaluated
// in fp64 for either data type.  Each lane owns the fp64 accumulator row of its query's vertex coordinates as a column
// of LDS, acc[v * 65 + lane] (v is wave-uniform: no bank conflicts; the stride 65 keeps the transposed, coalesced
// write-out free of conflicts too), rounded once to the output type at the write-out.  A cage with more vertices than
// LDS holds columns for is served in chunks of that many vertices: the wave walks the edge list once per chunk and
// evaluates the edges with an end in the chunk, so a vertex receives the same terms in the same order whatever the
// chunk size, and its coordinate is the same bits.  (An accumulator row in the output's own type in global memory
// would round every partial sum of an fp32 row to fp32.)  psi is staged in an LDS tile of 64 edges and written as
// whole row segments during the first walk.  A query's row does not depend on P, its position or the batch size.
//
// Backward: every pair is evaluated again and differentiated by hand (reverse mode through the closed form; a term
// that a rule of the contract takes as 0 has derivative 0).  dL/dquery is summed in registers; the two edge-end
// gradients of an edge are summed over the wave (fixed xor butterfly) and written by one lane into the workgroup's
// slice of the workspace; a second kernel adds the slices of a batch element in workgroup order; a third, one thread
// per vertex, collects the vertex's edge ends in ascending edge order (a scan of all F edges per vertex: cages are
// small).  No floating-point atomics anywhere: every output is reproducible bit for bit.
#include <math.h>

#include "cage_common.h"

using namespace pp::cage;

namespace {

constexpr double kPi = 3.14159265358979323846;
// code bits of a query row
constexpr int kNonFinite = 1, kBadIndex = 8;

// edge j as the pair evaluation takes it: reversed where the given normal points against the edge's own
struct Edge {
  int i1, i2;
  bool flip;
  double x1, y1, x2, y2;
};

template <typename T>
__device__ __forceinline__ Edge load_edge(const long long* fb, const T* vtx, const T* en, int j) {
  Edge E;
  E.i1 = (int)fb[(long long)j * 2];
  E.i2 = (int)fb[(long long)j * 2 + 1];
  E.x1 = (double)vtx[(long long)E.i1 * 2];
  E.y1 = (double)vtx[(long long)E.i1 * 2 + 1];
  E.x2 = (double)vtx[(long long)E.i2 * 2];
  E.y2 = (double)vtx[(long long)E.i2 * 2 + 1];
  E.flip = false;
  if (en) {
    const double ax = E.x2 - E.x1, ay = E.y2 - E.y1;
    E.flip = (double)en[(long long)j * 2] * ay - (double)en[(long long)j * 2 + 1] * ax < 0.0;
  }
  if (E.flip) {
    const int i = E.i1;
    E.i1 = E.i2;
    E.i2 = i;
    const double x = E.x1, y = E.y1;
    E.x1 = E.x2;
    E.y1 = E.y2;
    E.x2 = x;
    E.y2 = y;
  }
  return E;
}

// One (query, edge) pair, DESIGN.md's formulas in their order.  psi: the edge's coordinate; p1, p2: the terms of the
// vertex coordinates of v1 and v2.  An edge of length 0 (dead) gives zeros.
struct Pair {
  double ax, ay, bx, by, ex, ey;
  double Q, R, S, T, c, d, th, ln_t, ln_s, r, u, g, h, sq, M;
  bool dead, cz;
  double psi, p1, p2;
};

__device__ __forceinline__ Pair eval_pair(const Edge& E, double qx, double qy) {
  Pair p;
  p.ax = E.x2 - E.x1;
  p.ay = E.y2 - E.y1;
  p.bx = E.x1 - qx;
  p.by = E.y1 - qy;
  p.ex = E.x2 - qx;
  p.ey = E.y2 - qy;
  p.Q = p.ax * p.ax + p.ay * p.ay;
  p.S = p.bx * p.bx + p.by * p.by;
  p.T = p.ex * p.ex + p.ey * p.ey;
  p.R = 2.0 * (p.ax * p.bx + p.ay * p.by);
  p.c = p.ax * p.by - p.ay * p.bx;
  p.d = p.bx * p.ex + p.by * p.ey;
  p.dead = p.Q == 0.0;
  const double Q = p.dead ? 1.0 : p.Q;
  p.cz = p.c == 0.0;
  p.th = p.cz ? 0.0 : atan2(p.c, p.d);
  p.ln_t = p.T == 0.0 ? 0.0 : log(p.T);       // x ln 0 := 0: ln 0 is taken as 0 (x is 0 there)
  p.ln_s = p.S == 0.0 ? 0.0 : log(p.S);
  p.r = p.R / Q;
  p.u = 1.0 + p.r / 2.0;
  const double L = p.u * p.ln_t + (1.0 - p.u) * p.ln_s;
  p.g = p.cz ? 0.0 : p.c * (p.ln_t - p.ln_s) / (2.0 * Q);
  p.h = p.th / 2.0;
  p.sq = sqrt(Q);
  p.M = 2.0 * p.c * p.th / Q + L - 2.0;
  p.psi = -p.sq / (4.0 * kPi) * p.M;
  p.p1 = (p.g - p.h * (2.0 + p.r)) / (2.0 * kPi);
  p.p2 = (p.h * p.r - p.g) / (2.0 * kPi);
  if (p.dead) p.psi = p.p1 = p.p2 = 0.0;
  return p;
}

__device__ __forceinline__ bool finite3(double a, double b, double c) {
  return fabs(a) < INFINITY && fabs(b) < INFINITY && fabs(c) < INFINITY;
}

// LDS: acc (fp64, chunk columns), then the psi tile of 64 edges (T).  The prologue and the two transposes are written
// out here: on cage_common.h's helpers this kernel's fp64 form measured 1 % slower (profiles/cage_common/).
template <typename T>
__global__ __launch_bounds__(kWave) void gc2d_forward_kernel(
    const T* __restrict__ query, const T* __restrict__ vertices, const long long* __restrict__ faces, long long fsb,
    const T* __restrict__ normals, T* __restrict__ phi, T* __restrict__ psi, unsigned char* __restrict__ exterior,
    int* __restrict__ codes, int P, int N, int F, int chunk) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x, b = blockIdx.y;
  const int p0 = blockIdx.x * kWave, p = p0 + lane;
  const int rows = min(kWave, P - p0);
  const bool live = p < P;
  const long long row = (long long)b * P + (live ? p : P - 1);
  double* acc = (double*)smem;                                 // acc[v * 65 + lane], v in the chunk
  T* tile = (T*)(acc + (long long)chunk * kStride);            // tile[fi * 65 + lane]
  const T* vtx = vertices + (long long)b * N * 2;
  const T* en = normals ? normals + (long long)b * F * 2 : nullptr;
  const long long* fb = faces + (long long)b * fsb;
  if (!faces_ok<2>(fb, F, N)) {                                // the whole batch element: NaN rows
    if (live) {
      for (int j = 0; j < N; ++j) phi[row * N + j] = m_nan(T(0));
      for (int f = 0; f < F; ++f) psi[row * F + f] = m_nan(T(0));
      exterior[row] = 0;
      codes[row] = kBadIndex;
    }
    return;
  }
  const double qx = (double)query[row * 2], qy = (double)query[row * 2 + 1];
  bool bad = false;
  double sum = 0.0;
  for (int v0 = 0; v0 < N; v0 += chunk) {
    const int cn = min(chunk, N - v0);
    const bool first = v0 == 0;                                // the walk that also gives psi and the row's code
    for (int j = 0; j < cn; ++j) acc[j * kStride + lane] = 0.0;
    for (int f0 = 0; f0 < F; f0 += kWave) {
      const int nf = min(kWave, F - f0);
      for (int fi = 0; fi < nf; ++fi) {
        const Edge E = load_edge(fb, vtx, en, f0 + fi);
        const bool in1 = E.i1 >= v0 && E.i1 < v0 + cn, in2 = E.i2 >= v0 && E.i2 < v0 + cn;
        if (!(first || in1 || in2)) continue;                  // wave-uniform
        const Pair pr = eval_pair(E, qx, qy);
        if (first) {
          tile[fi * kStride + lane] = (T)pr.psi;
          bad = bad || !finite3(pr.psi, pr.p1, pr.p2);
        }
        if (in1) acc[(E.i1 - v0) * kStride + lane] += pr.p1;
        if (in2) acc[(E.i2 - v0) * kStride + lane] += pr.p2;
      }
      if (first) {
        __syncthreads();
        for (int r = 0; r < rows; ++r)
          if (lane < nf) psi[((long long)b * P + p0 + r) * F + f0 + lane] = tile[lane * kStride + r];
        __syncthreads();
      }
    }
    for (int j = 0; j < cn; ++j) sum += acc[j * kStride + lane];
    if (bad)
      for (int j = 0; j < cn; ++j) acc[j * kStride + lane] = m_nan(0.0);
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      T* o = phi + ((long long)b * P + p0 + r) * N + v0;
      for (int j = lane; j < cn; j += kWave) o[j] = (T)acc[j * kStride + r];
    }
    __syncthreads();
  }
  if (live) {
    if (bad)                                                   // (behind the barrier that follows the tiles' stores)
      for (int f = 0; f < F; ++f) psi[row * F + f] = m_nan(T(0));
    exterior[row] = (!bad && sum < 0.5) ? 1 : 0;
    codes[row] = bad ? kNonFinite : 0;
  }
}

// dL/d(v1, v2) of one pair into gv (x1, y1, x2, y2), -dL/dquery's share subtracted from gq: w1, w2, wp the
// cotangents of p1, p2 and psi.  Reverse mode through eval_pair; a, b, e are taken as functions of v1, v2 and the
// query (a = v2 - v1, b = v1 - q, e = v2 - q).
__device__ __forceinline__ void pair_grad(const Pair& p, double w1, double w2, double wp, double gv[4], double gq[2]) {
  const double k = 1.0 / (2.0 * kPi);
  const double Q = p.Q;                                          // the caller skips a dead pair
  const double D = p.ln_t - p.ln_s;
  const double g_g = p.cz ? 0.0 : k * (w1 - w2);
  const double g_h = k * (w2 * p.r - w1 * (2.0 + p.r));
  double g_r = k * p.h * (w2 - w1);
  const double g_M = -wp * p.sq / (4.0 * kPi);
  double g_Q = -wp * p.M / (4.0 * kPi) / (2.0 * p.sq);           // through sqrt(Q)
  double g_c = g_M * 2.0 * p.th / Q;
  double g_th = g_M * 2.0 * p.c / Q + g_h / 2.0;
  g_Q -= g_M * 2.0 * p.c * p.th / (Q * Q);
  // g = c D / (2Q)
  g_c += g_g * D / (2.0 * Q);
  const double g_D = g_g * p.c / (2.0 * Q);
  g_Q -= g_g * p.g / Q;
  // L = u ln T + (1 - u) ln S
  const double g_u = g_M * D;
  const double g_lt = g_M * p.u + g_D, g_ls = g_M * (1.0 - p.u) - g_D;
  const double g_T = p.T == 0.0 ? 0.0 : g_lt / p.T;
  const double g_S = p.S == 0.0 ? 0.0 : g_ls / p.S;
  g_r += g_u / 2.0;
  const double g_R = g_r / Q;
  g_Q -= g_r * p.r / Q;
  // th = atan2(c, d), taken as 0 where c == 0
  double g_d = 0.0;
  if (!p.cz) {
    const double den = p.c * p.c + p.d * p.d;
    g_c += g_th * p.d / den;
    g_d = -g_th * p.c / den;
  }
  const double gax = 2.0 * g_Q * p.ax + 2.0 * g_R * p.bx + g_c * p.by;
  const double gay = 2.0 * g_Q * p.ay + 2.0 * g_R * p.by - g_c * p.bx;
  const double gbx = 2.0 * g_S * p.bx + 2.0 * g_R * p.ax - g_c * p.ay + g_d * p.ex;
  const double gby = 2.0 * g_S * p.by + 2.0 * g_R * p.ay + g_c * p.ax + g_d * p.ey;
  const double gex = 2.0 * g_T * p.ex + g_d * p.bx;
  const double gey = 2.0 * g_T * p.ey + g_d * p.by;
  gv[0] = gbx - gax;
  gv[1] = gby - gay;
  gv[2] = gex + gax;
  gv[3] = gey + gay;
  gq[0] -= gbx + gex;
  gq[1] -= gby + gey;
}

// LDS: the tile of dL/dpsi of 64 edges (T), then (LDS) the rows of dL/dphi, a column per lane
template <typename T, bool LDS>
__global__ __launch_bounds__(kWave) void gc2d_backward_kernel(
    const T* __restrict__ query, const T* __restrict__ vertices, const long long* __restrict__ faces, long long fsb,
    const T* __restrict__ normals, const int* __restrict__ codes, const T* __restrict__ gphi,
    const T* __restrict__ gpsi, T* __restrict__ gq, T* __restrict__ part, int P, int N, int F) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auto [lane, b, p0, p, rows, live, row] = tile_of(P);
  const int tiles = gridDim.x;
  T* tile = (T*)smem;                                          // tile[fi * 65 + lane]
  T* gcol = tile + kWave * kStride;                            // gcol[v * 65 + lane]
  T* out = part + ((long long)b * tiles + blockIdx.x) * F * 4;
  const T* vtx = vertices + (long long)b * N * 2;
  const T* en = normals ? normals + (long long)b * F * 2 : nullptr;
  const long long* fb = faces + (long long)b * fsb;
  if (codes[(long long)b * P] & kBadIndex) {                   // the whole batch element (gc2d_collect_kernel: NaN)
    if (live) gq[row * 2] = gq[row * 2 + 1] = m_nan(T(0));
    return;
  }
  if (LDS && gphi) {
    rows_to_columns(gphi, (long long)b * P + p0, N, rows, N, lane, gcol);
    __syncthreads();
  }
  const T* grow = LDS ? gcol + lane : (gphi ? gphi + row * N : nullptr);
  const long long gs = LDS ? kStride : 1;
  const double qx = (double)query[row * 2], qy = (double)query[row * 2 + 1];
  double gqa[2] = {0.0, 0.0};
  for (int f0 = 0; f0 < F; f0 += kWave) {
    const int nf = min(kWave, F - f0);
    if (gpsi) {
      __syncthreads();
      tile_in(tile, rows, nf, lane, gpsi + f0, (long long)b * P + p0, F);
      __syncthreads();
    }
    for (int fi = 0; fi < nf; ++fi) {
      const int f = f0 + fi;
      const Edge E = load_edge(fb, vtx, en, f);
      const Pair pr = eval_pair(E, qx, qy);
      double gv[4] = {0.0, 0.0, 0.0, 0.0};
      if (live && !pr.dead) {
        const double w1 = gphi ? (double)grow[E.i1 * gs] : 0.0, w2 = gphi ? (double)grow[E.i2 * gs] : 0.0;
        const double wp = gpsi ? (double)tile[fi * kStride + lane] : 0.0;
        pair_grad(pr, w1, w2, wp, gv, gqa);
      }
      wave_sum(gv);
      if (lane == 0) {                                         // in the order of the edge's row of faces
        const int s1 = E.flip ? 2 : 0, s2 = E.flip ? 0 : 2;
        out[(long long)f * 4 + s1] = (T)gv[0];
        out[(long long)f * 4 + s1 + 1] = (T)gv[1];
        out[(long long)f * 4 + s2] = (T)gv[2];
        out[(long long)f * 4 + s2 + 1] = (T)gv[3];
      }
    }
  }
  if (live) {
    gq[row * 2] = (T)gqa[0];
    gq[row * 2 + 1] = (T)gqa[1];
  }
}

// the workgroups' slices (F,4) of batch element b, added in workgroup order into its first slice
template <typename T>
__global__ void gc2d_reduce_kernel(T* __restrict__ part, const int* __restrict__ codes, int B, int P, int F,
                                   int tiles) {
  const long long f4 = (long long)F * 4;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * f4) return;
  const long long b = i / f4, k = i - b * f4;
  if (codes[b * P] & kBadIndex) return;
  T s = T(0);
  for (int t = 0; t < tiles; ++t) s += part[(b * tiles + t) * f4 + k];
  part[b * tiles * f4 + k] = s;
}

// dL/dvertices[b, v] = the edge ends at v, in ascending edge order (an edge's first end before its second); NaN for a
// batch element whose edge list holds an out-of-range index
template <typename T>
__global__ void gc2d_collect_kernel(const T* __restrict__ part, const long long* __restrict__ faces, long long fsb,
                                    const int* __restrict__ codes, T* __restrict__ gv, int B, int P, int N, int F,
                                    int tiles) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * N) return;
  const long long b = i / N, v = i - b * N;
  if (codes[b * P] & kBadIndex) {
    gv[i * 2] = gv[i * 2 + 1] = m_nan(T(0));
    return;
  }
  const long long* fb = faces + b * fsb;
  const T* e = part + b * tiles * (long long)F * 4;
  T sx = T(0), sy = T(0);
  for (int j = 0; j < F; ++j) {
    if (fb[(long long)j * 2] == v) {
      sx += e[(long long)j * 4];
      sy += e[(long long)j * 4 + 1];
    }
    if (fb[(long long)j * 2 + 1] == v) {
      sx += e[(long long)j * 4 + 2];
      sy += e[(long long)j * 4 + 3];
    }
  }
  gv[i * 2] = sx;
  gv[i * 2 + 1] = sy;
}

template <typename T>
constexpr size_t tile_bytes() {
  return (size_t)kWave * kStride * sizeof(T);
}
// the most vertices whose accumulator columns fit beside the psi tile in `limit` bytes of LDS
template <typename T>
constexpr int chunk_cap(size_t limit) {
  return (int)((limit - tile_bytes<T>()) / (kStride * sizeof(double)));
}

template <typename T>
int forward(const T* query, const T* vertices, const long long* faces, long long fsb, const T* normals, T* phi, T* psi,
            unsigned char* exterior, int* codes, int B, int P, int N, int F, void* stream) {
  if (bad_sizes(B, P, N, F) || fsb < 0) return PP_EINVAL;
  if ((long long)B * P == 0) return PP_OK;
  if (!grid_ok(B)) return PP_EINVAL;
  if (!query || !exterior || !codes || (N > 0 && (!vertices || !phi)) || (F > 0 && (!faces || !psi))) return PP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles_of(P), (unsigned)B);
  static pp::DeviceFlags flags;
  int chunk = N < 1 ? 1 : (N < chunk_cap<T>(kMaxLds) ? N : chunk_cap<T>(kMaxLds));
  size_t lds = (size_t)chunk * kStride * sizeof(double) + tile_bytes<T>();
  if (lds > 65536 && pp::allow_big_lds(gc2d_forward_kernel<T>, kMaxLds, flags) != hipSuccess) {
    chunk = chunk_cap<T>(65536);
    lds = (size_t)chunk * kStride * sizeof(double) + tile_bytes<T>();
  }
  gc2d_forward_kernel<T><<<grid, dim3(kWave), lds, st>>>(query, vertices, faces, fsb, normals, phi, psi, exterior,
                                                         codes, P, N, F, chunk);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

template <typename T>
int backward(const T* query, const T* vertices, const long long* faces, long long fsb, const T* normals,
             const int* codes, const T* gphi, const T* gpsi, T* gq, T* gv, int B, int P, int N, int F, void* ws,
             size_t ws_bytes, void* stream) {
  if (bad_sizes(B, P, N, F) || fsb < 0) return PP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if ((long long)B * N > 0 && !gv) return PP_EINVAL;
  if ((long long)B * P > 0 && !gq) return PP_EINVAL;
  if ((long long)B * P == 0 || F == 0) {                        // no pair: the gradients are zero
    hipError_t e = pp::fill_bytes(gv, 0, (size_t)B * N * 2 * sizeof(T), st);
    if (e == hipSuccess) e = pp::fill_bytes(gq, 0, (size_t)B * P * 2 * sizeof(T), st);
    return (int)e;
  }
  if (!grid_ok(B)) return PP_EINVAL;
  const size_t need = workspace_bytes(B, P, F, 4, (int)sizeof(T));
  if (!query || !codes || !faces || (N > 0 && !vertices) || !ws || ws_bytes < need) return PP_EINVAL;
  T* part = (T*)ws;
  const int tiles = tiles_of(P);
  const dim3 grid((unsigned)tiles, (unsigned)B);
  static pp::DeviceFlags flags;
  const size_t tile = tile_bytes<T>(), lds = tile + (size_t)N * kStride * sizeof(T);
  if (lds_fits(gc2d_backward_kernel<T, true>, lds, flags))
    gc2d_backward_kernel<T, true><<<grid, dim3(kWave), lds, st>>>(query, vertices, faces, fsb, normals, codes, gphi,
                                                                   gpsi, gq, part, P, N, F);
  else
    gc2d_backward_kernel<T, false><<<grid, dim3(kWave), tile, st>>>(query, vertices, faces, fsb, normals, codes, gphi,
                                                                     gpsi, gq, part, P, N, F);
  PP_RETURN_IF_LAUNCH_FAILED();
  const long long n = (long long)B * F * 4;
  gc2d_reduce_kernel<T><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(part, codes, B, P, F, tiles);
  PP_RETURN_IF_LAUNCH_FAILED();
  if ((long long)B * N > 0) {
    const long long m = (long long)B * N;
    gc2d_collect_kernel<T><<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st>>>(part, faces, fsb, codes, gv, B, P,
                                                                                    N, F, tiles);
    PP_RETURN_IF_LAUNCH_FAILED();
  }
  return PP_OK;
}

}  // namespace

extern "C" size_t pp_gc2d_workspace_bytes(int B, int P, int F, int elem_bytes) {
  if (elem_bytes != 4 && elem_bytes != 8) return 0;
  return workspace_bytes(B, P, F, 4, elem_bytes);
}

extern "C" int pp_gc2d_forward_f32(const float* query, const float* vertices, const long long* faces,
                                   long long faces_batch_stride, const float* edge_normals, float* phi, float* psi,
                                   unsigned char* exterior, int* codes, int B, int P, int N, int F, void* stream) {
  return forward<float>(query, vertices, faces, faces_batch_stride, edge_normals, phi, psi, exterior, codes, B, P, N, F,
                        stream);
}

extern "C" int pp_gc2d_forward_f64(const double* query, const double* vertices, const long long* faces,
                                   long long faces_batch_stride, const double* edge_normals, double* phi, double* psi,
                                   unsigned char* exterior, int* codes, int B, int P, int N, int F, void* stream) {
  return forward<double>(query, vertices, faces, faces_batch_stride, edge_normals, phi, psi, exterior, codes, B, P, N,
                         F, stream);
}

extern "C" int pp_gc2d_backward_f32(const float* query, const float* vertices, const long long* faces,
                                    long long faces_batch_stride, const float* edge_normals, const int* codes,
                                    const float* grad_phi, const float* grad_psi, float* grad_query,
                                    float* grad_vertices, int B, int P, int N, int F, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return backward<float>(query, vertices, faces, faces_batch_stride, edge_normals, codes, grad_phi, grad_psi,
                         grad_query, grad_vertices, B, P, N, F, workspace, workspace_bytes, stream);
}

extern "C" int pp_gc2d_backward_f64(const double* query, const double* vertices, const long long* faces,
                                    long long faces_batch_stride, const double* edge_normals, const int* codes,
                                    const double* grad_phi, const double* grad_psi, double* grad_query,
                                    double* grad_vertices, int B, int P, int N, int F, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return backward<double>(query, vertices, faces, faces_batch_stride, edge_normals, codes, grad_phi, grad_psi,
                          grad_query, grad_vertices, B, P, N, F, workspace, workspace_bytes, stream);
}
