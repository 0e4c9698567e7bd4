// green.hip -- Green coordinates of query points with respect to a closed triangle cage (Lipman, Levin and Cohen-Or,
// "Green Coordinates", 2008), forward and backward, fp32 and fp64.
// Contract: DESIGN.md "Green coordinates" (reference network/geo_operations.py:625-773 and its _gcTriInt).
//
// Layout (as mvc.hip): one workgroup = one wave = 64 queries of one batch element; the whole wave walks the faces in
// order, so a face's indices, corners and normal are wave-uniform loads.  Each lane owns the accumulator row of its
// query's vertex coordinates:
//   fast path   a column of LDS, acc[v * 65 + lane] (v is wave-uniform: no bank conflicts; the stride 65 keeps the
//               transposed, coalesced write-out free of conflicts too);
//   general     the query's own output row in global memory (any N).
// The face coordinates of 64 faces are staged in an LDS tile on both paths and written as whole row segments.  Both
// paths perform the same operations in the same order: a query's row is the same bits on either, and does not depend
// on P, its position or the batch size.
//
// Every (query, face) pair is evaluated in fp64 for either data type, literally as the reference's chain (its clamps
// and filters in its order; the fp32 chain loses up to ~5e-4).  The backward evaluates every pair again on dual numbers
// (forward-mode derivatives in the query and the face normal, DUAL_K of them per pass) with torch's conventions at the
// kinks: a clamp passes the derivative on its closed interval, |x| has derivative sign(x), sign() and filtered values
// have none, a norm has none at 0; a discarded branch is never evaluated, so where the reference's gradient is NaN
// (0/0 of an unselected torch.where branch, a query on a vertex) this one is that of the branch taken.  dL/dquery is
// summed in registers; dL/dnormal of a face is summed over the wave (fixed xor butterfly) and written by one lane into
// the workgroup's slice of the workspace; a second kernel adds the slices of a batch element in workgroup order.  No
// floating-point atomics anywhere: every output is reproducible bit for bit.
#include <math.h>

#include "cage_common.h"

using namespace pp::cage;

namespace {

#ifndef GC_DUAL_K
#define GC_DUAL_K 3
#endif
constexpr int kDualK = GC_DUAL_K;           // derivatives carried per backward pass (query, then normal)

// _gcTriInt's constants and those of the pair (reference geo_operations.py)
constexpr double kPi = 3.141592653589793;   // np.pi
constexpr double kEps = 1e-6, kAngleEps = 1e-3, kDivGuard = 1e-12;
constexpr double kNEps = 1e-7, kOmegaEps = 1e-6, kPhiGuard = 1e-10;

// ------------------------------------------------------------------------------------------ scalars and duals
template <int K>
struct Dual {
  double v, d[K];
};

__device__ __forceinline__ double val(double x) { return x; }
template <int K>
__device__ __forceinline__ double val(const Dual<K>& x) {
  return x.v;
}

template <int K>
__device__ __forceinline__ Dual<K> dconst(double c) {
  Dual<K> r;
  r.v = c;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = 0.0;
  return r;
}
// y = f(x) with f'(x) = s
template <int K>
__device__ __forceinline__ Dual<K> chain(const Dual<K>& x, double y, double s) {
  Dual<K> r;
  r.v = y;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = s * x.d[i];
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator+(const Dual<K>& a, const Dual<K>& b) {
  Dual<K> r;
  r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator-(const Dual<K>& a, const Dual<K>& b) {
  Dual<K> r;
  r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator-(const Dual<K>& a) {
  return chain(a, -a.v, -1.0);
}
template <int K>
__device__ __forceinline__ Dual<K> operator*(const Dual<K>& a, const Dual<K>& b) {
  Dual<K> r;
  r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator/(const Dual<K>& a, const Dual<K>& b) {
  Dual<K> r;
  r.v = a.v / b.v;
#pragma unroll
  for (int i = 0; i < K; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
  return r;
}
template <int K>
__device__ __forceinline__ Dual<K> operator+(const Dual<K>& a, double c) {
  return chain(a, a.v + c, 1.0);
}
template <int K>
__device__ __forceinline__ Dual<K> operator+(double c, const Dual<K>& a) {
  return chain(a, c + a.v, 1.0);
}
template <int K>
__device__ __forceinline__ Dual<K> operator-(double c, const Dual<K>& a) {
  return chain(a, c - a.v, -1.0);
}
template <int K>
__device__ __forceinline__ Dual<K> operator*(double c, const Dual<K>& a) {
  return chain(a, c * a.v, c);
}
template <int K>
__device__ __forceinline__ Dual<K> operator*(const Dual<K>& a, double c) {
  return chain(a, a.v * c, c);
}

__device__ __forceinline__ double g_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ double g_acos(double x) { return acos(x); }
__device__ __forceinline__ double g_sin(double x) { return sin(x); }
__device__ __forceinline__ double g_cos(double x) { return cos(x); }
__device__ __forceinline__ double g_atan(double x) { return atan(x); }
__device__ __forceinline__ double g_log(double x) { return log(x); }
__device__ __forceinline__ double g_abs(double x) { return fabs(x); }
__device__ __forceinline__ double g_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ double g_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x)); }

template <int K>
__device__ __forceinline__ Dual<K> g_sqrt(const Dual<K>& x) {
  const double y = sqrt(x.v);
  return chain(x, y, 0.5 / y);
}
template <int K>
__device__ __forceinline__ Dual<K> g_acos(const Dual<K>& x) {
  return chain(x, acos(x.v), -1.0 / sqrt(1.0 - x.v * x.v));
}
template <int K>
__device__ __forceinline__ Dual<K> g_sin(const Dual<K>& x) {
  double s, c;
  sincos(x.v, &s, &c);
  return chain(x, s, c);
}
template <int K>
__device__ __forceinline__ Dual<K> g_cos(const Dual<K>& x) {
  double s, c;
  sincos(x.v, &s, &c);
  return chain(x, c, -s);
}
template <int K>
__device__ __forceinline__ Dual<K> g_atan(const Dual<K>& x) {
  return chain(x, atan(x.v), 1.0 / (1.0 + x.v * x.v));
}
template <int K>
__device__ __forceinline__ Dual<K> g_log(const Dual<K>& x) {
  return chain(x, log(x.v), 1.0 / x.v);
}
template <int K>
__device__ __forceinline__ Dual<K> g_abs(const Dual<K>& x) {
  return chain(x, fabs(x.v), g_sign(x.v));
}
template <int K>
__device__ __forceinline__ Dual<K> g_clamp(const Dual<K>& x, double lo, double hi) {
  return chain(x, g_clamp(x.v, lo, hi), (x.v >= lo && x.v <= hi) ? 1.0 : 0.0);
}

template <typename S>
struct Zero {
  __device__ static __forceinline__ S get() { return 0.0; }
};
template <int K>
struct Zero<Dual<K>> {
  __device__ static __forceinline__ Dual<K> get() { return dconst<K>(0.0); }
};
template <typename S>
__device__ __forceinline__ S zero_like() {
  return Zero<S>::get();
}

template <typename S>
__device__ __forceinline__ S dot3(const S a[3], const S b[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
// |a|, with no derivative at 0 (torch's norm)
template <typename S>
__device__ __forceinline__ S norm3(const S a[3]) {
  const S q = dot3(a, a);
  if (val(q) == 0.0) return zero_like<S>();
  return g_sqrt(q);
}
template <typename S>
__device__ __forceinline__ void cross3(const S a[3], const S b[3], S r[3]) {
  r[0] = a[1] * b[2] - a[2] * b[1];
  r[1] = a[2] * b[0] - a[0] * b[2];
  r[2] = a[0] * b[1] - a[1] * b[0];
}

// ------------------------------------------------------------------------------------------ the pair
// _gcTriInt(p, v1, v2, None) for one edge
template <typename S>
__device__ __forceinline__ S tri_int(const S p[3], const S v1[3], const S v2[3]) {
  S p_v1[3], v2_p[3], v2_v1[3], m_p_v1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p_v1[a] = p[a] - v1[a];
    v2_p[a] = v2[a] - p[a];
    v2_v1[a] = v2[a] - v1[a];
    m_p_v1[a] = -p_v1[a];
  }
  const S pn = norm3(p_v1);
  S t = dot3(v2_v1, p_v1) / (pn * norm3(v2_v1) + kDivGuard);
  t = g_clamp(t, -1.0, 1.0);
  bool mask = fabs(val(t)) > 1.0 - kEps;
  const S alpha = g_acos(g_clamp(t, -1.0 + kEps, 1.0 - kEps));
  mask = mask || fabs(val(alpha) - kPi) < kAngleEps || fabs(val(alpha)) < kAngleEps;
  t = dot3(m_p_v1, v2_p) / (pn * norm3(v2_p) + kDivGuard);
  t = g_clamp(t, -1.0, 1.0);
  mask = mask || fabs(val(t)) > 1.0 - kEps;
  if (mask) return zero_like<S>();                  // the filter only grows: the result is a filtered 0
  const S beta = g_acos(g_clamp(t, -1.0 + kEps, 1.0 - kEps));
  const S ps = pn * g_sin(alpha);
  const S lambd = ps * ps;
  const S c = dot3(p, p);
  const S theta_1 = g_clamp(kPi - alpha, 0.0, kPi);
  const S theta_2 = g_clamp(kPi - alpha - beta, -kPi, kPi);
  const S C_1 = g_cos(theta_1), C_2 = g_cos(theta_2);
  if (fabs(val(C_1) - 1.0) < kEps || fabs(val(C_2) - 1.0) < kEps) return zero_like<S>();
  const S S_1 = g_sin(theta_1), S_2 = g_sin(theta_2);
  const S sqrt_c = g_sqrt(c + kDivGuard);
  const S sqrt_l = g_sqrt(lambd + kDivGuard);
  S I[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const S& Sk = k == 0 ? S_1 : S_2;
    const S& Ck = k == 0 ? C_1 : C_2;
    const S omc = 1.0 - Ck;
    const S sqcot = Sk * Sk / (omc * omc + kDivGuard);
    const S den = kDivGuard + c * (1.0 + Ck) + lambd + sqrt_l * g_sqrt(lambd + c * Sk * Sk + kDivGuard);
    S in_log = sqrt_l * (1.0 - 2.0 * c * Ck / den) * 2.0 * sqcot;
    if (val(in_log) <= 0.0) in_log = zero_like<S>() + 1.0;        // masked_fill(in_log <= 0, 1)
    const S at = g_atan((sqrt_c * Ck) / g_sqrt(lambd + Sk * Sk * c + kDivGuard));
    I[k] = (-0.5 * g_sign(val(Sk))) * (2.0 * sqrt_c * at + sqrt_l * g_log(in_log));
  }
  return (-1.0 / (4.0 * kPi)) * g_abs(I[0] - I[1] - sqrt_c * beta);
}

// One (query, face) pair: v = the face's corners minus the query, n its normal -> psi (GC_face) and phi (the corners'
// unnormalised GC_vertex terms)
template <typename S>
__device__ __forceinline__ void gc_pair(const S v[3][3], const S n[3], S& psi, S phi[3]) {
  const S d0 = dot3(v[0], n);
  S p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = d0 * n[a];
  // per edge: the sign s_l and whether |N_l| < 1e-7 (II_l filtered), on the values alone (no derivative flows through
  // either); kept as scalars and bits, which stay in registers where a dynamically selected array would not
  double sgn0 = 0.0, sgn1 = 0.0, sgn2 = 0.0;
  int small = 0;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int l1 = (l + 1) % 3;
    double x[3], y[3], nv[3], cr[3], a[3], b[3], nl[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      x[ax] = val(v[l][ax]) - val(p[ax]);
      y[ax] = val(v[l1][ax]) - val(p[ax]);
      nv[ax] = val(n[ax]);
      a[ax] = val(v[l1][ax]);
      b[ax] = val(v[l][ax]);
    }
    cross3(x, y, cr);
    const double sg = g_sign(dot3(cr, nv));
    if (l == 0) sgn0 = sg;
    if (l == 1) sgn1 = sg;
    if (l == 2) sgn2 = sg;
    cross3(a, b, nl);
    if (norm3(nl) < kNEps) small |= 1 << l;               // the same value as norm3 of the dual N_l below
  }
  // the six _gcTriInt evaluations, one at a time (a rolled loop: unrolled, the scheduler interleaves them and the
  // backward's duals no longer fit the register file); operands are picked with selects, never by a dynamic index
  S I = zero_like<S>(), II[3];
#pragma unroll 1
  for (int e = 0; e < 6; ++e) {
    const int l = e < 3 ? e : e - 3;
    const bool second = e >= 3;                     // II_l = _gcTriInt(0, v_{l+1}, v_l); else I_l = (p, v_l, v_{l+1})
    S o[3], a[3], c[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const S vl = l == 0 ? v[0][ax] : (l == 1 ? v[1][ax] : v[2][ax]);
      const S vl1 = l == 0 ? v[1][ax] : (l == 1 ? v[2][ax] : v[0][ax]);
      o[ax] = second ? zero_like<S>() : p[ax];
      a[ax] = second ? vl1 : vl;
      c[ax] = second ? vl : vl1;
    }
    const bool skip = second && ((small >> l) & 1);           // masked_fill(|N_l| < 1e-7, 0)
    const S r = skip ? zero_like<S>() : tri_int(o, a, c);
    if (!second) {
      const double s = l == 0 ? sgn0 : (l == 1 ? sgn1 : sgn2);
      I = l == 0 ? s * r : I + s * r;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (second && l == k) II[k] = r;
  }
  I = -g_abs(I);
  psi = -I;
  S Nl[3][3], omega[3];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    cross3(v[(l + 1) % 3], v[l], Nl[l]);
    const S nn = norm3(Nl[l]);
    if (val(nn) > kNEps)
#pragma unroll
      for (int a = 0; a < 3; ++a) Nl[l][a] = Nl[l][a] / nn;
#pragma unroll
    for (int a = 0; a < 3; ++a) omega[a] = l == 0 ? Nl[l][a] * II[l] : omega[a] + Nl[l][a] * II[l];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) omega[a] = n[a] * I + omega[a];
  const double ov[3] = {val(omega[0]), val(omega[1]), val(omega[2])};
  const bool flat = norm3(ov) < kOmegaEps;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int l1 = (l + 1) % 3;
    phi[l] = flat ? zero_like<S>() : dot3(Nl[l1], omega) / (dot3(Nl[l1], v[l]) + kPhiGuard);
  }
}

// ------------------------------------------------------------------------------------------ kernels
// code bits of a query row
constexpr int kBadIndex = 8;

template <typename T>
__device__ __forceinline__ void load_face(const long long* fb, const T* vtx, const T* nb, int f, const double q[3],
                                          int ix[3], double v[3][3], double n[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) ix[k] = (int)fb[(long long)f * 3 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) v[k][a] = (double)vtx[(long long)ix[k] * 3 + a] - q[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) n[a] = (double)nb[(long long)f * 3 + a];
}

template <typename T, bool LDS>
__global__ __launch_bounds__(kWave) void gc_forward_kernel(const T* __restrict__ query, const T* __restrict__ vertices,
                                                           const long long* __restrict__ faces, long long fsb,
                                                           const T* __restrict__ normals, T* __restrict__ gcv,
                                                           T* __restrict__ gcf, T* __restrict__ sums,
                                                           int* __restrict__ codes, int P, int N, int F) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auto [lane, b, p0, p, rows, live, row] = tile_of(P);
  T* tile = (T*)smem;                                         // face coordinates of 64 faces, tile[fi * 65 + lane]
  T* acc = LDS ? tile + kWave * kStride + lane : gcv + row * N;
  const long long as = LDS ? kStride : 1;
  const bool own = LDS || live;                                // the general path's lanes past P own no row
  const T* vtx = vertices + (long long)b * N * 3;
  const T* nb = normals + (long long)b * F * 3;
  const long long* fb = faces + (long long)b * fsb;
  if (!faces_ok<3>(fb, F, N)) {                                // the whole batch element: NaN rows
    if (live) {
      for (int j = 0; j < N; ++j) gcv[row * N + j] = m_nan(T(0));
      for (int f = 0; f < F; ++f) gcf[row * F + f] = m_nan(T(0));
      sums[row] = m_nan(T(0));
      codes[row] = kBadIndex;
    }
    return;
  }
  const double q[3] = {(double)query[row * 3], (double)query[row * 3 + 1], (double)query[row * 3 + 2]};
  if (own)
    for (int j = 0; j < N; ++j) acc[j * as] = T(0);
  for (int f0 = 0; f0 < F; f0 += kWave) {
    const int nf = min(kWave, F - f0);
    for (int fi = 0; fi < nf; ++fi) {
      int ix[3];
      double v[3][3], n[3], psi, phi[3];
      load_face(fb, vtx, nb, f0 + fi, q, ix, v, n);
      gc_pair(v, n, psi, phi);
      tile[fi * kStride + lane] = (T)psi;
      if (own)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[ix[k] * as] += (T)phi[k];
    }
    __syncthreads();
    tile_out(tile, rows, nf, lane, gcf + f0, (long long)b * P + p0, F);
    __syncthreads();
  }
  T sum = T(0);
  if (own) {
    for (int j = 0; j < N; ++j) sum += acc[j * as];
    const T div = (T)((double)sum + kPhiGuard);
    for (int j = 0; j < N; ++j) acc[j * as] = acc[j * as] / div;
  }
  if (live) {
    sums[row] = sum;
    codes[row] = 0;
  }
  if (LDS) {
    __syncthreads();
    columns_to_rows(tile + kWave * kStride, rows, N, lane, gcv, (long long)b * P + p0, N);
  }
}

// dL/d(query, normal) of one pair: W the cotangents of phi (3) and psi; gq, gn accumulate
__device__ __forceinline__ void pair_grad(const double v[3][3], const double n[3], const double W[4], double gq[3],
                                          double gn[3]) {
  constexpr int K = kDualK;
  constexpr int kPasses = 6 / K;
#pragma unroll 1
  for (int pass = 0; pass < kPasses; ++pass) {
    Dual<K> vd[3][3], nd[3];
    // input i in 0..5 (query x, y, z, normal x, y, z) is component i - pass * K of this pass (seeded and read back
    // with selects: a dynamic index would put the arrays in scratch memory)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      nd[a].v = n[a];
#pragma unroll
      for (int i = 0; i < K; ++i) nd[a].d[i] = i + pass * K == 3 + a ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        vd[k][a].v = v[k][a];
#pragma unroll
        for (int i = 0; i < K; ++i) vd[k][a].d[i] = i + pass * K == a ? -1.0 : 0.0;   // v = vertex - query
      }
    }
    Dual<K> psi, phi[3];
    gc_pair(vd, nd, psi, phi);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double g = W[3] * psi.d[i] + W[0] * phi[0].d[i] + W[1] * phi[1].d[i] + W[2] * phi[2].d[i];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        gq[a] += i + pass * K == a ? g : 0.0;
        gn[a] += i + pass * K == 3 + a ? g : 0.0;
      }
    }
  }
}

template <typename T, bool LDS>
__global__ __launch_bounds__(kWave) void gc_backward_kernel(
    const T* __restrict__ query, const T* __restrict__ vertices, const long long* __restrict__ faces, long long fsb,
    const T* __restrict__ normals, const T* __restrict__ gcv, const T* __restrict__ sums, const int* __restrict__ codes,
    const T* __restrict__ ggcv, const T* __restrict__ ggcf, T* __restrict__ gq, T* __restrict__ part, int P, int N,
    int F) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auto [lane, b, p0, p, rows, live, row] = tile_of(P);
  const int tiles = gridDim.x;
  T* tile = (T*)smem;                                          // dL/dGC_face of 64 faces, tile[fi * 65 + lane]
  T* gcol = tile + kWave * kStride;                            // LDS: dL/dGC_vertex rows, column per lane
  T* out = part + ((long long)b * tiles + blockIdx.x) * F * 3;
  const T* vtx = vertices + (long long)b * N * 3;
  const T* nb = normals + (long long)b * F * 3;
  const long long* fb = faces + (long long)b * fsb;
  if (codes[(long long)b * P] & kBadIndex) {                   // the whole batch element (reduce_kernel: NaN)
    if (live)
#pragma unroll
      for (int a = 0; a < 3; ++a) gq[row * 3 + a] = m_nan(T(0));
    return;
  }
  if (LDS) {
    rows_to_columns(ggcv, (long long)b * P + p0, N, rows, N, lane, gcol);
    __syncthreads();
  }
  const T* grow = LDS ? gcol + lane : ggcv + row * N;
  const long long gs = LDS ? kStride : 1;
  // d(raw / (S + 1e-10))/d(raw): (G_k - sum_j G_j GC_vertex_j) / (S + 1e-10)
  double dot = 0.0;
  for (int j = 0; j < N; ++j) dot += (double)grow[j * gs] * (double)gcv[row * N + j];
  const double div = (double)(T)((double)sums[row] + kPhiGuard);
  const double q[3] = {(double)query[row * 3], (double)query[row * 3 + 1], (double)query[row * 3 + 2]};
  double gqa[3] = {0.0, 0.0, 0.0};
  for (int f0 = 0; f0 < F; f0 += kWave) {
    const int nf = min(kWave, F - f0);
    if (ggcf) {
      __syncthreads();
      tile_in(tile, rows, nf, lane, ggcf + f0, (long long)b * P + p0, F);
      __syncthreads();
    }
    for (int fi = 0; fi < nf; ++fi) {
      const int f = f0 + fi;
      int ix[3];
      double v[3][3], n[3], gn[3] = {0.0, 0.0, 0.0};
      load_face(fb, vtx, nb, f, q, ix, v, n);
      if (live) {
        double W[4];
#pragma unroll
        for (int k = 0; k < 3; ++k) W[k] = ((double)grow[ix[k] * gs] - dot) / div;
        W[3] = ggcf ? (double)tile[fi * kStride + lane] : 0.0;
        pair_grad(v, n, W, gqa, gn);
      }
      wave_sum(gn);
      if (lane == 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) out[(long long)f * 3 + a] = (T)gn[a];
    }
  }
  if (live)
#pragma unroll
    for (int a = 0; a < 3; ++a) gq[row * 3 + a] = (T)gqa[a];
}

template <typename T>
size_t lds_bytes(int N) {
  return (size_t)(N + kWave) * kStride * sizeof(T);
}

template <typename T>
int forward(const T* query, const T* vertices, const long long* faces, long long fsb, const T* normals, T* gcv, T* gcf,
            T* sums, int* codes, int B, int P, int N, int F, void* stream) {
  if (bad_sizes(B, P, N, F) || fsb < 0) return PP_EINVAL;
  if ((long long)B * P == 0) return PP_OK;
  if (!grid_ok(B)) return PP_EINVAL;
  if (!query || !sums || !codes || (N > 0 && (!vertices || !gcv)) || (F > 0 && (!faces || !normals || !gcf)))
    return PP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles_of(P), (unsigned)B);
  static pp::DeviceFlags flags;
  const size_t lds = lds_bytes<T>(N), tile = lds_bytes<T>(0);
  if (lds_fits(gc_forward_kernel<T, true>, lds, flags))
    gc_forward_kernel<T, true><<<grid, dim3(kWave), lds, st>>>(query, vertices, faces, fsb, normals, gcv, gcf, sums,
                                                                codes, P, N, F);
  else
    gc_forward_kernel<T, false><<<grid, dim3(kWave), tile, st>>>(query, vertices, faces, fsb, normals, gcv, gcf, sums,
                                                                  codes, P, N, F);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

template <typename T>
int backward(const T* query, const T* vertices, const long long* faces, long long fsb, const T* normals, const T* gcv,
             const T* sums, const int* codes, const T* ggcv, const T* ggcf, T* gq, T* gn, int B, int P, int N, int F,
             void* ws, size_t ws_bytes, void* stream) {
  if (bad_sizes(B, P, N, F) || fsb < 0) return PP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if ((long long)B * F > 0 && !gn) return PP_EINVAL;
  if ((long long)B * P == 0) {                      // no query: the normals' gradient is zero
    if ((long long)B * F > 0) return (int)pp::fill_bytes(gn, 0, (size_t)B * F * 3 * sizeof(T), st);
    return PP_OK;
  }
  if (!query || !sums || !codes || !gq || (N > 0 && (!vertices || !gcv || !ggcv))) return PP_EINVAL;
  if (F == 0) return (int)pp::fill_bytes(gq, 0, (size_t)B * P * 3 * sizeof(T), st);
  if (!grid_ok(B)) return PP_EINVAL;
  const size_t need = workspace_bytes(B, P, F, 3, (int)sizeof(T));
  if (!faces || !normals || !ws || ws_bytes < need) return PP_EINVAL;
  T* part = (T*)ws;
  const int tiles = tiles_of(P);
  const dim3 grid((unsigned)tiles, (unsigned)B);
  static pp::DeviceFlags flags;
  const size_t lds = lds_bytes<T>(N), tile = lds_bytes<T>(0);
  if (lds_fits(gc_backward_kernel<T, true>, lds, flags))
    gc_backward_kernel<T, true><<<grid, dim3(kWave), lds, st>>>(query, vertices, faces, fsb, normals, gcv, sums, codes,
                                                                 ggcv, ggcf, gq, part, P, N, F);
  else
    gc_backward_kernel<T, false><<<grid, dim3(kWave), tile, st>>>(query, vertices, faces, fsb, normals, gcv, sums,
                                                                   codes, ggcv, ggcf, gq, part, P, N, F);
  PP_RETURN_IF_LAUNCH_FAILED();
  const long long n = (long long)B * F * 3;
  // dL/dnormals[b]: the workgroups' slices in workgroup order; NaN where the face list holds an out-of-range index
  reduce_kernel<T><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(part, codes, gn, B, P, (long long)F * 3,
                                                                            tiles, kBadIndex);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

}  // namespace

extern "C" size_t pp_gc3d_workspace_bytes(int B, int P, int F, int elem_bytes) {
  if (elem_bytes != 4 && elem_bytes != 8) return 0;
  return workspace_bytes(B, P, F, 3, elem_bytes);
}

extern "C" int pp_gc3d_forward_f32(const float* query, const float* vertices, const long long* faces,
                                   long long faces_batch_stride, const float* normals, float* gc_vertex,
                                   float* gc_face, float* sums, int* codes, int B, int P, int N, int F, void* stream) {
  return forward<float>(query, vertices, faces, faces_batch_stride, normals, gc_vertex, gc_face, sums, codes, B, P, N,
                        F, stream);
}

extern "C" int pp_gc3d_forward_f64(const double* query, const double* vertices, const long long* faces,
                                   long long faces_batch_stride, const double* normals, double* gc_vertex,
                                   double* gc_face, double* sums, int* codes, int B, int P, int N, int F,
                                   void* stream) {
  return forward<double>(query, vertices, faces, faces_batch_stride, normals, gc_vertex, gc_face, sums, codes, B, P, N,
                         F, stream);
}

extern "C" int pp_gc3d_backward_f32(const float* query, const float* vertices, const long long* faces,
                                    long long faces_batch_stride, const float* normals, const float* gc_vertex,
                                    const float* sums, const int* codes, const float* grad_gc_vertex,
                                    const float* grad_gc_face, float* grad_query, float* grad_normals, int B, int P,
                                    int N, int F, void* workspace, size_t workspace_bytes, void* stream) {
  return backward<float>(query, vertices, faces, faces_batch_stride, normals, gc_vertex, sums, codes, grad_gc_vertex,
                         grad_gc_face, grad_query, grad_normals, B, P, N, F, workspace, workspace_bytes, stream);
}

extern "C" int pp_gc3d_backward_f64(const double* query, const double* vertices, const long long* faces,
                                    long long faces_batch_stride, const double* normals, const double* gc_vertex,
                                    const double* sums, const int* codes, const double* grad_gc_vertex,
                                    const double* grad_gc_face, double* grad_query, double* grad_normals, int B,
                                    int P, int N, int F, void* workspace, size_t workspace_bytes, void* stream) {
  return backward<double>(query, vertices, faces, faces_batch_stride, normals, gc_vertex, sums, codes, grad_gc_vertex,
                          grad_gc_face, grad_query, grad_normals, B, P, N, F, workspace, workspace_bytes, stream);
}
