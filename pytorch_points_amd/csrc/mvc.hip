// mvc.hip -- mean value coordinates of query points with respect to a closed triangle cage (Ju, Schaefer and Warren,
// "Mean value coordinates for closed triangular meshes", 2005), forward and backward, fp32 and fp64.
// Contract: DESIGN.md "Mean value coordinates" (reference network/geo_operations.py:349-456).
//
// Layout: one workgroup = one wave = 64 queries of one batch element; the whole wave walks the faces in order, so
// a face's indices and corners are wave-uniform loads.  Each lane owns the accumulator row of its query:
//   fast path   a column of LDS, acc[v * 65 + lane] (v is wave-uniform: no bank conflicts; the stride 65 keeps the
//               transposed, coalesced write-out free of conflicts too);
//   general     the query's own output row in global memory (any N).
// Both paths perform the same operations in the same order: a query's row is the same bits on either, and does not
// depend on P, its position or the batch size.
//
// Backward: every (query, face) pair is evaluated again and differentiated by hand (reverse mode through the scalar
// chain below).  dL/dquery is summed in registers; the per-face vertex contributions are summed over the wave (fixed
// DPP / butterfly order), then added by one lane, face after face, into the workgroup's partial (LDS on the fast path,
// its slice of the workspace otherwise); a second kernel adds the partials of a batch element in workgroup order.
// No floating-point atomics anywhere: every output is reproducible bit for bit.
#include <math.h>

#include "cage_common.h"

using namespace pp::cage;

namespace {

__device__ __forceinline__ float m_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double m_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ double m_asin(double x) { return asin(x); }
__device__ __forceinline__ void m_sincos(double x, double* s, double* c) { sincos(x, s, c); }
__device__ __forceinline__ double m_sin(double x) { return sin(x); }

template <typename T>
__device__ __forceinline__ T norm3(T x, T y, T z) {
  return m_sqrt(x * x + y * y + z * z);
}

// the pair is evaluated in fp64 for either data type: fp32 data then loses only its input and output rounding (in fp32
// the chain's cancellations -- c near +-1 for faces seen at small angles, large cancelling weights outside the cage --
// cost up to 0.5 absolute against the fp64 result)
struct Corners {
  double v[3][3];
};
template <typename T>
__device__ __forceinline__ Corners widen(const T v[3][3]) {
  Corners c;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) c.v[k][a] = (double)v[k][a];
  return c;
}

// Everything one (query, face) pair needs, forward and backward.  Corner k's neighbours are k1 = k+1 and k2 = k-1
// (mod 3).  Names follow DESIGN.md: u = v - q, d = |u|, e = u / max(d, 1e-12), l (clamped) and L (raw) the chord
// lengths, th the angles, h their half sum, c and s the cosines and signed sines of the dihedral angles.
template <typename T>
struct Pair {
  T u[3][3], d[3], e[3][3], df[3][3], L[3], l[3], th[3], sth[3], h, sh, shk[3], R[3], c[3], r[3], sgn, s[3], num[3],
      den[3], w[3], wf[3];
  bool zero, inside;

  __device__ __forceinline__ void eval(const T q[3], const Corners& cv) {
    const auto& v = cv.v;
    const T L_CLAMP = T(2.0 - 2e-5), C_CLAMP = T(1.0 - 1e-5);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int a = 0; a < 3; ++a) u[k][a] = v[k][a] - q[a];
      d[k] = norm3(u[k][0], u[k][1], u[k][2]);
      const T dn = d[k] > T(1e-12) ? d[k] : T(1e-12);
#pragma unroll
      for (int a = 0; a < 3; ++a) e[k][a] = u[k][a] / dn;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
#pragma unroll
      for (int a = 0; a < 3; ++a) df[k][a] = e[k1][a] - e[k2][a];
      L[k] = norm3(df[k][0], df[k][1], df[k][2]);
      l[k] = L[k] >= T(2) ? L[k] - (L[k] - L_CLAMP) : L[k];          // straight-through clamp
      th[k] = T(2) * m_asin(l[k] / T(2));
      sth[k] = m_sin(th[k]);
    }
    h = (th[0] + th[1] + th[2]) / T(2);
    sh = m_sin(h);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      shk[k] = m_sin(h - th[k]);
      R[k] = T(2) * sh * shk[k] / (sth[k1] * sth[k2]);               // c + 1 before the clamp
      T ck = R[k] - T(1);
      ck = ck >= T(1) ? ck - (ck - C_CLAMP) : ck;
      ck = ck <= T(-1) ? ck - (ck + C_CLAMP) : ck;
      c[k] = ck;
    }
    const T det = e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                  e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
    sgn = det > T(0) ? T(1) : (det < T(0) ? T(-1) : (det == T(0) ? T(0) : det));
    zero = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[k] = m_sqrt(T(1) - c[k] * c[k]);
      s[k] = sgn * r[k];
      zero = zero || fabs(s[k]) <= T(1e-5);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      num[k] = th[k] - c[k1] * th[k2] - c[k2] * th[k1];
      den[k] = d[k] * sth[k1] * s[k2];
      w[k] = num[k] / den[k];
      wf[k] = sth[k] * d[k2] * d[k1];
    }
    inside = T(3.1415927) - h < T(1e-4);
  }

  // Reverse mode: W = dL/dw (normal branch, ONFACE false) or dL/dwf (on-face branch) -> gu = dL/du (3 corners).
  template <bool ONFACE>
  __device__ __forceinline__ void grad(const T W[3], T gu[3][3]) const {
    T gth[3] = {0, 0, 0}, gsth[3] = {0, 0, 0}, gd[3] = {0, 0, 0};
    if (ONFACE) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        gsth[k] += W[k] * d[k2] * d[k1];
        gd[k2] += W[k] * sth[k] * d[k1];
        gd[k1] += W[k] * sth[k] * d[k2];
      }
    } else {
      T gc[3] = {0, 0, 0}, gs[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        const T gn = W[k] / den[k];
        const T gden = -W[k] * w[k] / den[k];
        gth[k] += gn;
        gc[k1] -= gn * th[k2];
        gth[k2] -= gn * c[k1];
        gc[k2] -= gn * th[k1];
        gth[k1] -= gn * c[k2];
        gd[k] += gden * sth[k1] * s[k2];
        gsth[k1] += gden * d[k] * s[k2];
        gs[k2] += gden * d[k] * sth[k1];
      }
      T gh = 0, gsh = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        const T gck = gc[k] - gs[k] * sgn * c[k] / r[k];              // s = sgn sqrt(1 - c^2); clamp: gradient 1
        const T Q = sth[k1] * sth[k2];
        gsh += gck * T(2) * shk[k] / Q;
        const T gshk = gck * T(2) * sh / Q;
        const T gQ = -gck * R[k] / Q;
        gsth[k1] += gQ * sth[k2];
        gsth[k2] += gQ * sth[k1];
        T sn, cs;
        m_sincos(h - th[k], &sn, &cs);
        gh += gshk * cs;
        gth[k] -= gshk * cs;
      }
      T sn, ch;
      m_sincos(h, &sn, &ch);
      gh += gsh * ch;
#pragma unroll
      for (int k = 0; k < 3; ++k) gth[k] += gh / T(2);
    }
    T ge[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      T sn, cth;
      m_sincos(th[k], &sn, &cth);
      const T g = gth[k] + gsth[k] * cth;
      const T half = l[k] / T(2);
      const T gl = g / m_sqrt(T(1) - half * half);                    // theta = 2 asin(l / 2); clamp: gradient 1
      const T f = L[k] > T(0) ? gl / L[k] : T(0);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        ge[k1][a] += f * df[k][a];
        ge[k2][a] -= f * df[k][a];
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (d[k] > T(1e-12)) {
        const T dot = e[k][0] * ge[k][0] + e[k][1] * ge[k][1] + e[k][2] * ge[k][2];
#pragma unroll
        for (int a = 0; a < 3; ++a) gu[k][a] = (ge[k][a] - e[k][a] * dot) / d[k] + gd[k] * e[k][a];
      } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) gu[k][a] = ge[k][a] / T(1e-12);
      }
    }
  }
};

template <typename T>
__device__ __forceinline__ bool load_face(const long long* faces, const T* vtx, int N, T v[3][3], int ix[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long i = faces[k];
    ok = ok && i >= 0 && i < N;
    ix[k] = ok ? (int)i : 0;
  }
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) v[k][a] = vtx[(long long)ix[k] * 3 + a];
  return true;
}

// code bits of a query row (kept for the backward)
constexpr int kSumReplaced = 1, kOnFace = 2, kOnVertex = 4, kBadIndex = 8;

template <typename T, bool LDS>
__global__ __launch_bounds__(kWave) void mvc_forward_kernel(const T* __restrict__ query, const T* __restrict__ vertices,
                                                            const long long* __restrict__ faces, long long fsb,
                                                            T* __restrict__ out, T* __restrict__ sums,
                                                            int* __restrict__ codes, T* __restrict__ wi, int P, int N,
                                                            int F) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auto [lane, b, p0, p, rows, live, row] = tile_of(P);
  if (!LDS && !live) return;                        // the general path has no cross-lane step
  T* acc = LDS ? (T*)smem + lane : out + row * N;
  const long long as = LDS ? kStride : 1;
  const T* vtx = vertices + (long long)b * N * 3;
  const long long* fb = faces + (long long)b * fsb;
  const T q[3] = {query[row * 3], query[row * 3 + 1], query[row * 3 + 2]};
  const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
  for (int j = 0; j < N; ++j) acc[j * as] = T(0);
  bool onface = false, bad = false;
  int first_on = 0;
  for (int f = 0; f < F; ++f) {
    T v[3][3];
    int ix[3];
    if (!load_face(fb + (long long)f * 3, vtx, N, v, ix)) {
      bad = true;
      continue;
    }
    Pair<double> pr;
    pr.eval(qd, widen(v));
    T w[3] = {T(0), T(0), T(0)};
    bool add = false;
    if (pr.inside) {
      if (!onface) {                                // the query lies on a face: only on-face faces count
        for (int j = 0; j < N; ++j) acc[j * as] = T(0);
        onface = true;
        first_on = f;
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = (T)pr.wf[k];
      add = true;
    } else if (!onface && !pr.zero) {
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = (T)pr.w[k];
      add = true;
    }
    if (add)
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[ix[k] * as] += w[k];
    if (wi && live)
#pragma unroll
      for (int k = 0; k < 3; ++k) wi[(row * F + f) * 3 + k] = w[k];
  }
  if (wi && live) {                                 // faces met before the first on-face one; a bad row: all
    const int upto = bad ? F : first_on;
    for (int f = 0; f < upto; ++f)
#pragma unroll
      for (int k = 0; k < 3; ++k) wi[(row * F + f) * 3 + k] = bad ? m_nan(T(0)) : T(0);
  }
  bool onvertex = false;
  for (int j = 0; j < N; ++j)
    onvertex = onvertex || norm3(vtx[j * 3] - q[0], vtx[j * 3 + 1] - q[1], vtx[j * 3 + 2] - q[2]) < T(1e-8);
  if (onvertex)
    for (int j = 0; j < N; ++j)
      acc[j * as] = norm3(vtx[j * 3] - q[0], vtx[j * 3 + 1] - q[1], vtx[j * 3 + 2] - q[2]) < T(1e-8) ? T(1) : T(0);
  T sum = T(0);
  for (int j = 0; j < N; ++j) sum += acc[j * as];
  int code = 0;
  if (sum == T(0)) {
    sum = T(1);
    code |= kSumReplaced;
  }
  if (onface) code |= kOnFace;
  if (onvertex) code |= kOnVertex;
  if (bad) {
    code |= kBadIndex;
    sum = m_nan(T(0));
  }
  for (int j = 0; j < N; ++j) acc[j * as] = acc[j * as] / sum;
  if (live) {
    sums[row] = sum;
    codes[row] = code;
  }
  if (LDS) {
    __syncthreads();
    columns_to_rows((const T*)smem, rows, N, lane, out, (long long)b * P + p0, N);
  }
}

// the fp32 form of the wave sum of nine values (cage_common.h has the fp64 one): DPP, every lane returns the same bits
using pp::cage::wave_sum;
__device__ __forceinline__ void wave_sum(float (&x)[9]) {
  float a[6] = {x[0], x[1], x[2], x[3], x[4], x[5]};
  float c[6] = {x[6], x[7], x[8], 0.f, 0.f, 0.f};
  pp::wave_reduce6_dpp<true, 6>(a);
  pp::wave_reduce6_dpp<true, 6>(c);
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a[i]), 63));
#pragma unroll
  for (int i = 0; i < 3; ++i) x[6 + i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c[i]), 63));
}

template <typename T, bool LDS>
__global__ __launch_bounds__(kWave) void mvc_backward_kernel(
    const T* __restrict__ query, const T* __restrict__ vertices, const long long* __restrict__ faces, long long fsb,
    const T* __restrict__ wj, const T* __restrict__ sums, const int* __restrict__ codes, const T* __restrict__ gwj,
    const T* __restrict__ gwi, T* __restrict__ gq, T* __restrict__ part, int P, int N, int F) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auto [lane, b, p0, p, rows, live, row] = tile_of(P);
  const int tiles = gridDim.x;
  T* gcol = (T*)smem;                                         // LDS: dL/dwj rows, column per lane
  T* dv = LDS ? gcol + (long long)N * kStride : part + ((long long)b * tiles + blockIdx.x) * N * 3;
  const T* vtx = vertices + (long long)b * N * 3;
  const long long* fb = faces + (long long)b * fsb;
  const int code = codes[row];
  const T sum = sums[row];
  const bool dead = !live || (code & (kOnVertex | kBadIndex));  // rows overridden to constants: no gradient
  if (LDS) {
    for (int i = lane; i < N * 3; i += kWave) dv[i] = T(0);
    rows_to_columns(gwj, (long long)b * P + p0, N, rows, N, lane, gcol);
    __syncthreads();
  }
  const T* grow = LDS ? gcol + lane : gwj + row * N;
  const long long gs = LDS ? kStride : 1;
  // d(wj / S)/d(wj): (G_k - sum_j G_j wjn_j) / S; with S replaced by 1 (a zero row sum) it is G_k
  T dot = T(0);
  if (!(code & kSumReplaced))
    for (int j = 0; j < N; ++j) dot += grow[j * gs] * wj[row * N + j];
  const T q[3] = {query[row * 3], query[row * 3 + 1], query[row * 3 + 2]};
  const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
  double gqa[3] = {0.0, 0.0, 0.0};
  for (int f = 0; f < F; ++f) {
    T v[3][3];
    int ix[3];
    if (!load_face(fb + (long long)f * 3, vtx, N, v, ix)) continue;
    T gu[9] = {T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0)};
    if (!dead) {
      Pair<double> pr;
      pr.eval(qd, widen(v));
      const bool onface = code & kOnFace;
      if (onface ? pr.inside : !pr.zero) {
        double W[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const T g = grow[ix[k] * gs];
          W[k] = (double)((code & kSumReplaced) ? g : (g - dot) / sum);
          if (gwi) W[k] += (double)gwi[(row * F + f) * 3 + k];
        }
        double g3[3][3];
        if (onface)
          pr.template grad<true>(W, g3);
        else
          pr.template grad<false>(W, g3);
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            gu[k * 3 + a] = (T)g3[k][a];
            gqa[a] -= g3[k][a];
          }
      }
    }
    wave_sum(gu);
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) dv[ix[k] * 3 + a] += gu[k * 3 + a];
  }
  if (live)
#pragma unroll
    for (int a = 0; a < 3; ++a) gq[row * 3 + a] = (code & kBadIndex) ? m_nan(T(0)) : (T)gqa[a];
  if (LDS) {
    __syncthreads();
    T* o = part + ((long long)b * tiles + blockIdx.x) * N * 3;
    for (int i = lane; i < N * 3; i += kWave) o[i] = dv[i];
  }
}

template <typename T>
size_t fwd_lds(int N) {
  return (size_t)N * kStride * sizeof(T);
}
template <typename T>
size_t bwd_lds(int N) {
  return (size_t)N * (kStride + 3) * sizeof(T);
}

template <typename T>
int forward(const T* query, const T* vertices, const long long* faces, long long fsb, T* wj, T* sums, int* codes,
            T* wi, int B, int P, int N, int F, void* stream) {
  if (bad_sizes(B, P, N, F) || fsb < 0) return PP_EINVAL;
  if ((long long)B * P == 0) return PP_OK;
  if (!grid_ok(B)) return PP_EINVAL;
  if (!query || !wj || !sums || !codes || (N > 0 && !vertices) || (F > 0 && !faces)) return PP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles_of(P), (unsigned)B);
  static pp::DeviceFlags flags;
  const size_t lds = fwd_lds<T>(N);
  if (N > 0 && lds_fits(mvc_forward_kernel<T, true>, lds, flags))
    mvc_forward_kernel<T, true><<<grid, dim3(kWave), lds, st>>>(query, vertices, faces, fsb, wj, sums, codes, wi, P, N, F);
  else
    mvc_forward_kernel<T, false><<<grid, dim3(kWave), 0, st>>>(query, vertices, faces, fsb, wj, sums, codes, wi, P, N, F);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

template <typename T>
int backward(const T* query, const T* vertices, const long long* faces, long long fsb, const T* wj, const T* sums,
             const int* codes, const T* gwj, const T* gwi, T* gq, T* gv, int B, int P, int N, int F, void* ws,
             size_t ws_bytes, void* stream) {
  if (bad_sizes(B, P, N, F) || fsb < 0) return PP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if ((long long)B * N > 0 && !gv) return PP_EINVAL;
  if ((long long)B * P == 0) {                      // no query: the vertex gradient is zero
    if ((long long)B * N > 0) return (int)pp::fill_bytes(gv, 0, (size_t)B * N * 3 * sizeof(T), st);
    return PP_OK;
  }
  if (!query || !wj || !sums || !codes || !gwj || !gq || (F > 0 && !faces)) return PP_EINVAL;
  if (N == 0) return (int)pp::fill_bytes(gq, 0, (size_t)B * P * 3 * sizeof(T), st);
  if (!grid_ok(B)) return PP_EINVAL;
  const size_t need = workspace_bytes(B, P, N, 3, (int)sizeof(T));
  if (!ws || ws_bytes < need || !vertices) return PP_EINVAL;
  T* part = (T*)ws;
  const int tiles = tiles_of(P);
  const dim3 grid((unsigned)tiles, (unsigned)B);
  static pp::DeviceFlags flags;
  const size_t lds = bwd_lds<T>(N);
  if (lds_fits(mvc_backward_kernel<T, true>, lds, flags)) {
    mvc_backward_kernel<T, true><<<grid, dim3(kWave), lds, st>>>(query, vertices, faces, fsb, wj, sums, codes, gwj, gwi,
                                                                  gq, part, P, N, F);
  } else {
    const hipError_t e = pp::fill_bytes(part, 0, need, st);
    if (e != hipSuccess) return (int)e;
    mvc_backward_kernel<T, false><<<grid, dim3(kWave), 0, st>>>(query, vertices, faces, fsb, wj, sums, codes, gwj, gwi,
                                                                 gq, part, P, N, F);
  }
  PP_RETURN_IF_LAUNCH_FAILED();
  const long long n = (long long)B * N * 3;
  // dL/dvertices[b]: the workgroups' partials in workgroup order; NaN where the face list holds an out-of-range index
  reduce_kernel<T><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(part, codes, gv, B, P, (long long)N * 3,
                                                                            tiles, kBadIndex);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

}  // namespace

extern "C" size_t pp_mvc3d_workspace_bytes(int B, int P, int N, int elem_bytes) {
  if (elem_bytes != 4 && elem_bytes != 8) return 0;
  return workspace_bytes(B, P, N, 3, elem_bytes);
}

extern "C" int pp_mvc3d_forward_f32(const float* query, const float* vertices, const long long* faces,
                                    long long faces_batch_stride, float* wj, float* sums, int* codes, float* wi, int B,
                                    int P, int N, int F, void* stream) {
  return forward<float>(query, vertices, faces, faces_batch_stride, wj, sums, codes, wi, B, P, N, F, stream);
}

extern "C" int pp_mvc3d_forward_f64(const double* query, const double* vertices, const long long* faces,
                                    long long faces_batch_stride, double* wj, double* sums, int* codes, double* wi,
                                    int B, int P, int N, int F, void* stream) {
  return forward<double>(query, vertices, faces, faces_batch_stride, wj, sums, codes, wi, B, P, N, F, stream);
}

extern "C" int pp_mvc3d_backward_f32(const float* query, const float* vertices, const long long* faces,
                                     long long faces_batch_stride, const float* wj, const float* sums, const int* codes,
                                     const float* grad_wj, const float* grad_wi, float* grad_query,
                                     float* grad_vertices, int B, int P, int N, int F, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return backward<float>(query, vertices, faces, faces_batch_stride, wj, sums, codes, grad_wj, grad_wi, grad_query,
                         grad_vertices, B, P, N, F, workspace, workspace_bytes, stream);
}

extern "C" int pp_mvc3d_backward_f64(const double* query, const double* vertices, const long long* faces,
                                     long long faces_batch_stride, const double* wj, const double* sums,
                                     const int* codes, const double* grad_wj, const double* grad_wi,
                                     double* grad_query, double* grad_vertices, int B, int P, int N, int F,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return backward<double>(query, vertices, faces, faces_batch_stride, wj, sums, codes, grad_wj, grad_wi, grad_query,
                          grad_vertices, B, P, N, F, workspace, workspace_bytes, stream);
}
