// linalg.hip -- batched SVD of small fp32 matrices (m, n <= 32): pp_batch_svd_f32 (include/pp_hip.h).
//
// Method: one-sided (Hestenes) Jacobi on W = A (m >= n) or W = A^T (m < n), so W is R x K with R = max(m, n) >= K =
// min(m, n).  A sweep visits every column pair (p, q) once; a pair is rotated unless
// |w_p . w_q| <= tol * ||w_p|| * ||w_q||.  The iteration ends after the first sweep that rotates nothing (info = the
// number of sweeps, that one included) or after max_sweeps sweeps (info = -1).  The rotations are accumulated into the
// K x K matrix Z (= V for m >= n, = U for m < n); sigma_j = ||w_j|| and the "W side" Y (= U for m >= n, = V otherwise)
// holds w_j / sigma_j.
//
// Determinism and range:
//   - every matrix is scaled by 2^-e first, e the exponent of its largest |entry| (frexp), and only s is scaled back:
//     the squared column norms cannot overflow or underflow for any finite input, and svd(2^k A) = (U, 2^k s, V) bit for
//     bit while no entry leaves the normal range under the scaling;
//   - a matrix's result depends on that matrix alone (never on the batch size or on its position); no atomics, no
//     workspace; the rotation of a pair is computed from its two columns in a fixed order (lower index first), so the
//     two lanes that own the columns in the column-per-lane layout compute the same (c, s) bit for bit;
//   - a matrix with a NaN or an infinity gets NaN in all of its s, U and V and info = -2, checked before any sweep.
//
// Two layouts:
//   svd_lane_kernel   K <= 4: one matrix per lane, W (RM x K, rows beyond R zero) and Z in registers.  Covers the 20 x 3
//                     neighbourhoods of batch_normals.
//   svd_cols_kernel   K > 4: one column of W and one of Z per lane, a group of G (a power of two >= K) lanes per
//                     matrix.  Sweeps are round-robin tournaments of G - 1 steps; the partner's column arrives by
//                     ds_bpermute (__shfl); a ballot over the group ends the sweep loop.
// Output columns are sorted by descending sigma when `sort` is set (ties: lower original column first).  Columns of Y
// with sigma == 0 and, in the full form, columns K..R-1 of Y are completed deterministically: Gram-Schmidt, applied
// twice, of e_1, e_2, ... in order against the columns already in place; the first candidate whose residual keeps a
// squared norm >= 1 / (2R) is taken (one always does: the squared residuals of all R candidates sum to >= 1).
#include <math.h>

#include <algorithm>

#include "pp_common.h"

namespace {

constexpr int kSvdThreads = 256;

// The rotation that orthogonalises columns x (lower index) and y: a = ||x||^2, b = ||y||^2, g = x.y.
// false: the pair is converged (also when g == 0 or a column is zero).
__device__ __forceinline__ bool jacobi_rotation(float a, float b, float g, float tol, float& c, float& s) {
  if (!(fabsf(g) > tol * (sqrtf(a) * sqrtf(b)))) return false;
  const float z = (b - a) / (2.0f * g);
  const float az = fabsf(z);
  // t = the smaller root of t^2 + 2zt - 1 = 0; for |z| > 2^60 sqrt(1 + z^2) = |z| to working precision, and z^2
  // could overflow
  const float t = az > 0x1p60f ? 0.5f / z : copysignf(1.0f, z) / (az + sqrtf(1.0f + z * z));
  c = 1.0f / sqrtf(1.0f + t * t);
  s = c * t;
  return true;
}

// x' = c x - s y (lower column), y' = s x + c y (higher column): the same two expressions in both layouts
__device__ __forceinline__ float rot_lo(float c, float s, float x, float y) { return c * x - s * y; }
__device__ __forceinline__ float rot_hi(float c, float s, float x, float y) { return s * x + c * y; }

struct SvdShape {
  int m, n, R, K, trans, ucols, vcols, ycols, full;
};

__host__ __device__ inline SvdShape svd_shape(int m, int n, int full) {
  SvdShape h;
  h.m = m;
  h.n = n;
  h.trans = m < n;
  h.R = h.trans ? n : m;
  h.K = h.trans ? m : n;
  h.ucols = full ? m : h.K;
  h.vcols = full ? n : h.K;
  h.ycols = full ? h.R : h.K;
  h.full = full;
  return h;
}

// bits 0..n-1
__device__ __forceinline__ unsigned low_bits(int n) { return n >= 32 ? ~0u : (1u << n) - 1u; }

// W[r][c] of matrix `a`
__device__ __forceinline__ float w_at(const float* a, const SvdShape& h, int r, int c) {
  return a[h.trans ? (long long)c * h.n + r : (long long)r * h.n + c];
}

// every output of a matrix with a non-finite entry: NaN, info -2
__device__ void write_nonfinite(float* u, float* s, float* v, int* info, long long i, const SvdShape& h) {
  const float nan = __builtin_nanf("");
  float* ui = u + i * h.m * h.ucols;
  float* vi = v + i * h.n * h.vcols;
  for (int k = 0; k < h.m * h.ucols; ++k) ui[k] = nan;
  for (int k = 0; k < h.n * h.vcols; ++k) vi[k] = nan;
  for (int k = 0; k < h.K; ++k) s[i * h.K + k] = nan;
  if (info) info[i] = -2;
}

// Fill the columns of Y (R x ycols, row stride ycols) whose bit in `valid` is clear, in ascending order, with the
// deterministic orthonormal completion described at the top.  One thread; the column being built is its own scratch.
__device__ void complete_columns(float* y, int R, int ycols, unsigned valid) {
  for (int j = 0; j < ycols; ++j) {
    if ((valid >> j) & 1u) continue;
    for (int e = 0; e < R; ++e) {
      for (int r = 0; r < R; ++r) y[(long long)r * ycols + j] = r == e ? 1.0f : 0.0f;
      for (int pass = 0; pass < 2; ++pass) {
        for (int c = 0; c < ycols; ++c) {
          if (!((valid >> c) & 1u)) continue;
          float d = 0.0f;
          for (int r = 0; r < R; ++r) d = __builtin_fmaf(y[(long long)r * ycols + c], y[(long long)r * ycols + j], d);
          for (int r = 0; r < R; ++r) {
            float* t = y + (long long)r * ycols + j;
            *t = *t - d * y[(long long)r * ycols + c];
          }
        }
      }
      float nn = 0.0f;
      for (int r = 0; r < R; ++r) nn = __builtin_fmaf(y[(long long)r * ycols + j], y[(long long)r * ycols + j], nn);
      if (nn * (float)(2 * R) >= 1.0f || e == R - 1) {
        const float nrm = sqrtf(nn);
        for (int r = 0; r < R; ++r) y[(long long)r * ycols + j] = y[(long long)r * ycols + j] / nrm;
        break;
      }
    }
    valid |= 1u << j;
  }
}

// Scan a matrix: false if it has a non-finite entry; otherwise the exponent e of its largest |entry| (0 for a zero
// matrix), so that every entry times 2^-e is below 1 in magnitude.
__device__ __forceinline__ bool scan_matrix(const float* a, int count, int& e) {
  float amax = 0.0f;
  bool finite = true;
  for (int k = 0; k < count; ++k) {
    const float x = fabsf(a[k]);
    finite = finite && x <= 3.40282347e38f;   // false for NaN and inf
    amax = fmaxf(amax, x);
  }
  e = 0;
  if (finite && amax > 0.0f) frexpf(amax, &e);
  return finite;
}

// ------------------------------------------------------------------------------------ one matrix per lane (K <= 4)
template <int RM, int KK>
__global__ __launch_bounds__(kSvdThreads) void svd_lane_kernel(const float* __restrict__ a, float* __restrict__ u,
                                                               float* __restrict__ s, float* __restrict__ v,
                                                               int* __restrict__ info, long long batch, int m, int n,
                                                               int full, int sort, float tol, int max_sweeps) {
  const SvdShape h = svd_shape(m, n, full);
  const long long stride = (long long)gridDim.x * kSvdThreads;
  for (long long i = (long long)blockIdx.x * kSvdThreads + threadIdx.x; i < batch; i += stride) {
    const float* ai = a + i * m * n;
    int e;
    if (!scan_matrix(ai, m * n, e)) {
      write_nonfinite(u, s, v, info, i, h);
      continue;
    }
    float w[RM][KK], z[KK][KK];
#pragma unroll
    for (int r = 0; r < RM; ++r)
#pragma unroll
      for (int c = 0; c < KK; ++c) w[r][c] = r < h.R ? ldexpf(w_at(ai, h, r, c), -e) : 0.0f;
#pragma unroll
    for (int r = 0; r < KK; ++r)
#pragma unroll
      for (int c = 0; c < KK; ++c) z[r][c] = r == c ? 1.0f : 0.0f;

    int sweeps = -1;
    for (int sweep = 1; sweep <= max_sweeps; ++sweep) {
      bool rotated = false;
#pragma unroll
      for (int p = 0; p < KK - 1; ++p)
#pragma unroll
        for (int q = p + 1; q < KK; ++q) {
          float aa = 0.0f, bb = 0.0f, gg = 0.0f;
#pragma unroll
          for (int r = 0; r < RM; ++r) {
            aa = __builtin_fmaf(w[r][p], w[r][p], aa);
            bb = __builtin_fmaf(w[r][q], w[r][q], bb);
            gg = __builtin_fmaf(w[r][p], w[r][q], gg);
          }
          float c, sn;
          if (jacobi_rotation(aa, bb, gg, tol, c, sn)) {
            rotated = true;
#pragma unroll
            for (int r = 0; r < RM; ++r) {
              const float x = w[r][p], y = w[r][q];
              w[r][p] = rot_lo(c, sn, x, y);
              w[r][q] = rot_hi(c, sn, x, y);
            }
#pragma unroll
            for (int r = 0; r < KK; ++r) {
              const float x = z[r][p], y = z[r][q];
              z[r][p] = rot_lo(c, sn, x, y);
              z[r][q] = rot_hi(c, sn, x, y);
            }
          }
        }
      if (!rotated) {
        sweeps = sweep;
        break;
      }
    }

    float sig[KK];
    int rank[KK];
#pragma unroll
    for (int c = 0; c < KK; ++c) {
      float nn = 0.0f;
#pragma unroll
      for (int r = 0; r < RM; ++r) nn = __builtin_fmaf(w[r][c], w[r][c], nn);
      sig[c] = sqrtf(nn);
    }
    unsigned valid = 0;
#pragma unroll
    for (int c = 0; c < KK; ++c) {
      int k = c;
      if (sort) {
        k = 0;
#pragma unroll
        for (int o = 0; o < KK; ++o) k += (sig[o] > sig[c]) || (sig[o] == sig[c] && o < c);
      }
      rank[c] = k;
      if (sig[c] > 0.0f) valid |= 1u << k;
    }

    float* ui = u + i * m * h.ucols;
    float* vi = v + i * n * h.vcols;
    float* yi = h.trans ? vi : ui;
    float* zi = h.trans ? ui : vi;
#pragma unroll
    for (int c = 0; c < KK; ++c) {
      const int k = rank[c];
      s[i * KK + k] = ldexpf(sig[c], e);
      const bool inv_ok = sig[c] > 0.0f;
#pragma unroll
      for (int r = 0; r < RM; ++r)
        if (r < h.R) yi[(long long)r * h.ycols + k] = inv_ok ? w[r][c] / sig[c] : 0.0f;
#pragma unroll
      for (int r = 0; r < KK; ++r) zi[r * KK + k] = z[r][c];
    }
    if (valid != low_bits(h.ycols)) complete_columns(yi, h.R, h.ycols, valid);
    if (info) info[i] = sweeps;
  }
}

// ---------------------------------------------------------------------------- one column per lane (4 < K <= 32)
// G lanes per matrix (G a power of two >= K; lanes K..G-1 hold zero columns, which never rotate), W rows padded to RM.
template <int RM, int G>
__global__ __launch_bounds__(kSvdThreads) void svd_cols_kernel(const float* __restrict__ a, float* __restrict__ u,
                                                               float* __restrict__ s, float* __restrict__ v,
                                                               int* __restrict__ info, long long batch, int m, int n,
                                                               int full, int sort, float tol, int max_sweeps) {
  constexpr int kPerBlock = kSvdThreads / G;
  const SvdShape h = svd_shape(m, n, full);
  const int lane = threadIdx.x & 63;
  const int col = lane & (G - 1);
  const int gbase = lane - col;                                   // the group's first lane in the wave
  const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << gbase;
  const bool real_col = col < h.K;
  // block-uniform loop: the __syncthreads below is reached by every thread of the block
  for (long long first = (long long)blockIdx.x * kPerBlock; first < batch; first += (long long)gridDim.x * kPerBlock) {
    const long long i = first + threadIdx.x / G;
    const bool have = i < batch;
    const float* ai = a + (have ? i : 0) * m * n;
    int e = 0;
    bool finite = true;
    if (have) finite = scan_matrix(ai, m * n, e);

    float w[RM], z[G];
#pragma unroll
    for (int r = 0; r < RM; ++r) w[r] = (have && finite && real_col && r < h.R) ? ldexpf(w_at(ai, h, r, col), -e) : 0.0f;
#pragma unroll
    for (int r = 0; r < G; ++r) z[r] = (real_col && r == col) ? 1.0f : 0.0f;

    bool done = !(have && finite);
    int sweeps = -1, sweep = 0;
    while (__ballot(!done) != 0ull) {
      bool rotated = false;
      for (int step = 0; step < G - 1; ++step) {
        // round-robin tournament: player G-1 meets `step`; every other player i meets (2 step - i) mod (G - 1)
        int partner;
        if (col == G - 1)
          partner = step;
        else if (col == step)
          partner = G - 1;
        else
          partner = (2 * step - col + 2 * (G - 1)) % (G - 1);
        const int src = gbase + partner;
        const bool lower = col < partner;
        float wp[RM];
#pragma unroll
        for (int r = 0; r < RM; ++r) wp[r] = __shfl(w[r], src);
        float aa = 0.0f, bb = 0.0f, gg = 0.0f;
#pragma unroll
        for (int r = 0; r < RM; ++r) {
          const float x = lower ? w[r] : wp[r], y = lower ? wp[r] : w[r];
          aa = __builtin_fmaf(x, x, aa);
          bb = __builtin_fmaf(y, y, bb);
          gg = __builtin_fmaf(x, y, gg);
        }
        float c = 1.0f, sn = 0.0f;
        const bool rot = !done && jacobi_rotation(aa, bb, gg, tol, c, sn);
        rotated = rotated || rot;
#pragma unroll
        for (int r = 0; r < RM; ++r) {
          const float x = lower ? w[r] : wp[r], y = lower ? wp[r] : w[r];
          const float nw = lower ? rot_lo(c, sn, x, y) : rot_hi(c, sn, x, y);
          w[r] = rot ? nw : w[r];
        }
#pragma unroll
        for (int r = 0; r < G; ++r) {
          const float zp = __shfl(z[r], src);
          const float x = lower ? z[r] : zp, y = lower ? zp : z[r];
          const float nz = lower ? rot_lo(c, sn, x, y) : rot_hi(c, sn, x, y);
          z[r] = rot ? nz : z[r];
        }
      }
      const bool group_rotated = (__ballot(rotated) & gmask) != 0ull;
      if (!done) {
        ++sweep;
        if (!group_rotated) {
          done = true;
          sweeps = sweep;
        } else if (sweep >= max_sweeps) {
          done = true;
        }
      }
    }

    float nn = 0.0f;
#pragma unroll
    for (int r = 0; r < RM; ++r) nn = __builtin_fmaf(w[r], w[r], nn);
    const float sig = sqrtf(nn);
    int k = col;   // output column: the rank of sigma (descending, ties to the lower column) when sorting
    if (sort) {
      k = 0;
      for (int o = 0; o < G; ++o) {
        const float so = __shfl(sig, gbase + o);
        k += o < h.K && (so > sig || (so == sig && o < col));
      }
    }
    unsigned valid = 0;
    for (int o = 0; o < G; ++o) {
      const int ko = __shfl(k, gbase + o);
      const float so = __shfl(sig, gbase + o);
      if (o < h.K && so > 0.0f) valid |= 1u << ko;
    }

    float* ui = u + (have ? i : 0) * m * h.ucols;
    float* vi = v + (have ? i : 0) * n * h.vcols;
    float* yi = h.trans ? vi : ui;
    float* zi = h.trans ? ui : vi;
    if (have && finite && real_col) {
      s[i * h.K + k] = ldexpf(sig, e);
#pragma unroll
      for (int r = 0; r < RM; ++r)
        if (r < h.R) yi[(long long)r * h.ycols + k] = sig > 0.0f ? w[r] / sig : 0.0f;
#pragma unroll
      for (int r = 0; r < G; ++r)
        if (r < h.K) zi[(long long)r * h.K + k] = z[r];
      if (col == 0 && info) info[i] = sweeps;
    }
    __syncthreads();   // the group's columns are in memory before one lane completes Y
    if (have && col == 0) {
      if (!finite)
        write_nonfinite(u, s, v, info, i, h);
      else if (valid != low_bits(h.ycols))
        complete_columns(yi, h.R, h.ycols, valid);
    }
  }
}

template <int RM, int KK>
void launch_lane(hipStream_t st, int blocks, const float* a, float* u, float* s, float* v, int* info, long long batch,
                 int m, int n, int full, int sort, float tol, int max_sweeps) {
  svd_lane_kernel<RM, KK><<<dim3((unsigned)blocks), dim3(kSvdThreads), 0, st>>>(a, u, s, v, info, batch, m, n, full,
                                                                                 sort, tol, max_sweeps);
}

template <int KK>
void dispatch_lane(int R, hipStream_t st, int blocks, const float* a, float* u, float* s, float* v, int* info,
                   long long batch, int m, int n, int full, int sort, float tol, int max_sweeps) {
#define PP_SVD_LANE(RMV) \
  if (R <= RMV) return launch_lane<RMV, KK>(st, blocks, a, u, s, v, info, batch, m, n, full, sort, tol, max_sweeps)
  PP_SVD_LANE(4);
  PP_SVD_LANE(8);
  PP_SVD_LANE(12);
  PP_SVD_LANE(16);
  PP_SVD_LANE(20);
  PP_SVD_LANE(24);
  PP_SVD_LANE(28);
  PP_SVD_LANE(32);
#undef PP_SVD_LANE
}

template <int RM, int G>
void launch_cols(hipStream_t st, long long batch, const float* a, float* u, float* s, float* v, int* info, int m,
                 int n, int full, int sort, float tol, int max_sweeps) {
  const long long per_block = kSvdThreads / G;
  const long long blocks = std::min<long long>((batch + per_block - 1) / per_block, 1ll << 20);
  svd_cols_kernel<RM, G><<<dim3((unsigned)blocks), dim3(kSvdThreads), 0, st>>>(a, u, s, v, info, batch, m, n, full,
                                                                                sort, tol, max_sweeps);
}

}  // namespace

extern "C" int pp_batch_svd_f32(const float* a, float* u, float* s, float* v, int* info, long long batch, int m, int n,
                                int full, int sort, float tol, int max_sweeps, void* stream) {
  if (batch < 0 || m < 1 || n < 1 || m > 32 || n > 32 || max_sweeps < 1 || !(tol >= 0.0f)) return PP_EINVAL;
  if (batch == 0) return PP_OK;
  if (!a || !u || !s || !v) return PP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  full = full ? 1 : 0;
  sort = sort ? 1 : 0;
  const int R = std::max(m, n), K = std::min(m, n);
  if (K <= 4) {
    const int blocks = (int)std::min<long long>((batch + kSvdThreads - 1) / kSvdThreads, 1ll << 20);
    switch (K) {
      case 1: dispatch_lane<1>(R, st, blocks, a, u, s, v, info, batch, m, n, full, sort, tol, max_sweeps); break;
      case 2: dispatch_lane<2>(R, st, blocks, a, u, s, v, info, batch, m, n, full, sort, tol, max_sweeps); break;
      case 3: dispatch_lane<3>(R, st, blocks, a, u, s, v, info, batch, m, n, full, sort, tol, max_sweeps); break;
      default: dispatch_lane<4>(R, st, blocks, a, u, s, v, info, batch, m, n, full, sort, tol, max_sweeps); break;
    }
  } else if (K <= 8) {
    if (R <= 8)
      launch_cols<8, 8>(st, batch, a, u, s, v, info, m, n, full, sort, tol, max_sweeps);
    else if (R <= 16)
      launch_cols<16, 8>(st, batch, a, u, s, v, info, m, n, full, sort, tol, max_sweeps);
    else
      launch_cols<32, 8>(st, batch, a, u, s, v, info, m, n, full, sort, tol, max_sweeps);
  } else if (K <= 16) {
    if (R <= 16)
      launch_cols<16, 16>(st, batch, a, u, s, v, info, m, n, full, sort, tol, max_sweeps);
    else
      launch_cols<32, 16>(st, batch, a, u, s, v, info, m, n, full, sort, tol, max_sweeps);
  } else {
    launch_cols<32, 32>(st, batch, a, u, s, v, info, m, n, full, sort, tol, max_sweeps);
  }
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}
