// emd.hip -- the earth mover's distance between two point clouds by the approximate matching of Fan, Su and Guibas
// (2017): ten rounds of "soft-assign by exp(level * d), then cap by what is left", every (k, l) pair walked in every
// round.  Contract in DESIGN.md "Earth mover's distance"; the torch form is emd.emd_composition.
//
//   The match is never stored.  match[k,l] = sum_j exp(level_j d_kl) a_j[k] b_j[l], so its whole state is the factors
//   a (B,10,N) and b (B,10,M); the cost and both gradients rebuild it pair by pair, from the ten factors of the lane's
//   own point in registers and the ten of the staged point in LDS.
//
//   walk         every kernel but the dense one has this shape: a workgroup of 256 lanes owns kEmdOwn = 64 points of one
//                side ("own") of one batch element and walks all points of the other side ("walked"), which come
//                through LDS in tiles of kEmdTile.  Lane t owns point t % 64 and walks the staged points l with
//                l % 4 == t / 64, ascending: its wave is slice t / 64.  The four partial sums of a point meet in LDS
//                and are added as ((p0 + p1) + p2) + p3 by the lanes of wave 0, which also do the epilogue.  That is
//                the one association of every sum over N or M here; it depends on nothing but the sizes.
//   row sweep    own = xyz1.  Step 5 of level j-1 (with b_{j-1} as weights) and step 1 of level j (with remainR) in one
//                launch: one d and two exps per pair.  Level 0 has no step 5 before it and takes its own form.
//   column sweep own = xyz2, weights a_j: steps 2-4.
//   cost         a row walk that gives (B,N) row costs, then one workgroup per batch element that adds them in a fixed
//                order.  gradients: a row walk for xyz1 and a column walk for xyz2, every output word written once.
//   dense        one workgroup per (b, k) row writes match[b,k,:], indexed in 64 bits.
//
// d = (dx dx + dy dy) + dz dz with every operation rounded on its own; exp(level d) is v_exp_f32 of d * (level log2 e).
// No floating-point atomics, no cooperative launch, no spin on another workgroup, nothing synchronises with the host.
// No loop bound and no address depends on the data: NaN and infinite coordinates propagate through the arithmetic and
// cannot hang or fault.  What they give is outside the contract.
#include "pp_common.h"

namespace {

constexpr int kEmdLevels = 10;
constexpr int kEmdThreads = 256;
constexpr int kEmdSlices = 4;                        // waves of a workgroup: each walks every fourth staged point
constexpr int kEmdOwn = kEmdThreads / kEmdSlices;    // own points of a workgroup: one per lane of a wave
constexpr int kEmdTile = 512;                        // staged points: 10 KB (sweeps), 32 KB (cost and gradients)
constexpr int kEmdRecord = 4;                        // float4 words of a staged point with its ten factors
constexpr float kLog2e = 1.4426950408889634f;

// level_j log2(e) for level_j = -4^(7-j), j = 0..8, and a last level 0: a power of four times one rounded constant
__device__ __forceinline__ float emd_scale(int j) {
  constexpr float s[kEmdLevels] = {-16384.0f * kLog2e, -4096.0f * kLog2e, -1024.0f * kLog2e, -256.0f * kLog2e,
                                   -64.0f * kLog2e,    -16.0f * kLog2e,   -4.0f * kLog2e,    -1.0f * kLog2e,
                                   -0.25f * kLog2e,    0.0f};
  return s[j];
}

__device__ __forceinline__ float emd_d(float px, float py, float pz, float qx, float qy, float qz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float emd_exp(float d, float scale) { return __builtin_amdgcn_exp2f(d * scale); }

struct EmdLane {
  int b, own, slice;
  long long i;   // the own point within its batch element; may lie past the end (a lane that only helps to stage)
};
__device__ __forceinline__ EmdLane emd_lane(int blocks_per_element) {
  EmdLane L;
  L.b = blockIdx.x / blocks_per_element;
  L.own = threadIdx.x & (kEmdOwn - 1);
  L.slice = threadIdx.x / kEmdOwn;
  L.i = (long long)(blockIdx.x - (unsigned)L.b * blocks_per_element) * kEmdOwn + L.own;
  return L;
}

// ((p0 + p1) + p2) + p3 of one value per lane: valid in the lanes of slice 0 after the call
__device__ __forceinline__ float emd_combine(float* s_part, const EmdLane& L, float v) {
  __syncthreads();   // the previous use of s_part is read
  s_part[L.slice * kEmdOwn + L.own] = v;
  __syncthreads();
  return ((s_part[L.own] + s_part[kEmdOwn + L.own]) + s_part[2 * kEmdOwn + L.own]) + s_part[3 * kEmdOwn + L.own];
}

// ---- the sweeps of the matching -------------------------------------------------------------------------------------
// sum[w] = sum over the walked points l of exp2(d * scale[w]) * weight_w[l], w < NW, for the lane's slice.
// weight0 == nullptr: the constant `fill` (level 0, where remainR is the multiplicity).
template <int NW>
__device__ __forceinline__ void emd_sweep(float4* s_pt, float* s_w1, float px, float py, float pz,
                                          const float* __restrict__ walked, const float* __restrict__ weight0,
                                          const float* __restrict__ weight1, float fill, int n_walked, float scale0,
                                          float scale1, int slice, float (&sum)[NW]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int w = 0; w < NW; ++w) sum[w] = 0.0f;
  for (int l0 = 0; l0 < n_walked; l0 += kEmdTile) {
    const int n = n_walked - l0 < kEmdTile ? n_walked - l0 : kEmdTile;
    __syncthreads();   // the previous tile's readers are done
    for (int k = t; k < n; k += kEmdThreads) {
      const float* __restrict__ q = walked + (size_t)(l0 + k) * 3;
      s_pt[k] = {q[0], q[1], q[2], weight0 ? weight0[l0 + k] : fill};
      if (NW == 2) s_w1[k] = weight1[l0 + k];
    }
    __syncthreads();
#pragma unroll 4
    for (int j = slice; j < n; j += kEmdSlices) {
      const float4 q = s_pt[j];
      const float d = emd_d(px, py, pz, q.x, q.y, q.z);
      sum[0] += emd_exp(d, scale0) * q.w;
      if (NW == 2) sum[1] += emd_exp(d, scale1) * s_w1[j];
    }
  }
}

// Row sweep of level `level`.  kFirst: remainL = mult_l and remainR = mult_r, nothing to finish.  Otherwise step 5 of
// level - 1 first: remainL = max(0, remainL - a_prev * sum_l exp(level_{-1} d) b_prev[l]).  Then step 1:
// a = remainL / (1e-9 + sum_l exp(level d) remainR[l]).
template <bool kFirst>
__global__ __launch_bounds__(kEmdThreads) void emd_row_kernel(const float* __restrict__ xyz1,
                                                              const float* __restrict__ xyz2, float* __restrict__ a,
                                                              const float* __restrict__ b_factors,
                                                              float* __restrict__ remain_l,
                                                              const float* __restrict__ remain_r, int N, int M,
                                                              int level, float mult_l, float mult_r,
                                                              int blocks_per_element) {
  __shared__ float4 s_pt[kEmdTile];
  __shared__ float s_w1[kFirst ? 1 : kEmdTile];
  __shared__ float s_part[kEmdThreads];
  const EmdLane L = emd_lane(blocks_per_element);
  const bool live = L.i < N;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (live) {
    const float* __restrict__ p = xyz1 + ((size_t)L.b * N + L.i) * 3;
    px = p[0], py = p[1], pz = p[2];
  }
  const float* __restrict__ walked = xyz2 + (size_t)L.b * M * 3;
  float* __restrict__ a_level = a + ((size_t)L.b * kEmdLevels + level) * N;
  if (kFirst) {
    float sum[1];
    emd_sweep<1>(s_pt, s_w1, px, py, pz, walked, nullptr, nullptr, mult_r, M, emd_scale(0), 0.0f, L.slice, sum);
    const float u = emd_combine(s_part, L, sum[0]);
    if (live && L.slice == 0) {
      remain_l[(size_t)L.b * N + L.i] = mult_l;
      a_level[L.i] = mult_l / (1e-9f + u);
    }
  } else {
    float sum[2];
    emd_sweep<2>(s_pt, s_w1, px, py, pz, walked, remain_r + (size_t)L.b * M,
                 b_factors + ((size_t)L.b * kEmdLevels + (level - 1)) * M, 0.0f, M, emd_scale(level),
                 emd_scale(level - 1), L.slice, sum);
    const float u = emd_combine(s_part, L, sum[0]);
    const float taken = emd_combine(s_part, L, sum[1]);
    if (live && L.slice == 0) {
      const float a_prev = a_level[L.i - N];   // level - 1 of the same point
      const float left = fmaxf(0.0f, remain_l[(size_t)L.b * N + L.i] - a_prev * taken);
      remain_l[(size_t)L.b * N + L.i] = left;
      a_level[L.i] = left / (1e-9f + u);
    }
  }
}

// Column sweep of level `level`, steps 2-4: s = (sum_k exp(level d) a[k]) remainR, b = min(remainR / (s + 1e-9), 1)
// remainR, remainR = max(0, remainR - s).
template <bool kFirst>
__global__ __launch_bounds__(kEmdThreads) void emd_col_kernel(const float* __restrict__ xyz1,
                                                              const float* __restrict__ xyz2,
                                                              const float* __restrict__ a, float* __restrict__ b_factors,
                                                              float* __restrict__ remain_r, int N, int M, int level,
                                                              float mult_r, int blocks_per_element) {
  __shared__ float4 s_pt[kEmdTile];
  __shared__ float s_part[kEmdThreads];
  const EmdLane L = emd_lane(blocks_per_element);
  const bool live = L.i < M;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (live) {
    const float* __restrict__ p = xyz2 + ((size_t)L.b * M + L.i) * 3;
    px = p[0], py = p[1], pz = p[2];
  }
  float sum[1];
  emd_sweep<1>(s_pt, nullptr, px, py, pz, xyz1 + (size_t)L.b * N * 3, a + ((size_t)L.b * kEmdLevels + level) * N,
               nullptr, 0.0f, N, emd_scale(level), 0.0f, L.slice, sum);
  const float v = emd_combine(s_part, L, sum[0]);
  if (live && L.slice == 0) {
    const size_t x = (size_t)L.b * M + L.i;
    const float r = kFirst ? mult_r : remain_r[x];
    const float s = v * r;
    b_factors[((size_t)L.b * kEmdLevels + level) * M + L.i] = fminf(r / (s + 1e-9f), 1.0f) * r;
    remain_r[x] = fmaxf(0.0f, r - s);
  }
}

// ---- the match rebuilt from its factors -----------------------------------------------------------------------------
// sum_j (exp(level_j d) a_j) b_j, j ascending from +0
__device__ __forceinline__ float emd_match(float d, const float (&fa)[kEmdLevels], const float (&fb)[kEmdLevels]) {
  float m = 0.0f;
#pragma unroll
  for (int j = 0; j < kEmdLevels; ++j) m += (emd_exp(d, emd_scale(j)) * fa[j]) * fb[j];
  return m;
}

__device__ __forceinline__ void emd_load_factors(const float* __restrict__ f, size_t stride, float (&out)[kEmdLevels]) {
#pragma unroll
  for (int j = 0; j < kEmdLevels; ++j) out[j] = f[j * stride];
}

// One walk for the cost and both gradients.  kRows: own = xyz1 with the factors a, walked = xyz2 with b; otherwise the
// roles are exchanged (the match keeps its association: the a factor is multiplied first).
//   !kGrad   out (B,N) = sum_l match sqrt(d)                                            (kRows only)
//   kGrad    out (B,own,3) = grad_cost[b] * sum_walked (match / max(sqrt(d), 1e-20)) (own - walked)
template <bool kRows, bool kGrad>
__global__ __launch_bounds__(kEmdThreads) void emd_pairs_kernel(const float* __restrict__ own_xyz,
                                                                const float* __restrict__ walked_xyz,
                                                                const float* __restrict__ own_factors,
                                                                const float* __restrict__ walked_factors,
                                                                const float* __restrict__ grad_cost,
                                                                float* __restrict__ out, int n_own, int n_walked,
                                                                int blocks_per_element) {
  __shared__ float4 s_rec[kEmdTile * kEmdRecord];   // (x, y, z, f0) (f1..f4) (f5..f8) (f9, 0, 0, 0)
  __shared__ float s_part[kEmdThreads];
  const int t = threadIdx.x;
  const EmdLane L = emd_lane(blocks_per_element);
  const bool live = L.i < n_own;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  float fo[kEmdLevels] = {};
  if (live) {
    const float* __restrict__ p = own_xyz + ((size_t)L.b * n_own + L.i) * 3;
    px = p[0], py = p[1], pz = p[2];
    emd_load_factors(own_factors + (size_t)L.b * kEmdLevels * n_own + L.i, (size_t)n_own, fo);
  }
  const float* __restrict__ wb = walked_xyz + (size_t)L.b * n_walked * 3;
  const float* __restrict__ wf = walked_factors + (size_t)L.b * kEmdLevels * n_walked;
  float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
  for (int l0 = 0; l0 < n_walked; l0 += kEmdTile) {
    const int n = n_walked - l0 < kEmdTile ? n_walked - l0 : kEmdTile;
    __syncthreads();   // the previous tile's readers are done
    for (int k = t; k < n; k += kEmdThreads) {
      const float* __restrict__ q = wb + (size_t)(l0 + k) * 3;
      float f[kEmdLevels];
      emd_load_factors(wf + l0 + k, (size_t)n_walked, f);
      s_rec[k * kEmdRecord] = {q[0], q[1], q[2], f[0]};
      s_rec[k * kEmdRecord + 1] = {f[1], f[2], f[3], f[4]};
      s_rec[k * kEmdRecord + 2] = {f[5], f[6], f[7], f[8]};
      s_rec[k * kEmdRecord + 3] = {f[9], 0.0f, 0.0f, 0.0f};
    }
    __syncthreads();
    for (int j = L.slice; j < n; j += kEmdSlices) {
      const float4 r0 = s_rec[j * kEmdRecord], r1 = s_rec[j * kEmdRecord + 1], r2 = s_rec[j * kEmdRecord + 2];
      const float f9 = s_rec[j * kEmdRecord + 3].x;
      const float fw[kEmdLevels] = {r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, f9};
      const float dx = px - r0.x, dy = py - r0.y, dz = pz - r0.z;
      const float d = (dx * dx + dy * dy) + dz * dz;
      const float m = kRows ? emd_match(d, fo, fw) : emd_match(d, fw, fo);
      const float root = __builtin_sqrtf(d);
      if (kGrad) {
        const float w = m / fmaxf(root, 1e-20f);
        acc0 += w * dx;
        acc1 += w * dy;
        acc2 += w * dz;
      } else {
        acc0 += m * root;
      }
    }
  }
  const float v0 = emd_combine(s_part, L, acc0);
  if (kGrad) {
    const float v1 = emd_combine(s_part, L, acc1);
    const float v2 = emd_combine(s_part, L, acc2);
    if (live && L.slice == 0) {
      const float g = grad_cost[L.b];
      float* __restrict__ o = out + ((size_t)L.b * n_own + L.i) * 3;
      o[0] = g * v0;
      o[1] = g * v1;
      o[2] = g * v2;
    }
  } else if (live && L.slice == 0) {
    out[(size_t)L.b * n_own + L.i] = v0;
  }
}

// cost[b] = the row costs of b: lane t adds rows t, t + 256, ... ascending from +0, then a binary tree over the lanes
__global__ __launch_bounds__(kEmdThreads) void emd_cost_sum_kernel(const float* __restrict__ row_cost,
                                                                   float* __restrict__ cost, int N) {
  __shared__ float s_sum[kEmdThreads];
  const int t = threadIdx.x;
  const float* __restrict__ rows = row_cost + (size_t)blockIdx.x * N;
  float acc = 0.0f;
  for (int k = t; k < N; k += kEmdThreads) acc += rows[k];
  s_sum[t] = acc;
  __syncthreads();
  for (int half = kEmdThreads / 2; half > 0; half >>= 1) {
    if (t < half) s_sum[t] += s_sum[t + half];
    __syncthreads();
  }
  if (t == 0) cost[blockIdx.x] = s_sum[0];
}

// match[b,k,:] by the workgroup of row (b,k)
__global__ __launch_bounds__(kEmdThreads) void emd_dense_kernel(const float* __restrict__ xyz1,
                                                                const float* __restrict__ xyz2,
                                                                const float* __restrict__ a,
                                                                const float* __restrict__ b_factors,
                                                                float* __restrict__ match, int N, int M) {
  const long long row = blockIdx.x;   // b * N + k
  const long long b = row / N;
  const float* __restrict__ p = xyz1 + (size_t)row * 3;
  const float px = p[0], py = p[1], pz = p[2];
  float fa[kEmdLevels], fb[kEmdLevels];
  emd_load_factors(a + (size_t)b * kEmdLevels * N + (row - b * N), (size_t)N, fa);
  const float* __restrict__ qb = xyz2 + (size_t)b * M * 3;
  const float* __restrict__ bf = b_factors + (size_t)b * kEmdLevels * M;
  float* __restrict__ out = match + (size_t)row * M;
  for (int l = threadIdx.x; l < M; l += kEmdThreads) {
    emd_load_factors(bf + l, (size_t)M, fb);
    const float d = emd_d(px, py, pz, qb[(size_t)l * 3], qb[(size_t)l * 3 + 1], qb[(size_t)l * 3 + 2]);
    out[l] = emd_match(d, fa, fb);
  }
}

// a negative size, or B*N or B*M beyond 2^31 - 1
bool emd_sizes_ok(int B, int N, int M) {
  if (B < 0 || N < 0 || M < 0) return false;
  return (long long)B * N <= 0x7fffffffLL && (long long)B * M <= 0x7fffffffLL;
}

unsigned emd_blocks(int B, int n_own) { return (unsigned)((long long)B * ((n_own + kEmdOwn - 1) / kEmdOwn)); }

}  // namespace

extern "C" size_t pp_emd_workspace_bytes(int B, int N, int M) {
  if (!emd_sizes_ok(B, N, M)) return 0;
  return ((size_t)B * N + (size_t)B * M) * sizeof(float);
}

extern "C" int pp_emd_match_f32(const float* xyz1, const float* xyz2, float* a, float* b, int B, int N, int M,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!emd_sizes_ok(B, N, M)) return PP_EINVAL;
  if (B == 0 || N == 0 || M == 0) return PP_OK;
  if (!xyz1 || !xyz2 || !a || !b || !workspace || workspace_bytes < pp_emd_workspace_bytes(B, N, M)) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* remain_l = (float*)workspace;
  float* remain_r = remain_l + (size_t)B * N;
  const int big = N > M ? N : M;
  const float mult_l = (float)(big / N), mult_r = (float)(big / M);
  const int per_row = (N + kEmdOwn - 1) / kEmdOwn, per_col = (M + kEmdOwn - 1) / kEmdOwn;
  const dim3 rows(emd_blocks(B, N)), cols(emd_blocks(B, M)), threads(kEmdThreads);
  emd_row_kernel<true><<<rows, threads, 0, s>>>(xyz1, xyz2, a, b, remain_l, remain_r, N, M, 0, mult_l, mult_r, per_row);
  PP_RETURN_IF_LAUNCH_FAILED();
  emd_col_kernel<true><<<cols, threads, 0, s>>>(xyz1, xyz2, a, b, remain_r, N, M, 0, mult_r, per_col);
  PP_RETURN_IF_LAUNCH_FAILED();
  for (int level = 1; level < kEmdLevels; ++level) {
    emd_row_kernel<false><<<rows, threads, 0, s>>>(xyz1, xyz2, a, b, remain_l, remain_r, N, M, level, mult_l, mult_r,
                                                   per_row);
    PP_RETURN_IF_LAUNCH_FAILED();
    emd_col_kernel<false><<<cols, threads, 0, s>>>(xyz1, xyz2, a, b, remain_r, N, M, level, mult_r, per_col);
    PP_RETURN_IF_LAUNCH_FAILED();
  }
  return PP_OK;
}

extern "C" int pp_emd_dense_f32(const float* xyz1, const float* xyz2, const float* a, const float* b, float* match,
                                int B, int N, int M, void* stream) {
  if (!emd_sizes_ok(B, N, M)) return PP_EINVAL;
  if (B == 0 || N == 0 || M == 0) return PP_OK;
  if (!xyz1 || !xyz2 || !a || !b || !match) return PP_EINVAL;
  emd_dense_kernel<<<dim3((unsigned)(B * N)), dim3(kEmdThreads), 0, (hipStream_t)stream>>>(xyz1, xyz2, a, b, match, N,
                                                                                          M);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_emd_cost_f32(const float* xyz1, const float* xyz2, const float* a, const float* b, float* cost,
                               int B, int N, int M, void* workspace, size_t workspace_bytes, void* stream) {
  if (!emd_sizes_ok(B, N, M)) return PP_EINVAL;
  if (B == 0 || N == 0 || M == 0) return PP_OK;
  if (!xyz1 || !xyz2 || !a || !b || !cost || !workspace || workspace_bytes < (size_t)B * N * sizeof(float))
    return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* row_cost = (float*)workspace;
  emd_pairs_kernel<true, false><<<dim3(emd_blocks(B, N)), dim3(kEmdThreads), 0, s>>>(
      xyz1, xyz2, a, b, nullptr, row_cost, N, M, (N + kEmdOwn - 1) / kEmdOwn);
  PP_RETURN_IF_LAUNCH_FAILED();
  emd_cost_sum_kernel<<<dim3((unsigned)B), dim3(kEmdThreads), 0, s>>>(row_cost, cost, N);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_emd_cost_backward_f32(const float* xyz1, const float* xyz2, const float* a, const float* b,
                                        const float* grad_cost, float* grad_xyz1, float* grad_xyz2, int B, int N, int M,
                                        void* stream) {
  if (!emd_sizes_ok(B, N, M)) return PP_EINVAL;
  if (B == 0 || N == 0 || M == 0) return PP_OK;
  if (!xyz1 || !xyz2 || !a || !b || !grad_cost) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (grad_xyz1) {
    emd_pairs_kernel<true, true><<<dim3(emd_blocks(B, N)), dim3(kEmdThreads), 0, s>>>(
        xyz1, xyz2, a, b, grad_cost, grad_xyz1, N, M, (N + kEmdOwn - 1) / kEmdOwn);
    PP_RETURN_IF_LAUNCH_FAILED();
  }
  if (grad_xyz2) {
    emd_pairs_kernel<false, true><<<dim3(emd_blocks(B, M)), dim3(kEmdThreads), 0, s>>>(
        xyz2, xyz1, b, a, grad_cost, grad_xyz2, M, N, (M + kEmdOwn - 1) / kEmdOwn);
    PP_RETURN_IF_LAUNCH_FAILED();
  }
  return PP_OK;
}
