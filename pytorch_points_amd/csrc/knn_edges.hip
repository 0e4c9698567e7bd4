// knn_edges.hip -- the two operators on the edges of a k-NN graph that the reference's point-cloud regularisers are
// built from (network/model_loss.py:73-163,362-398, geo_operations.py:128-152): with points (B,N,D) and idx (B,N,K),
//   edge lengths       out[b,n,k] = |points[b,idx[b,n,k]] - points[b,n]|^2, or its square root
//   uniform Laplacian  lap[b,n,:] = -(sum_k points[b,idx[b,n,k],:]) / K + points[b,n,:]
// The reference materialises the (B,N,K,D) gather through a (B,N,K,D) int64 index expansion and scatters the same
// amount back in the backward.  Here no edge ever exists in memory: the forwards are one pass over idx, and the
// backwards are GATHERS.  Once per backward call the reverse adjacency of idx is built (bucket_lists.h's chain: every
// point's bucket receives the numbers n*K+k of its incoming edges), and every point then adds its own centre term
// (ascending k) followed by the terms of its incoming edges.  No floating-point atomics in any form.  `ordered` sorts
// every incoming list by edge number first, so that the sum is the one a sequential loop over (n, k) makes:
// reproducible bit for bit (torch.use_deterministic_algorithms).  Without it a list keeps the order in which the
// cursors were served.
//
// Arithmetic (DESIGN.md "k-NN edge operators"): the squared length is the library's distance chain t0*t0,
// fma(t_c, t_c, acc) in ascending dimension (pp::chamfer_d3; knn.hip's sequential form), the root and the divisions
// are correctly rounded, and with -ffp-contract=off every other line below rounds as it is written.
//
// An index outside [0, N) is never dereferenced: its edge length is NaN, its Laplacian row is NaN, and in the
// backwards its row takes no part in the scatter while its centre point's gradient is NaN.
#include "bucket_lists.h"

namespace {

constexpr int kKeMaxK = 128;
constexpr int kKeMaxD = 32;
constexpr int kKeThreads = 256;
constexpr int kKeRows = 64;        // rows of idx per workgroup in the tiled kernels
constexpr int kKeTileK = 32;       // neighbours per row staged at a time by the Laplacian forward

// ---- forwards ---------------------------------------------------------------------------------------------------
// one thread per edge
template <int DS>
__global__ __launch_bounds__(kKeThreads) void ke_len_forward_kernel(const float* __restrict__ points,
                                                                    const long long* __restrict__ idx,
                                                                    float* __restrict__ out, long long edges, int N,
                                                                    int K, int D, int squared) {
  const long long e = (long long)blockIdx.x * kKeThreads + threadIdx.x;
  if (e >= edges) return;
  const int Dd = DS ? DS : D;
  const long long row = e / K;
  const long long j = idx[e];
  if (j < 0 || j >= N) {
    out[e] = pp::quiet_nan();
    return;
  }
  const float* __restrict__ pc = points + (size_t)row * Dd;
  const float* __restrict__ pj = points + ((size_t)(row / N) * N + (size_t)j) * Dd;
  float d;
  if (DS == 3) {
    d = pp::chamfer_d3(pj[0], pj[1], pj[2], pc[0], pc[1], pc[2]);
  } else {
    const float t0 = pj[0] - pc[0];
    d = t0 * t0;
    for (int c = 1; c < Dd; ++c) {
      const float t = pj[c] - pc[c];
      d = __builtin_fmaf(t, t, d);
    }
  }
  out[e] = squared ? d : sqrtf(d);   // correctly rounded in this build (__fsqrt_rn is the native approximation)
}

// kKeRows rows per workgroup; the rows' indices travel through LDS kKeTileK neighbours at a time (coalesced reads of
// idx), and work item (row, dimension) adds its neighbours' coordinates in ascending k
template <int DS>
__global__ __launch_bounds__(kKeThreads) void ke_lap_forward_kernel(const float* __restrict__ points,
                                                                    const long long* __restrict__ idx,
                                                                    float* __restrict__ lap, long long rows, int N,
                                                                    int K, int D) {
  __shared__ int s_idx[kKeRows][kKeTileK + 1];
  constexpr int U = DS == 3 ? 1 : kKeRows * kKeMaxD / kKeThreads;   // work items per thread
  const int Dd = DS ? DS : D;
  const int t = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * kKeRows;
  const int nr = (int)min((long long)kKeRows, rows - r0);
  const int items = nr * Dd;
  float acc[U];
  unsigned bad = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += kKeTileK) {
    const int kc = min(kKeTileK, K - k0);
    __syncthreads();
    for (int x = t; x < nr * kKeTileK; x += kKeThreads) {
      const int r = x / kKeTileK, kk = x - r * kKeTileK;
      if (kk < kc) {
        const long long j = idx[(size_t)(r0 + r) * K + k0 + kk];
        s_idx[r][kk] = (j < 0 || j >= N) ? -1 : (int)j;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int item = t + kKeThreads * u;
      if (item < items) {
        const int r = item / Dd, c = item - r * Dd;
        const float* __restrict__ pts = points + (size_t)((r0 + r) / N) * N * Dd + c;
        for (int kk = 0; kk < kc; ++kk) {
          const int j = s_idx[r][kk];
          if (j < 0) {
            bad |= 1u << u;
          } else {
            const float v = pts[(size_t)j * Dd];
            acc[u] = (k0 + kk == 0) ? v : acc[u] + v;
          }
        }
      }
    }
  }
  const float kf = (float)K;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int item = t + kKeThreads * u;
    if (item < items) {
      const size_t o = (size_t)r0 * Dd + item;
      const float m = -(acc[u] / kf);
      lap[o] = ((bad >> u) & 1u) ? pp::quiet_nan() : m + points[o];
    }
  }
}

// ---- reverse adjacency ------------------------------------------------------------------------------------------
// FILL = false: in-degrees; FILL = true: the lists.  A row with an out-of-range index takes no part.
template <bool FILL>
__global__ __launch_bounds__(kKeThreads) void ke_adjacency_kernel(const long long* __restrict__ idx,
                                                                  unsigned* __restrict__ cursor,
                                                                  unsigned* __restrict__ entries, long long rows,
                                                                  int N, int K) {
  __shared__ int s_bad[kKeRows];
  const int t = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * kKeRows;
  const int nr = (int)min((long long)kKeRows, rows - r0);
  const int ne = nr * K;
  const long long* __restrict__ tile = idx + (size_t)r0 * K;
  if (t < kKeRows) s_bad[t] = 0;
  __syncthreads();
  for (int e = t; e < ne; e += kKeThreads) {
    const long long j = tile[e];
    if (j < 0 || j >= N) s_bad[e / K] = 1;
  }
  __syncthreads();
  for (int e = t; e < ne; e += kKeThreads) {
    const int r = e / K;
    if (s_bad[r]) continue;
    const long long row = r0 + r;
    const long long b = row / N;
    const int n = (int)(row - b * N);
    pp::bucket_put<FILL>(cursor, entries, b, N, (long long)N * K, (size_t)tile[e],
                         (unsigned)n * (unsigned)K + (unsigned)(e - r * K));
  }
}

// ---- backwards --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ke_len_coef(float g, float o, int squared) {
  if (squared) return 2.0f * g;
  return o == 0.0f ? 0.0f : g / o;   // torch.norm's subgradient at a zero length
}

// The sums of the backwards: plain in the ordered form, compensated otherwise (bucket_lists.h).
using KeSum = pp::ListSum;

// DS == 3: one thread per point; else one thread per (point, dimension).  The point's own edges in ascending k, then
// its incoming list.  `out` is the forward's output (the length, or its square).
template <int DS>
__global__ __launch_bounds__(kKeThreads) void ke_len_backward_kernel(
    const float* __restrict__ points, const long long* __restrict__ idx, const float* __restrict__ out,
    const float* __restrict__ g, float* __restrict__ grad, const unsigned* __restrict__ start,
    const unsigned* __restrict__ cursor, const unsigned* __restrict__ entries, long long rows, int N, int K, int D,
    int squared, int detach, int ordered) {
  constexpr int NC = DS == 3 ? 3 : 1;
  const int Dd = DS ? DS : D;
  const long long tid = (long long)blockIdx.x * kKeThreads + threadIdx.x;
  const long long i = DS == 3 ? tid : tid / Dd;
  if (i >= rows) return;
  const int c0 = DS == 3 ? 0 : (int)(tid - i * Dd);
  const long long b = i / N;
  const float* __restrict__ pts = points + (size_t)b * N * Dd + c0;
  float pc[NC];
  KeSum acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    pc[c] = points[(size_t)i * Dd + c0 + c];
    acc[c] = {0.0f, 0.0f};
  }
  bool bad = false;
  const size_t e0 = (size_t)i * K;
  for (int k = 0; k < K; ++k) {
    const long long j = idx[e0 + k];
    if (j < 0 || j >= N) {
      bad = true;
      continue;
    }
    const float coef = ke_len_coef(g[e0 + k], out[e0 + k], squared);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c].add(coef * (pc[c] - pts[(size_t)j * Dd + c]), ordered);
  }
  if (!detach) {
    const size_t eb = (size_t)b * N * K;
    const unsigned* __restrict__ list = entries + eb;
    for (unsigned q = start[i], q1 = cursor[i]; q < q1; ++q) {
      const unsigned e = list[q];
      const unsigned n = e / (unsigned)K;
      const float coef = ke_len_coef(g[eb + e], out[eb + e], squared);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c].add(-(coef * (pts[(size_t)n * Dd + c] - pc[c])), ordered);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) grad[(size_t)i * Dd + c0 + c] = bad ? pp::quiet_nan() : acc[c].s;
}

template <int DS>
__global__ __launch_bounds__(kKeThreads) void ke_lap_backward_kernel(
    const long long* __restrict__ idx, const float* __restrict__ g, float* __restrict__ grad,
    const unsigned* __restrict__ start, const unsigned* __restrict__ cursor, const unsigned* __restrict__ entries,
    long long rows, int N, int K, int D, int ordered) {
  constexpr int NC = DS == 3 ? 3 : 1;
  const int Dd = DS ? DS : D;
  const long long tid = (long long)blockIdx.x * kKeThreads + threadIdx.x;
  const long long i = DS == 3 ? tid : tid / Dd;
  if (i >= rows) return;
  const int c0 = DS == 3 ? 0 : (int)(tid - i * Dd);
  const long long b = i / N;
  const float* __restrict__ gb = g + (size_t)b * N * Dd + c0;
  bool bad = false;
  for (int k = 0; k < K; ++k) {
    const long long j = idx[(size_t)i * K + k];
    bad |= j < 0 || j >= N;
  }
  KeSum acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = {g[(size_t)i * Dd + c0 + c], 0.0f};
  const float kf = (float)K;
  const unsigned* __restrict__ list = entries + (size_t)b * N * K;
  for (unsigned q = start[i], q1 = cursor[i]; q < q1; ++q) {
    const unsigned n = list[q] / (unsigned)K;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c].add(-(gb[(size_t)n * Dd + c] / kf), ordered);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) grad[(size_t)i * Dd + c0 + c] = bad ? pp::quiet_nan() : acc[c].s;
}

// ---- host -------------------------------------------------------------------------------------------------------
bool ke_shape_ok(int B, int N, int K, int D) {
  return B >= 0 && N >= 0 && K >= 1 && K <= kKeMaxK && D >= 1 && D <= kKeMaxD &&
         (long long)N * K <= 0x7fffffffLL && (long long)B * N <= 0x7fffffffLL &&
         ((long long)B * N * D + kKeThreads - 1) / kKeThreads <= 0x7fffffffLL &&
         ((long long)B * N * K + kKeThreads - 1) / kKeThreads <= 0x7fffffffLL;
}

// the reverse adjacency (bucket_lists.h): the edge numbers n*K+k of a batch element, bucketed by destination point
int ke_build_adjacency(const long long* idx, unsigned char* ws, const pp::BucketLayout& L, int B, int N, int K,
                       int ordered, hipStream_t s) {
  const long long rows = (long long)B * N;
  unsigned* cursor = reinterpret_cast<unsigned*>(ws + L.cursor);
  unsigned* entries = reinterpret_cast<unsigned*>(ws + L.entries);
  return pp::bucket_build(ws, L, entries, nullptr, B, N, (long long)N * K, ordered != 0, s, [&](bool fill) {
    const dim3 grid(pp::blocks(rows, kKeRows)), block(kKeThreads);
    if (fill)
      ke_adjacency_kernel<true><<<grid, block, 0, s>>>(idx, cursor, entries, rows, N, K);
    else
      ke_adjacency_kernel<false><<<grid, block, 0, s>>>(idx, cursor, entries, rows, N, K);
  });
}

}  // namespace

extern "C" size_t pp_knn_edges_workspace_bytes(int B, int N, int K) {
  if (B <= 0 || N <= 0 || !ke_shape_ok(B, N, K, 1)) return 0;
  return pp::bucket_layout(B, N, (long long)N * K, false).total;
}

extern "C" int pp_knn_edge_lengths_forward_f32(const float* points, const long long* idx, float* out, int B, int N,
                                               int K, int D, int squared, void* stream) {
  if (!ke_shape_ok(B, N, K, D)) return PP_EINVAL;
  if (B == 0 || N == 0) return PP_OK;
  if (!points || !idx || !out) return PP_EINVAL;
  const long long edges = (long long)B * N * K;
  hipStream_t s = (hipStream_t)stream;
  if (D == 3)
    ke_len_forward_kernel<3><<<dim3(pp::blocks(edges, kKeThreads)), dim3(kKeThreads), 0, s>>>(points, idx, out, edges,
                                                                                             N, K, D, squared);
  else
    ke_len_forward_kernel<0><<<dim3(pp::blocks(edges, kKeThreads)), dim3(kKeThreads), 0, s>>>(points, idx, out, edges,
                                                                                             N, K, D, squared);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_knn_edge_lengths_backward_f32(const float* points, const long long* idx, const float* out,
                                                const float* grad_out, float* grad_points, int B, int N, int K, int D,
                                                int squared, int detach_neighbors, int ordered, void* workspace,
                                                size_t workspace_bytes, void* stream) {
  if (!ke_shape_ok(B, N, K, D)) return PP_EINVAL;
  if (B == 0 || N == 0) return PP_OK;
  if (!points || !idx || !out || !grad_out || !grad_points) return PP_EINVAL;
  const pp::BucketLayout L = pp::bucket_layout(B, N, (long long)N * K, false);
  unsigned char* ws = (unsigned char*)workspace;
  if (!detach_neighbors && (!ws || workspace_bytes < L.total)) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (!detach_neighbors) {
    const int rc = ke_build_adjacency(idx, ws, L, B, N, K, ordered, s);
    if (rc != PP_OK) return rc;
  }
  const unsigned* start = detach_neighbors ? nullptr : reinterpret_cast<const unsigned*>(ws + L.start);
  const unsigned* cursor = detach_neighbors ? nullptr : reinterpret_cast<const unsigned*>(ws + L.cursor);
  const unsigned* entries = detach_neighbors ? nullptr : reinterpret_cast<const unsigned*>(ws + L.entries);
  const long long rows = (long long)B * N;
  if (D == 3)
    ke_len_backward_kernel<3><<<dim3(pp::blocks(rows, kKeThreads)), dim3(kKeThreads), 0, s>>>(
        points, idx, out, grad_out, grad_points, start, cursor, entries, rows, N, K, D, squared, detach_neighbors, ordered);
  else
    ke_len_backward_kernel<0><<<dim3(pp::blocks(rows * D, kKeThreads)), dim3(kKeThreads), 0, s>>>(
        points, idx, out, grad_out, grad_points, start, cursor, entries, rows, N, K, D, squared, detach_neighbors, ordered);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_knn_laplacian_forward_f32(const float* points, const long long* idx, float* lap, int B, int N,
                                            int K, int D, void* stream) {
  if (!ke_shape_ok(B, N, K, D)) return PP_EINVAL;
  if (B == 0 || N == 0) return PP_OK;
  if (!points || !idx || !lap) return PP_EINVAL;
  const long long rows = (long long)B * N;
  hipStream_t s = (hipStream_t)stream;
  if (D == 3)
    ke_lap_forward_kernel<3><<<dim3(pp::blocks(rows, kKeRows)), dim3(kKeThreads), 0, s>>>(points, idx, lap, rows, N, K, D);
  else
    ke_lap_forward_kernel<0><<<dim3(pp::blocks(rows, kKeRows)), dim3(kKeThreads), 0, s>>>(points, idx, lap, rows, N, K, D);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_knn_laplacian_backward_f32(const long long* idx, const float* grad_lap, float* grad_points, int B,
                                             int N, int K, int D, int ordered, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  if (!ke_shape_ok(B, N, K, D)) return PP_EINVAL;
  if (B == 0 || N == 0) return PP_OK;
  if (!idx || !grad_lap || !grad_points) return PP_EINVAL;
  const pp::BucketLayout L = pp::bucket_layout(B, N, (long long)N * K, false);
  unsigned char* ws = (unsigned char*)workspace;
  if (!ws || workspace_bytes < L.total) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int rc = ke_build_adjacency(idx, ws, L, B, N, K, ordered, s);
  if (rc != PP_OK) return rc;
  const unsigned* start = reinterpret_cast<const unsigned*>(ws + L.start);
  const unsigned* cursor = reinterpret_cast<const unsigned*>(ws + L.cursor);
  const unsigned* entries = reinterpret_cast<const unsigned*>(ws + L.entries);
  const long long rows = (long long)B * N;
  if (D == 3)
    ke_lap_backward_kernel<3><<<dim3(pp::blocks(rows, kKeThreads)), dim3(kKeThreads), 0, s>>>(
        idx, grad_lap, grad_points, start, cursor, entries, rows, N, K, D, ordered);
  else
    ke_lap_backward_kernel<0><<<dim3(pp::blocks(rows * D, kKeThreads)), dim3(kKeThreads), 0, s>>>(
        idx, grad_lap, grad_points, start, cursor, entries, rows, N, K, D, ordered);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}
