// edge_features.hip -- the edge tensor of an EdgeConv layer (reference network/layers.py:41-62,88-109): with features
// x (B,C,N) in channels-first layout, a graph idx (B,P,K) and the centres query (B,C,P) (the self graph: query = x),
//   out[b,   c, p, k] = query[b,c,p]
//   out[b, C+c, p, k] = x[b,c,idx[b,p,k]] - query[b,c,p]
// The reference gathers (B,P,K+1,C) through an int64 index expansion, permutes, slices, expands and concatenates:
// every step moves a tensor of the output's size or more, and the backward scatters as much.  Here the forward writes
// every output element exactly once, and the backwards are GATHERS with no floating-point atomics:
//   grad_query[b,c,p] = sum_k (g[b,c,p,k] - g[b,C+c,p,k])      ascending k in fp32, starting from the k = 0 term
//   grad_x[b,c,n]     = sum of g[b,C+c,p,k] over the incoming edges (p,k) with idx[b,p,k] == n, walked over the
//                       reverse adjacency of idx (bucket_lists.h's chain: N buckets, P*K edge numbers p*K+k per batch
//                       element), built once per backward call.  `ordered` sorts every list by edge number and adds
//                       plainly from +0.0: the sum of a sequential loop over (p, k).  Otherwise the list keeps the
//                       order in which the cursors were served and the sum is compensated (pp::ListSum).
//   self graph        grad_x = the centre sum, then the incoming terms added to it, in one pass over the point.
// fp16 and bf16 are widened (exact), every operation is made in fp32 and the result is rounded once to nearest even:
// torch's own 16-bit arithmetic.  DESIGN.md §4 "Edge features" states the contract.
//
// An index outside [0, N) is only compared, never used as an address: its difference elements are NaN, and in the
// backward its row (b,p) takes no part in the scatter while grad_query[b,:,p] is NaN.
#include "bucket_lists.h"
#include "pp_b16.h"

namespace {

constexpr int kEfMaxK = 128;
constexpr int kEfThreads = 256;
constexpr int kEfChannels = 64;    // channels per workgroup of the forward: a tile's indices are read once per that many
constexpr int kEfGroup = 2;        // channels per thread of the backwards (measured 1, 2, 4, 8: 2 and 1 lead)
constexpr int kEfTileK = 16;       // neighbours per row staged at a time by the centre sums
constexpr int kEfRows = 64;        // rows of idx per workgroup in the adjacency kernel

template <typename T>
__device__ __forceinline__ T ef_nan() {
  return pp::narrow<T>(pp::quiet_nan());
}

// ---- forward ----------------------------------------------------------------------------------------------------
// The lanes run along the linear (p,k) axis of one batch element; a thread owns V = 16 / sizeof(T) consecutive edges,
// so that both output streams of a channel leave as 16-byte stores wherever P*K is a multiple of V (every plane then
// starts on a 16-byte boundary), and as single elements otherwise and in the last, partial group.  The thread keeps
// its neighbours (-1: out of range) and rows in registers and loops over the workgroup's channels; a channel's row of
// x (N elements) and of query stay in cache for the gathers.  The output is written once and not read back by this
// kernel: its stores are non-temporal (measured at B=32, C=64, N=4096, K=16: 0.36 ms against 0.45 ms with plain
// stores in fp32, 0.19 against 0.25 ms in bf16; README "Edge features").
template <typename T, typename I>
__global__ __launch_bounds__(kEfThreads) void ef_forward_kernel(const T* __restrict__ x, const T* __restrict__ query,
                                                               const I* __restrict__ idx, T* __restrict__ out, int C,
                                                               int N, int P, int K, unsigned tiles) {
  constexpr int V = 16 / (int)sizeof(T);
  struct alignas(16) Pack {
    T v[V];
  };
  const long long PK = (long long)P * K;
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const long long e0 = ((long long)tile * kEfThreads + threadIdx.x) * V;
  if (e0 >= PK) return;
  const int nv = (int)min((long long)V, PK - e0);
  const bool packed = nv == V && PK % V == 0;
  int j[V], p[V];
  const I* __restrict__ row = idx + (size_t)b * PK + e0;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    j[v] = -1;
    p[v] = 0;
    if (v < nv) {
      const long long t = (long long)row[v];
      j[v] = (t < 0 || t >= N) ? -1 : (int)t;
      p[v] = (int)((e0 + v) / K);
    }
  }
  const int c0 = blockIdx.y * kEfChannels, c1 = min(C, c0 + kEfChannels);
  for (int c = c0; c < c1; ++c) {
    const T* __restrict__ xr = x + ((size_t)b * C + c) * N;
    const T* __restrict__ qr = query + ((size_t)b * C + c) * P;
    T* __restrict__ oc = out + ((size_t)b * 2 * C + c) * PK + e0;
    T* __restrict__ od = oc + (size_t)C * PK;
    Pack centre, diff;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (v < nv) {
        const T q = qr[p[v]];
        centre.v[v] = q;
        diff.v[v] = j[v] < 0 ? ef_nan<T>() : pp::narrow<T>(pp::widen(xr[j[v]]) - pp::widen(q));
      }
    }
    if (packed) {
      pp::i4 wc, wd;
      __builtin_memcpy(&wc, &centre, 16);
      __builtin_memcpy(&wd, &diff, 16);
      __builtin_nontemporal_store(wc, reinterpret_cast<pp::i4*>(oc));
      __builtin_nontemporal_store(wd, reinterpret_cast<pp::i4*>(od));
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (v < nv) {
          oc[v] = centre.v[v];
          od[v] = diff.v[v];
        }
      }
    }
  }
}

// ---- row flags and reverse adjacency ----------------------------------------------------------------------------
// MODE 0: flags only (flags[b*P+p] != 0: the row has an index outside [0, N)); 1: flags and in-degrees; 2: the lists.
// A flagged row takes no part in the lists.
template <int MODE, typename I>
__global__ __launch_bounds__(kEfThreads) void ef_adjacency_kernel(const I* __restrict__ idx,
                                                                 unsigned char* __restrict__ flags,
                                                                 unsigned* __restrict__ cursor,
                                                                 unsigned* __restrict__ entries, long long rows, int N,
                                                                 int P, int K) {
  __shared__ int s_bad[kEfRows];
  const int t = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * kEfRows;
  const int nr = (int)min((long long)kEfRows, rows - r0);
  const int ne = nr * K;
  const I* __restrict__ tile = idx + (size_t)r0 * K;
  if (t < kEfRows) s_bad[t] = 0;
  __syncthreads();
  for (int e = t; e < ne; e += kEfThreads) {
    const long long j = (long long)tile[e];
    if (j < 0 || j >= N) s_bad[e / K] = 1;
  }
  __syncthreads();
  if (MODE != 2 && t < nr) flags[r0 + t] = (unsigned char)s_bad[t];
  if (MODE == 0) return;
  for (int e = t; e < ne; e += kEfThreads) {
    const int r = e / K;
    if (s_bad[r]) continue;
    const long long rw = r0 + r;
    const long long b = rw / P;
    const int p = (int)(rw - b * P);
    pp::bucket_put<MODE == 2>(cursor, entries, b, N, (long long)P * K, (size_t)tile[e],
                              (unsigned)p * (unsigned)K + (unsigned)(e - r * K));
  }
}

// ---- backwards --------------------------------------------------------------------------------------------------
// The centre sums of kEfThreads consecutive rows (r0 ...) of one channel: t = g[c,p,k] - g[C+c,p,k], added in
// ascending k from the k = 0 term.  The rows' K elements are one contiguous run of each plane: they are read coalesced,
// kEfTileK neighbours of every row at a time, subtracted and staged in LDS, and thread t then adds row r0 + t's
// terms in order.  Every thread of the workgroup calls this (nr: valid rows); returns the sum of row r0 + t.
template <typename T>
__device__ __forceinline__ float ef_centre_sums(const T* __restrict__ gc, const T* __restrict__ gd, long long r0,
                                                int nr, int K, float (*s_t)[kEfTileK + 1]) {
  const int t = threadIdx.x;
  float acc = 0.0f;
  for (int k0 = 0; k0 < K; k0 += kEfTileK) {
    const int kc = min(kEfTileK, K - k0);
    __syncthreads();
    for (int x = t; x < nr * kEfTileK; x += kEfThreads) {
      const int r = x / kEfTileK, kk = x - r * kEfTileK;
      if (kk < kc) {
        const size_t o = (size_t)(r0 + r) * K + k0 + kk;
        s_t[r][kk] = pp::widen(gc[o]) - pp::widen(gd[o]);
      }
    }
    __syncthreads();
    if (t < nr)
      for (int kk = 0; kk < kc; ++kk) acc = (k0 + kk == 0) ? s_t[t][kk] : acc + s_t[t][kk];
  }
  return acc;
}

// a workgroup per kEfThreads rows p and kEfGroup channels
template <typename T>
__global__ __launch_bounds__(kEfThreads) void ef_grad_query_kernel(const T* __restrict__ g,
                                                                  const unsigned char* __restrict__ flags,
                                                                  T* __restrict__ grad_query, int C, int P, int K,
                                                                  unsigned tiles) {
  __shared__ float s_t[kEfThreads][kEfTileK + 1];
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const long long p0 = (long long)tile * kEfThreads;
  const int nr = (int)min((long long)kEfThreads, P - p0);
  const int t = threadIdx.x;
  const size_t PK = (size_t)P * K;
  const bool bad = t < nr && flags[(size_t)b * P + p0 + t];
  const int c0 = blockIdx.y * kEfGroup, c1 = min(C, c0 + kEfGroup);
  for (int c = c0; c < c1; ++c) {
    const T* __restrict__ gc = g + ((size_t)b * 2 * C + c) * PK;
    const float acc = ef_centre_sums(gc, gc + (size_t)C * PK, p0, nr, K, s_t);
    if (t < nr) grad_query[((size_t)b * C + c) * P + p0 + t] = bad ? ef_nan<T>() : pp::narrow<T>(acc);
  }
}

// One lane per destination point n, kEfGroup channels per thread: the point's list is walked once for the group (it
// is of any length and is never held in registers), two entries at a time, gathering from the planes g[b,C+c] of P*K
// elements; the loads of a step are independent, the additions of a channel keep the list's order.
template <typename T, bool SELF>
__global__ __launch_bounds__(kEfThreads) void ef_grad_x_kernel(const T* __restrict__ g,
                                                              const unsigned char* __restrict__ flags,
                                                              const unsigned* __restrict__ start,
                                                              const unsigned* __restrict__ cursor,
                                                              const unsigned* __restrict__ entries,
                                                              T* __restrict__ grad_x, int C, int N, int P, int K,
                                                              int ordered, unsigned tiles) {
  __shared__ float s_t[SELF ? kEfThreads : 1][kEfTileK + 1];
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const long long n0 = (long long)tile * kEfThreads;
  const int nr = (int)min((long long)kEfThreads, N - n0);
  const int t = threadIdx.x;
  const bool live = t < nr;
  const size_t PK = (size_t)P * K;
  const size_t i = (size_t)b * N + n0 + (live ? t : 0);
  const unsigned q0 = start[i], q1 = live ? cursor[i] : q0;
  const unsigned* __restrict__ list = entries + (size_t)b * PK;
  const bool bad = SELF && flags[i];
  const int c0 = blockIdx.y * kEfGroup;
  const T* __restrict__ gd[kEfGroup];
  pp::ListSum acc[kEfGroup];
#pragma unroll
  for (int u = 0; u < kEfGroup; ++u) {
    const int c = min(c0 + u, C - 1);          // a channel beyond C repeats the last one and is not stored
    const T* __restrict__ gc = g + ((size_t)b * 2 * C + c) * PK;
    gd[u] = gc + (size_t)C * PK;
    acc[u] = {0.0f, 0.0f};
    if (SELF) acc[u].s = ef_centre_sums(gc, gd[u], n0, nr, K, s_t);
  }
  unsigned q = q0;
  for (; q + 1 < q1; q += 2) {
    const unsigned ea = list[q], eb = list[q + 1];
    float va[kEfGroup], vb[kEfGroup];
#pragma unroll
    for (int u = 0; u < kEfGroup; ++u) {
      va[u] = pp::widen(gd[u][ea]);
      vb[u] = pp::widen(gd[u][eb]);
    }
#pragma unroll
    for (int u = 0; u < kEfGroup; ++u) {
      acc[u].add(va[u], ordered);
      acc[u].add(vb[u], ordered);
    }
  }
  if (q < q1) {
    const unsigned ea = list[q];
#pragma unroll
    for (int u = 0; u < kEfGroup; ++u) acc[u].add(pp::widen(gd[u][ea]), ordered);
  }
  if (!live) return;
#pragma unroll
  for (int u = 0; u < kEfGroup; ++u)
    if (c0 + u < C) grad_x[((size_t)b * C + c0 + u) * N + n0 + t] = bad ? ef_nan<T>() : pp::narrow<T>(acc[u].s);
}

// ---- host -------------------------------------------------------------------------------------------------------
bool ef_shape_ok(int B, int C, int N, int P, int K) {
  const long long lim = 0x7fffffffLL;
  return B >= 1 && C >= 1 && N >= 1 && P >= 1 && K >= 1 && K <= kEfMaxK && (long long)P * K <= lim &&
         (long long)B * N <= lim && (long long)B * P <= lim && (long long)B * C <= lim &&
         (long long)B * pp::blocks((long long)P * K, kEfThreads) <= lim &&
         (C + kEfGroup - 1) / kEfGroup <= 65535;
}

struct EfLayout {
  size_t flags, lists, total;   // u8 [B*P], then the bucket scratch
  pp::BucketLayout L;
};
EfLayout ef_layout(int B, int N, int P, int K, bool adjacency) {
  EfLayout W;
  W.flags = 0;
  W.lists = pp::bucket_align((size_t)B * P);
  W.L = pp::bucket_layout(B, N, (long long)P * K, false);
  W.total = W.lists + (adjacency ? W.L.total : 0);
  return W;
}

// calls f(T(), I()) with the element type of dtype (0 fp32, 1 fp16, 2 bf16) and the index type (int64 or int32)
template <typename F>
int ef_dispatch(int dtype, int idx64, F f) {
  if (dtype < 0 || dtype > 2) return PP_EINVAL;
  if (idx64) {
    if (dtype == 0) return f(float(), (long long)0);
    if (dtype == 1) return f(pp::f16(), (long long)0);
    return f(pp::bf16(), (long long)0);
  }
  if (dtype == 0) return f(float(), (int)0);
  if (dtype == 1) return f(pp::f16(), (int)0);
  return f(pp::bf16(), (int)0);
}

template <typename I>
int ef_flags_and_lists(const I* idx, unsigned char* ws, const EfLayout& W, int B, int N, int P, int K, bool adjacency,
                       int ordered, hipStream_t s) {
  const long long rows = (long long)B * P;
  unsigned char* flags = ws + W.flags;
  const dim3 grid(pp::blocks(rows, kEfRows)), block(kEfThreads);
  if (!adjacency) {
    ef_adjacency_kernel<0, I><<<grid, block, 0, s>>>(idx, flags, nullptr, nullptr, rows, N, P, K);
    PP_RETURN_IF_LAUNCH_FAILED();
    return PP_OK;
  }
  unsigned char* lists = ws + W.lists;
  unsigned* cursor = reinterpret_cast<unsigned*>(lists + W.L.cursor);
  unsigned* entries = reinterpret_cast<unsigned*>(lists + W.L.entries);
  return pp::bucket_build(lists, W.L, entries, nullptr, B, N, (long long)P * K, ordered != 0, s, [&](bool fill) {
    if (fill)
      ef_adjacency_kernel<2, I><<<grid, block, 0, s>>>(idx, flags, cursor, entries, rows, N, P, K);
    else
      ef_adjacency_kernel<1, I><<<grid, block, 0, s>>>(idx, flags, cursor, entries, rows, N, P, K);
  });
}

}  // namespace

extern "C" size_t pp_edge_features_workspace_bytes(int B, int N, int P, int K, int adjacency) {
  if (!ef_shape_ok(B, 1, N, P, K)) return 0;
  return ef_layout(B, N, P, K, adjacency != 0).total;
}

extern "C" int pp_edge_features_forward(const void* x, const void* query, const void* idx, void* out, int B, int C,
                                        int N, int P, int K, int dtype, int idx64, void* stream) {
  if (!ef_shape_ok(B, C, N, P, K) || !x || !query || !idx || !out) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return ef_dispatch(dtype, idx64, [&](auto tt, auto ii) {
    using T = decltype(tt);
    using I = decltype(ii);
    constexpr int V = 16 / (int)sizeof(T);
    const unsigned tiles = pp::blocks((long long)P * K, kEfThreads * V);
    const dim3 grid((unsigned)B * tiles, (unsigned)((C + kEfChannels - 1) / kEfChannels));
    ef_forward_kernel<T, I><<<grid, dim3(kEfThreads), 0, s>>>((const T*)x, (const T*)query, (const I*)idx, (T*)out, C,
                                                             N, P, K, tiles);
    PP_RETURN_IF_LAUNCH_FAILED();
    return (int)PP_OK;
  });
}

extern "C" int pp_edge_features_backward(const void* idx, const void* grad_out, void* grad_x, void* grad_query, int B,
                                         int C, int N, int P, int K, int dtype, int idx64, int self_graph, int ordered,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!ef_shape_ok(B, C, N, P, K) || !idx || !grad_out) return PP_EINVAL;
  if (self_graph && (P != N || grad_query)) return PP_EINVAL;
  if (!grad_x && !grad_query) return PP_OK;
  const EfLayout W = ef_layout(B, N, P, K, grad_x != nullptr);
  unsigned char* ws = (unsigned char*)workspace;
  if (!ws || workspace_bytes < W.total) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  return ef_dispatch(dtype, idx64, [&](auto tt, auto ii) {
    using T = decltype(tt);
    using I = decltype(ii);
    const int rc = ef_flags_and_lists((const I*)idx, ws, W, B, N, P, K, grad_x != nullptr, ordered, s);
    if (rc != PP_OK) return rc;
    const unsigned char* flags = ws + W.flags;
    if (grad_query) {
      const unsigned tiles = pp::blocks(P, kEfThreads);
      const dim3 grid((unsigned)B * tiles, (unsigned)((C + kEfGroup - 1) / kEfGroup));
      ef_grad_query_kernel<T><<<grid, dim3(kEfThreads), 0, s>>>((const T*)grad_out, flags, (T*)grad_query, C, P, K,
                                                               tiles);
      PP_RETURN_IF_LAUNCH_FAILED();
    }
    if (grad_x) {
      const unsigned char* lists = ws + W.lists;
      const unsigned* start = reinterpret_cast<const unsigned*>(lists + W.L.start);
      const unsigned* cursor = reinterpret_cast<const unsigned*>(lists + W.L.cursor);
      const unsigned* entries = reinterpret_cast<const unsigned*>(lists + W.L.entries);
      const unsigned tiles = pp::blocks(N, kEfThreads);
      const dim3 grid((unsigned)B * tiles, (unsigned)((C + kEfGroup - 1) / kEfGroup));
      if (self_graph)
        ef_grad_x_kernel<T, true><<<grid, dim3(kEfThreads), 0, s>>>((const T*)grad_out, flags, start, cursor, entries,
                                                                   (T*)grad_x, C, N, P, K, ordered, tiles);
      else
        ef_grad_x_kernel<T, false><<<grid, dim3(kEfThreads), 0, s>>>((const T*)grad_out, flags, start, cursor, entries,
                                                                    (T*)grad_x, C, N, P, K, ordered, tiles);
      PP_RETURN_IF_LAUNCH_FAILED();
    }
    return (int)PP_OK;
  });
}
