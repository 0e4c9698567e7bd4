// bucket_lists.h -- the one chain that builds per-vertex lists of integer codes, for knn_edges.hip (the reverse
// adjacency of a k-NN graph), edge_features.hip (the same over a feature-space graph with its own centres) and
// mesh_edges.hip (unique edges, edge incidence, corner incidence).
//
// A build has B batch elements of N vertices and up to `items` codes per batch element, each belonging to one vertex:
//   count   the caller's kernel sizes every vertex's bucket with integer atomics (bucket_put<false>)
//   scan    one workgroup per batch element turns the sizes into the buckets' first positions
//   fill    the caller's kernel again, now drawing a position from the bucket's cursor and storing its code there
//           (bucket_put<true>); afterwards `cursor` holds every bucket's end
//   sort    optional: every bucket ascending, one lane per bucket, a whole workgroup for a bucket beyond kBucketLong
// No floating-point atomics, and with the sort a result that does not depend on the order in which the atomics were
// served.  bucket_build is the chain; what a thread is, which index is out of range and what is flagged then differs
// per caller and stays in the caller's count-or-fill kernel.
//
// The kernels are templates (instantiated with <0>) so that they are defined once per program although two sources
// include this header, as in pp_common.h.
#pragma once
#include "pp_common.h"

namespace pp {

constexpr int kBucketThreads = 256;
constexpr int kBucketLong = 256;    // buckets beyond this are sorted by a whole workgroup
constexpr int kBucketSortThreads = 1024;
constexpr int kBucketSortBlocks = 256;
constexpr int kBucketScanThreads = 1024;

// scratch of one build, as byte offsets; `owner` (the bucket of every entry: unique edges only) exists on request
struct BucketLayout {
  size_t nlong, cursor, start, longlist, entries, owner, total;
};
inline size_t bucket_align(size_t x) { return (x + 255) & ~(size_t)255; }
inline BucketLayout bucket_layout(int B, int N, long long items, bool with_owner) {
  const size_t rows = (size_t)B * N, all = (size_t)B * (size_t)items;
  BucketLayout L;
  L.nlong = 0;                                     // one counter; zeroed together with the cursors behind it
  L.cursor = 256;                                  // u32 [B*N]: bucket size, then fill cursor, finally the bucket's end
  L.start = L.cursor + bucket_align(4 * rows);     // u32 [B*N]: the bucket's first entry (within the batch element)
  L.longlist = L.start + bucket_align(4 * rows);   // u32 [all / kBucketLong + 1]: buckets with a long list
  L.entries = L.longlist + bucket_align(4 * (all / kBucketLong + 1));   // u32 [B][items]: the codes by bucket
  L.owner = L.entries + bucket_align(4 * all);     // u32 [B][items]: the bucket of every entry
  L.total = L.owner + (with_owner ? bucket_align(4 * all) : 0);
  return L;
}

inline unsigned blocks(long long work, int per_block) { return (unsigned)((work + per_block - 1) / per_block); }

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

// The tail of a count-or-fill kernel, for one valid code of `vertex` in batch element b.  FILL = false: the bucket
// grows by one.  FILL = true: the code is stored at the position drawn from the bucket's cursor, which is below
// `items` (a batch element has no more valid codes than that); returns the entry's index in `entries`.
template <bool FILL>
__device__ __forceinline__ size_t bucket_put(unsigned* __restrict__ cursor, unsigned* __restrict__ entries,
                                             long long b, int N, long long items, size_t vertex, unsigned code) {
  unsigned* cur = cursor + (size_t)b * N + vertex;
  if (!FILL) {
    atomicAdd(cur, 1u);
    return 0;
  }
  const size_t slot = (size_t)b * (size_t)items + atomicAdd(cur, 1u);
  entries[slot] = code;
  return slot;
}

// The sum a vertex makes over its list in the gather backwards (knn_edges.hip, edge_features.hip).  ordered: plain fp32
// additions in the order given, the contract's sequential loop.  Otherwise the order of the list is not defined
// anyway, and the sum is compensated (Kahan): a hub point adds thousands of terms, whose plain sum would lose several
// digits.
struct ListSum {
  float s, comp;
  __device__ __forceinline__ void add(float v, bool ordered) {
    if (ordered) {
      s = s + v;
    } else {
      const float y = v - comp;
      const float t = s + y;
      comp = (t - s) - y;
      s = t;
    }
  }
};

// exclusive scan of one chunk of kBucketScanThreads values inside a workgroup; returns the value's exclusive prefix
// including `carry`, and leaves the chunk's total in *chunk_total (valid after the call for every thread)
__device__ __forceinline__ unsigned bucket_block_scan(unsigned v, unsigned carry, unsigned* s_wave,
                                                      unsigned* chunk_total) {
  const int t = threadIdx.x;
  unsigned incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_up(incl, off);
    if ((t & 63) >= off) incl += o;
  }
  __syncthreads();   // the previous chunk's readers of s_wave are done
  if ((t & 63) == 63) s_wave[t >> 6] = incl;
  __syncthreads();
  unsigned run = carry + incl - v, all = 0;
  for (int w = 0; w < kBucketScanThreads / 64; ++w) {
    const unsigned s = s_wave[w];
    if (w < (t >> 6)) run += s;
    all += s;
  }
  *chunk_total = all;
  return run;
}

// one workgroup per batch element: exclusive scan of the bucket sizes -> start, cursor; start2 (nullable, stride N+1,
// the incidences' public form) receives the same values and the total behind them
template <int>
__global__ __launch_bounds__(kBucketScanThreads) void bucket_scan_kernel(unsigned* __restrict__ cursor,
                                                                         unsigned* __restrict__ start,
                                                                         int* __restrict__ start2, int N) {
  __shared__ unsigned s_wave[kBucketScanThreads / 64];
  const int t = threadIdx.x;
  unsigned* cur = cursor + (size_t)blockIdx.x * N;
  unsigned* st = start + (size_t)blockIdx.x * N;
  int* st2 = start2 ? start2 + (size_t)blockIdx.x * ((size_t)N + 1) : nullptr;
  unsigned carry = 0;
  for (int i0 = 0; i0 < N; i0 += kBucketScanThreads) {
    const int i = i0 + t;
    const unsigned v = i < N ? cur[i] : 0u;
    unsigned chunk;
    const unsigned run = bucket_block_scan(v, carry, s_wave, &chunk);
    if (i < N) {
      st[i] = run;
      cur[i] = run;
      if (st2) st2[i] = (int)run;
    }
    carry += chunk;
  }
  if (st2 && t == 0) st2[N] = (int)carry;
}

// one lane per bucket sorts it ascending (pp::lane_sort); a bucket beyond kBucketLong entries is left to
// bucket_sort_long_kernel.  Equal keys (a pair that several faces share) need no order among themselves.
template <int>
__global__ __launch_bounds__(kBucketThreads) void bucket_sort_kernel(const unsigned* __restrict__ start,
                                                                     const unsigned* __restrict__ cursor,
                                                                     unsigned* __restrict__ entries,
                                                                     unsigned* __restrict__ nlong,
                                                                     unsigned* __restrict__ longlist, long long rows,
                                                                     int N, long long items) {
  const long long i = (long long)blockIdx.x * kBucketThreads + threadIdx.x;
  if (i >= rows) return;
  const unsigned s = start[i], n = cursor[i] - s;
  if (n > (unsigned)kBucketLong) {
    // rows = B*N < 2^31 is checked by every caller's host side (ke_shape_ok, me_build_ok), so a bucket's number fits
    // the word; there are at most all / kBucketLong long buckets
    longlist[atomicAdd(nlong, 1u)] = (unsigned)i;
    return;
  }
  unsigned* grp = entries + (size_t)(i / N) * (size_t)items + s;
  lane_sort(
      n, [&](unsigned a) { return grp[a]; },
      [&](unsigned a, unsigned b) {
        const unsigned e = grp[a];
        grp[a] = grp[b];
        grp[b] = e;
      });
}

// a workgroup per long bucket: bitonic network in place with every comparison ascending (the first step of a merge
// pairs i with its mirror image in the block), so that a list of any length sorts as if padded with +inf
template <int>
__global__ __launch_bounds__(kBucketSortThreads) void bucket_sort_long_kernel(const unsigned* __restrict__ start,
                                                                              const unsigned* __restrict__ cursor,
                                                                              unsigned* entries, const unsigned* nlong,
                                                                              const unsigned* longlist, int N,
                                                                              long long items) {
  const unsigned count = *nlong;
  for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
    const unsigned i = longlist[q];
    const unsigned s = start[i], n = cursor[i] - s;
    unsigned* grp = entries + (size_t)(i / (unsigned)N) * (size_t)items + s;
    auto pass = [&](unsigned mask) {
      for (unsigned a = threadIdx.x; a < n; a += kBucketSortThreads) {
        const unsigned b = a ^ mask;
        if (b > a && b < n) {
          const unsigned x = grp[a], y = grp[b];
          if (x > y) {
            grp[a] = y;
            grp[b] = x;
          }
        }
      }
      __syncthreads();
    };
    for (unsigned k = 2; (k >> 1) < n; k <<= 1) {
      pass(k - 1);
      for (unsigned j = k >> 2; j > 0; j >>= 1) pass(j);
    }
  }
}

inline int bucket_sort(unsigned char* ws, const BucketLayout& L, unsigned* entries, int B, int N, long long items,
                       hipStream_t s) {
  const long long rows = (long long)B * N;
  unsigned* nlong = reinterpret_cast<unsigned*>(ws + L.nlong);
  unsigned* cursor = reinterpret_cast<unsigned*>(ws + L.cursor);
  unsigned* start = reinterpret_cast<unsigned*>(ws + L.start);
  unsigned* longlist = reinterpret_cast<unsigned*>(ws + L.longlist);
  bucket_sort_kernel<0><<<dim3(blocks(rows, kBucketThreads)), dim3(kBucketThreads), 0, s>>>(
      start, cursor, entries, nlong, longlist, rows, N, items);
  PP_RETURN_IF_LAUNCH_FAILED();
  bucket_sort_long_kernel<0><<<dim3(kBucketSortBlocks), dim3(kBucketSortThreads), 0, s>>>(start, cursor, entries,
                                                                                          nlong, longlist, N, items);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

// The chain over the scratch `ws` (laid out by L, B > 0 and N > 0): pass(false) launches the caller's kernel as the
// count pass and pass(true) as the fill pass, both on `s` with ws + L.cursor as the cursors; the lists go to `entries`
// (ws + L.entries, or the caller's own tensor).  start2: bucket_scan_kernel's.  Returns at the first failed launch.
template <typename PASS>
inline int bucket_build(unsigned char* ws, const BucketLayout& L, unsigned* entries, int* start2, int B, int N,
                        long long items, bool sort, hipStream_t s, PASS pass) {
  const hipError_t e = fill_bytes(ws, 0, L.start, s);   // the counter and the bucket sizes
  if (e != hipSuccess) return (int)e;
  pass(false);
  PP_RETURN_IF_LAUNCH_FAILED();
  bucket_scan_kernel<0><<<dim3((unsigned)B), dim3(kBucketScanThreads), 0, s>>>(
      reinterpret_cast<unsigned*>(ws + L.cursor), reinterpret_cast<unsigned*>(ws + L.start), start2, N);
  PP_RETURN_IF_LAUNCH_FAILED();
  pass(true);
  PP_RETURN_IF_LAUNCH_FAILED();
  return sort ? bucket_sort(ws, L, entries, B, N, items, s) : PP_OK;
}

}  // namespace pp
