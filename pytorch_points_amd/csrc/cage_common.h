// cage_common.h -- the tile scheme that mvc.hip, green.hip, mvc2d.hip and green2d.hip share (DESIGN.md "Cage
// coordinates: the shared tile scheme"): one workgroup = one wave = 64 queries of one batch element, per-lane LDS
// columns of stride 65, and a backward that writes one slice of the workspace per workgroup and adds the slices in
// workgroup order.  Only what at least two of the four use: the pair mathematics and the face and edge loops stay
// in their files.
#pragma once
#include <limits.h>

#include "pp_common.h"

namespace pp {
namespace cage {

constexpr int kWave = 64;
constexpr int kStride = 65;                 // LDS column stride (elements)
constexpr int kMaxLds = 160 * 1024;         // LDS per workgroup on gfx950

__device__ __forceinline__ float m_nan(float) { return __builtin_nanf(""); }
__device__ __forceinline__ double m_nan(double) { return __builtin_nan(""); }

// A lane's place on the (tiles, B) grid: its query p of batch element b, the tile's first query p0 and its `rows`
// queries; a lane past P is not live and reads the last row
struct Tile {
  int lane, b, p0, p, rows;
  bool live;
  long long row;
};
__device__ __forceinline__ Tile tile_of(int P) {
  Tile t;
  t.lane = threadIdx.x;
  t.b = blockIdx.y;
  t.p0 = blockIdx.x * kWave;
  t.p = t.p0 + t.lane;
  t.rows = min(kWave, P - t.p0);
  t.live = t.p < P;
  t.row = (long long)t.b * P + (t.live ? t.p : P - 1);
  return t;
}

// every index of the F rows of D indices lies in [0, N)
template <int D>
__device__ __forceinline__ bool faces_ok(const long long* fb, int F, int N) {
  bool ok = true;
  for (int i = 0; i < F * D; ++i) {
    const long long x = fb[i];
    ok = ok && x >= 0 && x < N;
  }
  return ok;
}

// sum over the wave; every lane returns the same bits (xor butterfly: lane i and its partner add the same two values)
template <int K>
__device__ __forceinline__ void wave_sum(double (&x)[K]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int i = 0; i < K; ++i) x[i] += __shfl_xor(x[i], off, kWave);
}

// The LDS transposes.  g and o are (*, ld) arrays whose row r0 is the tile's first; the barriers stay with the
// caller.  rows of n elements -> a column per row, col[j * 65 + r]
template <typename T>
__device__ __forceinline__ void rows_to_columns(const T* g, long long r0, int ld, int rows, int n, int lane, T* col) {
  for (int r = 0; r < rows; ++r) {
    const T* row = g + (r0 + r) * ld;
    for (int j = lane; j < n; j += kWave) col[j * kStride + r] = row[j];
  }
}
// and back
template <typename T>
__device__ __forceinline__ void columns_to_rows(const T* col, int rows, int n, int lane, T* o, long long r0, int ld) {
  for (int r = 0; r < rows; ++r) {
    T* row = o + (r0 + r) * ld;
    for (int j = lane; j < n; j += kWave) row[j] = col[j * kStride + r];
  }
}
// the tile of nf <= 64 items, tile[fi * 65 + lane], out to (and in from) the items' segment of every row
template <typename T>
__device__ __forceinline__ void tile_out(const T* tile, int rows, int nf, int lane, T* o, long long r0, int ld) {
  for (int r = 0; r < rows; ++r)
    if (lane < nf) o[(r0 + r) * ld + lane] = tile[lane * kStride + r];
}
template <typename T>
__device__ __forceinline__ void tile_in(T* tile, int rows, int nf, int lane, const T* g, long long r0, int ld) {
  for (int r = 0; r < rows; ++r)
    if (lane < nf) tile[lane * kStride + r] = g[(r0 + r) * ld + lane];
}

// out[b] (n items) = the workgroups' slices of batch element b, added in workgroup order; NaN for a batch element
// whose first code carries one of `bad` (an out-of-range index: its slices were never written)
template <typename T>
__global__ void reduce_kernel(const T* __restrict__ part, const int* __restrict__ codes, T* __restrict__ out, int B,
                              int P, long long n, int tiles, int bad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * n) return;
  const int b = (int)(i / n);
  const long long k = i - (long long)b * n;
  if (codes[(long long)b * P] & bad) {
    out[i] = m_nan(T(0));
    return;
  }
  T s = T(0);
  for (int t = 0; t < tiles; ++t) s += part[((long long)b * tiles + t) * n + k];
  out[i] = s;
}

// ---- host side ----------------------------------------------------------------------------------------------------
// sizes no cage operator serves: negative ones, a P that tiles_of would overflow on, and an F or N whose slice or
// column index (F * 4, N * 65) would overflow an int
inline bool bad_sizes(int B, int P, int N, int F) {
  return B < 0 || P < 0 || N < 0 || F < 0 || P > INT_MAX - kWave || F > INT_MAX / 4 || N > INT_MAX / kStride;
}
inline int tiles_of(int P) { return (P + kWave - 1) / kWave; }
inline bool grid_ok(int B) { return B <= 65535; }            // gridDim.y of the (tiles, B) grid

// the backward's workspace: a slice of items * width elements per workgroup
inline size_t workspace_bytes(int B, int P, int items, int width, int elem) {
  if (B <= 0 || P <= 0 || items <= 0 || P > INT_MAX - kWave) return 0;
  return (size_t)B * tiles_of(P) * items * width * elem;
}

// whether `kernel` may be launched with `lds` bytes of LDS: up to 64 KiB always, up to 160 KiB where the device allows
template <typename K>
bool lds_fits(K kernel, size_t lds, DeviceFlags& flags) {
  return lds <= (size_t)kMaxLds && (lds <= 65536 || allow_big_lds(kernel, (int)lds, flags) == hipSuccess);
}

}  // namespace cage
}  // namespace pp
