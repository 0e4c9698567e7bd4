// sampling.hip -- gather_points, ball_query, group_points, three_nn, three_interpolate for gfx950.
// Replaces the reference's _ext/sampling_cuda.cu (gather :9-84, ball_query :340-397,
// group_points :447-513) and _ext/interpolate_gpu.cu (three_nn :9-74, three_interpolate :77-160).
#include "grid_common.h"
#include "pp_b16.h"

namespace pp {  // scatter.hip
size_t ssa_workspace_bytes(int B, long long P, int R, int Nd, bool weighted);
int ssa_run(const float* src, const int* dst, const float* weight, float* out, int B, int C,
            long long P, int R, int Nd, long long src_bstride, void* workspace, hipStream_t s, bool ordered);
// 16-bit sources (DESIGN.md §4 "16-bit features"): the same triples, `out` WRITTEN and rounded once
int ssa_run(const f16* src, const int* dst, const float* weight, f16* out, int B, int C,
            long long P, int R, int Nd, long long src_bstride, void* workspace, hipStream_t s, bool ordered);
int ssa_run(const bf16* src, const int* dst, const float* weight, bf16* out, int B, int C,
            long long P, int R, int Nd, long long src_bstride, void* workspace, hipStream_t s, bool ordered);
}  // namespace pp

namespace {

using pp::dist3;

// ------------------------------------------------------------------------------------------------
// The copying forward kernels are templates on the element E: float, or any 2-byte element as u16 (a copy moves
// bits, so one set of kernels serves fp16 and bf16: DESIGN.md §4 "16-bit features").  A lane of a vector form owns
// L = 16 / sizeof(E) consecutive positions -- a quad of floats, an octet of u16: 16 bytes either way.  Indices stay
// int32 and weights fp32; three_interpolate widens 16-bit features to fp32, runs the fp32 chain and rounds once.
// Every guard of a vector form names its real requirement: a row (b, c) starts at byte (b * C + c) * N * sizeof(E),
// 16-byte aligned only if N % L == 0, and the element-sized scalar forms serve any shape.
// ------------------------------------------------------------------------------------------------
typedef uint16_t u16;
typedef unsigned u4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack2(u16 lo, u16 hi) { return (unsigned)lo | ((unsigned)hi << 16); }
// the L indices of a lane's positions: L / 4 16-byte loads
template <int L>
__device__ __forceinline__ void load_indices(int (&ii)[L], const int* __restrict__ p) {
#pragma unroll
  for (int j = 0; j < L; j += 4) {
    const pp::i4 q = *reinterpret_cast<const pp::i4*>(p + j);
    ii[j] = q.x; ii[j + 1] = q.y; ii[j + 2] = q.z; ii[j + 3] = q.w;
  }
}
// 16 bytes of gathered elements s[ii[0]], s[ii[1]], ...
__device__ __forceinline__ pp::f4 gather16(const float* s, const int (&ii)[4]) {
  return pp::f4{s[ii[0]], s[ii[1]], s[ii[2]], s[ii[3]]};
}
__device__ __forceinline__ u4v gather16(const u16* s, const int (&ii)[8]) {
  return u4v{pack2(s[ii[0]], s[ii[1]]), pack2(s[ii[2]], s[ii[3]]), pack2(s[ii[4]], s[ii[5]]), pack2(s[ii[6]], s[ii[7]])};
}
// the same from two index quads, for group_points_lds_b16_kernel alone: its quads come out of a `p < P ? load : 0`
// select, and filled element by element into an int[8] behind that select the kernel compiles to another stream
__device__ __forceinline__ u4v gather8(const u16* s, const pp::i4& a, const pp::i4& b) {
  return u4v{pack2(s[a.x], s[a.y]), pack2(s[a.z], s[a.w]), pack2(s[b.x], s[b.y]), pack2(s[b.z], s[b.w])};
}
// a plain 16-byte store (fp32 through HIP's float4, the type group_points_kernel has always stored: hipcc addresses a
// store of pp::f4 differently, and the kernels' instruction streams are held fixed)
__device__ __forceinline__ void store16(float* p, const pp::f4& v) {
  *reinterpret_cast<float4*>(p) = make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store16(u16* p, const u4v& v) { *reinterpret_cast<u4v*>(p) = v; }
template <typename E, typename V16>  // the same past the caches
__device__ __forceinline__ void store16_nt(E* p, const V16& v) {
  __builtin_nontemporal_store(v, reinterpret_cast<V16*>(p));
}

// ------------------------------------------------------------------------------------------------
// gather_points: out[b,c,m] = points[b,c,idx[b,m]]            (ref sampling_cuda.cu:9-25)
// One thread per (b, m) column quad walks all channels: idx is read once, stores are contiguous.
// ------------------------------------------------------------------------------------------------
template <typename E>  // float, or any 2-byte element as uint16_t (a copy moves bits)
__global__ __launch_bounds__(256) void gather_fwd_kernel(const E* __restrict__ points,
                                                         const int* __restrict__ idx,
                                                         E* __restrict__ out, int C, int N,
                                                         int M, int c_per_block) {
  const int b = blockIdx.z;
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int i = idx[(size_t)b * M + m];
  const int c0 = blockIdx.y * c_per_block;
  const int c1 = min(C, c0 + c_per_block);
  for (int c = c0; c < c1; ++c)
    out[((size_t)b * C + c) * M + m] = points[((size_t)b * C + c) * N + i];
}

// gather_points through the LDS: a workgroup stages the row points[b,c,:] (coalesced 16-byte loads)
// and gathers from LDS, CPB channels in turn, the next row's loads in flight while this one is
// gathered.  Reads 4 N bytes per row instead of one 64-byte sector per gathered element: the better
// deal when N <= 16 M.  XCD mapping as group_points: idx of one batch element is read by one L2.
// VEC is the fp32 vector form; the element-sized form (VEC = false) also serves E = u16.
template <int KR, bool VEC, typename E = float>
__global__ __launch_bounds__(1024) void gather_fwd_lds_kernel(const E* __restrict__ points,
                                                              const int* __restrict__ idx,
                                                              E* __restrict__ out, int B, int C, int N,
                                                              int M, int cpb, int groups) {
  static_assert(!VEC || sizeof(E) == 4, "the 16-bit vector form is gather_fwd_lds_b16_kernel");
  extern __shared__ __attribute__((aligned(16))) unsigned char s_graw[];
  E* s_grow = reinterpret_cast<E*>(s_graw);
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / groups);
  if (b >= B) return;
  const int c0 = (y % groups) * cpb;
  const int c1 = min(C, c0 + cpb);
  const int t = threadIdx.x;
  const int* __restrict__ ib = idx + (size_t)b * M;
  if constexpr (VEC) {
    const int n4 = N >> 2;
    pp::f4 pre[KR];
    auto load_row = [&](int c) {
      const pp::f4* __restrict__ row = reinterpret_cast<const pp::f4*>(points + ((size_t)b * C + c) * N);
#pragma unroll
      for (int k = 0; k < KR; ++k) pre[k] = row[min(t + 1024 * k, n4 - 1)];
    };
    load_row(c0);
    for (int c = c0; c < c1; ++c) {
      __syncthreads();  // the previous row has been gathered
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (t + 1024 * k < n4) reinterpret_cast<pp::f4*>(s_grow)[t + 1024 * k] = pre[k];
      __syncthreads();
      if (c + 1 < c1) load_row(c + 1);
      float* __restrict__ o = out + ((size_t)b * C + c) * M;
      for (int m = t * 4; m < M; m += 4096) {
        const pp::i4 i = *reinterpret_cast<const pp::i4*>(ib + m);
        pp::f4 r = {s_grow[i.x], s_grow[i.y], s_grow[i.z], s_grow[i.w]};
        *reinterpret_cast<pp::f4*>(o + m) = r;
      }
    }
  } else {  // no alignment assumed: element-sized accesses, all coalesced
    for (int c = c0; c < c1; ++c) {
      __syncthreads();
      const E* __restrict__ row = points + ((size_t)b * C + c) * N;
      for (int e = t; e < N; e += 1024) s_grow[e] = row[e];
      __syncthreads();
      E* __restrict__ o = out + ((size_t)b * C + c) * M;
      for (int m = t; m < M; m += 1024) o[m] = s_grow[ib[m]];
    }
  }
}

// The 16-bit vector form (N % 8 == 0, M % 8 == 0, 16-byte aligned pointers): 16-byte row loads, two index quads and
// one 16-byte store per lane.  Unlike the fp32 vector form it loads each row between the barriers: no next row in
// flight through KR registers.
__global__ __launch_bounds__(1024) void gather_fwd_lds_b16_kernel(const u16* __restrict__ points,
                                                                  const int* __restrict__ idx,
                                                                  u16* __restrict__ out, int B, int C, int N,
                                                                  int M, int cpb, int groups) {
  extern __shared__ __attribute__((aligned(16))) u16 s_g16[];
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / groups);
  if (b >= B) return;
  const int c0 = (y % groups) * cpb;
  const int c1 = min(C, c0 + cpb);
  const int t = threadIdx.x;
  const int* __restrict__ ib = idx + (size_t)b * M;
  for (int c = c0; c < c1; ++c) {
    __syncthreads();  // the previous row has been gathered
    const u16* __restrict__ row = points + ((size_t)b * C + c) * N;
    u16* __restrict__ o = out + ((size_t)b * C + c) * M;
    for (int e = t; e < (N >> 3); e += 1024) reinterpret_cast<u4v*>(s_g16)[e] = reinterpret_cast<const u4v*>(row)[e];
    __syncthreads();
    for (int m = t * 8; m < M; m += 8192) {
      int ii[8];
      load_indices(ii, ib + m);
      store16(o + m, gather16(s_g16, ii));
    }
  }
}

// gather backward: grad_points[b,c,idx[b,m]] += grad_out[b,c,m]   (ref sampling_cuda.cu:47-64)
__global__ __launch_bounds__(256) void gather_bwd_kernel(const float* __restrict__ grad_out,
                                                         const int* __restrict__ idx,
                                                         float* __restrict__ grad_points, int C,
                                                         int N, int M, int c_per_block) {
  const int b = blockIdx.z;
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int i = idx[(size_t)b * M + m];
  const int c0 = blockIdx.y * c_per_block;
  const int c1 = min(C, c0 + c_per_block);
  for (int c = c0; c < c1; ++c)
    atomicAdd(grad_points + ((size_t)b * C + c) * N + i, grad_out[((size_t)b * C + c) * M + m]);
}

// ------------------------------------------------------------------------------------------------
// ball_query (ref sampling_cuda.cu:340-376): per centre the first `nsample` indices k (ascending)
// with dist3 < radius^2 (strict), padded with the first hit; rows with no hit are all zero.
//
// One lane per centre; the scanned point is wave-uniform (scalar loads -> SGPR operands), so the
// per-pair cost is 3 sub + 1 mul + 2 fma + 1 compare and a scalar branch over the rare hit path.
// Each wave stages its 64 rows (64 x nsample ints, contiguous in the output) in LDS and writes
// them out once with fully coalesced stores, including the padding -- the output needs no
// pre-zeroing.  The wave leaves the scan as soon as all of its centres are full.
// ------------------------------------------------------------------------------------------------
constexpr int kBqGroup = 8;

template <bool STAGE_LDS>
__global__ __launch_bounds__(256) void ball_query_kernel(const float* __restrict__ new_xyz,
                                                         const float* __restrict__ xyz,
                                                         int* __restrict__ idx, int N, int M,
                                                         float radius2, int nsample,
                                                         int tiles_per_b, const pp::GridSet* __restrict__ skip) {
  extern __shared__ __attribute__((aligned(16))) int s_rows[];  // [4 waves][64][nsample]
  const int b = blockIdx.x / tiles_per_b;
  const int tile = blockIdx.x - b * tiles_per_b;
  if (skip && skip[b].pad[0]) return;  // this batch element was handled by the grid search
  const int wave = pp::wave_id_uniform();
  const int lane = threadIdx.x & 63;
  const int m0 = tile * 256 + wave * 64;  // first centre of this wave
  if (m0 >= M) return;                    // wave-uniform
  const int m = m0 + lane;
  const bool valid = m < M;
  const int mc = valid ? m : M - 1;
  const float* __restrict__ q = new_xyz + ((size_t)b * M + mc) * 3;
  const float* __restrict__ p = xyz + (size_t)b * N * 3;
  const float qx = q[0], qy = q[1], qz = q[2];
  int* __restrict__ grow = idx + ((size_t)b * M + m) * nsample;  // this lane's output row
  int* srow = s_rows + ((size_t)wave * 64 + lane) * nsample;

  int cnt = valid ? 0 : nsample;  // out-of-range lanes count as full
  int first = 0;
  auto hit = [&](int k) {
    if (cnt == 0) first = k;
    if (STAGE_LDS)
      srow[cnt] = k;
    else
      grow[cnt] = k;
    ++cnt;
  };
  const int ngroups = N / kBqGroup;
  int k = 0;
  for (int g = 0; g < ngroups; ++g, k += kBqGroup) {
    if (__all(cnt >= nsample)) break;
    const float* __restrict__ rp = p + (size_t)k * 3;  // wave-uniform
    float rr[kBqGroup * 3];
#pragma unroll
    for (int e = 0; e < kBqGroup * 3; ++e) rr[e] = rp[e];
    float d[kBqGroup];
    bool any = false;
#pragma unroll
    for (int e = 0; e < kBqGroup; ++e) {
      d[e] = dist3(qx, qy, qz, rr[3 * e], rr[3 * e + 1], rr[3 * e + 2]);
      any |= d[e] < radius2;
    }
    if (__any(any)) {
#pragma unroll
      for (int e = 0; e < kBqGroup; ++e)
        if (d[e] < radius2 && cnt < nsample) hit(k + e);
    }
  }
  if (!__all(cnt >= nsample)) {
    for (k = ngroups * kBqGroup; k < N; ++k) {
      const float d = dist3(qx, qy, qz, p[3 * (size_t)k], p[3 * (size_t)k + 1], p[3 * (size_t)k + 2]);
      if (d < radius2 && cnt < nsample) hit(k);
    }
  }

  if (STAGE_LDS) {
    // rows of the wave's 64 centres are one contiguous run of 64*nsample ints in the output
    const int* wrows = s_rows + (size_t)wave * 64 * nsample;
    int* __restrict__ gout = idx + ((size_t)b * M + m0) * nsample;
    const int nrows = min(64, M - m0);
    const int total = nrows * nsample;
    for (int f0 = 0; f0 < total; f0 += 64) {  // uniform trip count: a shuffle needs its source lane active
      const int f = min(f0 + lane, total - 1);
      const int row = f / nsample;
      const int slot = f - row * nsample;
      const int rc = __shfl(cnt, row);
      const int rf = __shfl(first, row);
      // slot < rc: a recorded hit; otherwise the pad (first hit, or 0 when the ball is empty)
      const int v = slot < rc ? wrows[f] : rf;
      if (f0 + lane < total) gout[f] = v;
    }
  } else if (valid) {
    for (int s = cnt; s < nsample; ++s) grow[s] = first;
  }
}

// ------------------------------------------------------------------------------------------------
// ball_query v2: a workgroup = 64 centres x 4 waves; wave w scans the w-th quarter of the cloud
// (4x the waves of v1 at the same problem size -- v1 leaves the chip at 2 waves per SIMD at
// config 4) and records its in-radius indices, ascending, in its own LDS list (capped at nsample:
// later entries can never be output).  The row is then the concatenation of the four lists in
// quarter order, cut at nsample and padded with the first hit -- exactly the sequential scan's
// result.  Lists are stored as IT = uint16 when N <= 65536 (32 KiB per workgroup at nsample = 64).
// Per group of 8 scanned points the eight `d < r^2` tests become eight wave masks (v_cmp into
// SGPRs); points nobody hit are skipped with scalar branches.
// ------------------------------------------------------------------------------------------------
template <typename IT>
__global__ __launch_bounds__(256) void ball_query_split_kernel(const float* __restrict__ new_xyz,
                                                               const float* __restrict__ xyz,
                                                               int* __restrict__ idx, int N, int M,
                                                               float radius2, int nsample,
                                                               int tiles_per_b,
                                                               const pp::GridSet* __restrict__ skip) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  if (skip && skip[blockIdx.x / tiles_per_b].pad[0]) return;  // handled by the grid search
  IT* s_list = reinterpret_cast<IT*>(s_raw);                               // [4][64][nsample]
  int* s_cnt = reinterpret_cast<int*>(s_raw + (size_t)4 * 64 * nsample * sizeof(IT));  // [4][64]
  const int b = blockIdx.x / tiles_per_b;
  const int tile = blockIdx.x - b * tiles_per_b;
  const int wave = pp::wave_id_uniform();
  const int lane = threadIdx.x & 63;
  const int m0 = tile * 64;
  const int m = m0 + lane;
  const bool valid = m < M;
  const int mc = valid ? m : M - 1;
  const float* __restrict__ q = new_xyz + ((size_t)b * M + mc) * 3;
  const float* __restrict__ p = xyz + (size_t)b * N * 3;
  const float qx = q[0], qy = q[1], qz = q[2];
  IT* mylist = s_list + ((size_t)wave * 64 + lane) * nsample;

  // quarter [k0, k1), boundaries on multiples of the group size
  const int ngroups = N / kBqGroup;
  const int g0 = (int)(((long long)ngroups * wave) / 4), g1 = (int)(((long long)ngroups * (wave + 1)) / 4);
  int cnt = valid ? 0 : nsample;
  auto load_group = [&](float (&rr)[kBqGroup * 3], int g) {
    const float* __restrict__ rp = p + (size_t)g * (kBqGroup * 3);  // wave-uniform -> s_load
#pragma unroll
    for (int e = 0; e < kBqGroup * 3; ++e) rr[e] = rp[e];
  };
  auto scan_group = [&](const float (&rr)[kBqGroup * 3], int g) {
    const int k = g * kBqGroup;
    unsigned long long hit[kBqGroup];
    unsigned long long any = 0;
#pragma unroll
    for (int e = 0; e < kBqGroup; ++e) {
      const float d = dist3(qx, qy, qz, rr[3 * e], rr[3 * e + 1], rr[3 * e + 2]);
      hit[e] = __ballot(d < radius2);
      any |= hit[e];
    }
    if (any) {
#pragma unroll
      for (int e = 0; e < kBqGroup; ++e) {
        if (hit[e]) {
          if (((hit[e] >> lane) & 1ull) && cnt < nsample) {
            mylist[cnt] = (IT)(k + e);
            ++cnt;
          }
        }
      }
    }
  };
  // two groups per trip, the scalar loads of the next group issued before the current one is
  // scanned (ping-pong SGPR sets): the s_load latency is covered by this wave's own VALU work
  if (g0 < g1) {
    float ra[kBqGroup * 3], rb[kBqGroup * 3];
    load_group(ra, g0);
    int g = g0;
    for (; g + 1 < g1; g += 2) {
      if (__all(cnt >= nsample)) break;
      load_group(rb, g + 1);
      scan_group(ra, g);
      // scalar loads return out of order, so the only wait is lgkmcnt(0): make rb "used" here,
      // before the next loads are issued, or waiting for rb would also wait for them
      asm volatile("" ::"s"(rb[0]), "s"(rb[kBqGroup * 3 - 1]));
      load_group(ra, g + 2 < g1 ? g + 2 : g1 - 1);
      scan_group(rb, g + 1);
      asm volatile("" ::"s"(ra[0]), "s"(ra[kBqGroup * 3 - 1]));
    }
    if (g < g1 && !__all(cnt >= nsample)) scan_group(ra, g);
  }
  if (wave == 3 && !__all(cnt >= nsample)) {  // tail points (N mod 8), highest indices
    for (int k = ngroups * kBqGroup; k < N; ++k) {
      const float d = dist3(qx, qy, qz, p[3 * (size_t)k], p[3 * (size_t)k + 1], p[3 * (size_t)k + 2]);
      if (d < radius2 && cnt < nsample) {
        mylist[cnt] = (IT)k;
        ++cnt;
      }
    }
  }
  s_cnt[wave * 64 + lane] = valid ? cnt : 0;
  __syncthreads();

  // 64 rows x nsample ints, contiguous in the output
  int* __restrict__ gout = idx + ((size_t)b * M + m0) * nsample;
  const int nrows = min(64, M - m0);
  const int total = nrows * nsample;
  for (int f = threadIdx.x; f < total; f += 256) {
    const int row = f / nsample;
    const int slot = f - row * nsample;
    const int c0 = s_cnt[row], c1 = s_cnt[64 + row], c2 = s_cnt[128 + row], c3 = s_cnt[192 + row];
    const IT* l0 = s_list + (size_t)row * nsample;
    const IT* l1 = l0 + (size_t)64 * nsample;
    const IT* l2 = l1 + (size_t)64 * nsample;
    const IT* l3 = l2 + (size_t)64 * nsample;
    // first hit of the row = head of the first non-empty list (0 if the ball is empty)
    int first = 0;
    if (c0 > 0) first = (int)l0[0];
    else if (c1 > 0) first = (int)l1[0];
    else if (c2 > 0) first = (int)l2[0];
    else if (c3 > 0) first = (int)l3[0];
    int v = first;
    int sidx = slot;
    if (sidx < c0) v = (int)l0[sidx];
    else if ((sidx -= c0) < c1) v = (int)l1[sidx];
    else if ((sidx -= c1) < c2) v = (int)l2[sidx];
    else if ((sidx -= c2) < c3) v = (int)l3[sidx];
    gout[f] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// group_points: out[b,c,j,k] = points[b,c,idx[b,j,k]]        (ref sampling_cuda.cu:447-467)
// VEC: a thread owns L consecutive (j,k) positions: 16-byte idx loads, then per channel L gathers and one 16-byte
// store (P % L == 0, obs % L == 0, idx and out 16-byte aligned; the rows need no alignment: they are read one
// element at a time); otherwise one position per thread.  The reference launches B blocks; this fills the chip.
// ------------------------------------------------------------------------------------------------
template <typename E, bool VEC>
__global__ __launch_bounds__(256) void group_points_kernel(const E* __restrict__ points,
                                                           const int* __restrict__ idx,
                                                           E* __restrict__ out, int C, int N,
                                                           long long P, int c_per_block, long long obs) {
  constexpr int L = 16 / sizeof(E);
  const int b = blockIdx.z;
  const int c0 = blockIdx.y * c_per_block;
  const int c1 = min(C, c0 + c_per_block);
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const long long p = t * L;
    if (p >= P) return;
    int ii[L];
    load_indices(ii, idx + (size_t)b * P + p);
    for (int c = c0; c < c1; ++c) {
      const auto r = gather16(points + ((size_t)b * C + c) * N, ii);
      store16(out + (size_t)b * obs + (size_t)c * P + p, r);
    }
  } else {
    if (t >= P) return;
    const int i = idx[(size_t)b * P + t];
    for (int c = c0; c < c1; ++c)
      out[(size_t)b * obs + (size_t)c * P + t] = points[((size_t)b * C + c) * N + i];
  }
}

// v2: the channel row points[b,c,:] (N floats) is staged in LDS once per workgroup and the gathers
// become ds_read_b32 (random LDS addresses: ~3-4-way bank conflicts, still several times the rate
// of 64-distinct-line global gathers).  A 512-thread workgroup owns 512*4*V consecutive (j,k)
// positions of one batch element, keeps their indices in registers for all C channels (idx is
// read from HBM exactly once) and streams 16-byte stores.  Two workgroups per CU (<= 64 KiB of LDS
// each) overlap one's row load + barrier with the other's gather + store phase.  Workgroups of
// one batch element share blockIdx % 8 (one XCD's L2 serves the row re-reads).
// A 16-byte global load the compiler does not track: hipcc's waitcnt pass treats a vmcnt queue that
// holds both loads and stores as unordered and drains it (vmcnt(0)) at the first use of a load
// result -- which here would wait for the previous channel's 8 HBM stores every iteration.  The
// hardware retires vector-memory operations in issue order, so the loads (issued before the
// stores) are complete once at most `V` younger operations are outstanding: vm_wait<V>().
__device__ __forceinline__ void load16_untracked(pp::f4& dst, const pp::f4* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
template <int N, int KR>
__device__ __forceinline__ void vm_wait(pp::f4 (&r)[KR]) {
  // names every destination so that no use of them can be scheduled above the wait
  if constexpr (KR == 1)
    asm volatile("s_waitcnt vmcnt(%c1)" : "+v"(r[0]) : "i"(N));
  else if constexpr (KR == 2)
    asm volatile("s_waitcnt vmcnt(%c2)" : "+v"(r[0]), "+v"(r[1]) : "i"(N));
  else if constexpr (KR == 4)
    asm volatile("s_waitcnt vmcnt(%c4)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : "i"(N));
  else
    asm volatile("s_waitcnt vmcnt(%c8)"
                 : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7])
                 : "i"(N));
}

template <int V, int KR, bool FULL>
__device__ __forceinline__ void group_points_lds_loop(const pp::f4* __restrict__ row, float* __restrict__ out_b,
                                                      float* s_row, const pp::i4 (&ii)[V], int C, int n4,
                                                      long long P, long long p0, int t) {
  // The row loads are unconditional (indices clamped to the row: surplus lanes re-load and
  // re-write the last float4 with the same value).  Row c+1 is fetched into registers BEFORE the
  // stores of row c are issued; in the FULL instantiation exactly V stores follow the loads, so
  // vmcnt(V) retires the loads and leaves the stores in flight across the barriers.
  static_assert(KR == 1 || KR == 2 || KR == 4 || KR == 8, "");
  int ee[KR];
  pp::f4 pre[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    ee[k] = min(t + 512 * k, n4 - 1);
    load16_untracked(pre[k], row + ee[k]);
  }
  vm_wait<0, KR>(pre);
  for (int c = 0; c < C; ++c) {
    __syncthreads();  // everyone is done gathering from the previous row
    // FULL: exactly V stores were issued after the loads of this row; otherwise the count varies
    // per wave and the queue is drained.  (c == 0: retired before the loop.)
    if (c > 0) vm_wait<FULL ? V : 0, KR>(pre);
#pragma unroll
    for (int k = 0; k < KR; ++k) reinterpret_cast<pp::f4*>(s_row)[ee[k]] = pre[k];
    __syncthreads();
    // last iteration: harmless re-load of the same row (keeps the loop body branch-free)
    const pp::f4* __restrict__ nrow = row + (size_t)(c + 1 < C ? c + 1 : c) * n4;
#pragma unroll
    for (int k = 0; k < KR; ++k) load16_untracked(pre[k], nrow + ee[k]);
    float* __restrict__ o = out_b + (size_t)c * P;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const long long p = p0 + (long long)v * 2048;
      pp::f4 r;
      r.x = s_row[ii[v].x];
      r.y = s_row[ii[v].y];
      r.z = s_row[ii[v].z];
      r.w = s_row[ii[v].w];
      if (FULL || p < P) *reinterpret_cast<pp::f4*>(o + p) = r;
    }
  }
  vm_wait<0, KR>(pre);  // the surplus prefetch of the last iteration
}

template <int V, int KR>
__global__ __launch_bounds__(512, 4) void group_points_lds_kernel(const float* __restrict__ points,
                                                                  const int* __restrict__ idx,
                                                                  float* __restrict__ out, int B, int C,
                                                                  int N, long long P, int chunks, long long obs) {
  extern __shared__ __attribute__((aligned(16))) float s_row[];
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / chunks);
  const int chunk = y % chunks;
  if (b >= B) return;
  const int t = threadIdx.x;
  const long long p0 = (long long)chunk * (512 * 4 * V) + t * 4;
  const bool full = (long long)(chunk + 1) * (512 * 4 * V) <= P;  // every position of the chunk exists
  pp::i4 ii[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const long long p = p0 + (long long)v * 2048;
    ii[v] = p < P ? *reinterpret_cast<const pp::i4*>(idx + (size_t)b * P + p) : pp::i4{0, 0, 0, 0};
  }
  const pp::f4* __restrict__ row = reinterpret_cast<const pp::f4*>(points + (size_t)b * C * N);
  float* __restrict__ out_b = out + (size_t)b * obs;
  if (full)
    group_points_lds_loop<V, KR, true>(row, out_b, s_row, ii, C, N >> 2, P, p0, t);
  else
    group_points_lds_loop<V, KR, false>(row, out_b, s_row, ii, C, N >> 2, P, p0, t);
}

// ------------------------------------------------------------------------------------------------
// v5: the channel rows arrive by LDS-DMA (global_load_lds_dwordx4: no VGPR round trip, no ds_write) into ONE row
// buffer per 512-thread workgroup, two workgroups per CU: nothing overlaps inside a workgroup (DMA row c, wait,
// barrier, gather + store, barrier); the two workgroups of a CU overlap each other and are not in step (0.89 against
// 0.92 ms at config 4 for the 1024-thread ring of two buffers it replaced -- tools/archive/group_points_dma_ring_r2_r3
// -- ; the stores alone, without any barrier, would take 0.75 ms).  One wave instruction moves 1 KiB of the row.
// Full chunks of 512 * L * V positions only: V index quads (fp32) or octets (16-bit) per thread.
// ------------------------------------------------------------------------------------------------
constexpr int kDma1Threads = 512;
template <typename E, int V>
__global__ __launch_bounds__(kDma1Threads) void group_points_dma1_kernel(const E* __restrict__ points,
                                                                         const int* __restrict__ idx,
                                                                         E* __restrict__ out, int B, int C,
                                                                         int N, long long P, int chunks, int passes,
                                                                         int cgroups, int c_per_group, long long obs) {
  constexpr int L = 16 / sizeof(E);
  extern __shared__ __attribute__((aligned(16))) unsigned char s_row1[];
  const E* s_row = reinterpret_cast<const E*>(s_row1);
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int per_b = chunks * cgroups;
  const int b = x + 8 * (y / per_b);
  const int rem = y % per_b;
  const int chunk = rem / cgroups;
  const int c_begin = (rem % cgroups) * c_per_group;
  const int c_end = min(C, c_begin + c_per_group);
  if (b >= B || c_begin >= c_end) return;
  const int t = threadIdx.x;
  const int wave = pp::wave_id_uniform();
  const long long p0 = (long long)chunk * (kDma1Threads * L * V) + t * L;
  int ii[V][L];
#pragma unroll
  for (int v = 0; v < V; ++v) load_indices(ii[v], idx + (size_t)b * P + p0 + (long long)v * (kDma1Threads * L));
  const int n16 = N >> (L == 4 ? 2 : 3);  // 16-byte units of a row
  const u4v* __restrict__ row0 = reinterpret_cast<const u4v*>(points + (size_t)b * C * N);
  E* __restrict__ out_b = out + (size_t)b * obs;
  for (int c = c_begin; c < c_end; ++c) {
    const u4v* __restrict__ row = row0 + (size_t)c * n16;
    for (int k = 0; k < passes; ++k) {
      const int e = k * kDma1Threads + t;
      const int src = e < n16 ? e : n16 - 1;  // surplus lanes re-load the last unit into the buffer's slack
      unsigned char* dst = s_row1 + (size_t)(k * kDma1Threads + wave * 64) * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(row + src),
                                       (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    E* __restrict__ o = out_b + (size_t)c * P;
#pragma unroll
    for (int v = 0; v < V; ++v)
      store16_nt(o + p0 + (long long)v * (kDma1Threads * L), gather16(s_row, ii[v]));
    __builtin_amdgcn_s_barrier();  // every wave has read the row: the next one may land
    asm volatile("" ::: "memory");
  }
}

template <typename E, int V>
bool launch_group_dma1(const E* points, const int* idx, E* out, int B, int C, int N, long long P,
                       long long obs, hipStream_t s) {
  constexpr int L = 16 / sizeof(E);
  const long long per_block = (long long)kDma1Threads * L * V;
  if (P % per_block != 0) return false;
  const long long chunks = P / per_block;
  const long long base = 8LL * ((B + 7) / 8) * chunks;
  int cgroups = 1;
  while (base * cgroups < 512 && cgroups * 2 <= C) cgroups *= 2;
  const int c_per_group = (C + cgroups - 1) / cgroups;
  const long long blocks = base * cgroups;
  const int n16 = N / L;
  const int passes = (n16 + kDma1Threads - 1) / kDma1Threads;
  const size_t lds = (size_t)passes * kDma1Threads * 16;
  if (lds > 72 * 1024 || chunks > 0x7fffffLL || blocks > 0x7fffffffLL) return false;
  static pp::DeviceFlags lds_ok;
  if (pp::allow_big_lds(group_points_dma1_kernel<E, V>, 80 * 1024, lds_ok) != hipSuccess) return false;  // (another kernel)
  group_points_dma1_kernel<E, V><<<dim3((unsigned)blocks), dim3(kDma1Threads), lds, s>>>(
      points, idx, out, B, C, N, P, (int)chunks, passes, cgroups, c_per_group, obs);
  return true;
}

template <int V>
bool launch_group_lds(const float* points, const int* idx, float* out, int B, int C, int N,
                      long long P, long long obs, hipStream_t s) {
  const long long per_block = 512LL * 4 * V;
  const long long chunks = (P + per_block - 1) / per_block;
  const long long blocks = 8LL * ((B + 7) / 8) * chunks;
  if (chunks > 0x7fffffLL || blocks > 0x7fffffffLL) return false;
  // KR = float4 per thread per staging pass: 512 * KR * 16 B >= row bytes
  const dim3 grid((unsigned)blocks), block(512);
  const size_t lds = (size_t)N * sizeof(float);
  const int n4 = N / 4;
  if (n4 <= 512 * 1)
    group_points_lds_kernel<V, 1><<<grid, block, lds, s>>>(points, idx, out, B, C, N, P, (int)chunks, obs);
  else if (n4 <= 512 * 2)
    group_points_lds_kernel<V, 2><<<grid, block, lds, s>>>(points, idx, out, B, C, N, P, (int)chunks, obs);
  else if (n4 <= 512 * 4)
    group_points_lds_kernel<V, 4><<<grid, block, lds, s>>>(points, idx, out, B, C, N, P, (int)chunks, obs);
  else
    group_points_lds_kernel<V, 8><<<grid, block, lds, s>>>(points, idx, out, B, C, N, P, (int)chunks, obs);
  return true;
}

// The 16-bit VGPR-staged form: a 512-thread workgroup owns 512 * 8 * V consecutive positions of one batch element,
// keeps their indices in registers for all C channels and streams 16-byte stores; the last chunk may be ragged
// (P % 8 == 0: an octet exists whole or not at all).  Unlike group_points_lds_kernel it loads each row between the
// barriers with tracked loads: no prefetch of the next row, no vm_wait, no FULL split.
// Requires the vector conditions, N % 8 == 0 and 16-byte aligned points; 2 N bytes of LDS.
template <int V>
__global__ __launch_bounds__(512) void group_points_lds_b16_kernel(const u16* __restrict__ points,
                                                                   const int* __restrict__ idx,
                                                                   u16* __restrict__ out, int B, int C, int N,
                                                                   long long P, int chunks, long long obs) {
  extern __shared__ __attribute__((aligned(16))) u16 s_r16[];
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / chunks);
  const int chunk = y % chunks;
  if (b >= B) return;
  const int t = threadIdx.x;
  const long long p0 = (long long)chunk * (512 * 8 * V) + t * 8;
  pp::i4 ia[V], ic[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const long long p = p0 + (long long)v * 4096;
    ia[v] = p < P ? *reinterpret_cast<const pp::i4*>(idx + (size_t)b * P + p) : pp::i4{0, 0, 0, 0};
    ic[v] = p < P ? *reinterpret_cast<const pp::i4*>(idx + (size_t)b * P + p + 4) : pp::i4{0, 0, 0, 0};
  }
  const int n8 = N >> 3;
  const u4v* __restrict__ rows = reinterpret_cast<const u4v*>(points + (size_t)b * C * N);
  u16* __restrict__ out_b = out + (size_t)b * obs;
  for (int c = 0; c < C; ++c) {
    __syncthreads();  // everyone is done gathering from the previous row
    for (int e = t; e < n8; e += 512) reinterpret_cast<u4v*>(s_r16)[e] = rows[(size_t)c * n8 + e];
    __syncthreads();
    u16* __restrict__ o = out_b + (size_t)c * P;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const long long p = p0 + (long long)v * 4096;
      const u4v r = gather8(s_r16, ia[v], ic[v]);
      if (p < P) *reinterpret_cast<u4v*>(o + p) = r;
    }
  }
}

bool launch_group_lds_b16(const u16* points, const int* idx, u16* out, int B, int C, int N, long long P,
                          long long obs, hipStream_t s) {
  constexpr int V = 4;  // the one instantiation
  const long long chunks = (P + 512LL * 8 * V - 1) / (512LL * 8 * V);
  const long long blocks = 8LL * ((B + 7) / 8) * chunks;
  if (chunks > 0x7fffffLL || blocks > 0x7fffffffLL) return false;
  group_points_lds_b16_kernel<V><<<dim3((unsigned)blocks), dim3(512), (size_t)N * 2, s>>>(points, idx, out, B, C, N, P,
                                                                                        (int)chunks, obs);
  return true;
}

// LDS-staged form without any alignment requirement (P, N, the batch stride or the pointers not
// multiples of 4 elements) and for rows up to 152 KiB: 4-byte loads and stores, all coalesced; a thread
// keeps V positions (stride 1024) for all channels.  Slower than the 16-byte forms above, but the
// alternative for such shapes is the global-gather kernel at ~0.5 TB/s.
template <int V>
__global__ __launch_bounds__(1024) void group_points_lds_scalar_kernel(const float* __restrict__ points,
                                                                       const int* __restrict__ idx,
                                                                       float* __restrict__ out, int B, int C,
                                                                       int N, long long P, int chunks,
                                                                       long long obs) {
  extern __shared__ __attribute__((aligned(16))) float s_srow[];
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / chunks);
  const int chunk = y % chunks;
  if (b >= B) return;
  const int t = threadIdx.x;
  const long long p0 = (long long)chunk * (1024 * V) + t;
  int ii[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const long long p = p0 + 1024LL * v;
    ii[v] = p < P ? idx[(size_t)b * P + p] : 0;
  }
  const float* __restrict__ rows = points + (size_t)b * C * N;
  float* __restrict__ out_b = out + (size_t)b * obs;
  for (int c = 0; c < C; ++c) {
    __syncthreads();  // the previous row has been gathered
    const float* __restrict__ row = rows + (size_t)c * N;
    for (int e = t; e < N; e += 1024) s_srow[e] = row[e];
    __syncthreads();
    float* __restrict__ o = out_b + (size_t)c * P;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const long long p = p0 + 1024LL * v;
      if (p < P) o[p] = s_srow[ii[v]];
    }
  }
}

// group_points backward: grad_points[b,c,idx[b,j,k]] += grad_out[b,c,j,k]  (ref :482-503)
__global__ __launch_bounds__(256) void group_points_grad_kernel(const float* __restrict__ grad_out,
                                                                const int* __restrict__ idx,
                                                                float* __restrict__ grad_points,
                                                                int C, int N, long long P,
                                                                int c_per_block, long long gbs) {
  const int b = blockIdx.z;
  const int c0 = blockIdx.y * c_per_block;
  const int c1 = min(C, c0 + c_per_block);
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= P) return;
  const int i = idx[(size_t)b * P + t];
  for (int c = c0; c < c1; ++c)
    atomicAdd(grad_points + ((size_t)b * C + c) * N + i, grad_out[(size_t)b * gbs + (size_t)c * P + t]);
}

// The same with a DOUBLE column: on gfx950 ds_add_f64 runs at 3.3 lanes/clk/CU against 0.36 for
// ds_add_f32 (tools/lds_atomic_probe.hip), so widening the accumulator is 9x faster -- and the sum
// is rounded to fp32 once, at the end, instead of at every addend.  A workgroup owns W <= 19456
// destinations (8 W bytes of LDS) of one (batch, channel): the whole column when N fits, otherwise
// one of `nsplit` ranges, each workgroup streaming the column's grad_out and skipping the entries
// of the other ranges.  U 16-byte load pairs are in flight per thread before the first atomic.
// T = f16 / bf16 (DESIGN.md §4 "16-bit features"): the quad structure stays -- an 8-byte grad_out load beside the
// 16-byte index load, widened in registers -- and the column is written as T(float(sum)); always `overwrite`.
typedef unsigned u2v __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ pp::f4 widen_quad(const u2v w) {
  T a[4];
  __builtin_memcpy(a, &w, 8);
  return pp::f4{pp::widen(a[0]), pp::widen(a[1]), pp::widen(a[2]), pp::widen(a[3])};
}
template <typename T, bool NT>
__device__ __forceinline__ pp::f4 load_quad(const T* __restrict__ base, long long q) {
  if constexpr (std::is_same<T, float>::value) {
    const pp::f4* p = reinterpret_cast<const pp::f4*>(base) + q;
    return NT ? __builtin_nontemporal_load(p) : *p;
  } else {
    const u2v* p = reinterpret_cast<const u2v*>(base) + q;
    return widen_quad<T>(NT ? __builtin_nontemporal_load(p) : *p);
  }
}
template <int U, bool VEC = true, typename T = float>
__global__ __launch_bounds__(1024) void group_points_grad_lds64_kernel(const T* __restrict__ grad_out,
                                                                       const int* __restrict__ idx,
                                                                       T* __restrict__ grad_points,
                                                                       int B, int C, int N, long long P,
                                                                       long long gbs, int nsplit, int W, int overwrite) {
  extern __shared__ __attribute__((aligned(16))) double s_col64[];
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int per_b = C * nsplit;
  const int b = x + 8 * (y / per_b);
  const int r = y % per_b;
  const int c = r / nsplit;
  const int lo = (r - c * nsplit) * W;     // this workgroup's destinations: [lo, lo + w)
  const int w = min(W, N - lo);
  if (b >= B) return;
  const int t = threadIdx.x;
  for (int k = t; k < w; k += 1024) s_col64[k] = 0.0;
  __syncthreads();
  const T* __restrict__ go = grad_out + (size_t)b * gbs + (size_t)c * P;
  const int* __restrict__ ib = idx + (size_t)b * P;
  const long long p4 = P >> 2;
  auto add1 = [&](int i, double v) {
    if ((unsigned)(i - lo) < (unsigned)w) atomicAdd(&s_col64[i - lo], v);
  };
  // Runs of equal consecutive indices (the pad of a ball_query row repeats its first index) are
  // summed in registers and added once, by the run's first element: same-address LDS atomics
  // serialise, and at config 4 a third of all entries are pads.
  auto add4 = [&](const pp::f4& g, const pp::i4& i) {
    const bool e1 = i.y == i.x, e2 = i.z == i.y, e3 = i.w == i.z;
    const double sw = (double)g.w;
    const double sz = (double)g.z + (e3 ? sw : 0.0);
    const double sy = (double)g.y + (e2 ? sz : 0.0);
    const double sx = (double)g.x + (e1 ? sy : 0.0);
    add1(i.x, sx);
    if (!e1) add1(i.y, sy);
    if (!e2) add1(i.z, sz);
    if (!e3) add1(i.w, sw);
  };
  // The same for a wave whose 64 lanes hold 64 CONSECUTIVE quads (the main loop below), with runs merged ACROSS lanes
  // as well (round 5): the pad of a ball_query row is the row's first index repeated to the row's end --
  // at config 4 a third of a row, six quads in six neighbouring lanes that all add to ONE address in the same wave
  // instruction (same-address LDS atomics serialise).  A quad that is a single run and continues the run its left
  // neighbour ends with hands its sum to the left instead of adding it: a segmented suffix sum over the lanes of a row of
  // sixteen (DPP row shifts; 64 entries = a row of nsample = 64), in doubles, so that what is added is what the lanes would
  // have added one by one up to the order of a sum of doubles.
  auto add4_merged = [&](const pp::f4& g, const pp::i4& i) {
    const bool e1 = i.y == i.x, e2 = i.z == i.y, e3 = i.w == i.z;
    const double sw = (double)g.w;
    const double sz = (double)g.z + (e3 ? sw : 0.0);
    const double sy = (double)g.y + (e2 ? sz : 0.0);
    const double sx = (double)g.x + (e1 ? sy : 0.0);
    const bool full = e1 & e2 & e3;
    auto shl = [](int v, auto k_c) {  // lane l <- lane l + k of its row of sixteen; 0 beyond the row
      constexpr int K = decltype(k_c)::value;
      return __builtin_amdgcn_update_dpp(0, v, 0x100 + K, 0xf, 0xf, false);
    };
    auto shl_d = [&](double v, auto k_c) {
      const long long b = __builtin_bit_cast(long long, v);
      const unsigned lo = (unsigned)shl((int)(unsigned)b, k_c), hi = (unsigned)shl((int)(unsigned)(b >> 32), k_c);
      return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
    };
    using K1 = std::integral_constant<int, 1>; using K2 = std::integral_constant<int, 2>;
    using K4 = std::integral_constant<int, 4>; using K8 = std::integral_constant<int, 8>;
    // cont: this quad is one run and continues the run the left neighbour (same row of sixteen) ends with
    const int left_w = __builtin_amdgcn_update_dpp(0, i.w, 0x111, 0xf, 0xf, false);  // row_shr:1
    const bool cont = full && (threadIdx.x & 15) != 0 && i.x == left_w;
    // A = the sums of the quads to the right for as long as they continue this lane's last run
    // (every shift is evaluated by ALL lanes, then selected: inside `f ? shift : 0` it would run under f's mask and read
    //  the lanes that mask switches off -- the chain's last quad -- as zero)
    int f = shl(cont ? 1 : 0, K1{});                    // the right neighbour continues
    const double sx_right = shl_d(sx, K1{});
    double A = f ? sx_right : 0.0;
    {
      const double a2 = shl_d(A, K1{});
      const int f2 = shl(f, K1{});
      A += f ? a2 : 0.0;
      f &= f2;                                          // lanes l+1, l+2 both continue
    }
    {
      const double a4 = shl_d(A, K2{});
      const int f4 = shl(f, K2{});
      A += f ? a4 : 0.0;
      f &= f4;                                          // lanes l+1 .. l+4
    }
    {
      const double a8 = shl_d(A, K4{});
      const int f8 = shl(f, K4{});
      A += f ? a8 : 0.0;
      f &= f8;                                          // lanes l+1 .. l+8
    }
    {
      const double a16 = shl_d(A, K8{});
      A += f ? a16 : 0.0;
    }
    // the lane's LAST run takes A along; a continuing quad adds nothing
    if (!cont) add1(i.x, sx + (full ? A : 0.0));
    if (!e1) add1(i.y, sy + ((e2 & e3) ? A : 0.0));
    if (!e2) add1(i.z, sz + (e3 ? A : 0.0));
    if (!e3) add1(i.w, sw + A);
  };
  if constexpr (VEC) {
    long long e = t;
    // (the bound is the wave's LAST lane's: a wave enters the loop whole or not at all -- add4_merged's row shifts read
    //  the neighbouring lanes -- and the quads of a wave that straddles the end go to the lane-by-lane loop below)
    for (; (e | 63) + 1024 * (U - 1) < p4; e += 1024 * U) {
      pp::f4 g[U];
      pp::i4 i[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // (grad_out is read once: non-temporal, so that the 4 GiB stream does not push the indices -- re-read by
        //  every channel's workgroup -- out of the XCD's L2)
        g[u] = load_quad<T, true>(go, e + 1024 * u);
        i[u] = reinterpret_cast<const pp::i4*>(ib)[e + 1024 * u];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) add4_merged(g[u], i[u]);  // (every lane is active here: the DPP shifts see whole rows)
    }
    for (; e < p4; e += 1024) add4(load_quad<T, false>(go, e), reinterpret_cast<const pp::i4*>(ib)[e]);
    for (long long q = (p4 << 2) + t; q < P; q += 1024) add1(ib[q], (double)pp::widen(go[q]));
  } else {
    // rows that are not 16-byte aligned (P or the batch stride not a multiple of 4): 4-byte loads, still
    // coalesced, 2U in flight per thread -- slower than the vector form, far from the global-atomic one
    long long e = t;
    for (; e + 1024 * (2 * U - 1) < P; e += 1024 * 2 * U) {
      float g[2 * U];
      int i[2 * U];
#pragma unroll
      for (int u = 0; u < 2 * U; ++u) {
        g[u] = pp::widen(go[e + 1024 * u]);
        i[u] = ib[e + 1024 * u];
      }
#pragma unroll
      for (int u = 0; u < 2 * U; ++u) add1(i[u], (double)g[u]);
    }
    for (; e < P; e += 1024) add1(ib[e], (double)pp::widen(go[e]));
  }
  __syncthreads();
  T* __restrict__ gp = grad_points + ((size_t)b * C + c) * N + lo;
  if constexpr (!std::is_same<T, float>::value) {  // double -> float -> T: R_T of the fp32 operator's result
    for (int k = t; k < w; k += 1024) gp[k] = pp::narrow<T>((float)s_col64[k]);
  } else if (overwrite) {  // (uniform) pp_group_points_grad_out_*: every element is written once, nothing is read
    for (int k = t; k < w; k += 1024) gp[k] = (float)s_col64[k];
  } else {
    for (int k = t; k < w; k += 1024) gp[k] += (float)s_col64[k];  // accumulate: the reference ABI's contract
  }
}

// ------------------------------------------------------------------------------------------------
// three_nn (ref interpolate_gpu.cu:9-52): the three smallest dist3 and their indices, ascending,
// strict < at every rank (earlier index wins ties).  The reference keeps the bests as double
// initialised to 1e40 and stores them as float: identical to float bests initialised to +inf.
// One lane per query, known point wave-uniform.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ unknown,
                                                       const float* __restrict__ known,
                                                       float* __restrict__ dist2,
                                                       int* __restrict__ idx, int N, int M,
                                                       int tiles_per_b, const pp::GridSet* __restrict__ skip) {
  const int b = blockIdx.x / tiles_per_b;
  if (skip && skip[b].pad[0]) return;  // this batch element was handled by the grid search
  const int tile = blockIdx.x - b * tiles_per_b;
  const int n = tile * 256 + threadIdx.x;
  const bool valid = n < N;
  const int nc = valid ? n : N - 1;
  const float* __restrict__ u = unknown + ((size_t)b * N + nc) * 3;
  const float* __restrict__ kn = known + (size_t)b * M * 3;
  const float ux = u[0], uy = u[1], uz = u[2];
  float b1 = __builtin_inff(), b2 = __builtin_inff(), b3 = __builtin_inff();
  int i1 = 0, i2 = 0, i3 = 0;
  for (int k = 0; k < M; ++k) {
    const float d = dist3(ux, uy, uz, kn[3 * (size_t)k], kn[3 * (size_t)k + 1], kn[3 * (size_t)k + 2]);
    if (__any(d < b3)) {
      const bool l1 = d < b1, l2 = d < b2, l3 = d < b3;
      b3 = l2 ? b2 : (l3 ? d : b3);
      i3 = l2 ? i2 : (l3 ? k : i3);
      b2 = l1 ? b1 : (l2 ? d : b2);
      i2 = l1 ? i1 : (l2 ? k : i2);
      b1 = l1 ? d : b1;
      i1 = l1 ? k : i1;
    }
  }
  if (valid) {
    float* od = dist2 + ((size_t)b * N + n) * 3;
    int* oi = idx + ((size_t)b * N + n) * 3;
    od[0] = b1; od[1] = b2; od[2] = b3;
    oi[0] = i1; oi[1] = i2; oi[2] = i3;
  }
}

// three_interpolate (ref interpolate_gpu.cu:77-97): out[b,c,n] = w0*p[i0] + w1*p[i1] + w2*p[i2],
// canonical rounding fma(w2,p2, fma(w0,p0, w1*p1)).  A thread keeps (idx, weight) of one n and
// walks a slab of channels.
template <typename T>  // 16-bit T: widened operands, the same fp32 chain, one rounding
__global__ __launch_bounds__(256) void three_interpolate_kernel(const T* __restrict__ points,
                                                                const int* __restrict__ idx,
                                                                const float* __restrict__ weight,
                                                                T* __restrict__ out, int C,
                                                                int M, int N, int c_per_block) {
  const int b = blockIdx.z;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int* id = idx + ((size_t)b * N + n) * 3;
  const float* w = weight + ((size_t)b * N + n) * 3;
  const int i0 = id[0], i1 = id[1], i2 = id[2];
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const int c0 = blockIdx.y * c_per_block;
  const int c1 = min(C, c0 + c_per_block);
  for (int c = c0; c < c1; ++c) {
    const T* __restrict__ p = points + ((size_t)b * C + c) * M;
    out[((size_t)b * C + c) * N + n] = pp::narrow<T>(
        __builtin_fmaf(w2, pp::widen(p[i2]), __builtin_fmaf(w0, pp::widen(p[i0]), w1 * pp::widen(p[i1]))));
  }
}

// three_interpolate, LDS-staged form: like group_points v2 -- the channel row points[b,c,:]
// (M floats) is staged in LDS once per 512-thread workgroup (next row prefetched through
// registers), a thread keeps (idx, weight) of four consecutive n for all C channels and streams
// 16-byte stores.  Same canonical fma order as the gather form.
template <int KR>
__global__ __launch_bounds__(512, 4) void three_interpolate_lds_kernel(const float* __restrict__ points,
                                                                       const int* __restrict__ idx,
                                                                       const float* __restrict__ weight,
                                                                       float* __restrict__ out, int B, int C,
                                                                       int M, int N, int chunks) {
  extern __shared__ __attribute__((aligned(16))) float s_row[];
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / chunks);
  const int chunk = y % chunks;
  if (b >= B) return;
  const int t = threadIdx.x;
  const int n0 = chunk * 2048 + t * 4;  // four consecutive outputs per thread (N % 4 == 0)
  const bool active = n0 < N;
  const int nc = active ? n0 : 0;
  int ii[12];
  float ww[12];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const pp::i4 q = reinterpret_cast<const pp::i4*>(idx + ((size_t)b * N + nc) * 3)[e];
    const pp::f4 w = reinterpret_cast<const pp::f4*>(weight + ((size_t)b * N + nc) * 3)[e];
    ii[4 * e] = q.x; ii[4 * e + 1] = q.y; ii[4 * e + 2] = q.z; ii[4 * e + 3] = q.w;
    ww[4 * e] = w.x; ww[4 * e + 1] = w.y; ww[4 * e + 2] = w.z; ww[4 * e + 3] = w.w;
  }
  const int m4 = M >> 2;
  const pp::f4* __restrict__ row = reinterpret_cast<const pp::f4*>(points + (size_t)b * C * M);
  int ee[KR];
  pp::f4 pre[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    ee[k] = min(t + 512 * k, m4 - 1);
    pre[k] = row[ee[k]];
  }
  for (int c = 0; c < C; ++c) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KR; ++k) reinterpret_cast<pp::f4*>(s_row)[ee[k]] = pre[k];
    __syncthreads();
    const pp::f4* __restrict__ nrow = row + (size_t)(c + 1 < C ? c + 1 : c) * m4;
#pragma unroll
    for (int k = 0; k < KR; ++k) pre[k] = nrow[ee[k]];
    pp::f4 r;
    r.x = __builtin_fmaf(ww[2], s_row[ii[2]], __builtin_fmaf(ww[0], s_row[ii[0]], ww[1] * s_row[ii[1]]));
    r.y = __builtin_fmaf(ww[5], s_row[ii[5]], __builtin_fmaf(ww[3], s_row[ii[3]], ww[4] * s_row[ii[4]]));
    r.z = __builtin_fmaf(ww[8], s_row[ii[8]], __builtin_fmaf(ww[6], s_row[ii[6]], ww[7] * s_row[ii[7]]));
    r.w = __builtin_fmaf(ww[11], s_row[ii[11]], __builtin_fmaf(ww[9], s_row[ii[9]], ww[10] * s_row[ii[10]]));
    if (active) *reinterpret_cast<pp::f4*>(out + ((size_t)b * C + c) * N + n0) = r;
  }
}

template <int KR>
void launch_three_interpolate_lds(const float* points, const int* idx, const float* weight, float* out,
                                  int B, int C, int M, int N, hipStream_t s) {
  const int chunks = (N + 2047) / 2048;
  three_interpolate_lds_kernel<KR><<<dim3((unsigned)(8 * ((B + 7) / 8) * chunks)), dim3(512),
                                     (size_t)M * sizeof(float), s>>>(points, idx, weight, out, B, C, M, N, chunks);
}

// three_interpolate, channel-group form: a workgroup stages CG whole rows points[b, c0..c0+CG, :]
// in LDS once (one barrier) and then walks ALL n, four per thread and step: (idx, weight) of the
// four points are read once for the CG channels, 12 LDS gathers per channel, one 16-byte store per
// channel.  The row-at-a-time form above pays two barriers per channel row for 12 gathers; here
// the only serial part is the staging.  Same canonical fma order.
template <int CG, bool VEC>
__global__ __launch_bounds__(1024) void three_interpolate_rows_kernel(const float* __restrict__ points,
                                                                      const int* __restrict__ idx,
                                                                      const float* __restrict__ weight,
                                                                      float* __restrict__ out, int B, int C,
                                                                      int M, int N) {
  extern __shared__ __attribute__((aligned(16))) float s_irows[];  // [CG][M]
  const int groups = (C + CG - 1) / CG;
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / groups);
  if (b >= B) return;
  const int c0 = (y % groups) * CG;
  const int nc = min(CG, C - c0);
  const int t = threadIdx.x;
  for (int k = 0; k < nc; ++k) {
    const float* __restrict__ rowf = points + ((size_t)b * C + c0 + k) * M;
    if constexpr (VEC) {
      const pp::f4* __restrict__ row = reinterpret_cast<const pp::f4*>(rowf);
      for (int e = t; e < (M >> 2); e += 1024) reinterpret_cast<pp::f4*>(s_irows + (size_t)k * M)[e] = row[e];
    } else {
      for (int e = t; e < M; e += 1024) s_irows[(size_t)k * M + e] = rowf[e];
    }
  }
  __syncthreads();
  if constexpr (VEC) {
    for (int n0 = 4 * t; n0 < N; n0 += 4096) {
      int ii[12];
      float ww[12];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const pp::i4 q = reinterpret_cast<const pp::i4*>(idx + ((size_t)b * N + n0) * 3)[e];
        const pp::f4 w = reinterpret_cast<const pp::f4*>(weight + ((size_t)b * N + n0) * 3)[e];
        ii[4 * e] = q.x; ii[4 * e + 1] = q.y; ii[4 * e + 2] = q.z; ii[4 * e + 3] = q.w;
        ww[4 * e] = w.x; ww[4 * e + 1] = w.y; ww[4 * e + 2] = w.z; ww[4 * e + 3] = w.w;
      }
#pragma unroll
      for (int k = 0; k < CG; ++k)
        if (k < nc) {
          const float* __restrict__ sr = s_irows + (size_t)k * M;
          pp::f4 r;
          r.x = __builtin_fmaf(ww[2], sr[ii[2]], __builtin_fmaf(ww[0], sr[ii[0]], ww[1] * sr[ii[1]]));
          r.y = __builtin_fmaf(ww[5], sr[ii[5]], __builtin_fmaf(ww[3], sr[ii[3]], ww[4] * sr[ii[4]]));
          r.z = __builtin_fmaf(ww[8], sr[ii[8]], __builtin_fmaf(ww[6], sr[ii[6]], ww[7] * sr[ii[7]]));
          r.w = __builtin_fmaf(ww[11], sr[ii[11]], __builtin_fmaf(ww[9], sr[ii[9]], ww[10] * sr[ii[10]]));
          *reinterpret_cast<pp::f4*>(out + ((size_t)b * C + c0 + k) * N + n0) = r;
        }
    }
  } else {  // no alignment assumed: one n per thread and step, 4-byte accesses (all coalesced)
    for (int n = t; n < N; n += 1024) {
      const int* __restrict__ id = idx + ((size_t)b * N + n) * 3;
      const float* __restrict__ w = weight + ((size_t)b * N + n) * 3;
      const int i0 = id[0], i1 = id[1], i2 = id[2];
      const float w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
      for (int k = 0; k < CG; ++k)
        if (k < nc) {
          const float* __restrict__ sr = s_irows + (size_t)k * M;
          out[((size_t)b * C + c0 + k) * N + n] = __builtin_fmaf(w2, sr[i2], __builtin_fmaf(w0, sr[i0], w1 * sr[i1]));
        }
    }
  }
}

// The 16-bit channel-group form, the algorithm of three_interpolate_rows_kernel: CG rows of T staged in LDS (2 M bytes
// each), widened as they are gathered; the canonical chain in fp32 and one rounding.  VEC: M % 8 == 0, N % 4 == 0,
// points / idx / weight 16-byte and out 8-byte aligned -- 16-byte staging, four n per lane, one 8-byte store per channel.
// A kernel of its own because no common source compiles to both kernels' instruction streams (NOTEBOOK.md, "one set of
// forward kernels"); the two share launch_three_interpolate_rows.
template <int CG, bool VEC, typename T>
__global__ __launch_bounds__(1024) void three_interpolate_rows_b16_kernel(const T* __restrict__ points,
                                                                          const int* __restrict__ idx,
                                                                          const float* __restrict__ weight,
                                                                          T* __restrict__ out, int B, int C,
                                                                          int M, int N) {
  extern __shared__ __attribute__((aligned(16))) u16 s_i16[];  // [CG][M] of T
  T* s_rows = reinterpret_cast<T*>(s_i16);
  const int groups = (C + CG - 1) / CG;
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / groups);
  if (b >= B) return;
  const int c0 = (y % groups) * CG;
  const int nc = min(CG, C - c0);
  const int t = threadIdx.x;
  for (int k = 0; k < nc; ++k) {
    const T* __restrict__ rowp = points + ((size_t)b * C + c0 + k) * M;
    if constexpr (VEC) {
      for (int e = t; e < (M >> 3); e += 1024)
        reinterpret_cast<u4v*>(s_rows + (size_t)k * M)[e] = reinterpret_cast<const u4v*>(rowp)[e];
    } else {
      for (int e = t; e < M; e += 1024) s_rows[(size_t)k * M + e] = rowp[e];
    }
  }
  __syncthreads();
  if constexpr (VEC) {
    for (int n0 = 4 * t; n0 < N; n0 += 4096) {
      int ii[12];
      float ww[12];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const pp::i4 q = reinterpret_cast<const pp::i4*>(idx + ((size_t)b * N + n0) * 3)[e];
        const pp::f4 w = reinterpret_cast<const pp::f4*>(weight + ((size_t)b * N + n0) * 3)[e];
        ii[4 * e] = q.x; ii[4 * e + 1] = q.y; ii[4 * e + 2] = q.z; ii[4 * e + 3] = q.w;
        ww[4 * e] = w.x; ww[4 * e + 1] = w.y; ww[4 * e + 2] = w.z; ww[4 * e + 3] = w.w;
      }
#pragma unroll
      for (int k = 0; k < CG; ++k)
        if (k < nc) {
          const T* __restrict__ sr = s_rows + (size_t)k * M;
          T r[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            r[j] = pp::narrow<T>(__builtin_fmaf(ww[3 * j + 2], pp::widen(sr[ii[3 * j + 2]]),
                                                __builtin_fmaf(ww[3 * j], pp::widen(sr[ii[3 * j]]),
                                                               ww[3 * j + 1] * pp::widen(sr[ii[3 * j + 1]]))));
          u2v packed;
          __builtin_memcpy(&packed, r, 8);
          *reinterpret_cast<u2v*>(out + ((size_t)b * C + c0 + k) * N + n0) = packed;
        }
    }
  } else {  // no alignment assumed: one n per lane and step, 2-byte stores
    for (int n = t; n < N; n += 1024) {
      const int* __restrict__ id = idx + ((size_t)b * N + n) * 3;
      const float* __restrict__ w = weight + ((size_t)b * N + n) * 3;
      const int i0 = id[0], i1 = id[1], i2 = id[2];
      const float w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
      for (int k = 0; k < CG; ++k)
        if (k < nc) {
          const T* __restrict__ sr = s_rows + (size_t)k * M;
          out[((size_t)b * C + c0 + k) * N + n] = pp::narrow<T>(
              __builtin_fmaf(w2, pp::widen(sr[i2]), __builtin_fmaf(w0, pp::widen(sr[i0]), w1 * pp::widen(sr[i1]))));
        }
    }
  }
}

// one launcher for both: the fp32 kernel for float, the widening one for pp::f16 / pp::bf16
template <int CG, bool VEC, typename T>
static int launch_three_interpolate_rows(const T* points, const int* idx, const float* weight, T* out,
                                         int B, int C, int M, int N, hipStream_t s) {
  void (*kernel)(const T*, const int*, const float*, T*, int, int, int, int);
  if constexpr (std::is_same<T, float>::value)
    kernel = three_interpolate_rows_kernel<CG, VEC>;
  else
    kernel = three_interpolate_rows_b16_kernel<CG, VEC, T>;
  static pp::DeviceFlags ok;
  const hipError_t e = pp::allow_big_lds(kernel, 152 * 1024, ok);
  if (e != hipSuccess) return (int)e;
  const long long wgs = 8LL * ((B + 7) / 8) * ((C + CG - 1) / CG);
  if (wgs > 0x7fffffffLL) return PP_EINVAL;
  kernel<<<dim3((unsigned)wgs), dim3(1024), (size_t)CG * M * sizeof(T), s>>>(points, idx, weight, out, B, C, M, N);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

// three_interpolate backward (ref interpolate_gpu.cu:120-142)
__global__ __launch_bounds__(256) void three_interpolate_grad_kernel(
    const float* __restrict__ grad_out, const int* __restrict__ idx,
    const float* __restrict__ weight, float* __restrict__ grad_points, int C, int N, int M,
    int c_per_block) {
  const int b = blockIdx.z;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int* id = idx + ((size_t)b * N + n) * 3;
  const float* w = weight + ((size_t)b * N + n) * 3;
  const int i0 = id[0], i1 = id[1], i2 = id[2];
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const int c0 = blockIdx.y * c_per_block;
  const int c1 = min(C, c0 + c_per_block);
  for (int c = c0; c < c1; ++c) {
    const float g = grad_out[((size_t)b * C + c) * N + n];
    float* __restrict__ gp = grad_points + ((size_t)b * C + c) * M;
    atomicAdd(gp + i0, g * w0);
    atomicAdd(gp + i1, g * w1);
    atomicAdd(gp + i2, g * w2);
  }
}

// three_interpolate backward with LDS columns in double (see group_points_grad_lds64_kernel for why
// double): one workgroup per (batch, group of CG channels) keeps CG columns grad_points[b,c,:] in
// LDS, reads (idx, weight) of a point once for the CG channels and adds the fp32 products
// grad_out*weight (the reference's rounding, interpolate_gpu.cu:137-139) with ds_add_f64.
template <int CG, typename T = float>  // 16-bit T: widened grad_out, the columns WRITTEN as T(float(sum))
__global__ __launch_bounds__(1024) void three_interpolate_grad_lds64_kernel(
    const T* __restrict__ grad_out, const int* __restrict__ idx, const float* __restrict__ weight,
    T* __restrict__ grad_points, int B, int C, int N, int M) {
  extern __shared__ __attribute__((aligned(16))) double s_acc64[];  // [CG][M]
  const int groups = (C + CG - 1) / CG;
  const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
  const int b = x + 8 * (y / groups);
  const int c0 = (y % groups) * CG;
  if (b >= B) return;
  const int nc = min(CG, C - c0);
  const int t = threadIdx.x;
  for (int k = t; k < CG * M; k += 1024) s_acc64[k] = 0.0;
  __syncthreads();
  const T* __restrict__ go = grad_out + ((size_t)b * C + c0) * N;
  for (int n = t; n < N; n += 1024) {
    const int* id = idx + ((size_t)b * N + n) * 3;
    const float* w = weight + ((size_t)b * N + n) * 3;
    const int i0 = id[0], i1 = id[1], i2 = id[2];
    const float w0 = w[0], w1 = w[1], w2 = w[2];
    float g[CG];
#pragma unroll
    for (int k = 0; k < CG; ++k) g[k] = pp::widen(go[(size_t)min(k, nc - 1) * N + n]);
#pragma unroll
    for (int k = 0; k < CG; ++k)
      if (k < nc) {
        double* col = s_acc64 + (size_t)k * M;
        atomicAdd(col + i0, (double)(g[k] * w0));
        atomicAdd(col + i1, (double)(g[k] * w1));
        atomicAdd(col + i2, (double)(g[k] * w2));
      }
  }
  __syncthreads();
  for (int k = 0; k < nc; ++k) {
    T* __restrict__ gp = grad_points + ((size_t)b * C + c0 + k) * M;
    if constexpr (std::is_same<T, float>::value) {
      for (int m = t; m < M; m += 1024) gp[m] += (float)s_acc64[(size_t)k * M + m];  // accumulate: the ABI's contract
    } else {
      for (int m = t; m < M; m += 1024) gp[m] = pp::narrow<T>((float)s_acc64[(size_t)k * M + m]);
    }
  }
}

template <int CG, typename T>
static int launch_three_interpolate_grad_lds64(const T* grad_out, const int* idx, const float* weight,
                                               T* grad_points, int B, int C, int N, int M, hipStream_t s) {
  static pp::DeviceFlags ok;
  const hipError_t e = pp::allow_big_lds(three_interpolate_grad_lds64_kernel<CG, T>, 152 * 1024, ok);
  if (e != hipSuccess) return (int)e;
  const long long wgs = 8LL * ((B + 7) / 8) * ((C + CG - 1) / CG);
  if (wgs > 0x7fffffffLL) return PP_EINVAL;
  three_interpolate_grad_lds64_kernel<CG, T><<<dim3((unsigned)wgs), dim3(1024), (size_t)CG * M * sizeof(double), s>>>(
      grad_out, idx, weight, grad_points, B, C, N, M);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

// channels per block so that the grid has roughly >= 8 blocks per CU without re-reading idx more
// often than needed
int pick_c_per_block(long long col_blocks, int B, int C) {
  const long long want = 256LL * 8;
  long long have = col_blocks * B;
  int splits = 1;
  while (splits < C && have * splits < want) splits *= 2;
  if (splits > C) splits = C;
  return (C + splits - 1) / splits;
}

bool grid_ok(long long x, long long y, long long z) {
  return x > 0 && y > 0 && z > 0 && x <= 0x7fffffffLL && y <= 65535 && z <= 65535;
}

}  // namespace

// ================================================================================================
// The forward dispatches: one per operator, a template on the element (float; u16 for the copies of fp16 / bf16
// features; pp::f16 / pp::bf16 where there is arithmetic), written in L = 16 / sizeof(E) elements per 16 bytes.  Where
// the two element sizes follow different policies, the difference stands once, under `if constexpr`.
// ================================================================================================
// 0 = automatic; 1 = force the global-gather kernel; 2 = 16-bit: the LDS form wherever the row fits, fp32: as 0
// (tests and tuning)
static pp::Knob g_gather_variant;
extern "C" void pp_debug_set_gather_variant(int v) { g_gather_variant.set(v); }

namespace {

template <typename E>
int gather_forward(const E* points, const int* idx, E* out, int B, int C, int N, int M, void* stream) {
  constexpr int L = 16 / sizeof(E);
  constexpr bool k32 = sizeof(E) == 4;
  if (B < 0 || C < 0 || N < 0 || M < 0) return PP_EINVAL;
  if (B == 0 || C == 0 || M == 0) return PP_OK;
  if (!points || !idx || !out || N == 0) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int gv = g_gather_variant;
  // LDS-staged rows: the row fits, reading whole rows pays (N <= 16 M); the 16-byte variant when rows and the lanes'
  // index runs are aligned, the element-sized variant otherwise
  bool pays = (long long)N <= 16LL * M && (long long)B * C >= 512 && M >= 1024;
  if constexpr (!k32) pays = pays || gv == 2;  // 16-bit: knob 2 takes the form wherever the row fits (fp32 reads 2 as 0)
  if (gv != 1 && (size_t)N * sizeof(E) <= 152 * 1024 && pays) {
    bool vec = N % L == 0 && M % L == 0 && (uintptr_t)points % 16 == 0 && (uintptr_t)idx % 16 == 0 &&
               (uintptr_t)out % 16 == 0;
    if constexpr (k32) vec = vec && N <= 16384;  // fp32: the vector kernel prefetches a row of at most 64 KiB
    int cpb = 4;
    while (cpb > 1 && 8LL * ((B + 7) / 8) * ((C + cpb - 1) / cpb) < 1024) cpb /= 2;
    const int groups = (C + cpb - 1) / cpb;
    const long long wgs = 8LL * ((B + 7) / 8) * groups;
    if (wgs <= 0x7fffffffLL) {
      static pp::DeviceFlags ok1, ok2, ok4, oks;
      auto launch = [&](auto kernel, int lds_limit, pp::DeviceFlags& ok) -> int {
        if (pp::allow_big_lds(kernel, lds_limit, ok) != hipSuccess) return PP_EINVAL;
        kernel<<<dim3((unsigned)wgs), dim3(1024), (size_t)N * sizeof(E), s>>>(points, idx, out, B, C, N, M, cpb, groups);
        PP_RETURN_IF_LAUNCH_FAILED();
        return PP_OK;
      };
      if (!vec) return launch(gather_fwd_lds_kernel<1, false, E>, 152 * 1024, oks);
      if constexpr (k32) {  // fp32: KR = 16-byte units per thread of the prefetched row; LDS limit 64 KiB
        const int n4 = N / 4;
        if (n4 <= 1024) return launch(gather_fwd_lds_kernel<1, true>, 64 * 1024, ok1);
        if (n4 <= 2048) return launch(gather_fwd_lds_kernel<2, true>, 64 * 1024, ok2);
        return launch(gather_fwd_lds_kernel<4, true>, 64 * 1024, ok4);
      } else {  // 16-bit: one vector kernel, any row that fits
        return launch(gather_fwd_lds_b16_kernel, 152 * 1024, ok1);
      }
    }
  }
  const long long cols = (M + 255) / 256;
  const int cpb = pick_c_per_block(cols, B, C);
  const long long gy = (C + cpb - 1) / cpb;
  if (!grid_ok(cols, gy, B)) return PP_EINVAL;
  gather_fwd_kernel<E><<<dim3((unsigned)cols, (unsigned)gy, (unsigned)B), dim3(256), 0, s>>>(points, idx, out, C, N, M,
                                                                                           cpb);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

}  // namespace

extern "C" int pp_gather_forward_f32(const float* points, const int* idx, float* out, int B, int C,
                                     int N, int M, void* stream) {
  return gather_forward(points, idx, out, B, C, N, M, stream);
}
extern "C" int pp_gather_forward_b16(const void* points, const int* idx, void* out, int B, int C, int N, int M,
                                     void* stream) {
  return gather_forward((const u16*)points, idx, (u16*)out, B, C, N, M, stream);
}

// 0 = automatic; 1 = force the one-wave-per-64-centres kernel (tests and tuning)
static pp::Knob g_ball_variant;
extern "C" void pp_debug_set_ball_query_variant(int v) { g_ball_variant.set(v); }

static int ball_query_launch(const float* new_xyz, const float* xyz, int* idx, int B, int N, int M,
                             float radius, int nsample, const pp::GridSet* skip, void* stream) {
  if (B < 0 || N < 0 || M < 0 || nsample < 0) return PP_EINVAL;
  if (B == 0 || M == 0 || nsample == 0) return PP_OK;
  if (!new_xyz || !idx || (N > 0 && !xyz)) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const float radius2 = radius * radius;  // fp32, as the reference (sampling_cuda.cu:354)
  // split form: 4 waves share 64 centres (one cloud quarter each); needs its lists in LDS and
  // enough points for four quarters
  if (g_ball_variant != 1 && N >= 4 * kBqGroup) {
    const int tiles64 = (M + 63) / 64;
    const long long blocks64 = (long long)B * tiles64;
    const size_t esz = N <= 65536 ? sizeof(unsigned short) : sizeof(unsigned);
    const size_t lds64 = (size_t)4 * 64 * nsample * esz + (size_t)4 * 64 * sizeof(int);
    if (blocks64 <= 0x7fffffffLL && lds64 <= 64 * 1024) {
      if (esz == 2)
        ball_query_split_kernel<unsigned short><<<dim3((unsigned)blocks64), dim3(256), lds64, s>>>(
            new_xyz, xyz, idx, N, M, radius2, nsample, tiles64, skip);
      else
        ball_query_split_kernel<unsigned><<<dim3((unsigned)blocks64), dim3(256), lds64, s>>>(
            new_xyz, xyz, idx, N, M, radius2, nsample, tiles64, skip);
      PP_RETURN_IF_LAUNCH_FAILED();
      return PP_OK;
    }
  }
  const int tiles = (M + 255) / 256;
  const long long blocks = (long long)B * tiles;
  if (blocks > 0x7fffffffLL) return PP_EINVAL;
  const size_t lds = (size_t)4 * 64 * nsample * sizeof(int);
  if (lds <= 64 * 1024) {
    ball_query_kernel<true><<<dim3((unsigned)blocks), dim3(256), lds, s>>>(
        new_xyz, xyz, idx, N, M, radius2, nsample, tiles, skip);
  } else {
    ball_query_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(
        new_xyz, xyz, idx, N, M, radius2, nsample, tiles, skip);
  }
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_ball_query_f32(const float* new_xyz, const float* xyz, int* idx, int B, int N,
                                 int M, float radius, int nsample, void* stream) {
  return ball_query_launch(new_xyz, xyz, idx, B, N, M, radius, nsample, nullptr, stream);
}

namespace pp {
int ball_query_scan_unusable(const float* new_xyz, const float* xyz, int* idx, int B, int N, int M,
                             float radius, int nsample, const GridSet* sets, hipStream_t s) {
  return ball_query_launch(new_xyz, xyz, idx, B, N, M, radius, nsample, sets, (void*)s);
}
}  // namespace pp

// 0 = automatic; 1 = force the global-gather kernel; 2/4/8 = force the VGPR-staged LDS kernel (fp32: with that many
// index quads per thread; 16-bit: its one instantiation); 604/608/616 = the LDS-DMA kernel on chunks of 8192 / 16384 /
// 32768 positions where the positions fill whole chunks, the VGPR-staged one elsewhere; any other value above 100 = no
// LDS-DMA kernel (tests and tuning)
static pp::Knob g_group_variant;
extern "C" void pp_debug_set_group_points_variant(int v) { g_group_variant.set(v); }

namespace {

template <typename E>
int group_points_strided(const E* points, const int* idx, E* out, int B, int C, int N, int npoint, int nsample,
                         long long out_batch_stride, void* stream) {
  constexpr int L = 16 / sizeof(E);
  constexpr bool k32 = sizeof(E) == 4;
  if (B < 0 || C < 0 || N < 0 || npoint < 0 || nsample < 0) return PP_EINVAL;
  const long long P = (long long)npoint * nsample;
  const long long obs = out_batch_stride;
  if (obs < (long long)C * P) return PP_EINVAL;
  if (B == 0 || C == 0 || P == 0) return PP_OK;
  if (!points || !idx || !out || N == 0) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int gv = g_group_variant;
  const bool vec = (P % L == 0) && (obs % L == 0) && ((uintptr_t)idx % 16 == 0) && ((uintptr_t)out % 16 == 0);
  bool fills = (long long)B * P >= 256LL * 2048;  // enough positions to fill the chip
  // 16-bit: a knob value that names an LDS form takes it below that size too (tests); fp32: the floor always holds
  if constexpr (!k32) fills = fills || gv != 0;
  // LDS-staged forms: row within 64 KiB (two workgroups per CU), rows 16-byte aligned, enough channels to amortise
  // keeping the indices in registers
  if (gv != 1 && vec && N % L == 0 && (uintptr_t)points % 16 == 0 && (size_t)N * sizeof(E) <= 64 * 1024 && C >= 4 &&
      fills) {
    // the LDS-DMA form wherever the positions fill whole chunks of 32768, 16384 or 8192 (16 / 8 / 4 index quads per
    // thread, or 8 / 4 / 2 octets): measured round 6 at or ahead of every other form on every shape it can take
    // (tools/group_shapes_time.py); the output is written with non-temporal stores (4 GiB at config 4, nothing of it is
    // read back from the caches)
    bool ok = false;
    if (gv == 616 || gv == 0) ok = launch_group_dma1<E, 64 / L>(points, idx, out, B, C, N, P, obs, s);
    if (!ok && (gv == 608 || gv == 0)) ok = launch_group_dma1<E, 32 / L>(points, idx, out, B, C, N, P, obs, s);
    if (!ok && (gv == 604 || gv == 0)) ok = launch_group_dma1<E, 16 / L>(points, idx, out, B, C, N, P, obs, s);
    if (!ok) {  // ragged chunks, or forced by 2 / 4 / 8 / a value above 100: the VGPR-staged form
      if constexpr (k32) {
        // 8 / 4 / 2 index quads per thread by the positions a CU gets (> 100: the values 604 / 608 / 616 on shapes
        // their LDS-DMA kernel cannot take)
        const long long per_cu = (long long)B * P / 512;  // positions per half-CU
        if (gv == 8 || ((gv == 0 || gv > 100) && per_cu >= 512LL * 4 * 8))
          ok = launch_group_lds<8>(points, idx, out, B, C, N, P, obs, s);
        else if (gv == 4 || (gv == 0 && per_cu >= 512LL * 4 * 4))
          ok = launch_group_lds<4>(points, idx, out, B, C, N, P, obs, s);
        else
          ok = launch_group_lds<2>(points, idx, out, B, C, N, P, obs, s);
      } else {
        ok = launch_group_lds_b16(points, idx, out, B, C, N, P, obs, s);
      }
    }
    if (ok) {
      PP_RETURN_IF_LAUNCH_FAILED();
      return PP_OK;
    }
  }
  // fp32 only -- unaligned shapes, or rows beyond 64 KiB: the 4-byte LDS-staged form, from 2^28 output elements (measured
  // round 6: 1.89 against 7.7 ms for the global gather at config 4 less one point and one sample, but 0.27 against 0.21
  // at a fifth of a GiB and 0.079 against 0.050 at 69 MB: tools/group_shapes_time.py).  No 16-bit form of it.
  if constexpr (k32) {
    if (gv != 1 && (size_t)N * sizeof(float) <= 152 * 1024 && C >= 4 && (long long)B * P >= 256LL * 2048 &&
        (gv != 0 || (long long)B * P * C >= (1LL << 28))) {
      constexpr int V = 16;
      const long long chunks = (P + 1024LL * V - 1) / (1024LL * V);
      const long long blocks = 8LL * ((B + 7) / 8) * chunks;
      if (chunks <= 0x7fffffLL && blocks <= 0x7fffffffLL) {
        static pp::DeviceFlags ok_s;
        const hipError_t e = pp::allow_big_lds(group_points_lds_scalar_kernel<V>, 152 * 1024, ok_s);
        if (e != hipSuccess) return (int)e;
        group_points_lds_scalar_kernel<V><<<dim3((unsigned)blocks), dim3(1024), (size_t)N * sizeof(float), s>>>(
            points, idx, out, B, C, N, P, (int)chunks, obs);
        PP_RETURN_IF_LAUNCH_FAILED();
        return PP_OK;
      }
    }
  }
  const long long threads = vec ? P / L : P;
  const long long cols = (threads + 255) / 256;
  const int cpb = pick_c_per_block(cols, B, C);
  const long long gy = (C + cpb - 1) / cpb;
  if (!grid_ok(cols, gy, B)) return PP_EINVAL;
  const dim3 grid((unsigned)cols, (unsigned)gy, (unsigned)B);
  if (vec)
    group_points_kernel<E, true><<<grid, dim3(256), 0, s>>>(points, idx, out, C, N, P, cpb, obs);
  else
    group_points_kernel<E, false><<<grid, dim3(256), 0, s>>>(points, idx, out, C, N, P, cpb, obs);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

}  // namespace

extern "C" int pp_group_points_f32(const float* points, const int* idx, float* out, int B, int C,
                                   int N, int npoint, int nsample, void* stream) {
  return group_points_strided(points, idx, out, B, C, N, npoint, nsample, (long long)C * npoint * nsample, stream);
}
extern "C" int pp_group_points_strided_f32(const float* points, const int* idx, float* out, int B, int C,
                                           int N, int npoint, int nsample, long long out_batch_stride,
                                           void* stream) {
  return group_points_strided(points, idx, out, B, C, N, npoint, nsample, out_batch_stride, stream);
}
extern "C" int pp_group_points_strided_b16(const void* points, const int* idx, void* out, int B, int C, int N,
                                           int npoint, int nsample, long long out_batch_stride, void* stream) {
  return group_points_strided((const u16*)points, idx, (u16*)out, B, C, N, npoint, nsample, out_batch_stride, stream);
}

static int three_nn_launch(const float* unknown, const float* known, float* dist2, int* idx, int B, int N,
                           int M, const pp::GridSet* skip, void* stream) {
  if (B < 0 || N < 0 || M < 0) return PP_EINVAL;
  if (B == 0 || N == 0) return PP_OK;
  if (!unknown || !dist2 || !idx || (M > 0 && !known)) return PP_EINVAL;
  const int tiles = (N + 255) / 256;
  const long long blocks = (long long)B * tiles;
  if (blocks > 0x7fffffffLL) return PP_EINVAL;
  three_nn_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(
      unknown, known, dist2, idx, N, M, tiles, skip);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_three_nn_f32(const float* unknown, const float* known, float* dist2, int* idx,
                               int B, int N, int M, void* stream) {
  return three_nn_launch(unknown, known, dist2, idx, B, N, M, nullptr, stream);
}

// 0 = automatic; 1 = force the global-gather kernel; 2 = no channel-group form (fp32: the row-at-a-time LDS form
// where it applies; 16-bit: the global form); 3 = 16-bit: the channel-group form wherever the rows fit, fp32: as 0
// (tests and tuning)
static pp::Knob g_interp_variant;
extern "C" void pp_debug_set_three_interpolate_variant(int v) { g_interp_variant.set(v); }

namespace {

template <typename T>
int three_interpolate(const T* points, const int* idx, const float* weight, T* out, int B, int C, int M, int N,
                      void* stream) {
  constexpr int L = 16 / sizeof(T);
  constexpr bool k32 = sizeof(T) == 4;
  if (B < 0 || C < 0 || N < 0 || M < 0) return PP_EINVAL;
  if (B == 0 || C == 0 || N == 0) return PP_OK;
  if (!points || !idx || !weight || !out || M == 0) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int iv = g_interp_variant;
  // the 16-byte variants: aligned rows, index and weight quads; out aligned to a lane's four elements (fp32: 16 bytes,
  // 16-bit: 8)
  const bool vec = M % L == 0 && N % 4 == 0 && (uintptr_t)points % 16 == 0 && (uintptr_t)idx % 16 == 0 &&
                   (uintptr_t)weight % 16 == 0 && (uintptr_t)out % (4 * sizeof(T)) == 0;
  // channel-group form (rows staged once, §three_interpolate_rows_kernel): as many whole rows per workgroup as keep two
  // workgroups on a CU (4 x 16 KiB at M = 4096 floats), fewer for long rows
  const size_t rowb = (size_t)M * sizeof(T);
  bool enough = N >= 2048 && 8LL * ((B + 7) / 8) * ((C + 3) / 4) >= 256;
  if constexpr (!k32) enough = enough || iv == 3;  // 16-bit: knob 3 waives both floors (tests)
  if (iv != 1 && iv != 2 && rowb <= 152 * 1024 && enough) {
    int cg = (4 * rowb <= 64 * 1024 && C >= 4) ? 4 : 1;
    if constexpr (k32) {  // fp32 only: two rows where four do not fit
      if (cg == 1 && 2 * rowb <= 152 * 1024 && C >= 2) cg = 2;
    }
    if (vec) {
      if (cg == 4) return launch_three_interpolate_rows<4, true>(points, idx, weight, out, B, C, M, N, s);
      if constexpr (k32)
        if (cg == 2) return launch_three_interpolate_rows<2, true>(points, idx, weight, out, B, C, M, N, s);
      return launch_three_interpolate_rows<1, true>(points, idx, weight, out, B, C, M, N, s);
    }
    if (cg == 4) return launch_three_interpolate_rows<4, false>(points, idx, weight, out, B, C, M, N, s);
    if constexpr (k32)
      if (cg == 2) return launch_three_interpolate_rows<2, false>(points, idx, weight, out, B, C, M, N, s);
    return launch_three_interpolate_rows<1, false>(points, idx, weight, out, B, C, M, N, s);
  }
  // fp32 only, and what its knob value 2 selects -- the row-at-a-time LDS form: 16-byte aligned rows and quads, row
  // within 64 KiB, enough channels to amortise
  if constexpr (k32) {
    if (iv != 1 && vec && M <= 16384 && C >= 4 && (long long)B * N >= 64 * 2048) {
      const int m4 = M / 4;
      if (m4 <= 512) launch_three_interpolate_lds<1>(points, idx, weight, out, B, C, M, N, s);
      else if (m4 <= 1024) launch_three_interpolate_lds<2>(points, idx, weight, out, B, C, M, N, s);
      else if (m4 <= 2048) launch_three_interpolate_lds<4>(points, idx, weight, out, B, C, M, N, s);
      else launch_three_interpolate_lds<8>(points, idx, weight, out, B, C, M, N, s);
      PP_RETURN_IF_LAUNCH_FAILED();
      return PP_OK;
    }
  }
  const long long cols = (N + 255) / 256;
  const int cpb = pick_c_per_block(cols, B, C);
  const long long gy = (C + cpb - 1) / cpb;
  if (!grid_ok(cols, gy, B)) return PP_EINVAL;
  three_interpolate_kernel<T><<<dim3((unsigned)cols, (unsigned)gy, (unsigned)B), dim3(256), 0, s>>>(
      points, idx, weight, out, C, M, N, cpb);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

}  // namespace

extern "C" int pp_three_interpolate_f32(const float* points, const int* idx, const float* weight,
                                        float* out, int B, int C, int M, int N, void* stream) {
  return three_interpolate(points, idx, weight, out, B, C, M, N, stream);
}
extern "C" int pp_three_interpolate_f16(const void* points, const int* idx, const float* weight, void* out, int B,
                                        int C, int M, int N, void* stream) {
  return three_interpolate((const pp::f16*)points, idx, weight, (pp::f16*)out, B, C, M, N, stream);
}
extern "C" int pp_three_interpolate_bf16(const void* points, const int* idx, const float* weight, void* out, int B,
                                         int C, int M, int N, void* stream) {
  return three_interpolate((const pp::bf16*)points, idx, weight, (pp::bf16*)out, B, C, M, N, stream);
}

// ================================================================================================
// The scatter-add backwards: gather_backward, group_points_grad, three_interpolate_grad, for fp32 and 16-bit features
// (DESIGN.md §4).  Every entry point describes its call as a ScatterDesc; scatter_plan -- host arithmetic on the
// description and the three knobs, nothing else -- names the form, and scatter_run validates, serves the empty sizes,
// zero-fills where an accumulating form stands behind an entry that promises a write, and launches.
//   atomics  the reference's global atomicAdd kernels (fp32 only: there are no 16-bit floating-point atomics)
//   column   double accumulators in the LDS (group_points_grad_lds64_kernel, three_interpolate_grad_lds64_kernel)
//   sorted   the sorted triples of scatter.hip (pp::ssa_run) in the caller's workspace
//   ordered  the same with every destination's terms added in ascending source order (deterministic mode): no
//            atomics on floating-point data, bit-equal to a sequential loop in the reference's launch order
// fp32 outputs are ACCUMULATED into by every form but group's column with `overwrite`; 16-bit outputs are WRITTEN.
// ================================================================================================
// group_points_grad: 0 = automatic; 1 = no double column; 2 = the column also below 4096 positions; every other
// value means 0.  three_interpolate_grad: 0 = automatic; 1 and 3 = no double column; 2 = the column also below 2048
// points.  scatter mode: 1 = never the sorted form (the ordered form is an entry's contract, not a choice).
static pp::Knob g_group_grad_variant;
extern "C" void pp_debug_set_group_points_grad_variant(int v) { g_group_grad_variant.set(v); }
static pp::Knob g_interp_grad_variant;
extern "C" void pp_debug_set_three_interpolate_grad_variant(int v) { g_interp_grad_variant.set(v); }
static pp::Knob g_scatter_mode;
extern "C" void pp_debug_set_scatter_mode(int v) { g_scatter_mode.set(v); }

extern "C" size_t pp_scatter_workspace_bytes(int B, long long triples_per_batch, int destinations,
                                             int per_source, int weighted) {
  if (per_source < 1) return 0;
  return pp::ssa_workspace_bytes(B, triples_per_batch, per_source, destinations, weighted != 0);
}

namespace {

constexpr int kColumnLds = 152 * 1024;   // the LDS a double column may take
constexpr int kW64 = kColumnLds / 8;     // destinations per workgroup with a double column

// out[b, c, dst[b, p]] += (weight ? weight[b, p] : 1) * src[b * src_bstride + c * (P / R) + p / R], in the terms of
// pp_scatter_workspace_bytes
struct ScatterDesc {
  int op, B, C;           // PP_SCATTER_GATHER / _GROUP / _INTERPOLATE
  long long P;            // triples per batch element; < 0 when the entry was passed a negative size
  int R, Nd;              // triples per source, destinations per batch element
  bool weighted;
  long long src_bstride;
  int elem_bytes = 4;     // 4 = float, 2 = f16 / bf16 (scatter_run fills it in from its element type)
  bool write = false, ordered = false;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  ScatterDesc with(bool write_, bool ordered_, void* ws_, size_t bytes) const {
    ScatterDesc d = *this;
    d.write = write_, d.ordered = ordered_, d.ws = ws_, d.ws_bytes = ws_ ? bytes : 0;
    return d;
  }
};

ScatterDesc gather_desc(int B, int C, int N, int M) {
  return {PP_SCATTER_GATHER, B, C, N < 0 ? -1 : M, 1, N, false, (long long)C * M};
}
ScatterDesc group_desc(int B, int C, int N, int npoint, int nsample, long long grad_out_batch_stride) {
  const bool neg = N < 0 || npoint < 0 || nsample < 0;
  return {PP_SCATTER_GROUP, B, C, neg ? -1 : (long long)npoint * nsample, 1, N, false, grad_out_batch_stride};
}
ScatterDesc interp_desc(int B, int C, int N, int M) {
  return {PP_SCATTER_INTERPOLATE, B, C, M < 0 ? -1 : 3LL * N, 3, M, true, (long long)C * N};
}

struct ScatterKnobs {
  int group, interp, scatter;
};

// The policy, for B, C, P, Nd > 0.  Measured on the MI355X: at config 4 (16 triples per destination) the sorted form
// moves more bytes through each CU than group's column spends on its LDS atomics (6.3 vs 5.8 ms), and wins where the
// lists are short (P <= 4 Nd); interpolate's column (0.18 ms at B=32, C=128, N=16384, M=4096) beats the sorted form
// (0.55 ms) wherever it fits; below 2^20 products the sort does not pay for itself against fp32 atomics.
int scatter_plan(const ScatterDesc& d, const ScatterKnobs& k) {
  const size_t need = pp::ssa_workspace_bytes(d.B, d.P, d.R, d.Nd, d.weighted);
  const bool fits = need != 0 && d.ws_bytes >= need;   // (need == 0: more than 20480 destinations, too many chunks)
  if (d.ordered) return fits ? PP_SCATTER_FORM_ORDERED : PP_SCATTER_FORM_NONE;
  const bool sorted = fits && k.scatter != 1;
  const bool big = (long long)d.B * d.P * d.C >= (1LL << 20);
  const bool f32 = d.elem_bytes == 4;
  // where no column applies: fp32 has its atomics and sorts only what is big; 16-bit sorts or has no form at all
  const int rest = f32 ? (sorted && big ? PP_SCATTER_FORM_SORTED : PP_SCATTER_FORM_ATOMICS)
                       : (sorted ? PP_SCATTER_FORM_SORTED : PP_SCATTER_FORM_NONE);
  if (d.op == PP_SCATTER_GROUP) {
    if (sorted && big && d.P <= 4LL * d.Nd) return PP_SCATTER_FORM_SORTED;
    const int nsplit = (d.Nd + kW64 - 1) / kW64;   // the column in destination ranges, at most 16 passes over grad_out
    if (k.group != 1 && (k.group == 2 || d.P >= 4096) && nsplit <= 16 &&
        8LL * ((d.B + 7) / 8) * d.C * nsplit <= 0x7fffffffLL)
      return PP_SCATTER_FORM_COLUMN;
    return f32 ? PP_SCATTER_FORM_ATOMICS : rest;
  }
  if (d.op == PP_SCATTER_INTERPOLATE && k.interp != 1 && k.interp != 3 && (size_t)d.Nd * sizeof(double) <= kColumnLds &&
      (k.interp == 2 || d.P / 3 >= 2048))
    return PP_SCATTER_FORM_COLUMN;   // enough points per column to pay for zeroing and flushing it
  return rest;
}

template <bool VEC, typename T>
int launch_group_column(const ScatterDesc& d, const T* src, const int* dst, T* out, hipStream_t s) {
  static pp::DeviceFlags ok;
  const hipError_t e = pp::allow_big_lds(group_points_grad_lds64_kernel<8, VEC, T>, kColumnLds, ok);
  if (e != hipSuccess) return (int)e;
  const int nsplit = (d.Nd + kW64 - 1) / kW64;
  const long long wgs = 8LL * ((d.B + 7) / 8) * d.C * nsplit;
  const int W = nsplit == 1 ? d.Nd : kW64;
  // overwrite: the column form writes every element once (no read of the output, no fill in front of it: 2 x 256 MB
  // less traffic at config 4)
  group_points_grad_lds64_kernel<8, VEC, T><<<dim3((unsigned)wgs), dim3(1024), (size_t)W * sizeof(double), s>>>(
      src, dst, out, d.B, d.C, d.Nd, d.P, d.src_bstride, nsplit, W, d.write ? 1 : 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

template <typename T>
int launch_column(const ScatterDesc& d, const T* src, const int* dst, const float* weight, T* out, hipStream_t s) {
  if (d.op == PP_SCATTER_GROUP) {
    // 16-byte index quads beside quads of T (16 or 8 bytes)
    const bool vec = (uintptr_t)src % (4 * sizeof(T)) == 0 && (uintptr_t)dst % 16 == 0 && d.P % 4 == 0 &&
                     d.src_bstride % 4 == 0;
    return vec ? launch_group_column<true>(d, src, dst, out, s) : launch_group_column<false>(d, src, dst, out, s);
  }
  const int N = (int)(d.P / 3), M = d.Nd;
  const size_t col = (size_t)M * sizeof(double);
  if (d.C >= 4 && 4 * col <= kColumnLds)
    return launch_three_interpolate_grad_lds64<4>(src, dst, weight, out, d.B, d.C, N, M, s);
  if (d.C >= 2 && 2 * col <= kColumnLds)
    return launch_three_interpolate_grad_lds64<2>(src, dst, weight, out, d.B, d.C, N, M, s);
  return launch_three_interpolate_grad_lds64<1>(src, dst, weight, out, d.B, d.C, N, M, s);
}

int launch_atomics(const ScatterDesc& d, const float* src, const int* dst, const float* weight, float* out,
                   hipStream_t s) {
  const long long sources = d.P / d.R;
  const long long cols = (sources + 255) / 256;
  const int cpb = pick_c_per_block(cols, d.B, d.C);
  const long long gy = (d.C + cpb - 1) / cpb;
  if (!grid_ok(cols, gy, d.B)) return PP_EINVAL;
  const dim3 grid((unsigned)cols, (unsigned)gy, (unsigned)d.B), block(256);
  if (d.op == PP_SCATTER_GATHER)
    gather_bwd_kernel<<<grid, block, 0, s>>>(src, dst, out, d.C, d.Nd, (int)sources, cpb);
  else if (d.op == PP_SCATTER_GROUP)
    group_points_grad_kernel<<<grid, block, 0, s>>>(src, dst, out, d.C, d.Nd, d.P, cpb, d.src_bstride);
  else
    three_interpolate_grad_kernel<<<grid, block, 0, s>>>(src, dst, weight, out, d.C, (int)sources, d.Nd, cpb);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

// Return codes for degenerate arguments differ by the entry's kind, as the entries always had them: a negative size is
// PP_EINVAL before any pointer is looked at; the accumulating entries (the reference's contract) serve B, C or the
// sources being 0 and reject work without destinations; the writing ones serve B, C or the destinations being 0 and
// zero the output when there are no sources; the fp32 ordered ones serve any zero size.
template <typename T>
int scatter_run(ScatterDesc d, const T* src, const int* dst, const float* weight, T* out, void* stream) {
  constexpr bool kF32 = std::is_same<T, float>::value;
  d.elem_bytes = (int)sizeof(T);
  hipStream_t s = (hipStream_t)stream;
  if (d.B < 0 || d.C < 0 || d.P < 0 || d.Nd < 0) return PP_EINVAL;
  const bool short_stride = d.src_bstride < (long long)d.C * (d.P / d.R);
  const size_t out_bytes = (size_t)d.B * d.C * d.Nd * sizeof(T);
  if (d.write) {
    if (d.B == 0 || d.C == 0 || d.Nd == 0) return PP_OK;
    if (!out) return PP_EINVAL;
    if (d.P == 0) return (int)pp::fill_bytes(out, 0, out_bytes, s);   // (+0 in all three types)
  } else if (d.ordered) {
    if (d.B == 0 || d.C == 0 || d.Nd == 0 || d.P == 0) return PP_OK;
  } else {
    if (short_stride) return PP_EINVAL;
    if (d.B == 0 || d.C == 0 || d.P == 0) return PP_OK;
  }
  if (!src || !dst || !out || (d.weighted && !weight) || d.Nd == 0 || short_stride) return PP_EINVAL;
  const int form = scatter_plan(d, {g_group_grad_variant, g_interp_grad_variant, g_scatter_mode});
  if (form == PP_SCATTER_FORM_NONE) return PP_ENOTSUP;
  const bool writes = !kF32 || (form == PP_SCATTER_FORM_COLUMN && d.op == PP_SCATTER_GROUP);
  if (d.write && !writes) {   // (pp::fill_bytes: not hipMemsetAsync)
    const hipError_t e = pp::fill_bytes(out, 0, out_bytes, s);
    if (e != hipSuccess) return (int)e;
  }
  if (form == PP_SCATTER_FORM_COLUMN) return launch_column(d, src, dst, weight, out, s);
  if constexpr (kF32)
    if (form == PP_SCATTER_FORM_ATOMICS) return launch_atomics(d, src, dst, weight, out, s);
  return pp::ssa_run(src, dst, d.weighted ? weight : nullptr, out, d.B, d.C, d.P, d.R, d.Nd, d.src_bstride, d.ws, s,
                     form == PP_SCATTER_FORM_ORDERED);
}

constexpr bool kAccumulate = false, kWrite = true;

}  // namespace

extern "C" int pp_debug_scatter_plan(int op, int elem_bytes, int write, int ordered, int B, int C, long long sources,
                                     int destinations, size_t workspace_bytes) {
  if (op < PP_SCATTER_GATHER || op > PP_SCATTER_INTERPOLATE || (elem_bytes != 2 && elem_bytes != 4)) return -1;
  if (B <= 0 || C <= 0 || sources <= 0 || sources > 0x7fffffffLL || destinations <= 0) return -1;
  ScatterDesc d = op == PP_SCATTER_GATHER  ? gather_desc(B, C, destinations, (int)sources)
                  : op == PP_SCATTER_GROUP ? group_desc(B, C, destinations, (int)sources, 1, C * sources)
                                           : interp_desc(B, C, (int)sources, destinations);
  d.elem_bytes = elem_bytes, d.write = write != 0, d.ordered = ordered != 0, d.ws_bytes = workspace_bytes;
  return scatter_plan(d, {g_group_grad_variant, g_interp_grad_variant, g_scatter_mode});
}

// ---- fp32, accumulating into the caller's (zeroed) output: the reference's contract ----
extern "C" int pp_gather_backward_f32(const float* grad_out, const int* idx, float* grad_points,
                                      int B, int C, int N, int M, void* stream) {
  return scatter_run(gather_desc(B, C, N, M), grad_out, idx, nullptr, grad_points, stream);
}
extern "C" int pp_group_points_grad_f32(const float* grad_out, const int* idx, float* grad_points,
                                        int B, int C, int N, int npoint, int nsample, void* stream) {
  return scatter_run(group_desc(B, C, N, npoint, nsample, (long long)C * npoint * nsample), grad_out, idx, nullptr,
                     grad_points, stream);
}
extern "C" int pp_group_points_grad_strided_f32(const float* grad_out, const int* idx, float* grad_points,
                                                int B, int C, int N, int npoint, int nsample,
                                                long long grad_out_batch_stride, void* stream) {
  return scatter_run(group_desc(B, C, N, npoint, nsample, grad_out_batch_stride), grad_out, idx, nullptr, grad_points,
                     stream);
}
extern "C" int pp_three_interpolate_grad_f32(const float* grad_out, const int* idx, const float* weight,
                                             float* grad_points, int B, int C, int N, int M, void* stream) {
  return scatter_run(interp_desc(B, C, N, M), grad_out, idx, weight, grad_points, stream);
}

// ---- the same with a caller-provided workspace (pp_scatter_workspace_bytes), which admits the sorted form ----
extern "C" int pp_gather_backward_ws_f32(const float* grad_out, const int* idx, float* grad_points, int B,
                                         int C, int N, int M, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  return scatter_run(gather_desc(B, C, N, M).with(kAccumulate, false, workspace, workspace_bytes), grad_out, idx,
                     nullptr, grad_points, stream);
}
extern "C" int pp_group_points_grad_ws_f32(const float* grad_out, const int* idx, float* grad_points, int B,
                                           int C, int N, int npoint, int nsample,
                                           long long grad_out_batch_stride, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  return scatter_run(group_desc(B, C, N, npoint, nsample, grad_out_batch_stride)
                         .with(kAccumulate, false, workspace, workspace_bytes),
                     grad_out, idx, nullptr, grad_points, stream);
}
extern "C" int pp_three_interpolate_grad_ws_f32(const float* grad_out, const int* idx, const float* weight,
                                                float* grad_points, int B, int C, int N, int M,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  return scatter_run(interp_desc(B, C, N, M).with(kAccumulate, false, workspace, workspace_bytes), grad_out, idx,
                     weight, grad_points, stream);
}

// ---- grad_points WRITTEN, not accumulated into: the caller passes uninitialised memory (the Python shim:
// torch.empty instead of torch.zeros) ----
extern "C" int pp_group_points_grad_out_ws_f32(const float* grad_out, const int* idx, float* grad_points, int B,
                                               int C, int N, int npoint, int nsample,
                                               long long grad_out_batch_stride, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  return scatter_run(group_desc(B, C, N, npoint, nsample, grad_out_batch_stride)
                         .with(kWrite, false, workspace, workspace_bytes),
                     grad_out, idx, nullptr, grad_points, stream);
}

// ---- ORDERED (deterministic mode): selected by the Python / C++ host side when
// torch.are_deterministic_algorithms_enabled().  PP_ENOTSUP when the problem does not fit the form (more than 20480
// destinations per batch element, workspace too small): there is no deterministic substitute. ----
extern "C" int pp_gather_backward_ordered_f32(const float* grad_out, const int* idx, float* grad_points, int B,
                                              int C, int N, int M, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  return scatter_run(gather_desc(B, C, N, M).with(kAccumulate, true, workspace, workspace_bytes), grad_out, idx,
                     nullptr, grad_points, stream);
}
extern "C" int pp_group_points_grad_ordered_f32(const float* grad_out, const int* idx, float* grad_points, int B,
                                                int C, int N, int npoint, int nsample,
                                                long long grad_out_batch_stride, void* workspace,
                                                size_t workspace_bytes, void* stream) {
  return scatter_run(group_desc(B, C, N, npoint, nsample, grad_out_batch_stride)
                         .with(kAccumulate, true, workspace, workspace_bytes),
                     grad_out, idx, nullptr, grad_points, stream);
}
extern "C" int pp_three_interpolate_grad_ordered_f32(const float* grad_out, const int* idx, const float* weight,
                                                     float* grad_points, int B, int C, int N, int M,
                                                     void* workspace, size_t workspace_bytes, void* stream) {
  return scatter_run(interp_desc(B, C, N, M).with(kAccumulate, true, workspace, workspace_bytes), grad_out, idx,
                     weight, grad_points, stream);
}

// ---- 16-bit features: grad_points WRITTEN and rounded once; `ordered` is an argument; PP_ENOTSUP where no atomic-free
// form serves the shape (the caller widens and takes the fp32 entry) ----
#define PP_SCATTER_B16(SUFFIX, T)                                                                                     \
  extern "C" int pp_gather_backward_out_ws_##SUFFIX(const void* grad_out, const int* idx, void* grad_points, int B,  \
                                                    int C, int N, int M, void* workspace, size_t workspace_bytes,    \
                                                    int ordered, void* stream) {                                     \
    return scatter_run(gather_desc(B, C, N, M).with(kWrite, ordered != 0, workspace, workspace_bytes),               \
                       (const T*)grad_out, idx, nullptr, (T*)grad_points, stream);                                   \
  }                                                                                                                   \
  extern "C" int pp_group_points_grad_out_ws_##SUFFIX(const void* grad_out, const int* idx, void* grad_points, int B, \
                                                      int C, int N, int npoint, int nsample,                         \
                                                      long long grad_out_batch_stride, void* workspace,              \
                                                      size_t workspace_bytes, int ordered, void* stream) {           \
    return scatter_run(group_desc(B, C, N, npoint, nsample, grad_out_batch_stride)                                   \
                           .with(kWrite, ordered != 0, workspace, workspace_bytes),                                  \
                       (const T*)grad_out, idx, nullptr, (T*)grad_points, stream);                                   \
  }                                                                                                                   \
  extern "C" int pp_three_interpolate_grad_out_ws_##SUFFIX(const void* grad_out, const int* idx, const float* weight, \
                                                           void* grad_points, int B, int C, int N, int M,            \
                                                           void* workspace, size_t workspace_bytes, int ordered,     \
                                                           void* stream) {                                           \
    return scatter_run(interp_desc(B, C, N, M).with(kWrite, ordered != 0, workspace, workspace_bytes),               \
                       (const T*)grad_out, idx, weight, (T*)grad_points, stream);                                    \
  }
PP_SCATTER_B16(f16, pp::f16)
PP_SCATTER_B16(bf16, pp::bf16)
#undef PP_SCATTER_B16
