// mesh_winding.hip -- the winding number of a triangle mesh about every point of a cloud, alone or in the same walk as
// the exact point-to-mesh distance, by walking every (point, triangle) pair.  Contract in DESIGN.md "Mesh winding
// numbers and signed distance".
//
//   walk   mw_walk_kernel<kDistance>: pd_point_face_kernel's structure: one lane per point, a workgroup within one
//          batch element; the face records of pp_mesh_distance_records_f32 come through LDS in tiles of kMwFaceTile, in
//          ascending order; the record of a step is the same for every lane (an LDS broadcast), and a record whose
//          validity word is 0 is skipped by the whole workgroup.
//          kDistance = false: the half solid angle of every pair, from a, b, c of the record.
//          kDistance = true: the same, and then pd_pair on the same record, keeping (best, face, bary) under
//          mesh_distance.hip's choice: taken where d < best, so the lowest face among equal distances, never a NaN.
//
// mw_half_angle is Van Oosterom and Strackee's formula, every operation rounded on its own (the library is built with
// -ffp-contract=off): u = a - p, v = b - p, w = c - p, lu = sqrt(u.u), lv, lw likewise, x = v x w with each component
// two products and one difference, det = u.x, den = (((lu lv) lw + (u.v) lw) + (v.w) lu) + (w.u) lv, h = atan2f(det,
// den); every dot product is v3_dot_rounded.  Per point the halves are added in fp64 in ascending face order from +0
// and winding = (float)(sum / (2 pi)), rounded once.
//
// No atomics: every output word is written once and the bits are the same on every run.  The records hold no index, so
// nothing here is addressed by the data.
#include "mesh_common.h"   // pp::mesh_sizes_ok, V3 and v3_*; pp::blocks, pp::quiet_nan
#include "mesh_pair.h"     // pp::PdTri, PdPair, pd_pair, pd_unpack

namespace {

using namespace pp;

constexpr int kMwThreads = 256;
constexpr int kMwRecord = 16;       // floats of a face record of mesh_distance.hip: a, b, c, ab, ac, valid
constexpr int kMwFaceTile = 256;    // records in LDS: 16 KB
constexpr double kMwTwoPi = 6.283185307179586476925286766559;

// half the solid angle of triangle (a, b, c) seen from p, signed: positive where p sees the corners clockwise, which
// is from inside a mesh whose faces are oriented outwards
__device__ __forceinline__ float mw_half_angle(V3 p, V3 a, V3 b, V3 c) {
  const V3 u = v3_sub(a, p), v = v3_sub(b, p), w = v3_sub(c, p);
  const float lu = v3_len(u), lv = v3_len(v), lw = v3_len(w);
  const V3 x = {v.y * w.z - v.z * w.y, v.z * w.x - v.x * w.z, v.x * w.y - v.y * w.x};
  const float det = v3_dot_rounded(u, x);
  const float den = (((lu * lv) * lw + v3_dot_rounded(u, v) * lw) + v3_dot_rounded(v, w) * lu) + v3_dot_rounded(w, u) * lv;
  return atan2f(det, den);
}

template <bool kDistance>
__global__ __launch_bounds__(kMwThreads) void mw_walk_kernel(const float* __restrict__ points,
                                                             const float4* __restrict__ records,
                                                             float* __restrict__ dist, long long* __restrict__ face,
                                                             float* __restrict__ bary, float* __restrict__ winding,
                                                             int P, int F, int blocks_per_element) {
  __shared__ float4 s_rec[kMwFaceTile * (kMwRecord / 4)];
  const int t = threadIdx.x;
  const long long b = blockIdx.x / blocks_per_element;
  const long long i = (long long)(blockIdx.x - (unsigned)b * blocks_per_element) * kMwThreads + t;
  const bool live = i < P;
  V3 p = {0.0f, 0.0f, 0.0f};
  if (live) p = v3_load(points + (size_t)b * P * 3, i);
  const float4* __restrict__ rb = records + (size_t)b * F * (kMwRecord / 4);
  double sum = 0.0;
  float best = __builtin_inff();
  int arg = -1;
  float w0 = pp::quiet_nan(), w1 = w0, w2 = w0;
  for (int f0 = 0; f0 < F; f0 += kMwFaceTile) {
    const int n = F - f0 < kMwFaceTile ? F - f0 : kMwFaceTile;
    __syncthreads();   // the previous tile's readers are done
    for (int k = t; k < n * (kMwRecord / 4); k += kMwThreads) s_rec[k] = rb[(size_t)f0 * (kMwRecord / 4) + k];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const float4 q3 = s_rec[j * 4 + 3];
      if (q3.w == 0.0f) continue;   // (the whole workgroup) a face with a vertex index out of range
      const PdTri tri = pd_unpack(s_rec[j * 4], s_rec[j * 4 + 1], s_rec[j * 4 + 2], q3);
      sum += (double)mw_half_angle(p, tri.a, tri.b, tri.c);   // (before pd_pair: its operands are dead by then)
      if constexpr (kDistance) {
        const PdPair r = pd_pair(p, tri);
        if (r.d < best) {
          best = r.d;
          arg = f0 + j;
          w0 = r.w0, w1 = r.w1, w2 = r.w2;
        }
      }
    }
  }
  if (!live) return;
  const size_t x = (size_t)b * P + i;
  winding[x] = (float)(sum / kMwTwoPi);
  if constexpr (kDistance) {
    dist[x] = arg < 0 ? pp::quiet_nan() : best;
    face[x] = arg;
    v3_store(bary, x, {w0, w1, w2});
  }
}

template <bool kDistance>
int mw_launch(const float* points, const float* records, float* dist, long long* face, float* bary, float* winding,
              int B, int P, int F, void* stream) {
  if (!pp::mesh_sizes_ok(B, 0, F, P)) return PP_EINVAL;
  if (B == 0 || P == 0 || F == 0) return PP_OK;
  if (!points || !records || !winding || ((uintptr_t)records & 15u)) return PP_EINVAL;
  if (kDistance && (!dist || !face || !bary)) return PP_EINVAL;
  const int per_element = (int)pp::blocks(P, kMwThreads);
  if ((long long)B * per_element > 0x7fffffffLL) return PP_EINVAL;
  mw_walk_kernel<kDistance><<<dim3((unsigned)(B * per_element)), dim3(kMwThreads), 0, (hipStream_t)stream>>>(
      points, reinterpret_cast<const float4*>(records), dist, face, bary, winding, P, F, per_element);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

}  // namespace

extern "C" int pp_mesh_winding_forward_f32(const float* points, const float* records, float* winding, int B, int P,
                                           int F, void* stream) {
  return mw_launch<false>(points, records, nullptr, nullptr, nullptr, winding, B, P, F, stream);
}

extern "C" int pp_mesh_signed_distance_forward_f32(const float* points, const float* records, float* dist,
                                                   long long* face, float* bary, float* winding, int B, int P, int F,
                                                   void* stream) {
  return mw_launch<true>(points, records, dist, face, bary, winding, B, P, F, stream);
}
