// mesh_pair.h -- the (point, triangle) pair function of the every-pair mesh walks, shared by mesh_distance.hip and
// mesh_winding.hip: the face record's triangle, the closest point on it and the record's unpacking.
//
// pd_pair is the one pair function of the distances: Ericson's region walk with every operation rounded on its own, in
// the operation order of mesh_distance.distance_composition, which it equals to the bit.
#pragma once
#include "mesh_common.h"   // V3 and v3_*

namespace pp {

struct PdTri {
  V3 a, b, c, ab, ac;
};
struct PdPair {
  float d, w0, w1, w2;
};

// the closest point of triangle t to p as weights of (a, b, c), and the squared distance to it.  The regions are
// tried in the contract's order; each needs at most one division, so one is made, of the operands of the first
// region that holds among those that divide.
__device__ __forceinline__ PdPair pd_pair(V3 p, const PdTri& t) {
  const V3 ap = v3_sub(p, t.a), bp = v3_sub(p, t.b), cp = v3_sub(p, t.c);
  const float d1 = v3_dot_rounded(t.ab, ap), d2 = v3_dot_rounded(t.ac, ap);
  const float d3 = v3_dot_rounded(t.ab, bp), d4 = v3_dot_rounded(t.ac, bp);
  const float d5 = v3_dot_rounded(t.ab, cp), d6 = v3_dot_rounded(t.ac, cp);
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  const bool r1 = d1 <= 0.0f && d2 <= 0.0f;
  const bool r2 = d3 >= 0.0f && d4 <= d3;
  const bool r3 = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
  const bool r4 = d6 >= 0.0f && d5 <= d6;
  const bool r5 = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
  const bool r6 = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
  const float num = r3 ? d1 : r5 ? d2 : r6 ? e43 : 1.0f;
  const float den = r3 ? d1 - d3 : r5 ? d2 - d6 : r6 ? e43 + e56 : (va + vb) + vc;
  const float q = num / den;
  const float omq = 1.0f - q;
  const float v7 = vb * q, w7 = vc * q;
  const float u7 = (1.0f - v7) - w7;
  PdPair r;
  r.w0 = r1 ? 1.0f : r2 ? 0.0f : r3 ? omq : r4 ? 0.0f : r5 ? omq : r6 ? 0.0f : u7;
  r.w1 = r1 ? 0.0f : r2 ? 1.0f : r3 ? q : r4 ? 0.0f : r5 ? 0.0f : r6 ? omq : v7;
  r.w2 = r1 ? 0.0f : r2 ? 0.0f : r3 ? 0.0f : r4 ? 1.0f : r5 ? q : r6 ? q : w7;
  const V3 res = v3_sub(p, v3_weighted(r.w0, t.a, r.w1, t.b, r.w2, t.c));
  r.d = v3_dot_rounded(res, res);
  return r;
}

// the record as four float4 words, and back; w3.w is the validity word
__device__ __forceinline__ PdTri pd_unpack(float4 w0, float4 w1, float4 w2, float4 w3) {
  PdTri t;
  t.a = {w0.x, w0.y, w0.z};
  t.b = {w0.w, w1.x, w1.y};
  t.c = {w1.z, w1.w, w2.x};
  t.ab = {w2.y, w2.z, w2.w};
  t.ac = {w3.x, w3.y, w3.z};
  return t;
}

}  // namespace pp
