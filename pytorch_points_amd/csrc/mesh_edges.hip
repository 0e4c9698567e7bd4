// mesh_edges.hip -- the edge operators under the reference's mesh losses (network/model_loss.py:166-308,
// geo_operations.py:562-600): MeshEdgeLengthLoss, MeshStretchLoss and SimpleMeshRepulsionLoss all work on the squared
// lengths of a triangle mesh's unique edges.  The reference finds those edges per batch element with torch.unique (a
// host synchronisation each), gathers an (E,2,3) tensor per mesh, and scatters back with floating-point atomics.
//
// Here the topology is built ONCE and kept (a mesh's connectivity does not change between training steps):
//   unique edges   faces (Bt,F,3) -> edges (Bt,3F,2): the unordered vertex pairs as (min,max), ascending
//                  lexicographically, rows from count[b] on (-1,-1); row for row what torch.unique(dim=0) of the sorted
//                  half-edges returns.  Half-edges are bucketed by their min-vertex and every bucket is SORTED by
//                  max-vertex (bucket_lists.h's chain), the first entry of every run of equal pairs is ranked by a
//                  second scan and written compacted.  The sort makes the result independent of the order in which
//                  the atomics were served.
//   incidence      edges (Bt,Ecap,2), counts -> for every vertex the list of 2*e + side over the edges e < count[b]
//                  with edges[e,side] == v, ascending (the same chain).  The edge list may be any list: not unique,
//                  not sorted, with self-edges.  The same build with four columns (4*e + slot) serves the edge
//                  points of mesh_dihedral.hip.
// and a training step is two launches:
//   forward        out[b,e] = |v[b,edges[e,0]] - v[b,edges[e,1]]|^2 (pp::chamfer_d3: the bits of knn_edge_lengths'
//                  squared form), one thread per edge; 0 for the padding rows
//   backward       a GATHER, one thread per vertex: grad starts at 0 and walks the vertex's incidence list in order,
//                  t_e = (2 g[b,e]) * (v_a - v_b), side 0 adds t_e, side 1 subtracts it.  Plain fp32 sums in ascending
//                  (e, side): the bits of the sequential loop `for e: grad[a] += t_e; grad[b] -= t_e`, on every run.
//                  No floating-point atomics; there is no second form.
// A topology with one batch element is shared by a batch of vertex sets (topology batch stride 0).
//
// An index outside [0, n_vertices) is never used as an address: the builds only compare it, skip what it belongs to and
// set the batch element's flag word (the host raises); the forward writes NaN for such an edge and the backward adds NaN.
//
// The mesh Laplacians (geo_operations.py:155-346: UniformLaplacian, CotLaplacian, cotangent) stand on the same chain:
//   corner incidence   faces (Bt,F,L) -> for every vertex the list of L*f + c over the corners with faces[f,c] == v,
//                      ascending, and beside every slot its corner's (next, prev) vertices as int32
//   cotangent          one thread per face, the reference's operation order in fp32
//   apply              one thread per (b, vertex): a gather over the vertex's slice from +0 in slot order, plain fp32
//                      operations; the uniform operator's forward and backward and the cotangent operator (whose
//                      backward is the same call on the gradient) are three modes of one kernel
#include "mesh_common.h"   // pp::mesh_half_edge, mesh_build_ok, mesh_face, mesh_row, V3 and v3_*; bucket_lists.h

namespace {

using namespace pp;   // mesh_common.h's rows and three-vectors

constexpr int kMeThreads = 256;
constexpr int kMeScanThreads = pp::kBucketScanThreads;   // me_compact_kernel ranks with the chain's block scan

// ---- buckets ------------------------------------------------------------------------------------------------------
// Half-edge j of face f joins corners j and (j+1) mod 3.  FILL = false: bucket sizes by min-vertex; FILL = true: the
// buckets receive the max-vertices (and every position its bucket).  A half-edge with an index outside [0, N) is only
// compared: it sets its batch element's flag and takes no part.
template <bool FILL>
__global__ __launch_bounds__(kMeThreads) void me_half_edges_kernel(const long long* __restrict__ faces,
                                                                   unsigned* __restrict__ cursor,
                                                                   unsigned* __restrict__ entries,
                                                                   unsigned* __restrict__ owner,
                                                                   int* __restrict__ flags, long long total, int F,
                                                                   int N) {
  const long long h = (long long)blockIdx.x * kMeThreads + threadIdx.x;
  if (h >= total) return;
  const pp::MeshHalfEdge e = pp::mesh_half_edge(faces, h, F, N);
  if (!e.in_range) {
    if (!FILL) atomicOr(flags + e.b, 1);
    return;
  }
  const size_t slot = pp::bucket_put<FILL>(cursor, entries, e.b, N, 3LL * F, (unsigned)e.mn, (unsigned)e.mx);
  if (FILL) owner[slot] = (unsigned)e.mn;
}

// One thread per edge end (b, e, side), e < counts[b], of a table of COLS columns: 2 for an edge list, 4 for the edge
// points of mesh_dihedral.hip, 1 for the corners of faces (Bt,F,L) taken as L*F rows.  Without counts (a null pointer,
// the same for every thread) all rows count.  FILL = false: the vertices' degrees; FILL = true: the lists receive
// COLS*e + side.  An end outside [0, N) sets the flag and takes no part.
template <bool FILL, int COLS>
__global__ __launch_bounds__(kMeThreads) void me_edge_ends_kernel(const long long* __restrict__ edges,
                                                                  const int* __restrict__ counts,
                                                                  unsigned* __restrict__ cursor,
                                                                  unsigned* __restrict__ entries,
                                                                  int* __restrict__ flags, long long total, int Ecap,
                                                                  int N) {
  const long long x = (long long)blockIdx.x * kMeThreads + threadIdx.x;
  if (x >= total) return;
  const long long X = (long long)COLS * Ecap;
  const long long b = x / X;
  const unsigned code = (unsigned)(x - b * X);   // COLS*e + side
  if (counts != nullptr && (int)(code / (unsigned)COLS) >= counts[b]) return;
  const long long v = edges[x];
  if (v < 0 || v >= N) {
    if (!FILL) atomicOr(flags + b, 1);
    return;
  }
  pp::bucket_put<FILL>(cursor, entries, b, N, X, (size_t)v, code);
}

// one workgroup per batch element over its sorted (owner, entry) pairs: a position that differs from the one before it
// starts a run; the runs are ranked by a scan and written compacted, then the rows behind them are padded with -1
__global__ __launch_bounds__(kMeScanThreads) void me_compact_kernel(const unsigned* __restrict__ cursor,
                                                                    const unsigned* __restrict__ entries,
                                                                    const unsigned* __restrict__ owner,
                                                                    long long* __restrict__ edges,
                                                                    int* __restrict__ counts, int N, int F) {
  __shared__ unsigned s_wave[kMeScanThreads / 64];
  const int t = threadIdx.x;
  const size_t H = 3 * (size_t)F;
  const unsigned* __restrict__ ent = entries + (size_t)blockIdx.x * H;
  const unsigned* __restrict__ own = owner + (size_t)blockIdx.x * H;
  long long* __restrict__ out = edges + (size_t)blockIdx.x * H * 2;
  const unsigned T = N > 0 ? cursor[(size_t)blockIdx.x * N + (N - 1)] : 0u;   // the last bucket's end: valid half-edges
  unsigned carry = 0;
  for (unsigned q0 = 0; q0 < T; q0 += kMeScanThreads) {
    const unsigned q = q0 + t;
    unsigned first = 0, mn = 0, mx = 0;
    if (q < T) {
      mn = own[q];
      mx = ent[q];
      first = (q == 0 || own[q - 1] != mn || ent[q - 1] != mx) ? 1u : 0u;
    }
    unsigned chunk;
    const unsigned rank = pp::bucket_block_scan(first, carry, s_wave, &chunk);
    if (first) {
      out[2 * (size_t)rank] = (long long)mn;
      out[2 * (size_t)rank + 1] = (long long)mx;
    }
    carry += chunk;
  }
  if (t == 0) counts[blockIdx.x] = (int)carry;
  for (size_t w = 2 * (size_t)carry + t; w < 2 * H; w += kMeScanThreads) out[w] = -1;
}

// ---- the step -----------------------------------------------------------------------------------------------------
// one thread per edge
__global__ __launch_bounds__(kMeThreads) void me_sqrlen_forward_kernel(const float* __restrict__ vertices,
                                                                       const long long* __restrict__ edges,
                                                                       const int* __restrict__ counts,
                                                                       float* __restrict__ out, long long total, int N,
                                                                       int Ecap, int shared) {
  const long long x = (long long)blockIdx.x * kMeThreads + threadIdx.x;
  if (x >= total) return;
  const long long b = x / Ecap;
  const long long e = x - b * Ecap;
  const long long tb = shared ? 0 : b;
  if (e >= counts[tb]) {
    out[x] = 0.0f;
    return;
  }
  const long long a = edges[(tb * Ecap + e) * 2], c = edges[(tb * Ecap + e) * 2 + 1];
  if (a < 0 || a >= N || c < 0 || c >= N) {
    out[x] = pp::quiet_nan();
    return;
  }
  const float* __restrict__ pa = vertices + ((size_t)b * N + (size_t)a) * 3;
  const float* __restrict__ pc = vertices + ((size_t)b * N + (size_t)c) * 3;
  out[x] = pp::chamfer_d3(pa[0], pa[1], pa[2], pc[0], pc[1], pc[2]);
}

// one thread per vertex; the incidence list in order, however long it is
__global__ __launch_bounds__(kMeThreads) void me_sqrlen_backward_kernel(
    const float* __restrict__ vertices, const long long* __restrict__ edges, const int* __restrict__ inc_start,
    const unsigned* __restrict__ inc_entries, const float* __restrict__ g, float* __restrict__ grad, long long rows,
    int N, int Ecap, int shared) {
  const long long i = (long long)blockIdx.x * kMeThreads + threadIdx.x;
  if (i >= rows) return;
  const MeshRow w = mesh_row(i, N, shared);
  const float* __restrict__ vb = vertices + (size_t)w.b * N * 3;
  const long long* __restrict__ eb = edges + (size_t)w.tb * Ecap * 2;
  const unsigned* __restrict__ list = inc_entries + (size_t)w.tb * Ecap * 2;
  const float* __restrict__ gb = g + (size_t)w.b * Ecap;
  const int* __restrict__ st = inc_start + (size_t)w.tb * ((size_t)N + 1) + w.i;   // (read as it is, not clipped)
  const V3 p = v3_load(vb, w.i);
  V3 acc = {0.0f, 0.0f, 0.0f};
  for (int q = st[0], q1 = st[1]; q < q1; ++q) {
    const unsigned code = list[q];
    const unsigned e = code >> 1, side = code & 1u;
    const long long o = eb[2 * (size_t)e + (side ^ 1u)];   // the other end; this end is v
    const float coef = 2.0f * gb[e];
    V3 t = v3_nan();
    if (!(o < 0 || o >= N)) {
      const V3 po = v3_load(vb, o);
      t = v3_scale(coef, side ? v3_sub(po, p) : v3_sub(p, po));   // v_a - v_b, a = edges[e,0], b = edges[e,1]
    }
    acc = side ? v3_sub(acc, t) : v3_add(acc, t);
  }
  v3_store(grad, i, acc);
}

// ---- corners ------------------------------------------------------------------------------------------------------
// (their lists are me_edge_ends_kernel's with one column)
// One thread per slot of the sorted lists: (next, prev) of the slot's corner, -1 for a vertex outside [0, N), so that
// the apply reads its neighbours beside each other and never follows a 64-bit face row
__global__ __launch_bounds__(kMeThreads) void me_corner_nbr_kernel(const long long* __restrict__ faces,
                                                                   const int* __restrict__ start,
                                                                   const unsigned* __restrict__ codes,
                                                                   int* __restrict__ nbr, long long total, long long X,
                                                                   int L, int N) {
  const long long x = (long long)blockIdx.x * kMeThreads + threadIdx.x;
  if (x >= total) return;
  const long long b = x / X;
  const long long q = x - b * X;
  if (q >= start[b * ((long long)N + 1) + N]) return;   // behind the last slice (corners that were out of range)
  const unsigned code = codes[x];
  if ((long long)code >= X) return;
  const unsigned f = code / (unsigned)L, c = code - f * (unsigned)L;
  const long long* __restrict__ row = faces + b * X + (long long)f * L;
  const long long nx = row[c + 1 == (unsigned)L ? 0 : c + 1], pv = row[c == 0 ? L - 1 : c - 1];
  nbr[2 * x] = (nx < 0 || nx >= N) ? -1 : (int)nx;
  nbr[2 * x + 1] = (pv < 0 || pv >= N) ? -1 : (int)pv;
}

// ---- cotangent ----------------------------------------------------------------------------------------------------
// One thread per face: geo_operations.py:306-346 step for step (the build does not contract a*b + c).  A face with an
// index outside [0, N) writes NaN and reads nothing.
__global__ __launch_bounds__(kMeThreads) void me_cotangent_kernel(const float* __restrict__ vertices,
                                                                  const long long* __restrict__ faces,
                                                                  float* __restrict__ out, long long total, int N,
                                                                  int F, int shared) {
  const long long x = (long long)blockIdx.x * kMeThreads + threadIdx.x;
  if (x >= total) return;
  const long long b = x / F;
  const MeshFace t = mesh_face(faces, b, x - b * F, F, N, shared);
  if (!t.in_range) {
    v3_store(out, x, v3_nan());
    return;
  }
  const float* __restrict__ vb = vertices + (size_t)b * N * 3;
  const V3 p1 = v3_load(vb, t.i0), p2 = v3_load(vb, t.i1), p3 = v3_load(vb, t.i2);
  // v3_len: sqrtf((dx*dx + dy*dy) + dz*dz), correctly rounded in this build
  const float l1 = v3_len(v3_sub(p2, p3)), l2 = v3_len(v3_sub(p3, p1)), l3 = v3_len(v3_sub(p1, p2));
  const float sp = ((l1 + l2) + l3) * 0.5f;
  float inside = ((sp * (sp - l1)) * (sp - l2)) * (sp - l3);
  if (inside < 0.0f) inside = 0.0f;
  const float A = 2.0f * sqrtf(inside);
  if (A == 0.0f) {
    v3_store(out, x, v3_zero());
    return;
  }
  const float s1 = l1 * l1, s2 = l2 * l2, s3 = l3 * l3, den = A + 1e-10f;
  const V3 w = {(((s2 + s3) - s1) / den) / 4.0f, (((s1 + s3) - s2) / den) / 4.0f, (((s1 + s2) - s3) / den) / 4.0f};
  v3_store(out, x, w);
}

// ---- the Laplacian apply ------------------------------------------------------------------------------------------
// One thread per (b, vertex i), its slice in ascending slot order, acc from +0, every operation rounded as written.
//   MODE 0  uniform forward    acc += (x_i - x_next); acc += (x_i - x_prev);  out = acc / ((float)(2n) + 1e-12f)
//   MODE 1  uniform backward   the same sum over h_k = g_k / ((float)(2 n_k) + 1e-12f), not divided again.
//           The forward is out = D^-1 M x with D = diag(2n + 1e-12) and (M x)_i = sum over the slots at i of
//           (x_i - x_next) + (x_i - x_prev), so M = diag(2n) - W with W_ij = h(i,j) + h(j,i), h(p,q) the number of
//           half-edges p -> q (a slot at i with prev == j is a half-edge j -> i).  W, hence M, is symmetric, and
//           grad = (D^-1 M)^T g = M (D^-1 g) = M h: the forward's gather over h.  n_k is the length of k's own slice.
//   MODE 2  cotangent          slot code 3f + c: acc += W[b,f,(c+2)%3] * (x_next - x_i); acc += W[b,f,(c+1)%3] *
//           (x_prev - x_i).  L is symmetric and constant: the backward is this mode on the gradient.
// A neighbour outside [0, N) (the build stored -1) is not read: NaN is added.
template <int MODE>
__global__ __launch_bounds__(kMeThreads) void me_laplacian_apply_kernel(
    const float* __restrict__ x, const int* __restrict__ start, const int* __restrict__ nbr,
    const unsigned* __restrict__ codes, const float* __restrict__ weights, float* __restrict__ out, long long rows,
    int N, int F, long long X, int shared) {
  const long long r = (long long)blockIdx.x * kMeThreads + threadIdx.x;
  if (r >= rows) return;
  const MeshRow row = mesh_row(r, N, shared);
  const long long i = row.i;
  const float* __restrict__ xb = x + (size_t)row.b * N * 3;
  const int* __restrict__ st = start + (size_t)row.tb * ((size_t)N + 1);
  const int2* __restrict__ nb = reinterpret_cast<const int2*>(nbr) + (size_t)row.tb * (size_t)X;
  const unsigned* __restrict__ cd = codes + (size_t)row.tb * (size_t)X;
  const float* __restrict__ wb = weights + (size_t)row.b * F * 3;
  const int q0 = st[i], q1 = st[i + 1];   // (read as they are, not clipped)
  float px = xb[i * 3], py = xb[i * 3 + 1], pz = xb[i * 3 + 2];
  if (MODE == 1) {
    const float d = (float)(2 * (q1 - q0)) + 1e-12f;
    px = px / d;
    py = py / d;
    pz = pz / d;
  }
  float ax = 0.0f, ay = 0.0f, az = 0.0f;
  for (int q = q0; q < q1; ++q) {
    const int2 jk = nb[q];
    float w[2] = {1.0f, 1.0f};
    if (MODE == 2) {
      const unsigned code = cd[q];
      const unsigned f = code / 3u, c = code - f * 3u;
      if (f < (unsigned)F) {
        w[0] = wb[(size_t)f * 3 + (c == 0 ? 2 : c - 1)];   // (c + 2) % 3
        w[1] = wb[(size_t)f * 3 + (c == 2 ? 0 : c + 1)];   // (c + 1) % 3
      } else {
        w[0] = w[1] = quiet_nan();
      }
    }
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int j = side ? jk.y : jk.x;
      float ox, oy, oz;
      if (j < 0 || j >= N) {
        ox = oy = oz = quiet_nan();
      } else {
        ox = xb[(size_t)j * 3];
        oy = xb[(size_t)j * 3 + 1];
        oz = xb[(size_t)j * 3 + 2];
        if (MODE == 1) {
          const float d = (float)(2 * (st[j + 1] - st[j])) + 1e-12f;
          ox = ox / d;
          oy = oy / d;
          oz = oz / d;
        }
      }
      if (MODE == 2) {
        ax = ax + w[side] * (ox - px);
        ay = ay + w[side] * (oy - py);
        az = az + w[side] * (oz - pz);
      } else {
        ax = ax + (px - ox);
        ay = ay + (py - oy);
        az = az + (pz - oz);
      }
    }
  }
  if (MODE == 0) {
    const float d = (float)(2 * (q1 - q0)) + 1e-12f;
    ax = ax / d;
    ay = ay / d;
    az = az / d;
  }
  v3_store(out, r, {ax, ay, az});
}

// ---- host ---------------------------------------------------------------------------------------------------------
}  // namespace

extern "C" size_t pp_mesh_edges_workspace_bytes(int Bt, int n_vertices, long long items) {
  if (Bt <= 0 || n_vertices <= 0 || items <= 0 || !pp::mesh_build_ok(Bt, n_vertices, items, false)) return 0;
  return pp::bucket_layout(Bt, n_vertices, items, true).total;
}

extern "C" int pp_mesh_unique_edges(const long long* faces, long long* edges, int* counts, int* flags, int Bt, int F,
                                    int n_vertices, void* workspace, size_t workspace_bytes, void* stream) {
  const long long H = 3LL * (F > 0 ? F : 0);
  const int N = n_vertices;
  if (F < 0 || !pp::mesh_build_ok(Bt, N, H, false)) return PP_EINVAL;
  if (Bt == 0) return PP_OK;
  if (!counts || !flags) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = pp::fill_bytes(flags, 0, 4 * (size_t)Bt, s);
  if (e != hipSuccess) return (int)e;
  if (F == 0 || N == 0) {   // no face, or no vertex a face could name: no edges (a face of an empty mesh is flagged)
    e = pp::fill_bytes(counts, 0, 4 * (size_t)Bt, s);
    if (e != hipSuccess) return (int)e;
    if (F == 0) return PP_OK;
    if (!edges) return PP_EINVAL;
    e = pp::fill_bytes(edges, 0xff, (size_t)Bt * H * 16, s);
    if (e != hipSuccess) return (int)e;
    return (int)pp::fill_bytes(flags, 1, 4 * (size_t)Bt, s);   // (any non-zero word)
  }
  const pp::BucketLayout L = pp::bucket_layout(Bt, N, H, true);
  unsigned char* ws = (unsigned char*)workspace;
  if (!faces || !edges || !ws || workspace_bytes < L.total) return PP_EINVAL;
  unsigned* cursor = reinterpret_cast<unsigned*>(ws + L.cursor);
  unsigned* entries = reinterpret_cast<unsigned*>(ws + L.entries);
  unsigned* owner = reinterpret_cast<unsigned*>(ws + L.owner);
  const long long total = (long long)Bt * H;
  const int rc = pp::bucket_build(ws, L, entries, nullptr, Bt, N, H, true, s, [&](bool fill) {
    const dim3 grid(pp::blocks(total, kMeThreads)), block(kMeThreads);
    if (fill)
      me_half_edges_kernel<true><<<grid, block, 0, s>>>(faces, cursor, entries, owner, flags, total, F, N);
    else
      me_half_edges_kernel<false><<<grid, block, 0, s>>>(faces, cursor, entries, owner, flags, total, F, N);
  });
  if (rc != PP_OK) return rc;
  me_compact_kernel<<<dim3((unsigned)Bt), dim3(kMeScanThreads), 0, s>>>(cursor, entries, owner, edges, counts, N, F);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

namespace {
// the vertex lists of a table (Bt,Ecap,COLS): pp_mesh_edge_incidence, pp_mesh_edge_points_incidence and, with one
// column and no counts, pp_mesh_corner_incidence
template <int COLS>
int me_incidence(const long long* edges, const int* counts, int* inc_start, unsigned* inc_entries, int* flags, int Bt,
                 int Ecap, int N, void* workspace, size_t workspace_bytes, void* stream) {
  const long long X = (long long)COLS * (Ecap > 0 ? Ecap : 0);
  if (Ecap < 0 || !pp::mesh_build_ok(Bt, N, X, true)) return PP_EINVAL;
  if (Bt == 0) return PP_OK;
  if (!inc_start) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (Ecap == 0 || N == 0) {   // no list has an entry
    const hipError_t e = pp::fill_bytes(inc_start, 0, 4 * (size_t)Bt * ((size_t)N + 1), s);
    if (e != hipSuccess) return (int)e;
    if (Ecap == 0) return PP_OK;
  }
  if (!edges || (!counts && COLS != 1) || !flags) return PP_EINVAL;
  const long long total = (long long)Bt * X;
  if (N == 0) {   // every end of every counted edge is out of range: the count pass only compares and flags
    me_edge_ends_kernel<false, COLS><<<dim3(pp::blocks(total, kMeThreads)), dim3(kMeThreads), 0, s>>>(
        edges, counts, nullptr, nullptr, flags, total, Ecap, N);
    PP_RETURN_IF_LAUNCH_FAILED();
    return PP_OK;
  }
  const pp::BucketLayout L = pp::bucket_layout(Bt, N, X, false);
  unsigned char* ws = (unsigned char*)workspace;
  if (!inc_entries || !ws || workspace_bytes < L.entries) return PP_EINVAL;   // the lists are built in place
  unsigned* cursor = reinterpret_cast<unsigned*>(ws + L.cursor);
  return pp::bucket_build(ws, L, inc_entries, inc_start, Bt, N, X, true, s, [&](bool fill) {
    const dim3 grid(pp::blocks(total, kMeThreads)), block(kMeThreads);
    if (fill)
      me_edge_ends_kernel<true, COLS><<<grid, block, 0, s>>>(edges, counts, cursor, inc_entries, flags, total, Ecap, N);
    else
      me_edge_ends_kernel<false, COLS><<<grid, block, 0, s>>>(edges, counts, cursor, inc_entries, flags, total, Ecap, N);
  });
}
}  // namespace

extern "C" int pp_mesh_edge_incidence(const long long* edges, const int* counts, int* inc_start, unsigned* inc_entries,
                                      int* flags, int Bt, int Ecap, int n_vertices, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return me_incidence<2>(edges, counts, inc_start, inc_entries, flags, Bt, Ecap, n_vertices, workspace, workspace_bytes,
                         stream);
}

// the (E,4) edge points of mesh_dihedral.hip: vertex v's list holds 4*e + slot
extern "C" int pp_mesh_edge_points_incidence(const long long* edge_points, const int* counts, int* start,
                                             unsigned* entries, int* flags, int Bt, int Ecap, int n_vertices,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  return me_incidence<4>(edge_points, counts, start, entries, flags, Bt, Ecap, n_vertices, workspace, workspace_bytes,
                         stream);
}

extern "C" int pp_mesh_edge_sqrlen_forward_f32(const float* vertices, const long long* edges, const int* counts,
                                               float* out, int B, int N, int Ecap, int shared_topology, void* stream) {
  if (B < 0 || N < 0 || Ecap < 0 || (long long)B * Ecap > 0x7fffffffLL * (long long)kMeThreads ||
      (long long)B * N > 0x7fffffffLL)
    return PP_EINVAL;
  if (B == 0 || Ecap == 0) return PP_OK;
  if (!edges || !counts || !out || (N > 0 && !vertices)) return PP_EINVAL;
  const long long total = (long long)B * Ecap;
  me_sqrlen_forward_kernel<<<dim3(pp::blocks(total, kMeThreads)), dim3(kMeThreads), 0, (hipStream_t)stream>>>(
      vertices, edges, counts, out, total, N, Ecap, shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_edge_sqrlen_backward_f32(const float* vertices, const long long* edges, const int* inc_start,
                                                const unsigned* inc_entries, const float* grad_out,
                                                float* grad_vertices, int B, int N, int Ecap, int shared_topology,
                                                void* stream) {
  if (B < 0 || N < 0 || Ecap < 0 || (long long)B * N > 0x7fffffffLL || 2LL * Ecap > 0x7fffffffLL) return PP_EINVAL;
  if (B == 0 || N == 0) return PP_OK;
  if (!vertices || !inc_start || !grad_vertices || (Ecap > 0 && (!edges || !inc_entries || !grad_out))) return PP_EINVAL;
  const long long rows = (long long)B * N;
  me_sqrlen_backward_kernel<<<dim3(pp::blocks(rows, kMeThreads)), dim3(kMeThreads), 0, (hipStream_t)stream>>>(
      vertices, edges, inc_start, inc_entries, grad_out, grad_vertices, rows, N, Ecap, shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

// the corners (b, f, c) of faces (Bt,F,L) are the L*F rows of a one-column table: vertex v's list holds L*f + c
extern "C" int pp_mesh_corner_incidence(const long long* faces, int* start, unsigned* codes, int* nbr, int* flags,
                                        int Bt, int F, int L, int n_vertices, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  const int N = n_vertices;
  const long long X = (long long)L * F;
  if (F < 0 || L < 3 || !pp::mesh_build_ok(Bt, N, X, true)) return PP_EINVAL;
  if (Bt == 0) return PP_OK;
  const bool listed = F > 0 && N > 0;   // else no list has an entry (a corner of a mesh without vertices is flagged)
  if (!start || !flags || (listed && !nbr)) return PP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = pp::fill_bytes(flags, 0, 4 * (size_t)Bt, s);
  if (e != hipSuccess) return (int)e;
  const int rc = me_incidence<1>(faces, nullptr, start, codes, flags, Bt, (int)X, N, workspace, workspace_bytes,
                                 stream);
  if (rc != PP_OK || !listed) return rc;
  const long long total = (long long)Bt * X;
  me_corner_nbr_kernel<<<dim3(pp::blocks(total, kMeThreads)), dim3(kMeThreads), 0, s>>>(faces, start, codes, nbr, total,
                                                                                        X, L, N);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_cotangent_f32(const float* vertices, const long long* faces, float* out, int B, int N, int F,
                                     int shared_topology, void* stream) {
  if (B < 0 || N < 0 || F < 0 || (long long)B * F > 0x7fffffffLL || (long long)B * N > 0x7fffffffLL) return PP_EINVAL;
  if (B == 0 || F == 0) return PP_OK;
  if (!faces || !out || (N > 0 && !vertices)) return PP_EINVAL;
  const long long total = (long long)B * F;
  me_cotangent_kernel<<<dim3(pp::blocks(total, kMeThreads)), dim3(kMeThreads), 0, (hipStream_t)stream>>>(
      vertices, faces, out, total, N, F, shared_topology != 0);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}

extern "C" int pp_mesh_laplacian_apply_f32(const float* x, const int* start, const int* nbr, const unsigned* codes,
                                           const float* weights, float* out, int B, int N, int F, int L, int mode,
                                           int shared_topology, void* stream) {
  if (B < 0 || N < 0 || F < 0 || L < 3 || mode < 0 || mode > 2 || (mode == 2 && L != 3)) return PP_EINVAL;
  const long long X = (long long)L * F;
  if ((long long)B * N > 0x7fffffffLL || X > 0x7fffffffLL) return PP_EINVAL;
  if (B == 0 || N == 0) return PP_OK;
  if (!x || !start || !out || (F > 0 && (!nbr || !codes || (mode == 2 && !weights)))) return PP_EINVAL;
  const long long rows = (long long)B * N;
  const dim3 grid(pp::blocks(rows, kMeThreads)), block(kMeThreads);
  hipStream_t s = (hipStream_t)stream;
  const int sh = shared_topology != 0;
  if (mode == 0)
    me_laplacian_apply_kernel<0><<<grid, block, 0, s>>>(x, start, nbr, codes, weights, out, rows, N, F, X, sh);
  else if (mode == 1)
    me_laplacian_apply_kernel<1><<<grid, block, 0, s>>>(x, start, nbr, codes, weights, out, rows, N, F, X, sh);
  else
    me_laplacian_apply_kernel<2><<<grid, block, 0, s>>>(x, start, nbr, codes, weights, out, rows, N, F, X, sh);
  PP_RETURN_IF_LAUNCH_FAILED();
  return PP_OK;
}
