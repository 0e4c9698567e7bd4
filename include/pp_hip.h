/*
 * pp_hip.h -- C ABI of libpp_hip.so, the MI355X (gfx950) implementation of the pytorch_points
 * `_ext` hot path.
 *
 * Each entry point replaces one function of the reference's pybind modules
 * `pytorch_points._ext.losses` (_ext/nmdistance.cpp:30-34), `pytorch_points._ext.sampling`
 * (_ext/sampling.cpp:205-216) and `pytorch_points._ext.linalg` (_ext/torch_batch_svd.cpp:240-245); the reference interface each one stands in for is cited beside it
 * (paths relative to /root/reference/pytorch_points/).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous memory; fp32 data, int32 indices;
 *   - the caller allocates every output and every workspace; nothing is allocated, retained or
 *     synchronised inside the library.  Thread-safe: the only process-wide state is a set of atomic
 *     test / benchmark knobs, declared separately in pp_hip_debug.h and never set by product code,
 *     and idempotent per-device "LDS limit raised" flags;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); all work is
 *     enqueued on it, on the device that is current when the call is made;
 *   - return value: 0 on success, otherwise a hipError_t value (PP_EINVAL = hipErrorInvalidValue
 *     for bad sizes / null pointers).  Never exit()s, never prints.
 *   - NaN coordinates are outside the contract (the reference's behaviour for them is an
 *     artefact of its 512-point chunking).
 */
#ifndef PP_HIP_H
#define PP_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_OK 0
#define PP_EINVAL 1    /* == hipErrorInvalidValue */
#define PP_ENOTSUP 801 /* == hipErrorNotSupported: an *_ordered_* entry point cannot serve this shape */

/* library / build identification: "pp_hip <version> gfx950" */
const char* pp_version(void);

/* ---- _ext.losses ------------------------------------------------------------------------- */

/* Replaces losses.nmdistance_forward(xyz1,xyz2,dist1,dist2,idx1,idx2)
 *   (_ext/nmdistance.cpp:13-15 -> chamfer_cuda_forward, _ext/nmdistance_cuda.cu:118-140).
 * xyz1 (B,N,C), xyz2 (B,M,C) -> dist1,idx1 (B,N): nearest xyz2 point of every xyz1 point
 * (squared distance, lowest index on exact ties); dist2,idx2 (B,M): the converse.
 * N == 0 or M == 0: outputs are zero-filled (what the reference's Python wrapper leaves). */
int pp_nmdistance_forward_f32(const float* xyz1, const float* xyz2, float* dist1, int* idx1,
                              float* dist2, int* idx2, int B, int N, int M, int C, void* stream);

/* The same operation with a caller-provided scratch buffer.  With a workspace of at least
 * pp_nmdistance_forward_workspace_bytes(...) bytes (0 = not applicable to these sizes) the search
 * is an exact uniform-grid search with the brute force as its fallback -- bit-identical outputs,
 * far fewer distance evaluations; with workspace == NULL it is pp_nmdistance_forward_f32. */
size_t pp_nmdistance_forward_workspace_bytes(int B, int N, int M, int C);
int pp_nmdistance_forward_ws_f32(const float* xyz1, const float* xyz2, float* dist1, int* idx1,
                                 float* dist2, int* idx2, int B, int N, int M, int C,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Replaces losses.labeled_nmdistance_forward(xyz1,xyz2,label1,label2,dist1,dist2,idx1,idx2)
 *   (_ext/nmdistance.cpp:17-20 -> labeled_chamfer_cuda_forward, _ext/nmdistance_cuda.cu:142-166).
 * label1 (B,N), label2 (B,M) as fp32.  Unmatched query: idx -1, dist 0. */
int pp_labeled_nmdistance_forward_f32(const float* xyz1, const float* xyz2, const float* label1,
                                      const float* label2, float* dist1, int* idx1, float* dist2,
                                      int* idx2, int B, int N, int M, int C, void* stream);

/* The labeled forward through the exact uniform-grid search (same outputs; see
 * pp_nmdistance_forward_ws_f32).  The workspace is larger than the unlabeled one (the labels are
 * carried in sorted order); 0 bytes = not applicable, null / too small workspace = the call above. */
size_t pp_labeled_nmdistance_forward_workspace_bytes(int B, int N, int M, int C);
int pp_labeled_nmdistance_forward_ws_f32(const float* xyz1, const float* xyz2, const float* label1,
                                         const float* label2, float* dist1, int* idx1, float* dist2,
                                         int* idx2, int B, int N, int M, int C, void* workspace,
                                         size_t workspace_bytes, void* stream);

/* Replaces losses.nmdistance_backward(xyz1,xyz2,gradxyz1,gradxyz2,graddist1,graddist2,idx1,idx2)
 *   (_ext/nmdistance.cpp:23-27 -> chamfer_cuda_backward, _ext/nmdistance_cuda.cu:195-221).
 * gradxyz1 (B,N,C), gradxyz2 (B,M,C) are fully overwritten (the reference zeroes them first). */
int pp_nmdistance_backward_f32(const float* xyz1, const float* xyz2, const float* graddist1,
                               const float* graddist2, const int* idx1, const int* idx2,
                               float* gradxyz1, float* gradxyz2, int B, int N, int M, int C,
                               void* stream);

/* The same two operators for double clouds: the reference dispatches its kernels over the floating types
 * (AT_DISPATCH_FLOATING_TYPES_AND_HALF, _ext/nmdistance_cuda.cu:125,210), scalar_t = double for coordinates,
 * distances and gradients, int indices.  Every-pair scan (no workspace form); same tie rule and rounding order
 * as the reference's kernel instantiated for double. */
int pp_nmdistance_forward_f64(const double* xyz1, const double* xyz2, double* dist1, int* idx1,
                              double* dist2, int* idx2, int B, int N, int M, int C, void* stream);
int pp_nmdistance_backward_f64(const double* xyz1, const double* xyz2, const double* graddist1,
                               const double* graddist2, const int* idx1, const int* idx2,
                               double* gradxyz1, double* gradxyz2, int B, int N, int M, int C,
                               void* stream);
/* ... and for half clouds (scalar_t = at::Half, the third type of that dispatch): coordinates, distances and gradients
 * are IEEE binary16 words (torch.float16; opaque pointers here), every subtraction, product and sum rounded to half
 * separately as c10::Half's operators do (no fused operation), comparisons in half; the scattered gradient terms are
 * added with packed half atomics, each addition rounded, in arrival order (the reference: a CAS loop on at::Half).
 * bfloat16 is not part of the reference's dispatch and is not provided. */
int pp_nmdistance_forward_f16(const void* xyz1, const void* xyz2, void* dist1, int* idx1, void* dist2, int* idx2,
                              int B, int N, int M, int C, void* stream);
int pp_nmdistance_backward_f16(const void* xyz1, const void* xyz2, const void* graddist1, const void* graddist2,
                               const int* idx1, const int* idx2, void* gradxyz1, void* gradxyz2, int B, int N,
                               int M, int C, void* stream);

/* ---- _ext.sampling ----------------------------------------------------------------------- */

/* Replaces sampling.furthest_sampling(m, seedIdx, input, temp, idx)
 *   (_ext/sampling.cpp:68-82 -> furthest_sampling_cuda_forward, _ext/sampling_cuda.cu:235-325).
 * xyz (B,N,3); temp (B,N) in/out running min squared distance (caller pre-fills 1e10,
 * network/geo_operations.py:33); idx (B,npoint) out, idx[:,0] = seed_idx.  temp == NULL: every point starts at 1e10
 * and nothing is written back (the wrapper one level up allocates temp itself and never reads it) -- served where the
 * bucketed kernel runs, PP_ENOTSUP otherwise (the caller then passes a temp of its own).
 * workspace: pp_furthest_sampling_workspace_bytes(...) bytes of scratch (may be NULL if that is 0); a pure
 * host computation (an upper bound over devices).  Layout: a 256-byte status word | the ring of the cluster kernel |
 * the scratch of the bucketed kernel (the cloud re-ordered into spatial buckets: 16 B per point + one word per point,
 * 65536 words per batch element up to 65536 points).  With that scratch -- 2048 <= N <= 2^22 and 32 or more picks --
 * the sampling is ONE workgroup per batch element that visits, per pick, only the buckets the pick can change (an
 * exact test: same picks, same temp); nothing waits for another workgroup there.  Without it (or for N > 65536 when
 * the batch leaves room) the cluster kernel runs: the first 256 bytes hold its STICKY status word, which the caller
 * zeroes once after allocating the buffer.  That kernel shares a batch element between workgroups
 * that wait for each other; it is only launched with as many workgroups as the current device keeps resident
 * (its real CU count and the occupancy query), and every wait is bounded: if one times out (CUs held by a
 * kernel of another stream), the call leaves zeros from that step on in idx and sets the status word, which
 * stays set until the caller clears it. */
size_t pp_furthest_sampling_workspace_bytes(int B, int N, int npoint);
/* Reads the status word (synchronises `stream`): 0 = ok, 1 = a wait of some pp_furthest_sampling_f32 call
 * on this workspace has timed out since the word was last zeroed. */
int pp_furthest_sampling_status(const void* workspace, void* stream);
int pp_furthest_sampling_f32(const float* xyz, float* temp, int* idx, int B, int N, int npoint,
                             int seed_idx, void* workspace, size_t workspace_bytes, void* stream);
/* The same with the picked points' coordinates written as well: the caller one level up,
 * network/geo_operations.py:59-63 (furthest_point_sample = the sampling + gather_points of the coordinates; SURVEY.md
 * §8f N3), in ONE launch.  sampled (B,npoint,3), or (B,3,npoint) with channels_first != 0; NULL = idx only. */
int pp_furthest_sampling_gather_f32(const float* xyz, float* temp, int* idx, float* sampled, int channels_first,
                                    int B, int N, int npoint, int seed_idx, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* Replaces sampling.gather_forward(b,c,n,npoints,points,idx,out)
 *   (_ext/sampling.cpp:19-28 -> _ext/sampling_cuda.cu:9-45).  points (B,C,N), idx (B,M) -> out (B,C,M) */
int pp_gather_forward_f32(const float* points, const int* idx, float* out, int B, int C, int N,
                          int M, void* stream);

/* Replaces sampling.gather_backward(b,c,n,npoints,grad_out,idx,grad_points)
 *   (_ext/sampling.cpp:31-41 -> _ext/sampling_cuda.cu:47-84).  ACCUMULATES into grad_points (B,C,N),
 * which the caller zero-fills (network/operations.py:76-77). */
int pp_gather_backward_f32(const float* grad_out, const int* idx, float* grad_points, int B, int C,
                           int N, int M, void* stream);

/* Replaces sampling.ball_query(new_xyz, xyz, radius, nsample)
 *   (_ext/sampling.cpp:85-104 -> _ext/sampling_cuda.cu:340-397).
 * new_xyz (B,M,3) centres, xyz (B,N,3) -> idx (B,M,nsample), fully written (rows with no hit are
 * written as zeros, which is what the reference's zero-filled allocation leaves). */
int pp_ball_query_f32(const float* new_xyz, const float* xyz, int* idx, int B, int N, int M,
                      float radius, int nsample, void* stream);

/* The same operation through a uniform grid over xyz (exact, same output), with the scan as the
 * fallback for batch elements whose radius spans too many cells.  workspace:
 * pp_ball_query_workspace_bytes(...) bytes (0 = not applicable); NULL = the scan. */
size_t pp_ball_query_workspace_bytes(int B, int N, int M, int nsample);
int pp_ball_query_ws_f32(const float* new_xyz, const float* xyz, int* idx, int B, int N, int M,
                         float radius, int nsample, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Replaces sampling.group_points(points, idx)
 *   (_ext/sampling.cpp:113-138 -> _ext/sampling_cuda.cu:447-478).
 * points (B,C,N), idx (B,npoint,nsample) -> out (B,C,npoint,nsample), fully written. */
int pp_group_points_f32(const float* points, const int* idx, float* out, int B, int C, int N,
                        int npoint, int nsample, void* stream);

/* The same gather into a tensor whose batch stride (in elements) is larger than C*npoint*nsample,
 * e.g. the channel slice [3, 3+C) of QueryAndGroup's concatenated output
 * (network/operations.py:196-204): the fused caller writes its result once instead of
 * grouping and then torch.cat-ing 4 GiB. */
int pp_group_points_strided_f32(const float* points, const int* idx, float* out, int B, int C, int N,
                                int npoint, int nsample, long long out_batch_stride, void* stream);

/* Replaces sampling.group_points_grad(grad_out, idx, n)
 *   (_ext/sampling.cpp:140-161 -> _ext/sampling_cuda.cu:482-513).
 * ACCUMULATES into grad_points (B,C,N), which the caller zero-fills. */
int pp_group_points_grad_f32(const float* grad_out, const int* idx, float* grad_points, int B,
                             int C, int N, int npoint, int nsample, void* stream);

/* grad_out given as a channel slice of a wider tensor (batch stride in elements). */
int pp_group_points_grad_strided_f32(const float* grad_out, const int* idx, float* grad_points, int B,
                                     int C, int N, int npoint, int nsample,
                                     long long grad_out_batch_stride, void* stream);

/* Replaces sampling.three_nn_wrapper(b,n,m,unknown,known,dist2,idx)
 *   (_ext/sampling.cpp:163-172 -> _ext/interpolate_gpu.cu:9-74).
 * unknown (B,N,3), known (B,M,3) -> dist2 (B,N,3) squared distances ascending, idx (B,N,3).
 * M < 3: unused slots hold +inf / index 0. */
int pp_three_nn_f32(const float* unknown, const float* known, float* dist2, int* idx, int B, int N,
                    int M, void* stream);

/* The same three_nn through an exact uniform-grid search (three_nn_grid.hip): identical outputs,
 * a few dozen candidates per unknown point instead of M.  pp_three_nn_workspace_bytes returns 0
 * when the grid path does not apply (small N or M); with a null / too small workspace the call is
 * pp_three_nn_f32.  The workspace is scratch: no state is kept between calls. */
size_t pp_three_nn_workspace_bytes(int B, int N, int M);
int pp_three_nn_ws_f32(const float* unknown, const float* known, float* dist2, int* idx, int B, int N,
                       int M, void* workspace, size_t workspace_bytes, void* stream);

/* K nearest neighbours: replaces pytorch3d.ops.knn_points, which the reference calls at
 *   network/model_loss.py:120,147,378, geo_operations.py:112,139, layers.py:52,99,115
 *   (pytorch3d is an un-vendored dependency, environment.yml:11).
 * p1 (B,N,3), p2 (B,M,3) -> dist2 (B,N,K) squared distances ascending, idx (B,N,K); 1 <= K <= 32.
 * Ties go to the lower index.  lengths1 / lengths2 (B ints, may be null): valid points per cloud;
 * slots beyond the valid points of p2 and rows beyond lengths1 hold (0, 0).
 * pp_knn_ws_f32: the same through the exact uniform-grid search (identical outputs); ragged batches
 * and small clouds take the scan. */
int pp_knn_f32(const float* p1, const float* p2, const int* lengths1, const int* lengths2, float* dist2,
               int* idx, int B, int N, int M, int K, void* stream);
size_t pp_knn_workspace_bytes(int B, int N, int M, int K);
int pp_knn_ws_f32(const float* p1, const float* p2, const int* lengths1, const int* lengths2, float* dist2,
                  int* idx, int B, int N, int M, int K, void* workspace, size_t workspace_bytes,
                  void* stream);
/* The same operator for ANY point dimension D (1..512) and K up to 128 -- the reference's feature-space
 * searches, network/layers.py:52,99 (DenseEdgeConv: D = channel count, K = k + 1).  p1 (B,N,D), p2 (B,M,D).
 * Squared distance = the sequential chain d = fma(t_c, t_c, d), c = 0..D-1; ties to the lower index. */
int pp_knn_nd_f32(const float* p1, const float* p2, const int* lengths1, const int* lengths2, float* dist2,
                  int* idx, int B, int N, int M, int D, int K, void* stream);

/* Replaces sampling.three_interpolate_wrapper(b,c,m,n,points,idx,weight,out)
 *   (_ext/sampling.cpp:175-188 -> _ext/interpolate_gpu.cu:77-117).
 * points (B,C,M), idx (B,N,3), weight (B,N,3) -> out (B,C,N) */
int pp_three_interpolate_f32(const float* points, const int* idx, const float* weight, float* out,
                             int B, int C, int M, int N, void* stream);

/* Replaces sampling.three_interpolate_grad_wrapper(b,c,n,m,grad_out,idx,weight,grad_points)
 *   (_ext/sampling.cpp:190-203 -> _ext/interpolate_gpu.cu:120-160).
 * ACCUMULATES into grad_points (B,C,M), which the caller zero-fills
 * (network/pointnet2_utils.py:82). */
int pp_three_interpolate_grad_f32(const float* grad_out, const int* idx, const float* weight,
                                  float* grad_points, int B, int C, int N, int M, void* stream);

/* ---- the three scatter-add backwards with a caller-provided workspace -----------------------
 * Same contracts as pp_group_points_grad_strided_f32 / pp_gather_backward_f32 /
 * pp_three_interpolate_grad_f32 (they ACCUMULATE into caller-zeroed outputs).  With a workspace of
 * pp_scatter_workspace_bytes(B, triples per batch element, destinations per batch element,
 * triples per source element, weighted) bytes the (source, destination) pairs are sorted once per
 * call and no atomics are issued; without one (or when the size does not qualify: the function
 * returns 0 bytes) they are the atomic forms.
 *   group_points_grad:      triples = npoint*nsample, destinations = N, per_source = 1, weighted = 0
 *   gather_backward:        triples = M,              destinations = N, per_source = 1, weighted = 0
 *   three_interpolate_grad: triples = 3*N,            destinations = M, per_source = 3, weighted = 1 */
size_t pp_scatter_workspace_bytes(int B, long long triples_per_batch, int destinations, int per_source,
                                  int weighted);
int pp_group_points_grad_ws_f32(const float* grad_out, const int* idx, float* grad_points, int B, int C,
                                int N, int npoint, int nsample, long long grad_out_batch_stride,
                                void* workspace, size_t workspace_bytes, void* stream);
/* The same with grad_points (B,C,N) WRITTEN instead of accumulated into: it need not be initialised (the reference's
 * group_points_grad allocates a zero-filled tensor and adds into it, _ext/sampling.cpp:148-150 -- the fill and the read
 * of the output are 2 x 256 MB of traffic at B=32, C=128, N=16384 that this form does not move). */
int pp_group_points_grad_out_ws_f32(const float* grad_out, const int* idx, float* grad_points, int B, int C,
                                    int N, int npoint, int nsample, long long grad_out_batch_stride,
                                    void* workspace, size_t workspace_bytes, void* stream);
int pp_gather_backward_ws_f32(const float* grad_out, const int* idx, float* grad_points, int B, int C,
                              int N, int M, void* workspace, size_t workspace_bytes, void* stream);
int pp_three_interpolate_grad_ws_f32(const float* grad_out, const int* idx, const float* weight,
                                     float* grad_points, int B, int C, int N, int M, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ---- deterministic ("ordered") backward passes --------------------------------------------------
 * The reference adds every gradient term with a global fp32 atomic, so its sums depend on the order
 * the hardware happens to serve (nmdistance_cuda.cu:180-181, sampling_cuda.cu:63,499-500,
 * interpolate_gpu.cu:139-141); the default entry points above keep the same freedom.  These four add
 * each destination's terms in ASCENDING SOURCE ORDER with no floating-point atomics: the result is
 * identical from run to run, and identical bit for bit to a sequential loop over the reference's
 * launches (the CPU oracle under oracle/).  The host side selects them when
 * torch.are_deterministic_algorithms_enabled().  They return PP_ENOTSUP for shapes the ordered forms
 * cannot serve (Chamfer: C != 3 or a cloud beyond ~19000 points; scatter ops: more than 20480
 * destinations per batch element, or a workspace smaller than pp_scatter_workspace_bytes): there is no
 * deterministic substitute.  Workspaces as for the *_ws_* entry points; grad_points must be zero-filled
 * by the caller for the three scatter ops (they accumulate), gradxyz is overwritten. */
int pp_nmdistance_backward_ordered_f32(const float* xyz1, const float* xyz2, const float* graddist1,
                                       const float* graddist2, const int* idx1, const int* idx2,
                                       float* gradxyz1, float* gradxyz2, int B, int N, int M, int C,
                                       void* stream);
int pp_group_points_grad_ordered_f32(const float* grad_out, const int* idx, float* grad_points, int B, int C,
                                     int N, int npoint, int nsample, long long grad_out_batch_stride,
                                     void* workspace, size_t workspace_bytes, void* stream);
int pp_gather_backward_ordered_f32(const float* grad_out, const int* idx, float* grad_points, int B, int C,
                                   int N, int M, void* workspace, size_t workspace_bytes, void* stream);
int pp_three_interpolate_grad_ordered_f32(const float* grad_out, const int* idx, const float* weight,
                                          float* grad_points, int B, int C, int N, int M, void* workspace,
                                          size_t workspace_bytes, void* stream);

/* ---- 16-bit features (DESIGN.md §4 "16-bit features") --------------------------------------------
 * gather_points, group_points and three_interpolate on FEATURE tensors of IEEE half (_f16) or bfloat16 (_bf16)
 * elements; idx stays int32 and weight fp32.  Shapes and argument order as the _f32 entry points.
 *   _b16: a copy -- the gathered 2-byte words are moved unchanged (every NaN payload, both zeros, subnormals), so
 *     one entry point serves both types.  out_batch_stride is in elements.
 *   pp_three_interpolate_f16/_bf16: the operands widened (exact), the fp32 chain fma(w2,p2, fma(w0,p0, w1*p1)), one
 *     rounding to nearest even (half overflows to +-inf): bit-identical to rounding the _f32 result on the widened
 *     features.
 *   *_out_ws_f16/_bf16: the backwards.  grad_points is WRITTEN (no zero fill by the caller, the output is not read).
 *     Each destination's terms -- the widened grad_out, for three_interpolate the fp32 products with the weight -- are
 *     summed in the accumulator of the fp32 form (the double LDS column, or the fp32 slots of the sorted scatter) and
 *     rounded once: double -> float -> T, or float -> T.  No 16-bit floating-point atomics: PP_ENOTSUP when no
 *     atomic-free form serves the shape (no sorted-scatter workspace qualifies, e.g. more than 20480 destinations, and
 *     the double column does not apply: group_points below 4096 positions, three_interpolate below 2048 points or
 *     beyond 19456 known points; gather has the sorted form only) -- the caller then widens and uses the _f32 path.
 *     The deterministic mode is the `ordered` ARGUMENT (not separate symbols: it halves these declarations):
 *     ordered != 0 takes the sorted scatter in ascending source order -- the rounded result of the *_ordered_f32
 *     entry point, bit for bit -- or returns PP_ENOTSUP.  workspace: pp_scatter_workspace_bytes, as for _f32 (the
 *     triple lists do not depend on the element type).
 * Sizes of zero are served, a negative size returns PP_EINVAL, both before any pointer is looked at. */
int pp_gather_forward_b16(const void* points, const int* idx, void* out, int B, int C, int N, int M, void* stream);
int pp_group_points_strided_b16(const void* points, const int* idx, void* out, int B, int C, int N, int npoint,
                                int nsample, long long out_batch_stride, void* stream);
int pp_three_interpolate_f16(const void* points, const int* idx, const float* weight, void* out, int B, int C, int M,
                             int N, void* stream);
int pp_three_interpolate_bf16(const void* points, const int* idx, const float* weight, void* out, int B, int C, int M,
                              int N, void* stream);
int pp_gather_backward_out_ws_f16(const void* grad_out, const int* idx, void* grad_points, int B, int C, int N, int M,
                                  void* workspace, size_t workspace_bytes, int ordered, void* stream);
int pp_gather_backward_out_ws_bf16(const void* grad_out, const int* idx, void* grad_points, int B, int C, int N, int M,
                                   void* workspace, size_t workspace_bytes, int ordered, void* stream);
int pp_group_points_grad_out_ws_f16(const void* grad_out, const int* idx, void* grad_points, int B, int C, int N,
                                    int npoint, int nsample, long long grad_out_batch_stride, void* workspace,
                                    size_t workspace_bytes, int ordered, void* stream);
int pp_group_points_grad_out_ws_bf16(const void* grad_out, const int* idx, void* grad_points, int B, int C, int N,
                                     int npoint, int nsample, long long grad_out_batch_stride, void* workspace,
                                     size_t workspace_bytes, int ordered, void* stream);
int pp_three_interpolate_grad_out_ws_f16(const void* grad_out, const int* idx, const float* weight, void* grad_points,
                                         int B, int C, int N, int M, void* workspace, size_t workspace_bytes,
                                         int ordered, void* stream);
int pp_three_interpolate_grad_out_ws_bf16(const void* grad_out, const int* idx, const float* weight, void* grad_points,
                                          int B, int C, int N, int M, void* workspace, size_t workspace_bytes,
                                          int ordered, void* stream);

/* ---- _ext.linalg ------------------------------------------------------------------------
 * Replaces linalg.batch_svd_forward(a, is_sort, tol, max_sweeps) (torch_batch_svd.cpp:38-140, cuSOLVER gesvdj).
 * a (batch,m,n), m,n in 1..32 -> a = U[:, :, :k] diag(s) V[:, :, :k]^T, k = min(m,n); s (batch,k) >= 0;
 * full != 0: U (batch,m,m), V (batch,n,n); full == 0: U (batch,m,k), V (batch,n,k).  One-sided Jacobi: a column pair is
 * converged when |w_p.w_q| <= tol ||w_p|| ||w_q||; at most max_sweeps sweeps.  sort != 0: s descending (ties to the
 * lower column).  info (batch) int32, nullable: sweeps used (1..max_sweeps), -1 not converged, -2 a non-finite entry
 * (then that matrix's s, U and V are NaN).  Columns of U (V) beyond k or with s == 0 are a deterministic orthonormal
 * completion.  Each matrix's result depends on that matrix alone.  PP_EINVAL: m or n outside 1..32, batch < 0,
 * max_sweeps < 1, tol < 0 or NaN, a null pointer with batch > 0. */
int pp_batch_svd_f32(const float* a, float* u, float* s, float* v, int* info, long long batch, int m, int n,
                     int full, int sort, float tol, int max_sweeps, void* stream);

/* ---- mean value coordinates ---------------------------------------------------------------
 * Replaces network.geo_operations.mean_value_coordinates_3D(query, vertices, faces, verbose) (geo_operations.py:349-456,
 * torch composition); contract in DESIGN.md "Mean value coordinates".  query (B,P,3), vertices (B,N,3), faces int64
 * (B,F,3) read at faces + b * faces_batch_stride (elements; 0 = one face list for every batch element).
 * Forward -> wj (B,P,N) normalised weights; sums (B,P) the divisor used; codes (B,P) int32 branch bits (1 zero row sum,
 * 2 on a face, 4 on a vertex, 8 an out-of-range face index: the row is NaN); wi (B,P,F,3), nullable, the per-face
 * weights after the face branches.  Backward: grad_wj (B,P,N), grad_wi (nullable) -> grad_query (B,P,3),
 * grad_vertices (B,N,3), with a workspace of pp_mvc3d_workspace_bytes(B,P,N,sizeof element) bytes.  No floating-point
 * atomics: every output is reproducible bit for bit, and a query's row does not depend on the other queries. */
size_t pp_mvc3d_workspace_bytes(int B, int P, int N, int elem_bytes);
int pp_mvc3d_forward_f32(const float* query, const float* vertices, const long long* faces,
                         long long faces_batch_stride, float* wj, float* sums, int* codes, float* wi, int B, int P,
                         int N, int F, void* stream);
int pp_mvc3d_forward_f64(const double* query, const double* vertices, const long long* faces,
                         long long faces_batch_stride, double* wj, double* sums, int* codes, double* wi, int B, int P,
                         int N, int F, void* stream);
int pp_mvc3d_backward_f32(const float* query, const float* vertices, const long long* faces,
                          long long faces_batch_stride, const float* wj, const float* sums, const int* codes,
                          const float* grad_wj, const float* grad_wi, float* grad_query, float* grad_vertices, int B,
                          int P, int N, int F, void* workspace, size_t workspace_bytes, void* stream);
int pp_mvc3d_backward_f64(const double* query, const double* vertices, const long long* faces,
                          long long faces_batch_stride, const double* wj, const double* sums, const int* codes,
                          const double* grad_wj, const double* grad_wi, double* grad_query, double* grad_vertices,
                          int B, int P, int N, int F, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Green coordinates --------------------------------------------------------------------
 * Replaces network.geo_operations.green_coordinates_3D(query, vertices, faces, face_normals) (geo_operations.py:625-773,
 * torch composition) for the pair evaluation; contract in DESIGN.md "Green coordinates".  query (B,P,3), vertices
 * (B,N,3), faces int64 (B,F,3) read at faces + b * faces_batch_stride (elements; 0 = one face list for every batch
 * element), normals (B,F,3) the face normals n_t.  Forward -> gc_vertex (B,P,N) normalised vertex coordinates,
 * gc_face (B,P,F) face coordinates, sums (B,P) the unnormalised row sum S (exterior_flag = S < 0.5), codes (B,P) int32
 * (8: an out-of-range face index in the batch element; its rows and sums are NaN).  Backward: grad_gc_vertex (B,P,N),
 * grad_gc_face (nullable) -> grad_query (B,P,3), grad_normals (B,F,3), with a workspace of
 * pp_gc3d_workspace_bytes(B,P,F,sizeof element) bytes.  The vertices get no gradient here (the reference detaches
 * them).  No floating-point atomics: every output is reproducible bit for bit, and a query's row does not depend on
 * the other queries. */
size_t pp_gc3d_workspace_bytes(int B, int P, int F, int elem_bytes);
int pp_gc3d_forward_f32(const float* query, const float* vertices, const long long* faces,
                        long long faces_batch_stride, const float* normals, float* gc_vertex, float* gc_face,
                        float* sums, int* codes, int B, int P, int N, int F, void* stream);
int pp_gc3d_forward_f64(const double* query, const double* vertices, const long long* faces,
                        long long faces_batch_stride, const double* normals, double* gc_vertex, double* gc_face,
                        double* sums, int* codes, int B, int P, int N, int F, void* stream);
int pp_gc3d_backward_f32(const float* query, const float* vertices, const long long* faces,
                         long long faces_batch_stride, const float* normals, const float* gc_vertex,
                         const float* sums, const int* codes, const float* grad_gc_vertex, const float* grad_gc_face,
                         float* grad_query, float* grad_normals, int B, int P, int N, int F, void* workspace,
                         size_t workspace_bytes, void* stream);
int pp_gc3d_backward_f64(const double* query, const double* vertices, const long long* faces,
                         long long faces_batch_stride, const double* normals, const double* gc_vertex,
                         const double* sums, const int* codes, const double* grad_gc_vertex,
                         const double* grad_gc_face, double* grad_query, double* grad_normals, int B, int P, int N,
                         int F, void* workspace, size_t workspace_bytes, void* stream);

/* ---- mean value coordinates, 2-D -----------------------------------------------------------
 * Replaces network.geo_operations.mean_value_coordinates(points, polygon) (geo_operations.py:459-526, torch
 * composition); contract in DESIGN.md "Mean value coordinates, 2-D".  Channel-first: points (B,2,N), polygon (B,2,M),
 * vertices i+1 and i-1 taken cyclically; any M.  Forward -> phi (B,M,N) normalised weights; w (B,M,N), nullable, the
 * row before the division; sums (B,N) the divisor used; codes (B,N) int32 branch bits (1 zero row sum, 2 on an edge,
 * 4 on a vertex, 8 a non-finite input: the row is NaN).  Backward: grad_phi (B,M,N), grad_w (nullable) ->
 * grad_points (B,2,N), grad_polygon (B,2,M), with a workspace of pp_mvc2d_workspace_bytes(B,N,M,sizeof element) bytes
 * (0 for an element size that is not served).  A size of zero is served: the forward then writes nothing, the backward
 * zero gradients; a negative size returns PP_EINVAL before any pointer is looked at.  No floating-point atomics:
 * every output is reproducible bit for bit, and a query's row does not depend on the other queries. */
size_t pp_mvc2d_workspace_bytes(int B, int N, int M, int elem_bytes);
int pp_mvc2d_forward_f32(const float* points, const float* polygon, float* phi, float* w, float* sums, int* codes,
                         int B, int N, int M, void* stream);
int pp_mvc2d_forward_f64(const double* points, const double* polygon, double* phi, double* w, double* sums, int* codes,
                         int B, int N, int M, void* stream);
int pp_mvc2d_backward_f32(const float* points, const float* polygon, const float* phi, const float* sums,
                          const int* codes, const float* grad_phi, const float* grad_w, float* grad_points,
                          float* grad_polygon, int B, int N, int M, void* workspace, size_t workspace_bytes,
                          void* stream);
int pp_mvc2d_backward_f64(const double* points, const double* polygon, const double* phi, const double* sums,
                          const int* codes, const double* grad_phi, const double* grad_w, double* grad_points,
                          double* grad_polygon, int B, int N, int M, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- Green coordinates, 2-D ---------------------------------------------------------------
 * network.geo_operations.green_coordinates_2D(query, vertices, faces, edge_normals), which the reference declares and
 * leaves empty (geo_operations.py:622); contract in DESIGN.md "Green coordinates, 2-D".  query (B,P,2), vertices
 * (B,N,2), faces int64 (B,F,2), row j the directed edge (v1, v2), read at faces + b * faces_batch_stride (elements;
 * 0 = one edge list for every batch element); edge_normals (B,F,2), nullable, only orients: an edge whose own normal
 * (a_y, -a_x), a = v2 - v1, points against its row is taken reversed.  Forward -> phi (B,P,N) vertex coordinates (not
 * renormalised), psi (B,P,F) edge coordinates, exterior (B,P) bytes 0 / 1 (the fp64 row sum of phi < 0.5), codes (B,P)
 * int32 (8: an out-of-range index in the batch element; 1: a non-finite pair; the rows are NaN and exterior 0).
 * Backward: grad_phi (B,P,N) and grad_psi (B,P,F), either nullable -> grad_query (B,P,2), grad_vertices (B,N,2), with a
 * workspace of pp_gc2d_workspace_bytes(B,P,F,sizeof element) bytes (0 for an element size that is not served).  A size
 * of zero is served; a negative size returns PP_EINVAL before any pointer is looked at.  Every pair is evaluated in
 * fp64 for either data type.  No floating-point atomics: every output is reproducible bit for bit, and a query's row
 * does not depend on the other queries. */
size_t pp_gc2d_workspace_bytes(int B, int P, int F, int elem_bytes);
int pp_gc2d_forward_f32(const float* query, const float* vertices, const long long* faces,
                        long long faces_batch_stride, const float* edge_normals, float* phi, float* psi,
                        unsigned char* exterior, int* codes, int B, int P, int N, int F, void* stream);
int pp_gc2d_forward_f64(const double* query, const double* vertices, const long long* faces,
                        long long faces_batch_stride, const double* edge_normals, double* phi, double* psi,
                        unsigned char* exterior, int* codes, int B, int P, int N, int F, void* stream);
int pp_gc2d_backward_f32(const float* query, const float* vertices, const long long* faces,
                         long long faces_batch_stride, const float* edge_normals, const int* codes,
                         const float* grad_phi, const float* grad_psi, float* grad_query, float* grad_vertices, int B,
                         int P, int N, int F, void* workspace, size_t workspace_bytes, void* stream);
int pp_gc2d_backward_f64(const double* query, const double* vertices, const long long* faces,
                         long long faces_batch_stride, const double* edge_normals, const int* codes,
                         const double* grad_phi, const double* grad_psi, double* grad_query, double* grad_vertices,
                         int B, int P, int N, int F, void* workspace, size_t workspace_bytes, void* stream);

/* ---- k-NN edge operators -------------------------------------------------------------------
 * The (B,N,K,D) gather of a cloud's k-NN neighbourhoods and what the reference's point-cloud regularisers compute
 * from it, without the gather; contract in DESIGN.md "k-NN edge operators".  points (B,N,D) fp32, idx int64 (B,N,K) as
 * knn_points returns it, 1 <= K <= 128, 1 <= D <= 32 (D == 3 is specialised), N*K < 2^31.
 * Edge lengths replace the gather + torch.norm of network/model_loss.py:120-127,147-152 and the gather + squared sum of
 *   :378-385: out (B,N,K) = |points[idx[n,k]] - points[n]|^2 (the library's distance chain: bit-identical to
 *   knn_points' dists), or its correctly rounded root when squared == 0.
 * The Laplacian replaces network/geo_operations.py:128-152 pointUniformLaplacian:
 *   lap (B,N,D) = -(sum_k points[idx[n,k]]) / K + points[n], the sum in ascending k.
 * Backwards: gathers over the reverse adjacency of idx, built in a workspace of pp_knn_edges_workspace_bytes(B,N,K)
 * bytes (not needed with detach_neighbors); grad_points (B,N,D) is overwritten.  `out` is the forward's output.
 * detach_neighbors != 0: only the centre point of an edge receives its gradient (:379 detaches the neighbours).
 * No floating-point atomics.  ordered != 0: every point adds its own edges in ascending k, then its incoming edges in
 * ascending (n,k): reproducible bit for bit and equal to a sequential loop in that order; ordered == 0 leaves the
 * order of the incoming terms unspecified.
 * An index outside [0,N) is never dereferenced: that edge's length and that row of the Laplacian are NaN, and in the
 * backwards the row takes no part in the scatter and its centre point's gradient is NaN. */
size_t pp_knn_edges_workspace_bytes(int B, int N, int K);
int pp_knn_edge_lengths_forward_f32(const float* points, const long long* idx, float* out, int B, int N, int K, int D,
                                    int squared, void* stream);
int pp_knn_edge_lengths_backward_f32(const float* points, const long long* idx, const float* out,
                                     const float* grad_out, float* grad_points, int B, int N, int K, int D,
                                     int squared, int detach_neighbors, int ordered, void* workspace,
                                     size_t workspace_bytes, void* stream);
int pp_knn_laplacian_forward_f32(const float* points, const long long* idx, float* lap, int B, int N, int K, int D,
                                 void* stream);
int pp_knn_laplacian_backward_f32(const long long* idx, const float* grad_lap, float* grad_points, int B, int N, int K,
                                  int D, int ordered, void* workspace, size_t workspace_bytes, void* stream);

/* ---- edge features ---------------------------------------------------------------------------
 * The edge tensor of an EdgeConv layer (network/layers.py:41-62,88-109); contract in DESIGN.md "Edge features".
 * x (B,C,N), query (B,C,P), out (B,2C,P,K) of one element type: dtype 0 = fp32, 1 = fp16, 2 = bf16; idx (B,P,K) int64
 * (idx64 != 0) or int32.
 * pp_edge_features_forward: out[b,c,p,k] = query[b,c,p] (the words copied), out[b,C+c,p,k] = x[b,c,idx[b,p,k]] -
 *   query[b,c,p] (16-bit: widened, subtracted in fp32, rounded once); every element written exactly once.  The self
 *   graph passes query = x, P = N.
 * pp_edge_features_backward: grad_out (B,2C,P,K); grad_query (B,C,P) and grad_x (B,C,N) are overwritten, either may
 *   be NULL (not wanted: its pass, and for grad_x the adjacency build, is skipped).
 *   grad_query[b,c,p] = sum_k (g[b,c,p,k] - g[b,C+c,p,k]), ascending k in fp32 from the k = 0 term.
 *   grad_x[b,c,n] = the sum of g[b,C+c,p,k] over the edges with idx[b,p,k] == n, a gather over the reverse adjacency
 *   built in the workspace; no floating-point atomics.  ordered != 0: the edges in ascending p*K+k, plain fp32 sums
 *   from +0.0 (the same bits on every run); otherwise any order, compensated fp32 sums.
 *   self_graph != 0 (P == N, grad_query NULL): grad_x = the centre sum above, then the incoming terms added to it.
 * An index outside [0,N) is only compared: its difference elements are NaN, its row (b,p) takes no part in grad_x and
 *   its grad_query (self graph: grad_x) elements are NaN.
 * Workspace: pp_edge_features_workspace_bytes(B, N, P, K, adjacency) bytes, adjacency != 0 where grad_x is wanted
 *   (host arithmetic; 0 for a shape the entry points refuse).  PP_EINVAL for K > 128, an empty dimension, or where
 *   P*K, B*N, B*P or B*C exceeds 2^31 - 1. */
size_t pp_edge_features_workspace_bytes(int B, int N, int P, int K, int adjacency);
int pp_edge_features_forward(const void* x, const void* query, const void* idx, void* out, int B, int C, int N, int P,
                             int K, int dtype, int idx64, void* stream);
int pp_edge_features_backward(const void* idx, const void* grad_out, void* grad_x, void* grad_query, int B, int C,
                              int N, int P, int K, int dtype, int idx64, int self_graph, int ordered, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- mesh edge operators -------------------------------------------------------------------
 * What the reference's mesh losses (network/model_loss.py:166-308) and edge utilities (geo_operations.py:562-600) stand
 * on; contract in DESIGN.md "Mesh edge operators".  int64 indices, fp32 vertices (B,N,3).  The two builds run once per
 * topology, the two step kernels per training step.
 * pp_mesh_unique_edges replaces edge_vertex_indices (torch.unique over the sorted half-edges): faces (Bt,F,3) ->
 *   edges (Bt,3F,2): rows [0,counts[b]) the unique unordered vertex pairs as (min,max), ascending lexicographically
 *   (torch.unique's rows, bit for bit; a face with a repeated vertex keeps its (a,a) pair), every later row (-1,-1);
 *   counts (Bt) int32; flags (Bt) int32, non-zero where a face names a vertex outside [0,n_vertices): such an index is
 *   only compared, its half-edges are left out.  The result does not depend on the order atomics are served in.
 * pp_mesh_edge_incidence: edges (Bt,Ecap,2) -- any list: repeated pairs, unsorted, self-edges -- and counts (Bt) ->
 *   inc_start (Bt,n_vertices+1) int32 and inc_entries (Bt,2*Ecap) uint32: vertex v's slice
 *   [inc_start[v],inc_start[v+1]) holds 2*e + side for every e < counts[b] with edges[e,side] == v, ascending.  An end
 *   outside [0,n_vertices) is only compared, left out, and ORed into flags (Bt), which the caller has initialised.
 * Workspace: pp_mesh_edges_workspace_bytes(Bt, n_vertices, items) bytes, items = 3F for the unique edges and 2*Ecap
 *   for the incidence (host arithmetic; 0 for an empty problem).  PP_EINVAL where Bt*items or Bt*(n_vertices+1) exceeds
 *   2^31 - 1, the index words in use.
 * pp_mesh_edge_sqrlen_forward_f32: out (B,Ecap) = |v[b,edges[e,0]] - v[b,edges[e,1]]|^2 for e < counts, 0 behind; the
 *   library's distance chain (bit-identical to pp_knn_edge_lengths_forward_f32's squared form for the same pair).
 *   shared_topology != 0: edges, counts and the incidence have one batch element, read by every b.
 * pp_mesh_edge_sqrlen_backward_f32: grad_vertices (B,N,3), overwritten: every vertex walks its incidence slice in
 *   order with t = (2 grad_out[b,e]) * (v_a - v_b); side 0 adds t, side 1 subtracts it; plain fp32 sums from 0.
 *   Identical on every run and bit for bit the loop `for e: grad[a] += t; grad[b] -= t`.  No floating-point atomics.
 * An edge with an end outside [0,N) reads nothing there: NaN length, NaN added to the gradient of its other end. */
size_t pp_mesh_edges_workspace_bytes(int Bt, int n_vertices, long long items);
int pp_mesh_unique_edges(const long long* faces, long long* edges, int* counts, int* flags, int Bt, int F,
                         int n_vertices, void* workspace, size_t workspace_bytes, void* stream);
int pp_mesh_edge_incidence(const long long* edges, const int* counts, int* inc_start, unsigned* inc_entries,
                           int* flags, int Bt, int Ecap, int n_vertices, void* workspace, size_t workspace_bytes,
                           void* stream);
int pp_mesh_edge_sqrlen_forward_f32(const float* vertices, const long long* edges, const int* counts, float* out,
                                    int B, int N, int Ecap, int shared_topology, void* stream);
int pp_mesh_edge_sqrlen_backward_f32(const float* vertices, const long long* edges, const int* inc_start,
                                     const unsigned* inc_entries, const float* grad_out, float* grad_vertices, int B,
                                     int N, int Ecap, int shared_topology, void* stream);

/* ---- mesh Laplacians ------------------------------------------------------------------------
 * What the reference's UniformLaplacian, CotLaplacian and cotangent (geo_operations.py:155-346) stand on; contract in
 * DESIGN.md "Mesh Laplacians".  A corner is (f, c) with vertex faces[f,c], next = faces[f,(c+1)%L] and
 * prev = faces[f,(c-1)%L].
 * pp_mesh_corner_incidence: faces (Bt,F,L) int64, L >= 3 -> start (Bt,n_vertices+1) int32; codes (Bt,L*F) uint32:
 *   vertex v's slice [start[v],start[v+1]) holds L*f + c for every corner with faces[f,c] == v, ascending; nbr
 *   (Bt,L*F,2) int32: (next, prev) of every slot, -1 for an index outside [0,n_vertices).  flags (Bt) int32 is
 *   overwritten: non-zero where a face names such an index, which is only compared and whose corner is left out (the
 *   slots behind start[n_vertices] are then not written).  Scratch: pp_mesh_edges_workspace_bytes(Bt, n_vertices, L*F)
 *   bytes, and the same limits.  Built with the bucket / scan / fill / sort chain of the edge builds.
 * pp_mesh_cotangent_f32: vertices (B,N,3), triangles faces (Bt,F,3) -> out (B,F,3), columns for the edges 23, 31, 12:
 *   l = sqrt((dx*dx + dy*dy) + dz*dz); sp = ((l1+l2)+l3)*0.5; inside = sp*(sp-l1)*(sp-l2)*(sp-l3) left to right,
 *   negative -> 0; A = 2*sqrt(inside); out = ((l2*l2 + l3*l3) - l1*l1) / (A + 1e-10f) / 4 and its rotations, +0 where
 *   A == 0.  A face with an index outside [0,N) reads nothing and gives NaN.
 * pp_mesh_laplacian_apply_f32: out (B,N,3), overwritten; one gather per vertex over its slice in slot order, from +0,
 *   plain fp32 operations: no floating-point atomics, the same bits on every run.
 *   mode 0, uniform forward:  acc += (x_i - x_next); acc += (x_i - x_prev); out = acc / ((float)(2n) + 1e-12f), n the
 *     number of slots of i.
 *   mode 1, uniform backward: x is the incoming gradient g; the same sum over h_k = g_k / ((float)(2 n_k) + 1e-12f),
 *     not divided again (exact: the half-edge multiplicity matrix is symmetric).
 *   mode 2, cotangent (L == 3), weights (B,F,3): for a slot 3f + c, acc += W[b,f,(c+2)%3] * (x_next - x_i);
 *     acc += W[b,f,(c+1)%3] * (x_prev - x_i).  The operator is symmetric: its backward is mode 2 on the gradient.
 *   weights may be NULL in modes 0 and 1.  shared_topology != 0: start, codes and nbr have one batch element, read by
 *   every b; weights are always per batch element.  A neighbour stored as -1 adds NaN. */
int pp_mesh_corner_incidence(const long long* faces, int* start, unsigned* codes, int* nbr, int* flags, int Bt, int F,
                             int L, int n_vertices, void* workspace, size_t workspace_bytes, void* stream);
int pp_mesh_cotangent_f32(const float* vertices, const long long* faces, float* out, int B, int N, int F,
                          int shared_topology, void* stream);
int pp_mesh_laplacian_apply_f32(const float* x, const int* start, const int* nbr, const unsigned* codes,
                                const float* weights, float* out, int B, int N, int F, int L, int mode,
                                int shared_topology, void* stream);

/* ---- mesh dihedral angles -------------------------------------------------------------------
 * What the reference's get_normals / dihedral_angle (geo_operations.py:603-619, :775-789) and its (E,4) edge-points
 * table (utils/geometry_utils.py:242-341) stand on; contract in DESIGN.md "Mesh dihedral angles".  int64 indices, fp32
 * vertices (B,N,3).  The two builds run once per topology, the two step kernels per training step.
 * pp_mesh_edge_points: faces (Bt,F,3), edges (Bt,Ecap,2) and counts (Bt) as pp_mesh_unique_edges made them ->
 *   edge_points (Bt,Ecap,4): row e < counts[b] is [a, c, w0, w1], (a,c) = edges[e], w0 / w1 the corner opposite the
 *   edge in the incident half-edge with the lowest / highest number 3f + j (half-edge j joins corners j and (j+1)%3);
 *   a boundary edge has w1 == w0; every later row is -1.  nonmanifold (Bt) int32, initialised by the caller, is ORed
 *   where an edge has more than two incident half-edges.  A half-edge with an index outside [0,n_vertices) is only
 *   compared and takes no part (pp_mesh_unique_edges flags it).  Integer atomics only (min, max, count) in the rows
 *   themselves: no scratch, and a result that does not depend on the order they are served in.
 * pp_mesh_edge_points_incidence: edge_points (Bt,Ecap,4) -- any table -- and counts (Bt) -> start (Bt,n_vertices+1)
 *   int32 and entries (Bt,4*Ecap) uint32: vertex v's slice [start[v],start[v+1]) holds 4*e + slot for every
 *   e < counts[b] with edge_points[e,slot] == v, ascending (a boundary edge's repeated wing under both slots).  An
 *   entry outside [0,n_vertices) is only compared, left out, and ORed into flags (Bt), which the caller has
 *   initialised.  Scratch: pp_mesh_edges_workspace_bytes(Bt, n_vertices, 4*Ecap) bytes, and its limits.
 * pp_mesh_dihedral_forward_f32: out (B,Ecap), with p_k = vertices[b, row[k]] in canonical order (the two ends
 *   ascending, the two wings ascending: the value does not depend on either order, and so neither do its bits):
 *   na = (p2-p0) x (p1-p0), nb = (p3-p1) x (p0-p1), each divided by max(|n|, 1e-12f);
 *   d = clamp(na.nb, -1+1e-6, 1-1e-6); out = pi - acosf(d); 0 for e >= counts.  The products a*b - c*d are evaluated
 *   with explicit fused multiply-adds (Kahan's difference of products).  shared_topology != 0: edge_points, counts and
 *   the incidence have one batch element, read by every b.
 * pp_mesh_dihedral_backward_f32: grad_vertices (B,N,3), overwritten: every vertex walks its slice in order, evaluates
 *   the edge's chain again and adds its slot's term, plain fp32 sums from +0.  d(out)/d(d) = 1/sqrt((1-d)(1+d)) where
 *   the unclamped dot lies in the closed clamp interval, 0 outside it, and 0 for an edge with a normal of length
 *   <= 1e-12f.  Identical on every run; no floating-point atomics.
 * A row with an index outside [0,N) reads nothing there: NaN angle, NaN added to the gradients of its in-range
 * entries. */
int pp_mesh_edge_points(const long long* faces, const long long* edges, const int* counts, long long* edge_points,
                        int* nonmanifold, int Bt, int F, int Ecap, int n_vertices, void* stream);
int pp_mesh_edge_points_incidence(const long long* edge_points, const int* counts, int* start, unsigned* entries,
                                  int* flags, int Bt, int Ecap, int n_vertices, void* workspace,
                                  size_t workspace_bytes, void* stream);
int pp_mesh_dihedral_forward_f32(const float* vertices, const long long* edge_points, const int* counts, float* out,
                                 int B, int N, int Ecap, int shared_topology, void* stream);
int pp_mesh_dihedral_backward_f32(const float* vertices, const long long* edge_points, const int* start,
                                  const unsigned* entries, const float* grad_out, float* grad_vertices, int B, int N,
                                  int Ecap, int shared_topology, void* stream);

/* ---- mesh normals ---------------------------------------------------------------------------
 * The unit normals and areas of a triangle mesh's faces (the reference's compute_face_normals_and_areas,
 * geo_operations.py:529-559) and the unit normals of its vertices; contract in DESIGN.md "Mesh normals".  fp32 vertices
 * (B,N,3); faces (Bt,F,3) int64 and start (Bt,N+1), codes (Bt,3F), nbr (Bt,3F,2) as pp_mesh_corner_incidence made them
 * for L == 3.  shared_topology != 0: they have one batch element, read by every b; gradients and outputs are always per
 * batch element.  Every entry returns PP_EINVAL where B*N, B*F or 3F exceeds 2^31 - 1 or a size is negative, before any
 * launch, and PP_OK without a launch where B, N or F is 0.
 * pp_mesh_face_normals_forward_f32: with p_k = vertices[b, faces[f,k]], c = (p1-p0) x (p2-p1), the products a*b - c*d
 *   with explicit fused multiply-adds (Kahan's difference of products); len = sqrtf((cx*cx + cy*cy) + cz*cz);
 *   areas (B,F) = len * 0.5f; normals (B,F,3) = c / max(len, 1e-12f).
 * pp_mesh_face_normals_backward_f32: grad_vertices (B,N,3), overwritten: every vertex walks its slice in slot order;
 *   the slot 3f + c gives p0, p1, p2 from (the vertex, next, prev) and c, the forward chain is evaluated again, with
 *   u = c / len, G = (g_n - u (u.g_n)) / len + (g_a * 0.5f) u the slot adds (v_next - v_prev) x G; plain fp32 sums from
 *   +0.  A face with len <= 1e-12f adds 0.  grad_normals (B,F,3) or grad_areas (B,F) may be NULL (taken as 0).
 * pp_mesh_vertex_normals_forward_f32: out (B,N,3): S = sum over the vertex's slots in order of w(c), c = (v_next - v_i)
 *   x (v_prev - v_i); weighting 0 ("area") w(c) = c, 1 ("uniform") w(c) = c / max(|c|, 1e-12f);
 *   out = S / max(|S|, 1e-12f); a vertex without corners gives +0.  Anything else for weighting is PP_EINVAL.
 * pp_mesh_vertex_normals_backward_f32: grad_vertices (B,N,3), overwritten, in two launches: (a) per vertex S again and
 *   h = (g - n (n.g)) / |S|, n = S / |S|, 0 where |S| <= 1e-12f, into scratch (B,N,3) fp32, the caller's, not
 *   grad_vertices; (b) per vertex over its slots H = (h_i + h_next) + h_prev, for weighting 1 H <- (H - u (u.H)) / |c|
 *   with u = c / |c| (0 where |c| <= 1e-12f), and the slot adds (v_next - v_prev) x H.
 * No floating-point atomics: every word is written once, identical on every run.  A neighbour outside [0,N) (the build
 * stores -1), a face index outside [0,N) and a slot code >= 3F are only compared, never used as an address: the lane's
 * results are NaN. */
int pp_mesh_face_normals_forward_f32(const float* vertices, const long long* faces, float* normals, float* areas, int B,
                                     int N, int F, int shared_topology, void* stream);
int pp_mesh_face_normals_backward_f32(const float* vertices, const int* start, const int* nbr, const unsigned* codes,
                                      const float* grad_normals, const float* grad_areas, float* grad_vertices, int B,
                                      int N, int F, int shared_topology, void* stream);
int pp_mesh_vertex_normals_forward_f32(const float* vertices, const int* start, const int* nbr, float* out, int B,
                                       int N, int F, int weighting, int shared_topology, void* stream);
int pp_mesh_vertex_normals_backward_f32(const float* vertices, const int* start, const int* nbr, const float* grad_out,
                                        float* scratch, float* grad_vertices, int B, int N, int F, int weighting,
                                        int shared_topology, void* stream);

/* ---- mesh surface sampling -------------------------------------------------------------------
 * Area-weighted samples on a triangle mesh's surface and their re-evaluation on a deformed mesh; contract in DESIGN.md
 * "Mesh surface sampling".  fp32 vertices (B,N,3); faces (Bt,F,3) int64 and start, nbr, codes as in "mesh normals";
 * shared_topology != 0: they have one batch element, read by every b.  Every entry returns PP_EINVAL where B*N, B*F,
 * B*S or 3F exceeds 2^31 - 1 or a size is negative, before any launch, and PP_OK without a launch where a size it works
 * on is 0.
 * pp_mesh_sample_cdf_f32: cdf (B,F) fp64 = the inclusive prefix sum of the fp32 areas (B,F) in fp64, one workgroup per
 *   batch element with a fixed association: the same bytes on every run.
 * pp_mesh_sample_forward_f32: one launch, one lane per sample, in one of two forms.  cdf != NULL: u holds u_stride
 *   floats per sample, (u1) or (u1,u2,u3); target = double(u1) * cdf[b,F-1], face = the first f with cdf[b,f] > target,
 *   su = sqrtf(u2), bary = (1 - su, su * (1 - u3), su * u3); where cdf[b,F-1] is not a positive finite number (or no f
 *   is beyond target) face = -1 and bary is NaN; face_out (B,S) int64 and bary_out (B,S,3) receive them (either may be
 *   NULL; u_stride == 1 serves face_out alone, points == NULL).  cdf == NULL: face_in (B,S) int64 and bary_in (B,S,3)
 *   are the caller's.  points (B,S,3), d = 0..2: (w0*p0_d + w1*p1_d) + w2*p2_d with p_k = vertices[b, faces[face,k]],
 *   every operation rounded on its own.  normals (B,S,3), with face_normals (B,F,3), both or neither NULL:
 *   face_normals[b,face].  A face outside [0,F) and a vertex index outside [0,N) are only compared: points and normals
 *   of that sample are NaN.
 * pp_mesh_sample_backward_f32: grad_vertices (B,N,3), overwritten, from grad_points and grad_normals (B,S,3; one of
 *   them may be NULL).  Builds the face -> sample lists of (face, B, F, S) in `workspace` (at least
 *   pp_mesh_edges_workspace_bytes(B, F, S) bytes), sorted; per face gC[c] = sum over its samples in ascending order of
 *   bary[c] * grad_points and gN = sum of grad_normals, plain fp32 additions from +0 by one lane, and for a list of
 *   more than 256 samples by a workgroup of 512 lanes: lane t adds the entries t, t+512, ... in order, then a fixed
 *   tree over the lanes of a wave and the waves in order; per vertex the sum of gC over its corner slice in slot order,
 *   plus pp_mesh_face_normals_backward_f32's result for gN.  scratch: fp32, 9*B*F floats, and with grad_normals
 *   3*B*F + 3*B*N more; the caller's, not grad_vertices.  A sample with face outside [0,F) and a face with a vertex
 *   index outside [0,N) add nothing; a slot code >= 3F gives NaN.  No floating-point atomics: identical on every run. */
int pp_mesh_sample_cdf_f32(const float* areas, double* cdf, int B, int F, void* stream);
int pp_mesh_sample_forward_f32(const float* vertices, const long long* faces, const double* cdf, const float* u,
                               int u_stride, const long long* face_in, const float* bary_in, const float* face_normals,
                               long long* face_out, float* bary_out, float* points, float* normals, int B, int N, int F,
                               int S, int shared_topology, void* stream);
int pp_mesh_sample_backward_f32(const float* vertices, const long long* faces, const int* start, const int* nbr,
                                const unsigned* codes, const long long* face, const float* bary,
                                const float* grad_points, const float* grad_normals, float* scratch,
                                float* grad_vertices, int B, int N, int F, int S, int shared_topology, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- point-to-mesh distances -----------------------------------------------------------------
 * The exact squared distance between a cloud and a triangle mesh, every (point, triangle) pair walked; contract in
 * DESIGN.md "Point-to-mesh distances".  fp32 points (B,P,3) and vertices (B,N,3); faces (Bt,F,3) int64;
 * shared_topology != 0: faces have one batch element, read by every b.  Every entry returns PP_EINVAL where B*N, B*F,
 * B*P or 3F exceeds 2^31 - 1 or a size is negative, before any launch, and PP_OK without a launch where a size it works
 * on is 0.
 * The pair function of point p and triangle (a,b,c), fp32 with every operation rounded on its own, dot(u,v) =
 *   (ux*vx + uy*vy) + uz*vz: ab = b-a, ac = c-a, ap = p-a, bp = p-b, cp = p-c, d1 = ab.ap, d2 = ac.ap, d3 = ab.bp,
 *   d4 = ac.bp, d5 = ab.cp, d6 = ac.cp, vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4.  The first of
 *   these that holds gives the weights: (1) d1 <= 0 and d2 <= 0: (1,0,0); (2) d3 >= 0 and d4 <= d3: (0,1,0);
 *   (3) vc <= 0, d1 >= 0, d3 <= 0: t = d1/(d1-d3), (1-t,t,0); (4) d6 >= 0 and d5 <= d6: (0,0,1); (5) vb <= 0, d2 >= 0,
 *   d6 <= 0: t = d2/(d2-d6), (1-t,0,t); (6) va <= 0, d4-d3 >= 0, d5-d6 >= 0: t = (d4-d3)/((d4-d3)+(d5-d6)), (0,1-t,t);
 *   (7) t = 1/((va+vb)+vc), v = vb*t, w = vc*t, ((1-v)-w, v, w).  q_d = (w0*a_d + w1*b_d) + w2*c_d, r = p - q,
 *   d = (rx*rx + ry*ry) + rz*rz.
 * pp_mesh_distance_records_f32: records (B,F,16) fp32, 16-byte aligned: a, b, c, ab, ac of every face and a validity
 *   word, 1 or, for a face with a vertex index outside [0,N) (only compared, never used as an address), 0.
 * pp_mesh_point_face_forward_f32: one lane per point: from best = +inf, face = -1 the pairs f = 0, 1, ... in order, one
 *   taken where d < best (the lowest face among equal distances; never a NaN; never a face whose validity word is 0).
 *   dist (B,P), face (B,P) int64, bary (B,P,3) the weights of the pair taken; face = -1 leaves dist and bary NaN.
 * pp_mesh_face_point_forward_f32: the same with the roles exchanged, one lane per face over the points i = 0, 1, ...:
 *   dist (B,F), point (B,F) int64, bary (B,F,3).
 * pp_mesh_distance_backward_f32: one lane per item, the items being the points (item_point == NULL: item s is point s
 *   with the face item_face[b,s]) or the faces (item_face == NULL: item s is face s with the point item_point[b,s]);
 *   exactly one of the two is NULL.  With q interpolated again from bary (B,S,3) and r = p - q: vec (B,S,3) =
 *   (2*grad_dist) * r, neg (B,S,3) = -vec, face_out (B,S) int64 = the item's face; each of the three may be NULL, not
 *   both vec and neg.  An item whose face is outside [0,F), whose point is outside [0,P) or whose face holds a vertex
 *   index outside [0,N) gives +0 and face_out = -1.  grad_points (B,P,3), with item_point only, not vec: builds the
 *   point -> face lists in `workspace` (at least pp_mesh_edges_workspace_bytes(B, P, F) bytes), sorted, and per point
 *   adds vec over its faces in ascending order, plain fp32 additions from +0.  The vertices' gradient is
 *   pp_mesh_sample_backward_f32's for (face or face_out, bary, grad_points = neg).  No floating-point atomics:
 *   identical on every run. */
int pp_mesh_distance_records_f32(const float* vertices, const long long* faces, float* records, int B, int N, int F,
                                 int shared_topology, void* stream);
int pp_mesh_point_face_forward_f32(const float* points, const float* records, float* dist, long long* face,
                                   float* bary, int B, int P, int F, void* stream);
int pp_mesh_face_point_forward_f32(const float* points, const float* records, float* dist, long long* point,
                                   float* bary, int B, int P, int F, void* stream);
int pp_mesh_distance_backward_f32(const float* points, const float* vertices, const long long* faces,
                                  const long long* item_face, const long long* item_point, const float* bary,
                                  const float* grad_dist, float* vec, float* neg, long long* face_out,
                                  float* grad_points, int B, int N, int F, int P, int shared_topology, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---- mesh winding numbers and signed distance --------------------------------------------------
 * The winding number of a triangle mesh about every point of a cloud, every (point, triangle) pair walked, alone or
 * in the same walk as pp_mesh_point_face_forward_f32's choice; contract in DESIGN.md "Mesh winding numbers and signed
 * distance".  fp32 points (B,P,3); records (B,F,16) are pp_mesh_distance_records_f32's, 16-byte aligned.  Both entries
 * return PP_EINVAL where B*F, B*P or 3F exceeds 2^31 - 1 or a size is negative, before any launch, and PP_OK without a
 * launch (and without a write) where B, P or F is 0.
 * The half solid angle of point p and triangle (a,b,c), fp32 with every operation rounded on its own, dot(x,y) =
 *   (x0*y0 + x1*y1) + x2*y2: u = a-p, v = b-p, w = c-p, lu = sqrt(dot(u,u)), lv, lw likewise, x = cross(v,w) with
 *   x0 = v1*w2 - v2*w1, x1 = v2*w0 - v0*w2, x2 = v0*w1 - v1*w0, det = dot(u,x),
 *   den = (((lu*lv)*lw + dot(u,v)*lw) + dot(v,w)*lu) + dot(w,u)*lv, h = atan2f(det, den).
 * Per point the halves of the faces f = 0, 1, ... whose validity word is not 0 are added in fp64 in that order from +0,
 *   and winding = (float)(sum / (2 pi)), rounded once: +1 inside a closed mesh whose faces are oriented outwards, 0
 *   outside, negated by flipping the faces, a fraction for an open mesh, NaN for a NaN point (with a valid face).
 * pp_mesh_winding_forward_f32: winding (B,P).
 * pp_mesh_signed_distance_forward_f32: winding (B,P) with the same bits, and dist (B,P), face (B,P) int64, bary (B,P,3)
 *   with pp_mesh_point_face_forward_f32's bits, from one walk.
 * No atomics: every output word is written once, identical on every run. */
int pp_mesh_winding_forward_f32(const float* points, const float* records, float* winding, int B, int P, int F,
                                void* stream);
int pp_mesh_signed_distance_forward_f32(const float* points, const float* records, float* dist, long long* face,
                                        float* bary, float* winding, int B, int P, int F, void* stream);

/* ---- earth mover's distance ------------------------------------------------------------------
 * The approximate matching of Fan, Su and Guibas (2017) between fp32 clouds xyz1 (B,N,3) and xyz2 (B,M,3), every pair
 * walked in every round; contract in DESIGN.md "Earth mover's distance".  No counterpart in the reference.
 * d_kl = (dx*dx + dy*dy) + dz*dz; multiL = max(N,M)/N, multiR = max(N,M)/M (integer division); L = 10 levels,
 * level_j = -4^(7-j) for j = 0..8 and level_9 = 0; exp(level*d) is exp2 of d * (level * log2 e).  From remainL = multiL,
 * remainR = multiR, per level: a[k] = remainL[k] / (1e-9 + sum_l exp(level d) remainR[l]); s[l] = (sum_k exp(level d)
 * a[k]) remainR[l]; b[l] = min(remainR[l] / (s[l] + 1e-9), 1) remainR[l]; remainR[l] = max(0, remainR[l] - s[l]);
 * remainL[k] = max(0, remainL[k] - a[k] sum_l exp(level d) b[l]).  The match is never stored:
 * match[k,l] = sum_j (exp(level_j d_kl) a_j[k]) b_j[l], j ascending, xyz1 along the rows.
 * Every sum over N or M is four partial sums over the indices = 0, 1, 2, 3 (mod 4), each ascending from +0, added as
 * ((p0 + p1) + p2) + p3.  No floating-point atomics: identical on every run.  No loop bound or address depends on the
 * data; what NaN or infinite coordinates give is outside the contract.
 * Every entry returns PP_EINVAL where a size is negative or B*N or B*M exceeds 2^31 - 1, before any launch, and PP_OK
 * without a launch (and without a write) where B, N or M is 0.  N*M itself may exceed 2^31.
 * pp_emd_workspace_bytes: host arithmetic; the bytes pp_emd_match_f32 and pp_emd_cost_f32 need, 0 for a refused shape.
 * pp_emd_match_f32: the factors a (B,10,N) and b (B,10,M), twenty launches.
 * pp_emd_dense_f32: match (B,N,M) from the factors, indexed in 64 bits.
 * pp_emd_cost_f32: cost (B,) = sum_kl match[k,l] sqrt(d_kl); the rows' sums go through `workspace` and are added per
 *   batch element by lane t over the rows t, t + 256, ... and a binary tree over the 256 lanes.
 * pp_emd_cost_backward_f32: the match held constant: grad_xyz1[k] = grad_cost[b] * sum_l (match[k,l] / max(sqrt(d_kl),
 *   1e-20)) (xyz1_k - xyz2_l), grad_xyz2[l] the same over k with (xyz2_l - xyz1_k); overwritten; either may be NULL. */
size_t pp_emd_workspace_bytes(int B, int N, int M);
int pp_emd_match_f32(const float* xyz1, const float* xyz2, float* a, float* b, int B, int N, int M, void* workspace,
                     size_t workspace_bytes, void* stream);
int pp_emd_dense_f32(const float* xyz1, const float* xyz2, const float* a, const float* b, float* match, int B, int N,
                     int M, void* stream);
int pp_emd_cost_f32(const float* xyz1, const float* xyz2, const float* a, const float* b, float* cost, int B, int N,
                    int M, void* workspace, size_t workspace_bytes, void* stream);
int pp_emd_cost_backward_f32(const float* xyz1, const float* xyz2, const float* a, const float* b,
                             const float* grad_cost, float* grad_xyz1, float* grad_xyz2, int B, int N, int M,
                             void* stream);

/* The library also exports pp_debug_set_* switches that force one kernel variant or another; they
 * exist for the parity tests and for tuning and are deliberately not declared here. */

/* cuda_utils.h:11-16 opt_n_threads -- the FPS tie-break depends on it, so it is part of the ABI */
int pp_opt_n_threads(int work_size);

/* ---- batch-sharded execution (no counterpart in the reference, which has no multi-GPU code):
 * packing of a rank's Chamfer outputs for ONE collective per step, and unpacking of the gathered
 * buffer (pytorch_points_amd/sharded.py PackedShardGather).  n1 = B_local*N, n2 = B_local*M.
 * Packed layout: dist1 | dist2 | idx1 | idx2, indices as uint16 when compact != 0 (all < 65536).
 * pp_shard_packed_bytes: bytes of one rank's packed buffer (multiple of 16 = the row stride).
 * pp_shard_pack_f32 with dist1 == dist2 == NULL: the distances are IN PLACE already -- the caller gave the packed
 * buffer's first n1 + n2 floats to pp_nmdistance_forward*_f32 as its dist1 / dist2 outputs -- and only the indices are
 * narrowed in behind them.  pp_shard_unpack_f32 with dist1 == dist2 == NULL: indices only (the distances are read where
 * they were gathered, as strided views of the gathered buffer). */
size_t pp_shard_packed_bytes(long long n1, long long n2, int compact);
int pp_shard_pack_f32(const float* dist1, const float* dist2, const int* idx1, const int* idx2, void* packed,
                      long long n1, long long n2, int compact, void* stream);
int pp_shard_unpack_f32(const void* gathered, int world, long long stride_bytes, long long n1, long long n2,
                        int compact, float* dist1, float* dist2, int* idx1, int* idx2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PP_HIP_H */
