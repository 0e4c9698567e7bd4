/*
 * pp_hip_debug.h -- test and benchmark knobs of libpp_hip.so.  NOT part of the drop-in C ABI (pp_hip.h).
 *
 * Every operator of pp_hip.h picks its kernel variant from the problem size.  The functions below override
 * that choice process-wide so that tests can compare the variants with each other bit for bit and benchmarks
 * can time them; 0 always restores the automatic choice.  They are the library's only global mutable state
 * besides idempotent per-device "LDS limit raised" flags: each is one relaxed std::atomic<int>, safe to set
 * from any thread, read by the next call of the operator.  Product code (pytorch_points_amd/network, _ext)
 * never calls them.
 */
#ifndef PP_HIP_DEBUG_H
#define PP_HIP_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* Chamfer forward: 0 automatic, 1 brute force (every pair), 2 grid search wherever structurally possible */
void pp_debug_set_nmdistance_search(int mode);
/* brute-force kernel form (chamfer.hip).  C == 3: 0 automatic, which takes one of 1 = <Q 1 query per lane, G 8 points
 * per group>, 1002 = <2, 8, packed fp32>, 1416 = <4, 16, packed>; any other value makes the forward return PP_EINVAL.
 * C != 3: 9 = the one-lane-per-query kernels, any other value automatic */
void pp_debug_set_nmdistance_variant(int variant);
/* grid search, unlabeled: 0 = the stage-A kernel, then the list kernel over what it left (default; any other value
 * means this too); -1 = no stage-A kernel, the whole-search kernel serves every query */
void pp_debug_set_nmdistance_tile(int mode);
/* grid search, unlabeled: the build of sets of at most 16384 aligned points: 0 = sorted through the LDS, a slab owning
 * whole z-layers (default), 1 = the general build always (tests and A/B timing) */
void pp_debug_set_nmdistance_build(int general);
/* grid search, unlabeled: directions no search can prune (every reference point at nearly one distance from the queries)
 * are routed to the every-pair kernel, launched behind the search once an earlier call on the device has routed one:
 * 0 = that, 1 = never (the search serves every direction), 2 = the every-pair launch always follows */
void pp_debug_set_nmdistance_routing(int mode);
/* grid search, unlabeled: the far-field (group) search of the list kernel skips the cell rows that hold no points by a
 * per-set row bitmap written in the stage-A launch's tail: 0 = that (default), 1 = every row is looked up (tests, A/B) */
void pp_debug_set_nmdistance_row_bitmap(int off);
/* labeled Chamfer brute force: 1 = the one-lane-per-query kernel */
void pp_debug_set_labeled_variant(int variant);
/* Chamfer backward: 0 automatic (double LDS accumulators for C == 3 from N + M = 4096), 1 global atomics, 2 LDS fp32
 * columns; any other value means 0.  (The deterministic form, the ordered CSR lists, is an entry point of its own,
 * pp_nmdistance_backward_ordered_f32.) */
void pp_debug_set_nmdistance_backward_variant(int variant);
/* per-kernel HIP-event timing of the grid forward, read back after the call: the build and the search's two launches
 * (stage A by tiles, then what it left); stage_a_ms = 0 without a stage-A kernel */
void pp_debug_set_nmdistance_kernel_timing(int on);
int pp_debug_nmdistance_kernel_ms3(float* build_ms, float* stage_a_ms, float* rest_ms);

/* ... and the build's and the stage-A kernel's OWN durations of the most recent forward timed with the knob at 2 (the
 * launches' begin / end stamps, hipExtLaunchKernelGGL: what rocprofv3 reports per dispatch) */
int pp_debug_nmdistance_kernel_own_ms(float* build_ms, float* stage_a_ms);

/* unlabeled grid forward: queries its stage-A kernel left to the list kernel, per direction (2 B values; synchronises) */
int pp_debug_nmdistance_pending(const void* workspace, int B, int N, int M, unsigned* totals);

void pp_debug_set_fps_v1(int form); /* 0 = the library's choice, 1 = one workgroup per batch element over all points,
                                      * 2 = the CU cluster over all points, 3 = the bucketed kernel */
/* the bucketed FPS kernel's serial chain (N <= 65536): 0 = the library's choice (several mutually independent picks
 * per barrier round from 32768 points or 1024 picks, one pick per round below), 1 = one pick per round, 2 = several per round */
void pp_debug_set_fps_bucket_chain(int form);
/* the bucketed FPS kernel's sort: 0 = by the whole chip from 32768 points (six short launches in front of the kernel),
 * below that inside the kernel by its one workgroup; 1 = always inside the kernel */
void pp_debug_set_fps_bucket_sort(int mode);
/* gather_points forward: 0 automatic, 1 the global-gather kernel; 2 = the 16-bit dispatch (pp_gather_forward_b16) takes
 * its LDS form wherever the row fits (the fp32 dispatch reads 2 as 0) */
void pp_debug_set_gather_variant(int variant);
void pp_debug_set_ball_query_variant(int variant); /* scan kernels: 1 = one wave per 64 centres */
void pp_debug_set_ball_query_search(int mode);     /* 0 automatic, 1 scan, 2 grid wherever possible */
void pp_debug_set_ball_query_lpc(int lanes_per_centre);
/* group_points: 0 automatic, 1 the global-gather kernel, 2 / 4 / 8 the VGPR-staged LDS kernel with that many index
 * quads per thread, 604 / 608 / 616 the LDS-DMA kernel with 4 / 8 / 16 quads where the positions fill whole chunks (the
 * VGPR-staged one elsewhere); any other value above 100: no LDS-DMA kernel.  The 16-bit dispatch
 * (pp_group_points_strided_b16) reads the same values: 604 / 608 / 616 its LDS-DMA kernel with 2 / 4 / 8 index OCTETS
 * (the same chunks of positions), 2 / 4 / 8 and the other values above 100 its one register-staged LDS kernel; a value
 * that names an LDS form takes it below the automatic choice's 256 * 2048 positions as well (aligned shapes only) */
void pp_debug_set_group_points_variant(int variant);
/* group_points_grad: 0 automatic, 1 no double LDS column (fp32 without a sorted form: global atomics), 2 the double
 * LDS column also below 4096 positions; any other value means 0.  One policy reads it for fp32 and 16-bit tensors: 2
 * lowers the column's floor and leaves the sorted form its precedence for short lists of big problems */
void pp_debug_set_group_points_grad_variant(int variant);
void pp_debug_set_three_nn_search(int mode);       /* 0 automatic, 1 scan */
/* three_interpolate: 0 automatic, 1 the global-gather kernel, 2 no channel-group form (fp32: the row-at-a-time LDS form
 * where it applies; 16-bit: the global form); 3 = the 16-bit dispatch takes its channel-group form wherever the rows
 * fit (the fp32 dispatch reads 3 as 0) */
void pp_debug_set_three_interpolate_variant(int variant);
/* three_interpolate_grad: 0 automatic, 1 and 3 no double LDS column (fp32: the sorted form for big problems with a
 * workspace, else global atomics; 16-bit: the sorted form), 2 the double LDS column also below 2048 points */
void pp_debug_set_three_interpolate_grad_variant(int variant);
/* 1 = never use the sorted scatter-add form (the ordered form of deterministic mode is not a choice and stays) */
void pp_debug_set_scatter_mode(int mode);
/* The form the scatter-add backwards' one policy (sampling.hip: scatter_plan) picks for a described call under the
 * three knobs above as they stand: pure host arithmetic, no HIP call.  op and the result are the values below;
 * elem_bytes 4 = fp32, 2 = f16 / bf16; write: the entry WRITES its output (*_out_ws_*) rather than accumulating -- the
 * form does not depend on it, the zero fill in front of an accumulating form does; ordered: an *_ordered_* entry or
 * the 16-bit entries' flag; sources per batch element: M of gather_backward, npoint * nsample of group_points_grad, N
 * of three_interpolate_grad; destinations: N, N, M; workspace_bytes: what the caller passes beside a non-null
 * workspace (0: none).  PP_SCATTER_FORM_NONE is the entry's PP_ENOTSUP.  -1: the arguments describe no call (unknown
 * op or element size, a size <= 0: the entries serve those before any form is chosen) */
enum { PP_SCATTER_GATHER = 0, PP_SCATTER_GROUP = 1, PP_SCATTER_INTERPOLATE = 2 };
enum {
  PP_SCATTER_FORM_NONE = 0,
  PP_SCATTER_FORM_ATOMICS = 1, /* global atomicAdd (fp32 only) */
  PP_SCATTER_FORM_COLUMN = 2,  /* double accumulators in the LDS */
  PP_SCATTER_FORM_SORTED = 3,  /* sorted triples in the workspace */
  PP_SCATTER_FORM_ORDERED = 4  /* sorted triples, ascending source order per destination */
};
int pp_debug_scatter_plan(int op, int elem_bytes, int write, int ordered, int B, int C, long long sources,
                          int destinations, size_t workspace_bytes);
void pp_debug_set_knn_search(int mode);            /* 0 automatic, 1 scan */
/* a pure streaming store of `bytes` (16-byte stores, non-temporal or plain, `workgroups` x 1024 threads): the store
 * ceiling bench.py reports beside group_points (roofline.peak_measured) */
int pp_debug_store_ceiling(void* buf, size_t bytes, int nontemporal, int workgroups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PP_HIP_DEBUG_H */
