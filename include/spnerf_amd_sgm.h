/* Semi-global aggregation exports of libspnerf_amd.so (gfx950): the plane sweep's score volume
 * (spnerf_amd_sweep.h) regularised across cells before the pick, after Hirschmüller (2008).  The
 * sweep picks each cell's plane on its own; here the cost of every (cell, plane) is aggregated along
 * 4 or 8 scanline directions with a small penalty p1 for a change of one plane between neighbouring
 * cells and a larger one p2 for a jump, the directions are averaged, and the sweep's pick runs on
 * the result.  Occlusion is not modelled, p2 does not follow the image gradients, and cells without
 * any scored plane stay without an altitude (no hole filling).
 * A separate header so that the ABIs of spnerf_amd.h and its siblings stay as they are; the
 * conventions are those of spnerf_amd_sweep.h: every function returns SPNERF_OK or a negative
 * SPNERF_E_* code with the text in spnerf_last_error, pointers are device pointers, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics — results are
 * bit-reproducible from run to run.
 *
 * THE DEFINITION.  Everything below is fp32, every sum and difference is rounded once (nothing is
 * fused), in exactly the stated order.  The inputs are taken to be of a size at which no sum
 * overflows.
 *
 * Inputs: volume [K][H][W] fp32, scores of which higher is better, NaN or ±inf meaning unscored;
 * 1 <= K <= 512; H, W > 0 with H·W <= 2^32; penalties p1, p2, finite, 0 <= p1 <= p2; `unscored`,
 * finite, the cost of an unscored entry (1.0 is a ZNCC of 0); paths, 4 or 8.
 *
 * Cost.  C(p,k) = 1.0f - volume(p,k) where the score is finite, else `unscored`.  It is finite at
 * every cell and plane: a cell without any scored plane still carries paths through it, with a flat
 * cost.
 *
 * Directions, as (dj, di) steps — rows, columns — from the previous cell q to p = q + r, in this
 * order: (0,+1), (0,-1), (+1,0), (-1,0), (+1,+1), (-1,-1), (+1,-1), (-1,+1).  paths = 4 takes the
 * first four.
 *
 * Recurrence along direction r.  If q = p - r lies outside the grid, L_r(p,k) = C(p,k).  Otherwise
 * let M = min over k of L_r(q,k), and m the minimum of
 *   L_r(q,k);  L_r(q,k-1) + p1 (only if k >= 1);  L_r(q,k+1) + p1 (only if k <= K-2);  M + p2,
 * each sum rounded to fp32, the minimum exact (no NaN can occur).  Then
 *   L_r(p,k) = C(p,k) + (m - M):  the difference is rounded, then the sum.
 *
 * Aggregate.  S = L_0; S = S + L_1; ... in direction order, one rounding per addition;
 *   out(p,k) = 1.0f - S·(1/paths),
 * the product exact (1/paths is 0.25 or 0.125), so one rounding.  out is NaN at every plane of a
 * cell that has no finite score at any plane.  out is on the score scale — with p2 = 0 it is the
 * score again, up to rounding — and is a volume the pick takes unchanged.
 *
 * Pick.  Exactly the pick of spnerf_amd_sweep.h over the aggregated volume: index the lowest plane
 * with the largest non-NaN value, -1 where there is none; altitude moved to the vertex of the
 * parabola through its two neighbours; score the aggregated value at index.  In addition
 *   photo = the raw score volume(p, index) where it is finite, NaN where it is not or index is -1.
 * There is no `views` output: the fused sweep writes no per-plane view counts.
 */
#ifndef SPNERF_AMD_SGM_H
#define SPNERF_AMD_SGM_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_SGM_ABI_VERSION 1
#define SPNERF_SGM_MAX_PLANES 512
#define SPNERF_SGM_TILE 64 /* the transposing kernels move tiles of TILE cells x TILE planes through LDS */

int32_t spnerf_sgm_abi_version(void);

/* The bytes of workspace spnerf_sgm_aggregate needs for these sizes; the library allocates nothing.
 * (1 + paths) cell-major volumes [H·W][K] fp32 — the cost and one L_r per direction — and one byte
 * per cell. */
int32_t spnerf_sgm_workspace_bytes(int32_t n_planes, int32_t ysize, int32_t xsize, int32_t paths, int64_t* bytes);

/* The aggregation.  Three launches: the cost, transposed to cell-major through LDS tiles; every
 * direction's recurrence, one wavefront per path with its lanes over the planes; the sum over the
 * directions in their order, transposed back.
 *   volume     [n_planes][ysize][xsize] fp32
 *   out        [n_planes][ysize][xsize] fp32; must not overlap volume
 *   workspace  at least spnerf_sgm_workspace_bytes, 4-byte aligned; must overlap neither */
int32_t spnerf_sgm_aggregate(const float* volume, int32_t n_planes, int32_t ysize, int32_t xsize, float p1, float p2,
                             float unscored, int32_t paths, float* out, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* The pick over the aggregated volume, one thread per cell, and the raw score there.
 *   aggregated, volume  [n_planes][cells] fp32
 *   altitude, score, photo [cells] fp32; index [cells] int32 */
int32_t spnerf_sgm_pick(const float* aggregated, const float* volume, int32_t n_planes, int64_t cells, double alt_lo,
                        double step, float* altitude, float* score, int32_t* index, float* photo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_SGM_H */
