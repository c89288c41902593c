/* DSM cleaning exports of libspnerf_amd.so (gfx950): what the classical stereo chain does to a raster after
 * the aggregation — a speckle filter that drops small connected regions, a median that removes single
 * cells, and a fill of the holes the two and the sweep leave.  Each takes an (H, W) fp32 raster, row 0 the
 * northernmost, as the sweeps write their altitude, and writes new planes; the input is never written.
 * STAGED: this header lives in include/staged/ (and its ctypes table in _clean_abi.py, outside
 * _lib.BINDING_MODULES) because tests/test_abi_tables.py pins the list of headers in include/; both move to
 * include/spnerf_amd_clean.h / _clean_lib.py in the first change that may touch that test.
 * The conventions are those of spnerf_amd_sgm.h: every function returns SPNERF_OK or a negative code with
 * the text in spnerf_last_error, pointers are device pointers, `stream` is a hipStream_t, nothing is
 * allocated.  spnerf_clean_median and spnerf_clean_fill do not synchronise with the host and use no atomics.
 * spnerf_clean_speckle uses integer atomics (minimum and add) whose results do not depend on the order in
 * which they land, and it waits for its stream before it returns: it reads back the word that says whether a
 * bounded loop ran out (below), so it cannot be captured into a graph.
 *
 * THE DEFINITION.  A cell that is not finite (NaN, +inf, -inf) is a HOLE.  Nothing below rounds: the
 * operations are compares, selections and one exact-or-once-rounded fp32 subtraction that is only compared,
 * so the results are the bytes of the numpy statement (tests/clean_numpy.py).  H, W > 0 and
 * H·W <= 2^31 - 1: a cell's linear index y·W + x is an int32.
 *
 * Speckle.  Two finite cells that are 4-neighbours (east-west or north-south) are JOINED when
 *   fabsf(a - b) <= max_diff
 * with a - b one fp32 subtraction (a difference that overflows to inf joins nothing; NaN compares false).
 * A component is the transitive closure of "joined" — a ramp whose ends are far apart is one component.
 *   label  the smallest linear index y·W + x in the cell's component; -1 at a hole
 *   size   the number of cells in the cell's component; 0 at a hole
 *   out    the input where size > max_size; NaN (0x7fc00000) where 1 <= size <= max_size; the input's own
 *          bytes at a hole, so an inf stays an inf
 * max_diff is finite and >= 0, max_size >= 0 (0 removes nothing).  label is a minimum and size an integer
 * count, so none of the three depends on the order of any atomic.
 *
 * Median.  radius r in 1..3.  Over the (2r+1)^2 window clipped to the grid take the finite values, n of
 * them; the result is the one of rank (n - 1) / 2 in ascending order (the lower median: one of the inputs,
 * never an average) with 0.0f added, so that a zero comes out as +0.  If n < min_count the result is NaN
 * (1 <= min_count <= (2r+1)^2).  At a hole the input's own bytes are copied unless `fill` is 1, in which
 * case the hole gets the same result as any other cell.
 *
 * Fill.  A finite cell is copied and gets filled = 0.  From a hole the input is walked in the eight
 * directions E, NE, N, NW, W, SW, S, SE, in that order (N is towards row 0), each to its first finite cell
 * at most `reach` steps away (1 <= reach <= 4096) or to the grid's edge.  If fewer than min_dirs (1..8)
 * directions found one, the input's own bytes are copied and filled = 0.  Otherwise filled = 1 and
 *   mode 0 (SPNERF_CLEAN_LOWEST)   the minimum of the found values: a later direction replaces an earlier
 *                                  one only when strictly less — the background-preferring rule;
 *   mode 1 (SPNERF_CLEAN_NEAREST)  the value at the smallest squared distance, n^2 on an axis and 2n^2 on
 *                                  a diagonal after n steps (integers); ties go to the earlier direction.
 * The walk reads the input only, so the result does not depend on the order of the cells.
 */
#ifndef SPNERF_AMD_CLEAN_H
#define SPNERF_AMD_CLEAN_H

#include "../spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_CLEAN_ABI_VERSION 1
#define SPNERF_CLEAN_TILE 16 /* the labelling's first pass and the median work on tiles of TILE x TILE cells in LDS */
#define SPNERF_CLEAN_MAX_RADIUS 3
#define SPNERF_CLEAN_MAX_REACH 4096
#define SPNERF_CLEAN_LOWEST 0
#define SPNERF_CLEAN_NEAREST 1
#define SPNERF_CLEAN_E_BOUND (-4) /* a bounded loop of the labelling ran out: a defect, never an input's fault */

int32_t spnerf_clean_abi_version(void);

/* The bytes of workspace spnerf_clean_speckle needs: the union-find's parent plane and the roots' counts,
 * [H·W] int32 each, and 16 bytes that hold the word of the iteration bound. */
int32_t spnerf_clean_workspace_bytes(int32_t ysize, int32_t xsize, int64_t* bytes);

/* The speckle filter.  Union-find on the int32 parent plane, in which a link always points to a smaller
 * index of the same component: (1) one workgroup per tile labels the tile in LDS and writes every cell's
 * tile-local root; (2) one thread per pair of cells across a tile border unites the two with atomicMin;
 * (3) one thread per cell follows its links to the root — the component's smallest index — writes `label`
 * and adds 1 to the root's count, one add per wavefront where the wavefront shares a root; (4) one thread
 * per cell writes `size` and `out`.  Every loop that follows links or retries a union counts its
 * iterations against H·W and refuses a link that does not point downwards; either sets the workspace's
 * last word, and the call then returns SPNERF_CLEAN_E_BOUND after the launches.
 *   dsm        [ysize][xsize] fp32
 *   out        [ysize][xsize] fp32;  label, size  [ysize][xsize] int32;  none may overlap dsm
 *   workspace  at least spnerf_clean_workspace_bytes, 4-byte aligned; overlaps none of the four */
int32_t spnerf_clean_speckle(const float* dsm, int32_t ysize, int32_t xsize, float max_diff, int32_t max_size, float* out,
                             int32_t* label, int32_t* size, void* workspace, int64_t workspace_bytes, void* stream);

/* The median, one workgroup per tile with the tile and its halo staged in LDS once; each thread selects
 * by rank counting over its window.
 *   dsm, out  [ysize][xsize] fp32; must not overlap */
int32_t spnerf_clean_median(const float* dsm, int32_t ysize, int32_t xsize, int32_t radius, int32_t min_count, int32_t fill,
                            float* out, void* stream);

/* The fill, one thread per cell; a finite cell leaves at once.
 *   dsm, out  [ysize][xsize] fp32; filled [ysize][xsize] uint8; neither output may overlap dsm */
int32_t spnerf_clean_fill(const float* dsm, int32_t ysize, int32_t xsize, int32_t reach, int32_t mode, int32_t min_dirs,
                          float* out, uint8_t* filled, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_CLEAN_H */
