// The per-point network's option variables (spnerf_set_option, options.cpp).  Each is defined, with
// its measurement comment, in the unit that reads it.
#pragma once

namespace spn {

extern int g_pack_table;       // pack.hip
extern int g_heads_variant;    // point_kernels.hip
extern int g_bwd_streams;      // grad_marks.hip
// mlp_forward.hip
extern int g_l0_split, g_trunk_l0, g_pe_inline, g_heads_epi, g_zsave;
// mlp_backward.hip
extern int g_ray_tiles_pair;
extern int g_tn_split_tail, g_tn_group, g_tn_group_rounds, g_tn_group_last, g_tn_k64_pair, g_defer_heads;
// these two are internal to the library: not among the symbols it exports
extern int g_marks_flags __attribute__((visibility("hidden")));  // grad_marks.hip
extern int g_tile_rowsum __attribute__((visibility("hidden")));  // mlp_backward.hip

}  // namespace spn
