// spnerf_set_option / spnerf_get_option: the table of named option variables.
#include <string>

#include "common.h"
#include "gemm_bf16.h"
#include "gemm_f32.h"
#include "heads_dx.h"
#include "mlp_options.h"
#include "trunk.h"

using namespace spn;

static int* option_slot(const char* name) {
    const std::string n(name);
    // The product library's switches: the default kernels and their one documented alternate each
    // (INTEGRATION.md §Kernel selection), and two read-backs.
    if (n == "fused_trunk") return &g_fused_trunk;        // 0: layer-by-layer trunk GEMMs
    if (n == "trunk_tile") return &g_trunk_tile;          // 64 / 128-point training tiles
    if (n == "trunk_heads") return &g_trunk_heads;        // 0: inference heads in their own launch
    if (n == "heads_epi") return &g_heads_epi;            // 0: narrow training heads wave-per-point
    if (n == "trunk_l0") return &g_trunk_l0;              // layer 0 inside the fused trunk (1: inference only)
    if (n == "pe_inline") return &g_pe_inline;            // 0: k_encode writes the PE rows
    if (n == "tn_group") return &g_tn_group;              // weight-gradient GEMMs per group launch (1: none)
    if (n == "tn_group_last") return &g_tn_group_last;    // cap of the last group (bench.py: 2 when N > 1)
    if (n == "defer_heads") return &g_defer_heads;        // the heads' weight gradients in the group launch
    if (n == "fused_bwd") return &g_fused_bwd;            // 0: the dX chain layer by layer; 1: row-major D; 2: tile-ordered D; 3: and 128-point chain tiles
    if (n == "trunk_bwd_tile") return &g_trunk_bwd_tile;  // read-back: tile sizes (64 | 128) of the dX chain launches since zeroed
    if (n == "fused_heads_bwd") return &g_fused_heads_bwd;  // 0: the training heads' dX as four GEMMs
    if (n == "heads_bwd_path") return &g_heads_bwd_path;  // read-back: 1 = the fused heads dX ran, 2 = the four GEMMs, since zeroed
    if (n == "tn_bf16_variant") return &g_tn16_variant;   // 1: 128x128 TN tiles, 2: register-staged 256x256
    if (n == "tn_bf16_k64") return &g_tn16_k64;           // 0: N = 512, K = 64 weight gradients on 128x128 tiles
    if (n == "nt_f32_variant") return &g_nt_variant;      // the fp32 (parity) NT GEMM tilings
    if (n == "pack_table") return &g_pack_table;          // 0: one re-pack launch per parameter group
    if (n == "prof_shapes") return &g_prof_shapes;        // in-library timer keyed by launch shape
#ifdef SPN_ABLATIONS
#include "ablations/options.inc"  // the A/B switches and profiling ablations of the ablation build
#endif
    return nullptr;
}

extern "C" int32_t spnerf_set_option(const char* name, int32_t value) {
    SPN_ARG(name != nullptr, "set_option: NULL name");
    int* slot = option_slot(name);
    SPN_ARG(slot != nullptr, "set_option: unknown option '%s'", name);
    *slot = value;
    return SPNERF_OK;
}

extern "C" int32_t spnerf_get_option(const char* name, int32_t* value) {
    SPN_ARG(name != nullptr && value != nullptr, "get_option: NULL pointer");
    int* slot = option_slot(name);
    SPN_ARG(slot != nullptr, "get_option: unknown option '%s'", name);
    *value = *slot;
    return SPNERF_OK;
}
