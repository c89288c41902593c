    // The ablation build's entries of option_slot (options.cpp, included there under SPN_ABLATIONS).
    // A/B switches of kernels measured slower than the defaults (DESIGN.md §6, Appendix B) and
    // profiling ablations whose outputs are INVALID: only in a -DSPN_ABLATIONS build
    // (make -C sp-nerf_amd variant VDEF=-DSPN_ABLATIONS VLIB=libspnerf_amd_abl.so)
    if (n == "trunk_dbg") return &g_trunk_dbg;
    if (n == "trunk_var") return &g_trunk_var;
    if (n == "heads_dbg") return &g_heads_dbg;
    if (n == "trunk_nt") return &g_trunk_nt;
    if (n == "trunk_dreg") return &g_trunk_dreg;
    if (n == "trunk_bwd_dreg") return &g_trunk_bwd_dreg;
    if (n == "trunk_bwd_nt") return &g_trunk_bwd_nt;
    if (n == "trunk_sigma") return &g_trunk_sigma;
    if (n == "tn_f32_variant") return &g_tn_variant;
    if (n == "nt_bf16_variant") return &g_nt16_variant;
    if (n == "nt_bf16_ip") return &g_nt16_ip;
    if (n == "tn_bf16_ip") return &g_tn16_ip;
    if (n == "tn_bf16_bias_split") return &g_tn16_bias_split;
    if (n == "tn_bf16_few_tiles") return &g_tn16_few_tiles;
    if (n == "tn_bf16_pf") return &g_tn16_pf;
    if (n == "tn_bf16_quad") return &g_tn16_quad;
    if (n == "tn_bf16_m16") return &g_tn16_m16;
    if (n == "tn_bf16_rounds") return &g_tn16_rounds;
    if (n == "tn_group_rounds") return &g_tn_group_rounds;
    if (n == "tn_k64_pair") return &g_tn_k64_pair;
    if (n == "ray_tiles_pair") return &g_ray_tiles_pair;
    if (n == "nt_bf16_ip_gen") return &g_nt16_ip_gen;
    if (n == "nt_bf16_epi") return &g_nt16_epi;
    if (n == "grad_marks_flags") return &g_marks_flags;
    if (n == "heads_variant") return &g_heads_variant;
    if (n == "l0_split") return &g_l0_split;
    if (n == "bwd_streams") return &g_bwd_streams;
    if (n == "tn_bf16_min_points") return &g_tn16_min_points;
    if (n == "fused_heads") return &g_fused_heads;
    if (n == "zsave") return &g_zsave;
    if (n == "tn_split_tail") return &g_tn_split_tail;
    if (n == "tile_rowsum") return &g_tile_rowsum;
    if (n == "trunk2") return &g_trunk2;
    if (n == "trunk2_tile") return &g_trunk2_tile;
    if (n == "emu_bf16") return &g_emu_bf16;
