// Ablation half of launch_tn_bf16d (gemm_bf16.hip, included there under SPN_ABLATIONS): the
// weight-gradient kernels of gemm_tn_bf16_variants.inc (options tn_bf16_m16, tn_bf16_quad), the
// prefetched-fragment main loop (tn_bf16_pf) and the other issue placements (tn_bf16_ip) of
// k_gemm_tn_bf16d.  Returns whether it launched; the default placement is launch_tn_bf16d's own.
static bool abl_launch_tn_bf16d(const TN16Group& G, int ip, dim3 grid, dim3 block, hipStream_t s) {
    if (g_tn16_m16 >= 3) {
        if (g_tn16_m16 == 4) hipLaunchKernelGGL(k_gemm_tn_bf16x<5>, grid, dim3(1024), 0, s, G);
        else hipLaunchKernelGGL(k_gemm_tn_bf16x<4>, grid, dim3(1024), 0, s, G);
        return true;
    }
    if (g_tn16_m16) {
        if (g_tn16_m16 == 2) hipLaunchKernelGGL(k_gemm_tn_bf16m<5>, grid, block, 0, s, G);
        else hipLaunchKernelGGL(k_gemm_tn_bf16m<4>, grid, block, 0, s, G);
        return true;
    }
    if (g_tn16_quad) {
        hipLaunchKernelGGL(k_gemm_tn_bf16q, grid, dim3(256), 0, s, G);
        return true;
    }
    if (g_tn16_pf == 1 || (g_tn16_pf == 2 && G.start[G.n] <= num_cus())) {
        hipLaunchKernelGGL((k_gemm_tn_bf16d<1, true>), grid, block, 0, s, G);
        return true;
    }
    if (ip == 2) {
        hipLaunchKernelGGL(k_gemm_tn_bf16d<2>, grid, block, 0, s, G);
        return true;
    }
    if (ip == 4) {
        hipLaunchKernelGGL(k_gemm_tn_bf16d<4>, grid, block, 0, s, G);
        return true;
    }
    if (ip == 5) {
        hipLaunchKernelGGL(k_gemm_tn_bf16d<5>, grid, block, 0, s, G);
        return true;
    }
    if (ip == 0) {
        hipLaunchKernelGGL(k_gemm_tn_bf16d<0>, grid, block, 0, s, G);
        return true;
    }
    if (ip == 1) {
        hipLaunchKernelGGL(k_gemm_tn_bf16d<1>, grid, block, 0, s, G);
        return true;
    }
    return false;
}
