// Ablation half of launch_nt16d (gemm_bf16.hip, included there under SPN_ABLATIONS): the DMA NT
// GEMM's other issue placements of the next K-step (options nt_bf16_ip, nt_bf16_ip_gen).  Returns
// whether it launched; the default placement is launch_nt16d's own.
template <bool DM, int EV, bool HD>
static bool abl_launch_nt16d(int ip, dim3 grid, dim3 block, hipStream_t s, const NT16Args& a, int nt) {
    if (ip == 3) {
        hipLaunchKernelGGL((k_gemm_nt_bf16d<DM, 3, EV, HD>), grid, block, 0, s, a, nt);
        return true;
    }
    if (ip == 1) {
        hipLaunchKernelGGL((k_gemm_nt_bf16d<DM, 1, EV, HD>), grid, block, 0, s, a, nt);
        return true;
    }
    if (ip == 0) {
        hipLaunchKernelGGL((k_gemm_nt_bf16d<DM, 0, EV, HD>), grid, block, 0, s, a, nt);
        return true;
    }
    return false;
}
