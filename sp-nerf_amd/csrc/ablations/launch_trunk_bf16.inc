// Ablation half of trunk_bf16's launch (trunk_bf16.hip, included there under SPN_ABLATIONS): the
// profiling instances of k_trunk_bf16 (option trunk_var; outputs invalid) and the measured-slower
// 64-point tiling without the register-D epilogue (option trunk_dreg 0).  Returns whether it
// launched; the product's three instances are trunk_bf16's own.
static bool abl_launch_trunk_bf16(int tm, bool save, dim3 grid, dim3 block, hipStream_t s, const TrunkArgs& ad, int ntiles) {
    if (tm == 64 && g_trunk_dreg && g_trunk_var == kVarNoSin)  // no sin / cos in the epilogue
        hipLaunchKernelGGL((k_trunk_bf16<64, kVarDReg | kVarNoSin>), grid, block, 0, s, ad, ntiles);
    else if (tm == 64 && g_trunk_dreg && g_trunk_var == kVarNoEpi)  // no epilogue at all
        hipLaunchKernelGGL((k_trunk_bf16<64, kVarDReg | kVarNoEpi>), grid, block, 0, s, ad, ntiles);
    else if (tm == 64 && !g_trunk_dreg) hipLaunchKernelGGL(k_trunk_bf16<64>, grid, block, 0, s, ad, ntiles);
    else if (tm == 128 && g_trunk_var == kVarNoMfma) hipLaunchKernelGGL((k_trunk_bf16<128, kVarNoMfma>), grid, block, 0, s, ad, ntiles);
    else if (tm == 128 && g_trunk_var == kVarNoSin) hipLaunchKernelGGL((k_trunk_bf16<128, kVarNoSin>), grid, block, 0, s, ad, ntiles);
    else if (tm == 128 && g_trunk_var == kVarNoW) hipLaunchKernelGGL((k_trunk_bf16<128, kVarNoW>), grid, block, 0, s, ad, ntiles);
    else if (tm == 128 && g_trunk_var == kVarNoB) hipLaunchKernelGGL((k_trunk_bf16<128, kVarNoB>), grid, block, 0, s, ad, ntiles);
    else if (tm == 128 && g_trunk_var == kVarNoEpi) hipLaunchKernelGGL((k_trunk_bf16<128, kVarNoEpi>), grid, block, 0, s, ad, ntiles);
    else if (tm == 128 && g_trunk_var == (kVarNoMfma | kVarNoW | kVarNoB | kVarNoEpi))  // trunk_var 464
        hipLaunchKernelGGL((k_trunk_bf16<128, kVarNoMfma | kVarNoW | kVarNoB | kVarNoEpi>), grid, block, 0, s, ad, ntiles);
    else if (tm == 128 && save && g_trunk_var == kVarNoPe)
        hipLaunchKernelGGL((k_trunk_bf16<128, kVarSaving | kVarNoPe>), grid, block, 0, s, ad, ntiles);
    else return false;
    return true;
}
