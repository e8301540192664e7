"""Which test reaches which kernel: one row per __global__ function of the package's csrc/*.hip, kernel name -> (entry point of include/tnqs_debug.h or public call of
include/tnqs.h that launches it, test file that calls that entry point and checks its result).  tests/test_kernel_coverage_cpu.py keeps the table complete: a kernel
added without a row, a row whose entry point is not declared, or whose test file does not mention it, fails there.  A kernel whose only honest row is an end-to-end
call carries "end to end" in place of the entry point (none at present)."""

END_TO_END = "end to end"

K, GA, SK, BP, SS = "tests/test_gpu_kernels.py", "tests/test_gpu_gate_algebra.py", "tests/test_gpu_site_kernels.py", "tests/test_gpu_bp_post.py", "tests/test_gpu_small_site.py"
MISC, AMP, BMPS, LOOPS, INNER = "tests/test_gpu_misc_kernels.py", "tests/test_gpu_amplitudes.py", "tests/test_gpu_bmps.py", "tests/test_gpu_loops.py", "tests/test_gpu_inner.py"
P32, C128 = "tests/test_gpu_plane32.py", "tests/test_gpu_fiber_c128.py"

COVERAGE = {
    # kernels.hip: the generic vector kernels and the Gram reduction
    "fiber_gemm_kernel": ("tnqs_dbg_fiber_gemm", K),
    "gram_kernel": ("tnqs_dbg_gram", K),
    "reduce_kernel": ("tnqs_dbg_gram", K),
    # kernels_amp.hip
    "amp_leg_gemm_kernel": ("tnqs_dbg_amp_leg_gemm", AMP),
    "amp_absorb_kernel": ("tnqs_dbg_amp_absorb", AMP),
    "amp_finalize_kernel": ("tnqs_dbg_amp_finalize", AMP),
    "amp_sweep_end_kernel": ("tnqs_dbg_amp_sweep_end", MISC),
    "amp_scalar_kernel": ("tnqs_dbg_amp_scalar", MISC),
    # kernels_bmps.hip
    "bmps_contract_kernel": ("tnqs_dbg_bmps_contract", BMPS),
    "bmps_reduce_kernel": ("tnqs_dbg_bmps_contract", BMPS),
    "bmps_qr_kernel": ("tnqs_dbg_bmps_qr", BMPS),
    "bmps_norm_kernel": ("tnqs_dbg_bmps_norm", MISC),
    # kernels_bp.hip
    "msg_finalize_kernel": ("tnqs_dbg_msg_finalize", SS),
    "bp_small_site_kernel": ("tnqs_dbg_small_site", SS),
    "msg_rescale_kernel": ("tnqs_dbg_msg_rescale", BP),
    "edge_scalar_kernel": ("tnqs_dbg_edge_scalar", BP),
    "symg_build_kernel": ("tnqs_dbg_symg_build", BP),
    "symg_finish_kernel": ("tnqs_dbg_symg_finish", BP),
    # kernels_chi64.hip
    "mfma_gram64_kernel": ("tnqs_dbg_gram_mfma", K),
    "tall_gram_kernel": ("tnqs_dbg_svd_tall", K),
    "tall_rt_kernel": ("tnqs_dbg_svd_tall", K),
    "tall_w_kernel": ("tnqs_dbg_svd_tall", K),
    "tall_mj_kernel": ("tnqs_dbg_svd_tall", K),
    "copy_items_kernel": ("tnqs_dbg_copy_items", MISC),
    "mfma_rowgemm_kernel": ("tnqs_dbg_rowgemm", K),
    "mfma_gram128_f64_kernel": ("tnqs_dbg_gram_mfma", K),
    # kernels_chol.hip
    "chol_kernel": ("tnqs_dbg_chol", K),
    "chol_packed_kernel": ("tnqs_dbg_chol", K),
    "env_prepare_kernel": ("tnqs_dbg_env_prepare", BP),
    "env_finish_kernel": ("tnqs_dbg_env_finish", BP),
    # kernels_f64.hip
    "mfma_fiber_gemm_f64_kernel": ("tnqs_dbg_fiber_pass_c128", C128),
    "mfma_gram_f64in_kernel": ("tnqs_dbg_gram_c128", C128),
    # kernels_gate.hip
    "mfma_gauge_gram64_kernel": ("tnqs_dbg_gauge_gram", K),
    "mfma_gauge_gram32_kernel": ("tnqs_dbg_gauge_gram", K),
    # kernels_inner.hip
    "inner_gram_kernel": ("tnqs_dbg_inner_gram", INNER),
    "inner_finalize_kernel": ("tnqs_dbg_inner_finalize", INNER),
    "inner_scalar_kernel": ("tnqs_dbg_inner_scalar", SK),
    # kernels_loop.hip
    "loop_cgemm_kernel": ("tnqs_dbg_loop_cgemm", LOOPS),
    "loop_branch_gram_kernel": ("tnqs_dbg_loop_branch_gram", "tests/test_gpu_branched_loops.py"),
    "loop_antiproject_kernel": ("tnqs_dbg_loop_antiproject", LOOPS),
    "loop_trace_kernel": ("tnqs_dbg_loop_trace", LOOPS),
    "loop_trace_tail_kernel": ("tnqs_dbg_loop_trace", LOOPS),
    "loop_dot_kernel": ("tnqs_dbg_loop_dot", MISC),
    "loop_dot_tail_kernel": ("tnqs_dbg_loop_dot", MISC),
    # kernels_mfma.hip
    "mfma_fiber_gemm_w_kernel": ("tnqs_dbg_fiber_gemm", K),
    "mfma_gram32_kernel": ("tnqs_dbg_gram", K),
    "mfma_gram32_fused_kernel": ("tnqs_dbg_gram_fused", K),
    "mfma_pair_kernel": ("tnqs_dbg_pair", K),
    "mfma_pair_gram_kernel": ("tnqs_dbg_pair_gram", K),
    "mfma_pair_gram2_kernel": ("tnqs_dbg_pair_gram2", K),
    "recover_v_mfma_kernel": ("tnqs_dbg_jacobi", K),
    "mfma_gram64_f64_kernel": ("tnqs_dbg_gram", K),
    # kernels_plane.hip
    "mfma_pair16_kernel": ("tnqs_dbg_pair16", K),
    "mfma_pair16w_kernel": ("tnqs_dbg_pair16", K),
    "mfma_pair_gram2x16_kernel": ("tnqs_dbg_pair_gram2x16", K),
    # kernels_rdm.hip
    "edge_rdm_kernel": ("tnqs_dbg_edge_rdm", "tests/test_gpu_rdm_edges.py"),
    "path_apply_kernel": ("tnqs_dbg_path_apply", "tests/test_gpu_path_rdm.py"),
    # kernels_sample.hip
    "site_prob_partial_kernel": ("tnqs_dbg_site_prob", SK),
    "site_draw_kernel": ("tnqs_dbg_site_draw", SK),
    "site_project_kernel": ("tnqs_dbg_site_project", SK),
    # kernels_spectrum.hip
    "bond_rho_kernel": ("tnqs_dbg_bond_spectrum", "tests/test_gpu_bond_spectra.py"),
    "bond_spectrum_finish_kernel": ("tnqs_dbg_bond_spectrum", "tests/test_gpu_bond_spectra.py"),
    # kernels_svd.hip
    "jacobi_kernel": ("tnqs_dbg_jacobi", K),
    "jacobi_lds_kernel": ("tnqs_dbg_jacobi", K),
    "theta_svd_pre_kernel": ("tnqs_dbg_theta_svd_pre", K),
    "recover_v_kernel": ("tnqs_dbg_jacobi", K),
    "small_svd_prepare_kernel": ("tnqs_dbg_small_svd", GA),
    "small_svd_finish_kernel": ("tnqs_dbg_small_svd", GA),
    # kernels_theta.hip: the theta chain of the gate path (csrc/gate_theta.cpp) and the per-gate small algebra
    "gate_theta_kernel": ("tnqs_dbg_gate_theta", GA),
    "gate_theta_mm_kernel": ("tnqs_dbg_gate_theta", GA),
    "lowrank_g_kernel": ("tnqs_dbg_gate_theta", GA),
    "lowrank_m_kernel": ("tnqs_dbg_gate_theta", GA),
    "theta_scale_kernel": ("tnqs_dbg_gate_theta", GA),
    "lowrank_bw_kernel": ("tnqs_dbg_gate_theta", GA),
    "lowrank_ll_kernel": ("tnqs_dbg_gate_theta", GA),
    "qr2_rinv_kernel": ("tnqs_dbg_qr2", GA),
    "qr2_compose_kernel": ("tnqs_dbg_qr2", GA),
    "gate_finish_kernel": ("tnqs_dbg_gate_finish", GA),
    # kernels_util.hip
    "diag_kernel": ("tnqs_dbg_diag", BP),
    "norm_factor_kernel": ("tnqs_dbg_norm_factor", SK),
    "scale_kernel": ("tnqs_dbg_scale", SK),
    "cscale_kernel": ("tnqs_dbg_cscale", BP),
    "record_pack_kernel": ("tnqs_dbg_record_pack", MISC),
    "header_gather_kernel": ("tnqs_dbg_record_pack", MISC),
    "permute_kernel": ("tnqs_dbg_permute", MISC),
    "identity_kernel": ("tnqs_dbg_identity", MISC),
    "random_fill_kernel": ("tnqs_dbg_random_fill", MISC),
    "site1_c64_kernel": ("tnqs_dbg_site1", SK),
    "sum_doubles_kernel": ("tnqs_dbg_sum_doubles", MISC),
    # kernels_x3.hip: the bf16 x 3 route of the chi = 32 / chi = 64 kernels
    "x3_pair_gram2_kernel": ("tnqs_dbg_pair_gram32", P32),
    "x3_pair_kernel": ("tnqs_dbg_pair32", P32),
    "x3_rowgemm64_kernel": ("tnqs_dbg_rowgemm", K),
    "x3_gram64_kernel": ("tnqs_dbg_gram_mfma", K),
}
