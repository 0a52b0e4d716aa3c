"""The ledger of the stream tests (tests/test_gpu_streams.py, harness in tests/stream_gate.py).

STREAM_TESTS names, for every function of include/hint_amd.h that takes `void* stream`, the test that runs it S-gated and
null-gated with still_closed() asserted; no C entry point is exempt.  ROUTES lists the Python routes the same file runs, each
with the test that runs it and, where the route synchronises the host by contract, the line that does (`host_sync`): such a
route keeps every bit comparison and skips only the still_closed() assertion.  tests/test_stream_table_cpu.py parses the
header and fails, naming the function, when one is missing here; it also holds the exemptions to a quarter of the routes."""
T = "tests/test_gpu_streams.py::"

STREAM_TESTS = {
    "hint_block_pack": T + "test_block_families",
    "hint_block_forward": T + "test_block_families",
    "hint_block_backward": T + "test_block_families",
    "hint_block_inverse": T + "test_block_families",
    "hint_block_forward_ex": T + "test_ex_forms",
    "hint_block_backward_ex": T + "test_ex_forms",
    "hint_block_inverse_ex": T + "test_ex_forms",
    "hint_block_forward_noisy": T + "test_noisy_forwards",
    "hint_chain_forward_noisy": T + "test_noisy_forwards",
    "hint_chain_forward": T + "test_chains",
    "hint_chain_backward": T + "test_chains",
    "hint_chain_inverse": T + "test_chains",
    "hint_chain_backward_parts": T + "test_backward_parts_and_wgrad_ranges",
    "hint_chain_wgrad_range": T + "test_backward_parts_and_wgrad_ranges",
    "hint_chain_backward_adam": T + "test_fused_adam",
    "hint_chain_wgrad_adam": T + "test_fused_adam",
    "hint_block_backward_rows": T + "test_fused_adam",
    "hint_block_inverse_backward": T + "test_inverse_backward",
    "hint_block_ext_coeffs": T + "test_ext_coeffs_and_affine_chain",
    "hint_pack_group_run": T + "test_pack_group",
    "hint_pack_group_run_ex": T + "test_pack_group",
    "hint_adam_step": T + "test_adam_steps",
    "hint_adam_step_dev": T + "test_adam_steps",
    "hint_adam_multi_step": T + "test_adam_steps",
    "hint_mmd_run": T + "test_descriptors",
    "hint_abc_run": T + "test_descriptors",
    "hint_corr_run": T + "test_descriptors",
    "hint_curve_run": T + "test_descriptors",
    "hint_hausdorff_run": T + "test_descriptors",
    "hint_plus_run": T + "test_descriptors",
    "hint_lensfit_run": T + "test_descriptors",
    "hint_plusfit_run": T + "test_descriptors",
    "hint_overlap_run": T + "test_descriptors",
    "hint_lensgen_run": T + "test_descriptors",
    "hint_fcoef_run": T + "test_descriptors",
}

# route -> (test, host_sync): host_sync is None, or the source line that synchronises the host by contract
ROUTES = {
    "block_forward_wl": (T + "test_block_module", None),
    "block_forward_n3": (T + "test_block_module", None),
    "block_rev_wl": (T + "test_block_module", None),
    "block_rev_n3": (T + "test_block_module", None),
    "external_affine_coupling": (T + "test_external_coupling", None),
    "hint_flow_fused": (T + "test_hint_flow", None),
    "hint_flow_blockwise_reshuffle": (T + "test_hint_flow", None),
    "conditional_forward": (T + "test_conditional_flow", None),
    "conditional_sample_broadcast": (T + "test_conditional_flow", None),
    "conditional_sample_per_row": (T + "test_conditional_flow", None),
    "conditional_x_lane": (T + "test_conditional_flow", None),
    "clamp_adam_step": (T + "test_clamp_adam", None),
    "flow_trainer_eager": (T + "test_flow_trainer", None),
    "flow_trainer_graph": (T + "test_flow_trainer", None),
    "flow_trainer_graph_noisy": (T + "test_flow_trainer", None),
    "flow_trainer_step_many": (T + "test_flow_trainer", None),
    "conditional_trainer_eager": (T + "test_conditional_trainer", None),
    "conditional_trainer_eager_noise_switch": (
        T + "test_conditional_trainer",
        "hint_amd/conditional.py:637: `noise` switched on / off re-commits hac_x_0's gathered chain; hint_chain_commit copies its "
        "table with a synchronous hipMemcpy on the null stream, so the current stream is drained first"),
    "conditional_trainer_graph": (T + "test_conditional_trainer", None),
    "wrappers_metrics": (T + "test_wrappers", None),
    "wrappers_abc": (T + "test_wrappers", None),
    "wrappers_curves_distances": (T + "test_wrappers", None),
    "wrappers_curves_fits": (T + "test_wrappers", None),
    "wrappers_shapes": (T + "test_wrappers", None),
    "wrappers_shapes_checked_rows": (
        T + "test_wrappers",
        "hint_amd/_ops.py:132: rows taken from the caller (draws, counts) are checked, which reads the count of refused rows back"),
}
MAX_EXEMPT_SHARE = 0.25
