"""Every function include/sr_hip.h declares is either PINNED (mapped to the test that compares it with a reference of the
same operation) or EXEMPT (a non-compute entry point, with the reason).  A new entry point fails this test until it is
placed in one of the two tables; a removed one fails it until its row goes.  Runs without a GPU.

The same holds for include/sr_hip_edvr.h and include/sr_hip_dcn.h (MORE_HEADERS): their comments name entry points of other headers, so
their declarations are parsed as declarations (a return type at the start of a line), not as any ``sr_name(``."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip.h')

_LAYOUT = 'tests/test_layout_ops_gpu.py::'
_TRAIN = 'tests/test_train_ops_gpu.py::'
_CONV = 'tests/test_conv_ops_gpu.py::'

PINNED = {
    # layout.hip / layout_bf16.hip
    'sr_nchw_to_cb8_f32': _LAYOUT + 'test_nchw_to_cb',
    'sr_nchw_to_cb16_bf16': _LAYOUT + 'test_nchw_to_cb',
    'sr_cb8_to_nchw_f32': _LAYOUT + 'test_cb_to_nchw_is_the_adjoint_and_the_inverse',
    'sr_cb16_to_nchw_f32': _LAYOUT + 'test_cb_to_nchw_is_the_adjoint_and_the_inverse',
    'sr_upsample2x_bwd_f32': _LAYOUT + 'test_upsample2x_bwd',
    'sr_upsample2x_bwd_bf16': _LAYOUT + 'test_upsample2x_bwd',
    'sr_cb8_axpby_f32': _LAYOUT + 'test_cb_axpby_window',
    'sr_cb16_axpby_bf16': _LAYOUT + 'test_cb_axpby_window',
    # disc_bf16.hip
    'sr_cb16_unshuffle2_bf16': _LAYOUT + 'test_cb16_unshuffle2_both_ways',
    'sr_cb16_add_bf16': _LAYOUT + 'test_cb16_add_bf16',
    'sr_cb16_add_u2_bf16': _LAYOUT + 'test_cb16_add_u2_bf16',
    'sr_lrelu_fwd_bf16': _LAYOUT + 'test_lrelu_fwd_bwd_bf16',
    'sr_lrelu_bwd_bf16': _LAYOUT + 'test_lrelu_fwd_bwd_bf16',
    'sr_lrelu_bwd_diff_u2_bf16': _LAYOUT + 'test_lrelu_bwd_diff_u2_bf16',
    'sr_maxpool2x2_fwd_bf16': _LAYOUT + 'test_maxpool2x2_bf16',
    'sr_maxpool2x2_bwd_bf16': _LAYOUT + 'test_maxpool2x2_bf16',
    'sr_cb16_fork_bwd_bf16': _LAYOUT + 'test_cb16_fork_bwd',
    'sr_cb16_fork_bwd_u2_bf16': _LAYOUT + 'test_cb16_fork_bwd',
    'sr_bilinear2x_fwd_bf16': _LAYOUT + 'test_bilinear2x_fwd_bf16',
    'sr_bilinear2x_fwd_u2_bf16': _LAYOUT + 'test_bilinear2x_fwd_bf16',
    'sr_bilinear2x_bwd_bf16': _LAYOUT + 'test_bilinear2x_bwd_bf16',
    'sr_bilinear2x_bwd_lrelu_bf16': _LAYOUT + 'test_bilinear2x_bwd_bf16',
    # one target per symbol: the eval mode; the train mode of these four (both kernels, the edge shapes) is pinned next to it in
    # test_bn_lrelu_train_mode, and on the networks' own tensors in tests/test_f32_nets_opwise_gpu.py
    'sr_bn_lrelu_fwd_f32': _LAYOUT + 'test_bn_lrelu_eval_mode',
    'sr_bn_lrelu_bwd_f32': _LAYOUT + 'test_bn_lrelu_eval_mode',
    'sr_bn_lrelu_fwd_bf16': _LAYOUT + 'test_bn_lrelu_eval_mode',
    'sr_bn_lrelu_bwd_bf16': _LAYOUT + 'test_bn_lrelu_eval_mode',
    'sr_conv4x4s2_weight_as_3x3_f32': _CONV + 'test_conv4x4s2_weight_as_3x3',
    # train_ops.hip
    'sr_adam_step_f32': _TRAIN + 'test_adam_five_steps',
    'sr_add_f32': _TRAIN + 'test_add_bit_exact_and_rejects_ragged_length',
    'sr_axpby_f32': _TRAIN + 'test_ema_axpby',
    'sr_fill_scaled_f32': _TRAIN + 'test_fill_scaled',
    'sr_mean_f32': _TRAIN + 'test_flat_reduction_forward',
    'sr_l1_loss_fwd_f32': _TRAIN + 'test_flat_reduction_forward',
    'sr_pixel_loss_fwd_f32': _TRAIN + 'test_flat_reduction_forward',
    'sr_gan_point_loss_fwd_f32': _TRAIN + 'test_flat_reduction_forward',
    'sr_bce_logits_fwd_f32': _TRAIN + 'test_flat_reduction_forward',
    'sr_l1_loss_bwd_f32': _TRAIN + 'test_elementwise_backward',
    'sr_pixel_loss_bwd_f32': _TRAIN + 'test_elementwise_backward',
    'sr_gan_point_loss_bwd_f32': _TRAIN + 'test_elementwise_backward',
    'sr_bce_logits_bwd_f32': _TRAIN + 'test_elementwise_backward',
    'sr_bilinear2x_fwd_f32': _TRAIN + 'test_bilinear2x',
    'sr_bilinear2x_bwd_f32': _TRAIN + 'test_bilinear2x',
    'sr_channel_affine_f32': _TRAIN + 'test_channel_affine_bit_exact',
    'sr_linear_fwd_f32': _TRAIN + 'test_linear',
    'sr_linear_bwd_f32': _TRAIN + 'test_linear',
    'sr_lrelu_fwd_f32': _TRAIN + 'test_lrelu_bit_exact',
    'sr_lrelu_bwd_f32': _TRAIN + 'test_lrelu_bit_exact',
    'sr_maxpool2x2_fwd_f32': _TRAIN + 'test_maxpool2x2_bit_exact',
    'sr_maxpool2x2_bwd_f32': _TRAIN + 'test_maxpool2x2_bit_exact',
    'sr_spectral_norm_fwd_f32': _TRAIN + 'test_spectral_norm_forward',
    'sr_spectral_norm_bwd_f32': _TRAIN + 'test_spectral_norm_backward',
    'sr_spectral_norm_fwd_batch_f32': _TRAIN + 'test_spectral_norm_batch_equals_single_layer_calls',
    'sr_psnr_sse_f32': _TRAIN + 'test_psnr_ssim_device',
    'sr_ssim_sum_f32': _TRAIN + 'test_psnr_ssim_device',
    # convolutions
    'sr_conv3x3_f32': _CONV + 'test_conv3x3_f32',
    'sr_conv3x3_pack_f32': _CONV + 'test_conv3x3_f32',
    'sr_conv3x3_bf16': _CONV + 'test_conv3x3_bf16',
    'sr_conv3x3_pack_bf16': _CONV + 'test_conv3x3_bf16',
    'sr_conv4x4s2_f32': _CONV + 'test_conv4x4s2_f32_forward',
    'sr_conv4x4s2_pack_f32': _CONV + 'test_conv4x4s2_f32_forward',
    'sr_conv4x4s2_dgrad_f32': _CONV + 'test_conv4x4s2_f32_dgrad',
    'sr_conv3x3_wgrad_f32': _CONV + 'test_conv3x3_wgrad_f32',
    'sr_conv4x4s2_wgrad_f32': _CONV + 'test_conv4x4s2_wgrad_f32',
    'sr_conv3x3_wgrad_bf16': _CONV + 'test_conv3x3_wgrad_bf16',
    'sr_rdb_wgrad_bf16': _CONV + 'test_rdb_wgrad_bf16',
    'sr_conv3x3_chain_f32': 'tests/test_chain_f32_gpu.py::test_chain_equals_conv_by_conv_bit_for_bit',
    'sr_conv3x3_chain_bf16': 'tests/test_chain_bf16_gpu.py::test_chain_equals_conv_by_conv_bit_for_bit',
    # generators, their layout helpers and channel attention
    'sr_cb8_pixel_shuffle_f32': 'tests/test_msrresnet_gpu.py::test_pixel_shuffle_and_unshuffle_are_bit_exact_permutations',
    'sr_cb8_pixel_unshuffle_f32': 'tests/test_msrresnet_gpu.py::test_pixel_shuffle_and_unshuffle_are_bit_exact_permutations',
    'sr_bilinear_up_f32': 'tests/test_msrresnet_gpu.py::test_bilinear_up_matches_float64_interpolate',
    'sr_bilinear_up_bwd_f32': 'tests/test_msrresnet_gpu.py::test_bilinear_adjoint_matches_autograd_and_is_reproducible',
    'sr_ca_squeeze_f32': 'tests/test_rcan_gpu.py::test_channel_attention_kernels_match_float64',
    'sr_ca_excite_f32': 'tests/test_rcan_gpu.py::test_channel_attention_kernels_match_float64',
    'sr_ca_bwd_f32': 'tests/test_rcan_gpu.py::test_channel_attention_kernels_match_float64',
    'sr_ca_bwd_apply_f32': 'tests/test_rcan_gpu.py::test_channel_attention_kernels_match_float64',
    'sr_rrdbnet_pack_f32': 'tests/test_rrdbnet_gpu.py::test_network_vs_reference_goldens',
    'sr_rrdbnet_forward_f32': 'tests/test_rrdbnet_gpu.py::test_network_vs_reference_goldens',
    'sr_rrdbnet_forward_train_f32': 'tests/test_backward_gpu.py::test_small_nets_all_gradients_vs_oracle_autograd',
    'sr_rrdbnet_backward_f32': 'tests/test_backward_gpu.py::test_small_nets_all_gradients_vs_oracle_autograd',
    'sr_rrdbnet_pack_dgrad_f32': 'tests/test_backward_gpu.py::test_small_nets_all_gradients_vs_oracle_autograd',
    'sr_rrdbnet_pack_bf16': 'tests/test_bf16_gpu.py::test_rrdbnet_bf16_vs_reference_golden',
    'sr_rrdbnet_forward_bf16': 'tests/test_bf16_gpu.py::test_rrdbnet_bf16_vs_reference_golden',
    'sr_rrdbnet_forward_train_bf16': 'tests/test_bf16_gpu.py::test_bf16_gradients_equal_a_float64_model_of_bf16_storage',
    'sr_rrdbnet_backward_bf16': 'tests/test_bf16_gpu.py::test_bf16_gradients_equal_a_float64_model_of_bf16_storage',
    'sr_rrdbnet_pack_dgrad_bf16': 'tests/test_bf16_gpu.py::test_bf16_gradients_equal_a_float64_model_of_bf16_storage',
    # discriminators, perceptual loss, metrics, data
    'sr_vgg_pack_f32': 'tests/test_training_gpu.py::test_vgg_gradient_quality_vs_float64',
    'sr_vgg_forward_f32': 'tests/test_training_gpu.py::test_vgg_gradient_quality_vs_float64',
    'sr_vgg_backward_f32': 'tests/test_training_gpu.py::test_vgg_gradient_quality_vs_float64',
    'sr_vgg_apply_stats_f32': 'tests/test_vgg_driver_gpu.py::test_driver_is_bit_identical_to_the_per_layer_route',
    # the bf16 whole-network drivers: bit identity to the per-layer route is what these rows pin; the per-layer route's ops are pinned
    # one by one against float64 in tests/test_vgg_bf16_opwise_gpu.py
    'sr_vgg_pack_bf16': 'tests/test_vgg_driver_gpu.py::test_driver_is_bit_identical_to_the_per_layer_route',
    'sr_vgg_forward_bf16': 'tests/test_vgg_driver_gpu.py::test_driver_is_bit_identical_to_the_per_layer_route',
    'sr_vgg_backward_bf16': 'tests/test_vgg_driver_gpu.py::test_driver_is_bit_identical_to_the_per_layer_route',
    'sr_vgg_apply_stats_bf16': 'tests/test_vgg_driver_gpu.py::test_driver_is_bit_identical_to_the_per_layer_route',
    'sr_unet_pack_bf16': 'tests/test_unet_disc_bf16_gpu.py::test_unet_bf16_equals_a_float64_model_of_bf16_storage',
    'sr_unet_forward_bf16': 'tests/test_unet_disc_bf16_gpu.py::test_unet_bf16_equals_a_float64_model_of_bf16_storage',
    'sr_unet_backward_bf16': 'tests/test_unet_disc_bf16_gpu.py::test_unet_bf16_equals_a_float64_model_of_bf16_storage',
    'sr_gram_fwd_f32': 'tests/test_perceptual_gpu.py::test_gram_matrix_kernels_against_float64',
    'sr_gram_bwd_f32': 'tests/test_perceptual_gpu.py::test_gram_matrix_kernels_against_float64',
    'sr_niqe_luma_f32': 'tests/test_niqe_gpu.py::test_device_luma_and_mscn_are_bit_exact',
    'sr_niqe_moments_f32': 'tests/test_niqe_gpu.py::test_device_features_and_score_match_reference',
    'sr_patch_augment_u8_f32': 'tests/test_data_gpu.py::test_device_pipeline_is_bit_identical_to_the_host_pipeline',
}

_SIZE = 'size / workspace / parameter-count query: host arithmetic, no kernel'
EXEMPT = {
    'sr_version': 'ABI version',
    'sr_last_error': 'last error message',
    'sr_kernel_name': 'profiler: name of a kernel id',
    'sr_profile_start': 'profiler',
    'sr_profile_stop': 'profiler',
    'sr_abort_latch': 'abort latch',
    'sr_abort_latch_clear': 'abort latch',
    'sr_chain_watchdog': 'watchdog of the chained launches',
    'sr_backward_lane_join': 'lane join: stream ordering only',
    'sr_conv3x3_chain_sync_ints': 'chain sync: size of the hand-off counters',
    'sr_set_conv_chain': 'switch',
    'sr_set_conv_chain_f32': 'switch',
    'sr_set_forward_groups': 'switch',
    'sr_set_backward_wgrad_deferred': 'switch',
    'sr_conv3x3_cin_pad': _SIZE,
    'sr_conv3x3_cin_pad16': _SIZE,
    'sr_conv3x3_packed_weight_floats': _SIZE,
    'sr_conv3x3_packed_bias_floats': _SIZE,
    'sr_conv3x3_packed_weight_elems_bf16': _SIZE,
    'sr_conv4x4s2_packed_weight_floats': _SIZE,
    'sr_conv3x3_wgrad_slab_bytes': _SIZE,
    'sr_conv3x3_wgrad_slab_bytes_bf16': _SIZE,
    'sr_rdb_wgrad_slab_bytes_bf16': _SIZE,
    'sr_reduce_workspace_bytes': _SIZE,
    'sr_ca_workspace_bytes': _SIZE,
    'sr_niqe_workspace_bytes': _SIZE,
    'sr_rrdbnet_num_params': _SIZE,
    'sr_rrdbnet_packed_bytes': _SIZE,
    'sr_rrdbnet_packed_bytes_bf16': _SIZE,
    'sr_rrdbnet_packed_dgrad_bytes': _SIZE,
    'sr_rrdbnet_packed_dgrad_bytes_bf16': _SIZE,
    'sr_rrdbnet_workspace_bytes': _SIZE,
    'sr_rrdbnet_workspace_bytes_bf16': _SIZE,
    'sr_rrdbnet_saved_bytes': _SIZE,
    'sr_rrdbnet_saved_bytes_bf16': _SIZE,
    'sr_rrdbnet_backward_workspace_bytes': _SIZE,
    'sr_rrdbnet_backward_workspace_bytes_bf16': _SIZE,
    'sr_vgg_num_params': _SIZE,
    'sr_vgg_num_batchnorm': _SIZE,
    'sr_vgg_packed_bytes': _SIZE,
    'sr_vgg_packed_bytes_bf16': _SIZE,
    'sr_vgg_saved_bytes': _SIZE,
    'sr_vgg_saved_bytes_bf16': _SIZE,
    'sr_vgg_workspace_bytes': _SIZE,
    'sr_vgg_workspace_bytes_bf16': _SIZE,
    'sr_unet_num_params': _SIZE,
    'sr_unet_packed_bytes_bf16': _SIZE,
    'sr_unet_saved_bytes_bf16': _SIZE,
    'sr_unet_workspace_bytes_bf16': _SIZE,
}


_EDVR = 'tests/test_edvr_ops_gpu.py::'
_DCN = 'tests/test_dcn_ops_gpu.py::'
MORE_HEADERS = {
    'include/sr_hip_edvr.h': ({
        'sr_conv3x3s2_f32': _EDVR + 'test_conv3x3s2_forward',
        'sr_cb8_zero_insert2_f32': _EDVR + 'test_zero_insert_is_bit_exact',
        'sr_pool3x3s2_fwd_f32': _EDVR + 'test_pool_forward',
        'sr_pool3x3s2_bwd_f32': _EDVR + 'test_pool_backward',
        'sr_tsa_corr_fwd_f32': _EDVR + 'test_tsa_corr',
        'sr_tsa_corr_bwd_f32': _EDVR + 'test_tsa_corr',
        'sr_tsa_gate_fwd_f32': _EDVR + 'test_tsa_gate',
        'sr_tsa_gate_bwd_f32': _EDVR + 'test_tsa_gate',
    }, {
        'sr_conv3x3s2_lds_bytes': _SIZE,
    }),
    'include/sr_hip_dcn.h': ({
        'sr_dcn_fwd_f32': _DCN + 'test_forward',
        'sr_dcn_cols_f32': _DCN + 'test_backward',
        'sr_dcn_bwd_data_f32': _DCN + 'test_backward',
        # no test calls these two by name: they run inside DCNFn's backward (hip_ops.PackedDcnT packs Wt for dcol = Wt dz, from which
        # dx, doffset and dmask come; hip_ops.dcn_wgrad unpacks dweight), which this test holds against float64 on every DCN of EDVR
        'sr_dcn_pack_t_f32': 'tests/test_edvr_opwise_gpu.py::test_deformable_convolutions',
        'sr_dcn_weight_unpack_f32': 'tests/test_edvr_opwise_gpu.py::test_deformable_convolutions',
    }, {
        'sr_dcn_cols_bytes': _SIZE,
        'sr_dcn_packed_t_weight_floats': _SIZE,
    }),
}


def declared_functions(header_text):
    """Function names a header DECLARES: a return type at the start of a line, then the name."""
    return set(re.findall(r'^(?:int|size_t|const char\s*\*)\s+(sr_[a-z0-9_]+)\s*\(', header_text, re.M))


def declared_symbols(header_text):
    """Function names declared in the header (the parse of test_boundary.py::test_library_exports_every_declared_symbol)."""
    return set(re.findall(r'\b(sr_[a-z0-9_]+)\s*\(', header_text))


def ledger_problems(declared, pinned, exempt, root=ROOT):
    problems = []
    for s in sorted(declared):
        if (s in pinned) == (s in exempt):
            problems.append(f'{s}: in {"both tables" if s in pinned else "neither table"}')
    for s in sorted((set(pinned) | set(exempt)) - declared):
        problems.append(f'{s}: not declared in include/sr_hip.h any more')
    tests = {}
    for s, target in sorted(pinned.items()):
        path, _, func = target.partition('::')
        if not (path.startswith('tests/') and path.endswith('.py') and func):
            problems.append(f'{s}: malformed target {target!r}')
            continue
        if path not in tests:
            full = os.path.join(root, path)
            tests[path] = None
            if os.path.exists(full):
                tree = ast.parse(open(full).read())
                tests[path] = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        if tests[path] is None:
            problems.append(f'{s}: {path} does not exist')
        elif func not in tests[path]:
            problems.append(f'{s}: {path} has no test function {func}')
    return problems


def test_every_declared_entry_point_is_pinned_or_exempt():
    declared = declared_symbols(open(HEADER).read())
    assert len(declared) > 100, 'the header parse found too few declarations'
    assert not ledger_problems(declared, PINNED, EXEMPT), ledger_problems(declared, PINNED, EXEMPT)


def test_exemptions_are_not_compute_entry_points():
    """Nothing that launches a kernel on data hides in EXEMPT: only the kinds of entry point the ledger allows."""
    allowed = re.compile(r'(_bytes(_bf16)?|_num_params|_num_batchnorm|_cin_pad(16)?|_floats|_elems_bf16|^sr_set_|^sr_dev_|'
                         r'^sr_profile_|^sr_kernel_name|^sr_version|^sr_last_error|^sr_abort_latch|_watchdog|_lane_join|'
                         r'_chain_sync_ints)')
    for s in EXEMPT:
        assert allowed.search(s), s


def test_the_ledger_notices_a_new_declaration_and_a_dropped_row(tmp_path):
    text = open(HEADER).read()
    declared = declared_symbols(text + '\nint sr_new_kernel_f32(const float* x, float* y, void* stream);\n')
    assert any(p.startswith('sr_new_kernel_f32:') for p in ledger_problems(declared, PINNED, EXEMPT))
    declared = declared_symbols(text)
    fewer = dict(PINNED)
    del fewer['sr_upsample2x_bwd_bf16']
    assert ledger_problems(declared, fewer, EXEMPT) == ['sr_upsample2x_bwd_bf16: in neither table']
    both = dict(EXEMPT, sr_cb8_axpby_f32='x')
    assert ledger_problems(declared, PINNED, both) == ['sr_cb8_axpby_f32: in both tables']
    stale = dict(PINNED, sr_retired_f32=_LAYOUT + 'test_nchw_to_cb')
    assert ledger_problems(declared, stale, EXEMPT) == ['sr_retired_f32: not declared in include/sr_hip.h any more']
    wrong = dict(PINNED, sr_cb8_axpby_f32=_LAYOUT + 'test_no_such_test')
    assert ledger_problems(declared, wrong, EXEMPT) == [
        'sr_cb8_axpby_f32: tests/test_layout_ops_gpu.py has no test function test_no_such_test']


def test_every_entry_point_of_the_edvr_and_dcn_headers_is_pinned_or_exempt():
    allowed = re.compile(r'(_bytes|_floats)$')
    for header, (pinned, exempt) in MORE_HEADERS.items():
        declared = declared_functions(open(os.path.join(ROOT, header)).read())
        assert len(declared) >= 7, f'{header}: the parse found too few declarations'
        problems = [p.replace('include/sr_hip.h', header) for p in ledger_problems(declared, pinned, exempt)]
        assert not problems, problems
        for s in exempt:
            assert allowed.search(s), s
    dcn = declared_functions(open(os.path.join(ROOT, 'include', 'sr_hip_dcn.h')).read())
    assert {'sr_dcn_pack_t_f32', 'sr_dcn_weight_unpack_f32'} <= dcn
    fewer = dict(MORE_HEADERS['include/sr_hip_dcn.h'][0])
    del fewer['sr_dcn_pack_t_f32']
    assert ledger_problems(dcn, fewer, MORE_HEADERS['include/sr_hip_dcn.h'][1]) == ['sr_dcn_pack_t_f32: in neither table']
    # the two are reached from the Function the pinned test replays, and from nowhere else in the fp32 route
    ops = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    auto = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_autograd.py')).read()
    assert "launch('sr_dcn_pack_t_f32'" in ops and "launch('sr_dcn_weight_unpack_f32'" in ops
    assert 'H.PackedDcnT(weight)' in auto and 'H.dcn_wgrad(cols, dzc, cout, cin' in auto
