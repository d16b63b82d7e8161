"""ctypes binding of libsr_hip.so (C ABI declared in include/sr_hip.h, include/sr_hip_ridnet.h, include/sr_hip_gfpgan.h,
include/sr_hip_edsr.h, include/sr_hip_ca_bf16.h, include/sr_hip_dcn.h, include/sr_hip_edvr.h, include/sr_hip_edvr_bf16.h,
include/sr_hip_stylegan2.h, include/sr_hip_train_groups.h, include/sr_hip_degrade.h, include/sr_hip_flow.h and
include/sr_hip_flow_bwd.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails the
caller gets an exception.  The product path never routes through ``oracle/`` or
through PyTorch CPU/ATen convolutions.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SR_HIP_LIB_PATH') or os.path.join(_HERE, 'lib', 'libsr_hip.so')  # override: A/B builds of the kernels

SR_ABI_VERSION = 3


class SrHipError(RuntimeError):
    """Raised when a libsr_hip.so entry point returns a non-zero status."""


class ConvDesc(C.Structure):
    """struct sr_conv3x3_desc (include/sr_hip.h)."""
    _fields_ = [
        ('in_', C.c_void_p), ('in_img_stride', C.c_int64), ('cin_pad', C.c_int), ('cin_real', C.c_int), ('in_h', C.c_int), ('in_w', C.c_int),
        ('upsample', C.c_int), ('wpacked', C.c_void_p), ('bpacked', C.c_void_p), ('cout', C.c_int),
        ('out', C.c_void_p), ('out_img_stride', C.c_int64), ('out_nchw', C.c_int), ('n', C.c_int),
        ('act_slope', C.c_float), ('alpha', C.c_float),
        ('res1', C.c_void_p), ('res1_img_stride', C.c_int64), ('beta1', C.c_float),
        ('res2', C.c_void_p), ('res2_img_stride', C.c_int64), ('beta2', C.c_float), ('res_cbn', C.c_int),
        ('out_h', C.c_int), ('out_w', C.c_int), ('accumulate', C.c_int), ('mask_src', C.c_void_p), ('mask_img_stride', C.c_int64),
        ('mask_cb0', C.c_int), ('mask_cbn', C.c_int), ('mask_slope', C.c_float), ('s2_channels', C.c_int), ('s2_side', C.c_int),
        ('out_unshuffle2', C.c_int), ('res1_u2', C.c_int), ('res1_keep_sign', C.c_int),
    ]


class WgradDesc(C.Structure):
    """struct sr_conv3x3_wgrad_desc (include/sr_hip.h)."""
    _fields_ = [
        ('x', C.c_void_p), ('x_img_stride', C.c_int64), ('cin_pad', C.c_int), ('in_h', C.c_int), ('in_w', C.c_int),
        ('upsample', C.c_int), ('dy', C.c_void_p), ('dy_img_stride', C.c_int64), ('cout', C.c_int), ('cin', C.c_int),
        ('first_seg', C.c_int), ('seg', C.c_int), ('n', C.c_int), ('scale', C.c_float), ('dweight', C.c_void_p),
        ('dbias', C.c_void_p), ('accumulate', C.c_int), ('slab', C.c_void_p), ('slab_bytes', C.c_size_t),
    ]


class SnLayer(C.Structure):
    """struct sr_sn_layer (include/sr_hip.h)."""
    _fields_ = [('w_orig', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p), ('rows', C.c_int), ('cols', C.c_int),
                ('w_sn', C.c_void_p), ('sigma', C.c_void_p)]


class RRDBNetCfg(C.Structure):
    """struct sr_rrdbnet_cfg (include/sr_hip.h)."""
    _fields_ = [('num_in_ch', C.c_int), ('num_out_ch', C.c_int), ('scale', C.c_int), ('num_feat', C.c_int),
                ('num_block', C.c_int), ('num_grow_ch', C.c_int)]


class VGGCfg(C.Structure):
    """struct sr_vgg_cfg (include/sr_hip.h)."""
    _fields_ = [('num_in_ch', C.c_int), ('num_feat', C.c_int), ('input_size', C.c_int)]


class UNetCfg(C.Structure):
    """struct sr_unet_cfg (include/sr_hip.h)."""
    _fields_ = [('num_in_ch', C.c_int), ('num_feat', C.c_int), ('skip_connection', C.c_int)]


# name -> (restype, argtypes); every symbol include/sr_hip.h declares
SIGNATURES = {
    'sr_version': (C.c_int, []),
    'sr_last_error': (C.c_char_p, []),
    'sr_nchw_to_cb8_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int64, C.c_void_p]),
    'sr_cb8_to_nchw_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
    'sr_upsample2x_bwd_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_cb8_axpby_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_conv3x3_packed_weight_floats': (C.c_size_t, [C.c_int, C.c_int]),
    'sr_conv3x3_packed_bias_floats': (C.c_size_t, [C.c_int]),
    'sr_conv3x3_cin_pad': (C.c_int, [C.c_int, C.c_int, C.c_int]),
    'sr_conv3x3_pack_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    'sr_conv3x3_f32': (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    'sr_conv4x4s2_packed_weight_floats': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'sr_conv4x4s2_pack_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'sr_conv4x4s2_f32': (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    'sr_conv4x4s2_dgrad_f32': (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    'sr_conv3x3_wgrad_slab_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'sr_conv3x3_wgrad_f32': (C.c_int, [C.POINTER(WgradDesc), C.c_void_p]),
    'sr_conv4x4s2_wgrad_f32': (C.c_int, [C.POINTER(WgradDesc), C.c_void_p]),
    'sr_reduce_workspace_bytes': (C.c_size_t, [C.c_int]),
    'sr_bn_lrelu_fwd_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_bn_lrelu_bwd_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_lrelu_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_void_p]),
    'sr_linear_fwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_float, C.c_void_p]),
    'sr_linear_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'sr_bilinear2x_fwd_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p]),
    'sr_bilinear2x_bwd_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p]),
    'sr_spectral_norm_fwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_spectral_norm_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_spectral_norm_fwd_batch_f32': (C.c_int, [C.POINTER(SnLayer), C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_add_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'sr_gram_fwd_f32': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    'sr_gram_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    'sr_psnr_sse_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    'sr_niqe_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'sr_niqe_luma_f32': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'sr_niqe_moments_f32': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    'sr_maxpool2x2_fwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_maxpool2x2_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_channel_affine_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    'sr_lrelu_fwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_void_p]),
    'sr_ssim_sum_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    'sr_mean_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_l1_loss_fwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    'sr_l1_loss_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'sr_pixel_loss_fwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]),
    'sr_gan_point_loss_fwd_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p]),
    'sr_gan_point_loss_bwd_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'sr_pixel_loss_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    'sr_bce_logits_fwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_bce_logits_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    'sr_fill_scaled_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]),
    'sr_adam_step_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float,
                                   C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'sr_axpby_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int64, C.c_void_p, C.c_void_p]),
    'sr_abort_latch': (C.c_void_p, []),
    'sr_set_backward_wgrad_deferred': (C.c_int, [C.c_int]),
    'sr_backward_lane_join': (C.c_int, [C.c_void_p]),
    'sr_abort_latch_clear': (C.c_int, [C.c_void_p]),
    'sr_rrdbnet_num_params': (C.c_int, [C.POINTER(RRDBNetCfg)]),
    'sr_rrdbnet_packed_bytes': (C.c_size_t, [C.POINTER(RRDBNetCfg)]),
    'sr_rrdbnet_workspace_bytes': (C.c_size_t, [C.POINTER(RRDBNetCfg), C.c_int, C.c_int, C.c_int]),
    'sr_rrdbnet_pack_f32': (C.c_int, [C.POINTER(RRDBNetCfg), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    'sr_rrdbnet_forward_f32': (C.c_int, [C.POINTER(RRDBNetCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_nchw_to_cb16_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                       C.c_void_p]),
    'sr_cb16_to_nchw_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    'sr_conv3x3_cin_pad16': (C.c_int, [C.c_int, C.c_int, C.c_int]),
    'sr_conv3x3_packed_weight_elems_bf16': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'sr_conv3x3_pack_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    'sr_conv3x3_bf16': (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    'sr_conv3x3_wgrad_slab_bytes_bf16': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'sr_conv3x3_wgrad_bf16': (C.c_int, [C.POINTER(WgradDesc), C.c_void_p]),
    'sr_rdb_wgrad_slab_bytes_bf16': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'sr_rdb_wgrad_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_void_p), C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_upsample2x_bwd_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_cb16_axpby_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    'sr_cb16_unshuffle2_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]),
    'sr_conv4x4s2_weight_as_3x3_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_lrelu_bwd_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_void_p]),
    'sr_bilinear2x_fwd_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p]),
    'sr_cb16_add_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'sr_lrelu_fwd_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_void_p]),
    'sr_maxpool2x2_fwd_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_maxpool2x2_bwd_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_cb16_fork_bwd_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p]),
    'sr_bilinear2x_bwd_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p]),
    'sr_bilinear2x_bwd_lrelu_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p,
                                               C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_cb16_add_u2_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_bilinear2x_fwd_u2_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p]),
    'sr_cb16_fork_bwd_u2_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p]),
    'sr_lrelu_bwd_diff_u2_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_void_p]),
    'sr_bn_lrelu_fwd_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_bn_lrelu_bwd_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_rrdbnet_packed_bytes_bf16': (C.c_size_t, [C.POINTER(RRDBNetCfg)]),
    'sr_rrdbnet_workspace_bytes_bf16': (C.c_size_t, [C.POINTER(RRDBNetCfg), C.c_int, C.c_int, C.c_int]),
    'sr_rrdbnet_pack_bf16': (C.c_int, [C.POINTER(RRDBNetCfg), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    'sr_rrdbnet_forward_bf16': (C.c_int, [C.POINTER(RRDBNetCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_rrdbnet_saved_bytes_bf16': (C.c_size_t, [C.POINTER(RRDBNetCfg), C.c_int, C.c_int, C.c_int]),
    'sr_rrdbnet_backward_workspace_bytes_bf16': (C.c_size_t, [C.POINTER(RRDBNetCfg), C.c_int, C.c_int, C.c_int]),
    'sr_rrdbnet_packed_dgrad_bytes_bf16': (C.c_size_t, [C.POINTER(RRDBNetCfg)]),
    'sr_rrdbnet_pack_dgrad_bf16': (C.c_int, [C.POINTER(RRDBNetCfg), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    'sr_rrdbnet_forward_train_bf16': (C.c_int, [C.POINTER(RRDBNetCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_rrdbnet_backward_bf16': (C.c_int, [C.POINTER(RRDBNetCfg), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_int, C.c_void_p]),
    'sr_set_forward_groups': (C.c_int, [C.c_int]),
    'sr_rrdbnet_saved_bytes': (C.c_size_t, [C.POINTER(RRDBNetCfg), C.c_int, C.c_int, C.c_int]),
    'sr_rrdbnet_backward_workspace_bytes': (C.c_size_t, [C.POINTER(RRDBNetCfg), C.c_int, C.c_int, C.c_int]),
    'sr_rrdbnet_packed_dgrad_bytes': (C.c_size_t, [C.POINTER(RRDBNetCfg)]),
    'sr_rrdbnet_pack_dgrad_f32': (C.c_int, [C.POINTER(RRDBNetCfg), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    'sr_rrdbnet_forward_train_f32': (C.c_int, [C.POINTER(RRDBNetCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_rrdbnet_backward_f32': (C.c_int, [C.POINTER(RRDBNetCfg), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_int, C.c_void_p]),
}



class LaunchRecord(C.Structure):
    """struct sr_launch_record (include/sr_hip.h)."""
    _fields_ = [('kernel_id', C.c_int32), ('cin', C.c_int32), ('cout', C.c_int32), ('n', C.c_int32), ('h', C.c_int32),
                ('w', C.c_int32), ('flops', C.c_double), ('bytes', C.c_double), ('ms', C.c_float)]


SIGNATURES.update({
    'sr_conv3x3_chain_sync_ints': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'sr_conv3x3_chain_bf16': (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'sr_set_conv_chain': (C.c_int, [C.c_int]),
    'sr_chain_watchdog': (C.c_int, []),
    'sr_conv3x3_chain_f32': (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'sr_set_conv_chain_f32': (C.c_int, [C.c_int]),
    'sr_patch_augment_u8_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                          C.POINTER(C.c_float), C.c_void_p]),
    'sr_cb8_pixel_shuffle_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p]),
    'sr_cb8_pixel_unshuffle_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p]),
    'sr_bilinear_up_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_bilinear_up_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_ca_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'sr_ca_squeeze_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_ca_excite_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_float, C.c_void_p]),
    'sr_ca_bwd_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_ca_bwd_apply_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_float, C.c_void_p]),
    'sr_profile_start': (C.c_int, [C.c_int]),
    'sr_profile_stop': (C.c_int, [C.POINTER(LaunchRecord), C.c_int, C.POINTER(C.c_int)]),
    'sr_kernel_name': (C.c_char_p, [C.c_int]),
})

for _suf, _plain in (('_f32', ''), ('_bf16', '_bf16')):
    SIGNATURES.update({
        'sr_vgg_packed_bytes' + _plain: (C.c_size_t, [C.POINTER(VGGCfg)]),
        'sr_vgg_saved_bytes' + _plain: (C.c_size_t, [C.POINTER(VGGCfg), C.c_int]),
        'sr_vgg_workspace_bytes' + _plain: (C.c_size_t, [C.POINTER(VGGCfg), C.c_int]),
        'sr_vgg_pack' + _suf: (C.c_int, [C.POINTER(VGGCfg), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
        'sr_vgg_forward' + _suf: (C.c_int, [C.POINTER(VGGCfg), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
        'sr_vgg_apply_stats' + _suf: (C.c_int, [C.POINTER(VGGCfg), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.c_int,
                                                C.c_void_p]),
        'sr_vgg_backward' + _suf: (C.c_int, [C.POINTER(VGGCfg), C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p]),
    })
SIGNATURES.update({
    'sr_unet_num_params': (C.c_int, [C.POINTER(UNetCfg)]),
    'sr_unet_packed_bytes_bf16': (C.c_size_t, [C.POINTER(UNetCfg)]),
    'sr_unet_saved_bytes_bf16': (C.c_size_t, [C.POINTER(UNetCfg), C.c_int, C.c_int, C.c_int]),
    'sr_unet_workspace_bytes_bf16': (C.c_size_t, [C.POINTER(UNetCfg), C.c_int, C.c_int, C.c_int]),
    'sr_unet_pack_bf16': (C.c_int, [C.POINTER(UNetCfg), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    'sr_unet_forward_bf16': (C.c_int, [C.POINTER(UNetCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    'sr_unet_backward_bf16': (C.c_int, [C.POINTER(UNetCfg), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
})
SIGNATURES.update({'sr_vgg_num_params': (C.c_int, [C.POINTER(VGGCfg)]), 'sr_vgg_num_batchnorm': (C.c_int, [C.POINTER(VGGCfg)])})


class ConvdDesc(C.Structure):
    """struct sr_convd_desc (include/sr_hip_ridnet.h)."""
    _fields_ = [('base', ConvDesc), ('ksize', C.c_int), ('dilation', C.c_int), ('post_act', C.c_int), ('out_pre', C.c_void_p),
                ('out_pre_img_stride', C.c_int64)]


class ConvdWgradDesc(C.Structure):
    """struct sr_convd_wgrad_desc (include/sr_hip_ridnet.h)."""
    _fields_ = [('base', WgradDesc), ('ksize', C.c_int), ('dilation', C.c_int)]


# name -> (restype, argtypes); every symbol include/sr_hip_ridnet.h declares (kept apart from SIGNATURES, which mirrors sr_hip.h)
RIDNET_SIGNATURES = {
    'sr_convk_packed_weight_floats': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'sr_convk_pack_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'sr_convd_f32': (C.c_int, [C.POINTER(ConvdDesc), C.c_void_p]),
    'sr_convd_wgrad_slab_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'sr_convd_wgrad_f32': (C.c_int, [C.POINTER(ConvdWgradDesc), C.c_void_p]),
    'sr_ridnet_mean_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'sr_ridnet_sub_mean_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p]),
    'sr_ridnet_add_mean_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p]),
    'sr_ridnet_sub_mean_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_ridnet_add_mean_bwd_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_ca_scale_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p]),
    'sr_cb8_relu_mask_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_int64, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_void_p]),
}

class GfpganStyleLayer(C.Structure):
    """struct sr_gfpgan_style_layer (include/sr_hip_gfpgan.h)."""
    _fields_ = [('mod_w', C.c_void_p), ('mod_b', C.c_void_p), ('q', C.c_void_p), ('cin', C.c_int), ('cout', C.c_int),
                ('latent_index', C.c_int), ('wscale', C.c_float), ('s', C.c_void_p), ('d', C.c_void_p)]


class GfpganTail(C.Structure):
    """struct sr_gfpgan_tail (include/sr_hip_gfpgan.h)."""
    _fields_ = [('demod', C.c_void_p), ('noise', C.c_void_p), ('noise_img_stride', C.c_int64), ('noise_strength', C.c_float),
                ('sft_scale', C.c_void_p), ('sft_scale_img_stride', C.c_int64), ('sft_shift', C.c_void_p),
                ('sft_shift_img_stride', C.c_int64), ('sft_c0', C.c_int), ('s_next', C.c_void_p)]


class GfpganModconvDesc(C.Structure):
    """struct sr_gfpgan_modconv_desc (include/sr_hip_gfpgan.h)."""
    _fields_ = [('base', ConvDesc), ('tail', GfpganTail)]


# name -> (restype, argtypes); every symbol include/sr_hip_gfpgan.h declares
GFPGAN_SIGNATURES = {
    'sr_gfpgan_style_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.POINTER(GfpganStyleLayer), C.c_int, C.c_int,
                                      C.c_void_p]),
    'sr_gfpgan_norm_style_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'sr_gfpgan_modconv_f32': (C.c_int, [C.POINTER(GfpganModconvDesc), C.c_void_p]),
    'sr_gfpgan_upconv_f32': (C.c_int, [C.POINTER(GfpganModconvDesc), C.c_void_p]),
    'sr_gfpgan_blur_up_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_float,
                                        C.POINTER(GfpganTail), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'sr_gfpgan_torgb_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol include/sr_hip_edsr.h declares
EDSR_SIGNATURES = {
    'sr_cb16_pixel_shuffle_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p]),
    'sr_edsr_shift_in_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.c_float, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p]),
    'sr_edsr_shift_in_bf16': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.c_float, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p]),
    'sr_edsr_shift_out_f32': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}

# name -> (restype, argtypes); every symbol include/sr_hip_ca_bf16.h declares
CA_BF16_SIGNATURES = {
    'sr_ca_workspace_bytes_bf16': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'sr_ca_squeeze_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_ca_excite_bf16': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_float, C.c_void_p]),
}


class DcnDesc(C.Structure):
    """struct sr_dcn_desc (include/sr_hip_dcn.h)."""
    _fields_ = [('x', C.c_void_p), ('x_img_stride', C.c_int64), ('offset', C.c_void_p), ('offset_img_stride', C.c_int64),
                ('mask', C.c_void_p), ('mask_img_stride', C.c_int64), ('mask_is_logit', C.c_int), ('wpacked', C.c_void_p),
                ('bpacked', C.c_void_p), ('out', C.c_void_p), ('out_img_stride', C.c_int64), ('n', C.c_int), ('cin', C.c_int),
                ('cout', C.c_int), ('h', C.c_int), ('w', C.c_int), ('deformable_groups', C.c_int), ('ksize', C.c_int),
                ('stride', C.c_int), ('padding', C.c_int), ('dilation', C.c_int), ('groups', C.c_int), ('act_slope', C.c_float)]


class DcnBwdDesc(C.Structure):
    """struct sr_dcn_bwd_desc (include/sr_hip_dcn.h)."""
    _fields_ = [('fwd', DcnDesc), ('dcol', C.c_void_p), ('dx', C.c_void_p), ('dx_img_stride', C.c_int64), ('doffset', C.c_void_p),
                ('doffset_img_stride', C.c_int64), ('dmask', C.c_void_p), ('dmask_img_stride', C.c_int64)]


# name -> (restype, argtypes); every symbol include/sr_hip_dcn.h declares
DCN_SIGNATURES = {
    'sr_dcn_fwd_f32': (C.c_int, [C.POINTER(DcnDesc), C.c_void_p]),
    'sr_dcn_cols_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'sr_dcn_cols_f32': (C.c_int, [C.POINTER(DcnDesc), C.c_void_p, C.c_size_t, C.c_void_p]),
    'sr_dcn_packed_t_weight_floats': (C.c_size_t, [C.c_int, C.c_int]),
    'sr_dcn_pack_t_f32': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'sr_dcn_weight_unpack_f32': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'sr_dcn_bwd_data_f32': (C.c_int, [C.POINTER(DcnBwdDesc), C.c_void_p]),
}


class ConvS2Desc(C.Structure):
    """struct sr_conv3x3s2_desc (include/sr_hip_edvr.h)."""
    _fields_ = [('in_', C.c_void_p), ('in_img_stride', C.c_int64), ('cin_pad', C.c_int), ('in_h', C.c_int), ('in_w', C.c_int),
                ('wpacked', C.c_void_p), ('bpacked', C.c_void_p), ('cout', C.c_int), ('out', C.c_void_p),
                ('out_img_stride', C.c_int64), ('n', C.c_int), ('act_slope', C.c_float)]


_P, _S, _I = C.c_void_p, C.c_int64, C.c_int
# name -> (restype, argtypes); every symbol include/sr_hip_edvr.h declares
EDVR_SIGNATURES = {
    'sr_conv3x3s2_f32': (C.c_int, [C.POINTER(ConvS2Desc), _P]),
    'sr_conv3x3s2_lds_bytes': (C.c_size_t, [_I, _I, _I, _I]),
    'sr_cb8_zero_insert2_f32': (C.c_int, [_P, _S, _P, _S, _I, _I, _I, _I, _P]),
    'sr_pool3x3s2_fwd_f32': (C.c_int, [_P, _S, _P, _S, _P, _S, _I, _I, _I, _I, _P]),
    'sr_pool3x3s2_bwd_f32': (C.c_int, [_P, _S, _P, _S, _P, _S, _P, _S, _I, _I, _I, _I, _P]),
    'sr_tsa_corr_fwd_f32': (C.c_int, [_P, _S, _P, _S, _P, _S, _P, _P, _S, _I, _I, _I, _I, _I, _P]),
    'sr_tsa_corr_bwd_f32': (C.c_int, [_P, _S, _P, _S, _P, _S, _P, _S, _P, _P, _P, _S, _P, _S, _P, _S, _I, _I, _I, _I, _I, _P]),
    'sr_tsa_gate_fwd_f32': (C.c_int, [_P, _S, _P, _S, _P, _S, _P, _S, _I, _I, _I, _I, _P]),
    'sr_tsa_gate_bwd_f32': (C.c_int, [_P, _S, _P, _S, _P, _S, _P, _S, _P, _S, _I, _I, _I, _I, _P]),
}


class DcnBf16Desc(C.Structure):
    """struct sr_dcn_bf16_desc (include/sr_hip_edvr_bf16.h)."""
    _fields_ = [('x', C.c_void_p), ('x_img_stride', C.c_int64), ('offset', C.c_void_p), ('offset_img_stride', C.c_int64),
                ('mask', C.c_void_p), ('mask_img_stride', C.c_int64), ('mask_is_logit', C.c_int), ('wpacked', C.c_void_p),
                ('bpacked', C.c_void_p), ('out', C.c_void_p), ('out_img_stride', C.c_int64), ('n', C.c_int), ('cin', C.c_int),
                ('cout', C.c_int), ('h', C.c_int), ('w', C.c_int), ('deformable_groups', C.c_int), ('ksize', C.c_int),
                ('stride', C.c_int), ('padding', C.c_int), ('dilation', C.c_int), ('groups', C.c_int), ('act_slope', C.c_float)]


# name -> (restype, argtypes); every symbol include/sr_hip_edvr_bf16.h declares
EDVR_BF16_SIGNATURES = {
    'sr_dcn_fwd_bf16': (C.c_int, [C.POINTER(DcnBf16Desc), _P]),
    'sr_dcn_bf16_lds_bytes': (C.c_size_t, [_I, _I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'sr_conv1x1_packed_weight_elems_bf16': (C.c_size_t, [_I, _I]),
    'sr_conv1x1_pack_bf16': (C.c_int, [_P, _P, _I, _I, _P, _P, _P]),
    'sr_conv1x1_bf16': (C.c_int, [_P, _S, _P, _P, _P, _S, _I, _I, _I, _I, _I, C.c_float, _P]),
    'sr_cb16_subsample2_bf16': (C.c_int, [_P, _S, _P, _S, _I, _I, _I, _I, _P]),
    'sr_pool3x3s2_fwd_bf16': (C.c_int, [_P, _S, _P, _S, _P, _S, _I, _I, _I, _I, _P]),
    'sr_tsa_corr_fwd_bf16': (C.c_int, [_P, _S, _P, _S, _P, _S, _P, _P, _S, _I, _I, _I, _I, _I, _P]),
    'sr_tsa_gate_fwd_bf16': (C.c_int, [_P, _S, _P, _S, _P, _S, _P, _S, _I, _I, _I, _I, _P]),
}

# name -> (restype, argtypes); every symbol include/sr_hip_stylegan2.h declares
STYLEGAN2_SIGNATURES = {
    'sr_upfirdn2d_f32': (C.c_int, [_P, _S, _P, _S, _P] + [_I] * 15 + [_P]),
    'sr_upfirdn2d_instance': (C.c_int, [_I, _I, _I, _I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    'sr_fused_bias_act_f32': (C.c_int, [_P, _P, _P, _P, _I, _I, _S, C.c_float, C.c_float, _P]),
    'sr_fused_bias_act_workspace_bytes': (C.c_size_t, [_I, _I, _S]),
    'sr_fused_bias_act_bwd_f32': (C.c_int, [_P, _P, _P, _P, _I, _I, _S, C.c_float, C.c_float, _P, C.c_size_t, _P]),
}


class AdamClass(C.Structure):
    """struct sr_adam_class (include/sr_hip_train_groups.h)."""
    _fields_ = [('lr', C.c_float), ('step', C.c_int), ('active', C.c_int)]


# name -> (restype, argtypes); every symbol include/sr_hip_train_groups.h declares
TRAIN_GROUPS_SIGNATURES = {
    'sr_adam_step_groups_f32': (C.c_int, [_P, _P, _P, _P, _S, _P, C.POINTER(AdamClass), _I] + [C.c_float] * 5 + [_P, _P, _P]),
    'sr_adam_class_table': (C.c_int, [C.POINTER(AdamClass), _I, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_float), C.POINTER(C.c_int)]),
}

# name -> (restype, argtypes); every symbol include/sr_hip_degrade.h declares
DEGRADE_SIGNATURES = {
    'sr_filter2d_f32': (C.c_int, [_P, _P, _P] + [_I] * 6 + [_P]),
    'sr_resize_bilinear_f32': (C.c_int, [_P, _P, _P, _P] + [_I] * 6 + [_P]),
    'sr_add_gaussian_noise_f32': (C.c_int, [_P] * 6 + [_I] * 6 + [_P]),
    'sr_diffjpeg_f32': (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'sr_diffjpeg_bwd_f32': (C.c_int, [_P] * 5 + [_I, _I, _I, _P]),
    'sr_degrade_finish_f32': (C.c_int, [_P, _P, _P, _P, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
}


class Conv7x7Desc(C.Structure):
    """struct sr_conv7x7_desc (include/sr_hip_flow.h)."""
    _fields_ = [('in_', C.c_void_p), ('in_img_stride', C.c_longlong), ('cin', C.c_int), ('cout', C.c_int), ('n', C.c_int),
                ('h', C.c_int), ('w', C.c_int), ('packed', C.c_void_p), ('out', C.c_void_p), ('out_img_stride', C.c_longlong),
                ('relu', C.c_int), ('res1', C.c_void_p), ('res1_img_stride', C.c_longlong)]


# name -> (restype, argtypes); every symbol include/sr_hip_flow.h declares
FLOW_SIGNATURES = {
    'sr_conv7x7_instance': (C.c_int, [_I, _I]),
    'sr_conv7x7_packed_floats': (C.c_size_t, [_I, _I]),
    'sr_conv7x7_pack_f32': (C.c_int, [_P, _P, _I, _I, _P, _P]),
    'sr_conv7x7_f32': (C.c_int, [C.POINTER(Conv7x7Desc), _P]),
    'sr_flow_warp_f32': (C.c_int, [_P, _P, _P] + [_I] * 6 + [_P]),
    'sr_flow_warp_bwd_f32': (C.c_int, [_P] * 5 + [_I] * 6 + [_P]),
    'sr_spynet_level_input_f32': (C.c_int, [_P] * 5 + [_I] * 3 + [_P]),
    'sr_spynet_preprocess_f32': (C.c_int, [_P, _P, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    'sr_avgpool2x2_f32': (C.c_int, [_P, _P, _I, _I, _I, _P]),
}


class Conv7x7DgradDesc(C.Structure):
    """struct sr_conv7x7_dgrad_desc (include/sr_hip_flow_bwd.h)."""
    _fields_ = [('dy', C.c_void_p), ('dy_img_stride', C.c_longlong), ('cin', C.c_int), ('cout', C.c_int), ('n', C.c_int),
                ('h', C.c_int), ('w', C.c_int), ('packed', C.c_void_p), ('dx', C.c_void_p), ('dx_img_stride', C.c_longlong),
                ('mask', C.c_void_p), ('mask_img_stride', C.c_longlong)]


class Conv7x7WgradDesc(C.Structure):
    """struct sr_conv7x7_wgrad_desc (include/sr_hip_flow_bwd.h)."""
    _fields_ = [('x', C.c_void_p), ('x_img_stride', C.c_longlong), ('dy', C.c_void_p), ('dy_img_stride', C.c_longlong),
                ('cin', C.c_int), ('cout', C.c_int), ('n', C.c_int), ('h', C.c_int), ('w', C.c_int), ('scale', C.c_float),
                ('dweight', C.c_void_p), ('dbias', C.c_void_p), ('accumulate', C.c_int), ('slab', C.c_void_p),
                ('slab_bytes', C.c_size_t)]


# name -> (restype, argtypes); every symbol include/sr_hip_flow_bwd.h declares
FLOW_BWD_SIGNATURES = {
    'sr_conv7x7_dgrad_instance': (C.c_int, [_I, _I]),
    'sr_conv7x7_dgrad_packed_floats': (C.c_size_t, [_I, _I]),
    'sr_conv7x7_dgrad_pack_f32': (C.c_int, [_P, _I, _I, _P, _P]),
    'sr_conv7x7_dgrad_f32': (C.c_int, [C.POINTER(Conv7x7DgradDesc), _P]),
    'sr_conv7x7_wgrad_slab_bytes': (C.c_size_t, [_I] * 5),
    'sr_conv7x7_wgrad_f32': (C.c_int, [C.POINTER(Conv7x7WgradDesc), _P]),
    'sr_spynet_level_input_bwd_f32': (C.c_int, [_P] * 6 + [_I] * 3 + [_P]),
    'sr_resize_bilinear_adjoint_f32': (C.c_int, [_P, _P] + [_I] * 5 + [_P]),
}


class VsrPropDesc(C.Structure):
    """struct sr_vsr_prop_desc (include/sr_hip_vsr.h)."""
    _fields_ = [('frame', C.c_void_p), ('frame_img_stride', C.c_longlong), ('prev', C.c_void_p), ('prev_img_stride', C.c_longlong),
                ('flow', C.c_void_p), ('flow_img_stride', C.c_longlong), ('frame_out', C.c_void_p),
                ('frame_out_img_stride', C.c_longlong), ('warp_out', C.c_void_p), ('warp_out_img_stride', C.c_longlong),
                ('n', C.c_int), ('h', C.c_int), ('w', C.c_int), ('fb', C.c_int)]


class VsrTrunkCfg(C.Structure):
    """struct sr_vsr_trunk_cfg (include/sr_hip_vsr.h)."""
    _fields_ = [('num_feat', C.c_int), ('num_block', C.c_int), ('cin_segs', C.c_int)]


# name -> (restype, argtypes); every symbol include/sr_hip_vsr.h declares
VSR_SIGNATURES = {
    'sr_vsr_prop_input_f32': (C.c_int, [C.POINTER(VsrPropDesc), _P]),
    'sr_vsr_trunk_num_params': (C.c_int, [C.POINTER(VsrTrunkCfg)]),
    'sr_vsr_trunk_conv_wino': (C.c_int, [C.POINTER(VsrTrunkCfg), _I]),
    'sr_vsr_trunk_packed_bytes': (C.c_size_t, [C.POINTER(VsrTrunkCfg)]),
    'sr_vsr_trunk_pack_f32': (C.c_int, [C.POINTER(VsrTrunkCfg), C.POINTER(C.c_void_p), _P, _P]),
    'sr_vsr_trunk_workspace_bytes': (C.c_size_t, [C.POINTER(VsrTrunkCfg), _I, _I, _I]),
    'sr_vsr_trunk_f32': (C.c_int, [C.POINTER(VsrTrunkCfg), _P, _P, C.c_longlong, _P, C.c_longlong, _I, _I, _I, _P, C.c_size_t, _P]),
}


class RvsrPropDesc(C.Structure):
    """struct sr_rvsr_prop_desc (include/sr_hip_vsr_bf16.h)."""
    _fields_ = VsrPropDesc._fields_


# name -> (restype, argtypes); every symbol include/sr_hip_vsr_bf16.h declares
VSR_BF16_SIGNATURES = {
    'sr_rvsr_prop_input_bf16': (C.c_int, [C.POINTER(RvsrPropDesc), _P]),
    'sr_rvsr_trunk_packed_bytes_bf16': (C.c_size_t, [C.POINTER(VsrTrunkCfg)]),
    'sr_rvsr_trunk_pack_bf16': (C.c_int, [C.POINTER(VsrTrunkCfg), C.POINTER(C.c_void_p), _P, _P]),
    'sr_rvsr_trunk_workspace_bytes_bf16': (C.c_size_t, [C.POINTER(VsrTrunkCfg), _I, _I, _I]),
    'sr_rvsr_trunk_bf16': (C.c_int, [C.POINTER(VsrTrunkCfg), _P, _P, C.c_longlong, _P, C.c_longlong, _I, _I, _I, _P, C.c_size_t, _P]),
}



class VsrPropBwdDesc(C.Structure):
    """struct sr_vsr_prop_bwd_desc (include/sr_hip_vsr_bwd.h)."""
    _fields_ = [('g', C.c_void_p), ('g_img_stride', C.c_longlong), ('prev', C.c_void_p), ('prev_img_stride', C.c_longlong),
                ('flow', C.c_void_p), ('flow_img_stride', C.c_longlong), ('dprev', C.c_void_p), ('dprev_img_stride', C.c_longlong),
                ('dflow', C.c_void_p), ('dflow_img_stride', C.c_longlong), ('n', C.c_int), ('h', C.c_int), ('w', C.c_int),
                ('fb', C.c_int)]


class VsrTrunkBwdDesc(C.Structure):
    """struct sr_vsr_trunk_bwd_desc (include/sr_hip_vsr_bwd.h)."""
    _fields_ = [('packed_dgrad', C.c_void_p), ('in_', C.c_void_p), ('in_img_stride', C.c_longlong), ('out', C.c_void_p),
                ('out_img_stride', C.c_longlong), ('stack', C.c_void_p), ('stack_bytes', C.c_size_t), ('dout', C.c_void_p),
                ('dout_img_stride', C.c_longlong), ('din', C.c_void_p), ('din_img_stride', C.c_longlong),
                ('dparams', C.POINTER(C.c_void_p)), ('accumulate', C.c_int), ('n', C.c_int), ('h', C.c_int), ('w', C.c_int),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


# name -> (restype, argtypes); every symbol include/sr_hip_vsr_bwd.h declares
VSR_BWD_SIGNATURES = {
    'sr_vsr_prop_input_bwd_f32': (C.c_int, [C.POINTER(VsrPropBwdDesc), _P]),
    'sr_vsr_trunk_keep_bytes': (C.c_size_t, [C.POINTER(VsrTrunkCfg), _I, _I, _I]),
    'sr_vsr_trunk_keep_f32': (C.c_int, [C.POINTER(VsrTrunkCfg), _P, _P, C.c_longlong, _P, C.c_longlong, _I, _I, _I, _P, C.c_size_t, _P]),
    'sr_vsr_trunk_packed_dgrad_bytes': (C.c_size_t, [C.POINTER(VsrTrunkCfg)]),
    'sr_vsr_trunk_pack_dgrad_f32': (C.c_int, [C.POINTER(VsrTrunkCfg), C.POINTER(C.c_void_p), _P, _P]),
    'sr_vsr_trunk_bwd_workspace_bytes': (C.c_size_t, [C.POINTER(VsrTrunkCfg), _I, _I, _I]),
    'sr_vsr_trunk_bwd_f32': (C.c_int, [C.POINTER(VsrTrunkCfg), C.POINTER(VsrTrunkBwdDesc), _P]),
}


class VsrPropBwdDetDesc(C.Structure):
    """struct sr_vsr_prop_bwd_det_desc (include/sr_hip_vsr_det.h)."""
    _fields_ = [('d', VsrPropBwdDesc), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


# name -> (restype, argtypes); every symbol include/sr_hip_vsr_det.h declares
VSR_DET_SIGNATURES = {
    'sr_vsr_prop_input_bwd_det_workspace_bytes': (C.c_size_t, [_I, _I, _I, _I]),
    'sr_vsr_prop_input_bwd_det_f32': (C.c_int, [C.POINTER(VsrPropBwdDetDesc), _P]),
}


class DcnBwdDetDesc(C.Structure):
    """struct sr_dcn_bwd_det_desc (include/sr_hip_dcn_det.h)."""
    _fields_ = [('d', DcnBwdDesc), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


# name -> (restype, argtypes); every symbol include/sr_hip_dcn_det.h declares
DCN_DET_SIGNATURES = {
    'sr_dcn_bwd_data_det_workspace_bytes': (C.c_size_t, [_I, _I, _I, _I]),
    'sr_dcn_bwd_data_det_f32': (C.c_int, [C.POINTER(DcnBwdDetDesc), _P]),
}


class TofConv9x9Desc(C.Structure):
    """struct sr_tof_conv9x9_desc (include/sr_hip_tof.h)."""
    _fields_ = [('in_', C.c_void_p), ('in_img_stride', C.c_longlong), ('cin', C.c_int), ('cout', C.c_int), ('n', C.c_int),
                ('h', C.c_int), ('w', C.c_int), ('packed', C.c_void_p), ('out', C.c_void_p), ('out_img_stride', C.c_longlong),
                ('relu', C.c_int)]


# name -> (restype, argtypes); every symbol include/sr_hip_tof.h declares
TOF_SIGNATURES = {
    'sr_tof_conv9x9_packed_floats': (C.c_size_t, [_I, _I]),
    'sr_tof_conv9x9_pack_f32': (C.c_int, [_P, _P, _I, _I, _P, _P]),
    'sr_tof_conv9x9_f32': (C.c_int, [C.POINTER(TofConv9x9Desc), _P]),
    'sr_tof_level_input_f32': (C.c_int, [_P, C.c_longlong, _P, C.c_longlong, _I, _I, _P, _P, _P, _I, _I, _I, _P]),
    'sr_tof_align_f32': (C.c_int, [_P, _P, C.c_longlong, _P, C.c_longlong, _I, _I, _I, _I, _P]),
    'sr_tof_finish_f32': (C.c_int, [_P, C.c_longlong, _P, C.c_longlong, _P, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
}


class DufConvDesc(C.Structure):
    """struct sr_duf_conv_desc (include/sr_hip_duf.h)."""
    _fields_ = [('in_', C.c_void_p), ('in_frame_stride', C.c_longlong), ('in_clip_stride', C.c_longlong), ('cin', C.c_int),
                ('cout', C.c_int), ('kt', C.c_int), ('pad_t', C.c_int), ('b', C.c_int), ('t', C.c_int), ('h', C.c_int), ('w', C.c_int),
                ('packed', C.c_void_p), ('scale', C.c_void_p), ('shift', C.c_void_p), ('out', C.c_void_p),
                ('out_frame_stride', C.c_longlong), ('out_clip_stride', C.c_longlong), ('out_cb0', C.c_int), ('relu', C.c_int)]


# name -> (restype, argtypes); every symbol include/sr_hip_duf.h declares
DUF_SIGNATURES = {
    'sr_duf_conv3d_packed_floats': (C.c_size_t, [_I, _I, _I]),
    'sr_duf_conv3d_pack_f32': (C.c_int, [_P, _P, _I, _I, _I, _P, _P]),
    'sr_duf_conv3d_f32': (C.c_int, [C.POINTER(DufConvDesc), _P]),
    'sr_duf_pw_packed_floats': (C.c_size_t, [_I]),
    'sr_duf_pw_pack_f32': (C.c_int, [_P, _P, _I, _P, _P]),
    'sr_duf_pw_f32': (C.c_int, [C.POINTER(DufConvDesc), _P]),
    'sr_duf_filter_f32': (C.c_int, [_P, C.c_longlong, _P, C.c_longlong, _P, C.c_longlong, _P, _I, _I, _I, _I, _I, _I, _P]),
}

_lib = None


def load():
    """Loads libsr_hip.so (once).  Raises if it is missing or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SrHipError(f'{LIB_PATH} is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                         '(or `make -C image_restoration_amd/csrc`). There is no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(RIDNET_SIGNATURES.items()) + list(GFPGAN_SIGNATURES.items()) \
            + list(EDSR_SIGNATURES.items()) + list(CA_BF16_SIGNATURES.items()) + list(DCN_SIGNATURES.items()) + list(EDVR_SIGNATURES.items()) \
            + list(EDVR_BF16_SIGNATURES.items()) + list(STYLEGAN2_SIGNATURES.items()) + list(TRAIN_GROUPS_SIGNATURES.items()) \
            + list(DEGRADE_SIGNATURES.items()) + list(FLOW_SIGNATURES.items()) + list(VSR_SIGNATURES.items()) + list(VSR_BF16_SIGNATURES.items()) \
            + list(FLOW_BWD_SIGNATURES.items()) + list(VSR_BWD_SIGNATURES.items()) + list(VSR_DET_SIGNATURES.items()) \
            + list(DCN_DET_SIGNATURES.items()) + list(TOF_SIGNATURES.items()) + list(DUF_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    v = lib.sr_version()
    if v != SR_ABI_VERSION:
        raise SrHipError(f'libsr_hip.so ABI {v} != expected {SR_ABI_VERSION}: rebuild')
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().sr_last_error().decode('utf-8', 'replace')
        raise SrHipError(f'{what} failed (status {rc}): {msg}')
