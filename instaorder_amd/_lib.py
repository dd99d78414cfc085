"""ctypes binding of libinstaorder_hip.so (the C ABI declared in include/instaorder_hip.h).

There is NO fallback: if the shared library is missing, or an op is invoked without a
gfx950 device, a RuntimeError is raised.  Build with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C instaorder_amd/csrc``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# IO_LIB_PATH: a tuning build of the same library (csrc/Makefile VARIANT=...), for same-box A/B runs of kernel variants
LIB_PATH = os.environ.get("IO_LIB_PATH") or os.path.join(_HERE, "libinstaorder_hip.so")
_lib = None

c_float_p = C.c_void_p   # device pointers travel as integers (tensor.data_ptr())


def csrc_digest():
    """sha256 over the kernel sources (csrc/*.hip, csrc/*.h, the public header), in name order: what a measurement of a
    kernel (a PMC profile under profiles/) was taken on.  bench.py quotes such a measurement only while this matches."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "instaorder_hip.h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


class TensorInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("kind", C.c_int), ("ndim", C.c_int), ("shape", C.c_long * 4),
                ("offset", C.c_long), ("numel_storage", C.c_long), ("cin_storage", C.c_int),
                ("bn_index", C.c_int), ("running_offset", C.c_long)]


class PairDesc(C.Structure):
    _fields_ = [("image_off", C.c_int64), ("mask1_off", C.c_int64), ("mask2_off", C.c_int64), ("H", C.c_int32),
                ("W", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("flip", C.c_int32), ("interp", C.c_int32)]


class RleDesc(C.Structure):
    """io_rle_desc of include/instaorder_hip.h"""
    _fields_ = [("ends_off", C.c_int64), ("n_runs", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("value", C.c_int32), ("out_off", C.c_int64)]


class PolyPart(C.Structure):
    """io_poly_part of include/instaorder_hip.h"""
    _fields_ = [("vert_off", C.c_int64), ("n_verts", C.c_int32), ("mask", C.c_int32)]


class PolyMask(C.Structure):
    """io_poly_mask of include/instaorder_hip.h"""
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("value", C.c_int32), ("first_part", C.c_int32),
                ("n_parts", C.c_int32), ("reserved", C.c_int32), ("out_off", C.c_int64)]


class JpegDesc(C.Structure):
    """io_jpeg_desc of include/instaorder_hip.h"""
    _fields_ = [("data_off", C.c_int64), ("out_off", C.c_int64), ("data_bytes", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("n_comp", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("restart_interval", C.c_int32), ("table_set", C.c_int32), ("quant", C.c_uint8 * 4), ("dc", C.c_uint8 * 4),
                ("ac", C.c_uint8 * 4), ("reserved", C.c_int32)]


class JpegHuffRaw(C.Structure):
    """io_jpeg_huff_raw of include/instaorder_hip.h"""
    _fields_ = [("counts", C.c_uint8 * 16), ("symbols", C.c_uint8 * 256)]


class JpegProgScan(C.Structure):
    """io_jpeg_prog_scan of include/instaorder_hip.h"""
    _fields_ = [("data_off", C.c_int64), ("data_bytes", C.c_int32), ("image", C.c_int32), ("restart_interval", C.c_int32),
                ("level", C.c_int32), ("table", C.c_int32 * 3), ("n_comp", C.c_uint8), ("comp", C.c_uint8 * 3),
                ("ss", C.c_uint8), ("se", C.c_uint8), ("ah", C.c_uint8), ("al", C.c_uint8), ("reserved", C.c_int32 * 5)]


class JpegProgImage(C.Structure):
    """io_jpeg_prog_image of include/instaorder_hip.h"""
    _fields_ = [("first_scan", C.c_int32), ("n_scans", C.c_int32), ("n_levels", C.c_int32), ("reserved", C.c_int32)]


class PngDesc(C.Structure):
    """io_png_desc of include/instaorder_hip.h"""
    _fields_ = [("data_off", C.c_int64), ("out_off", C.c_int64), ("data_bytes", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("channels", C.c_int32), ("depth", C.c_int32), ("adler", C.c_uint32),
                ("reserved", C.c_int32 * 2)]


class DgradFused(C.Structure):
    """io_dgrad_fused of include/instaorder_hip.h (device pointers as integers, None = NULL)"""
    _fields_ = [(n, C.c_void_p) for n in ("xb_y", "xb_coef", "xb_dy_out", "add", "relu_mask", "ep_y", "ep_mean", "ep_rstd",
                                          "ep_scale", "ep_shift", "ep_act_out", "ep_p1", "ep_p2", "wino_scratch")] + \
               [("wino_scratch_floats", C.c_size_t), ("relu_maskbits", C.c_void_p)]


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_long), ("total_ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double), ("flops_executed", C.c_double)]


class ClipState(C.Structure):
    """io_clip_state of include/instaorder_hip.h: the 64-byte device record io_grad_norm leaves for the clipped updates"""
    _fields_ = [("norm", C.c_float), ("coef", C.c_float), ("nonfinite", C.c_int), ("reserved0", C.c_int),
                ("steps", C.c_uint64), ("clipped", C.c_uint64), ("skipped", C.c_uint64), ("reserved", C.c_uint64 * 3)]


_P, _I, _L, _F, _Z = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_size_t
_D = C.c_double

# name -> (restype, argtypes); every symbol include/instaorder_hip.h declares
SIGNATURES = {
    "io_abi_version": (_I, []),
    "io_last_error_string": (C.c_char_p, []),
    "io_device_count": (_I, []),
    "io_set_winograd": (_I, [_I]),
    "io_get_winograd": (_I, []),
    "io_set_bf16_p256": (_I, [_I]),
    "io_get_bf16_p256": (_I, []),
    "io_set_bf16_p256_xop": (_I, [_I]),
    "io_get_bf16_p256_xop": (_I, []),
    "io_conv2d_fwd_resid_dt": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "io_debug_last_nt_route": (_I, []),
    "io_conv2d_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "io_conv2d_bnstats_workspace_floats": (_Z, [_I, _I, _I, _I, _I, _I, _I, _I, _I]),
    "io_conv2d_fwd_bnstats": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _F, _F, _P, _P,
                                   _P, _P, _P, _Z, _P]),
    "io_conv2d_dgrad": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "io_conv2d_dgrad_bnbwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P,
                                   _P, _Z, _P]),
    "io_conv2d_wgrad_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I, _I, _I]),
    "io_conv2d_wgrad": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "io_filter_transpose": (_I, [_P, _I, _I, _I, _P, _P]),
    "io_bn_partial_floats": (_Z, [_I, _I, _I]),
    "io_bn_stats_finalize": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _Z, _P]),
    "io_bn_eval_prepare": (_I, [_I, _P, _P, _P, _P, _F, _P, _P, _P, _P]),
    "io_bn_apply": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "io_bn_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _P]),
    "io_maxpool_fwd": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "io_maxpool_bwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "io_avgpool_fc_fwd": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P, _P]),
    "io_avgpool_fc_bwd": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "io_pack_planes_nhwc8": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_long), _I, _I, _I, _I, _P, _P]),
    "io_pair_planes_u8": (_I, [_P, _Z, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "io_pair_planes_u8_hw": (_I, [_P, _Z, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    # ends_dev, ends_count, desc_dev, desc_host, n, out, out_bytes, stream
    "io_rle_decode_u8": (_I, [_P, _Z, _P, _P, _I, _P, _Z, _P]),
    "io_rle_lds_runs": (_I, []),
    # verts_dev, n_verts, parts_dev, parts_host, n_parts, masks_dev, masks_host, n_masks, out, out_bytes, workspace,
    # workspace_bytes, stream
    "io_poly_fill_u8": (_I, [_P, _Z, _P, _P, _I, _P, _P, _I, _P, _Z, _P, _Z, _P]),
    "io_poly_fill_workspace_bytes": (_Z, [_P, _I, _P, _I]),
    "io_poly_scan_words": (_I, []),
    # pool_dev, pool_bytes, tables_dev, tables_host, tables_bytes, desc_dev, desc_host, n, out, out_bytes, workspace,
    # workspace_bytes, status_dev, stream
    "io_jpeg_decode_u8": (_I, [_P, _Z, _P, _P, _Z, _P, _P, _I, _P, _Z, _P, _Z, _P, _P]),
    "io_jpeg_workspace_bytes": (_Z, [_P, _I]),
    # the arguments of io_jpeg_decode_u8 up to status_dev, then subseq_bytes, max_rounds, info_dev, stream
    "io_jpeg_decode_par_u8": (_I, [_P, _Z, _P, _P, _Z, _P, _P, _I, _P, _Z, _P, _Z, _P, _I, _I, _P, _P]),
    "io_jpeg_par_workspace_bytes": (_Z, [_P, _I, _I]),
    # pool_dev, pool_bytes, tables_dev, tables_host, tables_bytes, huff_dev, huff_host, n_huff, desc_dev, desc_host, image_dev,
    # image_host, n, scan_dev, scan_host, n_scans, out, out_bytes, workspace, workspace_bytes, status_dev, concurrent, stream
    "io_jpeg_decode_prog_u8": (_I, [_P, _Z, _P, _P, _Z, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _Z, _P, _Z, _P, _I, _P]),
    "io_jpeg_prog_workspace_bytes": (_Z, [_P, _I, _I, _I]),
    "io_jpeg_set_images_per_wave": (_I, [_I]),
    "io_jpeg_get_images_per_wave": (_I, []),
    "io_jpeg_lds_table_sets": (_I, []),
    # pool_dev, pool_bytes, desc_dev, desc_host, n, out, out_bytes, workspace, workspace_bytes, status_dev, stream
    "io_png_decode": (_I, [_P, _Z, _P, _P, _I, _P, _Z, _P, _Z, _P, _P]),
    "io_png_workspace_bytes": (_Z, [_P, _I]),
    "io_png_band_rows": (_I, []),
    # the arguments of io_png_decode up to status_dev, then chunk_bytes, info_dev, stream
    "io_png_decode_par": (_I, [_P, _Z, _P, _P, _I, _P, _Z, _P, _Z, _P, _I, _P, _P]),
    "io_png_par_workspace_bytes": (_Z, [_P, _I, _I]),
    "io_order_loss": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _F, _F, _F, _P, _P, _P]),
    "io_sgd_momentum": (_I, [_P, _P, _P, _Z, _F, _F, _F, _P]),
    # params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, stream
    "io_adam_step": (_I, [_P, _P, _P, _P, _Z, _D, _D, _D, _F, _F, _D, _D, _P]),
    # grads, n, seg_offsets (host size_t[nseg + 1]), nseg, max_norm, workspace, workspace_bytes, seg_sumsq, state, stream
    "io_grad_norm": (_I, [_P, _Z, C.POINTER(C.c_size_t), _I, _F, _P, _Z, _P, _P, _P]),
    "io_grad_norm_workspace_bytes": (_Z, [_Z, _I]),
    "io_grad_norm_chunk_floats": (_I, []),
    # io_sgd_momentum / io_adam_step with the io_clip_state record in front of the stream
    "io_sgd_momentum_clipped": (_I, [_P, _P, _P, _Z, _F, _F, _F, _P, _P]),
    "io_adam_step_clipped": (_I, [_P, _P, _P, _P, _Z, _D, _D, _D, _F, _F, _D, _D, _P, _P]),
    "io_net_create": (_P, [_I, _I, C.POINTER(C.c_int)]),
    "io_net_destroy": (None, [_P]),
    "io_net_param_floats": (_L, [_P]),
    "io_net_running_floats": (_L, [_P]),
    "io_net_num_tensors": (_I, [_P]),
    "io_net_tensor_info": (_I, [_P, _I, C.POINTER(TensorInfo)]),
    "io_net_num_logits": (_I, [_P]),
    "io_net_workspace_bytes": (_Z, [_P, _I, _I, _I]),
    "io_net_workspace_bytes_hw": (_Z, [_P, _I, _I, _I]),
    "io_net_forward_eval_hw": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P, _P]),
    "io_net_eval_taps_bytes": (_Z, [_P, _I, _I, _I]),
    "io_net_eval_tap_offset": (_L, [_P, _I, _I, _I, _I]),
    # net, params, running, x8, N, H, W, workspace, workspace_bytes, logits, taps, taps_bytes, routes (host int32), max_routes, stream
    "io_net_forward_eval_taps": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P, _P, _Z, C.POINTER(C.c_int32), _I, _P]),
    "io_net_activation_offset": (_L, [_P, _I, _I, _I]),
    "io_net_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _P, _P]),
    "io_net_backward": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "io_net_backward_num_stages": (_I, [_P]),
    "io_net_backward_stages": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _Z, _I, _I, _P]),
    # net, N, S, G, p256_mode, xop, ncu, out (host int32[max_blocks]), max_blocks
    "io_net_step_routes": (_I, [_P, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int32), _I]),
    "io_net_set_dtype": (_I, [_P, _I]),
    "io_net_get_dtype": (_I, [_P]),
    "io_pack_planes_nhwc8_dt": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "io_conv2d_fwd_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "io_conv2d_dgrad_dt": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "io_conv2d_wgrad_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _Z, _I, _I, _P]),
    "io_filter_prepare": (_I, [_P, _I, _I, _I, _P, _I, _I, _P]),
    "io_bn_stats_finalize_dt": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _Z, _I, _P]),
    "io_bn_apply_dt": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P]),
    "io_bn_apply_bits_dt": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "io_bn_bwd_dt": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _I, _P]),
    "io_gconv_pack": (_I, [_P, _I, _I, _I, _P, _P, _I, _P]),
    "io_gconv_unpack_grad": (_I, [_P, _I, _I, _I, _P, _P]),
    "io_gconv2d_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "io_gconv2d_dgrad": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "io_gconv2d_wgrad_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "io_gconv2d_wgrad": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _Z, _I, _P]),
    "io_upsample2x_bilinear_fwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "io_upsample2x_bilinear_bwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "io_bias_act": (_I, [_P, _P, _I, _I, _I, _P, _I, _P]),
    "io_relu_bwd": (_I, [_P, _P, _Z, _P, _I, _P]),
    "io_add": (_I, [_P, _P, _Z, _P, _I, _P]),
    "io_colsum_partial_floats": (_Z, [_I, _I]),
    "io_colsum": (_I, [_P, _I, _I, _P, _P, _Z, _I, _P]),
    "io_head1_fwd": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _I, _P]),
    "io_head1_bwd": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _Z, _I, _P]),
    "io_conv2d_fwd_bnstats_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _F, _F, _P,
                                      _P, _P, _P, _P, _Z, _I, _I, _P]),
    "io_conv2d_fwd_bias_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P]),
    "io_stem_packed_floats": (_Z, [_I]),
    "io_stem_wgrad_exact_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "io_stem_fwd_bnstats_exact": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _Z, _P,
                                       _P]),
    "io_stem_wgrad_exact": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _Z, _P, _P]),
    "io_stem_wgrad_exact_bn": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _P,
                                    _P]),
    # x8, da, y, dw, N, H, W, G, gamma, mean, rstd, scale, shift, dgamma, dbeta, coef, bn_partial, bn_partial_floats, ws, ws_bytes, stream
    "io_stem_wgrad_bn_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _P]),
    "io_stem_wgrad_bf16_workspace_bytes": (_Z, []),
    "io_debug_last_wgrad_route": (_I, []),
    "io_conv2d_fwd_resid": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P,
                                 _P, _P, _Z, _P]),
    "io_smooth_loss_workspace_floats": (_Z, [_I, _I, _I]),
    "io_smooth_loss_fwd": (_I, [_P, _P, _I, _I, _I, _F, _P, _P, _P, _Z, _P]),
    "io_smooth_loss_bwd": (_I, [_P, _P, _P, _F, _I, _I, _I, _I, _P, _P]),
    "io_disp_order_workspace_floats": (_Z, [_I, _I, _I]),
    "io_disp_order_count": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _Z, _P]),
    "io_bn_tile_partial_floats": (_Z, [_I, _I, _I]),
    "io_bn_bwd_coefs_dt": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _P]),
    "io_bn_bwd_coefs_from_tile_partials": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "io_conv2d_dgrad_fused_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(DgradFused), _I, _P]),
    "io_conv2d_dgrad_bnbwd_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                      _Z, _I, _I, _P]),
    "io_prof_launches": (_I, [_P, _I]),
    "io_weights_prepare": (_I, [_P, _I, _P, _P, _I, _P]),
    "io_weights_unpack_grads": (_I, [_P, _I, _P, _P, _P]),
    "io_maxpool_fwd_xf_dt": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _I, _P]),
    "io_conv2d_fwd_xf_dt": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _P,
                                 _P, _P, _P, _P, _Z, _I, _P]),
    "io_conv2d_wino_scratch_floats": (_Z, [_I, _I]),
    "io_conv2d_fwd_wino": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _Z,
                                _P, _Z, _P]),
    "io_maxpool_fwd_dt": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _P]),
    "io_maxpool_bwd_dt": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "io_avgpool_fc_fwd_dt": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P]),
    "io_avgpool_fc_bwd_dt": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    # pred, gt (uint16), B, H, W, gt_div, min_depth, max_depth, out (fp64 [B][10]), medians, workspace, workspace_bytes, stream
    "io_depth_errors_median_workspace_bytes": (_Z, [_I, _I, _I]),
    "io_depth_errors_median": (_I, [_P, _P, _I, _I, _I, _F, _F, _F, _P, _P, _P, _Z, _P]),
    "io_disp_sample_points": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    # masks (uint8), n, H, W, predicate, dilate, bits, stats, stream
    "io_mask_pack": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
    # p_bits, n_p, q_bits, n_q, H, W, counts, stream
    "io_mask_pair_counts": (_I, [_P, _I, _P, _I, _I, _I, _P, _P]),
    # masks (uint8), n, H, W, predicate, out (int32 [n][5]), stream
    "io_mask_bbox_u8": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "io_mask_bbox_band_rows": (_I, []),
    "io_instance_depth_select_workspace_bytes": (_Z, [_I, _I, _I]),
    # disp, H, W, masks, n, method, value, lo, hi, k, workspace, workspace_bytes, stream
    "io_instance_depth_select": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    # x, w_packed [9][Cin][32], bias, y, N, H, W, Cin, Cout (32), relu, stream
    "io_conv3x3_co32_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "io_set_unet_co32": (_I, [_I]),
    "io_get_unet_co32": (_I, []),
    "io_maxpool2x2_fwd": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    # x2 [N][2h][2w][C2], x1 [N][h][w][C1], N, h, w, C2, C1, out, stream
    "io_up2x_concat_fwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    # m1, m2, scale, P, HW, Cs, erase, out, stream
    "io_unet_pack_input": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "io_unet_head_partial_floats": (_Z, [_I, _I]),
    # act, wo, bo, m1, m2, target, P, HW, Cs, th, comp, counts, logits, partials, partial_floats, loss_sums, stream
    "io_unet_head": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _Z, _P, _P]),
    # dy, x, add, N, H, W, C, dx, stream
    "io_maxpool2x2_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    # dcat, N, h, w, C2, C1, dx2, dx1, stream
    "io_up2x_concat_bwd": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "io_unet_head_bwd_partial_floats": (_Z, [_I, _I]),
    # act, wo, bo, target, eraser, P, HW, Cs, inmask_weight, scale, gscale, dx, dwo, dbo, loss_sums, partials, partial_floats, stream
    "io_unet_head_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "io_prof_begin": (_I, []),
    "io_prof_begin_ex": (_I, [_I]),
    "io_prof_end": (_I, [C.POINTER(ProfEntry), _I]),
}


def lib():
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                "instaorder_amd: %s is missing -- the HIP extension has not been built "
                "(run `make -C instaorder_amd/csrc`). There is no CPU fallback." % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(_lib, name)
            fn.restype = res
            fn.argtypes = args
    return _lib


def last_error():
    return lib().io_last_error_string().decode()


def check(rc, what):
    if rc != 0:
        raise RuntimeError("instaorder_hip %s failed (%d): %s" % (what, rc, last_error()))


_gpu_ok = None


def require_gpu():
    """Fail loudly unless a gfx950 device is visible to HIP."""
    global _gpu_ok
    if _gpu_ok is None:
        _gpu_ok = lib().io_device_count() > 0
    if not _gpu_ok:
        raise RuntimeError("instaorder_amd: no gfx950 (MI355X) device visible; the HIP path cannot run "
                           "and there is no CPU fallback")
