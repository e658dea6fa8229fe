"""ctypes binding of libgwdepth_hip.so (C ABI: include/gwdepth.h).

There is no CPU fallback: importing works anywhere (so host-side logic can be unit-tested), but
every compute entry point raises HipUnavailable unless the shared library is present AND the
tensors live on a HIP device.  Tests may install a fake device library with `set_library()` to
exercise the host logic on CPU; the product never does.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GWD_LIB") or os.path.join(_HERE, "libgwdepth_hip.so")     # GWD_LIB: another build of the same ABI (same-box A/B of kernel variants)

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_GELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3, 4
WS_INORM_GELU, WS_RESAMPLE_BWD, WS_EVAL, WS_PLANE, WS_HEALTH, WS_REGIONS, WS_FUSION, WS_CLOUD, WS_SCENE, WS_VIEW = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9          # gwd_query_workspace ops
GATHER_CONV, GATHER_TRANSPOSED, GATHER_UPSAMPLED = 0, 1, 2
RESAMPLE_BILINEAR_AC, RESAMPLE_NEAREST = 0, 1

ENTRY_POINTS = [
    "gwd_version", "gwd_arch", "gwd_conv_forward", "gwd_conv_wgrad", "gwd_weight_prep", "gwd_act_backward",
    "gwd_colsum", "gwd_layernorm_forward", "gwd_layernorm_backward", "gwd_softmax_forward",
    "gwd_softmax_backward", "gwd_silog_sums", "gwd_silog_backward", "gwd_seg_ce_sum", "gwd_seg_ce_backward",
    "gwd_sqnorm", "gwd_adamw_step", "gwd_resample_forward", "gwd_resample_backward", "gwd_avgpool_forward",
    "gwd_avgpool_backward", "gwd_winattn_forward", "gwd_winattn_backward", "gwd_tokattn_forward",
    "gwd_tokattn_backward", "gwd_tokattn_pair_forward", "gwd_tokattn_pair_backward", "gwd_upsample_taps_collapse", "gwd_upsample_taps_fold", "gwd_certain_sample", "gwd_lsap", "gwd_window_map", "gwd_window_map_multi",
    "gwd_inorm_gelu_forward", "gwd_inorm_gelu_backward", "gwd_weight_prep_batch",
    "gwd_point_sample_forward", "gwd_point_sample_backward", "gwd_act_backward_colsum", "gwd_resample_backward_sep",
    "gwd_softmax_masked_forward", "gwd_softmax_scaled_backward", "gwd_query_workspace", "gwd_eval_accumulate", "gwd_colsum_batch", "gwd_conv_wgrad_batch",
    "gwd_conv_wgrad_takes_bias",
    "gwd_plane_loss_forward", "gwd_plane_loss_backward", "gwd_collate",
    "gwd_anchor_depth_forward", "gwd_anchor_depth_backward", "gwd_mha_flash_forward", "gwd_mha_flash_backward",
    "gwd_ref_scores_forward", "gwd_ref_scores_backward", "gwd_ref_mix_forward", "gwd_ref_mix_backward", "gwd_unpad_add_batch", "gwd_stem_pack", "gwd_stem_forward", "gwd_pos_sine", "gwd_silog_finalize", "gwd_psp_pool_forward", "gwd_psp_pool_backward",
    "gwd_match_cost", "gwd_set_losses_forward", "gwd_set_losses_backward", "gwd_set_losses_focal_forward", "gwd_set_losses_focal_backward", "gwd_resample_u8_pass", "gwd_gather2d", "gwd_point_sample_backward_gather", "gwd_point_sample_framed_forward", "gwd_point_sample_framed_backward", "gwd_stride_place", "gwd_color_adjust", "gwd_bmm",
    "gwd_dense_postprocess", "gwd_line_postprocess", "gwd_line_score",
    "gwd_dense_postprocess_resized",
    "gwd_resample_u8_pass_batch", "gwd_gather2d_batch", "gwd_color_adjust_batch",
    "gwd_pyr_tail_forward", "gwd_pyr_tail_backward", "gwd_pyr_tail_fold_wgrad",
    "gwd_widen_u16_batch",
    "gwd_line_nms",
    "gwd_eval_frames",
    "gwd_segment_stats", "gwd_health_decide", "gwd_adamw_step_guarded",
    "gwd_adamw_step_ema", "gwd_ema_swap",
    "gwd_glass_regions", "gwd_region_planes", "gwd_depth_planar",
    "gwd_line_profiles",
    "gwd_fusion_ring", "gwd_fusion_planes", "gwd_fusion_depth",
    "gwd_render_frames",
    "gwd_point_cloud",
    "gwd_scene_reset", "gwd_scene_integrate", "gwd_scene_extract",
    "gwd_cloud_view",
]


class HipUnavailable(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("w", ctypes.c_void_p), ("y", ctypes.c_void_p), ("z", ctypes.c_void_p),
                ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("residual", ctypes.c_void_p),
                ("zero_page", ctypes.c_void_p), ("mult", ctypes.c_void_p), ("gate", ctypes.c_void_p)] + \
               [(n, ctypes.c_int32) for n in ("B", "Hi", "Wi", "Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad",
                                              "gather", "Hv", "Wv", "act")] + \
               [("act_scale", ctypes.c_float), ("dtype", ctypes.c_int32), ("gate_act", ctypes.c_int32),
                ("ln_mean", ctypes.c_void_p), ("ln_rstd", ctypes.c_void_p), ("ln_C", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("dbias", ctypes.c_void_p)]


class BmmDesc(ctypes.Structure):
    """gwd_bmm_desc (include/gwdepth.h)."""
    _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("c", ctypes.c_void_p)] + \
               [(n, ctypes.c_int64) for n in ("a_sb0", "a_sb1", "a_ld", "b_sb0", "b_sb1", "b_ld", "c_sb0", "c_sb1", "c_ld")] + \
               [(n, ctypes.c_int32) for n in ("M", "N", "K", "nb0", "nb1", "a_kmajor", "b_kmajor", "c_is_f32_accumulate", "splits")] + \
               [("alpha", ctypes.c_float), ("dtype", ctypes.c_int32)]


class PrepJob(ctypes.Structure):
    """gwd_prep_job (include/gwdepth.h)."""
    _fields_ = [("w", ctypes.c_void_p), ("row_scale", ctypes.c_void_p), ("w_fwd", ctypes.c_void_p), ("w_dgrad", ctypes.c_void_p),
                ("N", ctypes.c_int32), ("taps", ctypes.c_int32), ("C", ctypes.c_int32), ("block0", ctypes.c_int32),
                ("Np", ctypes.c_int32), ("Cg", ctypes.c_int32), ("Cgp", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class UnpadJob(ctypes.Structure):
    """gwd_unpad_job (include/gwdepth.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("N", ctypes.c_int32), ("taps", ctypes.c_int32), ("G", ctypes.c_int32),
                ("Cg", ctypes.c_int32), ("Cgp", ctypes.c_int32), ("block0", ctypes.c_int32)]


UNPAD_BATCH = 24
STEM_PACKED_ELEMS = 14 * 2 * 64 * 8


def stem_out(n):
    """Output size of conv 7/2/3 followed by max-pool 3/2/1 along one axis."""
    return ((n - 1) // 2 + 1 - 1) // 2 + 1


class ColsumJob(ctypes.Structure):
    """gwd_colsum_job (include/gwdepth.h)."""
    _fields_ = [("g", ctypes.c_void_p), ("out", ctypes.c_void_p), ("rows", ctypes.c_int64), ("C", ctypes.c_int32),
                ("block0", ctypes.c_int32), ("blocks", ctypes.c_int32)]


COLSUM_BATCH = 16
LSAP_MAX_TARGETS = 1024   # gwd_lsap: targets per image and queries (MAXN in csrc/lsap.hip)
COLLATE_BATCH = 16


class ImageJob(ctypes.Structure):
    """gwd_image_job (include/gwdepth.h)."""
    _fields_ = [("rgb", ctypes.c_void_p), ("depth_mm", ctypes.c_void_p), ("labels", ctypes.c_void_p),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


class WidenJob(ctypes.Structure):
    """gwd_widen_job (include/gwdepth.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n", ctypes.c_int64)]


class FrameEvalJob(ctypes.Structure):
    """gwd_frame_eval_job (include/gwdepth.h)."""
    _fields_ = [("gt_depth_mm", ctypes.c_void_p), ("gt_label", ctypes.c_void_p), ("fh", ctypes.c_int32), ("fw", ctypes.c_int32)]


EVAL_FRAMES_BATCH = 16    # gwd_eval_frames: frames per call
EVAL_FRAMES_MAX_BINS = 8
EVAL_FRAMES_WS_BYTES = 128 + 16 * 256 * 32 + 16 * 5 * 256 * 160      # GWD_EVAL_FRAMES_WS_BYTES; the first 128 bytes start as zeros
HEALTH_CHUNK = 16384      # GWD_HEALTH_CHUNK: elements per piece of gwd_segment_stats
HEALTH_RECORD_BYTES, HEALTH_CTL_BYTES, HEALTH_RING_BYTES = 16, 64, 32      # gwd_segment_record / gwd_health_chunk, gwd_health_ctl, gwd_health_record
EMA_PASS = 1024 * 256 * 2 * 4        # GWD_EMA_PASS: elements per grid-stride pass of gwd_adamw_step_ema / gwd_ema_swap
WIDEN_BATCH = 16          # gwd_widen_u16_batch jobs: the depth planes of one batch
AUGMENT_BATCH = 16        # frames per grouped augmentation launch
REGION_MAX = 32           # GWD_REGION_MAX: kept regions per image, at most
REGION_RECORD = 12        # GWD_REGION_RECORD: int64 fields of a region's record
REGION_CANDIDATES = 8192  # GWD_REGION_CANDIDATES: default length of the candidate list per image
FUSION_MAX_RING = 32      # GWD_FUSION_MAX_RING: widest ring around a region, pixels
FUSION_PLANE = 12         # GWD_FUSION_PLANE: fp64 fields of a fusion plane
FUSED_SENSOR, FUSED_PLANE, FUSED_NETWORK = 1, 2, 3        # GWD_FUSED_*: fused_source
PROFILE_MAX_LINES = 2048      # GWD_PROFILE_MAX_LINES: rows per image of gwd_line_profiles
PROFILE_MAX_SAMPLES = 2048    # GWD_PROFILE_MAX_SAMPLES: samples per line, at most
PROFILE_COUNTS = 12           # GWD_PROFILE_COUNTS: int32 fields of a line's counts
RENDER_MAX_PANELS, RENDER_MAX_PLANES, RENDER_MAX_TABLES = 8, 4, 16      # GWD_RENDER_MAX_*: panels, planes of a kind, colour tables per call
RENDER_MAX_WIDTH8, RENDER_MAX_END_RADIUS = 128, 64    # GWD_RENDER_MAX_WIDTH8 (1/16 pixel), GWD_RENDER_MAX_END_RADIUS (pixels)
CLOUD_TILE = 1024         # GWD_CLOUD_TILE: candidates of one frame per workgroup of gwd_point_cloud
CLOUD_RECORD = 32         # GWD_CLOUD_RECORD: bytes of a point
CLOUD_MAX_STRIDE = 16     # GWD_CLOUD_MAX_STRIDE
CLOUD_KEEP = {"all": 0, "glass": 1, "non_glass": 2}       # GWD_CLOUD_KEEP_*
SCENE_TILE = 1024         # GWD_SCENE_TILE: rows (integrate) or ranks (extract) per workgroup
SCENE_VOXEL_BYTES = 128   # GWD_SCENE_VOXEL_BYTES: the accumulators of one voxel
SCENE_MAX_VOXELS = 1 << 27    # GWD_SCENE_MAX_VOXELS
SCENE_FLAG_MERGED = 16    # GWD_SCENE_FLAG_MERGED
SCENE_STATE = ("serial", "count", "points", "dropped", "status")      # the first five int64 of gwd_scene_desc.state
VIEW_TILE = 1024          # GWD_VIEW_TILE: rows of the cloud per workgroup of gwd_cloud_view's splat launch
VIEW_MAX_SPLAT = 64       # GWD_VIEW_MAX_SPLAT: the widest square a row is drawn as, pixels
VIEW_MAX_VIEWS = 16       # cameras per call of gwd_cloud_view
GATHER_BATCH = 48         # gwd_gather2d_batch jobs: RGB, depth and labels of AUGMENT_BATCH frames
COLOR_ADJUST, COLOR_SUMS = 0, 1


class RenderSlot(ctypes.Structure):
    """gwd_render_slot (include/gwdepth.h): one operand, frame by frame."""
    _fields_ = [("ptr", ctypes.c_void_p * 16), ("pitch", ctypes.c_int32 * 16)]


class RenderPanel(ctypes.Structure):
    """gwd_render_panel (include/gwdepth.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("base", "plane", "table", "lo_mm", "hi_mm", "tint", "tint_alpha", "outlines", "region_table",
                                              "lines", "line_table", "ends")] + \
               [(n, ctypes.c_uint8 * 4) for n in ("void_rgb", "tint_rgb", "line_rgb", "end_rgb")]


class RenderDesc(ctypes.Structure):
    """gwd_render_desc (include/gwdepth.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("canvas", "sizes", "tables", "lines", "count", "order", "scores", "kinds")] + \
               [(n, ctypes.c_double) for n in ("min_score", "score_lo", "score_k")] + \
               [(n, ctypes.c_int32) for n in ("B", "P", "Fh", "Fw", "C", "n_planes", "n_label_planes", "n_tables", "lines_dtype",
                                              "scores_dtype", "width8", "end_radius", "has_frames", "has_region_map")] + \
               [("ext_h", ctypes.c_int32 * 16), ("ext_w", ctypes.c_int32 * 16), ("frames", RenderSlot), ("region_map", RenderSlot),
                ("planes", RenderSlot * 4), ("label_planes", RenderSlot * 4), ("panels", RenderPanel * 8)]


class CloudDesc(ctypes.Structure):
    """gwd_cloud_desc (include/gwdepth.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("depth", "labels", "sizes", "intrinsics", "region_map", "region_count", "planes", "source",
                                               "poses", "workspace", "cloud", "cloud_offsets")] + \
               [(n, ctypes.c_double) for n in ("min_depth", "max_depth", "edge")] + [("capacity", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("B", "Fh", "Fw", "max_regions", "stride", "normals", "keep", "has_frames")] + \
               [("ext_h", ctypes.c_int32 * 16), ("ext_w", ctypes.c_int32 * 16), ("frames", RenderSlot)]


class SceneDesc(ctypes.Structure):
    """gwd_scene_desc (include/gwdepth.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("keys", "marks", "ranks", "voxels", "state")] + \
               [("voxel", ctypes.c_double), ("origin", ctypes.c_double * 3), ("max_voxels", ctypes.c_int64), ("slots", ctypes.c_int64)]


class ViewDesc(ctypes.Structure):
    """gwd_view_desc (include/gwdepth.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("cloud", "cloud_offsets", "sizes", "intrinsics", "poses", "workspace", "view_depth",
                                               "view_index", "view_labels", "view_rgb")] + \
               [(n, ctypes.c_double) for n in ("min_depth", "max_depth", "footprint")] + [("rows", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("n_offsets", "V", "Fh", "Fw", "max_splat", "keep")] + \
               [("ext_h", ctypes.c_int32 * 16), ("ext_w", ctypes.c_int32 * 16)]


class ResampleJob(ctypes.Structure):
    """gwd_resample_job (include/gwdepth.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("src_row_stride", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("bounds_off", "kk_off", "ksize", "n_out", "other", "base0", "step0", "base1", "step1",
                                              "block0", "blocks")]


class GatherJob(ctypes.Structure):
    """gwd_gather_job (include/gwdepth.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("src_row_stride_bytes", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("ytab_off", "xtab_off", "oh", "ow", "elem_bytes", "block0", "blocks")]


class ColorJob(ctypes.Structure):
    """gwd_color_job (include/gwdepth.h)."""
    _fields_ = [("rgb", ctypes.c_void_p), ("npix", ctypes.c_int64), ("mode", ctypes.c_int32), ("factor", ctypes.c_float),
                ("block0", ctypes.c_int32), ("blocks", ctypes.c_int32)]


class Strided(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("ws", ctypes.c_int64), ("ts", ctypes.c_int64), ("hs", ctypes.c_int64)]


def _strided(t):
    """(windows, tokens, heads, head_dim) tensor or view with unit channel stride."""
    if t.dim() != 4 or t.stride(3) != 1:
        raise ValueError("window-attention operand must be (W, N, heads, hd) with unit last stride")
    return Strided(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


_ZERO_PAGES = {}


def _zero_page(device):
    """256 zero bytes per device: the LDS-DMA convolution pipeline fetches out-of-image taps from here."""
    if device.type != "cuda":
        return None
    z = _ZERO_PAGES.get(device)
    if z is None:
        z = _ZERO_PAGES[device] = torch.zeros(256, dtype=torch.uint8, device=device)
    return ctypes.c_void_p(z.data_ptr())


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError("gw_depth_amd kernels take float32 or bfloat16, got %s" % t.dtype)


def _ptr_pitched(t):
    """Address of an operand whose pixel pitch the entry point takes separately (a channel slice of a pixel-major map)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ptr(t):
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("kernel operand must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


class HipLibrary:
    """Thin typed wrapper: tensors in, raw pointers + sizes + current stream out."""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise HipUnavailable(
                "libgwdepth_hip.so not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        self.lib = ctypes.CDLL(path)
        for name in ENTRY_POINTS:
            if not hasattr(self.lib, name):
                raise HipUnavailable("libgwdepth_hip.so lacks symbol " + name)
        self.lib.gwd_arch.restype = ctypes.c_char_p
        for name in ENTRY_POINTS[2:]:
            getattr(self.lib, name).restype = ctypes.c_int
        L = self.lib
        vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        L.gwd_conv_forward.argtypes = [ctypes.POINTER(ConvDesc), vp]
        L.gwd_conv_wgrad.argtypes = [ctypes.POINTER(ConvDesc), vp, vp]
        L.gwd_weight_prep.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
        L.gwd_act_backward.argtypes = [vp, vp, vp, vp, i64, i32, i32, f32, i32, vp]
        L.gwd_colsum.argtypes = [vp, vp, i64, i32, i32, vp]
        L.gwd_conv_wgrad_batch.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(ctypes.c_void_p), i32, vp]
        L.gwd_conv_wgrad_takes_bias.argtypes = [ctypes.POINTER(ConvDesc), i32]
        L.gwd_plane_loss_forward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp]
        L.gwd_plane_loss_backward.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp]
        L.gwd_collate.argtypes = [ctypes.POINTER(ImageJob), i32, i32, i32, ctypes.POINTER(ctypes.c_float),
                                  ctypes.POINTER(ctypes.c_float), vp, vp, vp, vp, i32, vp]
        L.gwd_mha_flash_forward.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, vp, i64, vp, i32, i32, i32, i32, f32, i32, vp]
        L.gwd_mha_flash_backward.argtypes = [vp] * 5 + [i64] * 5 + [vp] * 7 + [i64] * 3 + [i32, i32, i32, i32, f32, i32, vp]
        L.gwd_anchor_depth_forward.argtypes = [vp, vp, vp, i32, i64, i32, i32, vp]
        L.gwd_anchor_depth_backward.argtypes = [vp, vp, vp, vp, vp, i32, i64, i32, i32, vp]
        L.gwd_colsum_batch.argtypes = [ctypes.POINTER(ColsumJob), i32, i32, vp]
        L.gwd_layernorm_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp]
        L.gwd_layernorm_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, i32, vp]
        L.gwd_unpad_add_batch.argtypes = [ctypes.POINTER(UnpadJob), i32, vp]
        L.gwd_silog_finalize.argtypes = [vp, f32, f32, vp, vp]
        L.gwd_resample_u8_pass.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, i32, i32, i32, i32, vp]
        L.gwd_gather2d.argtypes = [vp, vp, vp, vp, i32, i32, i64, i32, vp]
        L.gwd_resample_u8_pass_batch.argtypes = [ctypes.POINTER(ResampleJob), i32, i32, i32, vp, i64, vp]
        L.gwd_gather2d_batch.argtypes = [ctypes.POINTER(GatherJob), i32, vp, i64, vp]
        L.gwd_color_adjust_batch.argtypes = [ctypes.POINTER(ColorJob), i32, vp, i32, vp]
        L.gwd_match_cost.argtypes = [vp] * 5 + [i32] * 6 + [f32, f32, vp]
        L.gwd_set_losses_forward.argtypes = [vp] * 9 + [f32] + [vp] * 4 + [i32] * 6 + [vp]
        L.gwd_set_losses_backward.argtypes = [vp] * 8 + [f32] + [vp] * 6 + [i32] * 6 + [vp]
        L.gwd_set_losses_focal_forward.argtypes = [vp] * 9 + [f32] * 2 + [vp] * 4 + [i32] * 6 + [vp]
        L.gwd_set_losses_focal_backward.argtypes = [vp] * 8 + [f32] * 2 + [vp] * 6 + [i32] * 6 + [vp]
        L.gwd_color_adjust.argtypes = [vp, vp, vp, i64, i32, f32, vp]
        L.gwd_bmm.argtypes = [ctypes.POINTER(BmmDesc), vp]
        L.gwd_stride_place.argtypes = [vp, vp, vp] + [i32] * 8 + [vp]
        L.gwd_psp_pool_forward.argtypes = [vp] * 5 + [i32] * 5 + [vp]
        L.gwd_psp_pool_backward.argtypes = [vp] * 6 + [i32] * 6 + [vp]
        L.gwd_pos_sine.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_stem_pack.argtypes = [vp, vp, vp, vp]
        L.gwd_stem_forward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
        L.gwd_softmax_forward.argtypes = [vp, vp, i64, i32, i32, vp]
        L.gwd_softmax_backward.argtypes = [vp, vp, vp, i64, i32, i32, vp]
        L.gwd_silog_sums.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_silog_backward.argtypes = [vp, vp, vp, vp, f32, f32, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_seg_ce_sum.argtypes = [vp, vp, vp, i64, i32, vp]
        L.gwd_seg_ce_backward.argtypes = [vp, vp, vp, f32, vp, i64, i32, vp]
        L.gwd_resample_forward.argtypes = [vp, vp] + [i32] * 9 + [vp]
        L.gwd_resample_backward.argtypes = [vp, vp] + [i32] * 7 + [vp, i32, i32, vp]
        L.gwd_avgpool_forward.argtypes = [vp, vp] + [i32] * 6 + [vp]
        L.gwd_avgpool_backward.argtypes = [vp, vp] + [i32] * 6 + [vp]
        sp = ctypes.POINTER(Strided)
        L.gwd_winattn_forward.argtypes = [sp, sp, sp, sp, vp, vp, i32, vp, i64, i32, i32, i32, f32, i32, vp]
        L.gwd_winattn_backward.argtypes = [sp] * 7 + [vp, vp, vp, i32, vp, i64, i32, i32, i32, f32, i32, i32, vp]
        L.gwd_ref_scores_forward.argtypes = [sp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp]
        L.gwd_ref_scores_backward.argtypes = [sp, vp, vp, sp, vp, i32, i32, i32, i32, i32, f32, i32, vp]
        L.gwd_ref_mix_forward.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_ref_mix_backward.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_tokattn_forward.argtypes = [sp] * 4 + [i64, i32, i32, f32, i32, vp]
        L.gwd_tokattn_backward.argtypes = [sp] * 7 + [i64, i32, i32, f32, i32, vp]
        L.gwd_upsample_taps_collapse.argtypes = [vp, vp, i32, i32, i32, vp]
        L.gwd_upsample_taps_fold.argtypes = [vp, vp, i32, i32, vp]
        L.gwd_tokattn_pair_forward.argtypes = [sp] * 6 + [i64, i32, i32, f32, i32, vp]
        L.gwd_tokattn_pair_backward.argtypes = [sp] * 10 + [i64, i32, i32, f32, i32, vp]
        L.gwd_certain_sample.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp]
        L.gwd_lsap.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
        L.gwd_inorm_gelu_forward.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, ctypes.c_float, i32, vp]
        L.gwd_inorm_gelu_backward.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp]
        L.gwd_query_workspace.argtypes = [i32, ctypes.POINTER(ctypes.c_int64), i32]
        L.gwd_query_workspace.restype = ctypes.c_int64
        L.gwd_eval_accumulate.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, i32, i64, f32, f32, i32, i32, vp]
        L.gwd_dense_postprocess.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, i32, vp]
        L.gwd_dense_postprocess_resized.argtypes = [vp, vp, i64, i64, i64, vp, vp, i32, vp, vp, vp] + [i32] * 5 + [f32, f32, i32, i32, vp]
        L.gwd_line_postprocess.argtypes = [vp] * 7 + [i32, i32, i32, f32, vp]
        dp = ctypes.POINTER(ctypes.c_double)
        L.gwd_line_score.argtypes = [vp] * 5 + [dp, i32, dp, i32] + [vp] * 4 + [i32] * 4 + [i64, i64, vp]
        L.gwd_softmax_masked_forward.argtypes = [vp, vp, vp, i64, i32, i64, ctypes.c_float, i32, vp]
        L.gwd_softmax_scaled_backward.argtypes = [vp, vp, vp, i64, i32, ctypes.c_float, i32, vp]
        L.gwd_resample_backward_sep.argtypes = [vp, vp, vp] + [i32] * 9 + [vp]
        L.gwd_act_backward_colsum.argtypes = [vp, vp, vp, vp, i64, i32, i32, ctypes.c_float, vp, i32, vp]
        L.gwd_point_sample_forward.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_point_sample_backward.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_point_sample_backward_gather.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_point_sample_framed_forward.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_point_sample_framed_backward.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_weight_prep_batch.argtypes = [vp, i32, i32, vp, vp]
        L.gwd_window_map.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_window_map_multi.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        L.gwd_sqnorm.argtypes = [vp, vp, i64, vp]
        L.gwd_adamw_step.argtypes = [vp, vp, vp, vp, vp, vp, i64] + [f32] * 9 + [vp]
        pvp, pi32 = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32)
        L.gwd_pyr_tail_forward.argtypes = [vp, pvp, pi32, pi32, i32] + [vp] * 6 + [i32] * 6 + [vp]
        L.gwd_pyr_tail_backward.argtypes = [vp, pvp, pi32, pi32, i32] + [i32] * 5 + [vp]
        L.gwd_pyr_tail_fold_wgrad.argtypes = [vp, pvp, i32, vp, i32, i32, i32, vp]
        L.gwd_widen_u16_batch.argtypes = [ctypes.POINTER(WidenJob), i32, vp]
        L.gwd_line_nms.argtypes = [vp] * 4 + [ctypes.c_double, f32] + [vp] * 4 + [i32] * 4 + [vp]
        L.gwd_eval_frames.argtypes = [ctypes.POINTER(FrameEvalJob), i32, vp, vp, i32, i32, i32, f32, f32, ctypes.POINTER(f32), i32,
                                      vp, i64, vp, vp, vp, vp, vp, vp]
        L.gwd_segment_stats.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp]
        L.gwd_health_decide.argtypes = [vp, i32, vp, vp, vp, i32, vp, ctypes.c_double, ctypes.c_double, f32, f32, vp]
        L.gwd_adamw_step_guarded.argtypes = [vp, vp, vp, vp, vp, vp, i64] + [f32] * 7 + [vp]
        L.gwd_adamw_step_ema.argtypes = [vp] * 8 + [i64] + [f32] * 9 + [ctypes.c_double, i32, i64, vp]
        L.gwd_ema_swap.argtypes = [vp, vp, vp, i64, vp]
        L.gwd_glass_regions.argtypes = [vp] * 3 + [i32] * 9 + [vp] * 6
        L.gwd_region_planes.argtypes = [vp] * 5 + [i32] * 6 + [vp] * 3
        L.gwd_depth_planar.argtypes = [vp] * 6 + [i32] * 4 + [f32, f32] + [vp] * 3
        L.gwd_line_profiles.argtypes = [vp, i32] + [vp] * 7 + [i32] * 4 + [ctypes.c_double] + [i32] * 5 + [vp] * 5
        L.gwd_fusion_ring.argtypes = [vp] * 6 + [i32] * 10 + [vp] * 4
        L.gwd_fusion_planes.argtypes = [vp] * 5 + [i32] * 7 + [ctypes.c_double, i32, ctypes.c_double] + [vp] * 3
        L.gwd_fusion_depth.argtypes = [vp] * 8 + [i32] * 6 + [f32, f32] + [vp] * 4
        L.gwd_render_frames.argtypes = [ctypes.POINTER(RenderDesc), vp]
        L.gwd_point_cloud.argtypes = [ctypes.POINTER(CloudDesc), vp]
        L.gwd_scene_reset.argtypes = [ctypes.POINTER(SceneDesc), vp]
        L.gwd_scene_integrate.argtypes = [ctypes.POINTER(SceneDesc), vp, vp, i64, i32, vp, vp]
        L.gwd_scene_extract.argtypes = [ctypes.POINTER(SceneDesc), i32, i32, vp, vp, vp, vp, vp]
        L.gwd_cloud_view.argtypes = [ctypes.POINTER(ViewDesc), vp]

    # ------------------------------------------------------------------ plumbing
    @staticmethod
    def _stream(*tensors):
        for t in tensors:
            if t is not None and not t.is_cuda:
                raise HipUnavailable("gw_depth_amd ops run on a HIP device only (got a %s tensor); "
                                     "there is no CPU path" % t.device)
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed with status %d" % (what, rc))

    def workspace_bytes(self, op, *dims):
        """gwd_query_workspace: bytes of caller-provided scratch for op (WS_INORM_GELU / WS_RESAMPLE_BWD)."""
        arr = (ctypes.c_int64 * len(dims))(*[int(d) for d in dims])
        n = self.lib.gwd_query_workspace(op, arr, len(dims))
        if n < 0:
            raise ValueError("gwd_query_workspace(%d, %r) -> %d" % (op, dims, n))
        return n

    def version(self):
        return self.lib.gwd_version()

    # ------------------------------------------------------------------ entry points
    @staticmethod
    def _desc(x, w, y, dims, z=None, scale=None, shift=None, residual=None, stride=1, pad=0,
              gather=GATHER_CONV, virt=(0, 0), act=ACT_NONE, act_scale=1.0, mult=None, gate=None, gate_act=ACT_NONE, ln=None,
              zero_page=True, dbias=None):
        B, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW = dims
        d = ConvDesc()
        d.x, d.w, d.y, d.z = _ptr(x), _ptr(w), _ptr(y), _ptr(z)
        d.scale, d.shift, d.residual = _ptr(scale), _ptr(shift), _ptr(residual)
        d.zero_page = _zero_page(x.device) if zero_page else None      # False: the register-staged kernels (gwd_conv_desc.zero_page = NULL)
        d.mult = _ptr(mult)
        d.gate, d.gate_act = _ptr(gate), (gate_act if gate is not None else ACT_NONE)
        d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout, d.KH, d.KW = B, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW
        d.stride, d.pad, d.gather, d.Hv, d.Wv = stride, pad, gather, virt[0], virt[1]
        d.act, d.act_scale, d.dtype = act, act_scale, dtype_code(x)
        if ln is not None:                              # ConvLn mode: (mean, rstd, real channel count), gwd_conv_desc.ln_*
            d.ln_mean, d.ln_rstd, d.ln_C = _ptr(ln[0]), _ptr(ln[1]), int(ln[2])
        d.dbias = _ptr(dbias)                           # weight gradient only: the bias gradient rides along (gwd_conv_desc.dbias)
        return d

    def conv_forward(self, x, w, y, dims, **kw):
        """dims = (B, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW); kw: z scale shift residual stride pad gather virt act act_scale mult
        gate gate_act (the epilogue's last step: backward of the activation whose output is `gate`); ln=(mean, rstd, C): the ConvLn
        epilogue (LayerNorm over the first C channels, scale / shift = gamma / beta) - returns False when the library has no fused
        kernel for the shape (nothing was launched).  zero_page=False leaves gwd_conv_desc.zero_page NULL: the register-staged
        kernels instead of the LDS-DMA route (the default, True, hands over the device's zero page)."""
        d = self._desc(x, w, y, dims, **kw)
        rc = self.lib.gwd_conv_forward(ctypes.byref(d), self._stream(x, w, y))
        if rc == -4 and kw.get("ln") is not None:
            return False                                # no fused ConvLn kernel for this shape: the caller runs the two kernels
        if rc == -4 and kw.get("gate") is not None and kw.get("gate_act") == ACT_GELU:
            return False                                # no kernel with the GELU gate for this shape: the caller applies it in a pass of its own
        self._check(rc, "gwd_conv_forward")

    def conv_wgrad(self, x, gy, dw, dims, **kw):
        """kw as for conv_forward, plus dbias: fp32 [Cout], the column sums of gy are ACCUMULATED into it by the weight-gradient kernel
        itself - only where conv_wgrad_takes_bias answers True, else the call fails with -4 (nothing launched)."""
        d = self._desc(x, None, gy, dims, **kw)
        self._check(self.lib.gwd_conv_wgrad(ctypes.byref(d), _ptr(dw), self._stream(x, gy, dw, kw.get("dbias"))), "gwd_conv_wgrad")

    def conv_wgrad_takes_bias(self, x, gy, dims, batched, **kw):
        """gwd_conv_wgrad_takes_bias: whether the kernel that conv_wgrad (batched: conv_wgrad_batch) selects for this problem sums the
        bias gradient too.  Host logic only."""
        d = self._desc(x, None, gy, dims, **kw)
        return self.lib.gwd_conv_wgrad_takes_bias(ctypes.byref(d), 1 if batched else 0) == 1

    def conv_wgrad_batch(self, jobs):
        """jobs: tuples (x, gy, dw, dims, kw) as for conv_wgrad; one library call, grouped launches (gwd_conv_wgrad_batch)."""
        descs = (ConvDesc * len(jobs))()
        dws = (ctypes.c_void_p * len(jobs))()
        ts = []
        for i, (x, gy, dw, dims, kw) in enumerate(jobs):
            descs[i] = self._desc(x, None, gy, dims, **kw)
            dws[i] = _ptr(dw)
            ts += [x, gy, dw, kw.get("dbias")]
        self._check(self.lib.gwd_conv_wgrad_batch(descs, dws, len(jobs), self._stream(*ts)), "gwd_conv_wgrad_batch")

    def weight_prep(self, w, row_scale, w_fwd, w_dgrad, N, taps, C, dtype):
        self._check(self.lib.gwd_weight_prep(_ptr(w), _ptr(row_scale), _ptr(w_fwd), _ptr(w_dgrad), N, taps, C, dtype,
                                             self._stream(w, w_fwd, w_dgrad)), "gwd_weight_prep")

    def act_backward(self, gy, ref, gx, scale, rows, C, act, act_scale):
        self._check(self.lib.gwd_act_backward(_ptr(gy), _ptr(ref), _ptr(gx), _ptr(scale), rows, C, act, act_scale,
                                              dtype_code(gy), self._stream(gy, ref, gx)), "gwd_act_backward")

    def act_backward_colsum(self, gy, ref, gx, dbias, rows, C, act, act_scale, mult=None):
        """Fused activation backward + bias gradient (gy first multiplied by `mult` when given); False when the shape is not
        supported (use the separate calls)."""
        rc = self.lib.gwd_act_backward_colsum(_ptr(gy), _ptr(ref), _ptr(gx), _ptr(dbias), rows, C, act, act_scale, _ptr(mult),
                                              dtype_code(gy), self._stream(gy, ref, gx))
        if rc == -4:
            return False
        self._check(rc, "gwd_act_backward_colsum")
        return True

    def colsum(self, g, out, rows, C):
        self._check(self.lib.gwd_colsum(_ptr(g), _ptr(out), rows, C, dtype_code(g), self._stream(g, out)), "gwd_colsum")

    def colsum_batch(self, jobs):
        """jobs: up to COLSUM_BATCH tuples (g, out, rows, C) of ONE dtype with vector-shaped C (colsum_batchable)."""
        recs = (ColsumJob * len(jobs))()
        for r, (g, out, rows, C) in zip(recs, jobs):
            r.g, r.out, r.rows, r.C = g.data_ptr(), out.data_ptr(), rows, C
            if not (g.is_contiguous() and out.is_contiguous()):
                raise ValueError("kernel operand must be contiguous")
        ts = [t for j in jobs for t in j[:2]]
        self._check(self.lib.gwd_colsum_batch(recs, len(jobs), dtype_code(jobs[0][0]), self._stream(*ts)), "gwd_colsum_batch")

    @staticmethod
    def colsum_batchable(g, C):
        vec = 8 if g.dtype == torch.bfloat16 else 4
        return C % vec == 0 and C // vec <= 256

    def layernorm_forward(self, x, gamma, beta, y, mean, rstd, rows, C, gelu, residual=None, ld=0):
        """ld: row pitch in elements (0 = C); channels C..ld-1 are zero padding, written as zeros."""
        self._check(self.lib.gwd_layernorm_forward(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(residual), _ptr(y), _ptr(mean), _ptr(rstd),
                                                   rows, C, ld, int(gelu), dtype_code(x), self._stream(x, y)),
                    "gwd_layernorm_forward")

    def layernorm_backward(self, gy, x, gamma, beta, mean, rstd, gx, dgamma, dbeta, rows, C, gelu, ld=0, gskip=None, elu_input=False):
        """gskip: a second gradient of x, added to gx in the kernel; elu_input: x is an ELU output whose backward is applied to gx
        as well (GWD_LN_ELU_INPUT).  Returns False when that could not be done (no vector kernel for the shape: the call has then
        run WITHOUT both and the caller does them)."""
        flags = int(bool(gelu)) | (2 if elu_input else 0)
        rc = self.lib.gwd_layernorm_backward(_ptr(gy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd), _ptr(gx), _ptr(dgamma),
                                             _ptr(dbeta), rows, C, ld, flags, _ptr(gskip), dtype_code(x), self._stream(gy, x, gx))
        if rc == -4 and (gskip is not None or elu_input):
            self._check(self.lib.gwd_layernorm_backward(_ptr(gy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd), _ptr(gx), _ptr(dgamma),
                                                        _ptr(dbeta), rows, C, ld, int(bool(gelu)), None, dtype_code(x), self._stream(gy, x, gx)),
                        "gwd_layernorm_backward")
            return False
        self._check(rc, "gwd_layernorm_backward")
        return True

    def pos_counts(self, mask_full, mask_level, counts):
        """mask_full (B,H,W) bool/u8 -> mask_level (B,h,w) bool (nearest), counts (B,h,w,2) int16 (gwd_pos_sine, first stage)."""
        B, H, W = mask_full.shape
        _, h, w = mask_level.shape
        if tuple(counts.shape) != (B, h, w, 2) or counts.dtype != torch.int16 or mask_full.element_size() != 1 or mask_level.element_size() != 1:
            raise ValueError("pos_counts: byte masks and int16 counts (B,h,w,2) expected")
        self._check(self.lib.gwd_pos_sine(_ptr(mask_full), _ptr(mask_level), _ptr(counts), None, None, B, H, W, h, w, 0, 0,
                                          self._stream(mask_full, mask_level, counts)), "gwd_pos_sine")

    def pos_emit(self, counts, dim_t, out, normalize):
        """counts (B,h,w,2) int16 + dim_t (F) fp32 -> out (B,h,w,2F) fp32 (gwd_pos_sine, second stage)."""
        B, h, w, _ = counts.shape
        F = dim_t.numel()
        if tuple(out.shape) != (B, h, w, 2 * F) or out.dtype != torch.float32 or dim_t.dtype != torch.float32:
            raise ValueError("pos_emit: out fp32 (B,h,w,2F) expected")
        self._check(self.lib.gwd_pos_sine(None, None, _ptr(counts), _ptr(dim_t), _ptr(out), B, 0, 0, h, w, F, int(bool(normalize)),
                                          self._stream(counts, dim_t, out)), "gwd_pos_sine")

    def stem_pack(self, w, scale, packed):
        """w fp32 (64,7,7,3) [* scale (64)] -> packed bf16 (STEM_PACKED_ELEMS,) in gwd_stem_forward's operand order."""
        if tuple(w.shape) != (64, 7, 7, 3) or w.dtype != torch.float32 or packed.numel() != STEM_PACKED_ELEMS or packed.dtype != torch.bfloat16:
            raise ValueError("stem_pack: w fp32 (64,7,7,3) and a bf16 buffer of %d values expected" % STEM_PACKED_ELEMS)
        self._check(self.lib.gwd_stem_pack(_ptr(w), _ptr(scale), _ptr(packed), self._stream(w, packed)), "gwd_stem_pack")

    def stem_forward(self, x, packed, shift, y):
        """conv 7x7 s2 p3 (3 -> 64) + shift + ReLU + max-pool 3x3 s2 p1: x bf16 (B,H,W,3) -> y bf16 (B,Hp,Wp,64)."""
        B, H, W, C = x.shape
        Hp, Wp = stem_out(H), stem_out(W)
        if C != 3 or tuple(y.shape) != (B, Hp, Wp, 64) or not x.is_contiguous() or not y.is_contiguous():
            raise ValueError("stem_forward: x (B,H,W,3) and y (B,%d,%d,64) contiguous expected" % (Hp, Wp))
        self._check(self.lib.gwd_stem_forward(_ptr(x), _ptr(packed), _ptr(shift), _ptr(y), B, H, W, dtype_code(x), self._stream(x, packed, y)),
                    "gwd_stem_forward")

    def unpad_add_batch(self, jobs):
        """jobs: tuples (src, dst, N, taps, G, Cg, Cgp): dst (N, taps, G*Cg) += src (.., taps, G*Cgp), fp32; one launch per
        UNPAD_BATCH jobs (gwd_unpad_add_batch)."""
        for i0 in range(0, len(jobs), UNPAD_BATCH):
            part = jobs[i0:i0 + UNPAD_BATCH]
            recs = (UnpadJob * len(part))()
            ts = []
            for i, (src, dst, N, taps, G, Cg, Cgp) in enumerate(part):
                if src.dtype != torch.float32 or dst.dtype != torch.float32 or not src.is_contiguous() or not dst.is_contiguous():
                    raise ValueError("unpad_add_batch: contiguous fp32 tensors expected")
                if dst.numel() != N * taps * G * Cg or src.numel() < N * taps * G * Cgp:
                    raise ValueError("unpad_add_batch: shapes do not match the job")
                r = recs[i]
                r.src, r.dst, r.N, r.taps, r.G, r.Cg, r.Cgp, r.block0 = src.data_ptr(), dst.data_ptr(), N, taps, G, Cg, Cgp, 0
                ts += [src, dst]
            self._check(self.lib.gwd_unpad_add_batch(recs, len(part), self._stream(*ts)), "gwd_unpad_add_batch")

    def softmax_forward(self, x, y, rows, L):
        self._check(self.lib.gwd_softmax_forward(_ptr(x), _ptr(y), rows, L, dtype_code(x), self._stream(x, y)),
                    "gwd_softmax_forward")

    def softmax_masked_forward(self, x, key_mask, y, rows, L, rows_per_mask, scale):
        self._check(self.lib.gwd_softmax_masked_forward(_ptr(x), _ptr(key_mask), _ptr(y), rows, L, rows_per_mask, scale,
                                                        dtype_code(x), self._stream(x, y)), "gwd_softmax_masked_forward")

    def softmax_scaled_backward(self, gy, y, gx, rows, L, scale):
        self._check(self.lib.gwd_softmax_scaled_backward(_ptr(gy), _ptr(y), _ptr(gx), rows, L, scale, dtype_code(y),
                                                         self._stream(gy, y, gx)), "gwd_softmax_scaled_backward")

    def softmax_backward(self, gy, y, gx, rows, L):
        self._check(self.lib.gwd_softmax_backward(_ptr(gy), _ptr(y), _ptr(gx), rows, L, dtype_code(y),
                                                  self._stream(gy, y, gx)), "gwd_softmax_backward")

    def eval_accumulate(self, pred, gt, seg, seg_strides, seg_gt, workspace, measures, running, confusion, B, HW, dmin, dmax):
        """gwd_eval_accumulate.  seg may be a strided view: seg_strides = (image, pixel, class) element strides."""
        sb, sp, sc = (int(v) for v in seg_strides) if seg is not None else (0, 0, 0)
        self._check(self.lib.gwd_eval_accumulate(
            _ptr(pred), _ptr(gt), None if seg is None else ctypes.c_void_p(seg.data_ptr()), sb, sp, sc, _ptr(seg_gt),
            _ptr(workspace), _ptr(measures), _ptr(running), _ptr(confusion), B, HW, float(dmin), float(dmax),
            dtype_code(pred) if pred is not None else F32, dtype_code(seg) if seg is not None else F32,
            self._stream(pred, gt, seg, seg_gt, workspace, measures, running, confusion)), "gwd_eval_accumulate")

    def dense_postprocess(self, depth, seg, seg_strides, sizes, depth_out, depth_mm, label, B, H, W, dmin, dmax):
        """gwd_dense_postprocess.  seg may be a strided view: seg_strides = (image, pixel, class) element strides; sizes (B,2)
        int32 or None; depth_mm uint16 or None."""
        for t, dt in ((sizes, torch.int32), (depth_out, torch.float32), (depth_mm, torch.uint16), (label, torch.uint8)):
            if t is not None and t.dtype != dt:
                raise TypeError("gwd_dense_postprocess: expected %s, got %s" % (dt, t.dtype))
        n = B * H * W
        if depth.numel() != n or depth_out.numel() != n or label.numel() != n or (depth_mm is not None and depth_mm.numel() != n) \
                or (sizes is not None and sizes.numel() != 2 * B):
            raise ValueError("gwd_dense_postprocess: operand sizes do not match (B, H, W) = (%d, %d, %d)" % (B, H, W))
        sb, sp, sc = (int(v) for v in seg_strides)
        self._check(self.lib.gwd_dense_postprocess(
            _ptr(depth), ctypes.c_void_p(seg.data_ptr()), sb, sp, sc, _ptr(sizes), _ptr(depth_out), _ptr(depth_mm), _ptr(label),
            B, H, W, float(dmin), float(dmax), dtype_code(depth), dtype_code(seg),
            self._stream(depth, seg, sizes, depth_out, depth_mm, label)), "gwd_dense_postprocess")

    def dense_postprocess_resized(self, depth, seg, seg_strides, sizes, frame_sizes, twin, depth_out, depth_mm, label, B, H, W, Fh, Fw,
                                  dmin, dmax):
        """gwd_dense_postprocess_resized.  depth / seg hold B + twin images of (H, W); sizes (B,2) int32 or None, frame_sizes (B,2)
        int32, both on the device; the outputs are (B, Fh, Fw)."""
        for t, dt in ((sizes, torch.int32), (frame_sizes, torch.int32), (depth_out, torch.float32), (depth_mm, torch.uint16),
                      (label, torch.uint8)):
            if t is not None and t.dtype != dt:
                raise TypeError("gwd_dense_postprocess_resized: expected %s, got %s" % (dt, t.dtype))
        n = B * Fh * Fw
        if twin < 0 or depth.numel() != (B + twin) * H * W or depth_out.numel() != n or label.numel() != n \
                or (depth_mm is not None and depth_mm.numel() != n) or (sizes is not None and sizes.numel() != 2 * B) \
                or frame_sizes.numel() != 2 * B:
            raise ValueError("gwd_dense_postprocess_resized: operand sizes do not match (B, twin, H, W, Fh, Fw) = (%d, %d, %d, %d, %d, %d)"
                             % (B, twin, H, W, Fh, Fw))
        sb, sp, sc = (int(v) for v in seg_strides)
        self._check(self.lib.gwd_dense_postprocess_resized(
            _ptr(depth), ctypes.c_void_p(seg.data_ptr()), sb, sp, sc, _ptr(sizes), _ptr(frame_sizes), int(twin), _ptr(depth_out),
            _ptr(depth_mm), _ptr(label), B, H, W, Fh, Fw, float(dmin), float(dmax), dtype_code(depth), dtype_code(seg),
            self._stream(depth, seg, sizes, frame_sizes, depth_out, depth_mm, label)), "gwd_dense_postprocess_resized")

    def line_postprocess(self, logits, lines, sizes, scores, lines_px, order, count, B, Q, ld, thresh):
        """gwd_line_postprocess: logits (B,Q,2) / lines (B,Q,ld) fp32, sizes (B,2) int32; Q <= 1024."""
        for t, dt in ((logits, torch.float32), (lines, torch.float32), (sizes, torch.int32), (scores, torch.float32),
                      (lines_px, torch.float32), (order, torch.int32), (count, torch.int32)):
            if t.dtype != dt:
                raise TypeError("gwd_line_postprocess: expected %s, got %s" % (dt, t.dtype))
        if logits.numel() != B * Q * 2 or lines.numel() != B * Q * ld or sizes.numel() != 2 * B or scores.numel() != B * Q \
                or lines_px.numel() != B * Q * 4 or order.numel() != B * Q or count.numel() != B:
            raise ValueError("gwd_line_postprocess: operand sizes do not match (B, Q, ld) = (%d, %d, %d)" % (B, Q, ld))
        self._check(self.lib.gwd_line_postprocess(
            _ptr(logits), _ptr(lines), _ptr(sizes), _ptr(scores), _ptr(lines_px), _ptr(order), _ptr(count), B, Q, ld, float(thresh),
            self._stream(logits, lines, sizes, scores, lines_px, order, count)), "gwd_line_postprocess")

    def line_score(self, logits, lines, sizes, gt, gt_count, nms_thresholds, sap_thresholds, flag, kept_lines, score, gt_seen, slot):
        """gwd_line_score: logits (B,Q,2) / lines (B,Q,ld) / gt (B,G,4) fp32, sizes (B,2) / gt_count (B,) int32; the outputs are the
        accumulator's whole buffers flag (T,S,cap,Q) uint8, kept_lines (T,cap,Q,4) f64, score (cap,Q) fp32, gt_seen (cap,) int32, of
        which images slot .. slot + B - 1 are written.  Q, G <= 1024; at most four thresholds of either kind."""
        for t, dt in ((logits, torch.float32), (lines, torch.float32), (sizes, torch.int32), (gt, torch.float32), (gt_count, torch.int32),
                      (flag, torch.uint8), (kept_lines, torch.float64), (score, torch.float32), (gt_seen, torch.int32)):
            if t.dtype != dt:
                raise TypeError("gwd_line_score: expected %s, got %s" % (dt, t.dtype))
        B, Q, ld = lines.shape
        G, T, S, cap = gt.shape[1], len(nms_thresholds), len(sap_thresholds), score.shape[0]
        if tuple(logits.shape) != (B, Q, 2) or tuple(sizes.shape) != (B, 2) or tuple(gt.shape) != (B, G, 4) or gt_count.numel() != B \
                or tuple(flag.shape) != (T, S, cap, Q) or tuple(kept_lines.shape) != (T, cap, Q, 4) or tuple(score.shape) != (cap, Q) \
                or gt_seen.numel() != cap or slot < 0 or slot + B > cap:
            raise ValueError("gwd_line_score: operand sizes do not match (B, Q, G, T, S, capacity, slot) = %r" % ((B, Q, G, T, S, cap, slot),))
        nms = (ctypes.c_double * T)(*[float(v) for v in nms_thresholds])
        sap = (ctypes.c_double * S)(*[float(v) for v in sap_thresholds])
        self._check(self.lib.gwd_line_score(
            _ptr(logits), _ptr(lines), _ptr(sizes), _ptr(gt), _ptr(gt_count), nms, T, sap, S, _ptr(flag), _ptr(kept_lines), _ptr(score),
            _ptr(gt_seen), B, Q, ld, G, cap, int(slot),
            self._stream(logits, lines, sizes, gt, gt_count, flag, kept_lines, score, gt_seen)), "gwd_line_score")

    def line_nms(self, logits, lines, sizes, order, threshold, min_score, nms_lines, nms_scores, nms_ids, nms_count, twin):
        """gwd_line_nms: logits (B+twin,Q,2) / lines (B+twin,Q,ld) fp32, sizes (B,2) int32, order (B+twin,Q) int32 or None; outputs
        nms_lines (B,C,4) f64, nms_scores (B,C) fp32, nms_ids (B,C) / nms_count (B,) int32 with C = Q, or 2 Q with twin = B.
        min_score None = no floor.  At most 1024 candidates per image."""
        for t, dt in ((logits, torch.float32), (lines, torch.float32), (sizes, torch.int32), (order, torch.int32),
                      (nms_lines, torch.float64), (nms_scores, torch.float32), (nms_ids, torch.int32), (nms_count, torch.int32)):
            if t is not None and t.dtype != dt:
                raise TypeError("gwd_line_nms: expected %s, got %s" % (dt, t.dtype))
        Bs, Q, ld = lines.shape
        twin = int(twin)
        B, C = Bs - twin, Q * (2 if twin else 1)
        if twin < 0 or B <= 0 or (twin and twin != B) or tuple(logits.shape) != (Bs, Q, 2) or tuple(sizes.shape) != (B, 2) \
                or (order is not None and tuple(order.shape) != (Bs, Q)) or tuple(nms_lines.shape) != (B, C, 4) \
                or tuple(nms_scores.shape) != (B, C) or tuple(nms_ids.shape) != (B, C) or nms_count.numel() != B:
            raise ValueError("gwd_line_nms: operand sizes do not match (B, Q, ld, twin) = %r" % ((B, Q, ld, twin),))
        self._check(self.lib.gwd_line_nms(
            _ptr(logits), _ptr(lines), _ptr(sizes), _ptr(order), float(threshold), float("nan") if min_score is None else float(min_score),
            _ptr(nms_lines), _ptr(nms_scores), _ptr(nms_ids), _ptr(nms_count), B, Q, ld, twin,
            self._stream(logits, lines, sizes, order, nms_lines, nms_scores, nms_ids, nms_count)), "gwd_line_nms")

    def plane_loss_forward(self, depth, valid, tri, n_planes, P, H, W, min_area, workspace, stats, loss):
        self._check(self.lib.gwd_plane_loss_forward(_ptr(depth), _ptr(valid), _ptr(tri), _ptr(n_planes), P, H, W, min_area,
                                                    _ptr(workspace), _ptr(stats), _ptr(loss), dtype_code(depth),
                                                    self._stream(depth, valid, tri, n_planes, workspace, stats, loss)), "gwd_plane_loss_forward")

    def plane_loss_backward(self, depth, valid, tri, n_planes, P, H, W, stats, gloss, gdepth):
        self._check(self.lib.gwd_plane_loss_backward(_ptr(depth), _ptr(valid), _ptr(tri), _ptr(n_planes), P, H, W, _ptr(stats),
                                                     _ptr(gloss), _ptr(gdepth), dtype_code(depth),
                                                     self._stream(depth, valid, tri, n_planes, stats, gloss, gdepth)), "gwd_plane_loss_backward")

    def collate(self, samples, H, W, mean, std, images, mask, depth, seg):
        """gwd_collate.  samples: (rgb uint8 (h,w,3), depth_mm int32 (h,w) | None, labels uint8 (h,w) | None) device tensors."""
        jobs = (ImageJob * len(samples))()
        ts = [images, mask, depth, seg]
        for j, (rgb, dmm, lab) in zip(jobs, samples):
            j.rgb, j.depth_mm, j.labels = _ptr(rgb), _ptr(dmm), _ptr(lab)
            j.h, j.w = rgb.shape[0], rgb.shape[1]
            ts += [rgb, dmm, lab]
        f3 = ctypes.c_float * 3
        self._check(self.lib.gwd_collate(jobs, len(samples), H, W, f3(*mean), f3(*std), _ptr(images), _ptr(mask), _ptr(depth),
                                         _ptr(seg), dtype_code(images), self._stream(*ts)), "gwd_collate")

    def widen_u16_batch(self, jobs):
        """gwd_widen_u16_batch.  jobs: up to WIDEN_BATCH pairs (src, dst): src the 2 * n bytes of a little-endian unsigned 16-bit plane
        (a uint8 view of a record, or a 2-byte tensor of n elements), dst a contiguous int32 tensor of n elements."""
        if not 0 < len(jobs) <= WIDEN_BATCH:
            raise ValueError("1..%d planes per call" % WIDEN_BATCH)
        recs = (WidenJob * len(jobs))()
        ts = []
        for r, (src, dst) in zip(recs, jobs):
            if dst.dtype != torch.int32 or src.element_size() not in (1, 2) or src.numel() * src.element_size() != 2 * dst.numel():
                raise ValueError("widen_u16_batch: 2 * n source bytes for an int32 plane of n elements expected")
            if not (src.is_contiguous() and dst.is_contiguous()):
                raise ValueError("kernel operand must be contiguous")
            # an empty view has no data_ptr(): its place in the storage stands in (the entry point skips n == 0 and reads nothing)
            r.src, r.dst = (t.data_ptr() or t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size() for t in (src, dst))
            r.n = dst.numel()
            ts += [src, dst]
        self._check(self.lib.gwd_widen_u16_batch(recs, len(jobs), self._stream(*ts)), "gwd_widen_u16_batch")

    def eval_frames(self, depth, label, gt, dmin, dmax, bin_edges, workspace, offset, sums, measures, conf, running, confusion):
        """gwd_eval_frames.  depth (B,Fh,Fw) fp32 and label (B,Fh,Fw) uint8 as predict_frames returns them; gt: B pairs (depth_mm,
        labels) of contiguous (fh,fw) tensors, depth_mm 2 or 4 bytes wide (all alike), labels uint8; bin_edges: host floats (R - 2
        of them, or none); workspace EVAL_FRAMES_WS_BYTES uint8 whose first 128 bytes started as zeros; sums (N,R,10) / measures
        (N,R,9) f64 and conf (N,4) int64 take the records offset .. offset + B - 1; running (R,10) f64 and confusion (4,) int64
        accumulate.  Returns the library's status for bad arguments (nothing launched) instead of raising: 0 on success."""
        B, Fh, Fw = depth.shape
        R = running.shape[0]
        n_bins = max(len(bin_edges) - 1, 0)
        if depth.dtype != torch.float32 or label.dtype != torch.uint8 or tuple(label.shape) != (B, Fh, Fw) or len(gt) != B:
            raise ValueError("eval_frames: depth (B,Fh,Fw) fp32, label (B,Fh,Fw) uint8 and B ground-truth pairs expected")
        if R != 3 + n_bins or tuple(running.shape) != (R, 10) or sums.shape[1:] != (R, 10) or measures.shape[1:] != (R, 9) \
                or conf.shape[1:] != (4,) or confusion.numel() != 4 or workspace.numel() < EVAL_FRAMES_WS_BYTES:
            raise ValueError("eval_frames: output shapes do not fit %d regions" % (3 + n_bins))
        if not 0 <= offset <= min(sums.shape[0], measures.shape[0], conf.shape[0]) - B:
            raise ValueError("eval_frames: records %d .. %d lie outside the output buffers" % (offset, offset + B - 1))
        for t, dt in ((sums, torch.float64), (measures, torch.float64), (running, torch.float64), (conf, torch.int64), (confusion, torch.int64)):
            if t.dtype != dt:
                raise TypeError("eval_frames: expected %s, got %s" % (dt, t.dtype))
        recs = (FrameEvalJob * max(B, 1))()
        ts = [depth, label, workspace, sums, measures, conf, running, confusion]
        width = gt[0][0].element_size() if B else 4
        for r, (dmm, lab) in zip(recs, gt):
            if dmm.dim() != 2 or lab.shape != dmm.shape or lab.dtype != torch.uint8 or dmm.element_size() != width \
                    or dmm.is_floating_point():
                raise ValueError("eval_frames: ground truth is (depth_mm (fh,fw) of one integer width, labels (fh,fw) uint8) per frame")
            r.gt_depth_mm, r.gt_label, r.fh, r.fw = _ptr(dmm), _ptr(lab), dmm.shape[0], dmm.shape[1]
            ts += [dmm, lab]
        edges = (ctypes.c_float * (n_bins + 1))(*[float(e) for e in bin_edges]) if n_bins else None
        return self.lib.gwd_eval_frames(recs, B, _ptr(depth), _ptr(label), Fh, Fw, width, float(dmin), float(dmax), edges, n_bins,
                                        _ptr(workspace), int(offset), _ptr(sums), _ptr(measures), _ptr(conf), _ptr(running),
                                        _ptr(confusion), self._stream(*ts))

    @staticmethod
    def _tok(t):
        """(B, tokens, E) tensor or last-dim slice: raw pointer + token stride; dense batches, unit channel stride."""
        if t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            raise ValueError("attention operand must be (B, tokens, E) with unit channel stride and dense token rows")
        return ctypes.c_void_p(t.data_ptr()), t.stride(1)

    def mha_flash_forward(self, q, k, v, key_padding_mask, mult, out, lse, H, scale):
        """gwd_mha_flash_forward: q (B,L,32H), k / v (B,S,32H) bf16 tensors or channel slices of a packed projection."""
        B, L, S = q.shape[0], q.shape[1], k.shape[1]
        (qp, qs), (kp, ks), (vp_, vs), (op, os_) = self._tok(q), self._tok(k), self._tok(v), self._tok(out)
        self._check(self.lib.gwd_mha_flash_forward(qp, kp, vp_, qs, ks, vs, _ptr(key_padding_mask), _ptr(mult), op, os_, _ptr(lse),
                                                   B, H, L, S, float(scale), dtype_code(q),
                                                   self._stream(q, k, v, key_padding_mask, mult, out, lse)), "gwd_mha_flash_forward")

    def mha_flash_backward(self, q, k, v, go, out, key_padding_mask, mult, lse, delta, gq, gk, gv, H, scale):
        B, L, S = q.shape[0], q.shape[1], k.shape[1]
        ts = [self._tok(t) for t in (q, k, v, go, out, gq, gk, gv)]
        self._check(self.lib.gwd_mha_flash_backward(ts[0][0], ts[1][0], ts[2][0], ts[3][0], ts[4][0], ts[0][1], ts[1][1], ts[2][1],
                                                    ts[3][1], ts[4][1], _ptr(key_padding_mask), _ptr(mult), _ptr(lse), _ptr(delta),
                                                    ts[5][0], ts[6][0], ts[7][0], ts[5][1], ts[6][1], ts[7][1], B, H, L, S,
                                                    float(scale), dtype_code(q),
                                                    self._stream(q, k, v, go, out, key_padding_mask, mult, lse, delta, gq, gk, gv)),
                    "gwd_mha_flash_backward")

    def anchor_depth_forward(self, att, anchor, pred, B, P, R):
        self._check(self.lib.gwd_anchor_depth_forward(_ptr(att), _ptr(anchor), _ptr(pred), B, P, R, dtype_code(att),
                                                      self._stream(att, anchor, pred)), "gwd_anchor_depth_forward")

    def anchor_depth_backward(self, att, anchor, gpred, datt, danchor, B, P, R):
        self._check(self.lib.gwd_anchor_depth_backward(_ptr(att), _ptr(anchor), _ptr(gpred), _ptr(datt), _ptr(danchor), B, P, R,
                                                       dtype_code(att), self._stream(att, anchor, gpred, datt, danchor)),
                    "gwd_anchor_depth_backward")

    def silog_sums(self, pred, gt, sums, B, h, w, H, W, log_err):
        self._check(self.lib.gwd_silog_sums(_ptr(pred), _ptr(gt), _ptr(sums), B, h, w, H, W, int(log_err),
                                            dtype_code(pred), self._stream(pred, gt, sums)), "gwd_silog_sums")

    def silog_finalize(self, sums, lam, scale, loss):
        self._check(self.lib.gwd_silog_finalize(_ptr(sums), lam, scale, _ptr(loss), self._stream(sums, loss)), "gwd_silog_finalize")

    def silog_backward(self, pred, gt, sums, gloss, weight, lam, gpred, B, h, w, H, W, log_err):
        self._check(self.lib.gwd_silog_backward(_ptr(pred), _ptr(gt), _ptr(sums), _ptr(gloss), weight, lam, _ptr(gpred),
                                                B, h, w, H, W, int(log_err), dtype_code(pred),
                                                self._stream(pred, gt, gpred)), "gwd_silog_backward")

    def seg_ce_sum(self, logits, target, out, P):
        self._check(self.lib.gwd_seg_ce_sum(_ptr(logits), _ptr(target), _ptr(out), P, dtype_code(logits),
                                            self._stream(logits, target, out)), "gwd_seg_ce_sum")

    def seg_ce_backward(self, logits, target, gloss, scale, glogits, P):
        self._check(self.lib.gwd_seg_ce_backward(_ptr(logits), _ptr(target), _ptr(gloss), scale, _ptr(glogits), P,
                                                 dtype_code(logits), self._stream(logits, glogits)), "gwd_seg_ce_backward")

    @staticmethod
    def _pixel_pitch(t, H, W, C):
        """Element pitch between pixels of a (B,H,W,C) tensor that may be a channel slice of a wider pixel-major map."""
        ld = t.stride(2) if t.dim() == 4 and W > 1 else C
        if t.dim() == 4 and (t.stride(3) != 1 or (H > 1 and t.stride(1) != W * ld) or (t.shape[0] > 1 and t.stride(0) != H * W * ld)):
            raise ValueError("pixel-major tensor or a channel slice of one expected, got strides %r" % (t.stride(),))
        return ld

    def resample_forward(self, x, y, B, Hs, Ws, Ho, Wo, C, mode):
        """y may be a channel slice of a wider (B,Ho,Wo,*) map: the result is written in place there."""
        self._check(self.lib.gwd_resample_forward(_ptr(x), _ptr_pitched(y), B, Hs, Ws, Ho, Wo, C, mode, self._pixel_pitch(y, Ho, Wo, C), dtype_code(x),
                                                  self._stream(x, y)), "gwd_resample_forward")

    def resample_backward(self, gy, gx, B, Hs, Ws, Ho, Wo, C, mode, gate=None, gate_act=ACT_NONE):
        """gate / gate_act: gx *= act'(.) of the activation whose output is `gate` (B,Hs,Ws,C); False when the shape cannot (the call
        has then run WITHOUT the gate)."""
        rc = self.lib.gwd_resample_backward(_ptr(gy), _ptr(gx), B, Hs, Ws, Ho, Wo, C, mode, _ptr(gate), gate_act if gate is not None else 0,
                                            dtype_code(gy), self._stream(gy, gx))
        if rc == -4 and gate is not None:
            self._check(self.lib.gwd_resample_backward(_ptr(gy), _ptr(gx), B, Hs, Ws, Ho, Wo, C, mode, None, 0, dtype_code(gy),
                                                       self._stream(gy, gx)), "gwd_resample_backward")
            return False
        self._check(rc, "gwd_resample_backward")
        return True

    def resample_backward_sep(self, gy, tmp, gx, B, Hs, Ws, Ho, Wo, C, mode):
        """Separable backward through the fp32 scratch `tmp` (B,Ho,Ws,C); False when C is not vector-sized."""
        rc = self.lib.gwd_resample_backward_sep(_ptr_pitched(gy), _ptr(tmp), _ptr(gx), B, Hs, Ws, Ho, Wo, C, mode, self._pixel_pitch(gy, Ho, Wo, C),
                                                dtype_code(gy), self._stream(gy, gx))
        if rc == -4:
            return False
        self._check(rc, "gwd_resample_backward_sep")
        return True

    def stride_place(self, src, residual, dst, stride):
        """dst (B,H,W,C) = [residual +] src (B,Ho,Wo,C) on the pixels (stride*i, stride*j), zeros elsewhere; False when C is not vector-sized."""
        B, H, W, C = dst.shape
        Ho, Wo = src.shape[1], src.shape[2]
        rc = self.lib.gwd_stride_place(_ptr(src), _ptr(residual), _ptr(dst), B, H, W, Ho, Wo, C, stride, dtype_code(dst), self._stream(src, dst))
        if rc == -4:
            return False
        self._check(rc, "gwd_stride_place")
        return True

    def psp_pool_forward(self, x, p16, p8, p4, p2):
        """x (B,H,W,C) -> its 16/8/4/2 average pools in one pass; False when the shape is not supported (use avgpool_forward)."""
        B, H, W, C = x.shape
        rc = self.lib.gwd_psp_pool_forward(_ptr(x), _ptr(p16), _ptr(p8), _ptr(p4), _ptr(p2), B, H, W, C, dtype_code(x), self._stream(x, p16, p8, p4, p2))
        if rc == -4:
            return False
        self._check(rc, "gwd_psp_pool_forward")
        return True

    def psp_pool_backward(self, g_pass, g16, g8, g4, g2, gx):
        """gx (B,H,W,C) = g_pass (may be a channel slice of a wider map, or None) + the four pools' gradients spread back."""
        B, H, W, C = gx.shape
        ld = self._pixel_pitch(g_pass, H, W, C) if g_pass is not None else 0
        self._check(self.lib.gwd_psp_pool_backward(_ptr_pitched(g_pass), _ptr(g16), _ptr(g8), _ptr(g4), _ptr(g2), _ptr(gx), B, H, W, C, ld,
                                                   dtype_code(gx), self._stream(gx, g16, g8, g4, g2)), "gwd_psp_pool_backward")

    def avgpool_forward(self, x, y, B, H, W, C, k):
        self._check(self.lib.gwd_avgpool_forward(_ptr(x), _ptr(y), B, H, W, C, k, dtype_code(x), self._stream(x, y)),
                    "gwd_avgpool_forward")

    def avgpool_backward(self, gy, gx, B, H, W, C, k):
        self._check(self.lib.gwd_avgpool_backward(_ptr(gy), _ptr(gx), B, H, W, C, k, dtype_code(gy),
                                                  self._stream(gy, gx)), "gwd_avgpool_backward")

    def winattn_forward(self, q, k, v, o, bias, region, wpi, scale, rel_index=None):
        """q,k,v,o: (W, 49, heads, hd) tensors or views; bias (heads,49,49) fp32 - or, with rel_index (49*49 int32), the
        (n_rel, heads) relative-position TABLE itself; region (wpi,49) int32 or None."""
        W, N, H, D = q.shape
        s = [_strided(t) for t in (q, k, v, o)]
        n_rel = bias.shape[0] if rel_index is not None else 0
        self._check(self.lib.gwd_winattn_forward(*[ctypes.byref(x) for x in s], _ptr(bias), _ptr(rel_index), n_rel, _ptr(region), W, wpi,
                                                 H, D, scale, dtype_code(q), self._stream(q, k, v, o, bias, rel_index)), "gwd_winattn_forward")

    def winattn_backward(self, q, k, v, go, gq, gk, gv, bias, dbias, region, wpi, scale, rel_index=None, head_major=False):
        """dbias: same layout as bias (dense, or the table's gradient with rel_index); ACCUMULATED into.  head_major (rel_index only):
        dbias is a (heads, n_rel) scratch instead of the (n_rel, heads) table gradient."""
        W, N, H, D = q.shape
        s = [_strided(t) for t in (q, k, v, go, gq, gk, gv)]
        n_rel = bias.shape[0] if rel_index is not None else 0
        self._check(self.lib.gwd_winattn_backward(*[ctypes.byref(x) for x in s], _ptr(bias), _ptr(dbias), _ptr(rel_index), n_rel,
                                                  _ptr(region), W, wpi, H, D, scale, int(bool(head_major)), dtype_code(q),
                                                  self._stream(q, go, gq, bias, dbias, rel_index)), "gwd_winattn_backward")

    def ref_scores_forward(self, q, ref_k, ra, B, nwin, scale):
        """q (B*nwin, 49, H, hd) operand / view, ref_k (B, R, H*hd), ra (B, nwin*49, R, H) out."""
        H, hd, R = q.shape[2], q.shape[3], ref_k.shape[1]
        sq = _strided(q)
        self._check(self.lib.gwd_ref_scores_forward(ctypes.byref(sq), _ptr(ref_k), _ptr(ra), B, nwin, R, H, hd, float(scale),
                                                    dtype_code(q), self._stream(q, ref_k, ra)), "gwd_ref_scores_forward")

    def ref_scores_backward(self, q, ref_k, g, dq, d_ref_k, B, nwin, scale):
        H, hd, R = q.shape[2], q.shape[3], ref_k.shape[1]
        sq, sdq = _strided(q), _strided(dq)
        self._check(self.lib.gwd_ref_scores_backward(ctypes.byref(sq), _ptr(ref_k), _ptr(g), ctypes.byref(sdq), _ptr(d_ref_k), B, nwin,
                                                     R, H, hd, float(scale), dtype_code(q), self._stream(q, ref_k, g, dq, d_ref_k)),
                    "gwd_ref_scores_backward")

    def ref_mix_forward(self, ra, ref_v, q_new, att, H):
        """ra (B, T, R, H), ref_v (B, R, C) -> q_new (B, T, C), att (B, T, R, H) or None."""
        B, T, R = ra.shape[0], ra.shape[1], ra.shape[2]
        self._check(self.lib.gwd_ref_mix_forward(_ptr(ra), _ptr(ref_v), _ptr(q_new), _ptr(att), B, T, R, H, ref_v.shape[2] // H,
                                                 dtype_code(ra), self._stream(ra, ref_v, q_new, att)), "gwd_ref_mix_forward")

    def ref_mix_backward(self, att, ref_v, g, d_ra, d_ref_v, H):
        B, T, R = att.shape[0], att.shape[1], att.shape[2]
        self._check(self.lib.gwd_ref_mix_backward(_ptr(att), _ptr(ref_v), _ptr(g), _ptr(d_ra), _ptr(d_ref_v), B, T, R, H,
                                                  ref_v.shape[2] // H, dtype_code(att), self._stream(att, ref_v, g, d_ra, d_ref_v)),
                    "gwd_ref_mix_backward")

    def tokattn_forward(self, q, k, v, o, scale):
        """q,o: (W,49,heads,4); k,v: (W,49,heads,e) tensors or views."""
        W, N, H, _ = q.shape
        s = [_strided(t) for t in (q, k, v, o)]
        self._check(self.lib.gwd_tokattn_forward(*[ctypes.byref(x) for x in s], W, H, k.shape[3], scale, dtype_code(q),
                                                 self._stream(q, k, v, o)), "gwd_tokattn_forward")

    def tokattn_backward(self, q, k, v, go, gq, gk, gv, scale):
        W, N, H, _ = q.shape
        s = [_strided(t) for t in (q, k, v, go, gq, gk, gv)]
        self._check(self.lib.gwd_tokattn_backward(*[ctypes.byref(x) for x in s], W, H, k.shape[3], scale, dtype_code(q),
                                                  self._stream(q, go, gq)), "gwd_tokattn_backward")

    def upsample_taps_collapse(self, w, wk):
        """w (Cout,3,3,Cin) fp32 -> wk (Cin,4,4,Cout): the 4x4 / stride-2 taps of a 3x3 convolution over a 2x nearest-upsampled map."""
        Cout, KH, KW, Cin = w.shape
        if (KH, KW) != (3, 3) or tuple(wk.shape) != (Cin, 4, 4, Cout) or w.dtype != torch.float32 or not (w.is_contiguous() and wk.is_contiguous()):
            raise ValueError("upsample_taps_collapse: w (Cout,3,3,Cin) fp32 -> wk (Cin,4,4,Cout), both contiguous")
        self._check(self.lib.gwd_upsample_taps_collapse(_ptr(w), _ptr(wk), Cout, Cin, dtype_code(wk), self._stream(w, wk)), "gwd_upsample_taps_collapse")

    def upsample_taps_fold(self, D, dw):
        """dw (Cout,3,3,Cin) fp32 += the 4x4-form weight gradient D (Cin,4,4,Cout) fp32 folded back onto the nine taps."""
        Cout, KH, KW, Cin = dw.shape
        if (KH, KW) != (3, 3) or tuple(D.shape) != (Cin, 4, 4, Cout) or D.dtype != torch.float32 or dw.dtype != torch.float32 \
                or not (D.is_contiguous() and dw.is_contiguous()):
            raise ValueError("upsample_taps_fold: D (Cin,4,4,Cout) fp32 -> dw (Cout,3,3,Cin) fp32, both contiguous")
        self._check(self.lib.gwd_upsample_taps_fold(_ptr(D), _ptr(dw), Cout, Cin, self._stream(D, dw)), "gwd_upsample_taps_fold")

    PYR_MAX_BRANCHES = 4

    @staticmethod
    def _pyr_branches(maps, B, N, like):
        """Pointer / size arrays of the product maps (B,h_k,w_k,9,N) of gwd_pyr_tail_forward / _backward."""
        if not 1 <= len(maps) <= HipLibrary.PYR_MAX_BRANCHES:
            raise ValueError("pyr_tail: 1 to %d low-resolution branches, got %d" % (HipLibrary.PYR_MAX_BRANCHES, len(maps)))
        for m in maps:
            if m.dim() != 5 or m.shape[0] != B or m.shape[3] != 9 or m.shape[4] != N or m.dtype != like.dtype or not m.is_contiguous():
                raise ValueError("pyr_tail: a product map is (B,h,w,9,N) contiguous in the map's dtype, got %r" % (tuple(m.shape),))
        ptrs = (ctypes.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
        hk = (ctypes.c_int32 * len(maps))(*[m.shape[1] for m in maps])
        wk = (ctypes.c_int32 * len(maps))(*[m.shape[2] for m in maps])
        return ptrs, hk, wk

    def pyr_tail_forward(self, part, Zs, gamma, beta, z, y, mean, rstd, gelu):
        """y = [GELU](LayerNorm(part + the bilinear gather of the product maps Zs)), mean, rstd; z (or None) receives the sum itself
        (gwd_pyr_tail_forward).  False when the library has no kernel for the shape (nothing was launched)."""
        B, H, W, N = part.shape
        ptrs, hk, wk = self._pyr_branches(Zs, B, N, part)
        rc = self.lib.gwd_pyr_tail_forward(_ptr(part), ptrs, hk, wk, len(Zs), _ptr(gamma), _ptr(beta), _ptr(z), _ptr(y), _ptr(mean), _ptr(rstd),
                                           B, H, W, N, int(bool(gelu)), dtype_code(part), self._stream(part, y, *Zs))
        if rc == -4:
            return False
        self._check(rc, "gwd_pyr_tail_forward")
        return True

    def pyr_tail_backward(self, gz, Gs):
        """Gs[k] (B,h_k,w_k,9,N) = the gradient of the product map Z_k from gz (B,H,W,N) (gwd_pyr_tail_backward)."""
        B, H, W, N = gz.shape
        ptrs, hk, wk = self._pyr_branches(Gs, B, N, gz)
        self._check(self.lib.gwd_pyr_tail_backward(_ptr(gz), ptrs, hk, wk, len(Gs), B, H, W, N, dtype_code(gz), self._stream(gz, *Gs)),
                    "gwd_pyr_tail_backward")

    def pyr_tail_fold_wgrad(self, d_hi, d_low, dw, C2):
        """dw (N,3,3,(1+nbr) C2) fp32 += d_hi (N,3,3,(1+nbr-nlow) C2) and the low branches' d_low[k] (9 N, C2) (gwd_pyr_tail_fold_wgrad)."""
        N, Cw, nlow = dw.shape[0], dw.shape[-1], len(d_low)
        nbr = Cw // C2 - 1
        ok = dw.dtype == torch.float32 and dw.is_contiguous() and tuple(dw.shape) == (N, 3, 3, (1 + nbr) * C2) and 1 <= nlow <= nbr \
            and d_hi.dtype == torch.float32 and d_hi.is_contiguous() and d_hi.numel() == N * 9 * (1 + nbr - nlow) * C2 \
            and all(d.dtype == torch.float32 and d.is_contiguous() and d.numel() == 9 * N * C2 for d in d_low)
        if not ok:
            raise ValueError("pyr_tail_fold_wgrad: contiguous fp32 tensors in the documented shapes expected")
        ptrs = (ctypes.c_void_p * nlow)(*[d.data_ptr() for d in d_low])
        self._check(self.lib.gwd_pyr_tail_fold_wgrad(_ptr(d_hi), ptrs, nlow, _ptr(dw), N, C2, nbr, self._stream(d_hi, dw, *d_low)),
                    "gwd_pyr_tail_fold_wgrad")

    def tokattn_pair_forward(self, q, q2, k, v, o, o2, scale):
        """Both class tokens against the same k / v in one launch (bf16): q, q2 -> o, o2.  False when the library declines the
        call (-4: an operand that is not 8-byte aligned, a stride that is not a multiple of 4, an e it has no kernel for) - it does so
        before launching anything, and the caller issues two tokattn_forward calls."""
        W, N, H, _ = q.shape
        s = [_strided(t) for t in (q, q2, k, v, o, o2)]
        rc = self.lib.gwd_tokattn_pair_forward(*[ctypes.byref(x) for x in s], W, H, k.shape[3], scale, dtype_code(q),
                                               self._stream(q, q2, k, v, o, o2))
        if rc == -4:
            return False
        self._check(rc, "gwd_tokattn_pair_forward")
        return True

    def tokattn_pair_backward(self, q, q2, k, v, go, go2, gq, gq2, gk, gv, scale):
        """gq, gq2 per token; gk, gv summed over both tokens.  False when the library declines the call (see tokattn_pair_forward)."""
        W, N, H, _ = q.shape
        s = [_strided(t) for t in (q, q2, k, v, go, go2, gq, gq2, gk, gv)]
        rc = self.lib.gwd_tokattn_pair_backward(*[ctypes.byref(x) for x in s], W, H, k.shape[3], scale, dtype_code(q),
                                                self._stream(q, go, gq))
        if rc == -4:
            return False
        self._check(rc, "gwd_tokattn_pair_backward")
        return True

    def certain_sample(self, small, large, coords, edges, sample_num):
        """small (B,1,hs,ws), large (B,1,H,W) fp32; edges (I+1,) fp32; coords (B,S,1,2) fp32 out."""
        B, _, hs, ws = small.shape
        H, W = large.shape[-2:]
        self._check(self.lib.gwd_certain_sample(_ptr(small), _ptr(large), _ptr(coords), B, hs, ws, H, W, _ptr(edges),
                                                edges.numel() - 1, sample_num, self._stream(small, large, coords)),
                    "gwd_certain_sample")

    def bmm(self, a, b, c, M, N, K, a_kmajor=False, b_kmajor=False, alpha=1.0, accumulate=False, splits=1):
        """c[b0][b1] (M x N) = alpha * A (M x K) @ B (N x K)^T over two batch dims (gwd_bmm).  a, b, c: 4-D tensors / views with unit
        inner stride, dims (b0, b1, outer, inner); an operand is (rows, K) - or (K, rows) when *_kmajor.  A batch dim of size 1 in a
        or b broadcasts.  accumulate: c is fp32 and is ADDED to (required for splits > 1)."""
        for t in (a, b, c):
            if t.dim() != 4 or t.stride(3) != 1:
                raise ValueError("bmm: 4-D operands with unit inner stride expected")
        nb0, nb1 = c.shape[0], c.shape[1]
        d = BmmDesc()
        d.a, d.b, d.c = a.data_ptr(), b.data_ptr(), c.data_ptr()
        bs = lambda t, i: 0 if t.shape[i] == 1 else t.stride(i)
        d.a_sb0, d.a_sb1, d.a_ld = bs(a, 0), bs(a, 1), a.stride(2)
        d.b_sb0, d.b_sb1, d.b_ld = bs(b, 0), bs(b, 1), b.stride(2)
        d.c_sb0, d.c_sb1, d.c_ld = c.stride(0), c.stride(1), c.stride(2)
        d.M, d.N, d.K, d.nb0, d.nb1 = M, N, K, nb0, nb1
        d.a_kmajor, d.b_kmajor, d.c_is_f32_accumulate, d.splits = int(a_kmajor), int(b_kmajor), int(accumulate), int(splits)
        if accumulate and c.dtype != torch.float32:
            raise ValueError("bmm: an accumulated result is fp32")
        d.alpha, d.dtype = float(alpha), dtype_code(a)
        self._check(self.lib.gwd_bmm(ctypes.byref(d), self._stream(a, b, c)), "gwd_bmm")

    COLOR_MODES = {"brightness": 0, "contrast": 1, "saturation": 2, "hue": 3}

    def color_adjust(self, rgb, out, mode, factor, scratch=None):
        """One ColorJitter adjustment on a uint8 (h,w,3) device image (gwd_color_adjust); scratch: 1-element int64 tensor for 'contrast'."""
        if rgb.dtype != torch.uint8 or out.dtype != torch.uint8 or rgb.shape != out.shape or rgb.shape[-1] != 3:
            raise ValueError("color_adjust: uint8 (h,w,3) images expected")
        self._check(self.lib.gwd_color_adjust(_ptr(rgb), _ptr(out), _ptr(scratch), rgb.numel() // 3, self.COLOR_MODES[mode], float(factor),
                                              self._stream(rgb, out)), "gwd_color_adjust")

    def resample_u8_pass(self, src, dst, bounds, kk, axis, row_stride, base0, step0, base1, step1):
        """One pass of Pillow's BILINEAR resize over uint8 pixels (gwd_resample_u8_pass); src may be a window / flipped view given by
        the index maps, dst dense: (other, n_out, C) for axis 1, (n_out, other, C) for axis 0."""
        n_out, ksize = kk.shape
        other, C = (dst.shape[0], dst.shape[2]) if axis == 1 else (dst.shape[1], dst.shape[2])
        if src.dtype != torch.uint8 or dst.dtype != torch.uint8 or bounds.dtype != torch.int32 or kk.dtype != torch.int32 or not dst.is_contiguous():
            raise ValueError("resample_u8_pass: uint8 images and int32 tables expected")
        if dst.shape[1 if axis == 1 else 0] != n_out or tuple(bounds.shape) != (n_out, 2):
            raise ValueError("resample_u8_pass: table / output shapes do not match")
        self._check(self.lib.gwd_resample_u8_pass(_ptr_pitched(src), _ptr(dst), _ptr(bounds), _ptr(kk), ksize, axis, n_out, other, C, row_stride,
                                                  base0, step0, base1, step1, self._stream(src, dst, bounds, kk)), "gwd_resample_u8_pass")

    def gather2d(self, src, dst, ytab, xtab, row_stride_bytes, elem_bytes):
        oh, ow = ytab.numel(), xtab.numel()
        if ytab.dtype != torch.int32 or xtab.dtype != torch.int32 or not dst.is_contiguous() or dst.numel() * dst.element_size() != oh * ow * elem_bytes:
            raise ValueError("gather2d: int32 tables and a dense (oh, ow) output expected")
        self._check(self.lib.gwd_gather2d(_ptr_pitched(src), _ptr(dst), _ptr(ytab), _ptr(xtab), oh, ow, row_stride_bytes, elem_bytes,
                                          self._stream(src, dst, ytab, xtab)), "gwd_gather2d")

    @staticmethod
    def _check_tables(tables, what):
        if tables.dtype != torch.int32 or tables.dim() != 1:
            raise ValueError(what + ": one flat int32 table buffer expected")

    def resample_u8_pass_batch(self, jobs, axis, C, tables):
        """gwd_resample_u8_pass_batch: ONE launch for up to AUGMENT_BATCH resample_u8_pass calls of one axis and channel count.
        jobs: (src, dst, row_stride, bounds_off, kk_off, ksize, base0, step0, base1, step1); bounds (n_out,2) and kk (n_out,ksize)
        start at those int32 offsets of `tables`; n_out / other are read off the dense dst as in resample_u8_pass."""
        self._check_tables(tables, "resample_u8_pass_batch")
        if not 0 < len(jobs) <= AUGMENT_BATCH:
            raise ValueError("resample_u8_pass_batch: 1..%d jobs per call" % AUGMENT_BATCH)
        recs = (ResampleJob * len(jobs))()
        ts = [tables]
        for r, (src, dst, row_stride, bounds_off, kk_off, ksize, base0, step0, base1, step1) in zip(recs, jobs):
            if src.dtype != torch.uint8 or dst.dtype != torch.uint8 or not dst.is_contiguous() or dst.dim() != 3 or dst.shape[2] != C:
                raise ValueError("resample_u8_pass_batch: uint8 images with a dense (.., .., C) output expected")
            n_out, other = (dst.shape[1], dst.shape[0]) if axis == 1 else (dst.shape[0], dst.shape[1])
            if min(bounds_off, kk_off) < 0 or bounds_off + 2 * n_out > tables.numel() or kk_off + n_out * ksize > tables.numel():
                raise ValueError("resample_u8_pass_batch: a table lies outside the table buffer")
            r.src, r.dst, r.src_row_stride = src.data_ptr(), dst.data_ptr(), row_stride
            r.bounds_off, r.kk_off, r.ksize, r.n_out, r.other = bounds_off, kk_off, ksize, n_out, other
            r.base0, r.step0, r.base1, r.step1 = base0, step0, base1, step1
            ts += [src, dst]
        self._check(self.lib.gwd_resample_u8_pass_batch(recs, len(jobs), axis, C, _ptr(tables), tables.numel(), self._stream(*ts)),
                    "gwd_resample_u8_pass_batch")

    def gather2d_batch(self, jobs, tables):
        """gwd_gather2d_batch: ONE launch for up to GATHER_BATCH gather2d calls.  jobs: (src, dst, row_stride_bytes, ytab_off,
        xtab_off, oh, ow, elem_bytes) with the index tables at those int32 offsets of `tables`; dst dense."""
        self._check_tables(tables, "gather2d_batch")
        if not 0 < len(jobs) <= GATHER_BATCH:
            raise ValueError("gather2d_batch: 1..%d jobs per call" % GATHER_BATCH)
        recs = (GatherJob * len(jobs))()
        ts = [tables]
        for r, (src, dst, row_stride_bytes, ytab_off, xtab_off, oh, ow, elem_bytes) in zip(recs, jobs):
            if not dst.is_contiguous() or dst.numel() * dst.element_size() != oh * ow * elem_bytes:
                raise ValueError("gather2d_batch: a dense (oh, ow) output expected")
            if min(ytab_off, xtab_off) < 0 or ytab_off + oh > tables.numel() or xtab_off + ow > tables.numel():
                raise ValueError("gather2d_batch: a table lies outside the table buffer")
            r.src, r.dst, r.src_row_stride_bytes = src.data_ptr(), dst.data_ptr(), row_stride_bytes
            r.ytab_off, r.xtab_off, r.oh, r.ow, r.elem_bytes = ytab_off, xtab_off, oh, ow, elem_bytes
            ts += [src, dst]
        self._check(self.lib.gwd_gather2d_batch(recs, len(jobs), _ptr(tables), tables.numel(), self._stream(*ts)), "gwd_gather2d_batch")

    def color_adjust_batch(self, jobs, sums, sums_only=False):
        """gwd_color_adjust_batch: one ColorJitter adjustment IN PLACE on each of up to AUGMENT_BATCH uint8 (h,w,3) device images
        in ONE launch.  jobs: (rgb, mode name | None = leave untouched, factor as color_adjust takes it); sums: int64 tensor with
        one zeroed element per job when a job is a 'contrast' (else None).  sums_only=True is the companion launch that adds
        each contrast job's luma sum to sums[job]; run it before the adjusting call."""
        if not 0 < len(jobs) <= AUGMENT_BATCH:
            raise ValueError("color_adjust_batch: 1..%d jobs per call" % AUGMENT_BATCH)
        if sums is not None and (sums.dtype != torch.int64 or sums.numel() < len(jobs)):
            raise ValueError("color_adjust_batch: sums is an int64 tensor with an element per job")
        recs = (ColorJob * len(jobs))()
        ts = [sums]
        for r, (rgb, mode, factor) in zip(recs, jobs):
            if rgb.dtype != torch.uint8 or rgb.shape[-1] != 3 or not rgb.is_contiguous():
                raise ValueError("color_adjust_batch: dense uint8 (h,w,3) images expected")
            r.rgb, r.npix = rgb.data_ptr(), rgb.numel() // 3
            r.mode, r.factor = (-1 if mode is None else self.COLOR_MODES[mode]), float(factor)
            ts.append(rgb)
        self._check(self.lib.gwd_color_adjust_batch(recs, len(jobs), _ptr(sums), COLOR_SUMS if sums_only else COLOR_ADJUST,
                                                    self._stream(*ts)), "gwd_color_adjust_batch")

    def match_cost(self, logits, lines, tgt_lines, tgt_labels, cost, w_line, w_class):
        """cost (L,B,Q,cap) of matcher.py:52-70 from logits (L,B,Q,K), lines (L,B,Q,D), padded targets (cap,D) / (cap,) int64."""
        L_, B, Q, K = logits.shape
        D, cap = lines.shape[-1], tgt_lines.shape[0]
        if tgt_labels.dtype != torch.int64 or tuple(cost.shape) != (L_, B, Q, cap) or any(t.dtype != torch.float32 for t in (logits, lines, tgt_lines, cost)):
            raise ValueError("match_cost: fp32 tensors, int64 labels and cost (L,B,Q,cap) expected")
        self._check(self.lib.gwd_match_cost(_ptr(logits), _ptr(lines), _ptr(tgt_lines), _ptr(tgt_labels), _ptr(cost), L_, B, Q, cap, K, D,
                                            w_line, w_class, self._stream(logits, lines, cost)), "gwd_match_cost")

    def set_losses_forward(self, logits, lines, tgt_lines, tgt_labels, bidx, valid, qot, class_weight, num_items, world, target_class, ce, l1, wsum,
                           gamma=None):
        """gamma None: weighted cross entropy (gwd_set_losses_forward); a float: the focal label term (gwd_set_losses_focal_forward)."""
        L_, B, Q, K = logits.shape
        D, cap = lines.shape[-1], tgt_lines.shape[0]
        if any(t.dtype != torch.int32 for t in (bidx, valid, qot, target_class)) or tgt_labels.dtype != torch.int64:
            raise ValueError("set_losses_forward: int32 bidx / valid / qot / target_class and int64 labels expected")
        head = (_ptr(logits), _ptr(lines), _ptr(tgt_lines), _ptr(tgt_labels), _ptr(bidx), _ptr(valid), _ptr(qot), _ptr(class_weight), _ptr(num_items),
                float(world))
        tail = (_ptr(target_class), _ptr(ce), _ptr(l1), _ptr(wsum), L_, B, Q, cap, K, D, self._stream(logits, lines, ce, l1))
        if gamma is None:
            self._check(self.lib.gwd_set_losses_forward(*head, *tail), "gwd_set_losses_forward")
        else:
            self._check(self.lib.gwd_set_losses_focal_forward(*head, float(gamma), *tail), "gwd_set_losses_focal_forward")

    def set_losses_backward(self, logits, lines, tgt_lines, bidx, valid, qot, class_weight, num_items, world, target_class, wsum, g_ce, g_l1,
                            dlogits, dlines, gamma=None):
        L_, B, Q, K = logits.shape
        D, cap = lines.shape[-1], tgt_lines.shape[0]
        head = (_ptr(logits), _ptr(lines), _ptr(tgt_lines), _ptr(bidx), _ptr(valid), _ptr(qot), _ptr(class_weight), _ptr(num_items), float(world))
        tail = (_ptr(target_class), _ptr(wsum), _ptr(g_ce), _ptr(g_l1), _ptr(dlogits), _ptr(dlines), L_, B, Q, cap, K, D,
                self._stream(logits, lines, dlogits, dlines))
        if gamma is None:
            self._check(self.lib.gwd_set_losses_backward(*head, *tail), "gwd_set_losses_backward")
        else:
            self._check(self.lib.gwd_set_losses_focal_backward(*head, float(gamma), *tail), "gwd_set_losses_focal_backward")

    def lsap(self, cost, col_offsets, out, max_targets):
        """cost (layers,B,Q,sumT) fp32; col_offsets (B+1,) int32 DEVICE data (image b owns columns [off[b], off[b+1]),
        at most max_targets <= 1024 of them; columns from off[B] on are padding); out (layers,sumT) int32: the query
        assigned to every target column, Q for padding columns and for the surplus targets of an image with more than Q."""
        L_, B, Q, sumT = cost.shape
        self._check(self.lib.gwd_lsap(_ptr(cost), _ptr(col_offsets), _ptr(out), L_, B, Q, sumT, max_targets,
                                      self._stream(cost, col_offsets, out)), "gwd_lsap")

    def inorm_gelu_forward(self, a, u, y, part, stat, B, L, C, S, eps):
        self._check(self.lib.gwd_inorm_gelu_forward(_ptr(a), _ptr(u), _ptr(y), _ptr(part), _ptr(stat), B, L, C, S, eps,
                                                    dtype_code(u), self._stream(a, u, y)), "gwd_inorm_gelu_forward")

    def inorm_gelu_backward(self, gy, u, stat, part, du, B, L, C, S):
        self._check(self.lib.gwd_inorm_gelu_backward(_ptr(gy), _ptr(u), _ptr(stat), _ptr(part), _ptr(du), B, L, C, S,
                                                     dtype_code(u), self._stream(gy, u, du)), "gwd_inorm_gelu_backward")

    def point_sample_forward(self, fmap, coords, out, B, H, W, C, S, mode):
        self._check(self.lib.gwd_point_sample_forward(_ptr(fmap), _ptr(coords), _ptr(out), B, H, W, C, S, mode, dtype_code(fmap),
                                                      self._stream(fmap, out)), "gwd_point_sample_forward")

    def point_sample_backward_gather(self, gout, coords, gmap, B, H, W, C, S, mode):
        """Writes every element of gmap (no pre-zeroing); False when the shape is not supported (zero gmap, point_sample_backward)."""
        rc = self.lib.gwd_point_sample_backward_gather(_ptr(gout), _ptr(coords), _ptr(gmap), B, H, W, C, S, mode, dtype_code(gmap),
                                                       self._stream(gout, gmap))
        if rc == -4:
            return False
        self._check(rc, "gwd_point_sample_backward_gather")
        return True

    def point_sample_framed_forward(self, fmap, coords, out, B, H, W, C, S, frame):
        """Nearest sampling in the padded / rolled (Hf, Wf, shift) frame of the map, without building it."""
        Hf, Wf, shift = frame
        self._check(self.lib.gwd_point_sample_framed_forward(_ptr(fmap), _ptr(coords), _ptr(out), B, H, W, C, S, Hf, Wf, shift, dtype_code(fmap),
                                                             self._stream(fmap, out)), "gwd_point_sample_framed_forward")

    def point_sample_framed_backward(self, gout, coords, gmap, B, H, W, C, S, frame):
        """Every element of gmap written; S <= 256 (the caller checks before choosing the framed form)."""
        Hf, Wf, shift = frame
        self._check(self.lib.gwd_point_sample_framed_backward(_ptr(gout), _ptr(coords), _ptr(gmap), B, H, W, C, S, Hf, Wf, shift, dtype_code(gmap),
                                                              self._stream(gout, gmap)), "gwd_point_sample_framed_backward")

    def point_sample_backward(self, gout, coords, gmap, B, H, W, C, S, mode):
        self._check(self.lib.gwd_point_sample_backward(_ptr(gout), _ptr(coords), _ptr(gmap), B, H, W, C, S, mode, dtype_code(gmap),
                                                       self._stream(gout, gmap)), "gwd_point_sample_backward")

    def weight_prep_batch(self, table, n_jobs, total_blocks, block_job=None):
        """table: device uint8 tensor holding n_jobs packed gwd_prep_job records (see PrepJob); block_job: device int32 (total_blocks,)
        job index per block (optional, saves every block a binary search)."""
        self._check(self.lib.gwd_weight_prep_batch(_ptr(table), n_jobs, total_blocks, _ptr(block_job), self._stream(table)), "gwd_weight_prep_batch")

    def window_map(self, src, dst, B, H, W, C, shift, gather, residual=None):
        self._check(self.lib.gwd_window_map(_ptr(src), _ptr(dst), _ptr(residual), B, H, W, C, shift, int(gather), dtype_code(src),
                                            self._stream(src, dst)), "gwd_window_map")

    def window_map_multi(self, srcs, dsts, B, H, W, Cs, shift, gather, residuals=None):
        """gwd_window_map for up to 4 maps of one geometry in one launch (residuals: list with None entries, or None).  False when the
        library declines the call (-4: a channel count whose rows are not whole 16-byte vectors) - before launching anything; the caller
        issues window_map per map."""
        n = len(srcs)
        vpn, i32n = ctypes.c_void_p * n, ctypes.c_int32 * n
        res = [None] * n if residuals is None else list(residuals)
        addr = lambda t: None if t is None else _ptr(t).value
        rc = self.lib.gwd_window_map_multi(vpn(*[addr(t) for t in srcs]), vpn(*[addr(t) for t in dsts]), vpn(*[addr(t) for t in res]),
                                           i32n(*[int(c) for c in Cs]), n, B, H, W, shift, int(gather), dtype_code(srcs[0]),
                                           self._stream(*srcs, *dsts))
        if rc == -4:
            return False
        self._check(rc, "gwd_window_map_multi")
        return True

    def sqnorm(self, g, sq, n):
        self._check(self.lib.gwd_sqnorm(_ptr(g), _ptr(sq), n, self._stream(g, sq)), "gwd_sqnorm")

    def adamw_step(self, p, g, m, v, p16, sq, n, lr, b1, b2, eps, wd, bc1, bc2, max_norm, grad_scale):
        self._check(self.lib.gwd_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p16), _ptr(sq), n, lr, b1, b2, eps,
                                            wd, bc1, bc2, max_norm, grad_scale, self._stream(p, g, m, v)),
                    "gwd_adamw_step")

    @staticmethod
    def _check_bytes(t, nbytes, what):
        if t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < nbytes:
            raise ValueError("%s: a flat uint8 buffer of at least %d bytes expected" % (what, nbytes))

    def segment_stats(self, x, seg_begin, seg_end, chunks, partial, out):
        """gwd_segment_stats.  x flat fp32; seg_begin / seg_end (S,) int64; chunks (n_chunks, 2) int64 = gwd_health_chunk records
        (engine.chunk_table); partial: uint8, workspace_bytes(WS_HEALTH, n_chunks); out: uint8, S * 16 bytes = S gwd_segment_record."""
        S, n_chunks = seg_begin.numel(), chunks.shape[0]
        if x.dtype != torch.float32 or x.dim() != 1:
            raise TypeError("segment_stats: x is a flat float32 buffer")
        if seg_begin.dtype != torch.int64 or seg_end.dtype != torch.int64 or seg_end.shape != seg_begin.shape or seg_begin.dim() != 1 or S < 1:
            raise ValueError("segment_stats: seg_begin and seg_end are (S,) int64 tables, S >= 1")
        if chunks.dtype != torch.int64 or chunks.dim() != 2 or chunks.shape[1] != 2:
            raise ValueError("segment_stats: chunks is an (n_chunks, 2) int64 table of gwd_health_chunk records")
        self._check_bytes(partial, max(n_chunks, 1) * HEALTH_RECORD_BYTES, "segment_stats: partial")
        self._check_bytes(out, S * HEALTH_RECORD_BYTES, "segment_stats: out")
        self._check(self.lib.gwd_segment_stats(_ptr(x), _ptr(seg_begin), _ptr(seg_end), S, _ptr(chunks), n_chunks, _ptr(partial), _ptr(out),
                                               self._stream(x, seg_begin, seg_end, chunks, partial, out)), "gwd_segment_stats")

    def health_decide(self, stats, S, loss, ctl, ring, ring_len, bad, beta1, beta2, max_norm, grad_scale):
        """gwd_health_decide.  stats: uint8, S gwd_segment_record; loss: None or one device fp32; ctl: uint8, 64 bytes; ring: uint8,
        ring_len * 32 bytes; bad (S,) int32."""
        self._check_bytes(stats, S * HEALTH_RECORD_BYTES, "health_decide: stats")
        self._check_bytes(ctl, HEALTH_CTL_BYTES, "health_decide: ctl")
        self._check_bytes(ring, ring_len * HEALTH_RING_BYTES, "health_decide: ring")
        if bad.dtype != torch.int32 or bad.numel() < S:
            raise ValueError("health_decide: bad is an int32 table of S entries")
        if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1):
            raise TypeError("health_decide: loss is one float32 value on the device, or None")
        self._check(self.lib.gwd_health_decide(_ptr(stats), S, _ptr(loss), _ptr(ctl), _ptr(ring), ring_len, _ptr(bad), float(beta1),
                                               float(beta2), max_norm, grad_scale, self._stream(stats, loss, ctl, ring, bad)),
                    "gwd_health_decide")

    def adamw_step_guarded(self, p, g, m, v, p16, ctl, n, lr, b1, b2, eps, wd, max_norm, grad_scale):
        self._check_bytes(ctl, HEALTH_CTL_BYTES, "adamw_step_guarded: ctl")
        if any(t.dtype != torch.float32 or t.numel() < n for t in (p, g, m, v)) or (p16 is not None and (p16.dtype != torch.bfloat16 or p16.numel() < n)):
            raise ValueError("adamw_step_guarded: p, g, m, v are float32 (p16 bfloat16) ranges of at least n elements")
        self._check(self.lib.gwd_adamw_step_guarded(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p16), _ptr(ctl), n, lr, b1, b2, eps, wd,
                                                    max_norm, grad_scale, self._stream(p, g, m, v, ctl)),
                    "gwd_adamw_step_guarded")

    def adamw_step_ema(self, p, g, m, v, p16, ema, sq, ctl, n, lr, b1, b2, eps, wd, bc1, bc2, max_norm, grad_scale, ema_decay, ema_warmup,
                       ema_t):
        """gwd_adamw_step_ema.  ctl None: the step of adamw_step (sq may be None), ema_t the 1-based update number; ctl (uint8, 64
        bytes): the step of adamw_step_guarded (sq, bc1, bc2 ignored), ema_t the applied-step count at which averaging began."""
        if ctl is not None:
            self._check_bytes(ctl, HEALTH_CTL_BYTES, "adamw_step_ema: ctl")
        if any(t.dtype != torch.float32 or t.numel() < n for t in (p, g, m, v, ema)) or \
                (p16 is not None and (p16.dtype != torch.bfloat16 or p16.numel() < n)):
            raise ValueError("adamw_step_ema: p, g, m, v, ema are float32 (p16 bfloat16) ranges of at least n elements")
        if sq is not None and (sq.dtype != torch.float64 or sq.numel() < 1):
            raise TypeError("adamw_step_ema: sq is one float64 value on the device, or None")
        if not 0.0 < float(ema_decay) < 1.0:
            raise ValueError("adamw_step_ema: ema_decay must lie in (0, 1), got %r" % (ema_decay,))
        self._check(self.lib.gwd_adamw_step_ema(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p16), _ptr(ema), _ptr(sq), _ptr(ctl), n, lr, b1, b2,
                                                eps, wd, bc1, bc2, max_norm, grad_scale, float(ema_decay), int(bool(ema_warmup)), int(ema_t),
                                                self._stream(p, g, m, v, ema, ctl)), "gwd_adamw_step_ema")

    def ema_swap(self, p, ema, p16, n):
        """gwd_ema_swap: p <-> ema in place over n elements, p16 (or None) = bf16(new p)."""
        if any(t.dtype != torch.float32 or t.numel() < n for t in (p, ema)) or (p16 is not None and (p16.dtype != torch.bfloat16 or p16.numel() < n)):
            raise ValueError("ema_swap: p and ema are float32 (p16 bfloat16) ranges of at least n elements")
        self._check(self.lib.gwd_ema_swap(_ptr(p), _ptr(ema), _ptr(p16), n, self._stream(p, ema)), "gwd_ema_swap")

    @staticmethod
    def _typed(what, pairs):
        for t, dt in pairs:
            if t is not None and t.dtype != dt:
                raise TypeError("%s: expected %s, got %s" % (what, dt, t.dtype))

    def glass_regions(self, labels, depth_mm, sizes, max_regions, min_area, connectivity, max_candidates, lo_mm, hi_mm, workspace,
                      region_map, region_count, region_total, records):
        """gwd_glass_regions: labels uint8 / depth_mm uint16 (B,Fh,Fw), sizes (B,2) int32; outputs region_map uint8 (B,Fh,Fw),
        region_count / region_total (B,) int32, records (B,max_regions,12) int64; workspace: a uint8 tensor of
        workspace_bytes(WS_REGIONS, B, Fh, Fw, max_candidates) bytes."""
        self._typed("gwd_glass_regions", ((labels, torch.uint8), (depth_mm, torch.uint16), (sizes, torch.int32), (workspace, torch.uint8),
                                          (region_map, torch.uint8), (region_count, torch.int32), (region_total, torch.int32),
                                          (records, torch.int64)))
        B, Fh, Fw = labels.shape
        if tuple(depth_mm.shape) != (B, Fh, Fw) or tuple(sizes.shape) != (B, 2) or tuple(region_map.shape) != (B, Fh, Fw) \
                or region_count.numel() != B or region_total.numel() != B or tuple(records.shape) != (B, max_regions, REGION_RECORD) \
                or workspace.numel() < self.workspace_bytes(WS_REGIONS, B, Fh, Fw, max_candidates):
            raise ValueError("gwd_glass_regions: operand sizes do not match (B, Fh, Fw, max_regions) = (%d, %d, %d, %d)"
                             % (B, Fh, Fw, max_regions))
        self._check(self.lib.gwd_glass_regions(
            _ptr(labels), _ptr(depth_mm), _ptr(sizes), B, Fh, Fw, int(max_regions), int(min_area), int(connectivity), int(max_candidates),
            int(lo_mm), int(hi_mm), _ptr(workspace), _ptr(region_map), _ptr(region_count), _ptr(region_total), _ptr(records),
            self._stream(labels, depth_mm, sizes, workspace, region_map, region_count, region_total, records)), "gwd_glass_regions")

    def region_planes(self, region_map, depth_mm, sizes, region_count, records, lo_mm, hi_mm, workspace, planes):
        """gwd_region_planes: the outputs and the workspace of glass_regions in, planes (B,max_regions,6) float64 out."""
        self._typed("gwd_region_planes", ((region_map, torch.uint8), (depth_mm, torch.uint16), (sizes, torch.int32),
                                          (region_count, torch.int32), (records, torch.int64), (workspace, torch.uint8),
                                          (planes, torch.float64)))
        B, Fh, Fw = region_map.shape
        R = records.shape[1]
        if tuple(depth_mm.shape) != (B, Fh, Fw) or tuple(sizes.shape) != (B, 2) or region_count.numel() != B \
                or tuple(records.shape) != (B, R, REGION_RECORD) or tuple(planes.shape) != (B, R, 6) \
                or workspace.numel() < self.workspace_bytes(WS_REGIONS, B, Fh, Fw, 1):
            raise ValueError("gwd_region_planes: operand sizes do not match (B, Fh, Fw, max_regions) = (%d, %d, %d, %d)" % (B, Fh, Fw, R))
        self._check(self.lib.gwd_region_planes(
            _ptr(region_map), _ptr(depth_mm), _ptr(sizes), _ptr(region_count), _ptr(records), B, Fh, Fw, R, int(lo_mm), int(hi_mm),
            _ptr(workspace), _ptr(planes), self._stream(region_map, depth_mm, sizes, region_count, records, workspace, planes)),
            "gwd_region_planes")

    def depth_planar(self, region_map, depth_mm, depth, sizes, region_count, planes, dmin, dmax, depth_planar, depth_planar_mm):
        """gwd_depth_planar: depth (B,Fh,Fw) float32 or None (millimetres / 1000); outputs float32 / uint16 (B,Fh,Fw)."""
        self._typed("gwd_depth_planar", ((region_map, torch.uint8), (depth_mm, torch.uint16), (depth, torch.float32), (sizes, torch.int32),
                                         (region_count, torch.int32), (planes, torch.float64), (depth_planar, torch.float32),
                                         (depth_planar_mm, torch.uint16)))
        B, Fh, Fw = region_map.shape
        R = planes.shape[1]
        shape = (B, Fh, Fw)
        if tuple(depth_mm.shape) != shape or (depth is not None and tuple(depth.shape) != shape) or tuple(sizes.shape) != (B, 2) \
                or region_count.numel() != B or tuple(planes.shape) != (B, R, 6) or tuple(depth_planar.shape) != shape \
                or tuple(depth_planar_mm.shape) != shape:
            raise ValueError("gwd_depth_planar: operand sizes do not match (B, Fh, Fw, max_regions) = (%d, %d, %d, %d)" % (B, Fh, Fw, R))
        self._check(self.lib.gwd_depth_planar(
            _ptr(region_map), _ptr(depth_mm), _ptr(depth), _ptr(sizes), _ptr(region_count), _ptr(planes), B, Fh, Fw, R, float(dmin),
            float(dmax), _ptr(depth_planar), _ptr(depth_planar_mm),
            self._stream(region_map, depth_mm, depth, sizes, region_count, planes, depth_planar, depth_planar_mm)), "gwd_depth_planar")

    def fusion_ring(self, labels, sensor_mm, depth_mm, sizes, region_map, region_count, max_regions, ring, gap, lo_mm, hi_mm, align,
                    min_align, workspace, fusion_ring, fusion_scale):
        """gwd_fusion_ring: labels / region_map uint8, sensor_mm / depth_mm uint16 (B,Fh,Fw), sizes (B,2) / region_count (B,) int32;
        outputs fusion_ring uint8 (B,Fh,Fw), fusion_scale (B,4) float64; workspace: a uint8 tensor of
        workspace_bytes(WS_FUSION, B, Fh, Fw) bytes."""
        self._typed("gwd_fusion_ring", ((labels, torch.uint8), (sensor_mm, torch.uint16), (depth_mm, torch.uint16), (sizes, torch.int32),
                                        (region_map, torch.uint8), (region_count, torch.int32), (workspace, torch.uint8),
                                        (fusion_ring, torch.uint8), (fusion_scale, torch.float64)))
        B, Fh, Fw = labels.shape
        shape = (B, Fh, Fw)
        if tuple(sensor_mm.shape) != shape or tuple(depth_mm.shape) != shape or tuple(region_map.shape) != shape \
                or tuple(fusion_ring.shape) != shape or tuple(sizes.shape) != (B, 2) or region_count.numel() != B \
                or tuple(fusion_scale.shape) != (B, 4) or workspace.numel() < self.workspace_bytes(WS_FUSION, B, Fh, Fw):
            raise ValueError("gwd_fusion_ring: operand sizes do not match (B, Fh, Fw) = (%d, %d, %d)" % shape)
        self._check(self.lib.gwd_fusion_ring(
            _ptr(labels), _ptr(sensor_mm), _ptr(depth_mm), _ptr(sizes), _ptr(region_map), _ptr(region_count), B, Fh, Fw, int(max_regions),
            int(ring), int(gap), int(lo_mm), int(hi_mm), int(bool(align)), int(min_align), _ptr(workspace), _ptr(fusion_ring),
            _ptr(fusion_scale),
            self._stream(labels, sensor_mm, depth_mm, sizes, region_map, region_count, workspace, fusion_ring, fusion_scale)),
            "gwd_fusion_ring")

    def fusion_planes(self, fusion_ring, sensor_mm, sizes, region_count, records, ring, lo_mm, hi_mm, trim, min_ring, max_rms, workspace,
                      fusion_planes):
        """gwd_fusion_planes: the ring and the workspace of fusion_ring in, fusion_planes (B,max_regions,12) float64 out; max_rms
        None: no limit."""
        self._typed("gwd_fusion_planes", ((fusion_ring, torch.uint8), (sensor_mm, torch.uint16), (sizes, torch.int32),
                                          (region_count, torch.int32), (records, torch.int64), (workspace, torch.uint8),
                                          (fusion_planes, torch.float64)))
        B, Fh, Fw = fusion_ring.shape
        R = records.shape[1]
        if tuple(sensor_mm.shape) != (B, Fh, Fw) or tuple(sizes.shape) != (B, 2) or region_count.numel() != B \
                or tuple(records.shape) != (B, R, REGION_RECORD) or tuple(fusion_planes.shape) != (B, R, FUSION_PLANE) \
                or workspace.numel() < self.workspace_bytes(WS_FUSION, B, Fh, Fw):
            raise ValueError("gwd_fusion_planes: operand sizes do not match (B, Fh, Fw, max_regions) = (%d, %d, %d, %d)" % (B, Fh, Fw, R))
        self._check(self.lib.gwd_fusion_planes(
            _ptr(fusion_ring), _ptr(sensor_mm), _ptr(sizes), _ptr(region_count), _ptr(records), B, Fh, Fw, R, int(ring), int(lo_mm),
            int(hi_mm), float(trim), int(min_ring), float("inf") if max_rms is None else float(max_rms), _ptr(workspace),
            _ptr(fusion_planes), self._stream(fusion_ring, sensor_mm, sizes, region_count, records, workspace, fusion_planes)),
            "gwd_fusion_planes")

    def fusion_depth(self, labels, sensor_mm, depth, sizes, region_map, region_count, fusion_planes, fusion_scale, lo_mm, hi_mm, dmin,
                     dmax, depth_fused, depth_fused_mm, fused_source):
        """gwd_fusion_depth: depth_fused float32 / depth_fused_mm uint16 / fused_source uint8 (B,Fh,Fw) out."""
        self._typed("gwd_fusion_depth", ((labels, torch.uint8), (sensor_mm, torch.uint16), (depth, torch.float32), (sizes, torch.int32),
                                         (region_map, torch.uint8), (region_count, torch.int32), (fusion_planes, torch.float64),
                                         (fusion_scale, torch.float64), (depth_fused, torch.float32), (depth_fused_mm, torch.uint16),
                                         (fused_source, torch.uint8)))
        B, Fh, Fw = labels.shape
        shape, R = (B, Fh, Fw), fusion_planes.shape[1]
        if any(tuple(t.shape) != shape for t in (sensor_mm, depth, region_map, depth_fused, depth_fused_mm, fused_source)) \
                or tuple(sizes.shape) != (B, 2) or region_count.numel() != B or tuple(fusion_planes.shape) != (B, R, FUSION_PLANE) \
                or tuple(fusion_scale.shape) != (B, 4):
            raise ValueError("gwd_fusion_depth: operand sizes do not match (B, Fh, Fw, max_regions) = (%d, %d, %d, %d)" % (B, Fh, Fw, R))
        self._check(self.lib.gwd_fusion_depth(
            _ptr(labels), _ptr(sensor_mm), _ptr(depth), _ptr(sizes), _ptr(region_map), _ptr(region_count), _ptr(fusion_planes),
            _ptr(fusion_scale), B, Fh, Fw, R, int(lo_mm), int(hi_mm), float(dmin), float(dmax), _ptr(depth_fused), _ptr(depth_fused_mm),
            _ptr(fused_source),
            self._stream(labels, sensor_mm, depth, sizes, region_map, region_count, fusion_planes, fusion_scale, depth_fused,
                         depth_fused_mm, fused_source)), "gwd_fusion_depth")

    def line_profiles(self, lines, count, order, labels, depth_mm, sizes, region_map, intrinsics, offset, max_samples, lo_mm, hi_mm,
                      hi, lo, counts, fits, kind, line_points):
        """gwd_line_profiles: lines (B,C,4) float32 or float64, count (B,) int32, order (B,C) int32 or None, labels uint8 / depth_mm
        uint16 (B,Fh,Fw), sizes (B,2) int32, region_map uint8 (B,Fh,Fw) or None, intrinsics (B,4) float64 with line_points (B,C,2,3)
        float64, or both None; outputs counts (B,C,12) int32, fits (B,C,3,5) float64, kind (B,C) int32."""
        if lines.dtype not in (torch.float32, torch.float64):
            raise TypeError("gwd_line_profiles: lines must be float32 or float64, got %s" % lines.dtype)
        self._typed("gwd_line_profiles", ((count, torch.int32), (order, torch.int32), (labels, torch.uint8), (depth_mm, torch.uint16),
                                          (sizes, torch.int32), (region_map, torch.uint8), (intrinsics, torch.float64),
                                          (counts, torch.int32), (fits, torch.float64), (kind, torch.int32), (line_points, torch.float64)))
        B, Fh, Fw = labels.shape
        C = lines.shape[1] if lines.dim() == 3 else -1
        shape = (B, Fh, Fw)
        if tuple(lines.shape) != (B, C, 4) or count.numel() != B or (order is not None and tuple(order.shape) != (B, C)) \
                or tuple(depth_mm.shape) != shape or tuple(sizes.shape) != (B, 2) or (region_map is not None and tuple(region_map.shape) != shape) \
                or (intrinsics is None) != (line_points is None) or (intrinsics is not None and tuple(intrinsics.shape) != (B, 4)) \
                or (line_points is not None and tuple(line_points.shape) != (B, C, 2, 3)) or tuple(counts.shape) != (B, C, PROFILE_COUNTS) \
                or tuple(fits.shape) != (B, C, 3, 5) or tuple(kind.shape) != (B, C):
            raise ValueError("gwd_line_profiles: operand sizes do not match (B, C, Fh, Fw) = (%d, %d, %d, %d)" % (B, C, Fh, Fw))
        self._check(self.lib.gwd_line_profiles(
            _ptr(lines), 1 if lines.dtype == torch.float64 else 0, _ptr(count), _ptr(order), _ptr(labels), _ptr(depth_mm), _ptr(sizes),
            _ptr(region_map), _ptr(intrinsics), B, C, Fh, Fw, float(offset), int(max_samples), int(lo_mm), int(hi_mm), int(hi), int(lo),
            _ptr(counts), _ptr(fits), _ptr(kind), _ptr(line_points),
            self._stream(lines, count, order, labels, depth_mm, sizes, region_map, intrinsics, counts, fits, kind, line_points)),
            "gwd_line_profiles")

    @staticmethod
    def render_desc(canvas, sizes, tables, panels, frames, planes, label_planes, region_map, lines, count, order, scores, kinds, opts):
        """The gwd_render_desc of a call (no device work): every operand per frame, with its row pitch; ext = what the operands of a
        frame cover.  Raises on a dtype, a layout or a size the kernel does not take."""
        HipLibrary._typed("gwd_render_frames", ((canvas, torch.uint8), (sizes, torch.int32), (tables, torch.uint8), (count, torch.int32),
                                                (order, torch.int32), (kinds, torch.int32)))
        if canvas.dim() != 5 or canvas.shape[4] != 3 or not canvas.is_contiguous():
            raise ValueError("gwd_render_frames: canvas must be a contiguous (B, P, Fh, Fw, 3) tensor")
        B, P, Fh, Fw = canvas.shape[:4]
        if not 1 <= B <= 16 or P != len(panels) or not 1 <= P <= RENDER_MAX_PANELS or tuple(sizes.shape) != (B, 2) or tables.dim() != 3 \
                or tuple(tables.shape[1:]) != (256, 3) or not 1 <= tables.shape[0] <= RENDER_MAX_TABLES or len(planes) > RENDER_MAX_PLANES \
                or len(label_planes) > RENDER_MAX_PLANES:
            raise ValueError("gwd_render_frames: operand sizes do not match (B, P, Fh, Fw) = (%d, %d, %d, %d)" % (B, P, Fh, Fw))
        d = RenderDesc()
        d.canvas, d.sizes, d.tables = canvas.data_ptr(), _ptr(sizes).value, _ptr(tables).value
        d.B, d.P, d.Fh, d.Fw, d.n_planes, d.n_label_planes, d.n_tables = B, P, Fh, Fw, len(planes), len(label_planes), tables.shape[0]
        ext = [[Fh, Fw] for _ in range(B)]

        def fill(slot, views, dtype, what, channels=None):
            if len(views) != B:
                raise ValueError("gwd_render_frames: %s must hold one view per frame (%d), got %d" % (what, B, len(views)))
            for b, t in enumerate(views):
                ok = t.dtype == dtype and t.dim() == (2 if channels is None else 3) and 0 not in t.shape and t.stride(0) < 2 ** 31
                ok = ok and (t.stride(1) == 1 if channels is None else (t.shape[2] == channels and t.stride(2) == 1 and t.stride(1) == channels))
                if not ok or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * (channels or 1)):
                    raise ValueError("gwd_render_frames: %s[%d] must be a %s %s view with dense rows, got %s %s strides %s"
                                     % (what, b, dtype, "(h, w)" if channels is None else "(h, w, %d)" % channels, t.dtype, tuple(t.shape), t.stride()))
                slot.ptr[b], slot.pitch[b] = t.data_ptr(), max(t.stride(0), 1)
                ext[b] = [min(ext[b][0], t.shape[0]), min(ext[b][1], t.shape[1])]

        if frames is not None:
            fill(d.frames, frames, torch.uint8, "frames", 3)
            d.has_frames = 1
        if region_map is not None:
            fill(d.region_map, region_map, torch.uint8, "region_map")
            d.has_region_map = 1
        for i, views in enumerate(planes):
            fill(d.planes[i], views, torch.uint16, "planes[%d]" % i)
        for i, views in enumerate(label_planes):
            fill(d.label_planes[i], views, torch.uint8, "label_planes[%d]" % i)
        for b in range(B):
            d.ext_h[b], d.ext_w[b] = ext[b]
        for k, r in enumerate(panels):
            pn = d.panels[k]
            for n in ("base", "plane", "table", "lo_mm", "hi_mm", "tint", "tint_alpha", "outlines", "region_table", "lines", "line_table", "ends"):
                setattr(pn, n, int(r[n]))
            for n, key in (("void_rgb", "void"), ("tint_rgb", "tint_rgb"), ("line_rgb", "line_rgb"), ("end_rgb", "end_rgb")):
                getattr(pn, n)[:3] = [int(v) for v in r[key]]
        if lines is not None:
            if lines.dtype not in (torch.float32, torch.float64) or (scores is not None and scores.dtype not in (torch.float32, torch.float64)):
                raise TypeError("gwd_render_frames: lines and scores must be float32 or float64")
            C = lines.shape[1] if lines.dim() == 3 else -1
            if tuple(lines.shape) != (B, C, 4) or not 1 <= C <= PROFILE_MAX_LINES or count is None or count.numel() != B \
                    or any(t is not None and tuple(t.shape) != (B, C) for t in (order, scores, kinds)):
                raise ValueError("gwd_render_frames: line operands do not match (B, C) = (%d, %d)" % (B, C))
            d.lines, d.count, d.order, d.scores, d.kinds = (None if t is None else _ptr(t).value for t in (lines, count, order, scores, kinds))
            d.C, d.lines_dtype = C, 1 if lines.dtype == torch.float64 else 0
            d.scores_dtype = 1 if scores is not None and scores.dtype == torch.float64 else 0
        elif any(t is not None for t in (count, order, scores, kinds)):
            raise ValueError("gwd_render_frames: count, order, scores and kinds belong to lines")
        d.width8, d.end_radius = int(opts["width8"]), int(opts["end_radius"])
        d.min_score, d.score_lo, d.score_k = float(opts["min_score"]), float(opts["score_lo"]), float(opts["score_k"])
        return d

    def render_frames(self, canvas, sizes, tables, panels, frames, planes, label_planes, region_map, lines, count, order, scores, kinds, opts):
        """gwd_render_frames: canvas (B,P,Fh,Fw,3) uint8 out, every byte written.  sizes (B,2) int32, tables (T,256,3) uint8, panels:
        the records of render.resolve; frames: None or B uint8 (h,w,3) views; planes / label_planes: lists of B-lists of uint16 / uint8
        (h,w) views with unit column stride (any row pitch); region_map: None or a B-list; lines (B,C,4) float32 / float64 with count
        (B,), order / scores / kinds (B,C) or None; opts: width8, end_radius, min_score, score_lo, score_k."""
        d = self.render_desc(canvas, sizes, tables, panels, frames, planes, label_planes, region_map, lines, count, order, scores, kinds, opts)
        every = [canvas, sizes, tables, lines, count, order, scores, kinds] + list(frames or []) + list(region_map or []) + \
            [t for views in list(planes) + list(label_planes) for t in views]
        self._check(self.lib.gwd_render_frames(ctypes.byref(d), self._stream(*every)), "gwd_render_frames")

    @staticmethod
    def cloud_desc(depth, labels, sizes, intrinsics, frames, region_map, region_count, planes, source, poses, frame_sizes, stride,
                   min_depth, max_depth, edge, normals, keep, workspace, cloud, cloud_offsets):
        """The gwd_cloud_desc of a call (no device work).  ext = what the host knows of every frame: the plane, the image handed over
        for it and frame_sizes (None, or B (fh, fw) pairs).  Raises on a dtype, a layout or a size the kernels do not take."""
        HipLibrary._typed("gwd_point_cloud", ((depth, torch.float32), (labels, torch.uint8), (sizes, torch.int32),
                                              (intrinsics, torch.float64), (region_map, torch.uint8), (region_count, torch.int32),
                                              (planes, torch.float64), (source, torch.uint8), (poses, torch.float64),
                                              (workspace, torch.uint8), (cloud, torch.uint8), (cloud_offsets, torch.int32)))
        if depth.dim() != 3:
            raise ValueError("gwd_point_cloud: depth must be (B, Fh, Fw)")
        B, Fh, Fw = depth.shape
        shape = (B, Fh, Fw)
        R = planes.shape[1] if planes is not None and planes.dim() == 3 else 0
        if not 1 <= B <= 16 or tuple(labels.shape) != shape or tuple(sizes.shape) != (B, 2) or tuple(intrinsics.shape) != (B, 4) \
                or any(t is not None and tuple(t.shape) != shape for t in (region_map, source)) \
                or len({t is None for t in (region_map, region_count, planes)}) != 1 \
                or (planes is not None and (tuple(planes.shape) != (B, R, 6) or region_count.numel() != B)) \
                or (poses is not None and tuple(poses.shape) != (B, 3, 4)) or cloud.dim() != 2 or cloud.shape[1] != CLOUD_RECORD \
                or cloud_offsets.numel() != B + 1 or (frame_sizes is not None and len(frame_sizes) != B) \
                or not 1 <= int(stride) <= CLOUD_MAX_STRIDE:
            raise ValueError("gwd_point_cloud: operand sizes do not match (B, Fh, Fw) = (%d, %d, %d)" % shape)
        d = CloudDesc()
        for n, t in (("depth", depth), ("labels", labels), ("sizes", sizes), ("intrinsics", intrinsics), ("region_map", region_map),
                     ("region_count", region_count), ("planes", planes), ("source", source), ("poses", poses), ("workspace", workspace),
                     ("cloud", cloud), ("cloud_offsets", cloud_offsets)):
            setattr(d, n, None if t is None else _ptr(t).value)
        d.min_depth, d.max_depth, d.edge = float(min_depth), float(max_depth), 0.0 if edge is None else float(edge)
        d.capacity = cloud.shape[0]
        d.B, d.Fh, d.Fw, d.max_regions, d.stride, d.normals, d.keep = B, Fh, Fw, R, int(stride), int(bool(normals)), CLOUD_KEEP[keep]
        for b in range(B):
            h, w = (Fh, Fw) if frame_sizes is None else (min(int(frame_sizes[b][0]), Fh), min(int(frame_sizes[b][1]), Fw))
            if frames is not None:
                t = frames[b]
                if t.dtype != torch.uint8 or t.dim() != 3 or 0 in t.shape or t.shape[2] != 3 or t.stride(2) != 1 or t.stride(1) != 3 \
                        or t.stride(0) >= 2 ** 31 or (t.shape[0] > 1 and t.stride(0) < 3 * t.shape[1]):
                    raise ValueError("gwd_point_cloud: frames[%d] must be a uint8 (h, w, 3) view with dense rows, got %s %s strides %s"
                                     % (b, t.dtype, tuple(t.shape), t.stride()))
                d.frames.ptr[b], d.frames.pitch[b] = t.data_ptr(), max(t.stride(0), 1)
                h, w = min(h, t.shape[0]), min(w, t.shape[1])
            if h < 1 or w < 1:
                raise ValueError("gwd_point_cloud: frame %d is empty (%d x %d)" % (b, h, w))
            d.ext_h[b], d.ext_w[b] = h, w
        d.has_frames = int(frames is not None)
        return d

    @staticmethod
    def cloud_worst_case(desc):
        """The points a call can yield at most: what its capacity must cover."""
        s = desc.stride
        return sum(-(-desc.ext_h[b] // s) * -(-desc.ext_w[b] // s) for b in range(desc.B))

    def point_cloud(self, depth, labels, sizes, intrinsics, frames, region_map, region_count, planes, source, poses, frame_sizes, stride,
                    min_depth, max_depth, edge, normals, keep, workspace, cloud, cloud_offsets):
        """gwd_point_cloud: cloud (capacity, 32) uint8 and cloud_offsets (B + 1,) int32 out, every byte written.  depth float32 /
        labels uint8 (B,Fh,Fw), sizes (B,2) int32, intrinsics (B,4) float64; frames: None or B uint8 (h,w,3) views; region_map uint8
        (B,Fh,Fw) with region_count (B,) int32 and planes (B,R,6) float64, or all None; source uint8 (B,Fh,Fw), poses (B,3,4) float64
        or None; frame_sizes: None or what the host knows of sizes; edge None or > 0; keep a key of CLOUD_KEEP; workspace: a uint8
        tensor of workspace_bytes(WS_CLOUD, B, Fh, Fw, stride) bytes."""
        d = self.cloud_desc(depth, labels, sizes, intrinsics, frames, region_map, region_count, planes, source, poses, frame_sizes, stride,
                            min_depth, max_depth, edge, normals, keep, workspace, cloud, cloud_offsets)
        if workspace.numel() < self.workspace_bytes(WS_CLOUD, d.B, d.Fh, d.Fw, d.stride):
            raise ValueError("gwd_point_cloud: the workspace is smaller than workspace_bytes(WS_CLOUD, B, Fh, Fw, stride)")
        if not self.cloud_worst_case(d) <= d.capacity <= 2 ** 31 - 1:
            raise ValueError("gwd_point_cloud: a capacity of %d rows does not cover the %d points these frames can yield (or exceeds "
                             "2^31 - 1)" % (d.capacity, self.cloud_worst_case(d)))
        every = [depth, labels, sizes, intrinsics, region_map, region_count, planes, source, poses, workspace, cloud, cloud_offsets] + \
            list(frames or [])
        self._check(self.lib.gwd_point_cloud(ctypes.byref(d), self._stream(*every)), "gwd_point_cloud")

    @staticmethod
    def scene_desc(keys, marks, ranks, voxels, state, voxel, origin):
        """The gwd_scene_desc of a map (no device work): keys / marks (slots,) int64, ranks (slots,) int32, voxels (max_voxels,
        SCENE_VOXEL_BYTES) uint8, state (8,) int64, all contiguous.  Raises on a dtype, a size or a parameter the kernels do not take."""
        HipLibrary._typed("gwd_scene", ((keys, torch.int64), (marks, torch.int64), (ranks, torch.int32), (voxels, torch.uint8),
                                        (state, torch.int64)))
        if any(t is None or not t.is_contiguous() for t in (keys, marks, ranks, voxels, state)):
            raise ValueError("gwd_scene: the map's five tensors are contiguous")
        slots = keys.numel()
        if keys.dim() != 1 or tuple(marks.shape) != (slots,) or tuple(ranks.shape) != (slots,) or voxels.dim() != 2 \
                or voxels.shape[1] != SCENE_VOXEL_BYTES or tuple(state.shape) != (8,):
            raise ValueError("gwd_scene: keys / marks / ranks are (slots,), voxels (max_voxels, %d), state (8,)" % SCENE_VOXEL_BYTES)
        max_voxels = voxels.shape[0]
        if not 1 <= max_voxels <= SCENE_MAX_VOXELS or slots <= max_voxels or slots > 2 * SCENE_MAX_VOXELS or slots & (slots - 1):
            raise ValueError("gwd_scene: 1 <= max_voxels <= 2^27 < slots, a power of two <= 2^28; got %d, %d" % (max_voxels, slots))
        voxel, origin = float(voxel), [float(v) for v in origin]
        if not 0.0 < voxel < float("inf") or len(origin) != 3 or not all(abs(v) < float("inf") for v in origin):
            raise ValueError("gwd_scene: voxel is finite and > 0, origin three finite numbers; got %r, %r" % (voxel, origin))
        d = SceneDesc()
        d.keys, d.marks, d.ranks, d.voxels, d.state = (_ptr(t).value for t in (keys, marks, ranks, voxels, state))
        d.voxel, d.max_voxels, d.slots = voxel, max_voxels, slots
        for k in range(3):
            d.origin[k] = origin[k]
        return d

    @staticmethod
    def scene_cloud_check(what, cloud, cloud_offsets):
        HipLibrary._typed(what, ((cloud, torch.uint8), (cloud_offsets, torch.int32)))
        if cloud is None or cloud_offsets is None or cloud.dim() != 2 or cloud.shape[1] != CLOUD_RECORD or cloud_offsets.dim() != 1 \
                or not cloud.is_contiguous() or not cloud_offsets.is_contiguous():
            raise ValueError("%s: cloud is a contiguous (rows, %d) uint8 tensor, cloud_offsets a contiguous int32 vector" % (what, CLOUD_RECORD))

    def scene_reset(self, desc, tensors):
        """gwd_scene_reset: desc of scene_desc, tensors the map's five (for the device check)."""
        self._check(self.lib.gwd_scene_reset(ctypes.byref(desc), self._stream(*tensors)), "gwd_scene_reset")

    def scene_integrate(self, desc, tensors, cloud, cloud_offsets, workspace):
        """gwd_scene_integrate: cloud (rows >= 1, 32) uint8 and cloud_offsets (>= 2,) int32 of point_cloud (or of an extraction) into
        the map; workspace: a uint8 tensor of workspace_bytes(WS_SCENE, rows, max_voxels) bytes."""
        self.scene_cloud_check("gwd_scene_integrate", cloud, cloud_offsets)
        if cloud.shape[0] < 1 or cloud.shape[0] > 2 ** 31 - 1 or cloud_offsets.numel() < 2:
            raise ValueError("gwd_scene_integrate: 1 <= rows <= 2^31 - 1 and at least two offsets, got %d, %d" % (cloud.shape[0], cloud_offsets.numel()))
        if workspace.numel() < self.workspace_bytes(WS_SCENE, cloud.shape[0], desc.max_voxels):
            raise ValueError("gwd_scene_integrate: the workspace is smaller than workspace_bytes(WS_SCENE, rows, max_voxels)")
        self._check(self.lib.gwd_scene_integrate(ctypes.byref(desc), _ptr(cloud), _ptr(cloud_offsets), cloud.shape[0], cloud_offsets.numel(),
                                                 _ptr(workspace), self._stream(cloud, cloud_offsets, workspace, *tensors)), "gwd_scene_integrate")

    def scene_extract(self, desc, tensors, min_obs, keep, workspace, cloud, cloud_offsets, voxel_stats):
        """gwd_scene_extract: cloud (max_voxels, 32) uint8, cloud_offsets (2,) int32 and voxel_stats (max_voxels, 4) int32 out, every
        byte written; keep a key of CLOUD_KEEP; workspace as for scene_integrate (any rows)."""
        self.scene_cloud_check("gwd_scene_extract", cloud, cloud_offsets)
        self._typed("gwd_scene_extract", ((voxel_stats, torch.int32),))
        if cloud.shape[0] != desc.max_voxels or cloud_offsets.numel() != 2 or tuple(voxel_stats.shape) != (desc.max_voxels, 4) \
                or not voxel_stats.is_contiguous() or not 1 <= int(min_obs) <= 2 ** 31 - 1:
            raise ValueError("gwd_scene_extract: cloud (max_voxels, 32), cloud_offsets (2,), voxel_stats (max_voxels, 4), min_obs >= 1")
        if workspace.numel() < self.workspace_bytes(WS_SCENE, 1, desc.max_voxels):
            raise ValueError("gwd_scene_extract: the workspace is smaller than workspace_bytes(WS_SCENE, 1, max_voxels)")
        self._check(self.lib.gwd_scene_extract(ctypes.byref(desc), int(min_obs), CLOUD_KEEP[keep], _ptr(workspace), _ptr(cloud),
                                               _ptr(cloud_offsets), _ptr(voxel_stats),
                                               self._stream(workspace, cloud, cloud_offsets, voxel_stats, *tensors)), "gwd_scene_extract")

    @staticmethod
    def view_desc(cloud, cloud_offsets, sizes, intrinsics, poses, view_sizes, min_depth, max_depth, footprint, max_splat, keep, workspace,
                  view_depth, view_index, view_labels, view_rgb):
        """The gwd_view_desc of a call (no device work).  ext = what the host knows of every view: the plane and view_sizes (None, or V
        (fh, fw) pairs).  Raises on a dtype, a layout, a size or an option the kernels do not take."""
        HipLibrary.scene_cloud_check("gwd_cloud_view", cloud, cloud_offsets)
        HipLibrary._typed("gwd_cloud_view", ((sizes, torch.int32), (intrinsics, torch.float64), (poses, torch.float64),
                                             (workspace, torch.uint8), (view_depth, torch.float32), (view_index, torch.int32),
                                             (view_labels, torch.uint8), (view_rgb, torch.uint8)))
        if any(t is None for t in (sizes, intrinsics, workspace, view_depth, view_index, view_labels, view_rgb)) or view_depth.dim() != 3:
            raise ValueError("gwd_cloud_view: view_depth must be (V, Fh, Fw), and only poses may be None")
        V, Fh, Fw = view_depth.shape
        shape = (V, Fh, Fw)
        if not 1 <= V <= VIEW_MAX_VIEWS or not 1 <= Fh <= 16384 or not 1 <= Fw <= 16384 or tuple(view_index.shape) != shape \
                or tuple(view_labels.shape) != shape or tuple(view_rgb.shape) != shape + (3,) or tuple(sizes.shape) != (V, 2) \
                or tuple(intrinsics.shape) != (V, 4) or (poses is not None and tuple(poses.shape) != (V, 3, 4)) \
                or (view_sizes is not None and len(view_sizes) != V) or not 1 <= cloud.shape[0] <= 2 ** 31 - 1 or cloud_offsets.numel() < 2:
            raise ValueError("gwd_cloud_view: operand sizes do not match (V, Fh, Fw) = (%d, %d, %d), V <= %d, sides <= 16384, 1 <= rows "
                             "<= 2^31 - 1, at least two offsets" % (shape + (VIEW_MAX_VIEWS,)))
        if any(t is not None and not t.is_contiguous() for t in (sizes, intrinsics, poses, workspace, view_depth, view_index, view_labels,
                                                                 view_rgb)):
            raise ValueError("gwd_cloud_view: every operand is contiguous")
        if isinstance(max_splat, bool) or int(max_splat) != max_splat or not 1 <= int(max_splat) <= VIEW_MAX_SPLAT or keep not in CLOUD_KEEP:
            raise ValueError("gwd_cloud_view: 1 <= max_splat <= %d and keep one of %s, got %r, %r" % (VIEW_MAX_SPLAT, sorted(CLOUD_KEEP), max_splat, keep))
        min_depth, max_depth, footprint = float(min_depth), float(max_depth), float(footprint)
        if not 0.0 < min_depth <= max_depth < float("inf") or not 0.0 <= footprint < float("inf"):
            raise ValueError("gwd_cloud_view: 0 < min_depth <= max_depth and footprint >= 0, all finite; got %r, %r, %r" % (min_depth, max_depth, footprint))
        d = ViewDesc()
        for n, t in (("cloud", cloud), ("cloud_offsets", cloud_offsets), ("sizes", sizes), ("intrinsics", intrinsics), ("poses", poses),
                     ("workspace", workspace), ("view_depth", view_depth), ("view_index", view_index), ("view_labels", view_labels),
                     ("view_rgb", view_rgb)):
            setattr(d, n, None if t is None else _ptr(t).value)
        d.min_depth, d.max_depth, d.footprint = min_depth, max_depth, footprint
        d.rows, d.n_offsets, d.V, d.Fh, d.Fw, d.max_splat, d.keep = cloud.shape[0], cloud_offsets.numel(), V, Fh, Fw, int(max_splat), CLOUD_KEEP[keep]
        for v in range(V):
            h, w = (Fh, Fw) if view_sizes is None else (min(int(view_sizes[v][0]), Fh), min(int(view_sizes[v][1]), Fw))
            if h < 1 or w < 1:
                raise ValueError("gwd_cloud_view: view %d is empty (%d x %d)" % (v, h, w))
            d.ext_h[v], d.ext_w[v] = h, w
        return d

    def cloud_view(self, cloud, cloud_offsets, sizes, intrinsics, poses, view_sizes, min_depth, max_depth, footprint, max_splat, keep,
                   workspace, view_depth, view_index, view_labels, view_rgb):
        """gwd_cloud_view: view_depth float32 / view_index int32 / view_labels uint8 (V,Fh,Fw) and view_rgb uint8 (V,Fh,Fw,3) out, every
        byte written.  cloud (rows >= 1, 32) uint8 with cloud_offsets (>= 2,) int32, sizes (V,2) int32, intrinsics (V,4) float64, poses
        (V,3,4) float64 camera-to-world or None; view_sizes: None or what the host knows of sizes; keep a key of CLOUD_KEEP; workspace:
        a uint8 tensor of workspace_bytes(WS_VIEW, V, Fh, Fw) bytes."""
        d = self.view_desc(cloud, cloud_offsets, sizes, intrinsics, poses, view_sizes, min_depth, max_depth, footprint, max_splat, keep,
                           workspace, view_depth, view_index, view_labels, view_rgb)
        if workspace.numel() < self.workspace_bytes(WS_VIEW, d.V, d.Fh, d.Fw):
            raise ValueError("gwd_cloud_view: the workspace is smaller than workspace_bytes(WS_VIEW, V, Fh, Fw)")
        every = (cloud, cloud_offsets, sizes, intrinsics, poses, workspace, view_depth, view_index, view_labels, view_rgb)
        self._check(self.lib.gwd_cloud_view(ctypes.byref(d), self._stream(*every)), "gwd_cloud_view")


_LIB = None


def library():
    """The process-wide device library; raises HipUnavailable when it cannot be loaded."""
    global _LIB
    if _LIB is None:
        _LIB = HipLibrary()
    return _LIB


def set_library(lib):
    """TEST HOOK: install a stand-in device library (tests/fake_device.py) or None to reset."""
    global _LIB
    _LIB = lib
