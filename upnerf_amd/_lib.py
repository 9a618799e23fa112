"""ctypes binding of libupnerf_hip.so (C ABI: include/upnerf_hip.h).

The product path has no CPU or PyTorch fallback: if the shared library is missing or does not export every
entry point, importing this module raises, loudly.  Build it with `python __graft_entry__.py` (or
`make -C upnerf_amd/csrc`)."""
from __future__ import annotations

import ctypes as C
import os

import torch

from .pass_plan import (AUXK, CK, RR_PART_STRIDE, TILE_PART_STRIDE, WG_F16_FRAG, WG_F16_TILE, WG_F24, WG_F32,  # noqa: F401
                        WG_PLANES, X0)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UPNERF_LIB") or os.path.join(_HERE, "libupnerf_hip.so")  # UPNERF_LIB: diagnostic builds only
MAX_D = 8

_fp = C.c_void_p


class Layout(C.Structure):
    _fields_ = [("W", C.c_int32), ("D", C.c_int32), ("skip", C.c_int32),
                ("w", C.c_int32 * MAX_D), ("b", C.c_int32 * MAX_D),
                ("we", C.c_int32), ("be", C.c_int32), ("wsig", C.c_int32), ("bsig", C.c_int32),
                ("wc1", C.c_int32), ("bc1", C.c_int32), ("wc2", C.c_int32), ("bc2", C.c_int32),
                ("wcsig", C.c_int32), ("bcsig", C.c_int32), ("wr1", C.c_int32), ("br1", C.c_int32),
                ("wr2", C.c_int32), ("br2", C.c_int32), ("total", C.c_int32),
                ("t_w", C.c_int32 * MAX_D), ("t_skipx", C.c_int32), ("t_we", C.c_int32), ("t_head", C.c_int32),
                ("t_wc2", C.c_int32), ("t_total", C.c_int32)]


class FieldFwdArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("S", C.c_int32), ("use_cand", C.c_int32), ("use_rgb", C.c_int32),
                ("rays_o", _fp), ("rays_d", _fp), ("z", _fp), ("c_rows", _fp), ("aux", _fp),
                ("wk_xyz", C.c_float * 10), ("P", _fp),
                ("sigma_s", _fp), ("sigma_c", _fp), ("rgb", _fp),
                ("x0", _fp), ("h", _fp), ("hmask", _fp), ("amax", _fp), ("e", _fp), ("g1", _fp), ("g2", _fp), ("r1", _fp),
                ("P16", _fp), ("wexp", _fp), ("wk_xyz_dev", _fp), ("planes", C.c_int32), ("tile_rows", C.c_int32), ("wnorm", _fp),
                ("h16", _fp), ("hexp", _fp), ("h_last_only", C.c_int32), ("x0f", _fp), ("e16", _fp), ("eexp", _fp),
                ("g2_16", _fp), ("g2exp", _fp), ("r1_16", _fp), ("r1exp", _fp), ("g1_16", _fp), ("g1exp", _fp), ("h_lo8", _fp),
                ("rows_capacity", C.c_int64)]


class CompositeFwdArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("S", C.c_int32), ("W", C.c_int32), ("mode", C.c_int32),
                ("z", _fp), ("sigma_s", _fp), ("sigma_c", _fp), ("rgb", _fp), ("has_rgb", C.c_int32),
                ("e", _fp), ("g2", _fp),
                ("w_all", _fp), ("w_sj", _fp), ("w_cj", _fp), ("w_s", _fp),
                ("E_s", _fp), ("G_c", _fp), ("sum_sfeat", _fp), ("t_weight", _fp), ("c_depth", _fp),
                ("s_depth", _fp), ("rgb_map", _fp), ("e16", _fp), ("eexp", _fp), ("g2_16", _fp), ("g2exp", _fp),
                ("rgb_joint_map", _fp)]


class CompositeBwdArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("S", C.c_int32), ("W", C.c_int32), ("mode", C.c_int32), ("has_rgb", C.c_int32),
                ("z", _fp), ("sigma_s", _fp), ("sigma_c", _fp), ("rgb", _fp), ("e", _fp), ("g2", _fp),
                ("w_all", _fp), ("w_sj", _fp), ("w_cj", _fp), ("w_s", _fp),
                ("g_E_s", _fp), ("g_G_c", _fp), ("g_sum_sfeat", _fp), ("g_t_weight", _fp), ("g_c_depth", _fp),
                ("g_s_depth", _fp), ("g_rgb_map", _fp), ("g_w_all", _fp), ("g_w_s", _fp),
                ("d_sigma_s", _fp), ("d_sigma_c", _fp), ("d_rgb", _fp), ("e16", _fp), ("eexp", _fp), ("g2_16", _fp), ("g2exp", _fp),
                ("g_rgb_joint_map", _fp)]


class FieldBwdArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("S", C.c_int32), ("use_cand", C.c_int32), ("use_rgb", C.c_int32),
                ("need_dxyz", C.c_int32),
                ("PT", _fp), ("P", _fp),
                ("d_sigma_s", _fp), ("d_sigma_c", _fp), ("d_rgb", _fp),
                ("sigma_s", _fp), ("sigma_c", _fp), ("rgb", _fp),
                ("w_feat_s", _fp), ("w_cj", _fp), ("g_E_s", _fp), ("g_G_c", _fp),
                ("x0", _fp), ("h", _fp), ("g1", _fp), ("g2", _fp), ("r1", _fp), ("hmask", _fp), ("gmax", _fp),
                ("gz_h", _fp), ("gz_e", _fp), ("gz_g1", _fp), ("gz_g2", _fp), ("gz_r1", _fp),
                ("dpre_sig_s", _fp), ("dpre_sig_c", _fp), ("dpre_rgb", _fp), ("dxyz", _fp),
                ("PT16", _fp), ("wexp", _fp), ("planes", C.c_int32), ("tile_rows", C.c_int32), ("gz16", _fp), ("gzexp", _fp), ("xs", _fp), ("tile_part", _fp), ("gz_rg_ld", C.c_int32), ("reserved_", C.c_int32), ("wnorm", _fp),
                ("gz_rg16", _fp), ("gzrgexp", _fp), ("gz_g2_16", _fp), ("gzg2exp", _fp), ("gz_lo8", _fp),
                ("rows_capacity", C.c_int64)]


class LossArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("F", C.c_int32), ("fine", C.c_int32), ("has_tw", C.c_int32),
                ("sched", C.c_float), ("depth_mult", C.c_float), ("alpha_reg", C.c_float), ("near", C.c_float),
                ("far", C.c_float),
                ("depth_direct", _fp), ("inv_depth", _fp), ("depth_scale_rows", _fp),
                ("s_depth_c", _fp), ("s_depth_f", _fp), ("t_weight_c", _fp), ("t_weight_f", _fp),
                ("feat_c", _fp), ("feat_f", _fp), ("feat_gt", _fp),
                ("rgb_c", _fp), ("rgb_f", _fp), ("rgb_gt", _fp), ("beta", _fp), ("alpha", _fp), ("sched_dev", _fp),
                ("term_mask", C.c_int32), ("reserved_", C.c_int32), ("total", _fp), ("g_total", _fp)]


class LossGrads(C.Structure):
    _fields_ = [("d_depth_scale_rows", _fp), ("d_depth", _fp), ("d_s_depth_c", _fp), ("d_s_depth_f", _fp),
                ("d_feat_c", _fp), ("d_feat_f", _fp), ("d_rgb_c", _fp), ("d_rgb_f", _fp), ("d_beta", _fp),
                ("d_alpha", _fp)]


class FragDesc(C.Structure):
    _fields_ = [("src_off", C.c_int32), ("src_ld", C.c_int32), ("transpose", C.c_int32), ("rows", C.c_int32),
                ("cols", C.c_int32), ("dst_off", C.c_int32), ("dst_kp", C.c_int32), ("dst_k0", C.c_int32)]


class PackDesc(C.Structure):
    _fields_ = [("ptr", _fp), ("rows", C.c_int32), ("cols", C.c_int32), ("src_ld", C.c_int32), ("dst_off", C.c_int32),
                ("dst_ld", C.c_int32), ("accumulate", C.c_int32)]


class TransientArgs(C.Structure):
    _fields_ = ([("R", C.c_int32), ("beta_min", C.c_float), ("feat", _fp), ("t_emb", _fp)]
                + [(n, _fp) for n in ("w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3", "wf", "bf", "wt", "bt", "wa", "ba", "wb", "bb",
                                      "wr", "br", "h", "e", "t", "alpha", "rgb", "beta", "spre")])


class TransientGrads(C.Structure):
    _fields_ = [(n, _fp) for n in ("d_alpha", "d_rgb", "d_beta", "dz_heads", "gz_t", "gz_e", "gz_h", "g_temb", "g_feat")]


class AdamDesc(C.Structure):
    _fields_ = [("g", _fp), ("off", C.c_int32), ("n", C.c_int32)]


MAX_ADAM_DESC = 96


class WgradPending(C.Structure):
    _fields_ = [("slabs", _fp), ("bslabs", _fp), ("dW", _fp), ("db", _fp), ("N", C.c_int32), ("K", C.c_int32), ("TN", C.c_int32),
                ("TK", C.c_int32), ("nsplit", C.c_int32), ("ldo", C.c_int32), ("rblocks", C.c_int32), ("n2", C.c_int32),
                ("dW2", _fp), ("db2", _fp), ("ldo2", C.c_int32), ("pad", C.c_int32), ("vslabs", _fp), ("dv", _fp), ("dbv", _fp)]


class WgradOperand(C.Structure):
    _fields_ = [("p", _fp), ("lo", _fp), ("exp", _fp), ("ld", C.c_int32), ("kind", C.c_int32)]


class WgradDesc(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("planes", C.c_int32), ("A", WgradOperand), ("B", WgradOperand),
                ("expo_a", _fp), ("expo_b", _fp), ("dW", _fp), ("db", _fp), ("ldo", C.c_int32), ("n2", C.c_int32), ("dW2", _fp),
                ("db2", _fp), ("ldo2", C.c_int32), ("nsplit", C.c_int32), ("v", _fp), ("dv", _fp), ("dbv", _fp), ("slabs", _fp)]


class WgradGroup(C.Structure):
    _fields_ = [("A", _fp), ("B", _fp), ("dW", _fp), ("db", _fp), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int32), ("ldb", C.c_int32), ("ldo", C.c_int32)]


MAX_WGRAD_GROUPS = 32


class EmbedGroup(C.Structure):
    _fields_ = [("g", _fp), ("out", _fp), ("dim", C.c_int32)]


class EmbedRowsGroup(C.Structure):
    _fields_ = [("table", _fp), ("rows", _fp), ("dim", C.c_int32)]


MAX_EMBED_GROUPS = 8


class GatherRaysArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("h", C.c_int32), ("C", C.c_int32), ("idx", _fp),
                ("all_ray_infos", _fp), ("all_directions", _fp), ("all_rgbs", _fp), ("all_pxl_coords", _fp),
                ("all_inv_depths", _fp), ("feat_maps", _fp), ("poses", _fp),
                ("ray_infos", _fp), ("directions", _fp), ("img_idx", _fp), ("c2w", _fp), ("rgbs", _fp), ("feats", _fp),
                ("inv_depths", _fp)]


class Frag16Desc(C.Structure):
    _fields_ = FragDesc._fields_ + [("exp_id", C.c_int32)]


class AddPair(C.Structure):
    _fields_ = [("a", _fp), ("b", _fp), ("out", _fp), ("n", C.c_int32)]


MAX_ADD_PAIRS = 8


class SsimArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pred", _fp), ("gt", _fp),
                ("pred_stride", C.c_int64 * 4), ("gt_stride", C.c_int64 * 4), ("ssim", _fp), ("map", _fp)]


class Conv2dArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C_in", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C_out", C.c_int32),
                ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("relu", C.c_int32), ("scale_in", C.c_int32),
                ("x", _fp), ("x_stride", C.c_int64 * 4), ("w", _fp), ("bias", _fp), ("y", _fp)]


class Maxpool2dArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("x", _fp), ("y", _fp)]


class LpipsDistArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("accumulate", C.c_int32),
                ("reserved_", C.c_int32), ("feat", _fp), ("w", _fp), ("out", _fp)]


class LpipsScratchArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("reserved_", C.c_int32),
                ("act0_elems", C.c_int64), ("act1_elems", C.c_int64), ("part_elems", C.c_int64)]


class VitPatchesArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("stride", C.c_int32), ("u8", C.c_int32), ("image", _fp),
                ("mean", C.c_float * 3), ("std", C.c_float * 3), ("rows", _fp)]


class VitAttentionArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32), ("reserved_", C.c_int32),
                ("q", _fp), ("k", _fp), ("v", _fp), ("ldq", C.c_int64), ("ldk", C.c_int64), ("ldv", C.c_int64),
                ("scale", C.c_float), ("reserved2_", C.c_float), ("out", _fp), ("ldo", C.c_int64)]


class PcaFitArgs(C.Structure):
    _fields_ = [("T", C.c_int32), ("D", C.c_int32), ("x", _fp), ("ldx", C.c_int64), ("mean", _fp), ("gram", _fp)]


class Conv3x3Args(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("C_in", C.c_int32), ("C_out", C.c_int32), ("stride", C.c_int32),
                ("pre_relu", C.c_int32), ("relu", C.c_int32), ("reserved_", C.c_int32), ("x", _fp), ("ldx", C.c_int64), ("w", _fp),
                ("bias", _fp), ("res", _fp), ("ldr", C.c_int64), ("y", _fp), ("ldy", C.c_int64)]


class Upsample2xArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("reserved_", C.c_int32), ("x", _fp), ("ldx", C.c_int64),
                ("y", _fp), ("ldy", C.c_int64)]


class DepthToSpaceArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("s", C.c_int32), ("x", _fp), ("ldx", C.c_int64),
                ("bias", _fp), ("y", _fp), ("ldy", C.c_int64)]


class ResizeCubicArgs(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("u8", C.c_int32),
                ("affine", C.c_int32), ("reserved_", C.c_int32), ("x", _fp), ("mean", C.c_float * 3), ("std", C.c_float * 3),
                ("y", _fp)]


class VitPatches16Args(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("patch", C.c_int32), ("reserved_", C.c_int32), ("image", _fp), ("rows", _fp)]


class SceneImage(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("x0", C.c_int32), ("x1", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("near", C.c_float), ("far", C.c_float), ("img_idx", C.c_float), ("reserved_", C.c_int32),
                ("row0", C.c_int64), ("pix_off", C.c_int64)]


class SceneRaysArgs(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("reserved_", C.c_int32), ("rows", C.c_int64), ("pix_bytes", C.c_int64),
                ("pixels", _fp), ("directions", _fp), ("ray_infos", _fp), ("pxl", _fp), ("rgbs", _fp)]


class ResizeMap(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("src_off", C.c_int64),
                ("dst_off", C.c_int64), ("scale", C.c_float), ("bias", C.c_float), ("reserved_", C.c_int32 * 2)]


class ResizeArgs(C.Structure):
    _fields_ = [("n_maps", C.c_int32), ("C", C.c_int32), ("pre", C.c_int32), ("reserved_", C.c_int32),
                ("src_elems", C.c_int64), ("dst_elems", C.c_int64), ("src", _fp), ("dst", _fp)]


RESIZE_PLAIN, RESIZE_L2, RESIZE_INVDEPTH = 0, 1, 2  # UPNERF_RESIZE_*


class VizDepthArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("pre", C.c_int32), ("range", C.c_int32), ("x", _fp), ("x_stride", C.c_int64),
                ("depth_scale", _fp), ("inv_far", C.c_float), ("near", C.c_float), ("mi", C.c_float), ("ma", C.c_float),
                ("range_dev", _fp), ("lut", _fp), ("rgb", _fp), ("index", _fp), ("value", _fp)]


class VizPcaArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("F", C.c_int32), ("reserved_", C.c_int32), ("feat", _fp),
                ("feat_ld", C.c_int64), ("m", _fp), ("c", _fp), ("img", _fp), ("rgb", _fp)]


class VizRgbArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("reserved_", C.c_int32), ("x", _fp),
                ("stride", C.c_int64), ("cstride", C.c_int64), ("rgb", _fp)]


VIZ_RANGE_OWN, VIZ_RANGE_HOST, VIZ_RANGE_DEVICE = 0, 1, 2  # UPNERF_VIZ_RANGE_*
VIZ_PLAIN, VIZ_PRED_DEPTH = 0, 1  # UPNERF_VIZ_PLAIN / UPNERF_VIZ_PRED_DEPTH


PATH_LINEAR, PATH_CATMULL = 0, 1  # UPNERF_PATH_*
PATH_MAX_TABLES, PATH_MAX_DIM = 4, 64  # UPNERF_PATH_MAX_*


class PathPosesArgs(C.Structure):
    _fields_ = [("K", C.c_int32), ("F", C.c_int32), ("mode", C.c_int32), ("reserved_", C.c_int32), ("key_c2w", _fp),
                ("key_nf", _fp), ("u", _fp), ("c2w", _fp), ("nf", _fp)]


class PathTable(C.Structure):
    _fields_ = [("table", _fp), ("dim", C.c_int32), ("n_rows", C.c_int32), ("out", _fp)]


class PathRaysArgs(C.Structure):
    _fields_ = [("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_tables", C.c_int32), ("row0", C.c_int64),
                ("R", C.c_int32), ("reserved_", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("c2w", _fp), ("nf", _fp), ("i0", _fp), ("i1", _fp), ("t", _fp), ("rays", _fp),
                ("tables", PathTable * PATH_MAX_TABLES)]


class GridColumnsArgs(C.Structure):
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32), ("S", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("col0", C.c_int64), ("count", C.c_int32), ("reserved_", C.c_int32), ("o", _fp), ("d", _fp),
                ("z", _fp)]


class MtetTables(C.Structure):
    _fields_ = [("tets", (C.c_int8 * 4) * 6), ("edges", (C.c_int8 * 3) * 7), ("tet_edges", (C.c_int8 * 2) * 6),
                ("tris", (C.c_int8 * 7) * 16), ("reserved_", C.c_int8 * 7)]


class MtetArgs(C.Structure):
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32), ("level", C.c_float), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("grid", _fp), ("tab", MtetTables), ("n_vertices", C.c_int32), ("n_faces", C.c_int32),
                ("cap_vertices", C.c_int32), ("cap_faces", C.c_int32), ("vertices", _fp), ("normals", _fp), ("faces", _fp),
                ("flags", C.c_int32), ("reserved2_", C.c_int32)]


MTET_SKIP_NONFINITE = 1  # UPNERF_MTET_SKIP_NONFINITE
TSDF_MAX_VIEWS = 8       # UPNERF_TSDF_MAX_VIEWS


class TsdfView(C.Structure):
    _fields_ = [("c2w", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("W", C.c_int32), ("H", C.c_int32), ("depth", _fp), ("opacity", _fp), ("rgb", _fp)]


class TsdfIntegrateArgs(C.Structure):
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32), ("n_views", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("trunc", C.c_float), ("min_opacity", C.c_float), ("weight_mode", C.c_int32),
                ("reserved_", C.c_int32), ("tsdf", _fp), ("weight", _fp), ("rgb", _fp), ("rgb_weight", _fp),
                ("views", TsdfView * TSDF_MAX_VIEWS)]


class TsdfSurfaceArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("min_weight", C.c_float), ("reserved_", C.c_int32), ("tsdf", _fp), ("weight", _fp), ("out", _fp)]


class TsdfSampleArgs(C.Structure):
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32), ("V", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("rgb", _fp), ("rgb_weight", _fp), ("points", _fp), ("out", _fp)]


class OccBuildArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("dilate", C.c_int32), ("level", C.c_float),
                ("reserved_", C.c_int32), ("grid", _fp), ("cells", _fp), ("words", _fp), ("scratch", _fp)]


class OccSpansArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("R", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("words", _fp), ("rays", _fp), ("t0", _fp), ("t1", _fp), ("hit", _fp)]


class OccCompactArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("n_tables", C.c_int32), ("hit", _fp), ("t0", _fp), ("t1", _fp), ("rays", _fp), ("rays_c", _fp),
                ("index", _fp), ("count", _fp), ("scratch", _fp), ("tables", PathTable * PATH_MAX_TABLES)]


class OccScatterArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("n_hit", C.c_int32), ("background", C.c_float), ("reserved_", C.c_int32), ("index", _fp),
                ("rays", _fp), ("rgb_c", _fp), ("depth_c", _fp), ("rgb", _fp), ("depth", _fp)]


class BakedRenderArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("R", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("step", C.c_float), ("background", C.c_float), ("stop", C.c_float), ("reserved_", C.c_int32),
                ("rgbs", _fp), ("words", _fp), ("rays", _fp), ("rgb", _fp), ("depth", _fp), ("opacity", _fp)]


class BakedPackArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("level", C.c_float), ("reserved_", C.c_int32), ("sigma", _fp), ("rgb", _fp), ("rgbs", _fp),
                ("kept", _fp)]


class BakedShRenderArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("R", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("step", C.c_float), ("background", C.c_float), ("stop", C.c_float), ("degree", C.c_int32),
                ("records", _fp), ("words", _fp), ("rays", _fp), ("rgb", _fp), ("depth", _fp), ("opacity", _fp)]


class ShAccumulateArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("nb", C.c_int32), ("first", C.c_int32), ("w", C.c_float * 9), ("reserved_", C.c_int32),
                ("rgb", _fp), ("acc", _fp)]


class BakedShPackArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("level", C.c_float), ("degree", C.c_int32), ("sigma", _fp), ("acc", _fp), ("records", _fp),
                ("kept", _fp)]


BRICK_POINTS = 9  # UPNERF_BRICK_POINTS: points per axis of a stored brick (its far faces included)


class BrickTableArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("reserved_", C.c_int32), ("words", _fp), ("slots", _fp),
                ("bricks", _fp), ("count", _fp), ("scratch", _fp)]


class BrickGatherArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("n_bricks", C.c_int32), ("E", C.c_int32),
                ("reserved_", C.c_int32), ("bricks", _fp), ("grid", _fp), ("pool", _fp)]


class BrickScatterArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("n_bricks", C.c_int32), ("E", C.c_int32),
                ("reserved_", C.c_int32), ("bricks", _fp), ("pool", _fp), ("grid", _fp)]


class BrickOccArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("n_bricks", C.c_int32), ("E", C.c_int32),
                ("sigma_offset", C.c_int32), ("slots", _fp), ("pool", _fp), ("words", _fp)]


class BrickColumnsArgs(C.Structure):
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32), ("S", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("line0", C.c_int64), ("count", C.c_int32), ("n_bricks", C.c_int32), ("bricks", _fp),
                ("o", _fp), ("d", _fp), ("z", _fp)]


class BakedSparseRenderArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("R", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("step", C.c_float), ("background", C.c_float), ("stop", C.c_float), ("degree", C.c_int32),
                ("pool", _fp), ("slots", _fp), ("words", _fp), ("rays", _fp), ("rgb", _fp), ("depth", _fp), ("opacity", _fp)]


class BakedRenderBwdArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("R", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("step", C.c_float), ("background", C.c_float), ("stop", C.c_float), ("degree", C.c_int32),
                ("points", _fp), ("words", _fp), ("rays", _fp), ("slots", _fp), ("g_rgb", _fp), ("g_depth", _fp), ("g_opacity", _fp),
                ("grad", _fp), ("grad_coef", _fp), ("grad_sigma", _fp)]


class BakedProjectArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("degree", C.c_int32), ("reserved_", C.c_int32), ("rgbs", _fp), ("sigma", _fp)]


class BakedSparseRenderBwdArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("R", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("step", C.c_float), ("background", C.c_float), ("stop", C.c_float), ("degree", C.c_int32),
                ("pool", _fp), ("slots", _fp), ("words", _fp), ("rays", _fp), ("g_rgb", _fp), ("g_depth", _fp), ("g_opacity", _fp),
                ("grad", _fp), ("grad_coef", _fp), ("grad_sigma", _fp)]


class BrickFaceSumArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("n_bricks", C.c_int32), ("F", C.c_int32),
                ("reserved_", C.c_int32), ("slots", _fp), ("bricks", _fp), ("data", _fp)]


class BakedRayBwdArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("R", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("step", C.c_float), ("background", C.c_float), ("stop", C.c_float), ("degree", C.c_int32),
                ("points", _fp), ("slots", _fp), ("words", _fp), ("rays", _fp), ("g_rgb", _fp), ("g_depth", _fp), ("g_opacity", _fp),
                ("g_rays", _fp)]


class BakedTvArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("n_bricks", C.c_int32), ("F", C.c_int32),
                ("sigma_stride", C.c_int32), ("eps", C.c_float), ("w", C.c_float * 28), ("reserved_", C.c_int32), ("words", _fp),
                ("slots", _fp), ("bricks", _fp), ("data", _fp), ("sigma", _fp), ("grad", _fp), ("partial", _fp)]


class BakedUpsampleArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("degree", C.c_int32), ("level", C.c_float),
                ("reserved_", C.c_int32), ("points", _fp), ("out", _fp)]


class BrickUpsampleArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("degree", C.c_int32), ("level", C.c_float),
                ("n_bricks", C.c_int32), ("n_child", C.c_int32), ("reserved_", C.c_int32), ("slots", _fp), ("pool", _fp),
                ("child_bricks", _fp), ("words", _fp), ("out", _fp)]


ENV_MAX_E = 8192  # UPNERF_ENV_MAX_E: cells per face side of an environment map at the most


class EnvRaysArgs(C.Structure):
    _fields_ = [("E", C.c_int32), ("count", C.c_int32), ("n0", C.c_int64), ("lo", C.c_float * 3), ("hi", C.c_float * 3),
                ("far", C.c_float), ("reserved_", C.c_int32), ("rays", _fp)]


class EnvSeamArgs(C.Structure):
    _fields_ = [("E", C.c_int32), ("reserved_", C.c_int32), ("env", _fp)]


class EnvCompositeArgs(C.Structure):
    _fields_ = [("E", C.c_int32), ("R", C.c_int32), ("env", _fp), ("rays", _fp), ("opacity", _fp), ("rgb_in", _fp), ("rgb_out", _fp)]


class EnvCompositeBwdArgs(C.Structure):
    _fields_ = [("E", C.c_int32), ("R", C.c_int32), ("env", _fp), ("rays", _fp), ("opacity", _fp), ("g_out", _fp), ("g_opacity", _fp),
                ("g_rays", _fp)]


class BakedVisibilityArgs(C.Structure):
    _fields_ = [("Cx", C.c_int32), ("Cy", C.c_int32), ("Cz", C.c_int32), ("R", C.c_int32), ("lo", C.c_float * 3),
                ("hi", C.c_float * 3), ("step", C.c_float), ("stop", C.c_float), ("E", C.c_int32), ("sigma_offset", C.c_int32),
                ("points", _fp), ("slots", _fp), ("words", _fp), ("rays", _fp), ("vis", _fp)]


class BakedPruneArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("min_weight", C.c_float), ("E", C.c_int32), ("vis", _fp), ("points", _fp), ("kept", _fp)]


class DensityGradArgs(C.Structure):
    _fields_ = [("M", C.c_int32), ("reserved_", C.c_int32), ("points", _fp), ("P", _fp), ("PT", _fp), ("wk_xyz", C.c_float * 10),
                ("sigma", _fp), ("grad", _fp)]


class NormalCompositeArgs(C.Structure):
    _fields_ = [("R", C.c_int32), ("S", C.c_int32), ("grad", _fp), ("w", _fp), ("normal", _fp)]


class VizNormalsArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("n", _fp), ("rot", _fp), ("rgb", _fp)]


class Rng(C.Structure):
    """upnerf_rng: key of the uniform draws a kernel generates itself."""
    _fields_ = [("seed", C.c_uint64), ("step", C.c_int32), ("row0", C.c_int32), ("row_stride", C.c_int32), ("step_dev", _fp)]


_i, _f, _p = C.c_int, C.c_float, C.c_void_p
_SIGNATURES = {
    "upnerf_abi_version": [],
    "upnerf_pose_rays_fwd": [_i, _p, _p, _p, _p, _p, _p],
    "upnerf_pose_rays_bwd": [_i, _p, _p, _p, _p, _p, _p, _p],
    "upnerf_sample_coarse": [_i, _i, _p, _p, _p, _f, _i, _p, _p],
    "upnerf_uniform_keyed": [_i, _i, C.c_uint64, _i, _p, _i, _i, _i, _p, _p],
    "upnerf_sample_pdf": [_i, _i, _p, _p, _p, _i, _i, _p, _i, _p],
    "upnerf_sort_rows": [_i, _i, _p, _p],
    "upnerf_sample_coarse_keyed": [_i, _i, _p, _p, C.POINTER(Rng), _f, _i, _p, _p],
    # (R, Nc, z, w_a, n_a, col_a, u_a, draw_a, w_b, n_b, col_b, u_b, draw_b, u_rows, rng, zf, stream)
    "upnerf_resample_sort": [_i, _i, _p, _p, _i, _i, _p, _i, _p, _i, _i, _p, _i, _i, C.POINTER(Rng), _p, _p],
    "upnerf_ray_aux": [_i, _p, _p, C.POINTER(C.c_float), _p, _p, _p],
    "upnerf_field_fwd": [C.POINTER(Layout), C.POINTER(FieldFwdArgs), _p],
    "upnerf_composite_fwd": [C.POINTER(CompositeFwdArgs), _p],
    "upnerf_composite_bwd": [C.POINTER(CompositeBwdArgs), _p],
    "upnerf_field_bwd": [C.POINTER(Layout), C.POINTER(FieldBwdArgs), _p],
    "upnerf_field_fwd_f16x3": [C.POINTER(Layout), C.POINTER(FieldFwdArgs), _p],
    "upnerf_field_bwd_f16x3": [C.POINTER(Layout), C.POINTER(FieldBwdArgs), _p],
    "upnerf_frag16": [_p, _p, _p, C.POINTER(Frag16Desc), _i, C.POINTER(Frag16Desc), _i, _p, _p, _i, _i, _p, _p],
    "upnerf_wgrad": [_i, _p, _i, _i, _p, _i, _i, _p, _i, _p, _p, _i, _p],
    "upnerf_wgrad16_scratch": [C.POINTER(WgradDesc)],
    "upnerf_wgrad16": [C.POINTER(WgradDesc), C.POINTER(WgradPending), _p],
    "upnerf_wgrad_finish": [_p, _p],
    "upnerf_transient_fwd": [C.POINTER(TransientArgs), _p],
    "upnerf_transient_bwd": [C.POINTER(TransientArgs), C.POINTER(TransientGrads), _p],
    "upnerf_wgrad_grouped_scratch": [C.POINTER(WgradGroup), _i, _i],
    "upnerf_wgrad_grouped": [C.POINTER(WgradGroup), _i, _p, _i, _p],
    "upnerf_vec_wgrad": [_i, _p, _i, _i, _p, _i, _i, _p, _p, _p, _i, _p],
    "upnerf_matvec": [_i, _i, _p, _i, _p, _p, _p, _i, _p],
    "upnerf_matvec_rank1": [_i, _i, _p, _i, _p, _p, _p, _i, _p, _p],
    "upnerf_add_pairs": [C.POINTER(AddPair), _i, _p],
    "upnerf_zero": [_p, C.c_longlong, _p],
    "upnerf_vec_wgrad_frag16": [_i, _p, _i, _i, _p, _p, _i, _p, _p, _p, _i, _p],
    "upnerf_ray_sum": [_i, _i, _p, _i, _p, _p],
    "upnerf_ray_part_finish": [_i, _i, _p, _p, _p, _p],
    "upnerf_tile_part_finish": [_i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "upnerf_ray_geom_bwd": [_i, _i, _p, _p, _p, _p, _p],
    "upnerf_pack": [_p, C.POINTER(PackDesc), _i, _i, _p],
    "upnerf_gather_rays": [C.POINTER(GatherRaysArgs), _p],
    "upnerf_embed_bwd": [_i, _i, _i, _p, _p, _p, _p],
    "upnerf_embed_bwd_grouped": [_i, _i, _p, C.POINTER(EmbedGroup), _i, _p],
    "upnerf_embed_fwd_grouped": [_i, _i, _p, C.POINTER(EmbedRowsGroup), _i, _p],
    "upnerf_linear": [_i, _i, _i, _p, _i, _p, _i, _p, _p, _i, _i, _p],
    "upnerf_loss_fwd": [C.POINTER(LossArgs), _p, _p, _p, _p],
    "upnerf_loss_bwd": [C.POINTER(LossArgs), _p, C.POINTER(LossGrads), _p],
    "upnerf_frag_copy": [_p, _p, C.POINTER(FragDesc), _i, _p],
    "upnerf_adam": [C.c_int64, _p, _p, _p, _p, _f, _f, _f, _f, _f, _p, _p],
    "upnerf_adam_gather": [_p, _p, _p, _p, _i, _f, _f, _f, _f, _f, _p, _p],
    "upnerf_set_scalars": [_p, _i, C.POINTER(C.c_float), _p],
    "upnerf_scale_exponents": [_p, _i, _p, _p],
    "upnerf_ssim_scratch": [C.POINTER(SsimArgs)],
    "upnerf_ssim": [C.POINTER(SsimArgs), _p, _p],
    "upnerf_conv2d": [C.POINTER(Conv2dArgs), _p],
    "upnerf_maxpool2d": [C.POINTER(Maxpool2dArgs), _p],
    "upnerf_lpips_dist": [C.POINTER(LpipsDistArgs), _p, _p],
    "upnerf_lpips_scratch": [C.POINTER(LpipsScratchArgs)],
    "upnerf_scene_rays": [C.POINTER(SceneRaysArgs), C.POINTER(SceneImage), _p, _p],
    "upnerf_resize_scratch": [C.POINTER(ResizeArgs)],
    "upnerf_resize_linear": [C.POINTER(ResizeArgs), C.POINTER(ResizeMap), _p, _p],
    "upnerf_viz_minmax_scratch": [C.c_longlong],
    "upnerf_viz_minmax": [_p, C.c_longlong, C.c_longlong, _p, _p, _p],
    "upnerf_viz_depth_scratch": [C.POINTER(VizDepthArgs)],
    "upnerf_viz_depth": [C.POINTER(VizDepthArgs), _p, _p],
    "upnerf_viz_pca_scratch": [C.POINTER(VizPcaArgs)],
    "upnerf_viz_pca": [C.POINTER(VizPcaArgs), _p, _p],
    "upnerf_viz_rgb": [C.POINTER(VizRgbArgs), _p],
    "upnerf_path_poses": [C.POINTER(PathPosesArgs), _p],
    "upnerf_path_rays": [C.POINTER(PathRaysArgs), _p],
    "upnerf_grid_columns": [C.POINTER(GridColumnsArgs), _p],
    "upnerf_mtet_scratch": [_i, _i, _i],
    "upnerf_mtet_count": [C.POINTER(MtetArgs), _p, _p, _p],
    "upnerf_mtet_emit": [C.POINTER(MtetArgs), _p, _p],
    "upnerf_occ_words": [_i, _i, _i],
    "upnerf_occ_build_scratch": [_i, _i, _i],
    "upnerf_occ_build": [C.POINTER(OccBuildArgs), _p],
    "upnerf_occ_spans": [C.POINTER(OccSpansArgs), _p],
    "upnerf_occ_compact_scratch": [_i],
    "upnerf_occ_compact": [C.POINTER(OccCompactArgs), _p],
    "upnerf_occ_scatter": [C.POINTER(OccScatterArgs), _p],
    "upnerf_density_grad": [C.POINTER(Layout), C.POINTER(DensityGradArgs), _p],
    "upnerf_normal_composite": [C.POINTER(NormalCompositeArgs), _p],
    "upnerf_viz_normals": [C.POINTER(VizNormalsArgs), _p],
    "upnerf_tsdf_integrate": [C.POINTER(TsdfIntegrateArgs), _p],
    "upnerf_tsdf_surface": [C.POINTER(TsdfSurfaceArgs), _p],
    "upnerf_tsdf_sample": [C.POINTER(TsdfSampleArgs), _p],
    "upnerf_vit_patches": [C.POINTER(VitPatchesArgs), _p],
    "upnerf_vit_embed": [_i, _i, _p, _p, _p, _p],
    "upnerf_layernorm": [_i, _i, _p, _i, _p, _p, _f, _p, _i, _p],
    "upnerf_vit_attention": [C.POINTER(VitAttentionArgs), _p],
    "upnerf_vit_gelu": [_p, C.c_longlong, _p],
    "upnerf_vit_residual": [_p, _p, C.c_longlong, _p],
    "upnerf_pca_fit_scratch": [_i, _i],
    "upnerf_pca_fit": [C.POINTER(PcaFitArgs), _p, _p],
    "upnerf_conv3x3": [C.POINTER(Conv3x3Args), _p],
    "upnerf_upsample2x": [C.POINTER(Upsample2xArgs), _p],
    "upnerf_depth_to_space": [C.POINTER(DepthToSpaceArgs), _p],
    "upnerf_resize_cubic": [C.POINTER(ResizeCubicArgs), _p],
    "upnerf_vit_patches16": [C.POINTER(VitPatches16Args), _p],
    "upnerf_baked_render": [C.POINTER(BakedRenderArgs), _p],
    "upnerf_baked_pack": [C.POINTER(BakedPackArgs), _p],
    "upnerf_baked_sh_render": [C.POINTER(BakedShRenderArgs), _p],
    "upnerf_sh_accumulate": [C.POINTER(ShAccumulateArgs), _p],
    "upnerf_baked_sh_pack": [C.POINTER(BakedShPackArgs), _p],
    "upnerf_brick_table_scratch": [_i, _i, _i],
    "upnerf_brick_table": [C.POINTER(BrickTableArgs), _p],
    "upnerf_brick_gather": [C.POINTER(BrickGatherArgs), _p],
    "upnerf_brick_scatter": [C.POINTER(BrickScatterArgs), _p],
    "upnerf_brick_occ": [C.POINTER(BrickOccArgs), _p],
    "upnerf_brick_columns": [C.POINTER(BrickColumnsArgs), _p],
    "upnerf_baked_sparse_render": [C.POINTER(BakedSparseRenderArgs), _p],
    "upnerf_baked_render_bwd": [C.POINTER(BakedRenderBwdArgs), _p],
    "upnerf_baked_project": [C.POINTER(BakedProjectArgs), _p],
    "upnerf_baked_sparse_render_bwd": [C.POINTER(BakedSparseRenderBwdArgs), _p],
    "upnerf_brick_face_sum": [C.POINTER(BrickFaceSumArgs), _p],
    "upnerf_baked_ray_bwd": [C.POINTER(BakedRayBwdArgs), _p],
    "upnerf_baked_tv_blocks": [_i, _i, _i, _i],
    "upnerf_baked_tv": [C.POINTER(BakedTvArgs), _p],
    "upnerf_baked_upsample": [C.POINTER(BakedUpsampleArgs), _p],
    "upnerf_brick_upsample_mark": [C.POINTER(BrickUpsampleArgs), _p],
    "upnerf_brick_upsample_fill": [C.POINTER(BrickUpsampleArgs), _p],
    "upnerf_env_rays": [C.POINTER(EnvRaysArgs), _p],
    "upnerf_env_seam": [C.POINTER(EnvSeamArgs), _p],
    "upnerf_env_composite": [C.POINTER(EnvCompositeArgs), _p],
    "upnerf_env_composite_bwd": [C.POINTER(EnvCompositeBwdArgs), _p],
    "upnerf_baked_visibility": [C.POINTER(BakedVisibilityArgs), _p],
    "upnerf_brick_face_max": [C.POINTER(BrickFaceSumArgs), _p],
    "upnerf_baked_prune": [C.POINTER(BakedPruneArgs), _p],
}
_LONGLONG = ("upnerf_wgrad16_scratch", "upnerf_mtet_scratch", "upnerf_occ_words", "upnerf_occ_build_scratch",
             "upnerf_occ_compact_scratch", "upnerf_pca_fit_scratch", "upnerf_brick_table_scratch", "upnerf_baked_tv_blocks")
MAX_SCALARS = 96
EXPORTS = tuple(_SIGNATURES)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python __graft_entry__.py` "
            "(there is no CPU/PyTorch fallback for the render_rays hot path).")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise ImportError(f"{LIB_PATH} does not export {name}; rebuild it")
        fn.argtypes = argtypes
        fn.restype = C.c_longlong if name in _LONGLONG else C.c_int
    return lib


lib = _load()
ABI_VERSION = 11
if lib.upnerf_abi_version() != ABI_VERSION:
    raise ImportError("libupnerf_hip.so ABI version mismatch; rebuild it")


_PTR_DTYPES = (torch.float32, torch.int64, torch.int32, torch.float16, torch.uint8, torch.float64)


def ptr(t):
    """Device pointer of a contiguous fp32/int64 CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    # explicit raises, not asserts: this is the only guard between Python and raw device pointers (python -O keeps it)
    if not t.is_cuda:
        raise RuntimeError("libupnerf_hip operates on device memory only (got a CPU tensor)")
    if not t.is_contiguous():
        raise RuntimeError("non-contiguous tensor handed to the HIP path")
    if t.dtype not in _PTR_DTYPES:
        raise TypeError(f"unsupported dtype {t.dtype} handed to the HIP path")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


CALLS = [0]  # C-ABI calls checked so far (bench.py reports calls per step)


def check(rc: int, what: str):
    CALLS[0] += 1
    if rc != 0:
        kind = {-1: "invalid argument", -2: "unsupported shape"}.get(rc, f"hipError_t {rc}")
        raise RuntimeError(f"{what} failed: {kind}")
