"""ctypes binding of the C-ABI declared in ``include/mi_restore.h``.

The library is loaded lazily on first use and the load fails loudly: there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI_RESTORE_LIB") or os.path.join(HERE, "libmi_restore.so")   # (override: A/B builds)

MI_F32, MI_BF16 = 0, 1
MI_SSIM_TILE = 32   # include/mi_restore.h: the tile edge of the SSIM loss kernels (map tiles and image tiles)
c_i64 = C.c_int64
vp = C.c_void_p
fp = C.c_void_p  # float* passed as raw addresses


class PwDesc(C.Structure):
    _fields_ = [("x1", vp), ("x1_bs", c_i64), ("x1_gs", c_i64), ("k1", C.c_int),
                ("x2", vp), ("x2_bs", c_i64), ("x2_gs", c_i64), ("k2", C.c_int),
                ("w", fp), ("w_bs", c_i64), ("w_gs", c_i64), ("w_sm", c_i64), ("w_sk", c_i64),
                ("bias", fp), ("bias_gs", c_i64),
                ("r", vp), ("r_bs", c_i64), ("r_gs", c_i64),
                ("y", vp), ("y_bs", c_i64), ("y_gs", c_i64),
                ("m", C.c_int), ("n", c_i64), ("batch", C.c_int), ("groups", C.c_int), ("dtype", C.c_int),
                ("ln_w", fp), ("ln_b", fp), ("ln_mean", fp), ("ln_rstd", fp), ("ln_mode", C.c_int),
                ("f8", C.c_int), ("f8_sx", C.c_float), ("f8_sw", C.c_float),
                ("y_split", C.c_int), ("y2", vp), ("y2_bs", c_i64), ("y2_gs", c_i64),
                ("w_b16", vp), ("w_b16_sm", c_i64)]


class GramDesc(C.Structure):
    _fields_ = [("a", vp), ("a_bs", c_i64), ("a_gs", c_i64), ("ma", C.c_int),
                ("b", vp), ("b_bs", c_i64), ("b_gs", c_i64), ("mb", C.c_int),
                ("n", c_i64), ("batch", C.c_int), ("groups", C.c_int), ("dtype", C.c_int),
                ("sum_batch", C.c_int), ("accumulate", C.c_int),
                ("out", fp), ("out_ld", c_i64), ("out_zs", c_i64), ("sumsq", fp)]


class MdtaShape(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("heads", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("dtype", C.c_int), ("ks", C.c_int)]


class MdtaParams(C.Structure):
    _fields_ = [("temperature", fp), ("qkv_w", fp), ("qkv_b", fp), ("dw_w", fp), ("dw_b", fp),
                ("proj_w", fp), ("proj_b", fp)]


class MdtaGrads(C.Structure):
    _fields_ = [("temperature", fp), ("qkv_w", fp), ("qkv_b", fp), ("dw_w", fp), ("dw_b", fp),
                ("proj_w", fp), ("proj_b", fp), ("accumulate", C.c_int)]


class XmdtaShape(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("heads", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("dtype", C.c_int), ("ks_q", C.c_int), ("ks_kv", C.c_int)]


class XmdtaParams(C.Structure):
    _fields_ = [(n, fp) for n in ("temperature", "q_w", "q_b", "q_dw_w", "q_dw_b", "kv_w", "kv_b", "kv_dw_w", "kv_dw_b",
                                  "proj_w", "proj_b")]


class XmdtaGrads(C.Structure):
    _fields_ = [(n, fp) for n in ("temperature", "q_w", "q_b", "q_dw_w", "q_dw_b", "kv_w", "kv_b", "kv_dw_w", "kv_dw_b",
                                  "proj_w", "proj_b")] + [("accumulate", C.c_int)]


class GdfnShape(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("hidden", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("dtype", C.c_int), ("ks", C.c_int), ("flags", C.c_int)]


class GdfnParams(C.Structure):
    _fields_ = [("in_w", fp), ("in_b", fp), ("dw_w", fp), ("dw_b", fp), ("out_w", fp), ("out_b", fp)]


class GdfnFusedShape(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("hidden", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("ln_with_bias", C.c_int)]


class LnHead(C.Structure):
    _fields_ = [("w", fp), ("b", fp), ("mean", fp), ("rstd", fp), ("with_bias", C.c_int)]


class F8Scales(C.Structure):
    _fields_ = [("x1", C.c_float), ("w1", C.c_float), ("x2", C.c_float), ("w2", C.c_float)]


class LnTail(C.Structure):
    _fields_ = [("w", fp), ("b", fp), ("mean", fp), ("rstd", fp), ("dres", vp), ("dw", fp), ("db", fp)]


class GroupedProblem(C.Structure):
    _fields_ = [("x", vp), ("x_rs", c_i64), ("w", fp), ("w_sm", c_i64), ("w_sk", c_i64), ("bias", fp), ("r", vp), ("r_rs", c_i64),
                ("y", vp), ("y_rs", c_i64), ("m", C.c_int), ("k", C.c_int), ("expert", C.c_int), ("x_local", C.c_int),
                ("y_local", C.c_int), ("r_local", C.c_int)]


class GdfnGrads(C.Structure):
    _fields_ = [("in_w", fp), ("in_b", fp), ("dw_w", fp), ("dw_b", fp), ("out_w", fp), ("out_b", fp),
                ("accumulate", C.c_int)]


class TksaShape(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("heads", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int),
                ("k1", C.c_int), ("k2", C.c_int), ("k3", C.c_int), ("k4", C.c_int)]


class TksaParams(C.Structure):
    _fields_ = [(n, fp) for n in ("attn1", "attn2", "attn3", "attn4")]


class TksaGrads(C.Structure):
    _fields_ = [(n, fp) for n in ("attn1", "attn2", "attn3", "attn4")]


MSFN_PARAM_NAMES = ("in_w", "in_b", "dw3_w", "dw3_b", "dw5_w", "dw5_b", "g3_w", "g3_b", "g5_w", "g5_b", "out_w", "out_b")


class MsfnShape(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("hidden", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int)]


class MsfnParams(C.Structure):
    _fields_ = [(n, fp) for n in MSFN_PARAM_NAMES]


class MsfnGrads(C.Structure):
    _fields_ = [(n, fp) for n in MSFN_PARAM_NAMES] + [("accumulate", C.c_int)]


class MefcShape(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int), ("steps", C.c_int)]


MEFC_STEP_FIELDS = (("sep_dw1", 4), ("sep_pw1", 4), ("sep_dw2", 4), ("sep_pw2", 4), ("dil_dw", 3), ("dil_pw", 3), ("out_w", 1))


class MefcStepParams(C.Structure):
    _fields_ = [(n, fp * k) if k > 1 else (n, fp) for n, k in MEFC_STEP_FIELDS]


class MefcStepGrads(C.Structure):
    _fields_ = [(n, fp * k) if k > 1 else (n, fp) for n, k in MEFC_STEP_FIELDS]


class MefcParams(C.Structure):
    _fields_ = [(n, fp) for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "pre_w")] + [("step", C.POINTER(MefcStepParams))]


class MefcGrads(C.Structure):
    _fields_ = [(n, fp) for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "pre_w")] + [("step", C.POINTER(MefcStepGrads)),
                                                                                     ("accumulate", C.c_int)]


class DilgateParams(C.Structure):
    _fields_ = [("w", fp * 4), ("b", fp * 4)]


class DilgateGrads(C.Structure):
    _fields_ = [("w", fp * 4), ("b", fp * 4), ("accumulate", C.c_int)]


class DblockShape(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int), ("n_dil", C.c_int),
                ("dil", C.c_int * 4), ("extra", C.c_int)]


# mi_dblock_params / mi_dblock_grads in field order; (name, 4): one pointer per branch
DBLOCK_FIELDS = (("norm1_w", 1), ("norm1_b", 1), ("conv1_w", 1), ("conv1_b", 1), ("extra_w", 1), ("extra_b", 1), ("br_w", 4), ("br_b", 4),
                 ("sca_w", 1), ("sca_b", 1), ("conv3_w", 1), ("conv3_b", 1), ("beta", 1), ("norm2_w", 1), ("norm2_b", 1),
                 ("conv4_w", 1), ("conv4_b", 1), ("conv5_w", 1), ("conv5_b", 1), ("gamma", 1))


class DblockParams(C.Structure):
    _fields_ = [(n, fp * k) if k > 1 else (n, fp) for n, k in DBLOCK_FIELDS]


class DblockGrads(C.Structure):
    _fields_ = [(n, fp * k) if k > 1 else (n, fp) for n, k in DBLOCK_FIELDS] + [("accumulate", C.c_int)]


class FremlpShape(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("expand", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int)]


class FourierUnitShape(C.Structure):
    _fields_ = [("B", C.c_int), ("c", C.c_int), ("groups", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int),
                ("training", C.c_int), ("eps", C.c_float), ("momentum", C.c_float)]


# mi_fourier_unit_params / mi_fourier_unit_grads in field order
FOURIER_UNIT_FIELDS = ("bn_w", "bn_b", "fdc_w", "fdc_b", "gate_w", "gate_b", "fpe_w", "fpe_b")


class FourierUnitParams(C.Structure):
    _fields_ = [(n, fp) for n in FOURIER_UNIT_FIELDS]


class FourierUnitGrads(C.Structure):
    _fields_ = [(n, fp) for n in FOURIER_UNIT_FIELDS] + [("accumulate", C.c_int)]


class SfhFfnShape(C.Structure):
    _fields_ = [("B", C.c_int), ("dim", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int)]


# mi_sfh_ffn_params / mi_sfh_ffn_grads and mi_sfh_local_params / mi_sfh_local_grads in field order
SFH_FFN_FIELDS = ("init_w", "init_b", "c1_w", "c1_b", "c2_w", "c2_b", "c3_w", "c3_b", "fina_w", "fina_b")
SFH_LOCAL_FIELDS = ("cd1_w", "cd1_b", "cd2_w", "cd2_b")


class SfhFfnParams(C.Structure):
    _fields_ = [(n, fp) for n in SFH_FFN_FIELDS]


class SfhFfnGrads(C.Structure):
    _fields_ = [(n, fp) for n in SFH_FFN_FIELDS] + [("accumulate", C.c_int)]


class SfhLocalShape(C.Structure):
    _fields_ = SfhFfnShape._fields_


class SfhLocalParams(C.Structure):
    _fields_ = [(n, fp) for n in SFH_LOCAL_FIELDS]


class SfhLocalGrads(C.Structure):
    _fields_ = [(n, fp) for n in SFH_LOCAL_FIELDS] + [("accumulate", C.c_int)]


class SfhMixerShape(C.Structure):
    """mi_sfh_global_shape / mi_sfh_mixer_shape (one struct)"""
    _fields_ = [("B", C.c_int), ("dim", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int), ("training", C.c_int),
                ("eps", C.c_float), ("momentum", C.c_float)]


# mi_sfh_global_params / _grads and mi_sfh_mixer_params / _grads in field order (the modules' named_parameters() order)
SFH_GLOBAL_FIELDS = ("init_w", "init_b", "fina_w", "fina_b") + FOURIER_UNIT_FIELDS
SFH_MIXER_FIELDS = SFH_LOCAL_FIELDS + SFH_GLOBAL_FIELDS + ("cac_w", "cac_b", "ca1_w", "ca1_b", "ca2_w", "ca2_b", "conv_w", "conv_b")


class SfhGlobalParams(C.Structure):
    _fields_ = [(n, fp) for n in SFH_GLOBAL_FIELDS]


class SfhGlobalGrads(C.Structure):
    _fields_ = [(n, fp) for n in SFH_GLOBAL_FIELDS] + [("accumulate", C.c_int)]


class SfhMixerParams(C.Structure):
    _fields_ = [(n, fp) for n in SFH_MIXER_FIELDS]


class SfhMixerGrads(C.Structure):
    _fields_ = [(n, fp) for n in SFH_MIXER_FIELDS] + [("accumulate", C.c_int)]


class Bn2dShape(C.Structure):
    """mi_bn2d_shape / mi_scale_res_shape (one struct)"""
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int), ("training", C.c_int),
                ("eps", C.c_float), ("momentum", C.c_float)]


# mi_sfh_block_params / _grads: norm1, the Mixer's struct, beta, norm2, the FFN's struct, gamma (the Block's named_parameters()
# order is beta, gamma, norm1, norm2, mixer, ffn: ops._sb_struct places them)
class SfhBlockParams(C.Structure):
    _fields_ = [("bn1_w", fp), ("bn1_b", fp), ("mixer", SfhMixerParams), ("beta", fp), ("bn2_w", fp), ("bn2_b", fp), ("ffn", SfhFfnParams),
                ("gamma", fp)]


class SfhBlockGrads(C.Structure):
    _fields_ = [("bn1_w", fp), ("bn1_b", fp), ("mixer", SfhMixerGrads), ("beta", fp), ("bn2_w", fp), ("bn2_b", fp), ("ffn", SfhFfnGrads),
                ("gamma", fp), ("accumulate", C.c_int)]


class SfhBlockStats(C.Structure):
    _fields_ = [(n, fp) for n in ("mean1", "var1", "mean2", "var2", "mean_fu", "var_fu")]


class EblockShape(C.Structure):
    _fields_ = DblockShape._fields_


# mi_eblock_params / mi_eblock_grads in field order; (name, 4): one pointer per branch
EBLOCK_FIELDS = (("norm1_w", 1), ("norm1_b", 1), ("extra_w", 1), ("extra_b", 1), ("conv1_w", 1), ("conv1_b", 1), ("br_w", 4), ("br_b", 4),
                 ("sca_w", 1), ("sca_b", 1), ("conv3_w", 1), ("conv3_b", 1), ("beta", 1), ("norm2_w", 1), ("norm2_b", 1),
                 ("fre_w1", 1), ("fre_b1", 1), ("fre_w2", 1), ("fre_b2", 1), ("gamma", 1))


class EblockParams(C.Structure):
    _fields_ = [(n, fp * k) if k > 1 else (n, fp) for n, k in EBLOCK_FIELDS]


class EblockGrads(C.Structure):
    _fields_ = [(n, fp * k) if k > 1 else (n, fp) for n, k in EBLOCK_FIELDS] + [("accumulate", C.c_int)]


# symbol -> (restype, argtypes); this table is also what tests/test_cabi.py checks against the header
SIGNATURES = {
    "mi_version": (C.c_int, []),
    "mi_last_error": (C.c_char_p, []),
    "mi_env_reload": (C.c_int, []),
    "mi_deferred_begin": (C.c_int, [vp, C.c_size_t]),
    "mi_deferred_record": (C.c_int, [C.c_int]),
    "mi_deferred_pending": (C.c_int, []),
    "mi_deferred_high_water": (C.c_size_t, []),
    "mi_deferred_flush": (C.c_int, [vp]),
    "mi_deferred_end": (C.c_int, []),
    "mi_ln_fwd": (C.c_int, [vp, fp, fp, vp, fp, fp, C.c_int, C.c_int, c_i64, C.c_int, C.c_int, vp]),
    "mi_ln_fwd_eps": (C.c_int, [vp, fp, fp, vp, fp, fp, C.c_int, C.c_int, c_i64, C.c_int, C.c_float, C.c_int, vp]),
    "mi_ln_bwd_workspace": (C.c_size_t, [C.c_int, C.c_int, c_i64]),
    "mi_ln_bwd": (C.c_int, [vp, vp, fp, fp, fp, vp, vp, fp, fp, C.c_int, C.c_int, c_i64, C.c_int, C.c_int, C.c_int,
                            vp, vp]),
    "mi_ln_plan": (C.c_int, [C.c_int, C.c_int, c_i64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "mi_dwconv_fwd": (C.c_int, [vp, fp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_dwconv_gate_fwd": (C.c_int, [vp, fp, fp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_dwconv_bwd_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_dwconv_bwd": (C.c_int, [vp, vp, fp, vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                vp, vp]),
    "mi_dwconv_gate_bwd": (C.c_int, [vp, vp, vp, fp, vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, vp, vp]),
    "mi_dwconv_gate_recompute_ok": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "mi_dwconv_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "mi_dwconv_gate_bwd_recompute": (C.c_int, [vp, vp, fp, fp, vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int, vp, vp]),
    "mi_pw_gemm_workspace": (C.c_size_t, [C.POINTER(PwDesc)]),
    "mi_pw_gemm": (C.c_int, [C.POINTER(PwDesc), vp, vp]),
    "mi_pw_cache_enable": (C.c_int, [vp, C.c_size_t, vp, vp]),
    "mi_pw_cache_refresh": (C.c_int, [vp]),
    "mi_pw_cache_invalidate": (C.c_int, []),
    "mi_pw_cache_pending": (C.c_int, []),
    "mi_gram_workspace": (C.c_size_t, [C.POINTER(GramDesc)]),
    "mi_gram": (C.c_int, [C.POINTER(GramDesc), vp, vp]),
    "mi_gram_plan": (C.c_int, [C.POINTER(GramDesc), C.POINTER(c_i64)]),
    "mi_mdta_saved_bytes": (C.c_size_t, [C.POINTER(MdtaShape)]),
    "mi_mdta_workspace": (C.c_size_t, [C.POINTER(MdtaShape)]),
    "mi_mdta_fwd": (C.c_int, [C.POINTER(MdtaShape), C.POINTER(MdtaParams), vp, vp, vp, vp, vp, vp]),
    "mi_mdta_bwd": (C.c_int, [C.POINTER(MdtaShape), C.POINTER(MdtaParams), vp, vp, vp, C.POINTER(MdtaGrads), vp, vp,
                              vp]),
    "mi_xmdta_saved_bytes": (C.c_size_t, [C.POINTER(XmdtaShape)]),
    "mi_xmdta_workspace": (C.c_size_t, [C.POINTER(XmdtaShape)]),
    "mi_xmdta_fwd": (C.c_int, [C.POINTER(XmdtaShape), C.POINTER(XmdtaParams), vp, vp, vp, vp, vp, vp, vp]),
    "mi_xmdta_bwd": (C.c_int, [C.POINTER(XmdtaShape), C.POINTER(XmdtaParams), vp, vp, vp, vp, vp, C.POINTER(XmdtaGrads), vp,
                               vp, vp]),
    "mi_gdfn_saved_bytes": (C.c_size_t, [C.POINTER(GdfnShape)]),
    "mi_gdfn_workspace": (C.c_size_t, [C.POINTER(GdfnShape)]),
    "mi_pw_gemm_ln_ok": (C.c_int, [C.POINTER(PwDesc)]),
    "mi_mdta_fwd_ln_ok": (C.c_int, [C.POINTER(MdtaShape)]),
    "mi_mdta_fwd_ln": (C.c_int, [C.POINTER(MdtaShape), C.POINTER(MdtaParams), C.POINTER(LnHead), vp, vp, vp, vp, vp, vp]),
    "mi_gdfn_fwd_ln_ok": (C.c_int, [C.POINTER(GdfnShape)]),
    "mi_gdfn_fwd_ln": (C.c_int, [C.POINTER(GdfnShape), C.POINTER(GdfnParams), C.POINTER(LnHead), vp, vp, vp, vp, vp, vp]),
    "mi_pw_gemm_f8_ok": (C.c_int, [C.POINTER(PwDesc)]),
    "mi_pw_gemm_split_ok": (C.c_int, [C.POINTER(PwDesc)]),
    "mi_pw_plan": (C.c_int, [C.POINTER(PwDesc), C.POINTER(c_i64)]),
    "mi_mdta_fwd_f8_ok": (C.c_int, [C.POINTER(MdtaShape), C.c_int]),
    "mi_mdta_fwd_f8": (C.c_int, [C.POINTER(MdtaShape), C.POINTER(MdtaParams), C.POINTER(LnHead), C.POINTER(F8Scales), vp, vp, vp,
                                 vp, vp]),
    "mi_gdfn_fwd_f8_ok": (C.c_int, [C.POINTER(GdfnShape), C.c_int]),
    "mi_gdfn_fwd_f8": (C.c_int, [C.POINTER(GdfnShape), C.POINTER(GdfnParams), C.POINTER(LnHead), C.POINTER(F8Scales), vp, vp, vp,
                                 vp, vp]),
    "mi_box_down": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_fre_rect": (C.c_int, [fp, fp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_fre_split_coef_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mi_fre_split_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_fre_split_max_hw": (C.c_int, []),
    "mi_fre_split_fwd": (C.c_int, [vp, vp, vp, vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_fre_split_bwd": (C.c_int, [vp, vp, fp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi_chan_maxmean_fwd": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_chan_maxmean_bwd": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_plane_max_fwd": (C.c_int, [vp, fp, vp, C.c_int, c_i64, C.c_int, vp]),
    "mi_pool_pair_bwd": (C.c_int, [fp, fp, vp, vp, C.c_int, c_i64, C.c_int, vp]),
    "mi_chan_gate_fwd": (C.c_int, [fp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, vp]),
    "mi_chan_gate_bwd": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_refine_mix_fwd": (C.c_int, [vp, vp, vp, fp, vp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_refine_mix_bwd": (C.c_int, [vp, vp, vp, fp, vp, vp, vp, vp, fp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_scale_add_fwd": (C.c_int, [vp, vp, fp, fp, vp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_scale_add_bwd": (C.c_int, [vp, vp, fp, fp, vp, vp, vp, fp, fp, C.c_int, C.c_int, c_i64, C.c_int, C.c_int, vp]),
    "mi_bwd_tail_ok": (C.c_int, [C.c_int, C.c_int, c_i64, C.c_int]),
    "mi_bwd_tail_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "mi_bwd_tail_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, c_i64, C.c_int, C.POINTER(c_i64)]),
    "mi_bwd_tail": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, fp, fp, fp, fp, fp, vp, fp, fp, fp, C.c_int, c_i64, C.c_int,
                              C.c_int, vp, vp]),
    "mi_mdta_bwd_ln_ok": (C.c_int, [C.POINTER(MdtaShape), C.c_int]),
    "mi_mdta_bwd_ln_workspace": (C.c_size_t, [C.POINTER(MdtaShape)]),
    "mi_mdta_bwd_ln": (C.c_int, [C.POINTER(MdtaShape), C.POINTER(MdtaParams), C.POINTER(LnTail), vp, vp, vp,
                                 C.POINTER(MdtaGrads), vp, vp, vp]),
    "mi_gdfn_bwd_ln_ok": (C.c_int, [C.POINTER(GdfnShape), C.c_int]),
    "mi_gdfn_bwd_ln_workspace": (C.c_size_t, [C.POINTER(GdfnShape)]),
    "mi_gdfn_bwd_ln": (C.c_int, [C.POINTER(GdfnShape), C.POINTER(GdfnParams), C.POINTER(LnTail), vp, vp, vp,
                                 C.POINTER(GdfnGrads), vp, vp, vp]),
    "mi_gdfn_fwd": (C.c_int, [C.POINTER(GdfnShape), C.POINTER(GdfnParams), vp, vp, vp, vp, vp, vp]),
    "mi_gdfn_bwd": (C.c_int, [C.POINTER(GdfnShape), C.POINTER(GdfnParams), vp, vp, vp, C.POINTER(GdfnGrads), vp, vp,
                              vp]),
    "mi_tksa_saved_bytes": (C.c_size_t, [C.POINTER(TksaShape)]),
    "mi_tksa_workspace": (C.c_size_t, [C.POINTER(TksaShape)]),
    "mi_tksa_fwd": (C.c_int, [C.POINTER(TksaShape), C.POINTER(MdtaParams), C.POINTER(TksaParams), vp, vp, vp, vp, vp, fp, vp]),
    "mi_tksa_bwd": (C.c_int, [C.POINTER(TksaShape), C.POINTER(MdtaParams), C.POINTER(TksaParams), vp, vp, vp, C.POINTER(MdtaGrads),
                              C.POINTER(TksaGrads), vp, vp, vp]),
    "mi_msfn_saved_bytes": (C.c_size_t, [C.POINTER(MsfnShape)]),
    "mi_msfn_workspace": (C.c_size_t, [C.POINTER(MsfnShape)]),
    "mi_msfn_fwd": (C.c_int, [C.POINTER(MsfnShape), C.POINTER(MsfnParams), vp, vp, vp, vp, vp, vp]),
    "mi_msfn_bwd": (C.c_int, [C.POINTER(MsfnShape), C.POINTER(MsfnParams), vp, vp, vp, C.POINTER(MsfnGrads), vp, vp, vp]),
    "mi_mefc_saved_bytes": (C.c_size_t, [C.POINTER(MefcShape)]),
    "mi_mefc_workspace": (C.c_size_t, [C.POINTER(MefcShape)]),
    "mi_mefc_fwd": (C.c_int, [C.POINTER(MefcShape), C.POINTER(MefcParams), vp, vp, vp, vp, vp]),
    "mi_mefc_bwd": (C.c_int, [C.POINTER(MefcShape), C.POINTER(MefcParams), vp, vp, vp, vp, C.POINTER(MefcGrads), vp, vp, vp]),
    "mi_dilgate_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(c_i64)]),
    "mi_dilgate_fwd_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_dilgate_fwd": (C.c_int, [vp, C.POINTER(DilgateParams), vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                 C.c_int, vp, vp]),
    "mi_dilgate_bwd_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_dilgate_bwd": (C.c_int, [vp, fp, vp, C.POINTER(DilgateParams), vp, C.POINTER(DilgateGrads), C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.POINTER(C.c_int), C.c_int, vp, vp]),
    "mi_pairconv3x3_fwd": (C.c_int, [vp, fp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_pairconv3x3_bwd_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_pairconv3x3_bwd": (C.c_int, [vp, vp, fp, vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi_dblock_saved_bytes": (C.c_size_t, [C.POINTER(DblockShape)]),
    "mi_dblock_workspace": (C.c_size_t, [C.POINTER(DblockShape)]),
    "mi_dblock_fwd": (C.c_int, [C.POINTER(DblockShape), C.POINTER(DblockParams), vp, vp, vp, vp, vp]),
    "mi_dblock_bwd": (C.c_int, [C.POINTER(DblockShape), C.POINTER(DblockParams), vp, vp, vp, C.POINTER(DblockGrads), vp, vp, vp]),
    "mi_gdfn_fused_ok": (C.c_int, [C.POINTER(GdfnFusedShape)]),
    "mi_gdfn_fused_pack_bytes": (C.c_size_t, [C.POINTER(GdfnFusedShape)]),
    "mi_gdfn_fused_pack": (C.c_int, [C.POINTER(GdfnFusedShape), fp, fp, C.POINTER(GdfnParams), vp, vp]),
    "mi_gdfn_fused_fwd": (C.c_int, [C.POINTER(GdfnFusedShape), vp, vp, vp, fp, fp, vp]),
    "mi_gdfn_fused_fwd_train_ok": (C.c_int, [C.POINTER(GdfnFusedShape)]),
    "mi_gdfn_fused_fwd_train": (C.c_int, [C.POINTER(GdfnFusedShape), vp, vp, vp, fp, fp, vp, vp]),
    "mi_gdfn_fused_fwd_f8": (C.c_int, [C.POINTER(GdfnFusedShape), vp, C.POINTER(F8Scales), vp, vp, vp]),
    "mi_gdfn_fused_plan": (C.c_int, [C.POINTER(GdfnFusedShape), C.c_int, C.POINTER(c_i64)]),
    "mi_mdta_fused_ok": (C.c_int, [C.POINTER(MdtaShape)]),
    "mi_mdta_fused_pays": (C.c_int, [C.POINTER(MdtaShape)]),
    "mi_mdta_fused_pack_bytes": (C.c_size_t, [C.POINTER(MdtaShape)]),
    "mi_mdta_fused_pack": (C.c_int, [C.POINTER(MdtaShape), fp, fp, C.POINTER(MdtaParams), vp, vp]),
    "mi_mdta_fused_workspace": (C.c_size_t, [C.POINTER(MdtaShape)]),
    "mi_mdta_fused_plan": (C.c_int, [C.POINTER(MdtaShape), C.POINTER(c_i64)]),
    "mi_mdta_fused_fwd": (C.c_int, [C.POINTER(MdtaShape), C.POINTER(MdtaParams), vp, C.c_int, vp, vp, vp, fp, fp, vp, vp]),
    "mi_adamw_step": (C.c_int, [fp, fp, fp, fp, c_i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                C.c_float, fp, vp]),
    "mi_grad_sumsq_workspace": (C.c_size_t, [c_i64]),
    "mi_grad_sumsq": (C.c_int, [fp, c_i64, fp, vp, vp]),
    "mi_adamw_step_ex": (C.c_int, [fp, fp, fp, fp, fp, c_i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                   C.c_float, fp, fp, C.c_float, fp, C.c_float, vp]),
    "mi_rows_gather": (C.c_int, [vp, vp, vp, C.c_int, c_i64, C.c_int, vp]),
    "mi_rows_gather_scaled": (C.c_int, [fp, vp, fp, vp, C.c_int, c_i64, C.c_int, vp]),
    "mi_rows_scatter_add": (C.c_int, [vp, vp, fp, vp, C.c_int, C.c_int, c_i64, C.c_int, C.c_int, vp]),
    "mi_rows_dot_workspace": (C.c_size_t, [C.c_int, c_i64]),
    "mi_rows_dot": (C.c_int, [fp, vp, vp, fp, C.c_int, c_i64, C.c_int, vp, vp]),
    "mi_glue3x3_ok": (C.c_int, [C.c_int, C.c_int]),
    "mi_conv3x3_ok": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "mi_conv3x3_pack_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mi_conv3x3_pack": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi_conv3x3_fwd": (C.c_int, [vp, vp, C.c_int64, fp, vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_conv3x3_wgrad_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_conv3x3_wgrad": (C.c_int, [vp, C.c_int64, vp, C.c_int64, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi_conv3x3_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(c_i64)]),
    "mi_chan_sum_workspace": (C.c_size_t, [C.c_int, C.c_int64]),
    "mi_chan_sum": (C.c_int, [vp, fp, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, vp, vp]),
    "mi_chan_sum_plan": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(c_i64)]),
    "mi_attn_small_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(c_i64)]),
    "mi_attn_small_fwd": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, fp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "mi_attn_small_bwd": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, fp, fp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "mi_im2col3x3": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_col2im3x3": (C.c_int, [vp, fp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_glue3x3_plan": (C.c_int, [c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(c_i64)]),
    "mi_grouped_pw_gemm": (C.c_int, [C.POINTER(GroupedProblem), C.c_int, vp, vp, C.c_int, c_i64, C.c_int, vp]),
    "mi_moe_route_fwd": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, fp, vp, fp, fp, vp, vp, vp, fp, vp, vp, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, vp]),
    "mi_moe_route_bwd": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, vp, fp, fp, vp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, vp]),
    "mi_patch_circconv": (C.c_int, [vp, c_i64, vp, c_i64, vp, c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_gelu_gap_fwd": (C.c_int, [vp, fp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_gelu_gap_bwd": (C.c_int, [vp, fp, vp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_ewise_fwd": (C.c_int, [vp, c_i64, vp, c_i64, vp, c_i64, c_i64, C.c_int, C.c_int, vp]),
    "mi_ewise_bwd": (C.c_int, [vp, c_i64, vp, c_i64, vp, vp, c_i64, vp, c_i64, c_i64, c_i64, C.c_int, C.c_int, vp]),
    "mi_pixel_shuffle2": (C.c_int, [vp, c_i64, vp, c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "mi_copy_rows": (C.c_int, [vp, c_i64, vp, c_i64, c_i64, c_i64, C.c_int, vp]),
    "mi_pixel_shuffle2_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_i64, c_i64, C.c_int, C.c_int, C.POINTER(c_i64)]),
    "mi_copy_rows_plan": (C.c_int, [c_i64, c_i64, c_i64, c_i64, C.c_int, C.c_int, C.POINTER(c_i64)]),
    "mi_patch_batch": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, fp, fp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "mi_psnr_ssim_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_psnr_ssim": (C.c_int, [vp, vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi_gap_fwd": (C.c_int, [vp, fp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_gap_bwd": (C.c_int, [fp, vp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_cast": (C.c_int, [vp, C.c_int, vp, C.c_int, c_i64, vp]),
    "mi_l1_loss": (C.c_int, [vp, vp, vp, fp, c_i64, C.c_float, C.c_int, vp]),
    "mi_fft_l1_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_fft_l1_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(c_i64)]),
    "mi_fft_l1_loss": (C.c_int, [vp, vp, vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp]),
    "mi_dft2_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_dft2_r2c": (C.c_int, [vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi_dft2_c2r": (C.c_int, [fp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "mi_fremlp_workspace": (C.c_size_t, [C.POINTER(FremlpShape)]),
    "mi_fremlp_saved_bytes": (C.c_size_t, [C.POINTER(FremlpShape)]),
    "mi_fremlp_plan": (C.c_int, [C.POINTER(FremlpShape), C.POINTER(c_i64)]),
    "mi_fremlp_fwd": (C.c_int, [C.POINTER(FremlpShape), fp, fp, fp, fp, vp, vp, vp, vp, vp]),
    "mi_fremlp_bwd": (C.c_int, [C.POINTER(FremlpShape), fp, fp, fp, vp, vp, fp, fp, fp, fp, C.c_int, vp, vp, vp]),
    "mi_fourier_unit_workspace": (C.c_size_t, [C.POINTER(FourierUnitShape)]),
    "mi_fourier_unit_saved_bytes": (C.c_size_t, [C.POINTER(FourierUnitShape)]),
    "mi_fourier_unit_plan": (C.c_int, [C.POINTER(FourierUnitShape), C.POINTER(c_i64)]),
    "mi_fourier_unit_fwd": (C.c_int, [C.POINTER(FourierUnitShape), C.POINTER(FourierUnitParams), vp, vp, fp, fp, vp, vp, vp]),
    "mi_fourier_unit_bwd": (C.c_int, [C.POINTER(FourierUnitShape), C.POINTER(FourierUnitParams), vp, vp, C.POINTER(FourierUnitGrads),
                                      vp, vp, vp]),
    "mi_sfh_ffn_workspace": (C.c_size_t, [C.POINTER(SfhFfnShape)]),
    "mi_sfh_ffn_saved_bytes": (C.c_size_t, [C.POINTER(SfhFfnShape)]),
    "mi_sfh_ffn_plan": (C.c_int, [C.POINTER(SfhFfnShape), C.POINTER(c_i64)]),
    "mi_sfh_ffn_fwd": (C.c_int, [C.POINTER(SfhFfnShape), C.POINTER(SfhFfnParams), vp, vp, vp, vp, vp]),
    "mi_sfh_ffn_bwd": (C.c_int, [C.POINTER(SfhFfnShape), C.POINTER(SfhFfnParams), vp, vp, vp, C.POINTER(SfhFfnGrads), vp, vp, vp]),
    "mi_sfh_local_workspace": (C.c_size_t, [C.POINTER(SfhLocalShape)]),
    "mi_sfh_local_plan": (C.c_int, [C.POINTER(SfhLocalShape), C.POINTER(c_i64)]),
    "mi_sfh_local_fwd": (C.c_int, [C.POINTER(SfhLocalShape), C.POINTER(SfhLocalParams), vp, vp, vp, vp]),
    "mi_sfh_local_bwd": (C.c_int, [C.POINTER(SfhLocalShape), C.POINTER(SfhLocalParams), vp, vp, vp, C.POINTER(SfhLocalGrads), vp, vp]),
    "mi_sfh_global_workspace": (C.c_size_t, [C.POINTER(SfhMixerShape)]),
    "mi_sfh_global_saved_bytes": (C.c_size_t, [C.POINTER(SfhMixerShape)]),
    "mi_sfh_global_plan": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(c_i64)]),
    "mi_sfh_global_fwd": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(SfhGlobalParams), vp, vp, fp, fp, vp, vp, vp]),
    "mi_sfh_global_bwd": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(SfhGlobalParams), vp, vp, vp, C.POINTER(SfhGlobalGrads), vp, vp,
                                    vp]),
    "mi_sfh_mixer_workspace": (C.c_size_t, [C.POINTER(SfhMixerShape)]),
    "mi_sfh_mixer_saved_bytes": (C.c_size_t, [C.POINTER(SfhMixerShape)]),
    "mi_sfh_mixer_plan": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(c_i64)]),
    "mi_sfh_mixer_fwd": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(SfhMixerParams), vp, vp, fp, fp, vp, vp, vp]),
    "mi_sfh_mixer_bwd": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(SfhMixerParams), vp, vp, vp, C.POINTER(SfhMixerGrads), vp, vp, vp]),
    "mi_bn2d_workspace": (C.c_size_t, [C.POINTER(Bn2dShape)]),
    "mi_bn2d_plan": (C.c_int, [C.POINTER(Bn2dShape), C.POINTER(c_i64)]),
    "mi_bn2d_fwd": (C.c_int, [C.POINTER(Bn2dShape), fp, fp, vp, vp, fp, fp, fp, fp, vp, vp]),
    "mi_bn2d_bwd": (C.c_int, [C.POINTER(Bn2dShape), fp, vp, vp, vp, vp, fp, fp, C.c_int, fp, vp, vp]),
    "mi_scale_res_workspace": (C.c_size_t, [C.POINTER(Bn2dShape)]),
    "mi_scale_res_plan": (C.c_int, [C.POINTER(Bn2dShape), C.POINTER(c_i64)]),
    "mi_scale_res_fwd": (C.c_int, [C.POINTER(Bn2dShape), fp, vp, vp, vp, fp, vp]),
    "mi_scale_res_bwd": (C.c_int, [C.POINTER(Bn2dShape), fp, vp, vp, vp, fp, C.c_int, vp, vp]),
    "mi_sfh_block_workspace": (C.c_size_t, [C.POINTER(SfhMixerShape)]),
    "mi_sfh_block_saved_bytes": (C.c_size_t, [C.POINTER(SfhMixerShape)]),
    "mi_sfh_block_plan": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(c_i64)]),
    "mi_sfh_block_fwd": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(SfhBlockParams), vp, vp, C.POINTER(SfhBlockStats), fp, fp, vp, vp, vp]),
    "mi_sfh_block_bwd": (C.c_int, [C.POINTER(SfhMixerShape), C.POINTER(SfhBlockParams), vp, vp, vp, C.POINTER(SfhBlockGrads), vp, vp, vp]),
    "mi_fregate_fwd": (C.c_int, [vp, vp, fp, vp, C.c_int, C.c_int, c_i64, C.c_int, vp]),
    "mi_fregate_bwd_workspace": (C.c_size_t, [C.c_int, C.c_int, c_i64]),
    "mi_fregate_bwd": (C.c_int, [vp, vp, vp, fp, vp, vp, fp, C.c_int, C.c_int, c_i64, C.c_int, C.c_int, vp, vp]),
    "mi_eblock_saved_bytes": (C.c_size_t, [C.POINTER(EblockShape)]),
    "mi_eblock_workspace": (C.c_size_t, [C.POINTER(EblockShape)]),
    "mi_eblock_plan": (C.c_int, [C.POINTER(EblockShape), C.POINTER(c_i64)]),
    "mi_eblock_fwd": (C.c_int, [C.POINTER(EblockShape), C.POINTER(EblockParams), vp, vp, vp, vp, vp]),
    "mi_eblock_bwd": (C.c_int, [C.POINTER(EblockShape), C.POINTER(EblockParams), vp, vp, vp, C.POINTER(EblockGrads), vp, vp, vp]),
    "mi_ssim_loss_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_ssim_loss": (C.c_int, [vp, vp, vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp]),
    "mi_edge_loss_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mi_edge_loss": (C.c_int, [vp, vp, vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp]),
    "mi_focal_l1_workspace": (C.c_size_t, [c_i64]),
    "mi_focal_l1_loss": (C.c_int, [vp, vp, vp, fp, c_i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, vp, vp]),
    "mi_prof_enable": (C.c_int, [C.c_int]),
    "mi_prof_kernel_count": (C.c_int, []),
    "mi_prof_kernel_name": (C.c_char_p, [C.c_int]),
    "mi_prof_collect": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(c_i64), C.c_int]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """The loaded library; raises RuntimeError (never falls back) when it is missing or incomplete."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().mi_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"mi_restore {what} failed (rc={rc}): {msg}")
