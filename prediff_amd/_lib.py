"""ctypes binding of libprediff_hip.so (include/prediff_hip.h) + thin tensor-level wrappers.

PyTorch is used here only as the owner of device memory and streams: every wrapper passes raw
device pointers and the current HIP stream to the C ABI.  There is NO fallback: if the shared
library is missing or a kernel reports an error, an exception is raised.
"""
import ctypes as C
import os
from typing import Optional

import torch

from .packing import pad64  # noqa: F401  (re-exported: L.pad64)

_HERE = os.path.dirname(os.path.abspath(__file__))
# PD_LIB_PATH: another build of the same library (A/B of compiler flags); the default is the in-tree build
LIB_PATH = os.environ.get("PD_LIB_PATH") or os.path.join(_HERE, "libprediff_hip.so")

ABI_VERSION = 4          # pd_abi_version() of the library this binding was written for

ACT = {"none": 0, None: 0, "identity": 0, "gelu": 1, "silu": 2, "leaky": 3, "relu": 4}


class PrediffHipError(RuntimeError):
    pass


class IgemmArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("A", "A_lo", "W", "W_lo", "bias", "rowvec", "residual", "mul", "out_f32", "out_bf16", "out_bf16_lo")] + \
               [(n, C.c_int64) for n in
                ("a_batch_stride", "w_batch_stride", "out_batch_stride", "outb_batch_stride", "res_batch_stride",
                 "w_tap_stride")] + \
               [(n, C.c_int32) for n in
                ("nbatch", "M", "N", "Cin", "taps", "lda", "ldw", "B", "Ti", "Hi", "Wi", "To", "Ho", "Wo",
                 "KT", "KH", "KW", "st", "sh", "sw", "pt", "ph", "pw", "ut", "uh", "uw", "vT", "vH", "vW",
                 "rows_per_sample", "ld_rowvec", "ld_res", "res_period", "ld_mul", "act", "ld_out", "ld_outb", "split")] + \
               [("alpha", C.c_float), ("tile", C.c_int32), ("vec_epilogue", C.c_int32), ("a_bytes", C.c_uint32), ("w_bytes", C.c_uint32), ("debug_flags", C.c_int32), ("ksplit", C.c_int32),
                ("splitk_ws", C.c_void_p), ("splitk_ws_elems", C.c_int64), ("fp8", C.c_int32), ("out_fp8_log2", C.c_int32),
                ("operand", C.c_int32), ("disable_256", C.c_int32), ("min_k_256", C.c_int32), ("splitk_max_tiles", C.c_int32),
                ("w_fold", C.c_int32), ("rowtab_rows", C.c_int32), ("rowtab", C.c_void_p)]


class CuboidAttnArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("qkv_bf16", "qkv_f32", "tok_index", "bias", "mask", "out_bf16", "out_bf16_lo", "out_f32")] + \
               [(n, C.c_int32) for n in ("B", "ntok", "C", "heads", "nc", "vol", "ld_qkv", "ld_out")] + \
               [("scale", C.c_float), ("force_generic", C.c_int32), ("out_fp8_log2", C.c_int32), ("tok_out", C.c_void_p),
                ("operand", C.c_int32), ("qkv_fp8_log2", C.c_int32)]


class MxOperands(C.Structure):
    """pd_mx_operands: the E8M0 block scales of the two operands of a pd_igemm_mx launch"""
    _fields_ = [("a_scales", C.c_void_p), ("w_scales", C.c_void_p), ("w_scale_tap_stride", C.c_int64), ("ld_a_scales", C.c_int32),
                ("ld_w_scales", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


TIME_EMBED_MAX_PROJ = 8                     # PD_TIME_EMBED_MAX_PROJ
OPERAND = {"bf16": 0, "fp16": 1}            # enum pd_operand


class CallOpts(C.Structure):
    """pd_call_opts: the per-call options of the library (operand type + A/B switches + profiling hooks).  A module owns one instance and
    passes it on every launch: nothing is process-global.  All-zero = bfloat16 operands, production settings.  `igemm_*` are host-side
    defaults the `igemm` wrapper copies into pd_igemm_args (the library's own struct has no such members)."""
    _fields_ = [(n, C.c_int32) for n in ("operand", "attn_block_table_ids", "ffn_rows128", "groupnorm_two_launches", "pair_form",
                                         "ffn_debug_flags", "attn_block_debug_flags", "small_grid", "w_fold", "reserved1")] + [("trace", C.c_void_p)]

    def __init__(self, operand="bf16", **kw):
        super().__init__()
        self.operand = OPERAND[operand] if isinstance(operand, str) else int(operand)
        # pd_igemm_args members a caller may preset for every pd_igemm launch made with these options (A/B switches of bench.py / scripts)
        self.igemm_tile = self.igemm_debug_or = self.igemm_disable_256 = self.igemm_min_k_256 = self.igemm_splitk_max_tiles = 0
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def dtype(self):
        """torch dtype of the 16-bit operand buffers these options describe"""
        return torch.float16 if self.operand == OPERAND["fp16"] else torch.bfloat16

    _HOST_FIELDS = ("igemm_tile", "igemm_debug_or", "igemm_disable_256", "igemm_min_k_256", "igemm_splitk_max_tiles")

    def _state(self):
        """every member but `trace` (a device pointer of a profiling run: meaningless in a copy or another process)"""
        st = {n: getattr(self, n) for n, _ in self._fields_ if n != "trace"}
        st.update({n: getattr(self, n) for n in self._HOST_FIELDS})
        return st

    def replace(self, **kw):
        """a copy with some members changed (the options a module passes are never mutated per launch)"""
        st = self._state()
        st["trace"] = self.trace
        st.update(kw)
        return CallOpts(**st)

    def __reduce__(self):
        # ctypes refuses to pickle structures holding pointers; a module that owns a CallOpts must stay deepcopy- / pickle-able
        # (EMA by deepcopy, DDP spawn, torch.save(module))
        return (_callopts_from_state, (self._state(),))


def _callopts_from_state(st):
    return CallOpts(**st)


def _opts_ref(opts):
    return C.byref(opts) if opts is not None else None


_lib = None

_PROTOS = {
    "pd_abi_version": (C.c_int, []),
    "pd_last_error": (C.c_char_p, []),
    "pd_sizeof_igemm_args": (C.c_int, []),
    "pd_sizeof_cuboid_attn_args": (C.c_int, []),
    "pd_sizeof_call_opts": (C.c_int, []),
    "pd_igemm": (C.c_int, [C.POINTER(IgemmArgs), C.c_void_p]),
    "pd_sizeof_mx_operands": (C.c_int, []),
    "pd_igemm_mx": (C.c_int, [C.POINTER(IgemmArgs), C.POINTER(MxOperands), C.c_void_p]),
    "pd_quantize_mx": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pd_layernorm_mx": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "pd_groupnorm_silu_mx": (C.c_int, [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_void_p]),
    "pd_layernorm": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_int, C.c_float, C.POINTER(CallOpts), C.c_void_p]),
    "pd_layernorm_fp8": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "pd_patch_merge_layernorm": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 9 + [C.c_float, C.c_void_p]),
    "pd_patch_merge_layernorm_ex": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 9 + [C.c_float, C.c_int, C.POINTER(CallOpts), C.c_void_p]),
    "pd_groupnorm_nchunk": (C.c_int, [C.c_int, C.c_int]),
    "pd_groupnorm_silu": (C.c_int, [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 5 +
                          [C.c_float, C.c_int, C.POINTER(CallOpts), C.c_void_p]),
    "pd_groupnorm_stats": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_float, C.c_void_p]),
    "pd_conv2d_gn_silu_supported": (C.c_int, [C.c_int] * 5),
    "pd_conv2d_gn_silu": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 6 + [C.POINTER(CallOpts), C.c_void_p]),
    "pd_conv2d_up2": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.POINTER(CallOpts), C.c_void_p]),
    "pd_groupnorm_silu_fp8": (C.c_int, [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_float, C.c_void_p]),
    "pd_groupnorm_silu_bwd": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_void_p]),
    "pd_cast_rows": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_int] * 6 + [C.POINTER(CallOpts), C.c_void_p]),
    "pd_cuboid_attention": (C.c_int, [C.POINTER(CuboidAttnArgs), C.c_void_p]),
    "pd_cuboid_attention_bwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 9 + [C.c_float, C.c_void_p]),
    "pd_softmax_rows": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_int] * 3 + [C.POINTER(CallOpts), C.c_void_p]),
    "pd_unet_build_input": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]),
    "pd_unet_build_input16": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p]),
    "pd_timestep_embedding": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p]),
    "pd_linear_small": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]),
    "pd_time_embed_supported": (C.c_int, [C.c_int, C.c_int]),
    "pd_time_embed": (C.c_int, [C.c_void_p] * 10 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "pd_add_rowtable": (C.c_int, [C.c_void_p] * 2 + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "pd_add": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "pd_ddpm_step": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_int, C.c_void_p]),
    "pd_ddim_step": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_ddim_step_guided": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_dpmpp_2m_step": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_dpmpp_2m_step_guided": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_dpmpp_2m_sde_step": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_dpmpp_2m_sde_step_guided": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_ddim_step_held": (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_dpmpp_2m_step_held": (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_dpmpp_2m_sde_step_held": (C.c_int, [C.c_void_p] * 10 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_hold_blend": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int64, C.c_void_p]),
    "pd_window_gather": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 8 + [C.c_void_p]),
    "pd_window_blend": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 8 + [C.c_void_p]),
    "pd_context_advance": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 10 + [C.c_float] + [C.c_int] * 3 + [C.c_void_p]),
    "pd_sevir_ingest": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 10 + [C.c_float] * 2 + [C.c_void_p]),
    "pd_sevir_export": (C.c_int, [C.c_void_p] * 2 + [C.c_int64] + [C.c_int] * 3 + [C.c_float] * 2 + [C.c_int, C.c_void_p]),
    "pd_lk_ws_bytes": (C.c_int64, [C.c_int64] + [C.c_int] * 7),
    "pd_lk_motion": (C.c_int, [C.c_void_p] * 2 + [C.c_int64] + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "pd_advect": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_int] * 3 + [C.c_int64, C.c_float, C.c_void_p]),
    "pd_steps_ws_bytes": (C.c_int64, [C.c_int64] + [C.c_int] * 5),
    "pd_steps_analyse": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_int] * 5 + [C.c_float] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]),
    "pd_steps_evolve": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int64] + [C.c_int] * 5 + [C.c_void_p] * 2 + [C.c_int64, C.c_void_p]),
    "pd_steps_finish": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int64] + [C.c_int] * 4 + [C.c_float] + [C.c_int] * 2 + [C.c_void_p]),
    "pd_anvil_ws_bytes": (C.c_int64, [C.c_int64] + [C.c_int] * 4),
    "pd_anvil_analyse": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_double, C.c_int64] + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "pd_anvil_evolve": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_int] * 5 + [C.c_void_p] * 2 + [C.c_int64, C.c_void_p]),
    "pd_nchw_to_nhwc": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "pd_nhwc_to_nchw": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "pd_ffn_fused_supported": (C.c_int, [C.c_int, C.c_int]),
    "pd_attn_block_fused_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "pd_attn_block_fused": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 6 + [C.c_float, C.c_float, C.c_void_p]),
    "pd_attn_block_fused_ex": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 6 + [C.c_float, C.c_float, C.c_void_p, C.POINTER(CallOpts), C.c_void_p]),
    "pd_ffn_fused": (C.c_int, [C.c_void_p] * 8 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(CallOpts), C.c_void_p]),
    "pd_attn_ffn_pair_supported": (C.c_int, [C.c_int] * 5),
    "pd_attn_ffn_pair_cuboids_per_group": (C.c_int, [C.c_int]),
    "pd_attn_ffn_pair": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_float] * 3 + [C.POINTER(CallOpts), C.c_void_p]),
    "pd_attn_ffn_pair_split_ws_floats": (C.c_int64, [C.c_int] * 3),
    "pd_attn_ffn_pair_split": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_float] * 3 + [C.c_void_p, C.c_int64, C.POINTER(CallOpts), C.c_void_p]),
    "pd_ffn_rows_supported": (C.c_int, [C.c_int] * 3),
    "pd_ffn_rows": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_float, C.POINTER(CallOpts), C.c_void_p]),
    "pd_sevir_skill_counts": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_float, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    "pd_sevir_skill_counts_pooled": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_float] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]),
    "pd_ensemble_score_ws_doubles": (C.c_int64, [C.c_int, C.c_void_p, C.c_int]),
    "pd_ensemble_score_update": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int]
                                 + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
    "pd_frame_score_ws_doubles": (C.c_int64, [C.c_int, C.c_void_p]),
    "pd_frame_score_update": (C.c_int, [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_int]
                              + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "pd_spectrum_ws_bytes": (C.c_int64, [C.c_int, C.c_void_p]),
    "pd_spectrum_update": (C.c_int, [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p] * 3
                           + [C.c_int64, C.c_void_p]),
    "pd_objects_ws_bytes": (C.c_int64, [C.c_int, C.c_void_p]),
    "pd_objects_label": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 3
                         + [C.c_int, C.c_void_p]),
    "pd_sal_update": (C.c_int, [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_int, C.c_float] + [C.c_int] * 3
                      + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "pd_pm_ws_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int]),
    "pd_rank_frames": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 3),
    "pd_cdf_match": (C.c_int, [C.c_void_p] * 2 + [C.c_int64] * 2 + [C.c_int] * 4 + [C.c_float, C.c_int] + [C.c_void_p] * 2
                     + [C.c_int64, C.c_void_p]),
    "pd_pmm": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_int64, C.c_void_p]),
    "pd_distance_ws_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_void_p]),
    "pd_distance_map": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "pd_distance_update": (C.c_int, [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_float, C.c_int, C.c_double, C.c_int]
                           + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "pd_scale_ws_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_void_p]),
    "pd_scale_energy": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "pd_scale_update": (C.c_int, [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 3
                        + [C.c_int64, C.c_void_p]),
    "pd_i3d_preprocess": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.POINTER(CallOpts), C.c_void_p]),
    "pd_maxpool3d_same": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 14 + [C.POINTER(CallOpts), C.c_void_p]),
    "pd_i3d_head": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]),
    "pd_feature_moments_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)


def lib():
    """Load the shared library (once).  Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PrediffHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C prediff_amd/csrc`. prediff_amd has no non-HIP execution path.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            f = getattr(l, name)      # AttributeError if a declared symbol is missing
            f.restype = res
            f.argtypes = args
        if (l.pd_sizeof_igemm_args() != C.sizeof(IgemmArgs) or l.pd_sizeof_cuboid_attn_args() != C.sizeof(CuboidAttnArgs)
                or l.pd_sizeof_call_opts() != C.sizeof(CallOpts) or l.pd_sizeof_mx_operands() != C.sizeof(MxOperands)
                or l.pd_abi_version() != ABI_VERSION):
            raise PrediffHipError(f"{LIB_PATH} is stale: its ABI version / argument structs do not match prediff_amd/_lib.py "
                                  f"(rebuild with `make -C prediff_amd/csrc`)")
        _lib = l
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        raise PrediffHipError(f"{what} failed (status {rc}): {lib().pd_last_error().decode()}")


def stream_ptr() -> int:
    """The current HIP stream of the current device.  Every module entry point (forward / encode / decode / sample / update) runs
    inside `on_device(x)`, which makes the operands' device the current one, so this is the stream of the tensors' device."""
    return torch.cuda.current_stream().cuda_stream


def on_device(t: torch.Tensor):
    """Context manager: make `t`'s device current (kernels are launched on the current stream of the current device; a module on
    cuda:1 called while cuda:0 is current must not launch on a device-0 stream with device-1 pointers)."""
    if not t.is_cuda:
        raise PrediffHipError("prediff_amd kernels need CUDA(HIP) tensors; got a CPU tensor")
    return torch.cuda.device(t.device)


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dev(t: torch.Tensor, dtype=None):
    if not t.is_cuda:
        raise PrediffHipError("prediff_amd kernels need CUDA(HIP) tensors; got a CPU tensor")
    if dtype is not None and t.dtype != dtype:
        raise PrediffHipError(f"expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise PrediffHipError("expected a contiguous tensor")
    return t


# --------------------------------------------------------------------------------------------------
# wrappers
# --------------------------------------------------------------------------------------------------
def igemm(A, W, *, M, N, Cin, lda=None, ldw=None, taps=1, w_tap_stride=0, geom=None,
          A_lo=None, W_lo=None, bias=None, rowvec=None, rows_per_sample=0, residual=None, res_period=0,
          ld_res=None, mul=None, act="none", alpha=1.0, out_f32=None, out_bf16=None, out_bf16_lo=None,
          ld_out=None, ld_outb=None, nbatch=1, a_batch_stride=0, w_batch_stride=0, out_batch_stride=0,
          outb_batch_stride=0, res_batch_stride=0, tile=0, debug_flags=0, splitk_ws=None, fp8=False, out_fp8_log2=0, rowtab=None,
          opts=None):
    """Thin wrapper around pd_igemm.  `geom` = dict(B,Ti,Hi,Wi,To,Ho,Wo,KT,KH,KW,st,sh,sw,pt,ph,pw,ut,uh,uw) or None
    for a plain linear layer.  `opts` (CallOpts): the operand type of A / W / out_bf16 and the caller's A/B presets for this launch."""
    a = _igemm_args(**{k: v for k, v in locals().items()})
    _check(lib().pd_igemm(C.byref(a), stream_ptr()), "pd_igemm")


def _igemm_args(A, W, *, M, N, Cin, lda, ldw, taps, w_tap_stride, geom, A_lo, W_lo, bias, rowvec, rows_per_sample, residual, res_period,
                ld_res, mul, act, alpha, out_f32, out_bf16, out_bf16_lo, ld_out, ld_outb, nbatch, a_batch_stride, w_batch_stride,
                out_batch_stride, outb_batch_stride, res_batch_stride, tile, debug_flags, splitk_ws, fp8, out_fp8_log2, rowtab, opts):
    """pd_igemm_args of a launch (the keywords of `igemm`)"""
    a = IgemmArgs()
    if opts is not None:
        a.operand = 0 if fp8 else opts.operand          # (e4m3 operands: the 16-bit OUTPUT of such a launch is bfloat16)
        tile = tile or opts.igemm_tile
        debug_flags |= opts.igemm_debug_or
        a.disable_256, a.min_k_256, a.splitk_max_tiles = opts.igemm_disable_256, opts.igemm_min_k_256, opts.igemm_splitk_max_tiles
    a.A, a.A_lo, a.W, a.W_lo = ptr(A), ptr(A_lo), ptr(W), ptr(W_lo)
    a.bias, a.rowvec, a.residual, a.mul = ptr(bias), ptr(rowvec), ptr(residual), ptr(mul)
    a.out_f32, a.out_bf16, a.out_bf16_lo = ptr(out_f32), ptr(out_bf16), ptr(out_bf16_lo)
    a.a_batch_stride, a.w_batch_stride = a_batch_stride, w_batch_stride
    a.out_batch_stride, a.outb_batch_stride, a.res_batch_stride = out_batch_stride, outb_batch_stride, res_batch_stride
    a.w_tap_stride = w_tap_stride
    a.lda = lda if lda is not None else Cin
    a.ldw = ldw if ldw is not None else Cin
    if getattr(W, "_pd_fold", False):
        # packing.fold_weights: W = the `taps` slabs of W_hi followed by the `taps` slabs of W_lo -- two weight products per tap against one
        # activation gather (precision="fp16x2"); the caller describes the layer as it would for a single product
        if A_lo is not None or W_lo is not None or fp8:
            raise PrediffHipError("pd_igemm: folded (hi + lo) weights go with single-rounded 16-bit activations only")
        a.w_fold = taps
        w_tap_stride = w_tap_stride or N * a.ldw
        a.w_tap_stride = w_tap_stride
        taps = 2 * taps
    a.nbatch, a.M, a.N, a.Cin, a.taps = nbatch, M, N, Cin, taps
    if geom is None:
        geom = dict(B=1, Ti=1, Hi=1, Wi=M, To=1, Ho=1, Wo=M, KT=1, KH=1, KW=1, st=1, sh=1, sw=1, pt=0, ph=0, pw=0,
                    ut=1, uh=1, uw=1)
    for k, v in geom.items():
        setattr(a, k, v)
    a.rows_per_sample = rows_per_sample
    a.ld_rowvec = N if rowvec is None else rowvec.shape[-1]
    a.ld_res = ld_res if ld_res is not None else N
    a.res_period = res_period
    a.ld_mul = N
    a.act = ACT[act]
    a.ld_out = ld_out if ld_out is not None else N
    a.ld_outb = ld_outb if ld_outb is not None else N
    a.split = 1 if A_lo is not None else 0
    a.alpha = alpha
    a.tile = tile
    a.debug_flags = debug_flags
    a.fp8 = 1 if fp8 else 0           # A / W are e4m3 bytes (torch.float8_e4m3fn); tensor scales in alpha
    a.out_fp8_log2 = out_fp8_log2     # k > 0: out_bf16 is an e4m3 byte tensor receiving e4m3(v * 2^k)
    if rowtab is not None:          # fp32 (rows, N): out row m += rowtab[m % rows], after the residual (pd_add_rowtable's bits)
        if rowtab.dim() != 2 or rowtab.shape[1] != N:
            raise PrediffHipError(f"pd_igemm: the row table must be (rows, N = {N}); got {tuple(rowtab.shape)}")
        a.rowtab, a.rowtab_rows = ptr(_dev(rowtab, torch.float32)), rowtab.shape[0]
    if splitk_ws is not None:       # fp32 workspace: lets the library split the K loop of small-grid, long-K launches
        a.splitk_ws, a.splitk_ws_elems = ptr(splitk_ws), splitk_ws.numel()
    return a


def _mx_pair(t, s, what):
    """payload / scale arrays of an MX operand: (rows..., ld) e4m3 bytes and (rows..., ld / 32) uint8, on the GPU, contiguous"""
    if t.dtype not in (torch.float8_e4m3fn, torch.uint8):
        raise PrediffHipError(f"{what}: the MX payload must be float8_e4m3fn (or raw uint8) bytes, got {t.dtype}")
    _dev(t)
    _dev(s, torch.uint8)
    if s.device != t.device:
        raise PrediffHipError(f"{what}: payload and scales live on different devices")
    ld = t.shape[-1]
    if ld % 32 or tuple(s.shape) != tuple(t.shape[:-1]) + (ld // 32,):
        raise PrediffHipError(f"{what}: scales {tuple(s.shape)} do not match one byte per 32 elements of payload {tuple(t.shape)}")
    return ld


def igemm_mx(A, a_scales, W, w_scales, *, M, N, taps=1, geom=None, bias=None, rowvec=None, rows_per_sample=0, residual=None, res_period=0,
             ld_res=None, mul=None, act="none", alpha=1.0, out_f32=None, out_bf16=None, ld_out=None, ld_outb=None, debug_flags=0,
             splitk_ws=None, opts=None):
    """pd_igemm_mx: the implicit GEMM on MX operands -- e4m3 payloads A (input rows, ld) and W ((taps,) N, ld) with their E8M0 block
    scales (packing.quantize_mx / pack_linear_mx / pack_conv_mx, or the *_mx producers); ld % 128 == 0.  A 16-bit output is bfloat16."""
    lda, ldw = _mx_pair(A, a_scales, "pd_igemm_mx A"), _mx_pair(W, w_scales, "pd_igemm_mx W")
    if lda != ldw or lda % 128:
        raise PrediffHipError(f"pd_igemm_mx: A rows of {lda} and W rows of {ldw} bytes: both operands need the same row length, a multiple of 128")
    if W.numel() != taps * N * ldw:
        raise PrediffHipError(f"pd_igemm_mx: W {tuple(W.shape)} is not ({taps}, {N}, {ldw})")
    rows_in = M if geom is None else geom["B"] * geom["Ti"] * geom["Hi"] * geom["Wi"]
    if A.numel() != rows_in * lda:
        raise PrediffHipError(f"pd_igemm_mx: A {tuple(A.shape)} is not ({rows_in}, {lda})")
    presets = dict(debug_flags=debug_flags | (opts.igemm_debug_or if opts is not None else 0))
    a = _igemm_args(A, W, M=M, N=N, Cin=lda, lda=lda, ldw=ldw, taps=taps, w_tap_stride=N * ldw if taps > 1 else 0, geom=geom, A_lo=None,
                    W_lo=None, bias=bias, rowvec=rowvec, rows_per_sample=rows_per_sample, residual=residual, res_period=res_period,
                    ld_res=ld_res, mul=mul, act=act, alpha=alpha, out_f32=out_f32, out_bf16=out_bf16, out_bf16_lo=None, ld_out=ld_out,
                    ld_outb=ld_outb, nbatch=1, a_batch_stride=0, w_batch_stride=0, out_batch_stride=0, outb_batch_stride=0,
                    res_batch_stride=0, tile=0, splitk_ws=splitk_ws, fp8=False, out_fp8_log2=0, rowtab=None, opts=None, **presets)
    if opts is not None:
        a.disable_256, a.splitk_max_tiles = 0, opts.igemm_splitk_max_tiles
    m = MxOperands()
    m.a_scales, m.w_scales = ptr(a_scales), ptr(w_scales)
    m.ld_a_scales, m.ld_w_scales = lda // 32, ldw // 32
    m.w_scale_tap_stride = N * (ldw // 32) if taps > 1 else 0
    _check(lib().pd_igemm_mx(C.byref(a), C.byref(m), stream_ptr()), "pd_igemm_mx")


def quantize_mx(x, q, scales, rows, K, ld=None, ld_x=None):
    """fp32 rows -> MX e4m3 (pd_quantize_mx): q (rows, ld) payload, scales (rows, ld / 32); columns [K, ld) are padding."""
    _dev(x, torch.float32)
    ld = _mx_pair(q, scales, "pd_quantize_mx") if ld is None else ld
    ld_x = K if ld_x is None else ld_x
    if K % 32:
        raise PrediffHipError(f"pd_quantize_mx: K = {K} is not a multiple of 32 (one scale per 32 elements)")
    if x.numel() < rows * ld_x or q.numel() != rows * ld or scales.numel() != rows * (ld // 32):
        raise PrediffHipError(f"pd_quantize_mx: x {tuple(x.shape)} / q {tuple(q.shape)} / scales {tuple(scales.shape)} do not hold {rows} rows of {K} (ld {ld})")
    _check(lib().pd_quantize_mx(ptr(x), ptr(q), ptr(scales), rows, K, ld_x, ld, stream_ptr()), "pd_quantize_mx")


def layernorm_mx(x, gamma, beta, out, scales, rows, Cn, eps=1e-5):
    """LayerNorm -> MX e4m3 rows (pd_layernorm_mx): the A operand of a pd_igemm_mx linear."""
    ld = _mx_pair(out, scales, "pd_layernorm_mx")
    for t in (x, gamma, beta):
        _dev(t, torch.float32)
    if out.numel() != rows * ld or x.numel() != rows * Cn:
        raise PrediffHipError(f"pd_layernorm_mx: x {tuple(x.shape)} / out {tuple(out.shape)} do not hold {rows} rows of {Cn}")
    _check(lib().pd_layernorm_mx(ptr(x), ptr(gamma), ptr(beta), ptr(out), ptr(scales), rows, Cn, ld, eps, stream_ptr()), "pd_layernorm_mx")


def groupnorm_silu_mx(x, gamma, beta, partials, out, scales, B, S, Cn, G, eps, silu=True, ss_scale=None, ss_shift=None, ld_ss=0):
    """GroupNorm [-> scale-shift] [-> SiLU] -> MX e4m3 rows (pd_groupnorm_silu_mx): the A operand of a pd_igemm_mx convolution."""
    ld = _mx_pair(out, scales, "pd_groupnorm_silu_mx")
    for t in (x, gamma, beta):
        _dev(t, torch.float32)
    _dev(partials, torch.float64)
    if out.numel() != B * S * ld or x.numel() != B * S * Cn or partials.numel() < B * groupnorm_nchunk(S, Cn) * G * 2:
        raise PrediffHipError(f"pd_groupnorm_silu_mx: x {tuple(x.shape)} / out {tuple(out.shape)} / partials do not hold {B} x {S} rows of {Cn}")
    _check(lib().pd_groupnorm_silu_mx(ptr(x), ptr(gamma), ptr(beta), ptr(ss_scale), ptr(ss_shift), ld_ss, ptr(partials), ptr(out),
                                      ptr(scales), B, S, Cn, G, ld, eps, 1 if silu else 0, stream_ptr()), "pd_groupnorm_silu_mx")


def conv_geom(B, in_thw, kernel, stride=(1, 1, 1), pad=(1, 1, 1), up=(1, 1, 1), out_thw=None, virt_thw=None):
    """virt_thw: size of the nearest-up-sampled input when it is not exactly in_thw*up (odd target sizes)."""
    Ti, Hi, Wi = in_thw
    KT, KH, KW = kernel
    if out_thw is None:
        v = virt_thw if virt_thw is not None else tuple(s * u for s, u in zip(in_thw, up))
        out_thw = tuple((s + 2 * p - k) // st + 1 for s, p, k, st in zip(v, pad, kernel, stride))
    To, Ho, Wo = out_thw
    vt, vh, vw = virt_thw if virt_thw is not None else (0, 0, 0)
    return dict(vT=vt, vH=vh, vW=vw, B=B, Ti=Ti, Hi=Hi, Wi=Wi, To=To, Ho=Ho, Wo=Wo, KT=KT, KH=KH, KW=KW, st=stride[0], sh=stride[1],
                sw=stride[2], pt=pad[0], ph=pad[1], pw=pad[2], ut=up[0], uh=up[1], uw=up[2])


def layernorm(x, gamma, beta, out, out_lo, rows, Cn, ld_out, eps=1e-5, opts=None):
    _check(lib().pd_layernorm(ptr(x), ptr(gamma), ptr(beta), ptr(out), ptr(out_lo), rows, Cn, ld_out, eps, _opts_ref(opts), stream_ptr()),
           "pd_layernorm")


def layernorm_fp8(x, gamma, beta, out, rows, Cn, ld_out, fp8_scale, eps=1e-5):
    """LayerNorm -> e4m3 rows (value * fp8_scale, saturating): the A operand of an fp8 pd_igemm launch."""
    _check(lib().pd_layernorm_fp8(ptr(x), ptr(gamma), ptr(beta), ptr(out), rows, Cn, ld_out, eps, fp8_scale, stream_ptr()),
           "pd_layernorm_fp8")


def patch_merge_layernorm(x, gamma, beta, out, out_lo, B, T, H, W, Cn, ds, ld_out, eps=1e-5, pad_nearest=False, opts=None):
    _check(lib().pd_patch_merge_layernorm_ex(ptr(x), ptr(gamma), ptr(beta), ptr(out), ptr(out_lo), B, T, H, W, Cn,
                                             ds[0], ds[1], ds[2], ld_out, eps, 1 if pad_nearest else 0, _opts_ref(opts), stream_ptr()),
           "pd_patch_merge_layernorm")


def groupnorm_nchunk(S, Cn):
    return lib().pd_groupnorm_nchunk(S, Cn)


def groupnorm_silu(x, gamma, beta, partials, out, out_lo, B, S, Cn, G, ld_out, eps, silu=True, ss_scale=None,
                   ss_shift=None, ld_ss=0, opts=None):
    _check(lib().pd_groupnorm_silu(ptr(x), ptr(gamma), ptr(beta), ptr(ss_scale), ptr(ss_shift), ld_ss, ptr(partials),
                                   ptr(out), ptr(out_lo), B, S, Cn, G, ld_out, eps, 1 if silu else 0, _opts_ref(opts), stream_ptr()),
           "pd_groupnorm_silu")


def groupnorm_stats(x, partials, stats, B, S, Cn, G, eps):
    """stats (B, G, 2) fp32 = {mean, rstd} of GroupNorm(G, Cn, eps) over channels-last x (B, S, Cn)."""
    _check(lib().pd_groupnorm_stats(ptr(x), ptr(partials), ptr(stats), B, S, Cn, G, eps, stream_ptr()), "pd_groupnorm_stats")


def conv2d_gn_silu_supported(H, W, Cin, Cout, G):
    return bool(lib().pd_conv2d_gn_silu_supported(H, W, Cin, Cout, G))


def conv2d_gn_silu(x, stats, gamma, beta, W, bias, residual, out, N, H, Wd, Cin, Cout, G, opts=None):
    """GroupNorm -> SiLU -> Conv2d 3x3 (+ bias, + fp32 residual) in one launch (csrc/conv2d_gn.hip): the VAE ResBlock body."""
    _check(lib().pd_conv2d_gn_silu(ptr(x), ptr(stats), ptr(gamma), ptr(beta), ptr(W), ptr(bias), ptr(residual), ptr(out), N, H, Wd, Cin,
                                   Cout, G, _opts_ref(opts), stream_ptr()), "pd_conv2d_gn_silu")


def conv2d_up2(x, W, bias, out, N, H, Wd, Cin, Cout, opts=None):
    """nearest x2 -> Conv2d 3x3 pad 1 (+ bias) of Upsample2D in one launch; H, Wd = OUTPUT size (pd_conv2d_up2)."""
    _check(lib().pd_conv2d_up2(ptr(x), ptr(W), ptr(bias), ptr(out), N, H, Wd, Cin, Cout, _opts_ref(opts), stream_ptr()), "pd_conv2d_up2")


def groupnorm_silu_fp8(x, gamma, beta, partials, out, B, S, Cn, G, eps, fp8_scale, silu=True, ss_scale=None, ss_shift=None, ld_ss=0):
    _check(lib().pd_groupnorm_silu_fp8(ptr(x), ptr(gamma), ptr(beta), ptr(ss_scale), ptr(ss_shift), ld_ss, ptr(partials), ptr(out),
                                       B, S, Cn, G, eps, 1 if silu else 0, fp8_scale, stream_ptr()), "pd_groupnorm_silu_fp8")


def groupnorm_silu_bwd(x, dy, gamma, beta, fwd_partials, bwd_partials, dx, B, S, Cn, G, eps=1e-5, silu=True):
    _check(lib().pd_groupnorm_silu_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(beta), ptr(fwd_partials), ptr(bwd_partials), ptr(dx), B, S, Cn, G,
                                       eps, 1 if silu else 0, stream_ptr()), "pd_groupnorm_silu_bwd")


def cast_rows(x, out, out_lo, n_samples, rows_in, row_off, rows_out, Cn, ld_in, ld_out, opts=None):
    _check(lib().pd_cast_rows(ptr(x), ptr(out), ptr(out_lo), n_samples, rows_in, row_off, rows_out, Cn, ld_in, ld_out,
                              _opts_ref(opts), stream_ptr()), "pd_cast_rows")


def cuboid_attention(*, qkv_bf16=None, qkv_f32=None, tok_index, bias, mask, out_bf16=None, out_bf16_lo=None,
                     out_f32=None, B, ntok, Cn, heads, nc, vol, ld_qkv, ld_out, scale, force_generic=False, out_fp8_log2=0, tok_out=None,
                     qkv_fp8_log2=0, opts=None):
    a = CuboidAttnArgs()
    a.operand = 0 if qkv_fp8_log2 else (opts.operand if opts is not None else 0)
    a.qkv_fp8_log2 = qkv_fp8_log2     # k > 0: qkv_bf16 is an e4m3 byte tensor holding q, k, v * 2^k; q k^T and attn v run on the fp8 MFMA
    a.qkv_bf16, a.qkv_f32, a.tok_index, a.bias, a.mask = ptr(qkv_bf16), ptr(qkv_f32), ptr(tok_index), ptr(bias), ptr(mask)
    a.out_bf16, a.out_bf16_lo, a.out_f32 = ptr(out_bf16), ptr(out_bf16_lo), ptr(out_f32)
    a.B, a.ntok, a.C, a.heads, a.nc, a.vol, a.ld_qkv, a.ld_out = B, ntok, Cn, heads, nc, vol, ld_qkv, ld_out
    a.scale = scale
    a.force_generic = 1 if force_generic else 0
    a.out_fp8_log2 = out_fp8_log2     # k > 0: out_bf16 is an e4m3 byte tensor receiving e4m3(o * 2^k) (MFMA cores only)
    a.tok_out = ptr(tok_out)          # [nc][vol] token that receives each slot's result (padding_type "nearest"), or None = tok_index
    _check(lib().pd_cuboid_attention(C.byref(a), stream_ptr()), "pd_cuboid_attention")


def cuboid_attention_bwd(*, qkv, d_out, tok_index, bias, mask, d_qkv, B, ntok, Cn, heads, nc, vol, ld_qkv, ld_dout, ld_dqkv, scale):
    _check(lib().pd_cuboid_attention_bwd(ptr(qkv), ptr(d_out), ptr(tok_index), ptr(bias), ptr(mask), ptr(d_qkv), B, ntok, Cn, heads, nc,
                                         vol, ld_qkv, ld_dout, ld_dqkv, scale, stream_ptr()), "pd_cuboid_attention_bwd")


def softmax_rows(x, out, out_lo, rows, n, ld_in, ld_out, opts=None):
    _check(lib().pd_softmax_rows(ptr(x), ptr(out), ptr(out_lo), rows, n, ld_in, ld_out, _opts_ref(opts), stream_ptr()), "pd_softmax_rows")


def unet_build_input(x, cond, out, B, T_in, T_out, HW, Cn, ld_out):
    _check(lib().pd_unet_build_input(ptr(x), ptr(cond), ptr(out), B, T_in, T_out, HW, Cn, ld_out, stream_ptr()),
           "pd_unet_build_input")


def unet_build_input16(x, cond, out, out16, B, T_in, T_out, HW, Cn, ld_out, ld16):
    """unet_build_input + the bfloat16 copy of its rows (ld16 elements each, zero padded) in one launch"""
    _check(lib().pd_unet_build_input16(ptr(x), ptr(cond), ptr(out), ptr(_dev(out16, torch.bfloat16)), B, T_in, T_out, HW, Cn, ld_out, ld16,
                                       stream_ptr()), "pd_unet_build_input16")


def timestep_freqs(dim, max_period=10000.0, device="cpu"):
    """exp(-ln(max_period) * arange(half) / half) in fp32, the reference's own expression (models/utils.py:79-81)."""
    import math
    half = dim // 2
    return torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half).to(device)


def timestep_embedding(t, freqs, out, B, dim):
    _check(lib().pd_timestep_embedding(ptr(t), ptr(freqs), ptr(out), B, dim, stream_ptr()), "pd_timestep_embedding")


def linear_small(x, W, b, out, M, K, N, act_in="none", act_out="none"):
    _check(lib().pd_linear_small(ptr(x), ptr(W), ptr(b), ptr(out), M, K, N, ACT[act_in], ACT[act_out], stream_ptr()),
           "pd_linear_small")


def time_embed_supported(dim, E, nproj):
    return nproj <= TIME_EMBED_MAX_PROJ and bool(lib().pd_time_embed_supported(dim, E))


def time_embed(t, freqs, W0, b0, W2, b2, proj, sin_out, h1, temb, B, dim, E):
    """The timestep-embedding chain (timestep_embedding, two linear_small, one SiLU-in linear_small per entry of `proj`) in four
    launches, bit-equal to it.  proj: a list of (W (N, E), b (N,) or None, out (B, N))."""
    n = len(proj)
    pw = (C.c_void_p * n)(*[ptr(_dev(w, torch.float32)) for w, _, _ in proj])
    pb = (C.c_void_p * n)(*[ptr(b) for _, b, _ in proj])
    po = (C.c_void_p * n)(*[ptr(_dev(o, torch.float32)) for _, _, o in proj])
    pn = (C.c_int * n)(*[w.shape[0] for w, _, _ in proj])
    _check(lib().pd_time_embed(ptr(_dev(t, torch.int64)), ptr(freqs), ptr(W0), ptr(b0), ptr(W2), ptr(b2), pw, pb, po, pn, n, ptr(sin_out),
                               ptr(h1), ptr(temb), B, dim, E, stream_ptr()), "pd_time_embed")


def add_rowtable(x, table, n_samples, rows, Cn):
    _check(lib().pd_add_rowtable(ptr(x), ptr(table), n_samples, rows, Cn, stream_ptr()), "pd_add_rowtable")


def add(a, b, out, n):
    _check(lib().pd_add(ptr(a), ptr(b), ptr(out), n, stream_ptr()), "pd_add")


def ddpm_step(zt, eps, noise, mean_shift, t, coef, T, out, B, per_sample, temperature=1.0, clip_denoised=False):
    _check(lib().pd_ddpm_step(ptr(zt), ptr(eps), ptr(noise), ptr(mean_shift), ptr(t), ptr(coef), T, ptr(out), B,
                              per_sample, temperature, 1 if clip_denoised else 0, stream_ptr()), "pd_ddpm_step")


def _step(fn, B, per_sample, width, nullable=(), **operands):
    """Check and launch pd_<fn>(*operands, B, per_sample, stream), the form of every sampler-step entry point: `operands` are its
    pointer arguments by name, in its order.  Each is a contiguous fp32 device tensor of >= B * per_sample elements, the coefficient
    rows (the operand named coef...) of >= B * width; only the names in `nullable` may be None."""
    for name, x in operands.items():
        need = B * (width if name.startswith("coef") else per_sample)
        if x is None:
            if name not in nullable:
                raise PrediffHipError(f"{fn}: {name} must not be None")
        elif x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda or x.numel() < need:
            raise PrediffHipError(f"{fn}: {name} must be a contiguous fp32 device tensor of >= {need} elements")
    _check(getattr(lib(), "pd_" + fn)(*map(ptr, operands.values()), B, per_sample, stream_ptr()), "pd_" + fn)


def ddim_step(zt, eps, noise, coef, out, B, per_sample):
    """One DDIM step (coef rows: a_t, a_prev, sigma); `noise` may be None (eta = 0)."""
    _step("ddim_step", B, per_sample, 3, ("noise",), zt=zt, eps=eps, noise=noise, coef=coef, out=out)


def ddim_step_guided(zt, eps, noise, shift, coef4, out, B, per_sample):
    """pd_ddim_step minus gamma * shift (coef4 rows: a_t, a_prev, sigma, gamma); `noise` may be None (eta = 0)."""
    _step("ddim_step_guided", B, per_sample, 4, ("noise",), zt=zt, eps=eps, noise=noise, shift=shift, coef4=coef4, out=out)


def dpmpp_2m_step(zt, eps, hist, coef4, out, B, per_sample):
    """One DPM-Solver++(2M) step (coef4 rows: a_t, c_x, c_d, w); `hist` (the previous x0) is updated in place."""
    _step("dpmpp_2m_step", B, per_sample, 4, zt=zt, eps=eps, hist=hist, coef4=coef4, out=out)


def dpmpp_2m_step_guided(zt, eps, hist, shift, coef5, out, B, per_sample):
    """pd_dpmpp_2m_step minus gamma * shift (coef5 rows: a_t, c_x, c_d, w, gamma)."""
    _step("dpmpp_2m_step_guided", B, per_sample, 5, zt=zt, eps=eps, hist=hist, shift=shift, coef5=coef5, out=out)


def dpmpp_2m_sde_step(zt, eps, noise, hist, coef5, out, B, per_sample):
    """One SDE-DPM-Solver++(2M) step (coef5 rows: a_t, c_x, c_d, w, c_n); `noise` is read only where c_n != 0, `hist` is updated in place."""
    _step("dpmpp_2m_sde_step", B, per_sample, 5, zt=zt, eps=eps, noise=noise, hist=hist, coef5=coef5, out=out)


def dpmpp_2m_sde_step_guided(zt, eps, noise, hist, shift, coef6, out, B, per_sample):
    """pd_dpmpp_2m_sde_step minus gamma * shift (coef6 rows: a_t, c_x, c_d, w, c_n, gamma)."""
    _step("dpmpp_2m_sde_step_guided", B, per_sample, 6, zt=zt, eps=eps, noise=noise, hist=hist, shift=shift, coef6=coef6, out=out)


def ddim_step_held(zt, eps, noise, shift, hold_x0, hold_mask, hold_noise, coef6, out, B, per_sample):
    """pd_ddim_step[_guided] and the hold in one launch (coef6 rows: a_t, a_prev, sigma, gamma, k_x, k_n); `noise` may be None (eta = 0),
    `shift` None is the un-guided step; `hold_noise` is read only where k_n != 0."""
    _step("ddim_step_held", B, per_sample, 6, ("noise", "shift"), zt=zt, eps=eps, noise=noise, shift=shift, hold_x0=hold_x0,
          hold_mask=hold_mask, hold_noise=hold_noise, coef6=coef6, out=out)


def dpmpp_2m_step_held(zt, eps, hist, shift, hold_x0, hold_mask, hold_noise, coef7, out, B, per_sample):
    """pd_dpmpp_2m_step[_guided] and the hold in one launch (coef7 rows: a_t, c_x, c_d, w, gamma, k_x, k_n)."""
    _step("dpmpp_2m_step_held", B, per_sample, 7, ("shift",), zt=zt, eps=eps, hist=hist, shift=shift, hold_x0=hold_x0, hold_mask=hold_mask,
          hold_noise=hold_noise, coef7=coef7, out=out)


def dpmpp_2m_sde_step_held(zt, eps, noise, hist, shift, hold_x0, hold_mask, hold_noise, coef8, out, B, per_sample):
    """pd_dpmpp_2m_sde_step[_guided] and the hold in one launch (coef8 rows: a_t, c_x, c_d, w, c_n, gamma, k_x, k_n)."""
    _step("dpmpp_2m_sde_step_held", B, per_sample, 8, ("shift",), zt=zt, eps=eps, noise=noise, hist=hist, shift=shift, hold_x0=hold_x0,
          hold_mask=hold_mask, hold_noise=hold_noise, coef8=coef8, out=out)


def hold_blend(z, x0, mask, noise, coef2, out, B, per_sample):
    """The start rule of a held run: out = mask-select of z and k_x x0 + k_n noise (coef2 rows: k_x, k_n); `out` may be `z`."""
    _step("hold_blend", B, per_sample, 2, z=z, x0=x0, mask=mask, noise=noise, coef2=coef2, out=out)


_origin_tables = {}      # (table bytes, canvas, window, device, covering) -> the checked device copy


def window_origins(origins, canvas_hw, window_hw, device, covering=False):
    """The device copy of a host origin table (nwin, 2) int32 of (y, x), checked once per (table, geometry, device) and kept: every window
    lies inside the canvas, and with `covering` every canvas cell lies in some window.  The first call for a table uploads it (a
    host-to-device copy); later calls, a graph capture's among them, only look it up."""
    if origins.is_cuda or origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 2 or origins.shape[0] < 1:
        raise PrediffHipError(f"window origins must be a host int32 tensor (nwin, 2); got {origins.dtype} {tuple(origins.shape)} on {origins.device}")
    (Hc, Wc), (h, w) = canvas_hw, window_hw
    device = torch.device(device)
    o = origins.contiguous().numpy()
    key = (o.tobytes(), Hc, Wc, h, w, str(device), bool(covering))
    dev = _origin_tables.get(key)
    if dev is None:
        if not (1 <= h <= Hc and 1 <= w <= Wc):
            raise PrediffHipError(f"window {h} x {w} does not fit the canvas {Hc} x {Wc}")
        if (o < 0).any() or (o[:, 0] > Hc - h).any() or (o[:, 1] > Wc - w).any():
            raise PrediffHipError(f"window origins leave the canvas {Hc} x {Wc} (window {h} x {w}): {o.tolist()}")
        if covering:
            hit = torch.zeros(Hc, Wc, dtype=torch.bool)
            for y, x in o.tolist():
                hit[y:y + h, x:x + w] = True
            if not bool(hit.all()):
                raise PrediffHipError(f"window origins leave {int((~hit).sum())} of the {Hc} x {Wc} canvas cells uncovered")
        dev = _origin_tables[key] = origins.contiguous().to(device)
    return dev


def _window_dims(fn, canvas, windows):
    _dev(canvas, torch.float32), _dev(windows, torch.float32)
    if canvas.dim() != 5 or windows.dim() != 6 or canvas.device != windows.device:
        raise PrediffHipError(f"{fn}: canvas (B, T, Hc, Wc, C) and windows (B, nwin, T, h, w, C) on one device; got {tuple(canvas.shape)} "
                              f"and {tuple(windows.shape)}")
    B, T, Hc, Wc, Cn = canvas.shape
    Bw, nwin, Tw, h, w, Cw = windows.shape
    if (Bw, Tw, Cw) != (B, T, Cn):
        raise PrediffHipError(f"{fn}: windows {tuple(windows.shape)} do not belong to the canvas {tuple(canvas.shape)}")
    return B, nwin, T, Hc, Wc, h, w, Cn


def window_gather(canvas, windows, origins):
    """windows[b, k] = canvas[b, :, y_k : y_k + h, x_k : x_k + w, :] (pd_window_gather); origins: host int32 (nwin, 2), see window_origins."""
    B, nwin, T, Hc, Wc, h, w, Cn = _window_dims("window_gather", canvas, windows)
    if origins.shape[0] != nwin:
        raise PrediffHipError(f"window_gather: {origins.shape[0]} origins for {nwin} windows")
    table = window_origins(origins, (Hc, Wc), (h, w), canvas.device)
    _check(lib().pd_window_gather(ptr(canvas), ptr(windows), ptr(table), B, nwin, T, Hc, Wc, h, w, Cn, stream_ptr()), "pd_window_gather")


def window_blend(windows, weights, origins, canvas):
    """canvas(cell) = sum over the covering windows, ascending, of weights[k] * windows[:, k] (pd_window_blend).  weights (nwin, h, w) fp32,
    normalised; origins as window_gather, and refused when they leave a canvas cell uncovered."""
    B, nwin, T, Hc, Wc, h, w, Cn = _window_dims("window_blend", canvas, windows)
    _dev(weights, torch.float32)
    if tuple(weights.shape) != (nwin, h, w) or weights.device != canvas.device or origins.shape[0] != nwin:
        raise PrediffHipError(f"window_blend: weights {tuple(weights.shape)} / {origins.shape[0]} origins for {nwin} windows of {h} x {w}")
    table = window_origins(origins, (Hc, Wc), (h, w), canvas.device, covering=True)
    _check(lib().pd_window_blend(ptr(windows), ptr(weights), ptr(table), ptr(canvas), B, nwin, T, Hc, Wc, h, w, Cn, stream_ptr()),
           "pd_window_blend")


def _overlaps(a, b):
    """whether the storage ranges of two contiguous tensors on one device intersect"""
    pa, pb = a.data_ptr(), b.data_ptr()
    return a.device == b.device and pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


def context_advance(ctx, z, origins, ctx_next, stride, z_scale, forecast=None, f_off=0, f_cnt=0):
    """The context of the next segment of a rolling forecast, and the kept frames, in one launch (pd_context_advance):
    ctx_next = cat([ctx, z_scale * z's windows], T)[:, :, stride : stride + T_in] and forecast[:, f_off : f_off + f_cnt] = z[:, : f_cnt].
    ctx, ctx_next: (B, nwin, T_in, h, w, C); z: (B, T_out, Hc, Wc, C); origins: host int32 (nwin, 2), see window_origins; forecast:
    (B, f_T, Hc, Wc, C), or None with f_cnt = 0.  z_scale is rounded to fp32 here."""
    fn = "context_advance"
    _dev(ctx, torch.float32), _dev(z, torch.float32), _dev(ctx_next, torch.float32)
    if ctx.dim() != 6 or z.dim() != 5 or ctx_next.shape != ctx.shape or not (ctx.device == z.device == ctx_next.device):
        raise PrediffHipError(f"{fn}: ctx and ctx_next (B, nwin, T_in, h, w, C) and z (B, T_out, Hc, Wc, C) on one device; got "
                              f"{tuple(ctx.shape)}, {tuple(ctx_next.shape)} and {tuple(z.shape)}")
    B, nwin, T_in, h, w, Cn = ctx.shape
    Bz, T_out, Hc, Wc, Cz = z.shape
    if (Bz, Cz) != (B, Cn) or origins.shape[0] != nwin:
        raise PrediffHipError(f"{fn}: the windows {tuple(ctx.shape)} ({origins.shape[0]} origins) do not belong to the canvas {tuple(z.shape)}")
    stride, f_off, f_cnt = int(stride), int(f_off), int(f_cnt)
    if not 1 <= stride <= T_out:
        raise PrediffHipError(f"{fn}: stride {stride} outside [1, T_out] = [1, {T_out}]")
    outs = [("ctx_next", ctx_next)]
    f_T = 0
    if forecast is None:
        if f_cnt != 0:
            raise PrediffHipError(f"{fn}: f_cnt = {f_cnt} without a forecast buffer")
    else:
        _dev(forecast, torch.float32)
        if forecast.dim() != 5 or forecast.device != z.device or (forecast.shape[0],) + tuple(forecast.shape[2:]) != (B, Hc, Wc, Cn):
            raise PrediffHipError(f"{fn}: forecast must be (B, f_T, Hc, Wc, C) like z {tuple(z.shape)}; got {tuple(forecast.shape)}")
        f_T = int(forecast.shape[1])
        if f_cnt < 0 or f_off < 0 or f_cnt > T_out or f_off + f_cnt > f_T:
            raise PrediffHipError(f"{fn}: forecast frames [{f_off}, {f_off} + {f_cnt}) do not fit f_T = {f_T} / T_out = {T_out}")
        outs.append(("forecast", forecast))
    for name, o in outs:
        for other, t in (("ctx", ctx), ("z", z)) + tuple(p for p in outs if p[1] is not o):
            if _overlaps(o, t):
                raise PrediffHipError(f"{fn}: {name} overlaps {other}")
    table = window_origins(origins, (Hc, Wc), (h, w), z.device)
    _check(lib().pd_context_advance(ptr(ctx), ptr(z), ptr(table), ptr(ctx_next), ptr(forecast) if f_cnt else None, B, nwin, T_in, T_out,
                                    Hc, Wc, h, w, Cn, stride, float(z_scale), f_T, f_off, f_cnt, stream_ptr()),
           "pd_context_advance")


def sevir_ingest(raw, starts, ctx, tgt, N, H, W, T, factors, nwin, in_len, out_len, scale, offset):
    """pd_sevir_ingest: raw (N, H, W, T) uint8 -> ctx (N nwin, in_len, H / fh, W / fw, 1) and tgt (..., out_len, ...) fp32 (tgt None with
    out_len = 0); starts: nwin int32 LR frame indices on the device, checked by the caller.  scale / offset are rounded to fp32 here."""
    ft, fh, fw = factors
    _dev(raw, torch.uint8), _dev(starts, torch.int32), _dev(ctx, torch.float32)
    if tgt is not None:
        _dev(tgt, torch.float32)
    Hl, Wl = H // fh, W // fw
    if (raw.numel() != N * H * W * T or starts.numel() != nwin or ctx.numel() != N * nwin * in_len * Hl * Wl
            or (tgt.numel() if tgt is not None else 0) != N * nwin * out_len * Hl * Wl):
        raise PrediffHipError(f"sevir_ingest: raw {tuple(raw.shape)} / {starts.numel()} starts / ctx {tuple(ctx.shape)} / tgt "
                              f"{None if tgt is None else tuple(tgt.shape)} do not hold {N} x {nwin} windows of {in_len} + {out_len} frames of {Hl} x {Wl}")
    _check(lib().pd_sevir_ingest(ptr(raw), ptr(starts), ptr(ctx), ptr(tgt), N, H, W, T, ft, fh, fw, nwin, in_len, out_len, float(scale),
                                 float(offset), stream_ptr()), "pd_sevir_ingest")


def sevir_export(x, out, B, T, H, W, scale, offset, mode):
    """pd_sevir_export: x (B, T, H, W, 1) fp32 -> x / scale - offset as fp32 (mode 0) or as clamped, rounded bytes NTHW (1) / NHWT (2)."""
    _dev(x, torch.float32), _dev(out, torch.float32 if mode == 0 else torch.uint8)
    if x.numel() != B * T * H * W or out.numel() != x.numel() or out.device != x.device:
        raise PrediffHipError(f"sevir_export: x {tuple(x.shape)} / out {tuple(out.shape)} do not hold ({B}, {T}, {H}, {W}) on one device")
    _check(lib().pd_sevir_export(ptr(x), ptr(out), B, T, H, W, float(scale), float(offset), mode, stream_ptr()), "pd_sevir_export")


def lk_ws_bytes(B, T, H, W, levels, iters, radius, pairs):
    """pd_lk_ws_bytes: the workspace of lk_motion at this shape, -1 for an unsupported shape or option (host-only)."""
    return int(lib().pd_lk_ws_bytes(int(B), int(T), int(H), int(W), int(levels), int(iters), int(radius), int(pairs)))


def lk_motion(ctx, motion, B, T, H, W, levels, iters, radius, damping, pairs, ws):
    """pd_lk_motion: ctx (B, T, H, W, 1) fp32 -> motion (B, 2, H, W) fp32 = (v_y, v_x); ws: a device tensor of lk_ws_bytes(...) bytes."""
    _dev(ctx, torch.float32), _dev(motion, torch.float32), _dev(ws)
    if ctx.numel() != B * T * H * W or motion.numel() != B * 2 * H * W or motion.device != ctx.device or ws.device != ctx.device:
        raise PrediffHipError(f"lk_motion: ctx {tuple(ctx.shape)} / motion {tuple(motion.shape)} do not hold ({B}, {T}, {H}, {W}) on one device")
    _check(lib().pd_lk_motion(ptr(ctx), ptr(motion), B, T, H, W, int(levels), int(iters), int(radius), float(damping), int(pairs), ptr(ws),
                              ws.numel() * ws.element_size(), stream_ptr()), "pd_lk_motion")


def advect(frame, motion, out, B, K, H, W, frame_stride, fill):
    """pd_advect: frame (B images of H x W fp32, `frame_stride` elements apart, each contiguous) and motion (B, 2, H, W) -> out
    (B, K, H, W, 1), lead k at [:, k - 1]."""
    _dev(motion, torch.float32), _dev(out, torch.float32)
    if not frame.is_cuda or frame.dtype != torch.float32:
        raise PrediffHipError(f"advect: the frame must be a float32 CUDA(HIP) tensor, got {frame.dtype} on {frame.device}")
    if motion.numel() != B * 2 * H * W or out.numel() != B * K * H * W or motion.device != frame.device or out.device != frame.device:
        raise PrediffHipError(f"advect: motion {tuple(motion.shape)} / out {tuple(out.shape)} do not hold ({B}, {K}, {H}, {W}) on one device")
    _check(lib().pd_advect(ptr(frame), ptr(motion), ptr(out), B, K, H, W, int(frame_stride), float(fill), stream_ptr()), "pd_advect")


def steps_ws_bytes(B, M, H, W, levels, ar_order):
    """pd_steps_ws_bytes: the workspace of B sequences and M members (M = 0: what steps_analyse alone needs), -1 for an unsupported
    shape or option (host-only)."""
    return int(lib().pd_steps_ws_bytes(int(B), int(M), int(H), int(W), int(levels), int(ar_order)))


def _steps_operands(fn, device, operands):
    for name, x, need in operands:
        if x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda or x.device != device or x.numel() != need:
            raise PrediffHipError(f"{fn}: {name} must be a contiguous fp32 tensor of {need} elements on {device}, got {tuple(x.shape)} "
                                  f"{x.dtype} on {x.device}")


def steps_analyse(ctx, motion, bands, B, T, H, W, levels, ar_order, threshold, mu, sigma, phi, gamma, ws):
    """pd_steps_analyse: ctx (B, T, H, W, 1), motion (B, 2, H, W), bands (levels, H, W) -> mu, sigma (B, levels), phi (B, levels, 3),
    gamma (B, levels, 2); ws: a device tensor of at least steps_ws_bytes(B, 0, ...) bytes, which pd_steps_evolve reads."""
    _dev(ws)
    _steps_operands("steps_analyse", ctx.device, (("ctx", ctx, B * T * H * W), ("motion", motion, B * 2 * H * W), ("bands", bands, levels * H * W),
                                                  ("mu", mu, B * levels), ("sigma", sigma, B * levels), ("phi", phi, B * levels * 3),
                                                  ("gamma", gamma, B * levels * 2)))
    _check(lib().pd_steps_analyse(ptr(ctx), ptr(motion), ptr(bands), B, T, H, W, int(levels), int(ar_order), float(threshold), ptr(mu), ptr(sigma),
                                  ptr(phi), ptr(gamma), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "pd_steps_analyse")


def steps_evolve(noise, bands, mu, sigma, phi, M, B, K, H, W, levels, ar_order, R, ws):
    """pd_steps_evolve: noise (M, B, K, H, W) or None -> R (M, B, K, H, W); mu / sigma / phi and ws as pd_steps_analyse left them, ws of
    at least steps_ws_bytes(B, M, ...) bytes."""
    _dev(ws)
    _steps_operands("steps_evolve", R.device, (() if noise is None else (("noise", noise, M * B * K * H * W),)) + (
        ("bands", bands, levels * H * W), ("mu", mu, B * levels), ("sigma", sigma, B * levels), ("phi", phi, B * levels * 3),
        ("R", R, M * B * K * H * W)))
    _check(lib().pd_steps_evolve(ptr(noise), ptr(bands), ptr(mu), ptr(sigma), ptr(phi), int(M), B, K, H, W, int(levels), int(ar_order), ptr(R),
                                 ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "pd_steps_evolve")


def steps_finish(ctx, motion, R, out, M, B, T, K, H, W, threshold, mask, match):
    """pd_steps_finish: R (M, B, K, H, W) -> out (M, B, K, H, W, 1): mask (0 / 1 "obs"), match (0 / 1 "mean"), the threshold cut and the
    advection of lead k."""
    _steps_operands("steps_finish", ctx.device, (("ctx", ctx, B * T * H * W), ("motion", motion, B * 2 * H * W), ("R", R, M * B * K * H * W),
                                                 ("out", out, M * B * K * H * W)))
    _check(lib().pd_steps_finish(ptr(ctx), ptr(motion), ptr(R), ptr(out), int(M), B, T, K, H, W, float(threshold), int(mask), int(match),
                                 stream_ptr()), "pd_steps_finish")


def anvil_ws_bytes(B, H, W, levels, ar_order):
    """pd_anvil_ws_bytes: the workspace of B sequences, -1 for an unsupported shape or option (host-only)."""
    return int(lib().pd_anvil_ws_bytes(int(B), int(H), int(W), int(levels), int(ar_order)))


def anvil_analyse(ctx, motion, bands, window, window_sum_sq, B, T, H, W, levels, ar_order, phi, gamma, ws):
    """pd_anvil_analyse: ctx (B, T, H, W, 1), motion (B, 2, H, W), bands (levels, H, W), window (2 r + 1,) = g[-r .. r] with
    window_sum_sq = (sum g)^2 -> phi, gamma (B, levels, 2, H, W); ws: a device tensor of at least anvil_ws_bytes(...) bytes, which
    pd_anvil_evolve reads."""
    _dev(ws)
    if window.dim() != 1 or window.numel() < 3 or window.numel() % 2 == 0:
        raise PrediffHipError(f"anvil_analyse: window must hold the 2 r + 1 weights g[-r .. r], r >= 1, got {tuple(window.shape)}")
    _steps_operands("anvil_analyse", ctx.device, (("ctx", ctx, B * T * H * W), ("motion", motion, B * 2 * H * W), ("bands", bands, levels * H * W),
                                                  ("window", window, window.numel()), ("phi", phi, B * levels * 2 * H * W),
                                                  ("gamma", gamma, B * levels * 2 * H * W)))
    if ws.device != ctx.device:
        raise PrediffHipError(f"anvil_analyse: ctx is on {ctx.device}, the workspace on {ws.device}")
    _check(lib().pd_anvil_analyse(ptr(ctx), ptr(motion), ptr(bands), ptr(window), window.numel() // 2, float(window_sum_sq), B, T, H, W,
                                  int(levels), int(ar_order), ptr(phi), ptr(gamma), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
           "pd_anvil_analyse")


def anvil_evolve(phi, B, K, H, W, levels, ar_order, R, ws):
    """pd_anvil_evolve: phi (B, levels, 2, H, W) and ws as pd_anvil_analyse left them -> R (B, K, H, W)."""
    _dev(ws)
    _steps_operands("anvil_evolve", R.device, (("phi", phi, B * levels * 2 * H * W), ("R", R, B * K * H * W)))
    if ws.device != R.device:
        raise PrediffHipError(f"anvil_evolve: R is on {R.device}, the workspace on {ws.device}")
    _check(lib().pd_anvil_evolve(ptr(phi), B, K, H, W, int(levels), int(ar_order), ptr(R), ptr(ws), ws.numel() * ws.element_size(),
                                 stream_ptr()), "pd_anvil_evolve")


def nchw_to_nhwc(x, out, N, Cn, HW, ld_out):
    _check(lib().pd_nchw_to_nhwc(ptr(x), ptr(out), N, Cn, HW, ld_out, stream_ptr()), "pd_nchw_to_nhwc")


def nhwc_to_nchw(x, out, N, Cn, HW, ld_in):
    _check(lib().pd_nhwc_to_nchw(ptr(x), ptr(out), N, Cn, HW, ld_in, stream_ptr()), "pd_nhwc_to_nchw")


def sevir_skill_counts(pred, target, thresholds, divisor, counts, outer, T, inner, keep_seq):
    _check(lib().pd_sevir_skill_counts(ptr(pred), ptr(target), ptr(thresholds), thresholds.numel(), divisor, ptr(counts), outer, T,
                                       inner, 1 if keep_seq else 0, stream_ptr()), "pd_sevir_skill_counts")


def _i64(vals):
    vals = [int(v) for v in vals]
    return (C.c_int64 * len(vals))(*vals)


def sevir_skill_counts_pooled(pred, target, thresholds, divisor, counts, sizes, pred_strides, target_strides, pool, keep_seq):
    """sizes / strides: the (N, T, H, W, C) sizes and element strides of pred and target (a missing axis: size 1, stride 0)."""
    _check(lib().pd_sevir_skill_counts_pooled(ptr(pred), ptr(target), ptr(thresholds), thresholds.numel(), divisor, ptr(counts),
                                              _i64(sizes), _i64(pred_strides), _i64(target_strides), int(pool), 1 if keep_seq else 0,
                                              stream_ptr()), "pd_sevir_skill_counts_pooled")


def ensemble_score_ws_doubles(M, sizes, pool):
    return int(lib().pd_ensemble_score_ws_doubles(int(M), _i64(sizes), int(pool)))


def ensemble_score_update(ens, target, thresholds, divisor, M, sizes, ens_strides, target_strides, pool, keep_seq, n_valid, brier, sums, ws):
    """ens_strides: member stride followed by the (N, T, H, W, C) strides; n_valid int64 [T'], brier int64 [thr, T'], sums fp64 [4, T']."""
    _check(lib().pd_ensemble_score_update(ptr(ens), ptr(target), ptr(thresholds), thresholds.numel(), divisor, int(M), _i64(sizes),
                                          _i64(ens_strides), _i64(target_strides), int(pool), 1 if keep_seq else 0, ptr(n_valid), ptr(brier),
                                          ptr(sums), ptr(ws), ws.numel(), stream_ptr()), "pd_ensemble_score_update")


def frame_score_ws_doubles(M, sizes):
    return int(lib().pd_frame_score_ws_doubles(int(M), _i64(sizes)))


def frame_score_update(pred, target, M, sizes, pred_strides, target_strides, data_range, range_buf, keep_seq, sums, counts, ws):
    """pred_strides: member stride followed by the (N, T, H, W, C) strides; sums fp64 [3, T'], counts int64 [2, T'].  range_buf: None
    (data_range is used) or a 2-float device tensor the call fills with the value ranges of pred and target and reads its range from."""
    _check(lib().pd_frame_score_update(ptr(pred), ptr(target), int(M), _i64(sizes), _i64(pred_strides), _i64(target_strides),
                                       float(data_range), ptr(range_buf), 1 if keep_seq else 0, ptr(sums), ptr(counts), ptr(ws),
                                       ws.numel(), stream_ptr()), "pd_frame_score_update")


def spectrum_ws_bytes(M, sizes):
    return int(lib().pd_spectrum_ws_bytes(int(M), _i64(sizes)))


def spectrum_update(pred, target, M, sizes, pred_strides, target_strides, cell_order, bin_start, nb, window, keep_seq, sums, frames, ws):
    """pred_strides: member stride followed by the (N, T, H, W, C) strides; cell_order / bin_start: int32 device tensors of
    spectrum.spectrum_bins; window: 0 none, 1 periodic Hann; sums fp64 [3, T', nb], frames int64 [T']; ws: uint8 workspace (a workspace
    below spectrum_ws_bytes(M, sizes) makes the call run in several chunks of pairs)."""
    _check(lib().pd_spectrum_update(ptr(pred), ptr(target), int(M), _i64(sizes), _i64(pred_strides), _i64(target_strides),
                                    ptr(cell_order), ptr(bin_start), int(nb), int(window), 1 if keep_seq else 0, ptr(sums), ptr(frames),
                                    ptr(ws), ws.numel() * ws.element_size(), stream_ptr()), "pd_spectrum_update")


def objects_ws_bytes(M, sizes):
    return int(lib().pd_objects_ws_bytes(int(M), _i64(sizes)))


def objects_label(frames, sizes, strides, threshold, thr_factor, connectivity, min_pixels, records, labels, table, max_objects):
    """frames: fp32, read in place through the (N, T, H, W, C) sizes / strides; threshold: None for thr_factor * max(frame); records fp64
    [N T, 9]; labels: None or int32 (N, T, H, W); table: None or fp64 (N, T, max_objects, 6)."""
    _check(lib().pd_objects_label(ptr(frames), _i64(sizes), _i64(strides), 0.0 if threshold is None else float(threshold),
                                  0 if threshold is None else 1, float(thr_factor), int(connectivity), int(min_pixels), ptr(records),
                                  ptr(labels), ptr(table), int(max_objects), stream_ptr()), "pd_objects_label")


def sal_update(pred, target, M, sizes, pred_strides, target_strides, threshold, thr_factor, connectivity, min_pixels, keep_seq, sums,
               counts, ws):
    """pred_strides: member stride followed by the (N, T, H, W, C) strides; sums fp64 [7, T'], counts int64 [8, T']; ws: fp64 workspace
    of objects_ws_bytes(M, sizes) bytes."""
    _check(lib().pd_sal_update(ptr(pred), ptr(target), int(M), _i64(sizes), _i64(pred_strides), _i64(target_strides),
                               0.0 if threshold is None else float(threshold), 0 if threshold is None else 1, float(thr_factor),
                               int(connectivity), int(min_pixels), 1 if keep_seq else 0, ptr(sums), ptr(counts), ptr(ws),
                               ws.numel() * ws.element_size(), stream_ptr()), "pd_sal_update")


def distance_ws_bytes(M, K, sizes):
    """pd_distance_ws_bytes: the workspace of distance_update; -1 for an unsupported M / K / shape (host-only)."""
    return int(lib().pd_distance_ws_bytes(int(M), int(K), _i64(sizes)))


def distance_map(frames, sizes, strides, threshold, divisor, d2):
    """frames: fp32, read in place through the (N, T, H, W, C) sizes / strides; event: frames / divisor >= threshold in fp32; d2: int32
    (N, T, H, W)."""
    _check(lib().pd_distance_map(ptr(frames), _i64(sizes), _i64(strides), float(threshold), float(divisor), ptr(d2), stream_ptr()),
           "pd_distance_map")


def distance_update(pred, target, M, sizes, pred_strides, target_strides, thresholds, divisor, cutoff, keep_seq, sums, counts, ws):
    """pred_strides: member stride followed by the (N, T, H, W, C) strides; thresholds: a host sequence of K numbers; cutoff: None or
    Baddeley's c in pixels; sums fp64 [4, K, T'], counts int64 [6, K, T']; ws: a device tensor of at least distance_ws_bytes(M, K, sizes)
    bytes."""
    thr = (C.c_float * len(thresholds))(*[float(t) for t in thresholds])
    _check(lib().pd_distance_update(ptr(pred), ptr(target), int(M), _i64(sizes), _i64(pred_strides), _i64(target_strides), thr,
                                    len(thresholds), float(divisor), 0 if cutoff is None else 1, 0.0 if cutoff is None else float(cutoff),
                                    1 if keep_seq else 0, ptr(sums), ptr(counts), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
           "pd_distance_update")


def scale_ws_bytes(M, K, sizes):
    """pd_scale_ws_bytes: the workspace of scale_update; -1 for an unsupported M / K / shape (host-only)."""
    return int(lib().pd_scale_ws_bytes(int(M), int(K), _i64(sizes)))


def scale_energy(frames, sizes, strides, threshold, divisor, q_out):
    """frames: fp32, read in place through the (N, T, H, W, C) sizes / strides; event: frames / divisor >= threshold in fp32; q_out: int64
    (N T, 8), Q_l of every frame's event field, zero above the frame's top level."""
    _check(lib().pd_scale_energy(ptr(frames), _i64(sizes), _i64(strides), float(threshold), float(divisor), ptr(q_out), stream_ptr()),
           "pd_scale_energy")


def scale_update(pred, target, M, sizes, pred_strides, target_strides, thresholds, divisor, keep_seq, energy, counts, ws):
    """pred_strides: member stride followed by the (N, T, H, W, C) strides; thresholds: a host sequence of K numbers; energy int64
    [3, K, 8, T'], counts int64 [2, T']; ws: a device tensor of at least scale_ws_bytes(M, K, sizes) bytes."""
    thr = (C.c_float * len(thresholds))(*[float(t) for t in thresholds])
    _check(lib().pd_scale_update(ptr(pred), ptr(target), int(M), _i64(sizes), _i64(pred_strides), _i64(target_strides), thr,
                                 len(thresholds), float(divisor), 1 if keep_seq else 0, ptr(energy), ptr(counts), ptr(ws),
                                 ws.numel() * ws.element_size(), stream_ptr()), "pd_scale_update")


PM_RANK, PM_CDF, PM_PMM = 0, 1, 2                       # the ops of pd_pm_ws_bytes


def pm_ws_bytes(op, M, frames, H, W):
    """pd_pm_ws_bytes: the workspace of op PM_RANK (0: none) / PM_CDF (`frames` reference frames) / PM_PMM (M members of `frames`
    frames); -1 for an unsupported shape (host-only)."""
    return int(lib().pd_pm_ws_bytes(int(op), int(M), int(frames), int(H), int(W)))


def _pm_operands(fn, device, operands):
    for name, x, dtype, need in operands:
        if x.dtype != dtype or not x.is_contiguous() or not x.is_cuda or x.device != device or x.numel() != need:
            raise PrediffHipError(f"{fn}: {name} must be a contiguous {dtype} tensor of {need} elements on {device}, got {tuple(x.shape)} "
                                  f"{x.dtype} on {x.device}")


def rank_frames(x, frames, H, W, sorted_out, order):
    """pd_rank_frames: x (frames, H W) fp32 -> sorted_out fp32, order int32, both (frames, H W)."""
    n = frames * H * W
    _pm_operands("rank_frames", x.device, (("x", x, torch.float32, n), ("sorted", sorted_out, torch.float32, n), ("order", order, torch.int32, n)))
    _check(lib().pd_rank_frames(ptr(x), int(frames), int(H), int(W), ptr(sorted_out), ptr(order), stream_ptr()), "pd_rank_frames")


def cdf_match(x, ref, lead, B, T, ref_T, H, W, threshold, out, ws):
    """pd_cdf_match: x (lead, B, T, H W), ref (B, ref_T, H W), ref_T = T or 1 -> out like x; threshold: None or a finite number; ws: a
    device tensor of at least pm_ws_bytes(PM_CDF, 1, B * ref_T, H, W) bytes."""
    _dev(ws)
    n = lead * B * T * H * W
    _pm_operands("cdf_match", x.device, (("x", x, torch.float32, n), ("ref", ref, torch.float32, B * ref_T * H * W), ("out", out, torch.float32, n)))
    _check(lib().pd_cdf_match(ptr(x), ptr(ref), int(lead), int(B), int(T), int(ref_T), int(H), int(W),
                              0.0 if threshold is None else float(threshold), 0 if threshold is None else 1, ptr(out), ptr(ws),
                              ws.numel() * ws.element_size(), stream_ptr()), "pd_cdf_match")


def pmm(ens, M, frames, H, W, out, ws):
    """pd_pmm: ens (M, frames, H W) -> out (frames, H W); ws: a device tensor of at least pm_ws_bytes(PM_PMM, M, frames, H, W) bytes."""
    _dev(ws)
    _pm_operands("pmm", ens.device, (("ens", ens, torch.float32, M * frames * H * W), ("out", out, torch.float32, frames * H * W)))
    _check(lib().pd_pmm(ptr(ens), int(M), int(frames), int(H), int(W), ptr(out), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
           "pd_pmm")


I3D_RES, I3D_STEM_WO, I3D_STEM_LD = 224, 112, 64         # pd_i3d_preprocess: crop side, operand rows per image row, operand row length


def i3d_preprocess(x, sizes, strides, normalize, auto_t, out, out_lo, out_f32=None, rescale=True, opts=None):
    """sizes / strides: the (N, T, H, W, C) sizes and element strides of fp32 x (read in place); out[/out_lo]: (N, T2, 224, 112, 64) 16-bit
    operand rows (the stem's im2col along W); out_f32: None or (N, T2, 224, 224, 3) fp32, the frames before the operand rounding.
    rescale: [0, 1] -> [-1, 1] at the end (False: the frames are in [-1, 1] already)."""
    _check(lib().pd_i3d_preprocess(ptr(x), _i64(sizes), _i64(strides), 1 if normalize else 0, 1 if auto_t else 0, 1 if rescale else 0, ptr(out), ptr(out_lo),
                                   ptr(out_f32), _opts_ref(opts), stream_ptr()), "pd_i3d_preprocess")


def same_pad(k, s, size):
    """total SAME padding of one dimension (pytorch_i3d.py compute_pad); the front pad is half of it, rounded down"""
    return max(k - s, 0) if size % s == 0 else max(k - size % s, 0)


def same_out(k, s, size):
    return (size + same_pad(k, s, size) - k) // s + 1


def maxpool3d_same(x, B, thw, Cn, kernel, stride, out_f32=None, outb=None, outb_lo=None, ld_in=None, ld_out=None, ld_outb=None, opts=None):
    """MaxPool3dSamePadding of channels-last fp32 x (B, *thw, Cn): zero padding that takes part in the max.  Returns the output (T, H, W)."""
    T, H, W = thw
    _check(lib().pd_maxpool3d_same(ptr(x), ptr(out_f32), ptr(outb), ptr(outb_lo), B, T, H, W, Cn, ld_in if ld_in is not None else Cn,
                                   *kernel, *stride, ld_out if ld_out is not None else Cn, ld_outb if ld_outb is not None else pad64(Cn),
                                   _opts_ref(opts), stream_ptr()), "pd_maxpool3d_same")
    return tuple(same_out(k, s, n) for k, s, n in zip(kernel, stride, thw))


def i3d_head(x, W, bias, pooled, out, B, T, HW, Cn, N):
    """(2, 7, 7) average pool -> logits layer -> mean over time of fp32 channels-last x (B, T, HW, Cn) -> out (B, N) fp32."""
    _check(lib().pd_i3d_head(ptr(x), ptr(W), ptr(bias), ptr(pooled), ptr(out), B, T, HW, Cn, N, stream_ptr()), "pd_i3d_head")


def feature_moments_update(f, sum_, cov_sum):
    """sum_ (d) += f.sum(0), cov_sum (d, d) += f^T f in fp64 for fp32 features f (n, d); fixed order, bit-reproducible."""
    n, d = f.shape
    _dev(f, torch.float32), _dev(sum_, torch.float64), _dev(cov_sum, torch.float64)
    if sum_.numel() != d or tuple(cov_sum.shape) != (d, d):
        raise PrediffHipError(f"feature_moments_update: state of {sum_.numel()} / {tuple(cov_sum.shape)} for {d} features")
    _check(lib().pd_feature_moments_update(ptr(f), n, d, d, ptr(sum_), ptr(cov_sum), stream_ptr()), "pd_feature_moments_update")


def attn_block_fused_supported(Cn, heads, vol):
    return bool(lib().pd_attn_block_fused_supported(Cn, heads, vol))


def attn_block_fused(x, out, gamma, beta, Wqkv, bqkv, Wp, bp, tok_index, bias, mask, B, ntok, Cn, heads, nc, vol, scale, eps=1e-5,
                     tok_affine=None, opts=None):
    """tok_affine: (n_inner, outer, inner, slot) from cuboid_geometry.affine_form(tok_index), or None (the kernel loads the table)."""
    aff = (C.c_int32 * 4)(*tok_affine) if tok_affine is not None else None
    _check(lib().pd_attn_block_fused_ex(ptr(x), ptr(out), ptr(gamma), ptr(beta), ptr(Wqkv), ptr(bqkv), ptr(Wp), ptr(bp), ptr(tok_index),
                                        ptr(bias), ptr(mask), B, ntok, Cn, heads, nc, vol, scale, eps,
                                        C.cast(aff, C.c_void_p) if aff is not None else None, _opts_ref(opts), stream_ptr()),
           "pd_attn_block_fused")


def ffn_fused_supported(Cn, Hd):
    return bool(lib().pd_ffn_fused_supported(Cn, Hd))


def ffn_fused(x, out, gamma, beta, W1, b1, W2, b2, M, Cn, Hd, act="gelu", eps=1e-5, opts=None):
    _check(lib().pd_ffn_fused(ptr(x), ptr(out), ptr(gamma), ptr(beta), ptr(W1), ptr(b1), ptr(W2), ptr(b2), M, Cn, Hd, ACT[act], eps,
                              _opts_ref(opts), stream_ptr()), "pd_ffn_fused")


def attn_ffn_pair_supported(Cn, heads, hidden, vol, act="gelu"):
    return bool(lib().pd_attn_ffn_pair_supported(Cn, heads, hidden, vol, ACT[act]))


def attn_ffn_pair_cuboids_per_group(vol):
    return 2 if 1 <= vol <= 8 else 1              # == pd_attn_ffn_pair_cuboids_per_group (tests/test_host_logic.py compares)


def attn_ffn_pair(x, out, wstream, vecs, tok_index, B, ntok, nc, vol, scale, eps_attn=1e-5, eps_ffn=1e-5, tok_affine=None, units=256,
                  opts=None):
    """One (CuboidSelfAttentionLayer, PositionwiseFFN) pair of a block (units 256 or 512) in one launch (csrc/pair_block.hip).
    wstream / vecs: packing.pack_pair_block / pack_pair_vecs."""
    aff = (C.c_int32 * 4)(*tok_affine) if tok_affine is not None else None
    _check(lib().pd_attn_ffn_pair(ptr(x), ptr(out), ptr(wstream), ptr(vecs), ptr(tok_index),
                                  C.cast(aff, C.c_void_p) if aff is not None else None, B, ntok, nc, vol, units, scale, eps_attn,
                                  eps_ffn, _opts_ref(opts), stream_ptr()), "pd_attn_ffn_pair")


def attn_ffn_pair_split_ws_floats(B, ntok, units):
    return 2 * 4 * B * ntok * units               # == pd_attn_ffn_pair_split_ws_floats (tests/test_host_logic.py compares)


def attn_ffn_pair_split(x, out, wstream, wffn_split, vecs, tok_index, B, ntok, nc, vol, scale, ws, eps_attn=1e-5, eps_ffn=1e-5, tok_affine=None,
                        units=512, opts=None):
    """The (attention, FFN) pair at units 512 for small grids: two tile launches + two row sums, four workgroups per 64-row tile (csrc/pair_block.hip MODE 1 / 2
    + pair_split_sum_kernel).  wffn_split: packing.pack_pair_ffn_split; ws: fp32 workspace of attn_ffn_pair_split_ws_floats(...) elements."""
    aff = (C.c_int32 * 4)(*tok_affine) if tok_affine is not None else None
    _check(lib().pd_attn_ffn_pair_split(ptr(x), ptr(out), ptr(wstream), ptr(wffn_split), ptr(vecs), ptr(tok_index),
                                        C.cast(aff, C.c_void_p) if aff is not None else None, B, ntok, nc, vol, units, scale, eps_attn, eps_ffn,
                                        ptr(ws), ws.numel(), _opts_ref(opts), stream_ptr()), "pd_attn_ffn_pair_split")


def ffn_rows_supported(Cn, Hd, act="gelu"):
    return bool(lib().pd_ffn_rows_supported(Cn, Hd, ACT[act]))


def ffn_rows(x, out, wffn, vecs, rows, units, eps=1e-5, opts=None):
    """PositionwiseFFN alone on the pair kernel's FFN half (csrc/pair_block.hip MODE 2, one hidden slice): x (rows, units) fp32 -> out (may alias).
    wffn: packing.pack_pair_ffn_split(w1, w2, nsplit=1); vecs: packing.pack_pair_vecs (LayerNorm-2, b1, b2 are read)."""
    _check(lib().pd_ffn_rows(ptr(x), ptr(out), ptr(wffn), ptr(vecs), rows, units, eps, _opts_ref(opts), stream_ptr()), "pd_ffn_rows")
