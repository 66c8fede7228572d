"""ctypes binding of liblbwn.so (include/lbwn.h).

The library is the product: there is no CPU fallback.  ``load()`` raises if the .so is
missing or was built for another ABI, and every wrapper raises ``LbwnError`` with the
library's message on a non-zero return.  torch is imported first so the process has ONE
HIP runtime (torch's bundled libamdhip64.so.7 satisfies the .so's NEEDED entry).
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the .so: shared HIP runtime)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'liblbwn.so')   # the in-tree build only (tools/with_lib.py loads variants)
ABI_VERSION = 5

c_int, c_int64, c_float, c_void_p, c_size_t = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
c_fp = ctypes.c_void_p   # device pointers are passed as integers


class LbwnError(RuntimeError):
    pass


class Arch(ctypes.Structure):
    _fields_ = [('n_blocks', c_int), ('n_block_layers', c_int), ('n_quant', c_int), ('n_res', c_int),
                ('n_dil', c_int), ('n_skip', c_int), ('n_post', c_int), ('n_gc_embed', c_int),
                ('n_gc_category', c_int), ('n_lc_in', c_int), ('n_lc_out', c_int),
                ('n_lc_upsample', c_int), ('lc_upsample', c_int * 8), ('use_bias', c_int)]


class Params(ctypes.Structure):
    _fields_ = [(n, c_fp) for n in (
        'pre', 'pre_b', 'sig', 'sig_b', 'gate', 'gate_b', 'res', 'res_b', 'skip', 'skip_b',
        'gc_embed', 'gc_sig', 'gc_gate', 'lc_sig', 'lc_gate')] + [('lc_up', c_fp * 8)] + [
        (n, c_fp) for n in ('post1', 'post1_b', 'post2', 'post2_b')]


class GemmExArgs(ctypes.Structure):
    """lbwn_gemm_ex_args (include/lbwn.h), field for field; struct_size is set on construction."""
    _fields_ = [('struct_size', c_size_t), ('A', c_fp), ('B', c_fp), ('C', c_fp),
                ('lda', c_int64), ('ldb', c_int64), ('ldc', c_int64),
                ('M', c_int), ('N', c_int), ('K', c_int),
                ('a_kcontig', c_int), ('b_kcontig', c_int), ('split_k', c_int),
                ('slab_ws', c_fp), ('bias', c_fp), ('mask', c_fp), ('ldm', c_int64),
                ('relu_a', c_int), ('relu_out', c_int), ('accumulate', c_int), ('xcd2d', c_int),
                ('b3', c_fp), ('colpart', c_fp), ('step_advance', c_fp),
                ('c_chain_ls', c_int64), ('a_kstride', c_int64), ('b_gstride', c_int64), ('a_gstride', c_int64),
                ('mbits_out', c_fp), ('mbits', c_fp),
                ('row_live', c_fp), ('k_live', c_fp), ('nk_live', c_fp), ('k_pre', c_fp),
                ('splits_deferred', ctypes.POINTER(c_int)),
                ('row_exact', c_int), ('reserved', c_int)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(GemmExArgs)


class AdamExArgs(ctypes.Structure):
    """lbwn_adam_ex_args (include/lbwn.h), field for field; struct_size is set on construction."""
    _fields_ = [('struct_size', c_size_t), ('params', c_fp), ('grads', c_fp), ('m', c_fp), ('v', c_fp),
                ('n_weights', c_int64), ('n_total', c_int64),
                ('lr', c_float), ('beta1', c_float), ('beta2', c_float), ('eps', c_float), ('l2_factor', c_float),
                ('stats', c_fp), ('counters', c_fp), ('step_status', c_fp),
                ('clip_norm', c_float), ('skip_nonfinite', c_int), ('ema_decay', c_float), ('ema_num_updates', c_int),
                ('ema', c_fp), ('lr_warmup_steps', c_int64), ('lr_decay_steps', c_int64),
                ('lr_decay_rate', c_float), ('lr_decay_staircase', c_int),
                ('ws', c_fp), ('info', c_fp), ('nonfinite_skips', c_fp)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(AdamExArgs)


class EvalArgs(ctypes.Structure):
    """lbwn_eval_args (include/lbwn.h), field for field; struct_size is set on construction."""
    _fields_ = [('struct_size', c_size_t), ('wav_q', c_fp), ('ids', c_fp), ('mel', c_fp), ('save', c_fp),
                ('acc', c_fp), ('nll', c_fp), ('ld_nll', c_int64), ('by_voice', c_fp), ('n_bins', c_int),
                ('status', c_fp), ('scratch', c_fp)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(EvalArgs)


class BackwardArgs(ctypes.Structure):
    """lbwn_backward_args (include/lbwn.h), field for field; struct_size is set on construction."""
    _fields_ = [('struct_size', c_size_t), ('wav_q', c_fp), ('ids', c_fp), ('mel', c_fp), ('dmel', c_fp)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(BackwardArgs)


class ForwardArgs(ctypes.Structure):
    """lbwn_forward_args (include/lbwn.h), field for field; struct_size is set on construction."""
    _fields_ = [('struct_size', c_size_t), ('wav_q', c_fp), ('ids', c_fp), ('mel', c_fp), ('save', c_fp),
                ('stats', c_fp), ('stats_ex', c_fp), ('teacher_logits', c_fp), ('ld_teacher', c_int64),
                ('distill_alpha', c_float), ('distill_temp', c_float), ('label_smoothing', c_float)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(ForwardArgs)


class MelCfg(ctypes.Structure):
    """lbwn_mel_cfg (include/lbwn.h), field for field; struct_size is set on construction."""
    _fields_ = [('struct_size', c_size_t), ('sample_rate', c_int), ('n_fft', c_int), ('win_length', c_int),
                ('hop', c_int), ('n_mels', c_int), ('fmin', c_float), ('fmax', c_float),
                ('power', c_int), ('htk', c_int), ('norm', c_int), ('log_floor', c_float)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(MelCfg)


class GenSession(ctypes.Structure):
    """lbwn_gen_session (include/lbwn.h), field for field."""
    _fields_ = [('slot', c_int), ('gc_id', c_int), ('key', c_int64), ('mel', c_fp), ('n_frames', c_int64)]


class GenPlanArgs(ctypes.Structure):
    """lbwn_gen_plan_args (include/lbwn.h), field for field; struct_size is set on construction."""
    _fields_ = [('struct_size', c_size_t), ('batch_sz', c_int), ('max_steps', c_int64), ('max_teacher', c_int64),
                ('ring_steps', c_int64)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = ctypes.sizeof(GenPlanArgs)


class GenExtendEntry(ctypes.Structure):
    """lbwn_gen_extend_entry (include/lbwn.h), field for field."""
    _fields_ = [('slot', c_int), ('mel', c_fp), ('n_frames', c_int64)]


_SIGS = {
    'lbwn_mel_plan_create': (c_int, [ctypes.POINTER(MelCfg), ctypes.POINTER(c_void_p)]),
    'lbwn_mel_plan_destroy': (None, [c_void_p]),
    'lbwn_mel_frames': (c_int64, [c_void_p, c_int64]),
    'lbwn_mel_workspace_bytes': (c_size_t, [c_void_p]),
    'lbwn_mel_filterbank': (c_int, [c_void_p, ctypes.POINTER(c_float)]),
    'lbwn_mel_init': (c_int, [c_void_p, c_fp, c_void_p]),
    'lbwn_mel_forward': (c_int, [c_void_p, c_fp, c_fp, c_int64, c_int, c_int64, c_fp, c_int64, c_void_p]),
    'lbwn_last_error': (ctypes.c_char_p, []),
    'lbwn_abi_version': (c_int, []),
    'lbwn_recep_field_sz': (c_int, [ctypes.POINTER(Arch)]),
    'lbwn_plan_create': (c_int, [ctypes.POINTER(Arch), c_int, c_int, ctypes.POINTER(c_void_p)]),
    'lbwn_plan_destroy': (None, [c_void_p]),
    'lbwn_plan_workspace_bytes': (c_size_t, [c_void_p]),
    'lbwn_plan_probe': (c_int, [c_void_p, ctypes.c_char_p, c_void_p, c_void_p]),
    'lbwn_plan_stream_wait': (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.POINTER(c_int)]),
    'lbwn_plan_tensor': (c_int, [c_void_p, ctypes.c_char_p, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    'lbwn_train_forward': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_void_p]),
    'lbwn_train_forward_ex': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, ctypes.POINTER(ForwardArgs), c_void_p]),
    'lbwn_train_backward': (c_int, [c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Params), c_fp, c_fp, c_fp,
                                    c_fp, c_void_p]),
    'lbwn_train_backward_ex': (c_int, [c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Params), c_fp,
                                       ctypes.POINTER(BackwardArgs), c_void_p]),
    'lbwn_train_eval_scratch_bytes': (c_size_t, [c_void_p, c_int]),
    'lbwn_train_eval': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, ctypes.POINTER(EvalArgs), c_void_p]),
    'lbwn_adam_tf1': (c_int, [c_fp, c_fp, c_fp, c_fp, c_int64, c_int64, c_float, c_float, c_float, c_float,
                              c_float, c_fp, c_fp, c_fp, c_void_p]),
    'lbwn_adam_ex_ws_floats': (c_int64, [c_int64]),
    'lbwn_adam_ex': (c_int, [ctypes.POINTER(AdamExArgs), c_void_p]),
    'lbwn_gen_plan_create': (c_int, [ctypes.POINTER(Arch), c_int, c_int64, c_int64, ctypes.POINTER(c_void_p)]),
    'lbwn_gen_plan_destroy': (None, [c_void_p]),
    'lbwn_gen_workspace_bytes': (c_size_t, [c_void_p]),
    'lbwn_gen_tensor': (c_int, [c_void_p, ctypes.c_char_p, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    'lbwn_gen_start': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, c_fp, c_fp, c_int64, ctypes.c_uint64, c_int,
                               c_void_p]),
    'lbwn_gen_set_mel': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, c_fp, c_int64, c_void_p]),
    'lbwn_gen_run': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, c_int, c_void_p]),
    'lbwn_gen_is_persistent': (c_int, [c_void_p]),
    'lbwn_gen_begin': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, ctypes.POINTER(GenSession), c_int, c_size_t,
                               c_void_p]),
    'lbwn_gen_plan_create_ex': (c_int, [ctypes.POINTER(Arch), ctypes.POINTER(GenPlanArgs), ctypes.POINTER(c_void_p)]),
    'lbwn_gen_extend': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, ctypes.POINTER(GenExtendEntry), c_int,
                                c_size_t, c_void_p]),
    'lbwn_gen_collect': (c_int, [c_void_p, c_fp, c_int, c_int64, c_int64, c_fp, c_fp, c_void_p]),
    'lbwn_gen_prefill': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, c_fp, c_int64, c_int64, c_void_p]),
    'lbwn_gen_score_scratch_bytes': (c_size_t, [c_void_p]),
    'lbwn_gen_score': (c_int, [c_void_p, ctypes.POINTER(Params), c_fp, c_fp, c_int64, c_int64, c_fp, c_int64, c_fp,
                               c_void_p]),
    'lbwn_gen_set_sampling': (c_int, [c_void_p, c_float, c_int, c_float]),
    'lbwn_gen_get_sampling': (c_int, [c_void_p, ctypes.POINTER(c_float), ctypes.POINTER(c_int),
                                      ctypes.POINTER(c_float)]),
    'lbwn_gen_state_bytes': (c_size_t, [c_void_p, c_int]),
    'lbwn_gen_state_save': (c_int, [c_void_p, c_fp, c_fp, c_void_p]),
    'lbwn_gen_state_load': (c_int, [c_void_p, c_fp, c_fp, c_int, c_fp, c_void_p]),
    'lbwn_mulaw_encode':(c_int, [c_fp, c_fp, c_int64, c_int, c_int, c_void_p]),
    'lbwn_mulaw_decode': (c_int, [c_fp, c_fp, c_int64, c_int, c_void_p]),
    'lbwn_gemm_f32': (c_int, [c_fp, c_int64, c_int, c_fp, c_int64, c_int, c_fp, c_int64, c_int, c_int, c_int,
                              c_fp, c_int, c_int, c_fp, c_int64, c_int, c_int, c_fp, c_void_p]),
    'lbwn_gemm_f32_presplit': (c_int, [c_fp, c_int64, c_int, c_fp, c_int, c_fp, c_int64, c_int, c_fp, c_int64, c_int,
                                       c_int, c_fp, c_int, c_int, c_fp, c_int64, c_int, c_void_p]),
    'lbwn_split_planes_elems_abi': (c_int64, [c_int, c_int]),
    'lbwn_split_planes': (c_int, [c_fp, c_int64, c_int, c_int, c_int, c_fp, c_void_p]),
    'lbwn_gemm_ex': (c_int, [ctypes.POINTER(GemmExArgs), c_void_p]),
    'lbwn_gemm_last_form': (ctypes.c_char_p, []),
    'lbwn_gemm_mbits_words_abi': (c_int64, [c_int, c_int]),
    'lbwn_colpart_parts_abi': (c_int, [c_int]),
    'lbwn_gemm_form_query': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'lbwn_plan_info': (c_int, [c_void_p, ctypes.c_char_p, ctypes.POINTER(c_int64)]),
    # (nup, strides, Li, Lo[, frames]); F / act / dF are host arrays of device pointers
    'lbwn_lc_upsample_fused_ok': (c_int, [c_int, ctypes.POINTER(c_int), c_int, c_int]),
    'lbwn_lc_upsample_part_floats': (c_int64, [c_int, ctypes.POINTER(c_int), c_int, c_int, c_int]),
    'lbwn_lc_upsample_forward': (c_int, [c_int, ctypes.POINTER(c_int), c_int, c_int, c_int, c_fp,
                                         ctypes.POINTER(c_fp), ctypes.POINTER(c_fp), c_void_p]),
    'lbwn_lc_upsample_backward': (c_int, [c_int, ctypes.POINTER(c_int), c_int, c_int, c_int, c_fp,
                                          ctypes.POINTER(c_fp), ctypes.POINTER(c_fp), c_fp, c_int, c_int64, c_fp,
                                          ctypes.POINTER(c_fp), c_void_p]),
    'lbwn_lc_upsample_backward_dmel': (c_int, [c_int, ctypes.POINTER(c_int), c_int, c_int, c_int, c_fp,
                                               ctypes.POINTER(c_fp), ctypes.POINTER(c_fp), c_fp, c_int, c_int64, c_fp,
                                               ctypes.POINTER(c_fp), c_fp, c_void_p]),
    'lbwn_gc_table': (c_int, [c_fp, c_fp, c_fp, c_fp, c_int, c_int, c_int, c_int, c_void_p]),
    'lbwn_gc_grads': (c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_int, c_int, c_int, c_int, c_void_p]),
    'lbwn_gc_part_floats_abi': (c_int64, [c_int, c_int, c_int]),
    'lbwn_gemm_set_mode': (c_int, [c_int]),
    'lbwn_gemm_get_mode': (c_int, []),
    'lbwn_layer_image_floats_abi': (c_int, []),
    'lbwn_layer_forward': (c_int, [c_fp, c_fp, c_fp, c_int64, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp,
                                   c_fp, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_fp, c_void_p]),
    'lbwn_layer_backward_ws_floats': (c_int64, [c_int, c_int, c_int]),
    'lbwn_layer_backward': (c_int, [c_fp, c_fp, c_int64, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp,
                                    c_int64, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_int64, c_fp, c_int,
                                    c_int, c_int, c_int, c_int, c_int, c_fp, c_void_p]),
    'lbwn_dsep_prepend': (c_int, [c_fp, c_int64, c_fp, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'lbwn_dsep_save': (c_int, [c_fp, c_int64, c_fp, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'lbwn_head_xent': (c_int, [c_fp, c_fp, c_fp, c_int, c_int, c_int, c_int, c_fp, c_fp, c_void_p]),
    'lbwn_head_xent_ex': (c_int, [c_fp, c_fp, c_fp, c_int, c_int, c_int, c_fp, c_int64, c_float, c_float, c_float,
                                  c_fp, c_fp, c_fp, c_void_p]),
}

EXPORTED = sorted(_SIGS)
_lib = None


def load(path=LIB_PATH):
    """Load liblbwn.so (once).  Raises LbwnError when it is absent: no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise LbwnError('liblbwn.so not found at %s — build it with __graft_entry__.build() '
                        '(or `make -C lb-wavenet_amd/csrc`); there is no CPU fallback' % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.lbwn_abi_version() != ABI_VERSION:
        raise LbwnError('liblbwn.so ABI %d != %d' % (lib.lbwn_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(ret):
    if ret != 0:
        msg = _lib.lbwn_last_error().decode() if _lib is not None else ''
        raise LbwnError('lbwn error %d: %s' % (ret, msg))
    return ret


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream
