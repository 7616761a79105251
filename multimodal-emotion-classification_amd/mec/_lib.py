"""ctypes binding of libmec_hip.so (the C ABI declared in include/mec.h).

The library is built in-tree by __graft_entry__.build() (csrc/Makefile). There is no
fallback: if the library or a GPU is missing, load() raises MecError.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# MEC_LIB selects another build of the same ABI (tools/ only: libmec_hip_probes.so, the
# -DMEC_PROBES build whose probe option values return wrong results).
LIB_PATH = os.environ.get('MEC_LIB') or os.path.join(_HERE, 'libmec_hip.so')
PROBES_LIB_PATH = os.path.join(_HERE, 'libmec_hip_probes.so')

c_vp = ctypes.c_void_p
c_int = ctypes.c_int
c_fp = ctypes.POINTER(ctypes.c_float)
c_dp = ctypes.POINTER(ctypes.c_double)


class GemmArgs(ctypes.Structure):
    """include/mec.h mec_gemm_args (mec_gemm_ex's descriptor), field for field. amode: A_PLAIN /
    A_CONV / A_DUAL below; oscale and cscale default to 1 (none)."""
    _fields_ = [('amode', c_int), ('A', c_vp), ('a_lo', ctypes.c_longlong), ('A2', c_vp), ('K1', c_int),
                ('B', c_vp), ('b_lo', ctypes.c_longlong), ('oscale', ctypes.c_float), ('bias', c_vp),
                ('R', c_vp), ('r_is_f32', c_int), ('r_lo', ctypes.c_longlong),
                ('r_stats', c_vp), ('r_gamma', c_vp), ('r_beta', c_vp),
                ('C16', c_vp), ('c_lo', ctypes.c_longlong), ('cscale', ctypes.c_float), ('C32', c_vp),
                ('M', c_int), ('N', c_int), ('K', c_int), ('act', c_int),
                ('n', c_int), ('H', c_int), ('W', c_int), ('C', c_int), ('ks', c_int), ('stride', c_int),
                ('pad', c_int)]

    def __init__(self, **kw):
        super().__init__(**{'oscale': 1.0, 'cscale': 1.0, **kw})


A_PLAIN, A_CONV, A_DUAL = 0, 1, 2


class AttnArgs(ctypes.Structure):
    """include/mec.h mec_attn_args (mec_bert_attn's descriptor), field for field. qks defaults to 1/8 and
    oscale to 1; a `*_lo` of X3_PAIRED says that split tensor is paired."""
    _fields_ = [('precision', c_int), ('form', c_int), ('fused', c_int), ('packed', c_int),
                ('qkv', c_vp), ('qkv_lo', ctypes.c_longlong), ('qc', c_vp), ('qc_lo', ctypes.c_longlong),
                ('hs', c_vp), ('hs_lo', ctypes.c_longlong), ('wqkv', c_vp), ('w_lo', ctypes.c_longlong),
                ('bqkv', c_vp), ('oscale', ctypes.c_float), ('mask', c_vp), ('cidx', c_vp),
                ('ctx', c_vp), ('ctx_lo', ctypes.c_longlong), ('qks', ctypes.c_float),
                ('rows', c_int), ('ns', c_int)]

    def __init__(self, **kw):
        super().__init__(**{'oscale': 1.0, 'qks': 0.125, **kw})


X3_PAIRED = -1


class FusionMixedArgs(ctypes.Structure):
    """include/mec.h mec_fusion_mixed_args (mec_fusion_fwd_mixed's descriptor), field for field."""
    _fields_ = [('s_feat', c_vp), ('t_feat', c_vp), ('i_feat', c_vp), ('s_pred', c_vp), ('t_pred', c_vp),
                ('i_pred', c_vp), ('ns', c_int), ('nt', c_int), ('ni', c_int),
                ('s_idx', c_vp), ('t_idx', c_vp), ('i_idx', c_vp), ('att', c_vp), ('n_att', c_int), ('B', c_int),
                ('fused', c_vp), ('logits', c_vp), ('attn_w', c_vp), ('dec_w', c_vp)]


class JpegHuff(ctypes.Structure):
    """include/mec.h mec_jpeg_huff: a Huffman table as the file states it, 16 counts and the values."""
    _fields_ = [('counts', ctypes.c_uint8 * 16), ('vals', ctypes.c_uint8 * 256)]


class JpegDesc(ctypes.Structure):
    """include/mec.h mec_jpeg_desc (mec_jpeg_probe's result, mec_jpeg_decode_ragged's input), field for field."""
    _fields_ = [('H', ctypes.c_int32), ('W', ctypes.c_int32), ('ncomp', ctypes.c_int32),
                ('hs', ctypes.c_int32 * 3), ('vs', ctypes.c_int32 * 3), ('restart', ctypes.c_int32),
                ('nseg', ctypes.c_int32), ('qt', (ctypes.c_uint16 * 64) * 3), ('dc', JpegHuff * 3), ('ac', JpegHuff * 3)]


# include/mec.h MEC_MOD_* (bits of a sample's `present`) and MEC_ROUTE_*
MOD_SPEECH, MOD_TEXT, MOD_IMAGE = 1, 2, 4
ROUTE_NONE, ROUTE_SINGLE, ROUTE_AVERAGE, ROUTE_ATTENTION = 0, 1, 2, 3

# name -> (restype, argtypes); mirrors include/mec.h one to one.
SIGNATURES = {
    'mec_version': (ctypes.c_char_p, []),
    'mec_last_error': (ctypes.c_char_p, []),
    'mec_blob_size': (ctypes.c_longlong, [c_int]),
    'mec_create': (c_int, [c_int, c_fp, ctypes.c_size_t, c_int, ctypes.POINTER(c_vp)]),
    'mec_create_ex': (c_int, [c_int, c_fp, ctypes.c_size_t, c_int, c_int, ctypes.POINTER(c_vp)]),
    'mec_create_opt': (c_int, [c_int, c_fp, ctypes.c_size_t, c_int, c_int, ctypes.c_char_p, ctypes.POINTER(c_vp)]),
    'mec_model_x3_report': (ctypes.c_char_p, [c_vp]),
    'mec_model_x3_observe': (c_int, [c_vp, c_int]),
    'mec_model_x3_observed': (c_int, [c_vp, c_fp, c_int]),
    'mec_model_x3_names': (ctypes.c_char_p, [c_vp]),
    'mec_create_x3_calibrated': (c_int, [c_int, c_fp, ctypes.c_size_t, c_int, ctypes.c_char_p, c_fp, c_int,
                                         ctypes.POINTER(c_vp)]),
    'mec_absmax_f32': (c_int, [c_vp, ctypes.c_longlong, c_fp, c_vp]),
    'mec_precision': (c_int, [c_vp]),
    'mec_destroy': (c_int, [c_vp]),
    'mec_speech_fwd': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    'mec_text_fwd': (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'mec_text_pack_plan': (c_int, [ctypes.POINTER(ctypes.c_int32), c_int, ctypes.POINTER(ctypes.c_int32),
                                   ctypes.POINTER(ctypes.c_int32)]),
    'mec_text_fwd_packed': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'mec_image_fwd': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    'mec_image_fwd_u8': (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'mec_fusion_fwd': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'mec_fusion_mixed_plan': (c_int, [ctypes.POINTER(ctypes.c_uint8), c_int, c_int] + [ctypes.POINTER(ctypes.c_int32)] * 6),
    'mec_fusion_fwd_mixed': (c_int, [c_vp, ctypes.POINTER(FusionMixedArgs), c_vp]),
    'mec_text_lstm_fwd': (c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'mec_lstm_seq_f32': (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    'mec_tok_create': (c_int, [c_vp, c_int, ctypes.POINTER(c_vp)]),
    'mec_tok_create_utf8': (c_int, [c_vp, c_vp, c_int, ctypes.POINTER(c_vp)]),
    'mec_tok_encode': (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    'mec_tok_destroy': (c_int, [c_vp]),
    'mec_audio_fwd': (c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    'mec_resample_on_gpu': (c_int, [c_int, c_int]),
    'mec_resample_plan': (c_int, [c_int, c_int] + [ctypes.POINTER(c_int)] * 3),
    'mec_resample_taps': (c_int, [c_int, c_int, c_vp, ctypes.c_size_t]),
    'mec_audio_load_ragged': (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, ctypes.c_size_t, c_vp, c_int, c_vp]),
    'mec_audio_load_prof_enable': (c_int, [c_int]),
    'mec_audio_load_prof_read': (c_int, [c_dp, ctypes.POINTER(c_int)]),
    'mec_fuse_weighted': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    'mec_fuse_weighted_f64': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    'mec_resize_u8': (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp]),
    'mec_resize_on_gpu': (c_int, [c_int, c_int]),
    'mec_resize_taps': (c_int, [c_int, c_int, c_vp, c_vp, c_vp, c_int]),
    'mec_resize_ragged_u8': (c_int, [c_vp, c_vp, c_vp, c_int, c_int, ctypes.c_size_t, c_vp, ctypes.c_size_t, c_vp,
                                     c_vp]),
    'mec_resize_prof_enable': (c_int, [c_int]),
    'mec_resize_prof_read': (c_int, [c_dp, c_dp, ctypes.POINTER(c_int)]),
    'mec_image_gray_ragged_u8': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, ctypes.c_size_t, c_vp, c_vp]),
    'mec_image_canon_ragged_u8': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, ctypes.c_size_t, c_vp,
                                          ctypes.c_size_t, c_vp]),
    'mec_image_canon_prof_enable': (c_int, [c_int]),
    'mec_image_canon_prof_read': (c_int, [c_dp, ctypes.POINTER(c_int), c_dp, ctypes.POINTER(c_int)]),
    'mec_jpeg_probe': (c_int, [c_vp, ctypes.c_size_t, ctypes.POINTER(JpegDesc), c_vp, c_int]),
    'mec_jpeg_workspace_bytes': (ctypes.c_longlong, [c_vp, c_int]),
    'mec_jpeg_decode_ragged': (c_int, [c_vp, ctypes.c_size_t, c_vp, c_vp, c_int, c_vp, c_vp, ctypes.c_size_t, c_vp,
                                       ctypes.c_size_t, c_vp, c_vp]),
    'mec_jpeg_prof_enable': (c_int, [c_int]),
    'mec_jpeg_prof_read': (c_int, [c_dp, c_dp, c_dp, ctypes.POINTER(c_int)]),
    'mec_gemm_f16': (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    'mec_gemm_f16x3': (c_int, [c_vp, ctypes.c_longlong, c_vp, ctypes.c_longlong, ctypes.c_float, c_vp, c_vp, c_vp,
                               ctypes.c_longlong, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    'mec_gemm_f16x3_paired': (c_int, [c_vp, c_vp, ctypes.c_float, c_vp, c_vp, c_vp, c_int, ctypes.c_longlong, c_vp,
                                      c_int, c_int, c_int, c_int, c_vp]),
    'mec_gemm_f16x3_paired_ln': (c_int, [c_vp, c_vp, ctypes.c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                         ctypes.c_longlong, ctypes.c_float, c_vp, c_int, c_int, c_int, c_int, c_vp,
                                         c_vp]),
    'mec_conv_f16': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_vp]),
    'mec_gemm_f32': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp]),
    'mec_conv_f32': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_vp]),
    'mec_gemm_ex': (c_int, [ctypes.POINTER(GemmArgs), c_vp]),
    'mec_bert_attn': (c_int, [ctypes.POINTER(AttnArgs), c_vp]),
    'mec_set_option': (c_int, [ctypes.c_char_p, c_int]),
    'mec_model_set_option': (c_int, [c_vp, ctypes.c_char_p, c_int]),
    'mec_build_flags': (c_int, []),
    'mec_model_gemm_query': (c_int, [c_vp, c_int, c_int, c_int, c_int]),
    'mec_gemm_query': (c_int, [c_int, c_int, c_int, c_int]),
    'mec_gemm_f32_query': (c_int, [c_int, c_int, c_int, c_int]),
    'mec_model_check': (c_int, [c_vp]),
    'mec_prof_enable': (c_int, [c_vp, c_int]),
    'mec_prof_read': (c_int, [c_vp, c_dp, ctypes.POINTER(c_int)]),
}

# Kernel tags for mec_prof_enable (csrc/mec_common.h KernelTag).
TAGS = {'bert_qkv': 1, 'bert_attn': 2, 'bert_oproj': 3, 'bert_ffn1': 4, 'bert_ffn2': 5, 'bert_ln': 6,
        'resnet_conv3x3': 7, 'resnet_conv1x1': 8, 'resnet_stem': 9, 'speech': 10, 'fusion': 11,
        'mbv2_blocks': 12, 'mbv2_last': 13, 'audio': 14,
        'lstm_proj': 16, 'lstm_rec1': 17, 'lstm_rec2': 18, 'lstm_head': 19}


# Handle precision (include/mec.h MEC_PREC_*): 'f16' = f16 MFMA operands with fp32
# accumulation / LayerNorm / softmax / residual (the fast path), 'fp32' = fp32 throughout,
# 'fp32x3' = the fp32 path with its GEMM operands as exact f16 hi/lo pairs on the f16 MFMA.
PRECISIONS = {'f16': 0, 'fp32': 1, 'fp32x3': 2}


# mec_model_check's return code for a raised fp32x3 range flag (include/mec.h MEC_ERR_X3_RANGE)
ERR_X3_RANGE = -2


class MecError(RuntimeError):
    pass


class X3RangeError(MecError):
    """An fp32x3 handle's activation planes left the f16 range (mec_model_check == MEC_ERR_X3_RANGE):
    the batch's outputs are invalid; it can be re-run on an fp32 handle of the same weights."""


_lib = None
_lock = threading.Lock()


def load(path: str = LIB_PATH):
    """Load and declare the library (no GPU needed to load it)."""
    global _lib
    with _lock:
        if _lib is not None and path == LIB_PATH:
            return _lib
        if not os.path.exists(path):
            raise MecError(f'{path} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"`')
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if path == LIB_PATH:
            _lib = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        err = load().mec_last_error()
        raise (X3RangeError if rc == ERR_X3_RANGE else MecError)(
            f'{what} failed: {err.decode() if err else "unknown error"}')
