"""ctypes binding of ``libkeep_hip.so`` (the C-ABI declared in ``include/keep_hip.h``).

This is the host side of the drop-in boundary: plain pointers and sizes cross it, torch only
supplies device memory (``tensor.data_ptr()``) and the stream.  There is NO fallback: if the
library is missing, was built for another ABI version, or the device is not gfx950, loading
raises -- the product path never silently runs on anything but the hand-written kernels.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('KEEP_HIP_LIB') or os.path.join(os.path.dirname(_HERE), 'csrc', 'libkeep_hip.so')   # (KEEP_HIP_LIB: dev A/B builds)
ABI_VERSION = 23

F32, BF16 = 0, 1
MMA_F32, MMA_BF16, MMA_X3, MMA_X1 = 0, 1, 2, 3
PRO_NONE, PRO_SWISH, PRO_RELU = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_GELU, ACT_SIGMOID, ACT_LRELU01, ACT_SILU = 0, 1, 2, 3, 4, 5, 6
PAD_ZERO, PAD_REFLECT = 0, 1
UPSAMPLE_X2_PHASES = 2
# keep_conv2d_args.flags / keep_attention_args.flags (include/keep_hip.h): kernel-selection overrides, 0 = the library's choice
(CONV_NO_COUT4, CONV_NO_C3, CONV_NO_HALO_F32, CONV_NO_HALO_X3, CONV_NO_GATHER_X3, CONV_NO_PLAIN, CONV_NO_FLATK_F32,
 CONV_SMALL_TILES, CONV_X3_EXACT_ACT, CONV_NO_STREAM, CONV_NO_GEMM_LAT, CONV_GEMM_LAT_WAVES, CONV_GEMM_LAT_TILES, CONV_NO_SMALL_PARTIALS) = (1 << i for i in range(14))
CONV_X1_HALO16 = 1 << 15    # opt-in: MMA_X1 also takes 3x3 stride-1 convolutions on 16 x 16-tile maps that are not 8 x 32 tileable (KEEP_CONV_X1_HALO16)
CONV_X1_UP2 = 1 << 16       # opt-in: MMA_X1 also takes upsample = UPSAMPLE_X2_PHASES where x3 plans the streaming phase form, Cin % 32 == 0 (KEEP_CONV_X1_UP2)
CONV_X1_GEMM = 1 << 14      # opt-in: MMA_X1 also takes the 1x1 stride-1 GEMM form (KEEP_CONV_X1_GEMM); ignored by every other policy
ATTN_NO_PACK, ATTN_NO_SFULL2, ATTN_NO_X3, ATTN_NO_SMALL, ATTN_NO_TWO_PASS = 1, 2, 4, 8, 16
ATTN_X1 = 1 << 5            # opt-in: MMA_X1 takes the packed D = Dv = 128 attention form on single fp16 operands (KEEP_ATTN_X1); ignored by every other policy

_vp, _i32, _i64, _f32, _u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint32
STATUS_NONFINITE_LOGITS, STATUS_NONFINITE_TENSOR = 1, 2


class ConvArgs(C.Structure):
    # field-for-field include/keep_hip.h:keep_conv2d_args ('inp' = `in`, a Python keyword); tests/test_host_logic.py checks the
    # names / order against the header, the size against keep_sizeof_conv2d_args(), and INTEGRATION.md's copy against this list
    _fields_ = [('struct_size', _u32), ('flags', _u32), ('inp', _vp), ('weight', _vp), ('bias', _vp), ('out', _vp), ('pro_scale', _vp), ('pro_shift', _vp),
                ('residual', _vp), ('aux', _vp), ('workspace', _vp)] + \
               [(n, _i32) for n in ('N', 'H', 'W', 'Cin', 'Cout', 'KH', 'KW', 'stride', 'pad_t', 'pad_l', 'Ho', 'Wo',
                                    'in_ld', 'out_ld', 'res_ld', 'upsample', 'pro_act', 'epi_act')] + \
               [('aux_w', _f32), ('split_k', _i32), ('dtype', _i32), ('mma', _i32), ('weight_bf16', _vp), ('stats_out', _vp), ('stats_P', _i32), ('bk256', _i32), ('out_dtype', _i32),
                ('weight_x3', _vp), ('x3_acc_scale', _f32), ('x3_in_amax', _vp), ('x3_out_amax', _vp), ('x3_out_amax_zeroed', _i32), ('in2', _vp), ('in2_cin1', _i32), ('pad_mode', _i32),
                ('ln_gamma', _vp), ('ln_beta', _vp), ('ln_eps', _f32), ('plan_ref_images', _i32)]


class ConvPlanOut(C.Structure):
    _fields_ = [('path', _i32), ('split_k', _i32), ('workspace_bytes', _i64), ('stats_rows', _i32), ('stats_P', _i32),
                ('wants_bf16_input', _i32), ('out_bf16_ok', _i32), ('out_amax_ok', _i32), ('kernel', C.c_char * 64)]


class AttnArgs(C.Structure):
    _fields_ = [('struct_size', _u32), ('flags', _u32), ('q', _vp), ('k', _vp), ('v', _vp), ('o', _vp)] + \
               [(n, _i64) for n in ('q_bs', 'q_ts', 'q_hs', 'k_bs', 'k_ts', 'k_hs', 'v_bs', 'v_ts', 'v_hs',
                                    'o_bs', 'o_ts', 'o_hs')] + \
               [(n, _i32) for n in ('B', 'H', 'Lq', 'Lk', 'D', 'Dv')] + [('scale', _f32), ('mode', _i32)] + \
               [(n, _i32) for n in ('T', 'seg_len', 'img_h', 'img_w', 'ksplit', 'shift', 'kv_rot', 'n_img', 'mma', 'in_dtype')] + \
               [('q_amax', _vp), ('k_amax', _vp), ('v_amax', _vp), ('workspace', _vp), ('workspace_bytes', _i64)]


class AttnPlanOut(C.Structure):
    # include/keep_cv_hip.h:keep_attention_plan_out
    _fields_ = [('waves', _i32), ('dvt', _i32), ('nslices', _i32), ('masked', _i32), ('win_tables', _i32), ('lds_bytes', _i64), ('scratch_bytes', _i64),
                ('kernel', C.c_char * 96)]


class ConvLaunchPlanOut(C.Structure):
    # include/keep_cv_hip.h:keep_conv2d_launch_plan_out
    _fields_ = [('n_kernels', _i32), ('kernels', C.c_char * 508)]


# name -> argtypes (restype is always int32 status); every symbol include/keep_hip.h declares
_SIGNATURES = {
    'keep_conv2d': [C.POINTER(ConvArgs), _vp],
    'keep_conv2d_plan': [C.POINTER(ConvArgs), C.POINTER(ConvPlanOut)],
    'keep_attention': [C.POINTER(AttnArgs), _vp],
    'keep_chan_stats': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_norm_finalize': [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    'keep_group_stats': [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp],
    'keep_affine_act': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    'keep_gm_mlp': [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    'keep_token_linear': [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp],
    'keep_gm_ffn_x3': [_vp, _vp, _vp, _f32, _vp, _f32, _vp, _vp, _f32, _vp, _i64, _i32, _i32, _i32, _vp],
    'keep_norm_act_bf16': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_gm_join': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    'keep_bilinear_upscale': [_vp, _vp, _i32, _i32, _i32, _i32, _vp],
    'keep_absmax': [_vp, _vp, _i32, _i64, _i32, _i64, _i64, _i32, _vp],
    'keep_layernorm': [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _f32, _vp],
    'keep_geglu': [_vp, _vp, _i32, _i32, _vp],
    'keep_layernorm_amax': [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _i32, _vp, _i32, _vp],
    'keep_geglu_amax': [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    'keep_argmax_gather': [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp],
    'keep_nonfinite_flag': [_vp, _i64, _vp, _vp],
    'keep_vq_nearest': [_vp, _vp, _vp, _i32, _i32, _i32, _vp],
    'keep_kalman_update': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    'keep_flow_warp': [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    'keep_convex_upsample': [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    'keep_nchw_to_nhwc': [_vp, _vp, _i32, _i32, _i32, _i32, _vp],
    'keep_rgb_s2d': [_vp, _vp, _i32, _i32, _i32, _vp],
    'keep_nhwc_to_nchw': [_vp, _vp, _i32, _i32, _i32, _vp],
    'keep_add_bcast': [_vp, _vp, _vp, _i64, _i64, _f32, _vp],
    'keep_concat2': [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp],
    'keep_tensor2img': [_vp, _vp, _i64, _vp],
    'keep_img2tensor': [_vp, _vp, _i64, _vp],
    'keep_bgr_u8_to_comfy': [_vp, _vp, _i64, _vp],
    'keep_comfy_to_bgr_u8': [_vp, _vp, _i64, _vp],
    'keep_channel_argmax': [_vp, _vp, _i64, _i32, _i32, _vp],
    'keep_maxpool3s2': [_vp, _vp, _i32, _i32, _i32, _i32, _vp],
    'keep_dwconv3x3': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_maxpool2d': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_slice_copy': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_channel_shuffle2': [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp],
    'keep_yolo_decode': [_vp, _vp, _i32, _i32, _i32, _f32, _vp, _i32, _i32, _vp],
    'keep_yolo_letterbox_u8': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_yolo_select': [_vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp],
    'keep_upsample_add': [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_act_inplace': [_vp, _i64, _i32, _vp],
    'keep_retina_decode': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _f32, _vp],
    'keep_retina_nms': [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp],
    'keep_retina_nms_ordered': [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp],
    'keep_sep_filter': [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    'keep_u8_to_f32': [_vp, _vp, _i64, _vp],
    'keep_f32_round_u8': [_vp, _vp, _i64, _vp],
    'keep_warp_affine_u8': [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp],
    'keep_warp_ones': [_vp, _i32, _i32, _i32, _i32, _vp, _vp],
    'keep_draw_box': [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp],
    'keep_erode_rect': [_vp, _vp, _vp, _i32, _i32, _i32, _vp],
    'keep_paste_face': [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_lanczos4_tables': [_i32, _i32, _vp, _vp],                        # (host-only: no stream argument)
    'keep_resize_lanczos4_u8': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
}
EXPORTED_SYMBOLS = ['keep_abi_version', 'keep_last_error', 'keep_device_ok', 'keep_attention_workspace_bytes',
                    'keep_sizeof_conv2d_args', 'keep_sizeof_attention_args'] + list(_SIGNATURES)

# the extension header include/keep_cv_hip.h of the same library: its own version, its own table (the core C-ABI above is frozen)
CV_ABI_VERSION = 1
_CV_SIGNATURES = {
    'keep_area_tables': [_i32, _i32, _i32, _vp, _vp, _vp],                 # (host-only: no stream argument)
    'keep_resize_area_u8': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'keep_resize_linear_u8': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    'keep_resize_linear_fxy_u8': [_vp, _vp, _i32, _i32, _i32, _i32, _i32, C.c_double, C.c_double, _vp],
    'keep_warp_batch_group': [_i32, _i32, _vp, _vp],                       # (host-only: no stream argument)
    'keep_warp_affine_batch_u8': [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp],
    'keep_warp_affine_batch_scatter_u8': [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    'keep_attention_plan': [C.POINTER(AttnArgs), C.POINTER(AttnPlanOut)],  # (host-only: no stream argument)
    'keep_conv2d_launch_plan': [C.POINTER(ConvArgs), C.POINTER(ConvLaunchPlanOut)],  # (host-only: no stream argument)
    'keep_gm_ffn_x1_plan': [_i32, _i32, _i32, _i32, _i32],                 # (host-only: no stream argument)
    'keep_gm_ffn_x1': [_vp, _vp, _vp, _f32, _vp, _f32, _vp, _vp, _f32, _vp, _i64, _i32, _i32, _i32, _vp],
    'keep_frame_signature_u8': [_vp, _i32, _i32, _i32, _vp, _vp],
    'keep_paste_face_w': [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    'keep_paste_face_aa': [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    'keep_tone_match_u8': [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    'keep_conv2d_split': [C.POINTER(ConvArgs), _i32, _i32, _vp],
    'keep_conv2d_split_plan': [C.POINTER(ConvArgs), _i32, _i32, C.POINTER(ConvPlanOut)],      # (host-only: no stream argument)
    'keep_attention_kv_split': [C.POINTER(AttnArgs), _vp],
    'keep_attention_kv_split_plan': [C.POINTER(AttnArgs), C.POINTER(AttnPlanOut)],            # (host-only: no stream argument)
}
CV_EXPORTED_SYMBOLS = ['keep_cv_abi_version'] + list(_CV_SIGNATURES)

_lib = None
_device_checked = set()


EINVAL, EUNSUP = -1, -2      # KEEP_EINVAL / KEEP_EUNSUP of include/keep_hip.h


class KeepHipError(RuntimeError):
    """``code``: the library's return code (EINVAL, EUNSUP, ...), None where no call returned one (library not found, ABI mismatch)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load(check_device=True):
    """dlopen the library, bind every symbol, verify the ABI version (and gfx950 when asked)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KeepHipError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
                f"There is no CPU/PyTorch fallback for the KEEP hot path.")
        lib = C.CDLL(LIB_PATH)
        lib.keep_abi_version.restype = _i32
        lib.keep_last_error.restype = C.c_char_p
        lib.keep_device_ok.restype = _i32
        lib.keep_device_ok.argtypes = [_i32]
        lib.keep_attention_workspace_bytes.restype = _i64
        lib.keep_attention_workspace_bytes.argtypes = [C.POINTER(AttnArgs)]
        ver = lib.keep_abi_version()
        if ver != ABI_VERSION:
            raise KeepHipError(f"libkeep_hip.so ABI version {ver} != expected {ABI_VERSION}; rebuild")
        lib.keep_sizeof_conv2d_args.restype = lib.keep_sizeof_attention_args.restype = _i32
        for name, struct in (('keep_sizeof_conv2d_args', ConvArgs), ('keep_sizeof_attention_args', AttnArgs)):
            want = getattr(lib, name)()
            if want != C.sizeof(struct):        # a layout drift between this binding and the library is a load-time error
                raise KeepHipError(f"{name}() = {want} but the ctypes {struct.__name__} is {C.sizeof(struct)} bytes; "
                                   f"engine/hiplib.py and include/keep_hip.h disagree")
        if not hasattr(lib, 'keep_cv_abi_version'):
            raise KeepHipError("libkeep_hip.so lacks the include/keep_cv_hip.h entry points (keep_cv_abi_version); rebuild")
        lib.keep_cv_abi_version.restype = _i32
        ver = lib.keep_cv_abi_version()
        if ver != CV_ABI_VERSION:
            raise KeepHipError(f"libkeep_hip.so keep_cv_hip.h version {ver} != expected {CV_ABI_VERSION}; rebuild")
        for name, argtypes in list(_SIGNATURES.items()) + list(_CV_SIGNATURES.items()):
            fn = getattr(lib, name)            # AttributeError if the symbol is missing
            fn.restype = _i32
            fn.argtypes = argtypes
        _lib = lib
    if check_device:
        dev = torch.cuda.current_device() if torch.cuda.is_available() else None
        if dev is None:
            raise KeepHipError("no HIP device visible: the KEEP hot path runs on MI355X (gfx950) only")
        if dev not in _device_checked:
            rc = _lib.keep_device_ok(dev)
            if rc != 0:
                raise KeepHipError(_lib.keep_last_error().decode(), code=rc)
            _device_checked.add(dev)
    return _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(rc, what):
    if rc != 0:
        raise KeepHipError(f"{what} failed (code {rc}): {_lib.keep_last_error().decode()}", code=rc)


def call(name, *args):
    """Invoke a flat-signature entry point on torch's current stream; tensors are passed as pointers."""
    lib = load()
    conv = [(_ptr(a) if isinstance(a, torch.Tensor) or a is None else a) for a in args]
    _check(getattr(lib, name)(*conv, _stream()), name)


def conv_args(**kw):
    a = ConvArgs()
    a.struct_size = C.sizeof(ConvArgs)
    for k, v in kw.items():
        setattr(a, k, _ptr(v) if (isinstance(v, torch.Tensor) or v is None) else v)
    return a


def conv2d_plan(a):
    """keep_conv2d_plan: the library's own decision for these arguments (kernel, split-K, workspace / statistics sizes)."""
    lib = load(check_device=False)
    out = ConvPlanOut()
    _check(lib.keep_conv2d_plan(C.byref(a), C.byref(out)), 'keep_conv2d_plan')
    return out


def conv2d_split_plan(a, split_cols):
    """keep_conv2d_split_plan: ``conv2d_plan`` for a launch that writes output columns ``split_cols = (c0, c1)`` as split-fp16 halves."""
    lib = load(check_device=False)
    out = ConvPlanOut()
    _check(lib.keep_conv2d_split_plan(C.byref(a), int(split_cols[0]), int(split_cols[1]), C.byref(out)), 'keep_conv2d_split_plan')
    return out


def conv2d_launch_plan(a):
    """keep_conv2d_launch_plan: the template instantiations keep_conv2d would launch for exactly these arguments, in launch order, joined
    by " + " (keep_conv2d_plan names the form; this names what the launch takes for the real N, flags and activations); a refused call
    raises KeepHipError with the library's code and reason.  Needs no device."""
    lib = load(check_device=False)
    out = ConvLaunchPlanOut()
    _check(lib.keep_conv2d_launch_plan(C.byref(a), C.byref(out)), 'keep_conv2d_launch_plan')
    return out.kernels.decode()


def attention_workspace_bytes(a):
    """keep_attention_workspace_bytes: scratch the library can use for this call (0 = none; -1 = MMA_X1 | ATTN_X1 refuses the call)."""
    return int(load(check_device=False).keep_attention_workspace_bytes(C.byref(a)))


def attention_plan(a, kv_split=False):
    """keep_attention_plan: what keep_attention would launch for exactly these arguments (instantiation, LDS, scratch); a refused call raises
    KeepHipError with the library's code and reason.  Needs no device.  ``kv_split``: keep_attention_kv_split_plan, the same for k / v
    that keep_conv2d_split wrote as split-fp16 halves."""
    lib = load(check_device=False)
    out = AttnPlanOut()
    if kv_split:
        _check(lib.keep_attention_kv_split_plan(C.byref(a), C.byref(out)), 'keep_attention_kv_split_plan')
        return out
    _check(lib.keep_attention_plan(C.byref(a), C.byref(out)), 'keep_attention_plan')
    return out


def attn_args(**kw):
    a = AttnArgs()
    a.struct_size = C.sizeof(AttnArgs)
    for k, v in kw.items():
        setattr(a, k, _ptr(v) if (isinstance(v, torch.Tensor) or v is None) else v)
    return a


def attention_x1_plan(**kw):
    """The library's answer to `this call under MMA_X1 | ATTN_X1`: the scratch bytes the single-fp16 form needs.  A refusal
    (keep_attention_workspace_bytes = -1, what keep_attention answers KEEP_EUNSUP to) raises KeepHipError with ``code == EUNSUP`` and the
    library's reason, like keep_conv2d_plan does; needs no device."""
    a = attn_args(**dict(kw, mma=MMA_X1, flags=int(kw.get('flags', 0)) | ATTN_X1))
    need = attention_workspace_bytes(a)
    if need < 0:
        raise KeepHipError(f"keep_attention plan failed (code -2): {_lib.keep_last_error().decode()}", code=EUNSUP)
    return need


def gm_ffn_x1_plan(C_, hidden, io_misalign=0, weight_misalign=0, ln_misalign=0):
    """keep_gm_ffn_x1_plan: the library's answer to `the fused GMFlow FFN on single fp16 for this per-token shape?` -- True, or KeepHipError
    with the library's code (``EUNSUP``: stay on keep_gm_ffn_x3) and reason.  The alignment classes are `address % 16` OR-ed over
    src / msg / out, the weight twins, gamma / beta.  Needs no device."""
    lib = load(check_device=False)
    _check(lib.keep_gm_ffn_x1_plan(int(C_), int(hidden), int(io_misalign), int(weight_misalign), int(ln_misalign)), 'keep_gm_ffn_x1_plan')
    return True


def conv2d_launch(a):
    _check(load().keep_conv2d(C.byref(a), _stream()), 'keep_conv2d')


def conv2d_split_launch(a, split_cols):
    _check(load().keep_conv2d_split(C.byref(a), int(split_cols[0]), int(split_cols[1]), _stream()), 'keep_conv2d_split')


def conv2d(**kw):
    conv2d_launch(conv_args(**kw))


def attention(kv_split=False, **kw):
    lib = load()
    a = attn_args(**kw)
    if kv_split:      # k / v are keep_conv2d_split's halves: one launch, no workspace
        _check(lib.keep_attention_kv_split(C.byref(a), _stream()), 'keep_attention_kv_split')
        return
    need = int(lib.keep_attention_workspace_bytes(C.byref(a)))       # the library asks; the host only allocates
    if need > 0:                                                     # (-1: a refused MMA_X1 call -- keep_attention below says why)
        ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=kw['q'].device)   # stream-ordered free after the call
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _check(lib.keep_attention(C.byref(a), _stream()), 'keep_attention')
