"""keep_conv2d_plan (host-side C, no GPU) for the x2-phase Upsample convolution: the streaming form (keep_conv_x3s.hip, Cin >= 32) and the
stage-barrier form (Cin = 16, KEEP_CONV_NO_STREAM) are one family to a caller -- the same kernel name, split-K, workspace and statistics
partition whichever of them the launch takes."""
import ctypes

from comfyui_keep_amd.engine import hiplib

KERNEL = 'conv3x3_halo_x3_kernel<32, x2 phases>'


def _plan(lib, ptr, **kw):
    base = dict(struct_size=ctypes.sizeof(hiplib.ConvArgs), N=2, H=16, W=64, Cin=128, Cout=128, KH=3, KW=3, stride=1, pad_t=1, pad_l=1,
                Ho=32, Wo=128, in_ld=128, out_ld=128, mma=hiplib.MMA_X3, upsample=hiplib.UPSAMPLE_X2_PHASES, inp=ptr, out=ptr, weight=ptr,
                weight_x3=ptr, x3_acc_scale=1.0)
    base.update(kw)
    out = hiplib.ConvPlanOut()
    rc = lib.keep_conv2d_plan(ctypes.byref(hiplib.ConvArgs(**base)), ctypes.byref(out))
    assert rc == 0, lib.keep_last_error()
    return out.kernel.decode(), out.split_k, out.workspace_bytes, out.stats_rows, out.stats_P, out.out_amax_ok


def test_up2_plan_is_the_same_for_both_launch_forms():
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_conv2d_plan.restype = ctypes.c_int32
    lib.keep_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 4096)()
    ptr = (ctypes.addressof(buf) + 63) // 64 * 64
    seen = set()
    for cin in (16, 32, 128):
        for flags in (0, hiplib.CONV_NO_STREAM):
            got = _plan(lib, ptr, Cin=cin, in_ld=cin, flags=flags)
            assert got[0] == KERNEL, (cin, flags, got)
            assert got[1] == 1 and got[2] == 0, (cin, flags, got)
            seen.add(got)
    assert len(seen) == 1, seen
    # four statistics partials per 8 x 32 source tile: one per phase, each over 256 output pixels
    assert next(iter(seen))[3:] == (256, (32 * 128) // 256, 1), seen
