"""CPU suite: host-side logic of the drop-in surface -- converters (P4), clip chunking / ordering (P1-P3),
weight ingestion (P5), node surface (8b), C-ABI exports."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT


# ------------------------------------------------------------------ stub ComfyUI runtime for the node surface
def _install_comfy_stub():
    if 'comfy' in sys.modules:
        return
    comfy = types.ModuleType('comfy')
    mm = types.ModuleType('comfy.model_management')
    mm.get_torch_device = lambda: torch.device('cpu')
    mm.unet_offload_device = lambda: torch.device('cpu')
    mm.soft_empty_cache = lambda: None
    cu = types.ModuleType('comfy.utils')

    class ProgressBar:
        last = None

        def __init__(self, total):
            self.total, self.current = total, 0
            ProgressBar.last = self

        def update(self, n):
            self.current += n

    cu.ProgressBar = ProgressBar
    cu.tiled_scale = None
    comfy.model_management, comfy.utils = mm, cu
    fp = types.ModuleType('folder_paths')
    fp.models_dir = '/nonexistent/models'
    sys.modules.update({'comfy': comfy, 'comfy.model_management': mm, 'comfy.utils': cu, 'folder_paths': fp})


_install_comfy_stub()
import importlib  # noqa: E402

nodes = importlib.import_module('comfyui_keep_amd.nodes')
from comfyui_keep_amd.modules import utils as U  # noqa: E402
from comfyui_keep_amd.modules.keep_model_loader import KEEPModelPack, convert_legacy_keys, select_params  # noqa: E402
from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor, split_clips  # noqa: E402
from comfyui_keep_amd.engine import synth  # noqa: E402


def test_node_surface():
    assert set(nodes.NODE_CLASS_MAPPINGS) == {'KEEP_ModelLoader', 'KEEP_FaceUpscaleImage', 'KEEP_ProcessImageSequence'}
    assert nodes.NODE_DISPLAY_NAME_MAPPINGS == {
        'KEEP_ModelLoader': 'Load KEEP Models', 'KEEP_FaceUpscaleImage': 'KEEP Single Image',
        'KEEP_ProcessImageSequence': 'KEEP Image Sequence'}
    seq = nodes.KEEP_ProcessImageSequenceNode
    req = seq.INPUT_TYPES()['required']
    assert list(req) == ['images', 'keep_model', 'final_upscale_factor', 'has_aligned_frames', 'only_center_face',
                         'draw_bounding_box', 'max_clip_length']
    assert req['max_clip_length'][1]['default'] == 20 and req['max_clip_length'][1]['max'] == 100
    assert req['final_upscale_factor'][1] == {**req['final_upscale_factor'][1], 'default': 1.0, 'min': 0.5, 'max': 4.0, 'step': 0.1}
    assert seq.RETURN_TYPES == ('IMAGE',) and seq.FUNCTION == 'process_sequence' and seq.CATEGORY == 'ComfyUI-KEEP'
    ld = nodes.KEEP_ModelLoaderNode
    assert ld.RETURN_TYPES == ('KEEP_MODEL_PACK',) and ld.FUNCTION == 'load_model_pack'
    it = ld.INPUT_TYPES()
    assert it['required']['model'][0] == ['KEEP', 'Asian']
    assert it['required']['detection_model'][0] == ['retinaface_resnet50', 'retinaface_mobile0.25', 'YOLOv5l', 'YOLOv5n']
    assert set(it['optional']) == {'bg_upscale_model', 'face_upscale_model'}


def test_processing_nodes_never_raise():
    img = torch.zeros(1, 8, 8, 3)
    assert nodes.KEEP_FaceUpscaleImageNode().upscale_face_image(img, "not a pack", 1.0, True, True, False) == (None,)

    class Boom:
        def __call__(self, *a, **k):
            raise RuntimeError("boom")

        def to(self, d):
            return self

    class Helper:
        pass

    pack = KEEPModelPack(Boom(), Helper(), None, None, 'KEEP')
    out = nodes.KEEP_ProcessImageSequenceNode().process_sequence(torch.zeros(2, 512, 512, 3), pack, 1.0, True, True, False, 20)
    assert out == (None,)


def test_config_table():
    a = U.KEEP_MODEL_CONFIGS['KEEP']['architecture']
    assert a['cft_list'] == ['16', '32', '64'] and a['temp_reg_list'] == ['32'] and a['kalman_attn_head_dim'] == 48
    assert U.KEEP_MODEL_CONFIGS['Asian']['architecture']['cft_list'] == ['32', '64', '128', '256']
    assert a['fix_modules'] == ['quantize', 'generator'] and a['latent_size'] == 256 and a['mask_ratio'] == 0.


def test_converters_edge_values():
    # comfy_image_to_cv2 truncates; channel order flips
    img = torch.tensor([[[[0.999, 0.5, 0.0]]]])
    assert U.comfy_image_to_cv2(img).tolist() == [[[0, 127, 254]]]
    # tensor2img: clamp, (x+1)/2*255, round half to even, RGB->BGR
    vals = torch.tensor([-1.2, -1.0, -0.5 / 255, 0.0, 1.0 / 255, 1.0, 1.3, 0.00392156862])
    t = vals.view(1, 1, -1).repeat(3, 1, 1)
    got = U.net_output_to_bgr_u8(t)[0, :, 0]
    exp = np.round((np.clip(vals.numpy(), -1, 1) + 1) / 2 * 255.0).astype(np.uint8)
    assert got.tolist() == exp.tolist()
    assert got[3] == 128 and got[0] == 0 and got[6] == 255            # 127.5 -> 128 (half to even)
    # crops -> net input: float32(u8/255.) then (x-0.5)/0.5, BGR->RGB
    crop = synth.ramp_image(4, 4)
    x = U.crops_to_net_input([crop])
    ref = ((crop / 255.).astype(np.float32)[..., ::-1].transpose(2, 0, 1) - np.float32(0.5)) / np.float32(0.5)
    assert np.array_equal(x[0].numpy(), ref)
    # round trip of exact grid values
    assert np.array_equal(U.net_output_to_bgr_u8(x[0]), crop)


@pytest.mark.parametrize("n,l", [(1, 20), (2, 20), (19, 20), (20, 20), (21, 20), (41, 20), (5, 1)])
def test_chunk_boundaries(n, l):
    chunks = split_clips(n, l)
    assert chunks[0][0] == 0 and chunks[-1][1] == n
    assert all(e - s <= l and e > s for s, e in chunks)
    assert all(chunks[i][1] == chunks[i + 1][0] for i in range(len(chunks) - 1))
    assert len(chunks) == -(-n // l)


class _RecordingNet:
    """keep_net stand-in: output = input + clip_index, records the clip lengths it was given."""

    def __init__(self):
        self.calls = []

    def __call__(self, x, need_upscale=True):
        assert need_upscale is False
        self.calls.append(x.shape[1])
        return x + float(len(self.calls))

    def to(self, d):
        return self


class _Helper:
    def clean_all(self):
        pass


def _pack(net):
    return KEEPModelPack(net, _Helper(), None, None, 'KEEP')


def test_sequence_clip_loop_aligned():
    net = _RecordingNet()
    proc = KEEPFaceProcessor(_pack(net))
    frames = torch.rand(41, 512, 512, 3)
    out = proc.process_image_sequence(frames, 1.0, True, True, False, max_clip_length=20)
    assert net.calls == [20, 20, 2]                    # 41 = 20 + 20 + 1, the singleton is duplicated to T=2
    assert len(proc.last_restored_faces) == 41
    # reference quirk P2: aligned sequences return the (resized) input, restored faces are discarded
    assert out.shape == (41, 512, 512, 3)
    assert torch.equal(out, (frames * 255).to(torch.uint8).float() / 255.0)
    from comfy.utils import ProgressBar
    assert ProgressBar.last.current == 41 * 3          # no paste ticks on the aligned path (Appendix A.2)


def test_sequence_aligned_fix_flag_returns_restored_faces():
    """Opt-in fix of reference quirk P2: with return_restored_aligned the aligned-sequence node returns the restored
    faces (here 255 - crop through the uint8 entry point) instead of its input; default stays bug-compatible."""
    net = _U8Net(True)
    proc = KEEPFaceProcessor(_pack(net))
    frames = torch.rand(3, 512, 512, 3)
    u8 = (frames * 255).to(torch.uint8)
    out_default = proc.process_image_sequence(frames, 1.0, True, True, False, max_clip_length=2)
    assert torch.equal(out_default, u8.float() / 255.0)
    proc.return_restored_aligned = True
    out_fixed = proc.process_image_sequence(frames, 1.0, True, True, False, max_clip_length=2)
    assert out_fixed.shape == (3, 512, 512, 3)
    assert torch.equal(out_fixed, (255 - u8).float() / 255.0)


def test_single_image_aligned_duplicates_to_T2():
    net = _RecordingNet()
    proc = KEEPFaceProcessor(_pack(net))
    img = synth.ramp_image()
    out = proc.process_image(img, 1.0, True, True, False)
    assert net.calls == [2] and out.shape == (512, 512, 3) and out.dtype == np.uint8


class _U8Net(_RecordingNet):
    """engine stand-in offering the device-side uint8 entry point: output clip = 255 - input, records clip lengths."""

    def __init__(self, single_frame):
        super().__init__()
        self.supports_single_frame = single_frame

    def run_clips_u8(self, clips, max_b=4):
        # contract of KeepNet.run_clips_u8: a clip is a uint8 [T,H,W,3] tensor or a list of T uint8 [H,W,3] crops
        clips = [torch.from_numpy(np.stack(c)) if isinstance(c, list) else c for c in clips]
        for c in clips:
            assert c.dtype == torch.uint8 and c.dim() == 4 and c.shape[1:] == (512, 512, 3)
            self.calls.append(c.shape[0])
        return [255 - c for c in clips]


@pytest.mark.parametrize("single_frame", [True, False])
def test_uint8_entry_point_chunking_and_lone_crops(single_frame):
    """SURVEY 8f-1 host logic: crops are handed over as uint8 clips chunked like keep_processor.py:263-270; a lone crop goes
    as T=1 when the engine supports it, else as the reference's T=2 duplicate with frame 0 kept -- same restored faces."""
    net = _U8Net(single_frame)
    proc = KEEPFaceProcessor(_pack(net))
    base = synth.ramp_image()
    crops = [np.ascontiguousarray(np.roll(base, k, axis=0)) for k in range(5)]
    faces = proc._restore_crops_u8(crops, 2)
    assert net.calls == ([2, 2, 1] if single_frame else [2, 2, 2])
    assert len(faces) == 5 and all(f.dtype == np.uint8 and f.shape == (512, 512, 3) for f in faces)
    assert all(np.array_equal(f, 255 - c) for f, c in zip(faces, crops))
    out = proc.process_image(base, 1.0, True, True, False)           # single-image node, aligned input
    assert net.calls[-1] == (1 if single_frame else 2) and np.array_equal(out, 255 - base)


def test_legacy_key_conversion_and_param_selection():
    sd = {'cross_fuse.16.norm1.weight': 1, 'fuse_convs_dict.32.scale.0.bias': 2, 'encoder.blocks.0.weight': 3}
    out = convert_legacy_keys(sd)
    assert set(out) == {'cfa.16.norm1.weight', 'cft.32.scale.0.bias', 'encoder.blocks.0.weight'}
    assert select_params({'params_ema': 'a', 'params': 'b'}) == 'a'
    assert select_params({'params': 'b'}) == 'b'
    plain = {'x': 1}
    assert select_params(plain) is plain


def test_strict_load_rejects_bad_state_dict(synth_weights):
    from comfyui_keep_amd.engine.net import KeepNet
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    net = KeepNet(**DEFAULT_ARCH)
    bad = dict(synth_weights)
    bad.pop('position_emb')
    with pytest.raises(RuntimeError, match='Missing key'):
        net.load_state_dict(bad, strict=True)
    bad = dict(synth_weights, extra=torch.zeros(1))
    with pytest.raises(RuntimeError, match='Unexpected key'):
        net.load_state_dict(bad, strict=True)


def test_gmflow_conv1_as_a_4x4_convolution_on_the_space_to_depth_image():
    """engine/weights.py:s2d_weights_7x7 + the layout keep_rgb_s2d writes: the 7x7 stride-2 pad-3 convolution of GMFlow's encoder
    (GM/backbone.py:69) equals a 4x4 stride-1 convolution (pad 2 top / left, 1 bottom / right) on the 2x2 space-to-depth image with
    channel (dy*2 + dx)*3 + c -- float64, every output."""
    from comfyui_keep_amd.engine.weights import s2d_weights_7x7
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 20, 28, generator=g, dtype=torch.float64)
    w = torch.randn(8, 3, 7, 7, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv2d(x, w, stride=2, padding=3)
    ws = s2d_weights_7x7(w.permute(0, 2, 3, 1).contiguous())                       # packed [Cout,7,7,3] -> [Cout,4,4,16]
    assert ws.shape == (8, 4, 4, 16) and float(ws[:, 0, :, 0:6].abs().max()) == 0.0 and float(ws[..., 12:].abs().max()) == 0.0
    N, C, H, W = x.shape
    s2d = x.view(N, C, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(N, 12, H // 2, W // 2)      # channel (dy*2+dx)*3 + c
    s2d = torch.nn.functional.pad(s2d, (2, 1, 2, 1))
    got = torch.nn.functional.conv2d(s2d, ws[..., :12].permute(0, 3, 1, 2))
    assert got.shape == ref.shape and float((got - ref).abs().max()) < 1e-12


def test_packed_blob_layouts(synth_weights):
    from comfyui_keep_amd.engine.weights import logical_tensors, pack_blob, views
    lt = logical_tensors(synth_weights)
    w = synth_weights['encoder.blocks.1.conv1.weight']
    assert torch.equal(lt['encoder.blocks.1.conv1.weight'], w.permute(0, 2, 3, 1))
    assert lt['encoder.blocks.17.qkv.weight'].shape == (1536, 512)
    assert torch.equal(lt['encoder.blocks.17.qkv.weight'][512:1024], synth_weights['encoder.blocks.17.k.weight'].view(512, 512))
    assert lt['cft.32.ss0.weight'].shape == (512, 3, 3, 256)
    assert lt['cfa.16.attn.to_kv.weight'].shape == (2048, 512)
    assert lt['flownet.model.transformer.layers.0.self_attn.qkv.weight'].shape == (384, 128)
    assert 'encoder.blocks.17.q.weight' not in lt
    blob, index = pack_blob(lt)
    v = views(torch.from_numpy(blob), index)
    assert all(off % 64 == 0 for off, _ in index.values())
    assert torch.equal(v['position_emb'], synth_weights['position_emb'])
    # the one ragged 3x3 convolution (GMFlow upsampler.0, Cin = 2 + 128) carries zero input columns up to 144
    up, src = lt['flownet.model.upsampler.0.weight'], synth_weights['flownet.model.upsampler.0.weight']
    assert up.shape == (256, 3, 3, 144) and torch.equal(up[..., :130], src.permute(0, 2, 3, 1)) and not up[..., 130:].any()
    n_in = sum(t.numel() for t in synth_weights.values())
    # ... and GMFlow's 7x7 stride-2 first convolution a derived [64,4,4,16] twin for the space-to-depth form (keep_rgb_s2d)
    assert lt['flownet.model.backbone.conv1.weight_s2d'].shape == (64, 4, 4, 16)
    # ... and (round 6) every CFT block's encode_enc first convolution and 1x1 shortcut once more as their encoder / decoder input-channel
    # halves (engine/net.py:_cft_enc_part): the same numbers, sliced
    for sz, C in (('16', 512), ('32', 256), ('64', 256)):
        q = f'cft.{sz}.encode_enc'
        full, sc = lt[f'{q}.conv1.weight'], lt[f'{q}.conv_out.weight']
        assert full.shape == (C, 3, 3, 2 * C) and sc.shape == (C, 2 * C)
        assert torch.equal(torch.cat([lt[f'{q}.conv1.weight_enc'], lt[f'{q}.conv1.weight_dec']], -1), full)
        assert torch.equal(torch.cat([lt[f'{q}.conv_out.weight_enc'], lt[f'{q}.conv_out.weight_dec']], -1), sc)
    halves = sum(C * 9 * 2 * C + C * 2 * C for C in (512, 256, 256))
    assert sum(t.numel() for t in lt.values()) == n_in + 256 * 9 * 14 + 64 * 4 * 4 * 16 + halves


def test_face_tracking_restatement():
    from comfyui_keep_amd.modules.face_tracks import interpolate_sequence, smooth_center_face, track_faces
    s = np.array([1.0, np.nan, 3.0, np.nan, np.nan, 6.0])
    assert np.allclose(interpolate_sequence(s), [1, 2, 3, 4, 5, 6])
    lm = lambda cx: np.tile(np.array([[cx, 10.0]]), (5, 1))  # noqa: E731
    tracks = track_faces([[lm(10), lm(300)], [lm(305), lm(12)], [], [lm(14)]])
    assert len(tracks) == 3                                    # the face re-appearing after a gap starts a new track
    assert np.allclose(tracks[0][1], lm(12)) and np.allclose(tracks[1][1], lm(305))
    assert np.isnan(tracks[0][2]).all() and np.isnan(tracks[0][3]).all()
    sm = smooth_center_face([[lm(10)], [], [lm(30)]])
    assert sm[0].shape == (3, 5, 2) and not np.isnan(sm[0]).any()


def test_model_pack_moves_a_yolo_detector_that_has_no_to():
    """the reference's YoloDetector is a plain class without .to(); load_device() / offload() must move its network
    (`.detector`) and retarget `.device` instead of raising AttributeError."""
    class _Net:
        def __init__(self):
            self.where = None

        def to(self, d):
            self.where = d
            return self

    class _Yolo:
        def __init__(self):
            self.detector, self.device = _Net(), 'cpu'

    helper = _Helper()
    helper.face_detector, helper.face_parse = _Yolo(), _Net()
    pack = KEEPModelPack(None, helper, None, None, 'KEEP')
    pack.load_device()
    assert helper.face_detector.detector.where == pack.device and helper.face_detector.device == pack.device
    assert helper.face_parse.where == pack.device and helper.device == pack.device
    pack.offload()
    assert helper.face_detector.detector.where == pack.offload_device and helper.face_detector.device == pack.offload_device


def test_c_abi_exports_every_declared_symbol():
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    declared = set(re.findall(r'\b(keep_[a-z0-9_]+)\s*\(', header))
    assert declared == set(hiplib.EXPORTED_SYMBOLS)
    assert os.path.exists(hiplib.LIB_PATH), "run `python __graft_entry__.py` (build) first"
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    for sym in declared:
        assert hasattr(lib, sym), sym
    lib.keep_abi_version.restype = ctypes.c_int32
    assert lib.keep_abi_version() == hiplib.ABI_VERSION
    hiplib.load(check_device=False)                             # binds every signature
    # argument validation is host-side C: callable without a GPU
    lib.keep_last_error.restype = ctypes.c_char_p
    lib.keep_conv2d.restype = ctypes.c_int32
    assert lib.keep_conv2d(None, None) == -1 and b'null args' in lib.keep_last_error()


def _header_struct_fields(header, name):
    """Field names of `typedef struct { ... } name;` in declaration order (comments stripped, `a, b, c;` lists expanded)."""
    end = re.search(r'\}\s*' + name + r'\s*;', header).start()
    body = header[header.rindex('typedef struct {', 0, end) + len('typedef struct {'):end]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(',')
        m = re.search(r'(\w+)\s*(\[\d+\])?$', first.strip())
        names.append(m.group(1))
        names += [r.strip().lstrip('*').strip() for r in rest]
    return names


def test_abi_struct_layouts_match_header_library_and_doc():
    """The three descriptions of the argument structs -- include/keep_hip.h, the ctypes binding, the built library -- and
    the copy printed in INTEGRATION.md agree: field names and order (header vs binding), byte size (binding vs
    keep_sizeof_*_args() of the built .so), documented listing (generated from the binding, tools/gen_abi_doc.py)."""
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    assert int(re.search(r'#define KEEP_ABI_VERSION (\d+)', header).group(1)) == hiplib.ABI_VERSION
    rename = {'inp': 'in'}
    for cname, cls in (('keep_conv2d_args', hiplib.ConvArgs), ('keep_conv2d_plan_out', hiplib.ConvPlanOut),
                       ('keep_attention_args', hiplib.AttnArgs)):
        assert [rename.get(n, n) for n, _ in cls._fields_] == _header_struct_fields(header, cname), cname
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_sizeof_conv2d_args.restype = lib.keep_sizeof_attention_args.restype = ctypes.c_int32
    assert lib.keep_sizeof_conv2d_args() == ctypes.sizeof(hiplib.ConvArgs)
    assert lib.keep_sizeof_attention_args() == ctypes.sizeof(hiplib.AttnArgs)
    assert hiplib.ConvArgs._fields_[0][0] == 'struct_size' and hiplib.AttnArgs._fields_[0][0] == 'struct_size'
    # the v12 minimum sizes the header promises to keep accepting are not larger than today's structs
    for macro, cls in (('KEEP_CONV2D_ARGS_V12_SIZE', hiplib.ConvArgs), ('KEEP_ATTENTION_ARGS_V12_SIZE', hiplib.AttnArgs)):
        assert int(re.search(rf'#define {macro} (\d+)', header).group(1)) <= ctypes.sizeof(cls)
    # a struct_size the library does not know is refused before anything is read
    lib.keep_last_error.restype = ctypes.c_char_p
    lib.keep_conv2d_plan.restype = ctypes.c_int32
    a, out = hiplib.ConvArgs(), hiplib.ConvPlanOut()
    for bad in (0, 128, ctypes.sizeof(hiplib.ConvArgs) + 8):
        a.struct_size = bad
        assert lib.keep_conv2d_plan(ctypes.byref(a), ctypes.byref(out)) == -1 and b'struct_size' in lib.keep_last_error()
    # the plan query itself is host-side C: a well-formed struct is answered without a GPU
    a = hiplib.ConvArgs(struct_size=ctypes.sizeof(hiplib.ConvArgs), N=2, H=64, W=64, Cin=128, Cout=128, KH=3, KW=3, stride=1,
                        pad_t=1, pad_l=1, Ho=64, Wo=64, in_ld=128, out_ld=128, mma=hiplib.MMA_F32)
    assert lib.keep_conv2d_plan(ctypes.byref(a), ctypes.byref(out)) == 0, lib.keep_last_error()
    assert out.kernel.decode().startswith('conv3x3_halo_f32_kernel')


def test_library_sources_have_no_build_switches():
    """The kernels say only what they do: no preprocessor conditional and no dev / ablation switch anywhere under csrc/ (the
    measurements those switches made are recorded in DESIGN.md and profiles/)."""
    csrc = os.path.join(ROOT, 'comfyui-keep_amd', 'csrc')
    cond = re.compile(r'^[ \t]*#[ \t]*(if|elif)\w*\b', re.M)
    found = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(('.hip', '.h')):
            continue
        text = open(os.path.join(csrc, f)).read()
        found += [f'{f}: {m.group(0).strip()}' for m in cond.finditer(text)]
        found += [f'{f}: {s}' for s in ('KEEP_DEV_ENV', '_ABL', 'KEEP_X3_ABLATE') if s in text]
    assert not found, found


def test_library_reads_no_environment_variable_and_flags_steer_the_plan(monkeypatch):
    """libkeep_hip.so reads no environment variable, in any build; what used to be
    KEEP_NO_* / KEEP_PLAN_REF_IMAGES / KEEP_GATHER_SMALL_M travels in keep_conv2d_args.flags / .plan_ref_images."""
    import subprocess
    from comfyui_keep_amd.engine import hiplib
    csrc = os.path.join(ROOT, 'comfyui-keep_amd', 'csrc')
    n_getenv = sum(open(os.path.join(csrc, f)).read().count('getenv') for f in os.listdir(csrc) if f.endswith(('.hip', '.h')))
    assert n_getenv == 0, n_getenv
    syms = subprocess.run(['nm', '-D', '--undefined-only', hiplib.LIB_PATH], capture_output=True, text=True).stdout
    assert 'getenv' not in syms, "the default build must not import getenv"
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_conv2d_plan.restype = ctypes.c_int32
    lib.keep_last_error.restype = ctypes.c_char_p

    def plan(**kw):
        base = dict(struct_size=ctypes.sizeof(hiplib.ConvArgs), N=1, H=64, W=64, Cin=128, Cout=128, KH=3, KW=3, stride=1, pad_t=1,
                    pad_l=1, Ho=64, Wo=64, in_ld=128, out_ld=128, mma=hiplib.MMA_F32)
        base.update(kw)
        out = hiplib.ConvPlanOut()
        assert lib.keep_conv2d_plan(ctypes.byref(hiplib.ConvArgs(**base)), ctypes.byref(out)) == 0, lib.keep_last_error()
        return out.kernel.decode(), out.split_k

    ref = plan()
    assert ref[0].startswith('conv3x3_halo_f32_kernel')
    for k in ('KEEP_NO_HALO_F32', 'KEEP_NO_HALO_X3', 'KEEP_NO_COUT4', 'KEEP_NO_C3', 'KEEP_NO_PLAIN', 'KEEP_X3_NO_STREAM'):
        monkeypatch.setenv(k, '1')
    monkeypatch.setenv('KEEP_PLAN_REF_IMAGES', '1')
    monkeypatch.setenv('KEEP_GATHER_SMALL_M', '1')
    assert plan() == ref                                                          # the environment is not looked at
    assert not plan(flags=hiplib.CONV_NO_HALO_F32)[0].startswith('conv3x3_halo_f32_kernel')      # ... the flag is
    # the reference batch of the plans: 16 images of 16x16 need no deeper split than 1 image's plan under reference 1
    g16 = dict(H=16, W=16, Ho=16, Wo=16, Cin=512, Cout=512, in_ld=512, out_ld=512)
    assert plan(plan_ref_images=1, **g16)[1] > plan(**g16)[1] and plan(plan_ref_images=16, **g16) == plan(**g16)
    small = dict(H=2304, W=1, Ho=2304, Wo=1, KH=1, KW=1, pad_t=0, pad_l=0, Cin=128, Cout=192, in_ld=128, out_ld=192)
    assert '2, 2, 2, 2' in plan(**small)[0] and '2, 2, 1, 1' in plan(flags=hiplib.CONV_SMALL_TILES, **small)[0]


def test_integration_doc_matches_the_binding():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_abi_doc
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    a, b = doc.index(gen_abi_doc.BEGIN), doc.index(gen_abi_doc.END) + len(gen_abi_doc.END)
    assert doc[a:b] == gen_abi_doc.block(), "INTEGRATION.md section 3 is stale: run python tools/gen_abi_doc.py"


def test_plan_is_batch_invariant_in_the_parity_policies():
    """keep_conv2d_plan (host-side C, no GPU needed): under the exact-f32 policy the split-K factor, the kernel and the
    statistics partition of a layer are the same for 1, 3, 16 and 320 images -- a clip's sums never depend on its
    batch-mates."""
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_conv2d_plan.restype = ctypes.c_int32
    lib.keep_last_error.restype = ctypes.c_char_p
    geoms = [(16, 16, 512, 512, 3), (32, 32, 256, 256, 3), (64, 64, 256, 128, 3), (256, 256, 128, 128, 3), (256, 1, 512, 1024, 1),
             (4096, 1, 128, 384, 1), (16, 16, 512, 1536, 1)]
    for H, W, Cin, Cout, k in geoms:
        seen = set()
        for N in (1, 3, 16, 320):
            a = hiplib.ConvArgs(struct_size=ctypes.sizeof(hiplib.ConvArgs), N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=k, KW=k,
                                stride=1, pad_t=k // 2, pad_l=k // 2, Ho=H, Wo=W, in_ld=Cin, out_ld=Cout, mma=hiplib.MMA_F32)
            out = hiplib.ConvPlanOut()
            assert lib.keep_conv2d_plan(ctypes.byref(a), ctypes.byref(out)) == 0, lib.keep_last_error()
            seen.add((out.split_k, out.kernel, out.stats_rows, out.stats_P))
        assert len(seen) == 1, (H, W, Cin, Cout, k, seen)


def test_plan_layernorm_epilogue_rules():
    """keep_conv2d_plan (host-side C): ln_gamma is accepted only where the LayerNorm epilogue exists -- the x3 GEMM form with
    128 output channels and whole 128-row tiles -- and refused with KEEP_EUNSUP (-2) everywhere else, never silently dropped."""
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_conv2d_plan.restype = ctypes.c_int32
    lib.keep_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 4096)()
    ptr = (ctypes.addressof(buf) + 63) // 64 * 64

    def plan(**kw):
        base = dict(struct_size=ctypes.sizeof(hiplib.ConvArgs), N=2, H=4096, W=1, Cin=128, Cout=128, KH=1, KW=1, stride=1, pad_t=0,
                    pad_l=0, Ho=4096, Wo=1, in_ld=128, out_ld=128, mma=hiplib.MMA_X3, inp=ptr, out=ptr, weight=ptr, weight_x3=ptr,
                    x3_acc_scale=1.0, ln_gamma=ptr, ln_beta=ptr, ln_eps=1e-5)
        base.update(kw)
        out = hiplib.ConvPlanOut()
        rc = lib.keep_conv2d_plan(ctypes.byref(hiplib.ConvArgs(**base)), ctypes.byref(out))
        return rc, out.kernel.decode(), out.split_k

    rc, kernel, sk = plan()
    assert rc == 0 and 'LayerNorm' in kernel and '<4, 1, 1, 4' in kernel and sk == 1, (rc, kernel, lib.keep_last_error())
    assert plan(Cin=1024, in_ld=1024)[0] == 0
    assert plan(ln_gamma=None, ln_beta=None)[1].startswith('conv_x3_kernel<2, 2, 2, 2')         # unchanged without it
    for bad in (dict(Cout=256, out_ld=256), dict(H=4000, Ho=4000), dict(epi_act=hiplib.ACT_GELU), dict(mma=hiplib.MMA_F32),
                dict(KH=3, KW=3, pad_t=1, pad_l=1, H=64, W=64, Ho=64, Wo=64), dict(split_k=2), dict(ln_beta=None)):
        rc, kernel, _ = plan(**bad)
        assert rc == -2 and b'ln_gamma' in lib.keep_last_error(), (bad, rc, kernel)


def test_attention_window_shift_is_zero_or_half_a_window():
    """keep_attention (host-side C): the region mask and the per-axis roll (wh/2, ww/2, GM/transformer.py:75-80) assume half a
    window, so a window-mode call with any other shift is refused with KEEP_EINVAL before anything launches."""
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_attention.restype = ctypes.c_int32
    lib.keep_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) // 64 * 64
    h, w, C = 40, 56, 128                        # windows 20 x 28: wh/2 = 10, ww/2 = 14
    for bad in (1, 5, 14, 19, 20, -10):
        s = (h * w * C, C, 0)
        a = hiplib.AttnArgs(struct_size=ctypes.sizeof(hiplib.AttnArgs), q=ptr, k=ptr, v=ptr, o=ptr, q_bs=s[0], q_ts=s[1], k_bs=s[0],
                            k_ts=s[1], v_bs=s[0], v_ts=s[1], o_bs=s[0], o_ts=s[1], B=8, H=1, Lq=560, Lk=560, D=C, Dv=C, scale=0.1,
                            mode=2, img_h=h, img_w=w, ksplit=2, shift=bad, kv_rot=1, n_img=2, mma=hiplib.MMA_X3)
        assert lib.keep_attention(ctypes.byref(a), None) == -1, bad
        assert b'shift' in lib.keep_last_error(), (bad, lib.keep_last_error())


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, 'comfyui-keep_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert 'keep_oracle' not in src and 'ref_import' not in src and 'import oracle' not in src, f


def test_paste_hook_defers_to_the_helper():
    """the GPU paste is opt-in and only takes the configuration it restates; everything else is the helper's
    own paste_faces_to_input_image with the reference's arguments."""
    calls = []

    class Hp(_Helper):
        use_parse, is_gray, upscale_factor, face_size = True, False, 1, (512, 512)
        face_parse = object()

        def paste_faces_to_input_image(self, upsample_img=None, draw_box=False, face_upsampler=None):
            calls.append((draw_box, face_upsampler))
            return upsample_img

    h = Hp()
    proc = KEEPFaceProcessor(KEEPModelPack(_RecordingNet(), h, None, None, 'KEEP'))
    bg = np.zeros((64, 64, 3), np.uint8)
    h.input_img, h.restored_faces, h.inverse_affine_matrices = bg, [np.zeros((512, 512, 3), np.uint8)], [np.eye(2, 3)]
    # unset environment = 'auto': the first paste self-checks the HIP path against cv2; without cv2 (this image) / without a GPU
    # it settles on the helper's own path
    assert proc.gpu_paste is None and proc._paste(h, bg, False) is bg and calls == [(False, None)]
    assert proc.gpu_paste is False
    proc.gpu_paste = True
    assert proc._gpu_paste_applies(h, bg, False)
    assert proc._gpu_paste_applies(h, bg, True)                                      # draw_box: on the device too (keep_draw_box)
    assert not proc._gpu_paste_applies(h, bg.astype(np.float32), False)              # not uint8
    assert not proc._gpu_paste_applies(h, np.zeros((32, 32, 3), np.uint8), False)    # background still to be resized
    h.use_parse = False
    # the erosion-mask path (face_restoration_helper.py:386-415) is on the device too, but it is not part of the cv2 self-check:
    # only an explicit KEEP_AMD_GPU_PASTE=1 turns it on
    assert not proc._gpu_paste_applies(h, bg, False)
    proc._gpu_paste_forced = True
    assert proc._gpu_paste_applies(h, bg, False)
    h.use_parse, proc.face_upscale_model = True, object()
    assert not proc._gpu_paste_applies(h, bg, False)


def test_batched_detection_prepass_equals_the_per_frame_loop():
    """SURVEY 8f-4 host logic: with a detector that offers ``detect_batch`` the processor runs ONE batched detection over the
    video and lets the helper post-process each frame from the stored result; landmarks must equal the per-frame loop's
    (keep_processor.py:207-213), the helper's own ``get_face_landmarks_5`` is called once per frame either way."""
    class Det:
        def __init__(self):
            self.single_calls, self.batch_calls = 0, 0

        def _res(self, img):
            k = float(img[0, 0, 0])                      # result depends on the frame content only
            return np.array([[k, 1, k + 50, 60, 0.99] + [k + 10, 20, k + 30, 20, k + 20, 30, k + 12, 40, k + 28, 40]], np.float32)

        def detect_faces(self, img, thr=0.8):
            self.single_calls += 1
            return self._res(img)

    class BatchDet(Det):
        def detect_batch(self, frames, thr=0.8):
            self.batch_calls += 1
            assert frames.ndim == 4 and thr == 0.97
            return [self._res(f) for f in frames]

    class Helper:
        det_model = 'retinaface_resnet50'

        def __init__(self, det):
            self.face_detector = det
            self.calls = 0

        def clean_all(self):
            self.all_landmarks_5, self.input_img = [], None

        def read_image(self, img):
            self.input_img = img

        def get_face_landmarks_5(self, only_center_face=False, resize=640, eye_dist_threshold=None):
            self.calls += 1
            b = self.face_detector.detect_faces(self.input_img, 0.97)
            self.all_landmarks_5 = [b[i, 5:].reshape(5, 2) for i in range(b.shape[0])]
            return len(self.all_landmarks_5)

    frames = [np.full((64, 80, 3), 7 * i, np.uint8) for i in range(5)]
    out = {}
    for name, det in (('loop', Det()), ('batch', BatchDet())):
        helper = Helper(det)
        proc = KEEPFaceProcessor(KEEPModelPack(_RecordingNet(), helper, None, None, 'KEEP'))
        out[name] = proc._detect_all(frames, True)
        assert helper.calls == 5 and helper.face_detector is det
        assert (det.single_calls, det.batch_calls) == ((5, 0) if name == 'loop' else (0, 1))
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(out['loop'], out['batch']))


def test_detection_prepass_overlaps_chunks_without_changing_results(monkeypatch):
    """Round 6: with several chunks of detector frames the forward of chunk k runs on a worker thread under the host preparation of
    chunk k + 1 (KEEP_AMD_DETECT_OVERLAP, default on).  Same landmarks as the one-after-the-other order and as the per-frame loop, every
    chunk prepared exactly once and in order, the detector called once per chunk from ONE worker thread; an exception inside the
    detector's forward surfaces in the caller."""
    import threading
    import types
    log = []

    class Det:
        def __init__(self, fail_at=None):
            self.engine = types.SimpleNamespace(max_frames=4)         # chunks of four frames
            self.threads, self.fail_at, self.n = set(), fail_at, 0

        def detect_batch(self, frames, thr=0.8):
            self.threads.add(threading.get_ident())
            log.append(('forward', int(frames[0, 0, 0, 0])))
            self.n += 1
            if self.fail_at == self.n:
                raise RuntimeError('detector down')
            return [np.array([[float(f[0, 0, 0]), 1, float(f[0, 0, 0]) + 50, 60, 0.99] + list(np.arange(10, dtype=np.float32) + float(f[0, 0, 0]))], np.float32)
                    for f in frames]

    class Helper:
        det_model = 'retinaface_resnet50'

        def __init__(self, det):
            self.face_detector = det

        def clean_all(self):
            self.all_landmarks_5, self.input_img = [], None

        def read_image(self, img):
            self.input_img = img
            log.append(('read', int(img[0, 0, 0])))

        def get_face_landmarks_5(self, only_center_face=False, resize=640, eye_dist_threshold=None):
            b = self.face_detector.detect_faces(self.input_img, 0.97)
            self.all_landmarks_5 = [b[i, 5:].reshape(5, 2) for i in range(b.shape[0])]
            return len(self.all_landmarks_5)

    frames = [np.full((32, 40, 3), i, np.uint8) for i in range(10)]
    outs = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('KEEP_AMD_DETECT_OVERLAP', mode)
        del log[:]
        det = Det()
        proc = KEEPFaceProcessor(KEEPModelPack(_RecordingNet(), Helper(det), None, None, 'KEEP'))
        outs[mode] = proc._detect_all(frames, True)
        assert [v for k, v in log if k == 'read'] == list(range(10))               # every frame prepared once, in order
        assert [v for k, v in log if k == 'forward'] == [0, 4, 8]                  # one forward per chunk, in order
        assert len(det.threads) == 1 and (threading.get_ident() in det.threads) == (mode == '0')
        if mode == '1':      # chunk 1 was prepared (reads 4..7) before chunk 0's forward was collected: the read of frame 4 precedes nothing that needs chunk 0's result
            assert log.index(('read', 4)) < log.index(('forward', 4))
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(outs['1'], outs['0'])) and len(outs['1']) == 10
    assert all(float(outs['1'][i][0][0, 0]) == float(i) for i in range(10))
    monkeypatch.setenv('KEEP_AMD_DETECT_OVERLAP', '1')
    proc = KEEPFaceProcessor(KEEPModelPack(_RecordingNet(), Helper(Det(fail_at=2)), None, None, 'KEEP'))
    with pytest.raises(RuntimeError, match='detector down'):
        proc._detect_all(frames, True)


def test_frames_from_comfy_host_fallbacks():
    """modules/keep_processor.py:frames_from_comfy without a GPU: a CPU device (and, on any device, inputs the device kernel does not take)
    yield the per-frame host converter's frames as a plain list -- the reference's `comfy_image_to_cv2` per frame."""
    from comfyui_keep_amd.modules import keep_processor as KPm
    from comfyui_keep_amd.modules.utils import comfy_image_to_cv2
    seq = torch.rand((3, 8, 10, 3), generator=torch.Generator().manual_seed(0))
    got = KPm.frames_from_comfy(seq, 'cpu')
    assert isinstance(got, list) and len(got) == 3
    assert all(np.array_equal(g, comfy_image_to_cv2(seq[i])) and g.dtype == np.uint8 and g.shape == (8, 10, 3) for i, g in enumerate(got))
    assert isinstance(KPm.frames_from_comfy(seq.double(), 'cuda'), list)          # not float32: the host converter, whatever the device


def test_device_crop_warp_hook_keeps_the_helper_contract(monkeypatch):
    """8f-2 host logic: with the GPU cv path on, ``_align_warp`` fits the similarity on the host (cv2.estimateAffinePartial2D) and
    crops on the device, filling ``affine_matrices`` / ``cropped_faces`` exactly like ``align_warp_face``; pad_blur or the cv path
    being off defers to the helper."""
    from comfyui_keep_amd.modules import keep_processor as KPm
    from comfyui_keep_amd.engine import paste as gp
    calls = []

    class Cv2:
        LMEDS = 4

        @staticmethod
        def estimateAffinePartial2D(lm, tmpl, method=None):
            return (np.array([[1.0, 0.0, float(lm[0, 0])], [0.0, 1.0, 0.0]]), None)

    class Hp(_Helper):
        pad_blur, face_size, face_template = False, (512, 512), np.zeros((5, 2))

        def __init__(self):
            self.affine_matrices, self.cropped_faces = [], []
            self.all_landmarks_5 = [np.full((5, 2), 3.0), np.full((5, 2), 7.0)]
            self.input_img = np.zeros((64, 64, 3), np.uint8)

        def align_warp_face(self):
            calls.append('helper')

    monkeypatch.setattr(KPm, '_cv2', lambda: Cv2)
    monkeypatch.setattr(gp, 'crop_faces', lambda frame, mats, size, dev: torch.zeros((len(mats), size[1], size[0], 3), dtype=torch.uint8))
    h = Hp()
    proc = KEEPFaceProcessor(KEEPModelPack(_RecordingNet(), h, None, None, 'KEEP'))
    proc.gpu_paste = True
    proc._align_warp(h)
    assert calls == [] and len(h.cropped_faces) == 2 and h.cropped_faces[0].shape == (512, 512, 3)
    assert [float(m[0, 2]) for m in h.affine_matrices] == [3.0, 7.0]
    h.pad_blur = True
    proc._align_warp(h)
    proc.gpu_paste, h.pad_blur = False, False
    proc._align_warp(h)
    assert calls == ['helper', 'helper']


def test_loader_swaps_the_helpers_networks_for_engine_objects(monkeypatch):
    """SURVEY 8f-4 host logic: ``engine_facelib`` replaces a ParseNet-shaped ``face_parse`` and a RetinaFace(resnet50 | mobile0.25)-shaped
    ``face_detector`` by engine-backed objects with the same call surface (weights packed on the host, nothing uploaded until
    ``.to('cuda')``), leaves other detectors alone, and KEEP_AMD_ENGINE_FACELIB=0 switches the swap off."""
    from comfyui_keep_amd.modules.keep_model_loader import engine_facelib
    from comfyui_keep_amd.engine import parsenet as PN, retinaface as RF

    class FakeModule:
        def __init__(self, sd, **attrs):
            self._sd = sd
            self.__dict__.update(attrs)

        def state_dict(self):
            return self._sd

    class Hp:
        pass
    h = Hp()
    h.face_parse = FakeModule(PN.synth_parsenet_state_dict(seed=0, in_size=128, out_size=128))
    h.face_detector = FakeModule(RF.synth_retinaface_state_dict(seed=0), backbone='Resnet50')
    engine_facelib(h)
    assert isinstance(h.face_parse, PN.EngineFaceParse) and (h.face_parse.engine.in_size, h.face_parse.engine.out_size) == (128, 128)
    assert isinstance(h.face_detector, RF.EngineRetinaFace) and h.face_detector.engine.w is None      # packed, not uploaded
    assert callable(h.face_detector.detect_faces) and callable(h.face_detector.detect_batch)
    with pytest.raises(RuntimeError):
        h.face_parse.engine.logits_nhwc(torch.zeros(1, 128, 128, 3))                                   # loud: not on a device
    h2 = Hp()
    h2.face_parse = object()                                    # not a ParseNet: untouched
    h2.face_detector = FakeModule({}, backbone='YOLOv5')       # no engine counterpart: untouched
    det2 = h2.face_detector
    engine_facelib(h2)
    assert h2.face_detector is det2 and not isinstance(h2.face_parse, PN.EngineFaceParse)
    hm = Hp()                                                   # retinaface_mobile0.25 (detection/__init__.py:38-41)
    hm.face_detector = FakeModule(RF.synth_retinaface_state_dict(seed=0, backbone='mobile0.25'), backbone='mobilenet0.25')
    engine_facelib(hm)
    assert isinstance(hm.face_detector, RF.EngineRetinaFace) and hm.face_detector.engine.backbone == 'mobile0.25'
    assert hm.face_detector.backbone == 'mobilenet0.25' and hm.face_detector.engine.w is None
    hy = Hp()                                                   # YOLOv5n / YOLOv5l: the YoloDetector keeps its host code, its network is swapped
    from comfyui_keep_amd.engine import yoloface as YF

    class FakeYolo:
        def __init__(self, sd):
            self.detector = FakeModule(sd)
    hy.face_detector = FakeYolo(YF.synth_yolo_state_dict('YOLOv5n', seed=0))
    engine_facelib(hy)
    assert isinstance(hy.face_detector, FakeYolo) and isinstance(hy.face_detector.detector, YF.EngineYoloModel)
    assert hy.face_detector.detector.engine.name == 'YOLOv5n' and float(hy.face_detector.detector.stride.max()) == 32.0
    assert not hasattr(hy.face_detector, 'detect_batch')      # (this fake has no _preprocess / _postprocess: per-frame path)
    # the batched pre-pass of a YoloDetector: its own _preprocess / _postprocess around ONE network call, detect_faces' rows per frame
    import types
    cv = types.ModuleType('cv2')
    cv.COLOR_BGR2RGB = 4
    cv.cvtColor = lambda img, code: img[..., ::-1]
    monkeypatch.setitem(sys.modules, 'cv2', cv)
    calls = []

    class FakeYolo2(FakeYolo):
        def _preprocess(self, images):
            calls.append(('pre', len(images), images[0][0, 0].tolist()))
            return torch.zeros(len(images), 3, 32, 32)

        def _postprocess(self, x, origimgs, pred, conf, iou):
            calls.append(('post', conf, iou, tuple(pred.shape)))
            return [[[1, 2, 30, 40]], [], [[5, 6, 7, 80], [9, 9, 20, 30]]], [[[[1, 1]] * 5], [], [[[2, 3]] * 5, [[4, 5]] * 5]]
    hy2 = Hp()
    hy2.face_detector = FakeYolo2(YF.synth_yolo_state_dict('YOLOv5n', seed=0))
    engine_facelib(hy2)
    hy2.face_detector.detector = lambda x: (torch.ones(x.shape[0], 7, 16), None)      # (no GPU here: the network itself is test_gpu_facelib's)
    frames = np.zeros((3, 8, 8, 3), np.uint8)
    frames[..., 0] = 9
    res = hy2.face_detector.detect_batch(frames, 0.97)
    assert calls == [('pre', 3, [0, 0, 9]), ('post', 0.97, 0.5, (3, 7, 16))]
    assert res[1] is None and res[0].shape == (1, 15) and res[2].shape == (2, 15)
    assert res[2][1].tolist() == [9, 9, 20, 30, 9, 4, 5, 4, 5, 4, 5, 4, 5, 4, 5]
    assert set(YF.synth_yolo_state_dict('YOLOv5l', seed=0)) == set(YF.yolo_state_dict_spec('YOLOv5l')) and YF.config_of(YF.yolo_state_dict_spec('YOLOv5l')) == 'YOLOv5l'
    with pytest.raises(RuntimeError):                           # a resnet50 trunk under the mobile name: loud
        RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0), backbone='mobile0.25')
    monkeypatch.setenv('KEEP_AMD_ENGINE_FACELIB', '0')
    h3 = Hp()
    h3.face_parse = FakeModule(PN.synth_parsenet_state_dict(seed=0, in_size=128, out_size=128))
    engine_facelib(h3)
    assert isinstance(h3.face_parse, FakeModule)


# ------------------------------------------------------------------------------------------------ footprint harness and tables
def _footprint_toy(kind):
    """Deliberately wrong torch "kernels" on the views the harness hands out: one writes one element past its payload, one lets
    a neighbour of its input reach the result through a multiplication by zero, one leaves an output element unwritten."""
    import footprint as FP
    n = 37
    x = torch.arange(n, dtype=torch.float32).reshape(1, n) + 1
    regions = [FP.single('x', x), FP.output('o', (1, n))]

    def reach(t, extra):      # the view widened by `extra` elements behind its end, as far as the allocation goes (none in a plain call)
        room = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset() - t.numel()
        return t.as_strided((t.numel() + min(extra, room),), (1,), t.storage_offset())

    def launch(t):
        if kind == 'ok':
            t['o'].copy_(t['x'] * 2)
        elif kind == 'write':
            wide = reach(t['o'], 1)
            wide[:n] = t['x'].reshape(-1) * 2
            wide[n:] = 1.0
        elif kind == 'read':
            t['o'].copy_(reach(t['x'], 2).sum() * 0 + t['x'] * 2)
        elif kind == 'unwritten':
            t['o'][:, :n - 1] = t['x'][:, :n - 1]
    return FP, regions, launch


def test_footprint_harness_bites():
    """tests/footprint.py on the CPU: a correct toy kernel passes; a write one element past the payload raises WriteOutside (and says
    where); `sum over a view reaching into the guard * 0 + x` raises ReadOutside (0 * NaN and 0 * Inf are NaN); an output element
    left unwritten is reported as non-finite."""
    FP, regions, launch = _footprint_toy('ok')
    out = FP.run(launch, regions, 'cpu')
    assert torch.equal(out['o'], (torch.arange(37, dtype=torch.float32).reshape(1, 37) + 1) * 2)
    FP, regions, launch = _footprint_toy('write')
    with pytest.raises(FP.WriteOutside, match=r'element \+37 relative to the payload start'):
        FP.run(launch, regions, 'cpu')
    FP, regions, launch = _footprint_toy('read')
    with pytest.raises(FP.ReadOutside, match='depends on memory outside'):
        FP.run(launch, regions, 'cpu')
    FP, regions, launch = _footprint_toy('unwritten')
    with pytest.raises(FP.ReadOutside, match='unwritten'):
        FP.run(launch, regions, 'cpu')


def test_footprint_harness_strided_gaps_and_shared_windows():
    """Gap columns of a strided payload are surroundings: a kernel that reads a whole padded row, or writes one column behind its
    slice, is caught; windows of one packed buffer are not each other's surroundings."""
    import footprint as FP
    a, b = torch.ones(5, 3), torch.full((5, 2), 2.0)

    def regions():
        return [FP.Region(5, 8, {'a': (1, 3, a), 'b': (4, 2, b)}, torch.float32, 'r'), FP.output('o', (5, 3), ld=6, off=2)]

    FP.run(lambda t: t['o'].copy_(t['a'] + t['b'].sum(1, keepdim=True)), regions(), 'cpu')      # reads both windows: fine

    def row_of(t, width):      # the rows of the window widened to `width` columns
        return t.as_strided((t.shape[0], width), (t.stride(0), 1), t.storage_offset())

    def wide_read(t):
        t['o'].copy_(row_of(t['a'], 6)[:, 5:6] * 0 + t['a'] * 3)            # column 6 of the packed rows: a gap
    with pytest.raises(FP.ReadOutside):
        FP.run(wide_read, regions(), 'cpu')

    def wide_write(t):
        t['o'].copy_(t['a'] * 3)
        row_of(t['o'], 4)[:, 3] = 0.0                                        # one column behind the slice
    with pytest.raises(FP.WriteOutside, match=r'element \+3 relative'):
        FP.run(wide_write, regions(), 'cpu')


def _family(s):
    """Kernel family of a plan string or of its format string: template arguments (numbers, booleans, %d / %s) dropped."""
    def args(m):
        rest = re.sub(r'%[ds]|\b\d+\b|\btrue\b|\bfalse\b|[,\s]', '', m.group(1))
        return f'<{rest}>' if rest else ''
    return re.sub(r'<([^>]*)>', args, s).strip()


# families of csrc/keep_conv_common.h:plan_kernel_name that no argument struct can reach (must stay empty unless a family truly is unreachable)
UNREACHABLE_CONV_FAMILIES = set()


def test_footprint_conv_table_reaches_every_kernel_family():
    """tests/test_gpu_footprint.py's convolution table against keep_conv2d_plan (host C): every case lands on the kernel it names,
    and the families reached are exactly the family strings plan_kernel_name can print -- a new family fails here until it has a case."""
    import test_gpu_footprint as T
    src = open(os.path.join(ROOT, 'comfyui-keep_amd', 'csrc', 'keep_conv_common.h')).read()
    declared = {_family(f) for f in re.findall(r'snprintf\(pl\.kernel, sizeof\(pl\.kernel\), "([^"]+)"', src)}
    assert len(declared) >= 14, declared
    reached, variants, auto_split = set(), set(), []
    for name, (expect, _, kw) in T.CONV_CASES.items():
        _, g, plan = T.conv_case_plan(name)
        got = plan.kernel.decode()
        assert got == expect, (name, got, expect)
        assert (plan.split_k > 1) == (plan.workspace_bytes > 0)
        if g.split_k > 1:
            assert plan.split_k == g.split_k, (name, plan.split_k)
        elif plan.split_k > 1:
            auto_split.append(name)
        if g.stats:
            assert plan.stats_P > 0, name
        if g.amax:
            assert plan.out_amax_ok, name
        reached.add(_family(got))
        variants.add(got)
    assert reached == declared - UNREACHABLE_CONV_FAMILIES, (sorted(declared - reached), sorted(reached - declared))
    for v in ('conv3x3_halo_x3_kernel<16>', 'conv3x3_halo_x3_kernel<32>', 'conv3x3_halo_f32_kernel<16>', 'conv3x3_halo_f32_kernel<32>',
              'gemm_x3l_kernel<4>', 'gemm_x3l_kernel<8>', 'conv_f32_kernel<4, 1, 1, 1>', 'conv_f32_kernel<2, 2, 1, 1>',
              'conv_f32_kernel<2, 2, 2, 2>', 'conv3x3_halo3_kernel<false, 32>', 'conv3x3_halo3_kernel<true, 16>',
              'conv_x3_kernel<2, 2, 1, 1, true, true>', 'conv_x3_kernel<2, 2, 2, 2, true, false>', 'conv_x3_kernel<2, 2, 1, 1, false, false>',
              'conv_bf16_kernel<2, 2, 1, 1, 256, 1, false>', 'conv_bf16_kernel<4, 1, 1, 1, 64, 1, false>',
              'conv_bf16_kernel<2, 2, 2, 2, 64, 1, true>'):
        assert v in variants, v
    assert auto_split, 'no case where the library itself chooses split-K'


# ------------------------------------------------------------------------------------------------ keep_conv2d: the table is complete
# launched instantiations that no table case reaches (must stay empty; only what no argument struct reaches may ever be listed, with the
# condition quoted)
UNREACHABLE_CONV_KERNELS = set()
# instantiations the launch macros COMPILE that no argument struct can reach, each with the condition that keeps it away
COMPILED_BUT_UNREACHABLE = {
    # keep_conv.hip plan_bf16: `if (p.in_bf16 && !g.no_pro) { pl.path = PATH_NEEDS_PRENORM; ...` comes before PATH_HALO_BF16_V1, whose only
    # reason is a prologue (`pl.path = g.no_pro ? PATH_HALO_BF16 : PATH_HALO_BF16_V1`): the first halo kernel never sees a bf16 input
    'conv3x3_halo_kernel<true, 16>', 'conv3x3_halo_kernel<true, 32>',
    # keep_gemm_x3l.hip keep_gemm_x3l_ok: `!a->pro_scale && a->pro_act == KEEP_PRO_NONE` -- FORM_GEMM_LAT is planned with plain == true only,
    # so neither the latency kernel nor the K-slice arm of KEEP_LAUNCH_GX (`p.kslice_steps > 0` without `plain`) runs its prologue form
    'gemm_x3l_kernel<4, 1, false>', 'gemm_x3l_kernel<8, 1, false>',
    'conv_x3_kernel<2, 2, 1, 1, false, true, true, true, false, false>', 'conv_x3_kernel<2, 2, 2, 2, false, true, true, true, false, false>',
    # keep_gemm_x3l.hip keep_conv2d_x3_gemm_lat: `tiles.tile = 1;` -- p.kslice_steps is set on the 64 x 64 tile alone, and KEEP_LAUNCH_GX's
    # `p.kslice_steps == 4 && plain && C * D == 1` arm is instantiated for C * D == 4 too (there it is the plain K-slice form again)
    'conv_x3_kernel<2, 2, 2, 2, true, true, true, true, false, false>',
    # keep_conv_x3.hip KEEP_LAUNCH_GX: `plain && C * D == 1 && M > 262144` is false at run time on the 128 x 128 tile, whose macro expansion
    # still instantiates the shallow pipeline
    'conv_x3_kernel<2, 2, 2, 2, true, false, false, false, false, false>',
}
# KEEP_CONV_LAUNCH sites per source: a new arm of a launch macro changes a count and must come with its cases
CONV_LAUNCH_SITES = {'keep_conv.hip': 25, 'keep_conv_x3.hip': 20, 'keep_conv_x3s.hip': 5, 'keep_conv_x3p.hip': 9, 'keep_gemm_x3l.hip': 2}
CONV_FAMILIES = {      # convolution instantiations per kernel template that a launch can take
    'conv3x3_c3_kernel': 1, 'conv3x3_c3_x3_kernel': 1, 'conv3x3_cout4_kernel': 1, 'conv3x3_halo3_kernel': 8, 'conv3x3_halo_f32_kernel': 6,
    'conv3x3_halo_kernel': 2, 'conv3x3_halo_x3_kernel': 19, 'conv3x3_halo_x3s_act_kernel': 48, 'conv3x3_halo_x3s_kernel': 8, 'conv3x3_up2_x1s_kernel': 1,
    'conv3x3_up2_x3s_kernel': 1, 'conv3x3_x3p_kernel': 16, 'conv3x3_x3q_kernel': 15, 'conv_bf16_kernel': 6, 'conv_f32_kernel': 5, 'conv_x3_kernel': 16,
    'gemm_x3l_kernel': 2,
}


def test_conv_table_reaches_every_instantiation():
    """tests/test_gpu_footprint.py's convolution table against keep_conv2d_launch_plan (host C: keep_conv2d's own dispatch code with every
    launch replaced by the launched kernel's name), as the attention table is held against keep_attention_plan below.

    Universe (tests/conv_universe.py: universe): the distinct strings the library answers over every mma (KEEP_MMA_X1 with no, each and all
    of its opt-in bits) x input / output dtype x k {1, 3, 7} x stride {1, 2} x every pro_act with and without pro_scale x the seven epi_act x
    {no residual, residual, residual + aux} x in2 x LayerNorm x {zero, reflect} padding x upsample {0, 1, x2 phases} x requested split_k
    {0 .. 4} x statistics x amax slots {none, zeroed, stale} x N {1, 3, 48} x maps {8x32, 16x16, 16x64, 64x64, 5x7, 64x128, 128x128,
    1026x1026 (stride 2: more than 262144 rows)} x Cin {3 .. 2048} x Cout {3 .. 128} x {aligned, out_ld off, pointers off} x {no flag, each
    KEEP_CONV_* selection flag} x bk256, as the union of full products over the axes one launcher reads together; refused points are
    skipped.  A launched string is `[zero_u32_kernel + ] convolution [+ split-K reducer | + statistics replica]`; the universe of
    CONVOLUTION instantiations is pinned at 156 (per template: CONV_FAMILIES).
    Census (conv_universe.census): the kernel handles in the built library's symbol table, restricted to the __global__ names of the five
    convolution sources -- an answer that does not go through keep_conv2d_launch_plan.  universe - census is empty; census - universe is
    COMPILED_BUT_UNREACHABLE, 8 instantiations, each with the condition that keeps every argument struct away from it.
    Reach: the launched strings of CONV_CASES, each asked for the very arguments the GPU tests launch, equal the expectation the table
    carries, and their convolutions are exactly the universe -- UNREACHABLE_CONV_KERNELS is empty -- and so are the follow-up kernels and
    the zero-fill.  Every family keeps the table's awkwardness where its kernels admit it: a strided input slice, a strided output,
    res_ld != Cout, N = 3 with per-image maxima, statistics."""
    import abi_ref as A
    import conv_universe as U
    import test_gpu_footprint as T
    found, points, refused = U.universe()
    assert points > 500000 and refused > 0, (points, refused)
    universe = {U.convolution(s) for s in found}
    by_template = {}
    for k in universe:
        by_template[k.split('<')[0]] = by_template.get(k.split('<')[0], 0) + 1
    assert by_template == CONV_FAMILIES and len(universe) == 156, by_template
    pieces = {p for s in found for p in s.split(' + ')}
    assert pieces - universe == set(U.FOLLOW_UPS) | {'zero_u32_kernel'}, sorted(pieces - universe)
    for s in found:      # the zero-fill comes first, at most one follow-up kernel comes last
        parts = s.split(' + ')
        assert 'zero_u32_kernel' not in parts[1:] and sum(p in U.FOLLOW_UPS for p in parts) <= 1 and not set(parts[:-1]) & set(U.FOLLOW_UPS), s

    census = U.census()
    assert U.launch_sites() == CONV_LAUNCH_SITES, U.launch_sites()
    assert len(census) == 169, len(census)
    assert pieces <= census, sorted(pieces - census)
    assert census - pieces == COMPILED_BUT_UNREACHABLE and len(COMPILED_BUT_UNREACHABLE) == 8, (sorted(census - pieces - COMPILED_BUT_UNREACHABLE),
                                                                                                sorted(COMPILED_BUT_UNREACHABLE - census))

    rows = []                                   # (name, geometry, launched string) of every launched table case
    for name, (_, expect, kw) in T.CONV_CASES.items():
        if kw.get('launch', True):
            got = T.conv_case_launched(name)
            assert got == expect, (name, got, expect)
            assert set(got.split(' + ')) <= pieces, (name, got)
            rows.append((name, T._Geom(kw), got))
    reached = {A.conv_kernel(s) for _, _, s in rows}
    assert reached == universe - UNREACHABLE_CONV_KERNELS, (sorted(universe - reached), sorted(reached - universe))
    assert not UNREACHABLE_CONV_KERNELS
    assert {p for _, _, s in rows for p in s.split(' + ')} == pieces
    by_family = {}
    for name, g, s in rows:
        by_family.setdefault(A.conv_kernel(s).split('<')[0], []).append(g)
    has = lambda fam, pred: any(pred(g) for g in by_family[fam])  # noqa: E731
    strided_in = lambda g: g.in_ld != g.cin1 and g.in_off  # noqa: E731
    strided_out = lambda g: g.out_ld != g.Cout and g.out_off  # noqa: E731
    res_ld = lambda g: g.res_ld and g.res_ld != g.Cout  # noqa: E731
    n3_amax = lambda g: g.N == 3 and g.amax  # noqa: E731
    everything = ('conv3x3_halo_x3s_kernel', 'conv3x3_halo_x3s_act_kernel', 'conv3x3_halo_x3_kernel', 'conv3x3_x3q_kernel', 'conv_x3_kernel')
    for fam in everything:
        for what, pred in (('strided input', strided_in), ('strided output', strided_out), ('res_ld', res_ld), ('N = 3 with amax', n3_amax),
                           ('statistics', lambda g: g.stats)):
            assert has(fam, pred), (fam, what)
    for fam in ('conv3x3_x3p_kernel', 'conv3x3_halo_f32_kernel', 'conv3x3_halo3_kernel', 'gemm_x3l_kernel'):      # (no amax / statistics on a split or bf16 launch)
        for what, pred in (('strided input', strided_in), ('strided output', strided_out), ('res_ld', res_ld), ('N = 3', lambda g: g.N == 3)):
            assert has(fam, pred), (fam, what)


def test_conv_launch_plan_query_is_host_c_and_follows_the_launch():
    """keep_conv2d_launch_plan (include/keep_cv_hip.h): header, binding and library agree on the struct; a refusal is the launch's own, code
    and text, and zeroes the answer; keep_conv2d_plan's family string stays what it was where the launch takes another instantiation."""
    import test_gpu_footprint as T
    from comfyui_keep_amd.engine import hiplib as L
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    assert [n for n, _ in L.ConvLaunchPlanOut._fields_] == _header_struct_fields(header, 'keep_conv2d_launch_plan_out')
    assert ctypes.sizeof(L.ConvLaunchPlanOut) == 4 + 508
    lib = L.load(check_device=False)
    _, g, plan = T.conv_case_plan('x3q_small')
    assert plan.kernel == b'conv3x3_halo_x3s_kernel' and T.conv_case_launched('x3q_small') == 'conv3x3_x3q_kernel<0, false, 0> + conv_stats_replica_kernel'
    out = L.ConvLaunchPlanOut()
    t = T._fake_tensors(g)

    def refused(code, text, **over):
        a = T._conv_args(g, {**t, **{k: v for k, v in over.items() if k in ('x', 'ws', 'stats', 'amax')}})
        for k, v in over.items():
            if k not in ('x', 'ws', 'stats', 'amax'):
                setattr(a, k, v)
        out.n_kernels = 7
        assert lib.keep_conv2d_launch_plan(ctypes.byref(a), ctypes.byref(out)) == code, over
        assert text in lib.keep_last_error() and lib.keep_last_error().startswith(b'keep_conv2d'), lib.keep_last_error()
        assert out.n_kernels == 0 and out.kernels == b''
    refused(L.EINVAL, b'struct_size', struct_size=8)
    refused(L.EINVAL, b'null tensor pointer', x=None)
    refused(L.EINVAL, b'split_k>1 requires a workspace', split_k=2)
    refused(L.EINVAL, b'stats_P=', stats=0x10000, stats_P=5)
    refused(L.EINVAL, b'bad mma', mma=9)
    assert lib.keep_conv2d_launch_plan(None, ctypes.byref(out)) == L.EINVAL and lib.keep_conv2d_launch_plan(ctypes.byref(T._conv_args(g, t)), None) == L.EINVAL
    with pytest.raises(L.KeepHipError, match='bad mma') as e:
        a = T._conv_args(g, t)
        a.mma = 9
        L.conv2d_launch_plan(a)
    assert e.value.code == L.EINVAL


# ------------------------------------------------------------------------------------------------ keep_attention: the table is complete
# instantiations keep_attention_plan can name that no table case can reach (must stay empty unless one truly is unreachable)
UNREACHABLE_ATTN_KERNELS = set()
# the forms of the requirements below, by the kernel string keep_attention_plan prints
ATTN_FORMS = {
    'f32 4-wave': r'attn_f32_kernel<4, \d>', 'bf16 4-wave': r'attn_bf16_kernel<4, \d>', 'bf16 1-wave': r'attn_bf16_kernel<1, \d>',
    'bf16in': r'attn_bf16in_kernel<\d, (true|false)>', 'NQ8 4-wave': r'attn_x3_kernel<4, \d, 8, false, false>',
    'NQ8 1-wave': r'attn_x3_kernel<1, \d, 8, false, false>', 'NQ16': r'attn_x3_kernel<4, \d, 16, false, false>',
    'NQ0': r'attn_x3_kernel<4, \d, 0, false, false>', 'packed': r'attn_pack_kv_x3_kernel<\d+, \d+, false> \+ attn_x3_kernel<4, \d, \d+, true, false>',
    'sfull': r'attn_x3_sfull_kernel<\d>', 'sfull2': r'attn_x3_sfull2_kernel', 'small': r'attn_x3_small_kernel',
}


def _attn_form(kernel):
    hit = [f for f, pat in ATTN_FORMS.items() if re.fullmatch(pat, kernel)]
    return hit[0] if hit else None


def _attention_universe():
    """Every (kernel string, lds_bytes) keep_attention_plan answers over the grid of the docstring below; checks scratch_bytes against
    keep_attention_workspace_bytes at every admitted point on the way."""
    from comfyui_keep_amd.engine import hiplib as L
    lib = L.load(check_device=False)
    a, out = L.AttnArgs(), L.AttnPlanOut()
    a.struct_size = ctypes.sizeof(L.AttnArgs)
    a.q = a.k = a.v = a.o = 0x10000
    a.H, a.scale = 1, 1.0
    pa, po = ctypes.byref(a), ctypes.byref(out)
    no_bits = (0, L.ATTN_NO_PACK, L.ATTN_NO_SFULL2, L.ATTN_NO_X3, L.ATTN_NO_SMALL, L.ATTN_NO_TWO_PASS)
    found, points = {}, 0
    for mma, x1 in ((L.MMA_F32, 0), (L.MMA_BF16, 0), (L.MMA_X3, 0), (L.MMA_X1, L.ATTN_X1)):
        for in_dtype in (L.F32, L.BF16):
            for mode in (0, 1, 2):
                # mode 2: Lq == Lk == the window, so both length axes give windows (2 rows of L / 2 tokens, unshifted and shifted)
                lengths = [(Lq, Lk, sh) for Lq in (20, 24, 200, 256, 300) for Lk in (200, 256, 300, 4224) for sh in (0,)] if mode != 2 else \
                          [(L_, L_, sh) for L_ in (20, 24, 200, 256, 300, 4224) for sh in (0, 1)]
                for Lq, Lk, shift in lengths:
                    a.mma, a.in_dtype, a.mode, a.Lq, a.Lk, a.shift = mma, in_dtype, mode, Lq, Lk, shift
                    a.B = a.T = 2 if mode == 1 else 1
                    a.seg_len = Lk // 2
                    a.img_h, a.img_w, a.ksplit, a.n_img = 2, Lk // 2, 1, 1
                    for D in (32, 48, 64, 128, 256, 384, 512):
                        for Dv in (2, 8, 32, 64, 128, 256, 384, 512):
                            a.D, a.Dv = D, Dv
                            a.q_ts = a.k_ts = a.q_hs = a.k_hs = D
                            a.v_ts = a.o_ts = a.v_hs = a.o_hs = Dv
                            a.q_bs, a.k_bs, a.v_bs, a.o_bs = Lq * D, Lk * D, Lk * Dv, Lq * Dv
                            for flags in no_bits:
                                a.flags = flags | x1
                                for amax in (0, 0x10000):
                                    a.q_amax = a.k_amax = a.v_amax = amax
                                    a.workspace, a.workspace_bytes = None, 0
                                    need = lib.keep_attention_workspace_bytes(pa)
                                    for ws in (False, True):
                                        if ws:
                                            if need <= 0:
                                                break                   # nothing to bring: the same point again
                                            a.workspace, a.workspace_bytes = 0x10000, need
                                        if lib.keep_attention_plan(pa, po) != 0:
                                            continue                    # a refused combination
                                        points += 1
                                        assert out.scratch_bytes == need, (out.kernel, out.scratch_bytes, need)
                                        kernel = out.kernel.decode()
                                        found[kernel] = max(found.get(kernel, 0), out.lds_bytes)
    return found, points


def test_attention_table_reaches_every_instantiation():
    """tests/test_gpu_footprint.py's attention table against keep_attention_plan (host C), as the convolution table is held against
    keep_conv2d_plan above.

    Universe: the distinct `kernel` strings the library answers over mma {F32, BF16, X3, X1 | ATTN_X1} x in_dtype {F32, BF16} x mode {0, 1, 2}
    x D {32 .. 512} x Dv {2 .. 512} x Lq {20, 24, 200, 256, 300} x Lk {200, 256, 300, 4224} (mode 2: windows of each of these lengths,
    unshifted and shifted) x workspace {absent, the size the library asks for} x {no flag, each ATTN_NO_* bit} x range probes {off, on};
    refused combinations are skipped.  Its size is pinned to the count of the `switch` in keep_attention (csrc/keep_attn.hip):
        attn_f32_kernel<1|4, 1|2|4> 6 + attn_bf16_kernel<1|4, 1|2|4> 6 + attn_bf16in_kernel<1|2|4, false|true> 6
        + attn_x3_kernel<1|4, 1|2|4, 8> 6 + <4, 1|2|4, 16> 3 + <4, 1|2|4, 0> 3 + packed <4, 1|2|4, 8|16, true> 6 + its single-fp16 twin 1
        + attn_x3_small_kernel 1 + the two-pass pair 1 + attn_x3_sfull_kernel<1|2|4> 3 + attn_x3_sfull2_kernel 1 = 43.
    Reach: the strings of ATTN_CASES (each planned from its own arguments with the workspace it really passes) and of the single-fp16
    cases of tests/test_gpu_attn_x1.py are exactly the universe.  Then, per flash form: modes 0, 1 and 2-with-shift; mode 2 with and
    without the LDS window tables, the tables once on a plain four-wave launch and once on the packed form, and a four-wave launch of a
    form that has tables running WITHOUT them (windows of more than 4096 tokens); range probes on every x3 form that takes them;
    key AND query counts that are no multiples of 32 on the forms that had none.  Every universe member fits the CU's 160 KiB of LDS and
    scratch_bytes equals keep_attention_workspace_bytes at every point of the sweep."""
    import test_gpu_attn_x1 as TX
    import test_gpu_footprint as T
    from comfyui_keep_amd.engine import hiplib as L
    universe, points = _attention_universe()
    assert points > 50000, points
    assert len(universe) == 43, sorted(universe)
    for kernel, lds in universe.items():
        assert 0 <= lds <= 160 * 1024, (kernel, lds)
        assert kernel.count(' + ') == (1 if kernel.startswith(('attn_pack_kv_x3_kernel', 'attn_scores_x3l_kernel')) else 0), kernel

    rows = []                                   # (case, kernel, plan) of every table case
    for c in T.ATTN_CASES:
        plan = T.attn_case_plan(c)
        rows.append((c, plan.kernel.decode(), plan))
        assert (plan.scratch_bytes > 0) == (plan.kernel.count(b' + ') == 1) or not c['ws'] or c['flags'] & L.ATTN_NO_PACK, c['name']
    reached = {k for _, k, _ in rows}
    for name, make in TX.CASES.items():         # the single-fp16 cases, as test_gpu_attn_x1.call builds them
        kw = make()['kw']
        a = L.attn_args(q=0x10000, k=0x10000, v=0x10000, o=0x10000, in_dtype=L.F32, **dict(kw, **TX.X1))
        a.workspace, a.workspace_bytes = 0x10000, L.attention_workspace_bytes(a)
        assert a.workspace_bytes == TX.x1_bytes(kw['B'], kw['Lk'])
        reached.add(L.attention_plan(a).kernel.decode())
    assert reached == set(universe) - UNREACHABLE_ATTN_KERNELS, (sorted(set(universe) - reached), sorted(reached - set(universe)))
    assert not UNREACHABLE_ATTN_KERNELS

    by_form = {}
    for c, kernel, plan in rows:
        by_form.setdefault(_attn_form(kernel), []).append((c, plan))
    assert set(ATTN_FORMS) <= set(by_form), sorted(set(ATTN_FORMS) - set(by_form))
    has = lambda form, pred: any(pred(c, plan) for c, plan in by_form[form])  # noqa: E731
    for form in ('f32 4-wave', 'bf16 4-wave', 'bf16in', 'NQ8 4-wave', 'NQ16', 'NQ0', 'packed'):
        for mode in (0, 1):
            assert has(form, lambda c, _: c['mode'] == mode), (form, mode)
        assert has(form, lambda c, _: c['mode'] == 2 and c['shift'] > 0), (form, 'mode 2 with shift')
    mode2 = [(c, kernel, plan) for c, kernel, plan in rows if c['mode'] == 2]
    assert {plan.win_tables for _, _, plan in mode2} == {0, 1}
    assert any(plan.win_tables and _attn_form(k) in ('NQ8 4-wave', 'NQ16') for _, k, plan in mode2)
    assert any(plan.win_tables and _attn_form(k) == 'packed' for _, k, plan in mode2)
    assert any(not plan.win_tables and plan.waves == 4 and c['Lk'] > 4096 and c['shift'] > 0 and _attn_form(k) == 'NQ8 4-wave' for c, k, plan in mode2)
    assert all(plan.masked == (c['mode'] == 2 and c['shift'] > 0) for c, plan in by_form['bf16in'])
    for form in ('NQ8 1-wave', 'NQ16', 'NQ0', 'packed', 'sfull', 'sfull2', 'small'):
        assert has(form, lambda c, _: c['amax']), (form, 'range probes')
    for form in ('sfull', 'sfull2', 'small', 'NQ16', 'NQ0', 'packed', 'bf16 4-wave', 'bf16 1-wave', 'bf16in'):
        assert has(form, lambda c, _: c['Lk'] % 32 and c['Lq'] % 32), (form, 'ragged key and query counts')
    # the slices and edges the table lacked: several dv slices per head, the chunked D > 128 staging of the f32 / bf16 kernels, the small
    # form at its lower edge (Lq = 64, one key past a tile)
    for form in ('f32 4-wave', 'bf16 4-wave'):
        assert has(form, lambda c, _: c['D'] > 128), (form, 'D > 128')
    for form in ('NQ16', 'NQ0', 'packed', 'sfull'):
        assert has(form, lambda c, plan: plan.nslices > 1), (form, 'dv slices')
    assert has('small', lambda c, _: c['Lq'] == 64 and c['Lk'] == 33)


def test_attention_plan_query_is_host_c_and_follows_the_launch():
    """keep_attention_plan (include/keep_cv_hip.h): header, binding and library agree on the struct; a refusal is the launch's own, code and
    text; scratch counts exactly as in the launch (given, 16-byte aligned, large enough), and `scratch_bytes` is the workspace query's answer
    either way."""
    from comfyui_keep_amd.engine import hiplib as L
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    assert [n for n, _ in L.AttnPlanOut._fields_] == _header_struct_fields(header, 'keep_attention_plan_out')
    assert ctypes.sizeof(L.AttnPlanOut) == 5 * 4 + 4 + 2 * 8 + 96
    lib = L.load(check_device=False)

    def args(**kw):
        base = dict(q=0x10000, k=0x10000, v=0x10000, o=0x10000, B=1, H=1, Lq=300, Lk=77, D=128, Dv=128, scale=1.0, mma=L.MMA_X3, q_bs=300 * 128, q_ts=128,
                    q_hs=128, k_bs=77 * 128, k_ts=128, k_hs=128, v_bs=77 * 128, v_ts=128, v_hs=128, o_bs=300 * 128, o_ts=128, o_hs=128)
        return L.attn_args(**dict(base, **kw))
    flash, packed = 'attn_x3_kernel<4, 4, 8, false, false>', 'attn_pack_kv_x3_kernel<128, 128, false> + attn_x3_kernel<4, 4, 8, true, false>'
    need = L.attention_workspace_bytes(args())
    assert need > 0
    for ws, nbytes, want in ((None, 0, flash), (0x10000, need, packed), (0x10000, need - 16, flash), (0x10008, need, flash)):
        plan = L.attention_plan(args(workspace=ws, workspace_bytes=nbytes))
        assert (plan.kernel.decode(), plan.scratch_bytes, plan.waves, plan.dvt, plan.nslices) == (want, need, 4, 4, 1), (ws, nbytes, plan.kernel)
    out = L.AttnPlanOut()
    out.waves = 7
    for kw, code, text in ((dict(D=130), L.EINVAL, b'D=130 must be even'), (dict(mode=3), L.EINVAL, b'bad mode'),
                           (dict(mma=L.MMA_X1, flags=L.ATTN_X1), L.EUNSUP, b'KEEP_MMA_X1 needs a 16-byte aligned workspace'),
                           (dict(struct_size=8), L.EINVAL, b'struct_size')):
        assert lib.keep_attention_plan(ctypes.byref(args(**kw)), ctypes.byref(out)) == code, kw
        assert text in lib.keep_last_error() and lib.keep_last_error().startswith(b'keep_attention'), lib.keep_last_error()
        assert out.waves == 0 and out.kernel == b''
    assert lib.keep_attention_plan(None, ctypes.byref(out)) == L.EINVAL and lib.keep_attention_plan(ctypes.byref(args()), None) == L.EINVAL
    with pytest.raises(L.KeepHipError, match='bad mode') as e:
        L.attention_plan(args(mode=3))
    assert e.value.code == L.EINVAL


def test_footprint_tables_name_every_launcher():
    """Every keep_* entry point include/keep_hip.h declares is either host-only or has footprint cases (>= 2 each for the flat ops)."""
    import test_gpu_footprint as T
    header = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    declared = set(re.findall(r'\b(keep_[a-z0-9_]+)\s*\(', header))
    covered = set(T.FLAT_CASES) | set(T.STRUCT_LAUNCHERS)
    assert T.HOST_ONLY <= declared
    assert covered | T.HOST_ONLY == declared, (sorted(declared - covered - T.HOST_ONLY), sorted(covered - declared))
    assert not (covered & T.HOST_ONLY)
    for fn, cases in T.FLAT_CASES.items():
        assert len(cases) >= 2 and len({cid for cid, _, _ in cases}) == len(cases), fn


# ------------------------------------------------------------------------------------------------ the case-value judge (tests/abi_ref.py)
def _payloads(regions):
    return {n: d for r in regions for n, (_, _, d) in r.windows.items() if d is not None}


def _conv_case_refs():
    """(name, kernel, geometry, plan, payloads, reference) of every launched convolution case of the footprint table."""
    import abi_ref as A
    import test_gpu_footprint as T
    for name, (_, _, kw) in T.CONV_CASES.items():
        if kw.get('launch', True):
            g, plan, regions, _ = T._conv_regions(name)
            t = _payloads(regions)
            yield name, plan.kernel.decode(), g, plan, t, A.conv2d_ref(g, t)


_ATTN_REFS = {}        # (case name, removal or None) -> float64 reference: computed once, shared by the tests below, never modified


def _attn_ref(c, t, remove=None):
    import abi_ref as A
    key = (c['name'], remove)
    if key not in _ATTN_REFS:
        _ATTN_REFS[key] = A.attention_ref(c, t['q'], t['k'], t['v'], remove=remove)
    return _ATTN_REFS[key]


def _attn_case_refs():
    import test_gpu_footprint as T
    for c in T.ATTN_CASES:
        t = _payloads(T.attn_case_launch(c)[0])
        yield c, t, _attn_ref(c, t)


def test_abi_ref_restates_the_bindings_constants():
    import abi_ref as A
    from comfyui_keep_amd.engine import hiplib as L
    for n in ('MMA_F32', 'MMA_BF16', 'MMA_X3', 'PRO_NONE', 'PRO_SWISH', 'PRO_RELU', 'ACT_NONE', 'ACT_RELU', 'ACT_LRELU02', 'ACT_GELU',
              'ACT_SIGMOID', 'ACT_LRELU01', 'ACT_SILU', 'ATTN_NO_X3'):
        assert getattr(A, n) == getattr(L, n), n


CONV_CLASS_COUNTS = {'f32': 22, 'x3': 111, 'x1': 35, 'bf16': 22, 'plan-only': 1}      # table cases per tolerance class


def test_case_value_references_refuse_unknown_keys_and_classify_every_case():
    """conv2d_ref / attention_ref raise on a key they do not know (a key added to the table later cannot be silently ignored); every
    table case maps to exactly one tolerance class through the kernel name its plan reports, a family nobody classified raises, and
    the exact-f32 twin of every x3 case plans onto an exact-f32 kernel."""
    import abi_ref as A
    import test_gpu_footprint as T
    g, _, regions, _ = T._conv_regions('halo_f32_32')
    with pytest.raises(KeyError, match='dilation'):
        A.conv2d_ref(A.dict_view(g, dilation=2), _payloads(regions))
    c = T.ATTN_CASES[0]
    t = _payloads(T.attn_case_launch(c)[0])
    with pytest.raises(KeyError, match='causal'):
        A.attention_ref(dict(c, causal=True), t['q'], t['k'], t['v'])
    with pytest.raises(KeyError):
        A.conv_class('conv_fp8_kernel<2, 2>')
    classes = {}
    for name, (expect, _, kw) in T.CONV_CASES.items():
        _, g, plan = T.conv_case_plan(name)
        klass = A.conv_class(plan.kernel.decode())
        assert (klass == 'plan-only') == (not g.launch), name
        if g.launch:      # the class is the launched instantiation's; the family string of the plan says the same
            assert A.conv_class(T.CONV_CASES[name][1]) == klass == A.conv_class(T.conv_case_launched(name)), name
        classes.setdefault(klass, []).append(name)
        if klass == 'x3':
            _, _, twin = T.conv_case_plan(name, A.conv_twin_kw(kw))
            assert A.conv_class(twin.kernel.decode()) == 'f32', (name, twin.kernel.decode())
        elif klass == 'x1':
            assert g.mma == A.MMA_X1 and A.X1_TOL == 2.0 ** -10 + 2e-6, name
        elif klass != 'plan-only':
            assert A.conv_tol(klass, g) in (2e-4, 2e-5, 2e-3, 2e-5 + 2.0 ** -8), name
    assert {k_: len(v) for k_, v in classes.items()} == CONV_CLASS_COUNTS, {k_: len(v) for k_, v in classes.items()}
    for k_ in COMPILED_BUT_UNREACHABLE:      # (no instantiation the library holds is unclassified)
        assert A.conv_class(k_) in ('x3', 'bf16'), k_
    # 'f32_t2_x3_fallback' asks for x3 and runs on an f32 kernel: the class follows the kernel, not the request
    assert 'f32_t2_x3_fallback' in classes['f32'] and 'cout4_x3' in classes['f32']
    assert sorted({A.attn_class(c) for c in T.ATTN_CASES}) == ['bf16', 'f32', 'x3']


def test_case_value_references_feel_every_optional_input():
    """For every case and every optional input it switches on, the reference without that input differs from the full reference by
    at least 100 x the case's tolerance x scale: a kernel that ignores the input cannot pass tests/test_gpu_case_values.py.
    Convolutions: bias, pro_scale, pro_shift, the per-image rows of both, prologue / epilogue activation, residual, aux, reflect, in2,
    LayerNorm gamma / beta.  Attention: the mode-2 mask, roll and kv_rot, the mode-1 second key segment, the head stride."""
    import abi_ref as A
    seen = set()
    for name, kernel, g, plan, t, ref in _conv_case_refs():
        lim = A.conv_bound(A.conv_class(kernel), g, ref)      # (per element; uniform tolerance x scale in every class but x1)
        for what, g2, t2 in A.conv_removals(g, t):
            d = float(((A.conv2d_ref(g2, t2)['out'] - ref['out']).abs() / lim).max())
            assert d >= A.SENSITIVITY, (name, what, d)
            seen.add(what)
    assert seen == {'bias', 'pro_scale', 'pro_shift', 'per-image prologue rows', 'prologue activation', 'epilogue activation', 'residual', 'aux',
                    'reflect', 'in2', 'ln_gamma', 'ln_beta'}, seen
    seen = set()
    for c, t, ref in _attn_case_refs():
        tol, sc = A.attn_tol(A.attn_class(c)), max(1.0, float(ref.abs().max()))
        for what in A.attn_case_removals(c):
            d = float((_attn_ref(c, t, what) - ref).abs().max())
            assert d >= A.SENSITIVITY * tol * sc, (c['name'], what, d / sc, tol)
            seen.add(what)
    assert seen == set(A.ATTN_REMOVALS), seen


def test_case_value_judge_tells_neighbouring_instantiations_apart():
    """The risk of a dispatch of 156 instantiations is the NEIGHBOURING one: a wrong arm of a launch macro picks another EACT, another
    prologue form, the other padding.  For every launched case the float64 reference, computed as such a neighbour would compute it, misses
    the case's tolerance by at least abi_ref.SENSITIVITY: with any other epi_act of the seven; with any other pro_act, and with the affine
    dropped; with the activation applied after the residual instead of before it; with zero padding in place of reflection padding and
    the other way round.  A condition on the table's inputs (bias_amp, pro_amp, x_amp, w_amp, w_peak), checked before a GPU is touched."""
    import abi_ref as A
    seen, n = set(), 0
    for name, kernel, g, plan, t, ref in _conv_case_refs():
        lim = A.conv_bound(A.conv_class(kernel), g, ref)
        for what, out in A.conv_neighbours(g, t, ref):
            d = float(((out - ref['out']).abs() / lim).max())
            assert d >= A.SENSITIVITY, (name, what, d)
            seen.add(what.split()[0])
            n += 1
    assert seen == {'epi_act', 'pro_act', 'affine', 'activation', 'zero', 'reflection'} and n >= 1700, (seen, n)


def _fake_device_conv(g, P, out64, stats_from=None):
    """What a correct kernel would hand back for reference output ``out64``: `out` in the case's output dtype, P statistics partials per
    image (of ``stats_from`` if given: an output and statistics that disagree), and the amax arena."""
    out = out64.to(torch.bfloat16 if g.out_bf16 else torch.float32)
    got = {'out': out}
    if g.stats:
        s = (out64 if stats_from is None else stats_from).reshape(g.N, P, -1, g.Cout)
        got['stats'] = torch.stack([s.sum(2), (s * s).sum(2)], dim=-1).float().reshape(1, -1)
    if g.amax:
        got['amax'] = out.float().reshape(g.N, -1).abs().amax(1).reshape(1, g.N)
        got['amax_lo'], got['amax_hi'] = torch.zeros(1, 3), torch.zeros(1, 8 - g.N)
    return got


def test_case_value_judge_bites(capsys):
    """abi_ref.judge_conv / judge_attn on the CPU, for every table case: the reference itself (rounded to the output dtype) passes; the
    same with ONE element moved by 10 x tol x scale fails; the reference of the case with any one optional input dropped fails; for
    cases with fused outputs, statistics of another tensor than `out`, an amax slot one ulp off and a written neighbour slot fail."""
    import abi_ref as A
    n_bites = 0
    for name, kernel, g, plan, t, ref in _conv_case_refs():
        klass, P = A.conv_class(kernel), plan.stats_P
        sc = max(1.0, float(ref['out'].abs().max()))
        twin = ref['out'].float() if klass == 'x3' else None
        A.judge_conv(name, kernel, g, _fake_device_conv(g, P, ref['out']), ref, twin, P)
        moved = ref['out'].clone()
        moved.view(-1)[moved.numel() // 2] += 10 * float(A.conv_bound(klass, g, ref).view(-1)[moved.numel() // 2])
        wrong = [('one element', _fake_device_conv(g, P, moved))]
        removed = {what: A.conv2d_ref(g2, t2)['out'] for what, g2, t2 in A.conv_removals(g, t)}
        wrong += [(what, _fake_device_conv(g, P, o)) for what, o in removed.items()]
        if g.stats:
            wrong.append(('statistics of another tensor', _fake_device_conv(g, P, ref['out'], stats_from=removed['bias'])))
        if g.amax:
            ulp = _fake_device_conv(g, P, ref['out'])
            ulp['amax'] = torch.nextafter(ulp['amax'], torch.full_like(ulp['amax'], 1e30))
            nb = _fake_device_conv(g, P, ref['out'])
            nb['amax_hi'][0, 0] = 1.0
            wrong += [('amax one ulp off', ulp), ('neighbour slot written', nb)]
        for what, got in wrong:
            with pytest.raises(AssertionError):
                A.judge_conv(name, kernel, g, got, ref, twin, P)
                pytest.fail(f'{name}: the judge let "{what}" pass')
            n_bites += 1
    for c, t, ref in _attn_case_refs():
        klass = A.attn_class(c)
        twin = ref.float() if klass == 'x3' else None
        A.judge_attn(c, ref.float(), ref, twin)
        moved = ref.clone()
        moved.view(-1)[moved.numel() // 2] += 10 * A.attn_tol(klass) * max(1.0, float(ref.abs().max()))
        wrong = [('one element', moved)] + [(what, _attn_ref(c, t, what)) for what in A.attn_case_removals(c)]
        for what, got in wrong:
            with pytest.raises(AssertionError):
                A.judge_attn(c, got.float(), ref, twin)
                pytest.fail(f"{c['name']}: the judge let \"{what}\" pass")
            n_bites += 1
    assert n_bites >= 200, n_bites
    assert capsys.readouterr().out.count('[case-values]') >= n_bites


# ------------------------------------------------------------------------------------------------ the flat-op value judge (tests/flat_ref.py)
FLAT_CLASSES = {'exact', 'f32-arith', 'bf16', 'reduction', 'reduction+amax', 'f32-arith+amax', 'amax', 'index', 'dets', 'matrix'}


def _flat_case_refs():
    """(entry point, case id, parameters, payloads, regions, specs) of every flat case of the footprint table."""
    import flat_ref as R
    import test_gpu_footprint as T
    for fn, cases in T.FLAT_CASES.items():
        for cid, _, _ in cases:
            regions, _, _, params = T.flat_case(fn, cid)
            t = R.payloads(regions, fn, params)
            yield fn, cid, params, t, regions, R.reference(fn, params, t)


def test_flat_refs_cover_every_case_with_exactly_one_class():
    """Every (entry point, case) of FLAT_CASES has a reference in tests/flat_ref.py that judges every output the case declares (regions
    that are written and compared) and falls into exactly one class; an entry point without a reference and a parameter the reference
    does not know both raise, so a case added later cannot slip past the judge."""
    import flat_ref as R
    import test_gpu_footprint as T
    from comfyui_keep_amd.engine import hiplib as L
    assert (R.KEEP_F32, R.KEEP_BF16) == (L.F32, L.BF16)
    assert (R.AMAX_SLOTS, R.AMAX_OFF) == (T.AMAX_SLOTS, T.AMAX_OFF)
    assert set(R.REFS) == set(T.FLAT_CASES)
    seen = {}
    for fn, cid, params, t, regions, specs in _flat_case_refs():
        outs = {n for r in regions if r.role != 'r' and r.compare for n in r.windows}
        judged = set(specs) | ({'counts'} if any(s['kind'] == 'dets' for s in specs.values()) else set())
        assert judged == outs, (fn, cid, sorted(judged), sorted(outs))
        klass = R.case_class(fn, specs)
        assert klass in FLAT_CLASSES, (fn, cid, klass)
        seen.setdefault(klass, set()).add(fn)
        with pytest.raises(KeyError, match='dilation'):
            R.reference(fn, dict(params, dilation=2), t)
    assert set(seen) == FLAT_CLASSES, sorted(FLAT_CLASSES - set(seen))
    with pytest.raises(KeyError):
        R.reference('keep_fft', {}, {})
    # the two entry points whose class depends on a parameter have a case of either class
    assert seen['exact'] >= {'keep_nchw_to_nhwc', 'keep_act_inplace'} and seen['f32-arith'] >= {'keep_nchw_to_nhwc', 'keep_act_inplace'}


def test_flat_judge_bites(capsys):
    """flat_ref.judge on the CPU, for every flat case: the reference itself (cast to the output dtype) passes; it fails with the LAST element
    of any output (the ragged tail) or a middle one moved by 10 x tol x scale -- one bit or one index for exact and index outputs --, with
    an amax slot one ulp off, a written neighbour slot, a miscounted or foreign survivor."""
    import flat_ref as R
    n_bites = n_cases = 0
    for fn, cid, params, t, regions, specs in _flat_case_refs():
        got = R.fake_outputs(specs)
        R.judge(fn, cid, specs, got)
        n_cases += 1
        for what, wrong in R.doctored(specs, got):
            with pytest.raises(AssertionError):
                R.judge(fn, cid, specs, wrong)
                pytest.fail(f'{fn}[{cid}]: the judge let "{what}" pass')
            n_bites += 1
    assert n_cases >= 111 and n_bites >= 2 * n_cases, (n_cases, n_bites)
    assert capsys.readouterr().out.count('[flat-values]') >= n_bites


def test_flat_refs_feel_every_optional_input():
    """For every flat case and every optional input or switch it uses, the reference without it differs from the full one by at least
    SENSITIVITY x tol x scale (bits of an exact output differ): a kernel that ignores the input cannot pass."""
    import flat_ref as R
    seen = set()
    for fn, cid, params, t, regions, specs in _flat_case_refs():
        for what, name, other in R.removals(fn, params, t):
            s = specs[name]
            if s['kind'] == 'exact':
                assert not torch.equal(other['ref'], s['ref']), (fn, cid, what)
                got = dict(R.fake_outputs(specs), **{name: other['ref']})
            else:
                tol, sc, _ = R.spec_tol(s)
                d = float((other['ref'].to(torch.float64) - s['ref']).abs().max())
                assert d >= R.SENSITIVITY * tol * sc, (fn, cid, what, d / sc, tol)
                got = dict(R.fake_outputs(specs), **{name: other['ref'].float().to(R.fake_outputs(specs)[name].dtype)})
            with pytest.raises(AssertionError):
                R.judge(fn, cid, specs, got)
                pytest.fail(f'{fn}[{cid}]: the judge let a kernel without "{what}" pass')
            seen.add((fn, what))
    assert seen == {('keep_layernorm', 'residual'), ('keep_layernorm', 'pos'), ('keep_layernorm', 'out2 is not out'), ('keep_layernorm_amax', 'residual'),
                    ('keep_norm_finalize', 'gamma'), ('keep_norm_finalize', 'beta'), ('keep_group_stats', 'gamma'), ('keep_group_stats', 'beta'),
                    ('keep_norm_act_bf16', 'scale / shift'), ('keep_gm_join', 'sa'), ('keep_gm_join', 'ha'),
                    ('keep_token_linear', 'bias'), ('keep_dwconv3x3', 'bias'), ('keep_affine_act', 'activation'), ('keep_dwconv3x3', 'activation'),
                    ('keep_act_inplace', 'activation'), ('keep_norm_act_bf16', 'activation'), ('keep_add_bcast', 'alpha'), ('keep_nchw_to_nhwc', 'mode'),
                    ('keep_slice_copy', 'up'), ('keep_sep_filter', 'classes + lut'), ('keep_paste_face', 'mask_border'),
                    ('keep_warp_affine_u8', 'border colour'), ('keep_yolo_letterbox_u8', 'swap_rb')}, sorted(seen)


def test_flat_table_inputs_respect_the_caps_of_the_judge():
    """The caps of the index / selection rules hold for the table's own inputs, computed from the float64 references alone: the vq margin
    rule leaves out no row (cap 1 %); every score of the two selectors sits farther than 1e-6 from its threshold; the `aligned` cases hold
    every frame's survivors and the `ragged_overflow` cases hold at least one frame beside at least one that overflows."""
    import flat_ref as R
    for fn, cid, params, t, regions, specs in _flat_case_refs():
        for s in specs.values():
            if s['kind'] == 'argmin':
                top2 = torch.topk(s['d'], 2, dim=1, largest=False).values
                clear = (top2[:, 1] - top2[:, 0]) > R.VQ_MARGIN * float(s['d'].abs().max())
                assert 1.0 - float(clear.float().mean()) <= R.VQ_MAX_SKIPPED and bool(clear.all()), (fn, cid)
            if s['kind'] == 'dets':
                assert float((s['score'] - s['thr']).abs().min()) > 100 * R.THRESHOLD_BAND, (fn, cid)
                cnt = s['alive'].sum(1).tolist()
                fits = [c <= s['cap'] for c in cnt]
                assert all(c > 0 for c in cnt)
                assert all(c < s['cap'] for c in cnt) if cid == 'aligned' else (any(fits) and not all(fits)), (fn, cid, cnt, s['cap'])
