"""Host-side launch record of one source tree, WITHOUT a device: every library entry point is replaced by a recorder and 'cuda' devices
map to the CPU, so what the host decides -- plans (keep_conv2d_plan is host code and runs for real), policies, flags, scales, call order --
is written down exactly as it would be handed to the GPU.  Per engine and precision: the ordered calls, for every keep_conv2d its plan's
kernel name and every non-pointer field of keep_conv2d_args plus which pointers are set, for keep_attention its policy, flags and shape, for
every other call its name and numeric arguments.  KeepNet is recorded per (precision, flow knob, upsample knob), two forwards each (the second
is served from the route and plan caches), with ``twin_bytes`` and ``clips_per_call`` before and after the twins are built.

    python tools/dev/host_launch_record.py TREE OUT.json          # TREE: this checkout or an exported copy of another commit (with its built library)

Two records of two trees compare with ``==`` on the JSON; profiles/f16_policy_unification.txt is such a comparison."""

import contextlib, ctypes as C, json, os, sys
ROOT = os.path.abspath(sys.argv[1]); OUT = sys.argv[2]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch
def _cpu(d):
    return torch.device('cpu') if d is not None and 'cuda' in str(d) else d
for fn in ('empty', 'zeros', 'ones', 'tensor', 'full', 'arange', 'as_tensor'):
    def mk(orig):
        def f(*a, **k):
            if 'device' in k: k['device'] = _cpu(k['device'])
            return orig(*a, **k)
        return f
    setattr(torch, fn, mk(getattr(torch, fn)))
_to = torch.Tensor.to
def to(self, *a, **k):
    a = tuple(_cpu(x) if isinstance(x, (str, torch.device)) else x for x in a)
    if 'device' in k: k['device'] = _cpu(k['device'])
    return _to(self, *a, **k)
torch.Tensor.to = to
torch.Tensor.cuda = lambda self, *a, **k: self
torch.cuda.current_device = lambda: 0
torch.cuda.device = lambda d: contextlib.nullcontext()
torch.cuda.synchronize = lambda *a: None
class _Dummy:
    def __init__(self, *a, **k): pass
    def __enter__(self): return self
    def __exit__(self, *a): return False
    def record(self, *a): pass
    def wait(self, *a): pass
    def synchronize(self): pass
    def wait_event(self, *a): pass
    def wait_stream(self, *a): pass
    def query(self): return True
torch.cuda.Stream = torch.cuda.Event = _Dummy
torch.cuda.stream = lambda s: _Dummy()
torch.cuda.current_stream = lambda *a: _Dummy()
torch.Tensor.pin_memory = lambda self, *a, **k: self
torch.Tensor.record_stream = lambda self, *a: None
os.environ['KEEP_AMD_GRAPH'] = '0'
from __graft_entry__ import load_package
load_package()
from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import parsenet as PN, retinaface as RF, yoloface as YF
_load = L.load
L.load = lambda check_device=True: _load(check_device=False)
LOG = []
_plan = L.conv2d_plan
PTR = {n for n, t in L.ConvArgs._fields_ if t is C.c_void_p}
def launch(a):
    pl = _plan(a)
    rec = ['keep_conv2d', pl.kernel.decode(), int(a.mma), int(a.flags), int(a.split_k)]
    for n, _ in L.ConvArgs._fields_:
        v = getattr(a, n)
        rec.append(bool(v) if n in PTR else (v if isinstance(v, (int, float)) else repr(v)))
    LOG.append(rec)
def call(name, *args):
    LOG.append([name] + [x for x in args if isinstance(x, (int, float))])
L.conv2d_launch, L.call = launch, call
def attention(**kw):      # the policy of the call (the single-fp16 route shows in mma / flags), its shape, and which range pointers are set
    LOG.append(['keep_attention'] + [int(kw[f]) for f in ('mma', 'flags', 'in_dtype', 'B', 'H', 'Lq', 'Lk', 'D', 'Dv', 'mode', 'ksplit', 'shift')]
               + [kw[f] is not None for f in ('q_amax', 'k_amax', 'v_amax')])
L.attention = attention
def nhwc(t): return t.permute(0, 2, 3, 1).contiguous()
rows = []
from comfyui_keep_amd.engine import synth
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
from comfyui_keep_amd.engine.net import KeepNet
W = synth.synth_state_dict(seed=0)
clip = synth.synth_clip(T=2, B=1, seed=1234)
def free_hbm(free):      # clips_per_call reads the free memory of the device: a fixed figure, nothing reserved
    torch.cuda.mem_get_info = lambda *a: (int(free), int(288e9))
    torch.cuda.memory_reserved = torch.cuda.memory_allocated = lambda *a: 0
def clips(net):
    """clips_per_call(20) at 200 GB free, and a reading fine enough to see every twin's bytes: 64 x 64 frames, T = 1, 2.5 GB free, no cap."""
    free_hbm(200e9); coarse = net.clips_per_call(20)
    free_hbm(2.5e9); os.environ['KEEP_AMD_MAX_CLIPS'] = str(10 ** 6)
    fine = net.clips_per_call(1, 64, 64)
    del os.environ['KEEP_AMD_MAX_CLIPS']
    return [coarse, fine]
# (precision, flow, upsample): the four base policies, then the two knobs alone, together on 'f16'
for prec, flow, up in (('fp32', 'x3', 'x3'), ('x3', 'x3', 'x3'), ('bf16', 'x3', 'x3'), ('f16', 'x3', 'x3'),
                       ('x3', 'f16', 'x3'), ('x3', 'x3', 'f16'), ('f16', 'f16', 'f16')):
    net = KeepNet(**DEFAULT_ARCH); net.load_state_dict(W, strict=True); net.to('cuda').eval().set_precision(prec)
    net.set_flow_precision(flow); net.set_upsample_precision(up)
    name = 'KeepNet/' + prec + ('' if (flow, up) == ('x3', 'x3') else f'/flow={flow}/up={up}')
    row = {'name': name, 'clips_unbuilt': clips(net)}
    for leg in ('calls', 'calls_again'):      # the second forward: routes and plans served from the caches
        del LOG[:]
        try:
            net(clip)
        except Exception as e:
            import traceback; traceback.print_exc(limit=3)
            LOG.append(['EXC', type(e).__name__, str(e)[:80]])
        row[leg] = list(LOG)
        print(name, leg, len(LOG), sum(1 for c in LOG if c[0] == 'keep_conv2d'), sum(1 for c in LOG if c[0] == 'keep_conv2d' and c[2] == L.MMA_X1),
              sum(1 for c in LOG if c[0] == 'keep_attention'), sum(1 for c in LOG if c[0] == 'keep_attention' and c[1] == L.MMA_X1),
              sum(1 for c in LOG if c[0] == 'keep_absmax'), [c for c in LOG if c[0] == 'EXC'], flush=True)
    row.update(mma=int(net.o.mma), twin_elems=[net.twin_bytes(p) for p in ('fp32', 'x3', 'bf16', 'f16')] + [net.twin_bytes()], clips_built=clips(net))
    rows.append(row)
def record(name, make, run):
    eng = make(); del LOG[:]
    try:
        run(eng)
    except Exception as e:      # (host code behind the network that reads device results may choke on uninitialised memory)
        LOG.append(['EXC', type(e).__name__, str(e)[:80]])
    rows.append({'name': name, 'calls': list(LOG), 'mma': int(eng.o.mma), 'x1': eng.o.blobx1 is not None, 'x3': eng.o.blobx3 is not None,
                 'twin_elems': [0 if t is None else t.numel() for t in (eng.o.blobx3, eng.o.blobx1)]})
    print(name, len(LOG), sum(1 for c in LOG if c[0] == 'keep_conv2d'), sum(1 for c in LOG if c[0] == 'keep_absmax'), [c for c in LOG if c[0] == 'EXC'], flush=True)
for size, n in ((128, 2), (512, 1), (512, 16)):
    Wp = PN.synth_parsenet_state_dict(seed=0, in_size=size, out_size=size)
    x = torch.zeros(n, size, size, 3)
    for prec in ('x3', 'fp32', 'f16'):
        record(f'ParseNet{size}x{n}/{prec}', lambda: PN.ParseNetEngine(Wp, in_size=size, out_size=size, precision=prec).to('cuda'), lambda e: e.logits_nhwc(x))
for bb in ('resnet50', 'mobile0.25'):
    Wr = RF.synth_retinaface_state_dict(seed=0, backbone=bb)
    for shape in ((2, 160, 224, 3), (1, 720, 1280, 3)):
        x = torch.zeros(shape)
        for prec in ('x3', 'fp32', 'f16'):
            record(f'RetinaFace-{bb}{shape}/{prec}', lambda: RF.RetinaFaceEngine(Wr, precision=prec).to('cuda'), lambda e: e.raw_outputs(x))
for name in ('YOLOv5l', 'YOLOv5n'):
    Wy = YF.synth_yolo_state_dict(name, seed=0)
    for shape in ((2, 96, 128, 3), (2, 128, 128, 3), (1, 768, 1280, 3)):
        x = torch.zeros(shape)
        for prec in ('x3', 'fp32', 'f16'):
            record(f'{name}{shape}/{prec}', lambda: YF.YoloFaceEngine(Wy, precision=prec).to('cuda'), lambda e: e.forward_nhwc(x))
json.dump(rows, open(OUT, 'w'))
