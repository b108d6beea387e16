"""keep_conv2d_plan of one library over a fixed grid of keep_conv2d_args, WITHOUT a device: per row the return code, every field of
keep_conv2d_plan_out and the keep_last_error text.  Pointers are fake addresses (the planner reads only their alignment).  Two libraries
plan alike when their tables are the same file (``cmp``); profiles/conv_plan_refactor.txt is such a comparison.

    python tools/dev/conv_plan_table.py LIB.so OUT.txt [--record RECORD.json] [--time PASSES [--versus OTHER.so]]

The grid: tests/test_gpu_footprint.py's CONV_CASES, the distinct keep_conv2d rows of a tools/dev/host_launch_record.py record (--record),
and a product over policy x kernel form x map x Cin x Cout with one option varied at a time around it (N, plan_ref_images, split_k, upsample,
reflect, prologue, epilogue, second input, LayerNorm, statistics, bk256, bf16 tensors, every flag bit, absent / misaligned tensors).
--time: also print the median seconds of PASSES passes of keep_conv2d_plan over the rows; with --versus every pass times OTHER, LIB and
OTHER again, in this one process, and the three medians are printed (OTHER's two are its own spread)."""
import argparse, ctypes as C, hashlib, itertools, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('lib'); ap.add_argument('out'); ap.add_argument('--record'); ap.add_argument('--time', type=int, default=0); ap.add_argument('--versus')
opt = ap.parse_args()
os.environ['KEEP_HIP_LIB'] = os.path.abspath(opt.lib)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
from __graft_entry__ import load_package
load_package()
from comfyui_keep_amd.engine import hiplib as L
import test_gpu_footprint as T

lib = L.load(check_device=False)
lib.keep_last_error.restype = C.c_char_p
BASE = 0x10000
PTRS = [n for n, t in L.ConvArgs._fields_ if t is C.c_void_p]
KSP = {'3x3': (3, 1, 1), '3x3s2': (3, 2, 1), '1x1': (1, 1, 0), '7x7': (7, 1, 3), '4x4s4': (4, 4, 0)}
MAPS = [(8, 32), (16, 16), (16, 32), (64, 64), (5, 7), (20, 12), (18, 18), (300, 1), (777, 1), (4133, 1)]
CINS, COUTS = [2, 3, 16, 24, 32, 48, 128, 512], [3, 4, 20, 32, 48, 64, 96, 128, 130]
FLAG_BITS = [1 << b for b in range(16)]
X1_BITS = [L.CONV_X1_GEMM, L.CONV_X1_HALO16, L.CONV_X1_GEMM | L.CONV_X1_HALO16]


def make(mma, ksp, hw, cin, cout, N=1, ref=0, split_k=0, upsample=0, reflect=False, pro=False, pro_act=0, act=0, res=False, aux=False,
         in2=0, ln=False, stats=False, bk256=0, in_bf16=False, out_bf16=False, flags=0, no_wx3=False, mis=None, acc_scale=0.5):
    """One argument struct with every optional tensor at an aligned fake address (`mis`: the name of one tensor 4 bytes off)."""
    k, s, pad = KSP[ksp]
    H, W = hw
    Hv, Wv = (2 * H, 2 * W) if upsample else (H, W)
    Ho, Wo = (Hv + 2 * pad - k) // s + 1, (Wv + 2 * pad - k) // s + 1
    if Ho <= 0 or Wo <= 0:
        return None
    p = {'inp': BASE, 'weight': BASE, 'bias': BASE, 'out': BASE}
    if pro: p['pro_scale'] = p['pro_shift'] = BASE
    if res or aux: p['residual'] = BASE
    if aux: p['aux'] = BASE
    if mma == L.MMA_BF16: p['weight_bf16'] = BASE
    if mma in (L.MMA_X3, L.MMA_X1) and not no_wx3: p['weight_x3'] = BASE
    if in2: p['in2'] = BASE
    if ln: p['ln_gamma'] = p['ln_beta'] = BASE
    if split_k > 1: p['workspace'] = BASE
    if stats: p['stats_out'] = BASE
    if mis: p[mis] = p.get(mis, BASE) + 4
    cin1 = in2 if in2 else cin
    return L.conv_args(N=N, H=H, W=W, Cin=cin, Cout=cout, KH=k, KW=k, stride=s, pad_t=pad, pad_l=pad, Ho=Ho, Wo=Wo, in_ld=cin1, out_ld=cout,
                       res_ld=cout if (res or aux) else 0, upsample=upsample, pro_act=pro_act, epi_act=act, aux_w=0.5, split_k=split_k,
                       dtype=L.BF16 if in_bf16 else L.F32, mma=mma, stats_P=0, bk256=bk256, out_dtype=L.BF16 if out_bf16 else L.F32,
                       x3_acc_scale=acc_scale, in2_cin1=in2, pad_mode=L.PAD_REFLECT if reflect else L.PAD_ZERO, ln_eps=1e-5 if ln else 0.0,
                       flags=flags, plan_ref_images=ref, **p)


VARIANTS = [dict(N=3), dict(N=16), dict(ref=2), dict(ref=256), dict(split_k=1), dict(split_k=3), dict(upsample=1), dict(upsample=2),
            dict(reflect=True), dict(pro=True), dict(pro=True, pro_act=1), dict(pro=True, pro_act=2), dict(pro_act=1), dict(pro=True, reflect=True),
            dict(act=2), dict(res=True), dict(aux=True), dict(in2=32), dict(in2=16), dict(ln=True), dict(ln=True, N=3), dict(stats=True), dict(bk256=1),
            dict(in_bf16=True), dict(out_bf16=True), dict(in_bf16=True, pro=True), dict(in_bf16=True, out_bf16=True), dict(no_wx3=True),
            dict(acc_scale=0.0), dict(ref=256, flags=L.CONV_X1_HALO16), dict(ref=1, flags=L.CONV_X1_HALO16), dict(split_k=3, flags=L.CONV_X1_HALO16),
            dict(act=2, flags=L.CONV_X1_HALO16), dict(mis='inp'), dict(mis='out'), dict(mis='bias'), dict(mis='pro_scale', pro=True),
            dict(mis='weight_x3'), dict(mis='weight_bf16')] + [dict(flags=f) for f in FLAG_BITS + X1_BITS]


def invalid_rows():
    """One row per argument check of validate_conv / conv_args_in (each breaks one field of a valid call)."""
    def base(**kw):
        a = make(L.MMA_X3, '3x3', (8, 32), 32, 32)
        for n, v in kw.items(): setattr(a, n, v)
        return a
    rows = [base(struct_size=8), base(dtype=7), base(dtype=L.BF16), base(N=0), base(in_ld=8), base(out_ld=8), base(pro_scale=BASE),
            base(aux=BASE), base(residual=BASE, res_ld=8), base(split_k=-1), base(Ho=40), base(mma=9), base(upsample=3), base(pad_mode=5),
            base(N=1 << 23), base(ln_gamma=BASE)]
    for mma in (L.MMA_F32, L.MMA_BF16, L.MMA_X1):
        a = base(mma=mma, in2=BASE, in2_cin1=16, upsample=0); rows.append(a)
        a = base(mma=mma, upsample=2); rows.append(a)
        a = base(mma=mma, pad_mode=L.PAD_REFLECT, pad_t=0); rows.append(a)
    rows.append(base(pad_mode=L.PAD_REFLECT, pad_l=0))
    return rows


def grid(record):
    rows = []
    for name in T.CONV_CASES:
        captured = []
        orig = L.conv2d_plan
        L.conv2d_plan = lambda a: captured.append(a) or orig(a)
        try:
            T.conv_case_plan(name)
        finally:
            L.conv2d_plan = orig
        rows.append(captured[0])
    if record:      # [name, kernel, mma, flags, split_k, field values in ConvArgs order (pointers as set / not set)]
        seen = set()
        for eng in json.load(open(record)):
            for c in eng['calls']:
                if c[0] != 'keep_conv2d' or json.dumps(c[5:]) in seen: continue
                seen.add(json.dumps(c[5:]))
                a = L.ConvArgs()
                for (n, t), v in zip(L.ConvArgs._fields_, c[5:]):
                    setattr(a, n, (BASE if v else None) if t is C.c_void_p else v)
                rows.append(a)
    # the product: policy x form x map x Cin x Cout, plain calls
    for mma, ksp, hw, cin, cout in itertools.product(range(4), KSP, MAPS, CINS, COUTS):
        rows.append(make(mma, ksp, hw, cin, cout))
    # one option at a time around a deterministic 1-in-9 slice of the product (plus the GEMM / LayerNorm shapes the options need)
    for i, (mma, ksp, hw, cin, cout) in enumerate(itertools.product(range(4), KSP, MAPS, CINS, COUTS)):
        if i % 9 != (i // 9) % 9: continue
        for v in VARIANTS:
            rows.append(make(mma, ksp, hw, cin, cout, **v))
    for mma, hw, cin, cout, v in itertools.product((L.MMA_X3, L.MMA_X1), [(8, 8), (64, 1), (192, 1), (256, 1)], (128, 256, 512, 1024, 2048), (32, 128),
                                                   [dict()] + VARIANTS):
        rows.append(make(mma, '1x1', hw, cin, cout, **v))
    for hw, cin, v in itertools.product([(8, 32), (16, 16), (16, 32)], (16, 32, 64), VARIANTS):      # cout4 / c3 / halo forms with every option
        for mma, cout in itertools.product(range(4), (4, 64)):
            rows.append(make(mma, '3x3', hw, cin, cout, **v))
            rows.append(make(mma, '3x3', hw, 3, cout, **v))
    return [r for r in rows if r is not None] + invalid_rows() + [None, 'no out']      # (NULL args, NULL plan output)


def plan_row(a):
    out = L.ConvPlanOut()
    if not isinstance(a, L.ConvArgs):
        rc = lib.keep_conv2d_plan(None, C.byref(out)) if a is None else lib.keep_conv2d_plan(C.byref(rows[0]), None)
    else:
        rc = lib.keep_conv2d_plan(C.byref(a), C.byref(out))
    if rc != 0:
        return f'rc={rc} err={lib.keep_last_error().decode()}'
    return 'rc=0 ' + ' '.join(f'{n}={getattr(out, n).decode() if n == "kernel" else getattr(out, n)}' for n, _ in L.ConvPlanOut._fields_)


rows = grid(opt.record)
lines = [plan_row(a) for a in rows]
open(opt.out, 'w').write('\n'.join(lines) + '\n')
kernels = sorted({l.split('kernel=')[1] for l in lines if 'kernel=' in l})
errors = sorted({l.split('err=')[1] for l in lines if 'err=' in l})
print(json.dumps({'rows': len(lines), 'sha256': hashlib.sha256(open(opt.out, 'rb').read()).hexdigest(), 'kernels': kernels, 'errors': errors}, indent=1))
if opt.time:
    out = L.ConvPlanOut(); refs = [C.byref(a) for a in rows if isinstance(a, L.ConvArgs)]; o = C.byref(out)
    fs = [C.CDLL(os.path.abspath(opt.lib)).keep_conv2d_plan]      # (fresh handles: both libraries are called without declared argument types)
    if opt.versus:
        other = C.CDLL(os.path.abspath(opt.versus)).keep_conv2d_plan
        fs = [other, fs[0], other]
    ts = [[] for _ in fs]
    for _ in range(opt.time):
        for f, t in zip(fs, ts):
            t0 = time.perf_counter()
            for r in refs: f(r, o)
            t.append(time.perf_counter() - t0)
    print('median_seconds', *[sorted(t)[len(t) // 2] for t in ts])
