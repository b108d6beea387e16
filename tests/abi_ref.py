"""Plain float64 restatements of the two struct ABIs of include/keep_hip.h -- ``keep_conv2d`` and ``keep_attention`` -- and the
judge that compares a launch of a footprint-table case (tests/test_gpu_footprint.py: CONV_CASES / ATTN_CASES) with them.  torch on
the CPU only: no GPU, no library.  tests/test_gpu_case_values.py feeds the judge device outputs; tests/test_host_logic.py feeds it
doctored references (it must bite) and checks that every optional input of every case moves the reference by far more than the
tolerance (a kernel that ignores an input cannot pass).

Tolerances (chosen by the kernel instantiation the launch takes, not by the `mma` requested):

    exact-f32 kernels   err <= 2e-4 * scale                                   (TOL of the GPU modules)
    x3 kernels          err_x3 <= max(3 * err_f32, 2e-6 * scale), err_f32 <= 2e-4 * scale   (``yardstick``; err_f32: the exact-f32 twin)
    x1 kernels          per output: err <= (2^-10 + 2e-6) * sum |x| |w|  (single fp16: both operands rounded once, relative 2^-11 each,
                        the range scales are powers of two; x is what enters the product, behind the prologue; 2e-6: the x3 bound
                        of the fp32 accumulation and epilogue -- tests/test_gpu_conv_x3s_schedule.py derives the same from the format)
    bf16 kernels        against the reference on bf16-rounded operands: 2e-5 * scale, 2e-3 * scale with a prologue activation
                        (a fast-exp swish moves a bf16 rounding of the activated input), 6e-3 * scale for attention (P is
                        rounded too); a bf16 OUTPUT adds one bf16 ulp at scale, 2^-8 * scale, against the unrounded reference

err = max |out - reference| over every element, scale = max(1, max |reference|).
"""
import copy
import math

import torch
import torch.nn.functional as F

import keep_oracle as O

TOL = 2e-4
BF16_TOL, BF16_TOL_PRO_ACT, BF16_TOL_ATTN, BF16_ULP = 2e-5, 2e-3, 6e-3, 2.0 ** -8
X1_TOL = 2.0 ** -10 + 2e-6   # per output, times sum |x| |w|
SENSITIVITY = 100.0          # an optional input removed must move the reference by >= SENSITIVITY * tol * scale
AUX_W, LN_EPS = 0.5, 1e-5    # the constants the table passes as keep_conv2d_args.aux_w / ln_eps

# numeric values of include/keep_hip.h (engine/hiplib.py carries the same; tests/test_host_logic.py compares them)
MMA_F32, MMA_BF16, MMA_X3, MMA_X1 = 0, 1, 2, 3
PRO_NONE, PRO_SWISH, PRO_RELU = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_GELU, ACT_SIGMOID, ACT_LRELU01, ACT_SILU = 0, 1, 2, 3, 4, 5, 6
ATTN_NO_X3 = 4


def bf16r(t):
    """RNE rounding to bf16, as a float64 tensor."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def measure(got, ref):
    """(err, scale, flat position of the worst element) of a device result against a float64 reference of the same shape."""
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    d = (got - ref).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, math.inf))
    pos = int(d.reshape(-1).argmax())
    return float(d.reshape(-1)[pos]), max(1.0, float(ref.abs().max())), pos


def yardstick(what, e3, e32, sc, e3np=None):
    """The suite's x3 bound; prints the ratios the PR description quotes (run with -s)."""
    extra = '' if e3np is None else f' err_x3_nopack {e3np:.3e}'
    print(f'[x3-yardstick] {what}: err_x3 {e3:.3e} err_f32 {e32:.3e} ratio {e3 / max(e32, 1e-300):.2f}{extra} scale {sc:.3g}')
    assert e32 <= TOL * sc, f'{what}: f32 kernel err {e32:.3e} (scale {sc:.3g})'
    assert e3 <= max(3.0 * e32, 2e-6 * sc), f'{what}: x3 err {e3:.3e} vs f32-kernel err {e32:.3e} (scale {sc:.3g})'
    if e3np is not None:
        assert e3np <= max(3.0 * e32, 2e-6 * sc), f'{what}: un-packed x3 err {e3np:.3e} vs f32-kernel err {e32:.3e} (scale {sc:.3g})'


# ------------------------------------------------------------------------------------------------ keep_conv2d
# every attribute a _Geom of the table can carry: the table's keys and the sizes _Geom derives from them
GEOM_KEYS = {'mma', 'N', 'H', 'W', 'Cin', 'Cout', 'k', 'stride', 'pad', 'pad_t', 'pad_l', 'Ho', 'Wo', 'in_ld', 'in_off', 'out_ld', 'out_off',
             'res_ld', 'aux', 'pro', 'pro_act', 'act', 'split_k', 'stats', 'amax', 'in_amax', 'in2_cin1', 'reflect', 'upsample', 'in_bf16',
             'out_bf16', 'bk256', 'ln', 'flags', 'launch', 'cin1', 'x3', 'x1', 'amax_stale', 'pro_amp', 'bias_amp', 'w_amp', 'w_peak', 'w_floor', 'x_amp', 'act_after_res'}


def _act_pro(x, kind):
    if kind == PRO_NONE:
        return x
    if kind == PRO_SWISH:
        return x * torch.sigmoid(x)
    if kind == PRO_RELU:
        return torch.relu(x)
    raise ValueError(f'prologue activation {kind}')


def _act(x, kind):
    if kind == ACT_NONE:
        return x
    if kind == ACT_RELU:
        return torch.relu(x)
    if kind in (ACT_LRELU02, ACT_LRELU01):
        return F.leaky_relu(x, 0.2 if kind == ACT_LRELU02 else 0.1)
    if kind == ACT_GELU:
        return F.gelu(x)                      # exact erf form
    if kind == ACT_SIGMOID:
        return torch.sigmoid(x)
    if kind == ACT_SILU:
        return x * torch.sigmoid(x)
    raise ValueError(f'epilogue activation {kind}')


def conv2d_ref(g, t, linear=None):
    """keep_conv2d of include/keep_hip.h in float64.  ``g``: a ``_Geom`` of the table; ``t``: name -> PAYLOAD tensor (x [N,H,W,cin1],
    w [Cout, k*k*Cin], bias, pro_scale / pro_shift [N,Cin], res / aux [N*Ho*Wo, Cout], x2, ln_gamma / ln_beta, wb); an absent
    optional tensor is the identity of its step.  Returns out [N*Ho*Wo, Cout], the per-(n, c) sum / sum of squares of it
    (``stats_sum`` / ``stats_sumsq`` [N, Cout]), ``amax`` [N], ``absdot`` (sum |x| |w| of every output, x behind the prologue: what the x1
    bound scales with) and ``out_rounded`` (RNE bf16) for a bf16 output.  ``g.act_after_res`` (no table case sets it): the activation
    applied to conv + residual instead of before the residual -- a deliberately wrong variant for the sensitivity checks.
    ``linear``: the ``linear`` entry of an earlier answer for the same inputs, prologue and padding (the convolution before the bias
    and its sum |x| |w|), for a variant that differs behind it only."""
    unknown = set(vars(g)) - GEOM_KEYS
    if unknown:
        raise KeyError(f'conv2d_ref: geometry keys it does not know: {sorted(unknown)}')
    N, H, W, Cin, Cout, k = g.N, g.H, g.W, g.Cin, g.Cout, g.k
    if linear is None:
        bf = g.mma == MMA_BF16
        x = t['x'].to(torch.float64).reshape(N, H, W, g.cin1)
        if g.in2_cin1:
            x = torch.cat([x, t['x2'].to(torch.float64).reshape(N, H, W, Cin - g.cin1)], dim=-1)
        if t.get('pro_scale') is not None:
            x = x * t['pro_scale'].to(torch.float64).reshape(N, 1, 1, Cin)
        if t.get('pro_shift') is not None:
            x = x + t['pro_shift'].to(torch.float64).reshape(N, 1, 1, Cin)
        x = _act_pro(x, g.pro_act)
        w = (t['wb'] if bf and t.get('wb') is not None else t['w']).to(torch.float64).reshape(Cout, k, k, Cin)
        if bf:                                     # operands RNE-rounded to bf16 when staged (a bf16 tensor is unchanged by it)
            x, w = bf16r(x), bf16r(w)
        x = x.permute(0, 3, 1, 2)
        if g.upsample:                             # 1 and KEEP_UPSAMPLE_X2_PHASES: nearest x2
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        Hv, Wv = x.shape[2:]
        if g.reflect:
            assert g.pad_t == g.pad_l < min(Hv, Wv)
            x = F.pad(x, (g.pad_l, g.pad_l, g.pad_t, g.pad_t), mode='reflect')
        else:                                      # the caller's Ho / Wo decide how far the window runs: missing bottom / right taps are zeros
            need_h, need_w = (g.Ho - 1) * g.stride + k, (g.Wo - 1) * g.stride + k
            x = F.pad(x, (g.pad_l, max(0, need_w - Wv - g.pad_l), g.pad_t, max(0, need_h - Hv - g.pad_t)))
        rows = lambda y: y[:, :, :g.Ho, :g.Wo].permute(0, 2, 3, 1).reshape(N * g.Ho * g.Wo, Cout)  # noqa: E731
        v = F.conv2d(x, w.permute(0, 3, 1, 2), None, stride=g.stride)
        assert v.shape[2] >= g.Ho and v.shape[3] >= g.Wo, (tuple(v.shape), g.Ho, g.Wo)
        v = rows(v)
        absdot = rows(F.conv2d(x.abs(), w.abs().permute(0, 3, 1, 2), None, stride=g.stride))
    else:
        v, absdot = linear
    linear = (v, absdot)
    if t.get('bias') is not None:
        v = v + t['bias'].to(torch.float64).reshape(1, Cout)
    if g.ln:                                   # biased variance, before the residual
        mu = v.mean(1, keepdim=True)
        v = (v - mu) / torch.sqrt(((v - mu) ** 2).mean(1, keepdim=True) + LN_EPS)
        if t.get('ln_gamma') is not None:
            v = v * t['ln_gamma'].to(torch.float64).reshape(1, Cout)
        if t.get('ln_beta') is not None:
            v = v + t['ln_beta'].to(torch.float64).reshape(1, Cout)
    after = getattr(g, 'act_after_res', False)
    a = v if after else _act(v, g.act)
    r = t['res'].to(torch.float64).reshape(-1, Cout) if t.get('res') is not None else None
    if after:
        assert r is not None and t.get('aux') is None
        out = _act(a + r, g.act)
    elif t.get('aux') is not None:
        r0 = 0.0 if r is None else r
        out = r0 + AUX_W * (r0 * t['aux'].to(torch.float64).reshape(-1, Cout) + a)
    elif r is not None:
        out = a + r
    else:
        out = a
    per = out.reshape(N, g.Ho * g.Wo, Cout)
    res = dict(out=out, stats_sum=per.sum(1), stats_sumsq=(per * per).sum(1), amax=per.abs().amax((1, 2)), absdot=absdot, linear=linear)
    if g.out_bf16:
        res['out_rounded'] = bf16r(out)
    return res


CONV_FOLLOW_UPS = ('conv_splitk_reduce4_kernel', 'conv_splitk_reduce_kernel', 'conv_stats_replica_kernel', 'conv_x3_gather_stats_replica_kernel')
# template position of the single-fp16 flag X1 in the kernels that have one (keep_conv2d_launch_plan spells every argument out)
_X1_ARG = {'conv3x3_halo_x3s_kernel': (3, 2), 'conv3x3_halo_x3s_act_kernel': (4, 2), 'conv3x3_halo_x3_kernel': (7, 6), 'conv_x3_kernel': (10, 9)}


def conv_kernel(launched):
    """The convolution kernel of a string keep_conv2d_launch_plan answers: without the zero-fill of the amax slots before it and the
    follow-up kernels behind it (a split-K reducer, a statistics replica), which are judged through what they write."""
    parts = [p for p in launched.split(' + ') if p not in ('zero_u32_kernel', 'LayerNorm') and p not in CONV_FOLLOW_UPS]      # ('+ LayerNorm': the plan's name of that form)
    assert len(parts) == 1, launched
    return parts[0]


def conv_class(kernel):
    """Tolerance class -- 'f32', 'x3', 'x1', 'bf16', or 'plan-only' for a plan that launches nothing -- of a kernel string: the launched
    instantiation keep_conv2d_launch_plan names (follow-up kernels included) or the family string of keep_conv2d_plan.  Anything else
    raises: a new instantiation must be classified before its cases can be judged."""
    if kernel == '(keep_norm_act_bf16 first)':
        return 'plan-only'
    kernel = conv_kernel(kernel)
    name, _, rest = kernel.partition('<')
    args = [a.strip() for a in rest.rstrip('>').split(',')] if rest else []
    if name in ('conv_f32_kernel', 'conv3x3_halo_f32_kernel', 'conv3x3_cout4_kernel'):
        return 'f32'
    if name in ('conv3x3_halo3_kernel', 'conv3x3_halo_kernel', 'conv_bf16_kernel', 'conv3x3_c3_kernel'):
        return 'bf16'
    if name == 'conv3x3_up2_x1s_kernel' or args == ['32', 'x2 phases', 'true']:
        return 'x1'
    if name in _X1_ARG and len(args) == _X1_ARG[name][0]:
        return 'x1' if args[_X1_ARG[name][1]] in ('true', '1') else 'x3'
    if name in ('conv3x3_halo_x3_kernel', 'gemm_x3l_kernel', 'conv_x3_kernel', 'conv3x3_c3_x3_kernel', 'conv3x3_halo_x3s_kernel', 'conv3x3_x3p_kernel',
                'conv3x3_x3q_kernel', 'conv3x3_up2_x3s_kernel'):      # (the shorter argument lists of the plan's family strings: x3 forms)
        return 'x3'
    raise KeyError(f'no tolerance class for kernel {kernel!r}')


def conv_tol(klass, g):
    """Element tolerance of a convolution case, relative to scale (x3: the ceiling of its yardstick's f32 leg).  The x1 class has none:
    its bound is per output (``conv_bound``)."""
    if klass in ('f32', 'x3'):
        return TOL
    assert klass == 'bf16', klass
    return (BF16_TOL_PRO_ACT if g.pro_act != PRO_NONE else BF16_TOL) + (BF16_ULP if g.out_bf16 else 0.0)


def conv_bound(klass, g, ref):
    """What |out - reference| may reach per output element: a [N*Ho*Wo, Cout] tensor for x1, else tolerance x scale."""
    if klass == 'x1':
        return X1_TOL * ref['absdot']
    return torch.full_like(ref['out'], conv_tol(klass, g) * max(1.0, float(ref['out'].abs().max())))


def conv_twin_kw(kw):
    """Geometry of the exact-f32 twin of an x3 case: KEEP_MMA_F32, the x3-only inputs and flags cleared.  The three features with
    no f32 kernel are decomposed by the caller: `ln` (GEMM, then keep_layernorm with the residual), `in2` (GEMM on the
    materialised concatenation), x2 phases (upsample = 1 with the plain weights).  Fused statistics / the output maximum are not
    asked of the twin: only its `out` is used."""
    tw = dict(kw, mma=MMA_F32, flags=0)
    for key in ('in_amax', 'amax', 'stats', 'in2_cin1', 'ln'):
        tw.pop(key, None)
    if kw.get('ln'):
        tw.pop('res_ld', None)
    if kw.get('in2_cin1'):
        tw.pop('in_ld', None)
        tw.pop('in_off', None)
    if tw.get('upsample'):
        tw['upsample'] = 1
    return tw


def _where(pos, g):
    row, c = divmod(pos, g.Cout)
    n, p = divmod(row, g.Ho * g.Wo)
    return f'image {n} pixel ({p // g.Wo}, {p % g.Wo}) channel {c}'


def judge_conv(name, kernel, g, got, ref, twin_out=None, stats_P=0):
    """Compare one launch of a convolution case with ``conv2d_ref``'s answer ``ref``.  ``got``: name -> device result: 'out'
    [N*Ho*Wo, Cout]; 'stats' (g.stats) the [N][stats_P][Cout][2] partials; 'amax' (g.amax) with 'amax_lo' / 'amax_hi', the other
    slots of its arena.  ``twin_out``: the exact-f32 twin's `out` (x3 kernels).  Prints the case's line; raises AssertionError."""
    klass = conv_class(kernel)
    out = got['out']
    err, sc, pos = measure(out, ref['out'])
    line = f'[case-values] conv {name}: {kernel} [{klass}] err {err:.3e} scale {sc:.3g} worst at {_where(pos, g)}'
    if klass == 'x3':
        assert twin_out is not None, f'{name}: an x3 kernel is judged against its exact-f32 twin'
        e32, _, _ = measure(twin_out, ref['out'])
        print(f'{line} err_f32 {e32:.3e}')
        yardstick(f'conv {name}', err, e32, sc)
        bound = max(3.0 * e32, 2e-6 * sc)
    elif klass == 'x1':      # per output, against its own sum |x| |w|
        lim = conv_bound(klass, g, ref)
        d = (out.detach().cpu().to(torch.float64) - ref['out']).abs()
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
        over = (d / lim).reshape(-1)
        pos = int(over.argmax())
        bound = float(lim.max())
        print(f'{line} bound {bound:.3e} worst err / (sum|x||w|) {float(over[pos]) * X1_TOL:.3e} of {X1_TOL:.3e}')
        assert float(over[pos]) <= 1.0, (f'conv {name} ({kernel}): err {float(d.reshape(-1)[pos]):.3e} > {float(lim.reshape(-1)[pos]):.3e} = '
                                         f'{X1_TOL:.3e} x sum|x||w| at {_where(pos, g)}')
    else:
        bound = conv_tol(klass, g) * sc
        print(f'{line} bound {bound:.3e}')
    assert klass == 'x1' or err <= bound, f'conv {name} ({kernel}): err {err:.3e} > {bound:.3e} (scale {sc:.3g}), worst at {_where(pos, g)}'
    N, HW, Cout = g.N, g.Ho * g.Wo, g.Cout
    if g.amax:
        per = out.detach().cpu().float().reshape(N, -1).abs().amax(1)
        slots = got['amax'].detach().cpu().reshape(N)
        assert torch.equal(slots.view(torch.int32), per.view(torch.int32)), f'conv {name}: amax slots {slots.tolist()} != max |out[n]| {per.tolist()}'
        for side in ('amax_lo', 'amax_hi'):
            assert not got[side].detach().cpu().view(torch.int32).any(), f"conv {name}: a neighbouring amax slot was written: {side} = {got[side].tolist()}"
    if g.stats:
        assert stats_P > 0
        base = bound if klass in ('x3', 'x1') else conv_tol(klass, dict_view(g, out_bf16=False)) * sc      # statistics are taken before a bf16 rounding
        part = got['stats'].detach().cpu().to(torch.float64).reshape(N, stats_P, Cout, 2).sum(1)
        absum = ref['out'].abs().reshape(N, HW, Cout).sum(1)
        for what, have, want, lim in (('sum', part[..., 0], ref['stats_sum'], HW * base + HW * 2.0 ** -24 * absum),
                                      ('sumsq', part[..., 1], ref['stats_sumsq'], HW * base * 2 * sc + HW * 2.0 ** -24 * ref['stats_sumsq'])):
            over = (have - want).abs() - lim
            i = int(over.reshape(-1).argmax())
            assert float(over.reshape(-1)[i]) <= 0, (f'conv {name}: fused {what} of image {i // Cout} channel {i % Cout}: {float(have.reshape(-1)[i])!r} vs '
                                                    f'{float(want.reshape(-1)[i])!r}, allowed {float(lim.reshape(-1)[i]):.3e}')
    return err, sc


def dict_view(g, **over):
    """A copy of geometry ``g`` with some attributes replaced."""
    g2 = copy.copy(g)
    g2.__dict__.update(over)
    return g2


def conv_removals(g, t):
    """(what, geometry, tensors) of the reference with one optional input of the case removed -- every input the case switches on."""
    N = g.N
    drop = lambda *names: {k_: v for k_, v in t.items() if k_ not in names}  # noqa: E731
    if t.get('bias') is not None:
        yield 'bias', g, drop('bias')
    if g.pro:
        yield 'pro_scale', g, drop('pro_scale')
        yield 'pro_shift', g, drop('pro_shift')
        if N > 1:
            yield 'per-image prologue rows', g, dict(t, pro_scale=t['pro_scale'].roll(1, 0), pro_shift=t['pro_shift'].roll(1, 0))
    if g.pro_act != PRO_NONE:
        yield 'prologue activation', dict_view(g, pro_act=PRO_NONE), t
    if g.act != ACT_NONE:
        yield 'epilogue activation', dict_view(g, act=ACT_NONE), t
    if g.res_ld:
        yield 'residual', g, drop('res')
    if g.aux:
        yield 'aux', g, drop('aux')
    if g.reflect:
        yield 'reflect', dict_view(g, reflect=False), t
    if g.in2_cin1:
        yield 'in2', g, dict(t, x2=torch.zeros_like(t['x2']))
    if g.ln:
        yield 'ln_gamma', g, drop('ln_gamma')
        yield 'ln_beta', g, drop('ln_beta')


def conv_neighbours(g, t, ref):
    """(what, `out`) of the case as a NEIGHBOURING instantiation or a wrong epilogue order would compute it -- what a wrong arm of a launch
    macro gives: every other epilogue activation of the seven; every other prologue activation, and the affine dropped; the activation
    applied after the residual instead of before it; zero padding in place of reflection padding and the other way round (where the
    convolution pads at all).  ``ref``: the case's own answer (its linear part is reused where the variant differs behind it only)."""
    for act in (ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_GELU, ACT_SIGMOID, ACT_LRELU01, ACT_SILU):
        if act != g.act:
            yield f'epi_act {act}', conv2d_ref(dict_view(g, act=act), t, ref['linear'])['out']
    # (bf16 tensors: conv3x3_halo3_kernel / conv_bf16_kernel carry no PRO template argument -- a bf16 input admits no prologue at all, and
    # a bf16 output is judged to one bf16 ulp at scale, which no prologue variant of these cases clears a hundredfold beside its bias)
    pro_forms = not (g.in_bf16 or g.out_bf16)
    for pact in (PRO_NONE, PRO_SWISH, PRO_RELU):
        if pact != g.pro_act and pro_forms:
            yield f'pro_act {pact}', conv2d_ref(dict_view(g, pro_act=pact), t)['out']
    if g.pro and pro_forms:
        yield 'affine dropped', conv2d_ref(g, {k_: v for k_, v in t.items() if k_ not in ('pro_scale', 'pro_shift')})['out']
    if g.res_ld and g.act != ACT_NONE and not g.aux:
        yield 'activation after the residual', conv2d_ref(dict_view(g, act_after_res=True), t, ref['linear'])['out']
    Hv, Wv = (2 * g.H, 2 * g.W) if g.upsample else (g.H, g.W)
    if g.k > 1 and g.pad_t == g.pad_l == g.k // 2 and g.pad_t < min(Hv, Wv) and g.mma != MMA_BF16:      # (KEEP_MMA_BF16 refuses KEEP_PAD_REFLECT: no such neighbour)
        yield ('zero padding' if g.reflect else 'reflection padding'), conv2d_ref(dict_view(g, reflect=not g.reflect), t)['out']


# ------------------------------------------------------------------------------------------------ keep_attention: mode 2
def win_shift(h, w, ks, shift):
    wh, ww = h // ks, w // ks
    return (wh // 2, ww // 2) if shift else (0, 0)


def win_split(x, h, w, ks, sy, sx):
    """[n, h*w, C] image frame -> [n*ks*ks, wh*ww, C]: rolled by (-sy, -sx), cut into windows (GM/transformer.py:75-85)."""
    n, _, c = x.shape
    x = torch.roll(x.reshape(n, h, w, c), shifts=(-sy, -sx), dims=(1, 2))
    return O._split_cl(x.contiguous(), ks).reshape(n * ks * ks, -1, c)


def win_merge(x, h, w, ks, sy, sx):
    """The inverse of ``win_split``: [n*ks*ks, wh*ww, C] window frame -> [n, h*w, C] image frame."""
    c = x.shape[-1]
    img = O._merge_cl(x.reshape(-1, h // ks, w // ks, c), ks)
    return torch.roll(img, shifts=(sy, sx), dims=(1, 2)).reshape(-1, h * w, c)


def win_regions(h, w, ks):
    """[ks*ks, wh*ww] region id of every window token in the rolled frame (the slices of GM/transformer.py:24-35)."""
    wh, ww = h // ks, w // ks
    img = torch.zeros((1, h, w, 1))
    cnt = 0
    for hs in (slice(0, -wh), slice(-wh, -(wh // 2)), slice(-(wh // 2), None)):
        for ws in (slice(0, -ww), slice(-ww, -(ww // 2)), slice(-(ww // 2), None)):
            img[:, hs, ws, :] = cnt
            cnt += 1
    return O._split_cl(img, ks).reshape(ks * ks, -1)


def win_ref(q, k, v, h, w, ks, shift, kv_rot, rows, mask_value=-100.0, scale=None, roll=True):
    """fp64 window attention at window-local query rows `rows`: [n*ks*ks, len(rows), C].  Image i reads keys / values of image
    (i + kv_rot) % n; shift adds `mask_value` to cross-region scores (the reference: -100).  ``scale``: 1 / sqrt(C) unless given;
    ``roll`` = False leaves the grid un-rolled under the same mask (a deliberately wrong variant for sensitivity checks)."""
    n, _, c = q.shape
    sy, sx = win_shift(h, w, ks, shift and roll)
    qw = win_split(q.double(), h, w, ks, sy, sx)[:, rows]
    kw = win_split(torch.roll(k.double(), -kv_rot, 0), h, w, ks, sy, sx)
    vw = win_split(torch.roll(v.double(), -kv_rot, 0), h, w, ks, sy, sx)
    s = torch.matmul(qw, kw.transpose(1, 2)) * (1.0 / math.sqrt(c) if scale is None else scale)
    if shift:
        reg = win_regions(h, w, ks).repeat(n, 1)
        s = torch.where(reg[:, rows, None] != reg[:, None, :], s + mask_value, s)
    return torch.matmul(torch.softmax(s, dim=-1), vw)


# ------------------------------------------------------------------------------------------------ keep_attention: mode 1
def sparse_causal_keys(t, Bc, T, second=True):
    """[Bc*T, Lt, C] -> [Bc*T, 2 Lt, C]: the keys / values of frame f are [frame 0 ; frame max(f-1, 0)] of the same clip (KA:704-716);
    ``second`` = False reads frame 0 twice (a deliberately wrong variant for sensitivity checks)."""
    Lt, C = t.shape[1:]
    former = torch.clamp(torch.arange(T) - 1, min=0) if second else torch.zeros(T, dtype=torch.long)
    t = t.reshape(Bc, T, Lt, C)
    return torch.cat([t[:, [0] * T], t[:, former]], dim=2).reshape(Bc * T, 2 * Lt, C)


def sparse_causal_ref(qkv, Bc, T, Lt, H, D, rows):
    """KA:704-716 in fp64: keys / values of frame f = [frame 0 ; frame max(f-1, 0)] of the same clip; [Bc*T, rows, H*D]."""
    inner = H * D
    q, k, v = (t.double() for t in qkv.reshape(Bc * T, Lt, 3 * inner).split(inner, dim=-1))
    return heads_ref(q[:, rows], sparse_causal_keys(k, Bc, T), sparse_causal_keys(v, Bc, T), H, 1.0 / math.sqrt(D))


def heads_ref(q, k, v, H, scale):
    """Plain multi-head softmax(scale q k^T) v in the dtype given: q [B, Lq, H*D], k [B, Lk, H*D], v [B, Lk, H*Dv] -> [B, Lq, H*Dv]."""
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    hs = lambda t, L_: t.reshape(B, L_, H, -1).permute(0, 2, 1, 3)  # noqa: E731
    s = torch.matmul(hs(q, Lq), hs(k, Lk).transpose(2, 3)) * scale
    return torch.matmul(torch.softmax(s, dim=-1), hs(v, Lk)).permute(0, 2, 1, 3).reshape(B, Lq, -1)


# ------------------------------------------------------------------------------------------------ keep_attention: the table cases
ATTN_KEYS = {'name', 'mma', 'B', 'H', 'Lq', 'Lk', 'D', 'Dv', 'mode', 'packed', 'o_ld', 'o_off', 'amax', 'in_bf16', 'flags', 'ws', 'T', 'seg_len',
             'img_h', 'img_w', 'ksplit', 'shift', 'kv_rot', 'n_img', 'lk_rows', 'scale_mul', 'amp'}
ATTN_REMOVALS = ('mask', 'roll', 'kv_rot', 'second segment', 'heads')


def attn_scale(c):
    """keep_attention_args.scale of a table case: ``scale_mul`` / sqrt(D)."""
    return c.get('scale_mul', 1.0) / math.sqrt(c['D'])


def attention_ref(c, q, k, v, remove=None):
    """keep_attention of include/keep_hip.h in float64 for table case ``c`` on the payloads q [B, Lq, H*D], k [B, rows, H*D],
    v [B, rows, H*Dv] -> o [B*Lq, H*Dv].  KEEP_MMA_BF16: q, k, v RNE-rounded to bf16 first.  ``remove``: one of ATTN_REMOVALS,
    the deliberately wrong variants of the sensitivity checks."""
    unknown = set(c) - ATTN_KEYS
    if unknown:
        raise KeyError(f'attention_ref: case keys it does not know: {sorted(unknown)}')
    assert remove is None or remove in ATTN_REMOVALS, remove
    B, H, Lq, Lk, D, Dv = c['B'], c['H'], c['Lq'], c['Lk'], c['D'], c['Dv']
    rnd_ = bf16r if c['mma'] == MMA_BF16 else (lambda t: t.to(torch.float64))
    q, k, v = rnd_(q).reshape(B, Lq, H * D), rnd_(k).reshape(B, -1, H * D), rnd_(v).reshape(B, -1, H * Dv)
    scale = attn_scale(c)
    if remove == 'heads':                      # keys / values of the wrong head
        k, v = k.reshape(B, -1, H, D).flip(2).reshape(B, -1, H * D), v.reshape(B, -1, H, Dv).flip(2).reshape(B, -1, H * Dv)
    if c['mode'] == 0:
        assert k.shape[1] == Lk
        o = heads_ref(q, k, v, H, scale)
    elif c['mode'] == 1:
        T, seg = c['T'], c['seg_len']
        assert B % T == 0 and k.shape[1] == seg and Lk == 2 * seg
        second = remove != 'second segment'
        o = heads_ref(q, sparse_causal_keys(k, B // T, T, second), sparse_causal_keys(v, B // T, T, second), H, scale)
    elif c['mode'] == 2:
        h, w, ks, n = c['img_h'], c['img_w'], c['ksplit'], c['n_img']
        assert H == 1 and B == n * ks * ks and Lq == Lk == (h // ks) * (w // ks)
        img = lambda t: t.reshape(n, h * w, -1)  # noqa: E731
        shift = c['shift'] > 0
        # (query rows in blocks of 1024: the float64 scores of a 4224-token window frame would be 0.6 GB at once)
        ow = torch.cat([win_ref(img(q), img(k), img(v), h, w, ks, shift, 0 if remove == 'kv_rot' else c['kv_rot'], rows,
                                mask_value=0.0 if remove == 'mask' else -100.0, scale=scale, roll=remove != 'roll')
                        for rows in torch.arange(Lq).split(1024)], dim=1)
        o = win_merge(ow, h, w, ks, *win_shift(h, w, ks, shift))
    else:
        raise ValueError(f"mode {c['mode']}")
    return o.reshape(B * Lq, H * Dv)


def attn_class(c):
    if c['mma'] == MMA_BF16:
        return 'bf16'
    return 'x3' if c['mma'] == MMA_X3 and not c['flags'] & ATTN_NO_X3 else 'f32'


def attn_tol(klass):
    return BF16_TOL_ATTN if klass == 'bf16' else TOL


def attn_case_removals(c):
    """The removals that apply to table case ``c`` (each switches off something the case switches on)."""
    if c['mode'] == 2:
        if c['shift']:
            yield 'mask'
            yield 'roll'
        if c['kv_rot']:
            yield 'kv_rot'
    if c['mode'] == 1:
        yield 'second segment'
    if c['H'] > 1:
        yield 'heads'


def judge_attn(c, got, ref, twin_out=None):
    """Compare one launch of attention case ``c`` (`got`: o [B*Lq, H*Dv]) with ``attention_ref``'s answer."""
    klass = attn_class(c)
    err, sc, pos = measure(got, ref)
    row, col = divmod(pos, c['H'] * c['Dv'])
    where = f"batch {row // c['Lq']} query {row % c['Lq']} head {col // c['Dv']} channel {col % c['Dv']}"
    line = f"[case-values] attn {c['name']}: [{klass}] err {err:.3e} scale {sc:.3g} worst at {where}"
    if klass == 'x3':
        assert twin_out is not None, f"{c['name']}: an x3 kernel is judged against its exact-f32 twin"
        e32, _, _ = measure(twin_out, ref)
        print(f'{line} err_f32 {e32:.3e}')
        yardstick(f"attn {c['name']}", err, e32, sc)
        bound = max(3.0 * e32, 2e-6 * sc)
    else:
        bound = attn_tol(klass) * sc
        print(f'{line} bound {bound:.3e}')
    assert err <= bound, f"attn {c['name']}: err {err:.3e} > {bound:.3e} (scale {sc:.3g}), worst at {where}"
    return err, sc
