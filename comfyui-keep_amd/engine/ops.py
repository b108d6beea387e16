"""Tensor-level wrappers over the C-ABI: shape bookkeeping + output allocation only.

All activations are channels-last fp32 device tensors: feature maps ``[N,H,W,C]``, token
matrices ``[M,C]`` (same memory).  torch is used for allocation (caching allocator -> safe
inside hipGraph capture) and views; every arithmetic op is a ``libkeep_hip.so`` kernel.

Nothing here knows how ``keep_conv2d`` tiles its work: kernel choice, split-K, workspace and
statistics sizes come from ``keep_conv2d_plan`` (cached per argument signature).  The precision
policy and the weight blobs it needs live on an ``Ops`` INSTANCE owned by one ``KeepNet`` -- two
nets (or two threads) with different policies never share state.  The module-level functions
are the methods of a default fp32 instance (kernel tests call them with explicit ``mma=``).
"""
import bisect
import os

import torch

from . import hiplib as L

TOKEN_LINEAR = os.environ.get('KEEP_NO_TOKEN_LINEAR') is None   # dev switch: streaming GEMM for the GMFlow projections
UP2_PHASES = os.environ.get('KEEP_X3_UP2', '1') != '0'      # x3 policy: nearest x2 + 3x3 as four 2x2-tap phase convolutions (A/B: 0)
ATTN_PRESPLIT = os.environ.get('KEEP_X3_ATTN_PRESPLIT', '1') != '0'   # x3 policy: GMFlow's k / v projections write split-fp16 halves, no pack pass (A/B: 0)
FUSE_LN = os.environ.get('KEEP_X3_FUSE_LN', '1') != '0'      # x3 policy: GMFlow `merge -> norm1` / `mlp.2 -> norm2` LayerNorms in the GEMM epilogue (A/B: 0)
USE_BK256 = bool(int(os.environ.get('KEEP_BK256', '0')))   # measured slower than BK=64 + split-K at B<=4 (kept for A/B)
# bf16 policy: inputs of fewer pixels (N*H*W) than this skip the normalise+activate -> bf16 pass in front of the halo
# conv and use the kernel variant that applies the prologue while staging (A/B switch, default: always the two-pass form)
HALO_PRENORM_MINPIX = int(os.environ.get('KEEP_HALO_PRENORM_MINPIX', '0'))

DEBUG_SYNC = os.environ.get('KEEP_DEBUG_SYNC') is not None
X3_STREAM_KERNEL = 'conv3x3_halo_x3s_kernel'      # keep_conv2d_plan's name of the x3 streaming 3x3 kernel: the one family KeepNet's 'f16' substitutes
X1_UP2_KERNEL = 'conv3x3_halo_x3_kernel<32, x2 phases, true>'    # keep_conv2d_plan's name of the single-fp16 x2-phase Upsample kernel (L.CONV_X1_UP2): what ``Ops.up2_x1`` routes to
_PLAN_CACHE = {}
POLICY_NAMES = {L.MMA_F32: 'fp32', L.MMA_BF16: 'bf16', L.MMA_X3: 'x3'}      # the base policies of an Ops
# Deployment settings of the library, read ONCE here (the library itself reads no environment variable: they travel in the argument
# structs).  KEEP_PLAN_REF_IMAGES: the fixed reference batch of the parity policies' plans (default 16; 2 = latency profile for single
# clips; results are batch-invariant within one value).  KEEP_X3_EXACT_ACT=1: library expf / erff inside the x3 kernels.
PLAN_REF_IMAGES = int(os.environ.get('KEEP_PLAN_REF_IMAGES', '0') or 0)
DEFAULT_CONV_FLAGS = L.CONV_X3_EXACT_ACT if os.environ.get('KEEP_X3_EXACT_ACT') else 0


class Plan:
    __slots__ = ('split_k', 'ws_floats', 'stats_P', 'wants_bf16_input', 'out_bf16_ok', 'out_amax_ok', 'kernel')

    def __init__(self, o):
        self.split_k = o.split_k
        self.ws_floats = o.workspace_bytes // 4
        self.stats_P = o.stats_P
        self.wants_bf16_input = bool(o.wants_bf16_input)
        self.out_bf16_ok = bool(o.out_bf16_ok)
        self.out_amax_ok = bool(o.out_amax_ok)
        self.kernel = o.kernel.decode()


class Stats:
    """What a producing convolution knows about its output for free (reduced in its epilogue): per-channel (sum, sumsq)
    partials [N,P,C,2] for the next GroupNorm / InstanceNorm, and (x3 policy) the per-image max |y| [N] -- the range probe
    of the next x3 operator that reads the tensor un-normalised.  Either may be None."""
    __slots__ = ('part', 'P', 'amax')

    def __init__(self, part=None, P=0, amax=None):
        self.part, self.P, self.amax = part, P, amax


def _plan(a, key, split_cols=None):
    """keep_conv2d_plan for these arguments, cached by everything the decision can depend on (shapes, flags, which
    optional tensors exist, pointer alignment class) -- never by values.  ``split_cols`` (part of ``key``): keep_conv2d_split_plan."""
    pl = _PLAN_CACHE.get(key)
    if pl is None:
        pl = _PLAN_CACHE[key] = Plan(L.conv2d_plan(a) if split_cols is None else L.conv2d_split_plan(a, split_cols))
    return pl


def _row_of(table, off, n):
    """Row (first element, one past the last, 2^-e) of the tensor that holds elements off .. off + n of the packed blob, in a
    ``([first element], rows)`` table sorted by offset (``make_x3_blob`` / ``make_x1_blob``); None when no tensor of the table does."""
    starts, rows = table
    i = bisect.bisect_right(starts, off) - 1
    return rows[i] if i >= 0 and off + n <= rows[i][1] else None


def empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def offset(t, off):
    """Flat view of ``t`` starting ``off`` elements in (channel-slice pointer for strided kernels)."""
    return t.view(-1)[off:] if off else t


class Ops:
    def __init__(self):
        # matrix-core operand precision of keep_conv2d / keep_attention launches, the BASE policy of this Ops:
        #   L.MMA_F32 exact f32 (parity), L.MMA_X3 split fp16 x 3 (parity-grade fast policy), L.MMA_BF16 (speed policy).
        #   Single fp16 (L.MMA_X1, 'f16') is never a base: it is a base policy plus an x1 twin (set_x1_twin)
        self.mma = L.MMA_F32
        self.attn_mma = L.MMA_F32
        self.blob32 = None      # packed fp32 weight blob the twins below are resolved against (same element offsets)
        self.blob16 = None      # bf16 twin
        self.blobx3 = None      # split-fp16 twin: int16 tensor, 2 elements per weight, per-tensor [.., Cin/16, hi16|lo16]
        self.x3_acc_scale = 1.0
        self._x3_table = None
        self._up2, self._up2_src = {}, (None, None)
        # bench.py's roofline leg: when a list, every keep_conv2d launch is bracketed by HIP events on the launch stream
        # and appended as (kernel family, algorithmic_flops, split_k, start_event, end_event, algorithmic_bytes)
        self.profile = None
        self.amax_arena = None     # x3: per-forward arena of fused max|out| slots (begin_forward)
        self.amax_pos = 0
        self.status = None         # one device int32: KEEP_STATUS_* bits raised by this forward's kernels (begin_forward zeroes it)
        self.arena_generation = 0  # bumped when the block is (re)allocated: hipGraphs captured before that are stale
        # keep_conv2d_args.flags / .plan_ref_images and keep_attention_args.flags of every launch of this Ops (kernel-selection
        # overrides for tests and A/B runs: hiplib.CONV_* / ATTN_*; the plan's reference batch: a per-net numerics setting)
        self.flags = DEFAULT_CONV_FLAGS
        self.attn_flags = 0
        self.plan_ref_images = PLAN_REF_IMAGES
        # 'f16': a hi-only twin (make_x1_blob) attached to the base policy by set_x1_twin -- conv() substitutes L.MMA_X1 in every call of
        # the base policy whose weight has such a twin and whose X1 plan the library admits (_route).  None: the plain base policy.
        self.blobx1 = None
        self._x1_table = None      # ([first element], [(first, one past the last, 2^-e)]) of the tensors blobx1 holds, sorted
        # what the library answered to `this call under L.MMA_X1?` (_route), per rule: the blob twin and the phase twin (``up2_x1``): base
        # plan key -> the call's X1 Plan | False; ``attn_x1``: shape key -> True | False
        self._x1_route, self._up2_x1_route, self._attn_x1_route = {}, {}, {}
        self._kv_split_route = {}      # shape key -> True | False: the library's answer to `this attention call with kv_split?`
        self.x1_flags = L.CONV_X1_GEMM      # opt-in form bits OR-ed into the X1 plan query and launch
        self.x1_base = L.MMA_X3             # the policy a call without a twin, or one the library refuses, stays on
        self.x1_base_kernel = None          # restriction: substitute only where the base plan is this kernel, un-split (None: everywhere)
        self.census = None         # when a dict: kernel name (plan string) -> launches, counted by conv() (tests, tools/bench_precision.py)
        # single-fp16 attention (L.MMA_X1 | L.ATTN_X1): off by default.  True: attention() asks the library about every call of the x3
        # base once per shape (_route) and runs it single-fp16 where admitted -- KeepNet's flow Ops (KEEP_AMD_FLOW_PRECISION=f16)
        self.attn_x1 = False
        # single-fp16 x2-phase Upsample convolutions (L.MMA_X1 | L.CONV_X1_UP2): off by default -- conv() then issues no plan query beyond the
        # base's.  True: the up2 branch of conv() asks the library once per plan key (_route) and runs the call on the hi-only phase twin
        # (up2_x1_twin) where admitted -- KeepNet's KEEP_AMD_UPSAMPLE_PRECISION=f16
        self.up2_x1 = False
        # single-fp16 fused GMFlow FFN (keep_gm_ffn_x1): off by default -- gm_ffn() is then gm_ffn_x3(), no plan query.  True: gm_ffn() asks the
        # library once per token shape and alignment class (_route, keep_gm_ffn_x1_plan) and runs the block on the hi-only twins
        # (ffn_w0_x1_twin / ffn_w2_x1_twin) where admitted -- KeepNet's KEEP_AMD_FLOW_FFN_PRECISION=f16
        self.ffn_x1 = False
        self._ffn_x1_route = {}      # (C, hidden, alignment classes) -> True | False

    def begin_forward(self, device):
        """Zero this forward's bookkeeping words with ONE fill launch: the status word (non-finite logits / tensors, see
        keep_argmax_gather, keep_nonfinite_flag) and, for the x3 policy, the arena of per-image max|out| slots the convolutions
        fill with atomicMax (instead of one zero-fill launch per convolution: 2.4 k launches per 16-clip step).  A slot lives
        until the next begin_forward: Stats objects never outlive the forward pass that made them.
        The block is allocated ONCE per Ops and device and never freed or swapped while the Ops lives: captured hipGraphs
        bake its address in, so dropping it on a policy change (as round 2 did) left replays writing through a dangling pointer."""
        self.ensure_arena(device)
        self._block.zero_()
        self.amax_pos = 0

    def ensure_arena(self, device):
        device = torch.device(device)
        if self.amax_arena is None or self.amax_arena.device != device:
            self._block = torch.empty((1 << 18) + 4, dtype=torch.float32, device=device)
            self.amax_arena = self._block[4:]
            self.status = self._block[:1].view(torch.int32)
            self.arena_generation += 1

    def set_precision(self, mma, blob32=None, blob16=None, blobx3=None, x3_acc_scale=1.0, x3_scales=None):
        """x3_scales: per-tensor accumulator scales of the split-fp16 twin, [(first element, one past the last, 2^-e), ...] sorted
        by offset (``make_x3_blob``); without it every tensor of the blob carries ``x3_acc_scale``."""
        if mma not in (L.MMA_F32, L.MMA_BF16, L.MMA_X3):
            raise ValueError(f"set_precision: {mma!r} is no base policy (single fp16 is a base policy plus set_x1_twin)")
        self._x3_table = ([a for a, _, _ in x3_scales], list(x3_scales)) if x3_scales else None
        self.mma = self.attn_mma = mma
        self.set_x1_twin()      # ('f16' re-attaches its twin after every policy change)
        self._forget_routes(self._x1_route, self._up2_x1_route, self._attn_x1_route, self._ffn_x1_route, self._kv_split_route)
        if blobx3 is not None and (blob32 is not self._up2_src[0] or blobx3 is not self._up2_src[1]):
            # phase kernels of the Upsample convolutions (up2_twin): derived from THESE blob objects -- a new upload, even one that lands
            # on the same addresses, starts from an empty cache; a policy switch on the same blobs keeps it (captured x3 graphs hold
            # the addresses of its tensors)
            self._up2, self._up2_src = {}, (blob32, blobx3)
        self.blob32, self.blob16, self.blobx3, self.x3_acc_scale = blob32, blob16, blobx3, float(x3_acc_scale)

    def set_x1_twin(self, blobx1=None, ranges=None, flags=L.CONV_X1_GEMM, base=L.MMA_X3, base_kernel=None):
        """'f16' on top of the base policy set by ``set_precision``: ``blobx1`` is ``make_x1_blob``'s hi-only twin, ``ranges`` its (first
        element, one past the last, 2^-e) table -- the x1 launches take their ``x3_acc_scale`` from it.  None: back to the plain base.
        ``flags``: opt-in form bits of the X1 plan query and launch (RetinaFace: L.CONV_X1_GEMM, the default; YOLOv5-face adds
        L.CONV_X1_HALO16; ParseNet and KeepNet: 0).  ``base``: the policy the twin rides on, which must be this Ops' (a call without a
        twin, or one the library refuses, stays there).  ``base_kernel``: substitute only calls whose base plan is this kernel, un-split
        (KeepNet: X3_STREAM_KERNEL)."""
        if blobx1 is not None and self.mma != base:
            raise ValueError(f"set_x1_twin: this twin rides on the {POLICY_NAMES[base]} policy (set_precision(...) with it first)")
        self.blobx1, self.x1_flags, self.x1_base, self.x1_base_kernel = blobx1, int(flags), base, base_kernel
        self._x1_table = None
        if blobx1 is not None:
            rows = sorted((int(a), int(b), float(s)) for a, b, s in ranges)
            self._x1_table = ([a for a, _, _ in rows], rows)
        self._forget_routes(self._x1_route)

    def _x1_of(self, w):
        """(hi-only fp16 copy, accumulator scale 2^-e) of an fp32 weight view, or None when no twin is attached or the tensor has none
        (a view that does not lie inside the packed blob has none: the call runs as it would without 'f16')."""
        if self.blobx1 is None or not w.is_contiguous():
            return None
        off = (w.data_ptr() - self.blob32.data_ptr()) // 4
        row = _row_of(self._x1_table, off, w.numel())
        return None if row is None else (self.blobx1[off:off + w.numel()], row[2])

    def x1_twin(self, w):
        """Hi-only fp16 copy of an fp32 weight view for the 'f16' substitution, or None (then the layer stays on the base policy)."""
        tw = self._x1_of(w)
        return None if tw is None else tw[0]

    @staticmethod
    def _route(routes, key, query):
        """The single-fp16 substitution rule of every call site: what the library answered to `this call under L.MMA_X1?`, asked once
        per ``key`` of ``routes`` (``_x1_route``, ``_up2_x1_route``: ``query()`` is keep_conv2d_plan under L.MMA_X1 with the rule's twin and flags,
        the answer the call's X1 Plan; ``_attn_x1_route``: ``hiplib.attention_x1_plan``, the answer True).  KEEP_EUNSUP is the library's answer 'no kernel of
        this grade, stay on the base': False, cached like any other.  Every other failure is an error: it propagates and nothing is cached.
        The keys hold the per-image geometry, the alignment classes, the flags and the reference batch, never N: a route never depends on
        a clip's or frame's batch-mates."""
        r = routes.get(key)
        if r is None:
            try:
                r = query()
            except L.KeepHipError as e:
                if e.code != L.EUNSUP:
                    raise
                r = False
            routes[key] = r
        return r

    @staticmethod
    def _forget_routes(*routes):
        for r in routes:
            r.clear()

    # ------------------------------------------------------------------ weight twins
    def _blob_off(self, w):
        if self.blob32 is None:
            raise RuntimeError("this precision policy needs the packed weight blobs registered (Ops.set_precision)")
        off = (w.data_ptr() - self.blob32.data_ptr()) // 4
        if off < 0 or off + w.numel() > self.blob32.numel() or not w.is_contiguous():
            raise RuntimeError("weight view is not inside the packed blob; pass the twin explicitly")
        return off

    def bf16_twin(self, w):
        """bf16 copy of an fp32 weight view that lives inside the registered packed blob."""
        if self.blob16 is None:
            raise RuntimeError("bf16 policy needs the bf16 blob registered (Ops.set_precision)")
        off = self._blob_off(w)
        return self.blob16[off:off + w.numel()]

    def up2_twin(self, w):
        """(weight_x3, acc_scale) of the four 2x2-tap phase kernels of ``w`` (packed [Cout,3,3,Cin]) for
        ``upsample = UPSAMPLE_X2_PHASES`` -- built once per weight tensor (the first, eager, call) and kept for the lifetime of the
        blob it points into."""
        key = (w.data_ptr(), tuple(w.shape))
        tw = self._up2.get(key)
        if tw is None:
            w4 = up2_phase_weights(w)
            sc = x3_scale_for(float(w4.abs().max()))
            tw = self._up2[key] = (split_x3(w4.reshape(-1, w.shape[-1]), sc).view(-1), 1.0 / sc)
        return tw

    def up2_x1_twin(self, w):
        """(weight_x3, acc_scale) of the HI-ONLY phase twin of ``w`` for ``upsample = UPSAMPLE_X2_PHASES`` under L.MMA_X1 with
        L.CONV_X1_UP2: fp16(up2_phase_weights(w) * 2^e) as plain [4, Cout, 3*3, Cin] fp16 bit patterns and 2^-e (``up2_twin``'s scale).
        Built once per weight tensor (outside any stream capture: ``KeepNet._activate_precision``) and kept with the up2 twins."""
        key = ('up2_x1', w.data_ptr(), tuple(w.shape))
        tw = self._up2.get(key)
        if tw is None:
            w4 = up2_phase_weights(w)
            sc = x3_scale_for(float(w4.abs().max()))
            tw = self._up2[key] = ((w4 * sc).to(torch.float16).view(torch.int16).view(-1), 1.0 / sc)
        return tw

    def ffn_w2_twin(self, w2):
        """(weight_x3, acc_scale) of ``w2`` [C, hidden] for ``keep_gm_ffn_x3``: every group of 16 hidden units in the order
        [0-3, 8-11, 4-7, 12-15] (``ffn_w2_perm``), split with the tensor's own power-of-two scale.  Built once per weight tensor
        (outside any stream capture: ``KeepNet._activate_precision``) and kept with the up2 twins for the lifetime of the blob."""
        key = ('ffn_w2', w2.data_ptr(), tuple(w2.shape))
        tw = self._up2.get(key)
        if tw is None:
            wp = ffn_w2_perm(w2)
            sc = x3_scale_for(float(wp.abs().max()))
            tw = self._up2[key] = (split_x3(wp, sc).view(-1), 1.0 / sc)
        return tw

    def gm_ffn_x3(self, src, msg, w0, w2, gamma, beta, eps):
        """GMFlow FFN + norm2 + residual as one launch (x3 policy): LayerNorm(W2 . gelu(W0 . cat[src | msg])) + src; src, msg [M, C]
        fp32, w0 [8C, 2C] / w2 [C, 8C] fp32 views of the packed blob (their x3 twins are used)."""
        C = src.shape[-1]
        M = src.numel() // C
        out = empty((M, C), src)
        w2p, asc2 = self.ffn_w2_twin(w2)
        if self.profile is not None:            # bench.py's roofline leg: the fused block counts with the conv / GEMM path it replaces
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            Hd = w0.shape[0]
            self.profile.append(('gm_ffn_x3_kernel', 2.0 * M * (2 * C * Hd + Hd * C), 1, e0, e1,
                                 3 * M * C * 4 + (2 * C * Hd + Hd * C) * 4, (M // 4096 if M % 4096 == 0 else 1, M, 1, 2 * C, C, 1, 1, 0, False)))
            e0.record()
        L.call('keep_gm_ffn_x3', src, msg, self.x3_twin(w0), float(self.x3_scale_of(w0)), w2p, float(asc2), gamma, beta, float(eps), out,
               M, C, w0.shape[0], 1 if (self.flags & L.CONV_X3_EXACT_ACT) else 0)
        if self.profile is not None:
            self.profile[-1][4].record()
        return out.view(src.shape)

    def ffn_w0_x1_twin(self, w0):
        """(hi-only fp16 twin, acc_scale) of ``w0`` [hidden, 2C] for ``keep_gm_ffn_x1``: fp16(w0 * 2^e) as plain row-major bit patterns with
        the x3 twin's power of two (``x3_scale_of``) -- the numbers of the x3 twin's hi half.  Built once per weight tensor (outside any
        stream capture: ``KeepNet._activate_precision``) and kept with the up2 twins for the lifetime of the blob."""
        key = ('ffn_w0_x1', w0.data_ptr(), tuple(w0.shape))
        tw = self._up2.get(key)
        if tw is None:
            asc = float(self.x3_scale_of(w0))
            tw = self._up2[key] = ((w0.float() * (1.0 / asc)).to(torch.float16).view(torch.int16).view(-1), asc)
        return tw

    def ffn_w2_x1_twin(self, w2):
        """(hi-only fp16 twin, acc_scale) of ``w2`` [C, hidden] for ``keep_gm_ffn_x1``: fp16(ffn_w2_perm(w2) * 2^e) as [C, hidden] bit
        patterns with ``ffn_w2_twin``'s power of two -- the numbers of that twin's hi half.  Built and kept like ``ffn_w0_x1_twin``."""
        key = ('ffn_w2_x1', w2.data_ptr(), tuple(w2.shape))
        tw = self._up2.get(key)
        if tw is None:
            wp = ffn_w2_perm(w2)
            sc = x3_scale_for(float(wp.abs().max()))
            tw = self._up2[key] = ((wp * sc).to(torch.float16).view(torch.int16).view(-1), 1.0 / sc)
        return tw

    def gm_ffn(self, src, msg, w0, w2, gamma, beta, eps):
        """The fused GMFlow FFN of the x3 policy under the substitution rule ``ffn_x1``.  Off (default): ``gm_ffn_x3``, nothing else.  On:
        the library is asked once per (C, hidden, alignment classes) -- never M: a clip's route does not depend on its batch-mates -- whether
        it has the single-fp16 form (_route, keep_gm_ffn_x1_plan); where it has, the block runs as ``keep_gm_ffn_x1`` on the hi-only twins
        with the x3 twins' scales; KEEP_EUNSUP keeps the call on ``gm_ffn_x3``; any other failure raises."""
        if not self.ffn_x1:
            return self.gm_ffn_x3(src, msg, w0, w2, gamma, beta, eps)
        C = src.shape[-1]
        M = src.numel() // C
        Hd = w0.shape[0]
        out = empty((M, C), src)
        w0x, asc0 = self.ffn_w0_x1_twin(w0)
        w2x, asc2 = self.ffn_w2_x1_twin(w2)

        def mis(*ts):
            r = 0
            for t in ts:
                r |= t.data_ptr() % 16
            return r
        key = (C, Hd, mis(src, msg, out), mis(w0x, w2x), mis(gamma, beta))
        if not self._route(self._ffn_x1_route, key, lambda: L.gm_ffn_x1_plan(*key)):
            return self.gm_ffn_x3(src, msg, w0, w2, gamma, beta, eps)
        if self.profile is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.profile.append(('gm_ffn_x1_kernel', 2.0 * M * (2 * C * Hd + Hd * C), 1, e0, e1,
                                 3 * M * C * 4 + (2 * C * Hd + Hd * C) * 2, (M // 4096 if M % 4096 == 0 else 1, M, 1, 2 * C, C, 1, 1, 0, False)))
            e0.record()
        L.call('keep_gm_ffn_x1', src, msg, w0x, float(asc0), w2x, float(asc2), gamma, beta, float(eps), out,
               M, C, Hd, 1 if (self.flags & L.CONV_X3_EXACT_ACT) else 0)
        if self.profile is not None:
            self.profile[-1][4].record()
        return out.view(src.shape)

    def x3_twin(self, w):
        """split-fp16 copy of an fp32 weight view (row slices of a [Cout, .., Cin] tensor keep their layout), or None
        when the policy has no x3 blob / the tensor's Cin is not a multiple of 16 (such layers run on the f32 kernels)."""
        if self.blobx3 is None or w.shape[-1] % 16:
            return None
        off = self._blob_off(w)
        return self.blobx3[2 * off:2 * (off + w.numel())]

    def x3_scale_of(self, w):
        """Accumulator scale (2^-e) of the twin of weight view ``w``: its own tensor's (a row slice shares its tensor's scale)."""
        if self._x3_table is None:
            return self.x3_acc_scale
        row = _row_of(self._x3_table, self._blob_off(w), w.numel())
        if row is None:
            raise RuntimeError("weight view does not lie inside one tensor of the x3 blob")
        return row[2]

    # ------------------------------------------------------------------ keep_conv2d
    def conv(self, x, w, bias=None, *, stride=1, pad=1, ksize=3, down=False, upsample=False, pro=None, pro_act=L.PRO_NONE,
             act=L.ACT_NONE, residual=None, aux=None, aux_w=1.0, cin=None, in_off=0, out=None, split_k=None, wb=None,
             wx3=None, x3_acc_scale=None, mma=None, stats=False, out_bf16=False, bounded=False, x_amax=None, x2=None,
             reflect=False, out_ld=None, ln=None, out_hw=None, split_cols=None):
        """x [N,H,W,ld] -> [N,Ho,Wo,Cout].  ``w`` packed [Cout,KH,KW,Cin].  ``cin``/``in_off`` select a channel
        slice of a wider input buffer.  ``down`` = VQGAN Downsample geometry (pad right/bottom only, stride 2).
        ``stats=True`` returns ``(out, st)``: ``st`` is a ``Stats`` (epilogue-reduced GroupNorm partials and, under the x3
        policy, the per-image max |out|), or None when this launch could emit neither (split-K).  ``x_amax``: the
        producer's ``Stats.amax`` of x (any upper bound of max |x| per image works), replacing the range probe.
        ``bounded=True``: the caller vouches that |x| stays far below the fp16 range (normalised / attention-averaged
        inputs); otherwise an x3 launch without a normalising prologue first probes the input range (keep_absmax).
        ``x3_acc_scale`` belongs to the caller's ``wx3``: a call that leaves the weight operand to this Ops takes the scale of the twin it runs
        on (the x1 twin's own table where 'f16' routes it to L.MMA_X1).
        ``ln=(gamma, beta, eps)``: LayerNorm over the output channels in the epilogue, BEFORE the residual is added (x3 GEMM form,
        Cout == 128, rows % 128 == 0: ``ln_fusable``); the library refuses anything else.
        ``split_cols=(c0, c1)``: output columns c0 .. c1 are written as the split-fp16 halves ``attention(kv_split=True)`` reads
        (keep_conv2d_split: x3 GEMM form); the library refuses anything else."""
        # -- geometry
        N, H, W, ld = x.shape
        Cout = w.shape[0]
        Cin = ld if cin is None else cin
        if x2 is not None:          # K-concatenated second input (x3 GEMM form, keep_conv2d in2): channels ld.. come from x2
            assert bounded and pro is None and cin is None and in_off == 0, 'x2 needs a bounded, unsliced, prologue-free input'
            Cin = ld + x2.shape[-1]
        KH = KW = ksize
        assert w.numel() == Cout * KH * KW * Cin, (w.shape, Cout, KH, KW, Cin)
        Hv, Wv = (2 * H, 2 * W) if upsample else (H, W)
        if down:
            stride, pad_t, pad_l = 2, 0, 0
            Ho, Wo = Hv // 2, Wv // 2
        else:
            pad_t = pad_l = pad
            Ho = (Hv + 2 * pad - KH) // stride + 1
            Wo = (Wv + 2 * pad - KW) // stride + 1
        if out_hw is not None:      # fewer output rows / columns than the symmetric padding gives (an even kernel: pad only top / left)
            assert out_hw[0] <= Ho and out_hw[1] <= Wo
            Ho, Wo = out_hw
        M = N * Ho * Wo
        # -- operands and policy
        mma = self.mma if mma is None else mma
        in_dtype = L.BF16 if x.dtype == torch.bfloat16 else L.F32
        if mma == L.MMA_BF16 and wb is None and self.blob16 is not None:
            wb = self.bf16_twin(w)      # (without a twin the library still accepts the exact-fp32 Cout <= 4 kernel)
        up_mode = L.UPSAMPLE_X2_PHASES if upsample == L.UPSAMPLE_X2_PHASES and upsample is not True else int(bool(upsample))   # (explicit 2: the caller brings phase weights)
        own_up2 = False              # the phase weights are this Ops' own (up2_twin of ``w``): what ``up2_x1`` may replace by the phase x1 twin
        if (upsample and mma == L.MMA_X3 and wx3 is None and UP2_PHASES and KH == 3 and stride == 1 and pad == 1 and not down
                and pro is None and pro_act == L.PRO_NONE and act == L.ACT_NONE and aux is None and x2 is None and not reflect
                and split_k in (None, 1) and H % 8 == 0 and W % 32 == 0 and Cin % 16 == 0 and Cout % 64 == 0 and in_dtype == L.F32
                and not out_bf16 and self.x3_twin(w) is not None):
            # nearest x2 + 3x3 as four 2x2-tap phase convolutions on the source grid: 4 of 9 taps are multiplied
            wx3, x3_acc_scale = self.up2_twin(w)
            up_mode = L.UPSAMPLE_X2_PHASES
            own_up2 = True
        own_w = wx3 is None          # the weight operand is this Ops' to choose (not a caller's tensor -- the phase weights of an Upsample): what 'f16' may replace by the x1 twin
        if mma == L.MMA_X3 and wx3 is None:
            wx3 = self.x3_twin(w)
            if wx3 is not None and x3_acc_scale is None:
                x3_acc_scale = self.x3_scale_of(w)
        if x3_acc_scale is None:
            x3_acc_scale = self.x3_acc_scale
        want_bf16_out = bool(out_bf16) and mma == L.MMA_BF16 and residual is None
        xin = x if in_off == 0 else x.view(-1)[in_off:]

        def in_range():      # per-image max |x|: the producer's, or one keep_absmax probe
            return x_amax if (x_amax is not None and x_amax.numel() == N) else absmax(xin, N, H * W, Cin, ld, H * W * ld, self)
        probes = pro is None and not bounded      # (a normalising prologue / a vouched-for input needs no range)
        in_amax = None
        if ((mma == L.MMA_X3 and (wx3 is not None or (Cin <= 3 and KH == 3))) or mma == L.MMA_X1) and probes:   # (RGB convs split fp32 weights in-kernel)
            in_amax = in_range()
        out_ld = (Cout if out is None else out.shape[-1]) if out_ld is None else out_ld
        # -- plan: re-derived (``planned``) after the bf16 pre-normalisation, the single-fp16 swap and a refused bf16 output
        sk_req = 0 if split_k is None else int(split_k)
        odt = L.BF16 if want_bf16_out else L.F32
        pol = (mma, wx3, float(x3_acc_scale), self.flags)      # what the call launches under: (policy, weight_x3, x3_acc_scale, flags)

        def planned(p=None):
            """(arguments, Plan, plan key) of the call as these locals stand NOW, under ``p`` (default: ``pol``)."""
            mma, wx3, acc_scale, flags = p or pol
            a = L.conv_args(
                inp=xin, weight=w, bias=bias, out=out, pro_scale=None if pro is None else pro[0],
                pro_shift=None if pro is None else pro[1], residual=residual, aux=aux, workspace=None,
                N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad_t=pad_t, pad_l=pad_l, Ho=Ho, Wo=Wo,
                in_ld=ld, out_ld=out_ld, res_ld=0 if residual is None else residual.shape[-1],
                upsample=up_mode, pro_act=pro_act, epi_act=act, aux_w=float(aux_w), split_k=sk_req, dtype=in_dtype,
                mma=mma, weight_bf16=wb if mma == L.MMA_BF16 else None, stats_out=None, stats_P=0,
                bk256=int(USE_BK256), out_dtype=odt, weight_x3=wx3 if mma in (L.MMA_X3, L.MMA_X1) else None,
                x3_acc_scale=acc_scale, x3_in_amax=in_amax, x3_out_amax=None,
                in2=x2, in2_cin1=0 if x2 is None else ld, pad_mode=L.PAD_REFLECT if reflect else L.PAD_ZERO,
                ln_gamma=None if ln is None else ln[0], ln_beta=None if ln is None else ln[1],
                ln_eps=0.0 if ln is None else float(ln[2]), flags=flags, plan_ref_images=self.plan_ref_images)
            key = (N, H, W, ld, Cin, Cout, KH, stride, pad_t, pad_l, Ho, Wo, out_ld, up_mode, pro_act, act, in_dtype, mma,
                   odt, sk_req, pro is not None, residual is not None, 0 if residual is None else residual.shape[-1],
                   aux is not None, bias is not None, in_off % 8, wx3 is not None, USE_BK256, x2 is not None, bool(reflect),
                   ln is not None, flags, self.plan_ref_images, None if split_cols is None else tuple(split_cols))
            return a, _plan(a, key, split_cols), key

        a, pl, key = planned()
        if (pl.wants_bf16_input and in_off == 0 and Cin == ld and N * H * W >= HALO_PRENORM_MINPIX):
            # bf16 policy, 3x3 halo geometry with a prologue: normalise + activate once per element into a bf16 tensor
            x16 = torch.empty((N, H, W, ld), dtype=torch.bfloat16, device=x.device)
            L.call('keep_norm_act_bf16', x, None if pro is None else pro[0], None if pro is None else pro[1], x16,
                   N, H * W, ld, pro_act, in_dtype)
            x = xin = x16
            pro, pro_act, in_dtype = None, L.PRO_NONE, L.BF16
            a, pl, key = planned()
        # The call's ONE single-fp16 candidate (its routes, weight_x3, x3_acc_scale, flags to OR in); it runs single-fp16 iff the library plans it so
        # (_route).  ``up2_x1``: the hi-only phase twin, when the phase weights are this Ops' own -- it has whole 32-channel weight rows: a
        # depth that is no multiple of 32 has no twin (none is built here, possibly inside a capture, to be refused).  Otherwise 'f16': the
        # blob twin of ``w``, only where ``x1_base_kernel`` allows (KeepNet: the un-split x3 streaming 3x3 kernel, so the GEMM forms, the
        # split-K forms and im2col shapes stay x3 unasked).  The two exclude each other: an Ops-owned phase twin has set ``wx3``.
        cand = None
        if own_up2:
            if self.up2_x1 and Cin % 32 == 0:
                cand = (self._up2_x1_route, *self.up2_x1_twin(w), L.CONV_X1_UP2)
        elif (self.blobx1 is not None and own_w and mma == self.mma == self.x1_base and x2 is None
              and (self.x1_base_kernel is None or (pl.kernel == self.x1_base_kernel and pl.split_k == 1))):
            tw1 = self._x1_of(w)
            if tw1 is not None:
                cand = (self._x1_route, *tw1, self.x1_flags)
        if cand is not None:
            x1 = (L.MMA_X1, cand[1], cand[2], self.flags | cand[3])
            pl1 = self._route(cand[0], key, lambda: planned(x1)[1])
            if pl1:
                if in_amax is None and probes:      # (a base that reads no range -- exact f32 -- left the probe to this point)
                    in_amax = in_range()
                pol = x1
                a, pl = planned()[0], pl1
        if want_bf16_out and not pl.out_bf16_ok:
            want_bf16_out, odt = False, L.F32
            a, pl, key = planned()
        # -- launch
        if out is None:
            out = torch.empty((N, Ho, Wo, Cout), dtype=torch.bfloat16 if want_bf16_out else torch.float32, device=x.device)
            a.out = out.data_ptr()
        a.split_k = pl.split_k
        ws = empty((pl.ws_floats,), x) if pl.ws_floats else None
        if ws is not None:
            a.workspace = ws.data_ptr()
        st = None
        if stats and ((pl.stats_P and stats != 'amax') or pl.out_amax_ok):
            st = Stats()
            if pl.stats_P and stats != 'amax':      # ('amax': only the fused max|out| -- a GEMM whose consumer needs a range, not a GroupNorm)
                st.part, st.P = empty((N, pl.stats_P, Cout, 2), x), pl.stats_P
                a.stats_out, a.stats_P = st.part.data_ptr(), pl.stats_P
            if pl.out_amax_ok:
                st.amax, a.x3_out_amax_zeroed = self._amax_slots(N, x)
                a.x3_out_amax = st.amax.data_ptr()
        if self.profile is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            # algorithmic bytes: one read of the input window at its storage type, the weights, one write of the output
            alg_bytes = (N * H * W * Cin * x.element_size() + Cout * KH * KW * Cin * (2 if mma == L.MMA_BF16 else 4)
                         + M * Cout * out.element_size() + (0 if residual is None else M * Cout * 4))
            self.profile.append((pl.kernel, 2.0 * M * Cout * KH * KW * Cin, pl.split_k, e0, e1, alg_bytes,
                                 (N, H, W, Cin, Cout, KH, stride, int(upsample), pro is not None)))
            e0.record()
        if DEBUG_SYNC:      # dev aid: name every launch and wait for it, so a GPU fault is attributed to its kernel
            import sys
            print(f'[keep] {pl.kernel} N={N} H={H} W={W} ld={ld} Cin={Cin} Cout={Cout} k={KH} s={stride} up={int(upsample)} '
                  f'split={pl.split_k} in_off={in_off} pro={pro is not None}/{pro_act} act={act} res={residual is not None} '
                  f'aux={aux is not None} statsP={pl.stats_P if stats else 0}', file=sys.stderr, flush=True)
        if self.census is not None:
            self.census[pl.kernel] = self.census.get(pl.kernel, 0) + 1
        if split_cols is None:
            L.conv2d_launch(a)
        else:
            L.conv2d_split_launch(a, split_cols)
        if DEBUG_SYNC:
            torch.cuda.synchronize()
            if not bool(torch.isfinite(out.float()).all()):
                import sys
                print(f'[keep] NON-FINITE output of {pl.kernel}; input finite={bool(torch.isfinite(x.float()).all())} '
                      f'absmax={float(x.float().abs().max()):.4g} pro={None if pro is None else [float(t.abs().max()) for t in pro]} '
                      f'res absmax={None if residual is None else float(residual.abs().max())}', file=sys.stderr, flush=True)
        if self.profile is not None:
            self.profile[-1][4].record()
        return (out, st) if stats else out

    def linear(self, x, w, bias=None, *, act=L.ACT_NONE, residual=None, pro=None, pro_act=L.PRO_NONE, cin=None, in_off=0,
               n_img=None, out_bf16=False, bounded=False, x_amax=None, x2=None, ln=None, want_amax=False, split_cols=None):
        """x [M,ld] (or any [...,ld]) @ w[Cout,Cin]^T.  ``n_img``: the rows are n_img independent images (frames, clips) of
        M/n_img rows each -- the unit of the per-image prologue AND of the library's plan (kernel tile / split-K are chosen
        from the per-image row count, so a clip's result never depends on its batch-mates).  Default: the leading axis of a
        3-D+ input, 1 for a plain [M,ld] matrix (callers that flatten independent images into rows pass it).
        ``split_cols=(c0, c1)``: see ``conv`` -- the returned fp32 tensor holds fp16 halves in those columns, for ``attention(kv_split=True)`` alone."""
        shp = x.shape
        ld = shp[-1]
        M = x.numel() // ld
        if n_img is None:
            n_img = shp[0] if x.dim() >= 3 else 1
        assert M % n_img == 0, (tuple(shp), n_img)
        if (TOKEN_LINEAR and self.mma == L.MMA_BF16 and ld == 128 and w.shape[0] in (128, 256, 384) and w.shape[-1] == 128
                and M >= 65536 and act == L.ACT_NONE and residual is None and pro is None and pro_act == L.PRO_NONE and split_cols is None
                and cin is None and in_off == 0 and x.dtype == torch.float32 and x.is_contiguous()):
            return self.token_linear(x.view(M, ld), w.view(w.shape[0], 128), bias, out_bf16).reshape(*shp[:-1], w.shape[0])
        x4 = x.reshape(n_img, M // n_img, 1, ld)
        x24 = None if x2 is None else x2.reshape(n_img, M // n_img, 1, x2.shape[-1])
        res4 = None if residual is None else residual.reshape(n_img, M // n_img, 1, residual.shape[-1])
        y = self.conv(x4, w, bias, stride=1, pad=0, ksize=1, pro=pro, pro_act=pro_act, act=act, residual=res4, cin=cin,
                      in_off=in_off, out_bf16=out_bf16, bounded=bounded, x_amax=x_amax, x2=x24, ln=ln, stats='amax' if want_amax else False,
                      split_cols=split_cols)
        if want_amax:      # (y, per-image max |y| from the GEMM's epilogue, or None where the launch cannot emit it): the range probe of the consumer
            y, st = y
            return y.reshape(*shp[:-1], w.shape[0]), (None if st is None else st.amax)
        return y.reshape(*shp[:-1], w.shape[0])

    def ln_fusable(self, w, rows_per_image):
        """Can ``linear(x, w, ln=...)`` run its LayerNorm in the GEMM's epilogue?  (x3 policy with a split twin of ``w``, 128 output
        channels, K a multiple of 32, whole 128-row tiles per image -- a rule that never looks at the batch.)"""
        return (FUSE_LN and self.mma == L.MMA_X3 and w.shape[0] == 128 and w.shape[-1] % 32 == 0 and rows_per_image % 128 == 0
                and self.x3_twin(w) is not None)

    # ------------------------------------------------------------------ normalisation
    @staticmethod
    def norm_affine(x, gamma, beta, groups, eps, stats=None):
        """GroupNorm / InstanceNorm statistics of x [N,H,W,C] -> (scale, shift) [N,C] for a conv prologue.
        groups == C and gamma=None -> InstanceNorm2d(affine=False).  ``stats``: the (partials, P) the producing
        convolution reduced in its epilogue (saves one full read of x)."""
        N, H, W, C = x.shape
        HW = H * W
        scale = empty((N, C), x)
        shift = empty((N, C), x)
        if stats is not None and stats.part is not None:
            L.call('keep_norm_finalize', stats.part, gamma, beta, scale, shift, N, HW, C, groups, stats.P, float(eps))
            return scale, shift
        assert x.dtype == torch.float32, "bf16 activations carry their statistics from the producing conv's epilogue"
        cpg = C // groups
        if ((cpg % 4 == 0 and HW * cpg <= 32768) or HW <= 1024) and C % 4 == 0 and groups >= 2:   # (per-image rule: never N)
            # small maps: one block per (image, group), one launch
            L.call('keep_group_stats', x, gamma, beta, scale, shift, N, HW, C, groups, float(eps))
            return scale, shift
        P = max(1, min(HW // 64, 1024))
        part = empty((N, P, C, 2), x)
        L.call('keep_chan_stats', x, part, N, HW, C, C, P)
        L.call('keep_norm_finalize', part, gamma, beta, scale, shift, N, HW, C, groups, P, float(eps))
        return scale, shift

    @staticmethod
    def layernorm(x, gamma, beta, *, res=None, pos=None, eps=1e-5):
        """LN over the last dim.  Returns y (+res); with ``pos`` ([P,C], broadcast over rows mod P) also y+pos."""
        C = x.shape[-1]
        M = x.numel() // C
        out = torch.empty_like(x)
        out2 = torch.empty_like(x) if pos is not None else None
        L.call('keep_layernorm', x, gamma, beta, res, out, pos, 0 if pos is None else pos.shape[0], out2, M, C, float(eps))
        return out if pos is None else (out, out2)

    @staticmethod
    def geglu(x):
        F = x.shape[-1] // 2
        M = x.numel() // (2 * F)
        out = empty((*x.shape[:-1], F), x)
        L.call('keep_geglu', x, out, M, F)
        return out

    def _amax_slots(self, N, like):
        """N result words for a fused max|out|: from the per-forward arena (zeroed once in begin_forward) when it has room."""
        if self.amax_arena is not None and self.amax_pos + N <= self.amax_arena.numel():
            out = self.amax_arena[self.amax_pos:self.amax_pos + N]
            self.amax_pos += N
            return out, 1
        return torch.empty((N,), dtype=torch.float32, device=like.device), 0

    def layernorm_amax(self, x, gamma, beta, *, n_img, res=None, eps=1e-5):
        """``layernorm`` (+res) and the per-image max |out| of the result in one launch: (y, amax [n_img]) -- the x3 range scale of the
        GEMM that reads y (bit-identical y; amax == ``absmax(y)``)."""
        C = x.shape[-1]
        M = x.numel() // C
        out = torch.empty_like(x)
        am, zeroed = self._amax_slots(n_img, x)
        L.call('keep_layernorm_amax', x, gamma, beta, res, out, M, C, float(eps), M // n_img, am, zeroed)
        return out, am

    def geglu_amax(self, x, *, n_img):
        """``geglu`` and the per-image max |out|: (y, amax [n_img])."""
        F = x.shape[-1] // 2
        M = x.numel() // (2 * F)
        out = empty((*x.shape[:-1], F), x)
        am, zeroed = self._amax_slots(n_img, x)
        L.call('keep_geglu_amax', x, out, n_img, M // n_img, F, am, zeroed)
        return out, am

    # ------------------------------------------------------------------ keep_attention
    def attention(self, q, k, v, o, *, B, H, Lq, Lk, D, Dv, scale, q_str, k_str, v_str, o_str, mode=0, T=0, seg_len=0,
                  img_h=0, img_w=0, ksplit=0, shift=0, kv_rot=0, n_img=0, mma=None, probe=False, amax=None, kv_split=False):
        """Strides are (batch, token, head) element strides.  ``probe=True`` (x3 policy, mode 0): q / k / v are projections
        of an un-normalised tensor -- their ranges are probed and the kernel rescales them into the fp16 window.
        ``kv_split=True``: k / v are slices of a ``linear(split_cols=...)`` output (``kv_split_ok`` said so); the library refuses what its
        pre-split form does not cover."""
        mma = self.attn_mma if mma is None else mma
        in_dtype = L.F32
        if q.dtype == torch.bfloat16:
            assert k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16
            in_dtype, mma = L.BF16, L.MMA_BF16
        elif mma != L.MMA_F32 and (D % 16 or any(s % 4 for s in (*q_str, *k_str))):
            mma = L.MMA_F32
        given = amax
        amax = (None, None, None)
        if given is not None and all(t is not None and t.numel() == B for t in given) and mma == L.MMA_X3 and mode == 0 and in_dtype == L.F32:
            amax = tuple(given)      # per-batch upper bounds of max |q|, |k|, |v| the caller already holds (producers' fused maxima)
        elif probe and mma == L.MMA_X3 and mode == 0 and in_dtype == L.F32:
            # rows of batch b: tokens x (H heads x D) starting at b*bs; heads are contiguous slices of one row here
            amax = (absmax(q, B, Lq, H * D, q_str[1], q_str[0], self), absmax(k, B, Lk, H * D, k_str[1], k_str[0], self),
                    absmax(v, B, Lk, H * Dv, v_str[1], v_str[0], self))
        if DEBUG_SYNC:
            import sys
            print(f'[keep] attention mma={mma} in_dtype={in_dtype} B={B} H={H} Lq={Lq} Lk={Lk} D={D} Dv={Dv} mode={mode}',
                  file=sys.stderr, flush=True)
        kw = dict(q=q, k=k, v=v, o=o,
                  q_bs=q_str[0], q_ts=q_str[1], q_hs=q_str[2], k_bs=k_str[0], k_ts=k_str[1], k_hs=k_str[2],
                  v_bs=v_str[0], v_ts=v_str[1], v_hs=v_str[2], o_bs=o_str[0], o_ts=o_str[1], o_hs=o_str[2],
                  B=B, H=H, Lq=Lq, Lk=Lk, D=D, Dv=Dv, scale=float(scale), mode=mode, T=T, seg_len=seg_len,
                  img_h=img_h, img_w=img_w, ksplit=ksplit, shift=shift, kv_rot=kv_rot, n_img=n_img, mma=mma,
                  in_dtype=in_dtype, q_amax=amax[0], k_amax=amax[1], v_amax=amax[2], flags=self.attn_flags)
        if kv_split:
            kw.update(kv_split=True)
        elif self.attn_x1 and mma == self.attn_mma == L.MMA_X3 and in_dtype == L.F32:
            key = (H, Lq, Lk, D, Dv, mode, ksplit, img_h, img_w, shift, tuple(s % 4 for s in (*q_str, *k_str, *v_str)),
                   tuple(t.data_ptr() % 16 for t in (q, k, v)), amax[0] is not None, self.attn_flags)
            if self._route(self._attn_x1_route, key, lambda: L.attention_x1_plan(**kw) is not None):      # single fp16 where the library admits it, x3 otherwise
                kw.update(mma=L.MMA_X1, flags=self.attn_flags | L.ATTN_X1)
        L.attention(**kw)
        if DEBUG_SYNC:
            torch.cuda.synchronize()
            if not bool(torch.isfinite(o).all()):
                import sys
                print(f'[keep] NON-FINITE attention output; q/k/v absmax {float(q.float().abs().max()):.4g} '
                      f'{float(k.float().abs().max()):.4g} {float(v.float().abs().max()):.4g}', file=sys.stderr, flush=True)
        return o

    def kv_split_ok(self, *, B, Lq, Lk, D, Dv, q_str, k_str, v_str, img_h, img_w, ksplit, shift, n_img, gemm=None):
        """Does the library take this window-attention call (H = 1, fp32 tensors, 16-byte aligned bases) with ``kv_split`` -- and the projection
        that feeds it, ``gemm = (rows per image, Cin, Cout, split_cols)`` of a bias-free ``linear(split_cols=...)`` on aligned tensors, with the
        split output?  The library's own answers (keep_attention_kv_split_plan, keep_conv2d_split_plan), asked once per shape; never under the
        single-fp16 attention policy, which keeps the pack path."""
        if not ATTN_PRESPLIT or self.attn_x1 or self.attn_mma != L.MMA_X3:
            return False
        key = (Lq, Lk, D, Dv, tuple(q_str), tuple(k_str), tuple(v_str), img_h, img_w, ksplit, shift, self.attn_flags,
               None if gemm is None else (tuple(gemm[:3]), tuple(gemm[3]), self.mma, self.flags, self.plan_ref_images, USE_BK256))

        def query():
            a = L.attn_args(q=0x10000, k=0x10000, v=0x10000, o=0x10000, q_bs=q_str[0], q_ts=q_str[1], q_hs=q_str[2], k_bs=k_str[0], k_ts=k_str[1],
                            k_hs=k_str[2], v_bs=v_str[0], v_ts=v_str[1], v_hs=v_str[2], o_bs=Lq * ksplit * ksplit * Dv, o_ts=Dv, o_hs=0, B=B, H=1,
                            Lq=Lq, Lk=Lk, D=D, Dv=Dv, scale=1.0, mode=2, img_h=img_h, img_w=img_w, ksplit=ksplit, shift=shift, kv_rot=0,
                            n_img=n_img, mma=L.MMA_X3, in_dtype=L.F32, flags=self.attn_flags)
            L.attention_plan(a, kv_split=True)
            if gemm is not None:      # (one image stands for any number: the form follows the reference batch, the row rule holds per image)
                rows, cin, cout, cols = gemm
                g = L.conv_args(inp=0x10000, weight=0x10000, out=0x10000, weight_x3=0x10000, x3_acc_scale=1.0, N=1, H=rows, W=1, Cin=cin, Cout=cout,
                                KH=1, KW=1, stride=1, Ho=rows, Wo=1, in_ld=cin, out_ld=cout, mma=self.mma, dtype=L.F32, out_dtype=L.F32,
                                bk256=int(USE_BK256), flags=self.flags, plan_ref_images=self.plan_ref_images)
                L.conv2d_split_plan(g, cols)
            return True
        return self._route(self._kv_split_route, key, query)

    def token_linear(self, x, w, bias=None, out_bf16=False):
        """Streaming GEMM for the GMFlow projections (bf16 policy): x [M,128] fp32 @ w[N,128]^T, N in {128,256,384}."""
        K = x.shape[-1]
        M = x.numel() // K
        N = w.shape[0]
        out = torch.empty((M, N), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
        L.call('keep_token_linear', x, self.bf16_twin(w), bias, out, M, K, N, L.BF16 if out_bf16 else L.F32)
        return out

    def gm_mlp(self, a, b, w0, w2):
        """GMFlow FFN fused (bf16 policy): W2 . gelu(W0 . cat[a | b]); a, b [M,C] fp32, w0 [8C,2C], w2 [C,8C] fp32 views of
        the packed blob (their bf16 twins are used)."""
        C = a.shape[-1]
        M = a.numel() // C
        out = empty((M, C), a)
        L.call('keep_gm_mlp', a, b, self.bf16_twin(w0), self.bf16_twin(w2), out, M, C)
        return out


def absmax(x, N, R, C, ld, img_stride, ops=None):
    """Range probe: max |x| per image over R rows x C columns (row stride ld, image stride img_stride) -> [N] floats.
    ``ops``: take the result slots from that Ops' per-forward arena (already zero: no zero-fill launch)."""
    out, zeroed = (empty((N,), x), 0) if ops is None else ops._amax_slots(N, x)
    L.call('keep_absmax', x, out, N, R, C, ld, img_stride, zeroed)
    return out


def concat2(a, b, pad_to=1):
    """cat([a, b], -1); ``pad_to``: zero-pad the channel count up to a multiple (a 130-channel conv input becomes 144 wide so
    that the 16-channel-chunk MFMA kernels take it; the weights carry matching zero columns, engine/weights.py)."""
    C1, C2 = a.shape[-1], b.shape[-1]
    M = a.numel() // C1
    ld = (C1 + C2 + pad_to - 1) // pad_to * pad_to
    out = empty((*a.shape[:-1], ld), a)
    L.call('keep_concat2', a, b, out, M, C1, C2, ld)
    return out


def add_bcast(a, t, alpha=1.0):
    out = torch.empty_like(a)
    L.call('keep_add_bcast', a, t, out, a.numel(), t.numel(), float(alpha))
    return out


def nchw_to_nhwc(x, mode=0):
    N, C, H, W = x.shape
    out = empty((N, H, W, C), x)
    L.call('keep_nchw_to_nhwc', x, out, N, C, H * W, mode)
    return out


def rgb_s2d(x):
    """[N,3,H,W] in [-1,1] -> [N,H/2,W/2,16]: GMFlow's input normalisation + 2x2 space-to-depth (keep_rgb_s2d)."""
    N, C, H, W = x.shape
    assert C == 3 and H % 2 == 0 and W % 2 == 0
    out = empty((N, H // 2, W // 2, 16), x)
    L.call('keep_rgb_s2d', x, out, N, H, W)
    return out


def nhwc_to_nchw(x):
    N, H, W, C = x.shape
    out = empty((N, C, H, W), x)
    L.call('keep_nhwc_to_nchw', x, out, N, C, H * W)
    return out


def split_x3(w2d, scale):
    """[rows, Cin] fp32 (Cin % 16 == 0) -> int16 [rows, Cin/16, 2, 16]: fp16 bit patterns of hi = fp16(w*scale) and
    lo = fp16(w*scale - hi) per 16-channel chunk -- the `weight_x3` layout of keep_conv2d (csrc/keep_conv_x3.hip)."""
    rows, cin = w2d.shape
    ws = w2d.float() * scale
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    out = torch.stack((hi.view(rows, cin // 16, 16), lo.view(rows, cin // 16, 16)), dim=2)
    return out.contiguous().view(torch.int16)


FFN_W2_PERM = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def ffn_w2_perm(w2):
    """[C, hidden] -> the same matrix with every group of 16 hidden units reordered [0-3, 8-11, 4-7, 12-15]: the order in which the
    accumulator layout of v_mfma_f32_32x32x16_f16 hands a lane (half g) its hidden units {4g + (r & 3) + 8 (r >> 2)} -- the K order of
    the second product inside keep_gm_ffn_x3 (csrc/keep_ffn_x3.hip)."""
    C, Hd = w2.shape
    idx = torch.tensor(FFN_W2_PERM, device=w2.device)
    return w2.float().view(C, Hd // 16, 16).index_select(2, idx).reshape(C, Hd).contiguous()


def up2_phase_weights(w):
    """Packed [Cout,3,3,Cin] fp32 -> [4,Cout,3,3,Cin]: the 3x3 kernel of `nearest x2 -> conv3x3(pad 1)` (VQ:146-156) as four phase
    kernels on the SOURCE grid.  Output pixel (2y+py, 2x+px) reads upsampled rows 2y+py-1 .. 2y+py+1 = source rows (y-1, y, y) for
    py = 0 and (y, y, y+1) for py = 1: taps that meet the same source pixel are added (fp32), the freed taps are zero -- phase
    (py, px) keeps taps kh in {py, py+1}, kw in {px, px+1} of a 3x3 window centred on source pixel (y, x)."""
    r = torch.zeros(2, 3, 3, dtype=w.dtype, device=w.device)          # r[p][new][old]
    r[0, 0, 0] = 1; r[0, 1, 1] = 1; r[0, 1, 2] = 1                     # phase 0: new0 = old0, new1 = old1 + old2
    r[1, 1, 0] = 1; r[1, 1, 1] = 1; r[1, 2, 2] = 1                     # phase 1: new1 = old0 + old1, new2 = old2
    w4 = torch.einsum('pak,qbl,oklc->pqoabc', r, r, w.float())
    return w4.reshape(4, w.shape[0], 3, 3, w.shape[3]).contiguous()


def make_x3_blob(dev_blob, index, weights, names):
    """Split-fp16 twin of the tensors ``names`` of a packed fp32 blob (``index``: name -> (element offset, shape); ``weights``:
    name -> device view) with ONE POWER-OF-TWO SCALE PER TENSOR: each tensor's largest |w| lands just below 2^15, so a tensor of
    small weights keeps normal `lo` halves whatever the largest weight elsewhere in the net is (one shared scale -- rounds 2 / 3 --
    let a single large tensor push every other layer's `lo` halves towards the fp16 subnormals).  Returns (int16 blob with two
    elements per weight, [(first element, one past the last, accumulator scale 2^-e), ...] sorted by offset) for
    ``Ops.set_precision(..., x3_scales=)``."""
    bx = torch.zeros(2 * dev_blob.numel(), dtype=torch.int16, device=dev_blob.device)
    table = []
    for n in names:
        off, shape = index[n]
        t = weights[n]
        sc = x3_scale_for(float(t.abs().max()))
        bx[2 * off:2 * (off + t.numel())] = split_x3(t.reshape(-1, shape[-1]), sc).view(-1)
        table.append((int(off), int(off + t.numel()), 1.0 / sc))
    table.sort()
    return bx, table


def make_x1_blob(dev_blob, index, weights, names):
    """Hi-only fp16 twin of the tensors ``names`` for ``L.MMA_X1``: element i of the int16 result is the fp16 bit pattern of
    fp16(blob[i] * scale) -- ONE element per weight at the fp32 blob's own offsets, so a packed [Cout,KH,KW,Cin] tensor keeps its
    element order (the `weight_x3` layout of KEEP_MMA_X1, include/keep_hip.h) -- with ``make_x3_blob``'s power-of-two scale per
    tensor and the same (first element, one past the last, 2^-e) table."""
    bx = torch.zeros(dev_blob.numel(), dtype=torch.int16, device=dev_blob.device)
    table = []
    for n in names:
        off, shape = index[n]
        t = weights[n]
        sc = x3_scale_for(float(t.abs().max()))
        bx[off:off + t.numel()] = (t.reshape(-1).float() * sc).to(torch.float16).view(torch.int16)
        table.append((int(off), int(off + t.numel()), 1.0 / sc))
    table.sort()
    return bx, table


def x3_scale_for(max_abs):
    """Power of two that puts the largest weight just below 2^15 (fp16 max 65504), so that small weights keep a normal lo."""
    import math
    if not max_abs > 0:
        return 1.0
    return float(2.0 ** (14 - math.ceil(math.log2(max_abs))))


# default instance: fp32 policy, no blobs -- kernel tests pass mma= / wb= / wx3= explicitly
DEFAULT = Ops()
conv = DEFAULT.conv
linear = DEFAULT.linear
norm_affine = Ops.norm_affine
layernorm = Ops.layernorm
geglu = Ops.geglu
attention = DEFAULT.attention
token_linear = DEFAULT.token_linear
gm_mlp = DEFAULT.gm_mlp
