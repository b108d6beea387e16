"""What can keep_conv2d launch?  Two independent answers, both on the CPU:

* ``universe()``: the distinct strings ``keep_conv2d_launch_plan`` (include/keep_cv_hip.h, host C: the launch with the launches taken
  out) answers over a grid of argument structs wide enough to flip every condition the launchers read;
* ``census()``: the kernel instantiations that exist in the built library -- the host-side kernel handles of libkeep_hip.so's symbol
  table (read from the ELF file, demangled by the C++ runtime), restricted to the ``__global__`` names the convolution sources define.
  Names only; no kernel code is looked at.

tests/test_host_logic.py holds the two against each other and against the case table of tests/test_gpu_footprint.py.
"""
import ctypes
import itertools
import os
import re
import struct

from comfyui_keep_amd.engine import hiplib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'comfyui-keep_amd', 'csrc')
CONV_SOURCES = ('keep_conv.hip', 'keep_conv_x3.hip', 'keep_conv_x3s.hip', 'keep_conv_x3p.hip', 'keep_gemm_x3l.hip')
CONV_INCLUDES = ('keep_conv_common.h', 'keep_conv_up2s.inc')      # kernels the five sources take in by #include
FOLLOW_UPS = ('conv_splitk_reduce4_kernel', 'conv_splitk_reduce_kernel', 'conv_stats_replica_kernel', 'conv_x3_gather_stats_replica_kernel')
A = 0x10000                                                       # an aligned made-up address: no pointer is dereferenced


# ------------------------------------------------------------------------------------------------ census
def conv_kernel_names():
    """The ``__global__`` function names of the five convolution sources and what they include."""
    src = '\n'.join(open(os.path.join(CSRC, f)).read() for f in CONV_SOURCES + CONV_INCLUDES)
    names = set(re.findall(r'__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', src))
    for macro in [n for n in names if n.isupper()]:               # a kernel body included under several names (#define XU_KERNEL name)
        names.remove(macro)
        given = set(re.findall(r'#define\s+%s\s+(\w+)\s*$' % macro, src, re.M))
        assert given, macro
        names |= given
    return names


def launch_sites():
    """KEEP_CONV_LAUNCH uses per convolution source (a new arm of a launch macro changes the count)."""
    return {f: len(re.findall(r'\bKEEP_CONV_LAUNCH\(', open(os.path.join(CSRC, f)).read())) for f in CONV_SOURCES}


def _elf_object_symbols(path):
    """Names of the defined OBJECT symbols of an ELF64 little-endian file's .symtab (a HIP kernel's host-side handle is one)."""
    data = open(path, 'rb').read()
    assert data[:6] == b'\x7fELF\x02\x01', 'not an ELF64 little-endian file'
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3A)
    sections = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
    out = []
    for _, sh_type, _, _, off, size, link, _, _, entsize in sections:
        if sh_type != 2:                                           # SHT_SYMTAB
            continue
        str_off = sections[link][4]
        for i in range(size // entsize):
            st_name, st_info, _, st_shndx, _, _ = struct.unpack_from('<IBBHQQ', data, off + i * entsize)
            if st_info & 0xF == 1 and st_shndx != 0:               # STT_OBJECT, defined
                end = data.index(b'\0', str_off + st_name)
                out.append(data[str_off + st_name:end])
    return out


def _demangle(names):
    cxx = ctypes.CDLL('libstdc++.so.6')
    libc = ctypes.CDLL(None)
    cxx.__cxa_demangle.restype = ctypes.c_void_p
    cxx.__cxa_demangle.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    libc.free.argtypes = [ctypes.c_void_p]
    for n in names:
        status = ctypes.c_int()
        p = cxx.__cxa_demangle(n, None, None, ctypes.byref(status))
        if status.value == 0 and p:
            yield ctypes.string_at(p).decode()
            libc.free(p)


def instantiation(demangled):
    """'void k<1, true>(ConvP, int)' -> 'k<1, true>': the form keep_conv2d_launch_plan prints."""
    depth = 0
    for i, ch in enumerate(demangled):
        depth += (ch == '<') - (ch == '>')
        if ch == '(' and depth == 0:
            demangled = demangled[:i]
            break
    return demangled[5:] if demangled.startswith('void ') else demangled


def census(lib_path=None):
    """The convolution kernel instantiations present in the built library."""
    names = conv_kernel_names()
    mangled = [n for n in _elf_object_symbols(lib_path or L.LIB_PATH) if n.startswith(b'_Z')]
    found = {instantiation(d) for d in _demangle(mangled)}
    return {k for k in found if k.split('<')[0] in names}


# ------------------------------------------------------------------------------------------------ universe
ALL_FLAGS = (L.CONV_NO_COUT4, L.CONV_NO_C3, L.CONV_NO_HALO_F32, L.CONV_NO_HALO_X3, L.CONV_NO_GATHER_X3, L.CONV_NO_PLAIN, L.CONV_NO_FLATK_F32,
             L.CONV_SMALL_TILES, L.CONV_X3_EXACT_ACT, L.CONV_NO_STREAM, L.CONV_NO_GEMM_LAT, L.CONV_GEMM_LAT_WAVES, L.CONV_GEMM_LAT_TILES,
             L.CONV_NO_SMALL_PARTIALS)
LAUNCH_FLAGS = (0, L.CONV_NO_STREAM, L.CONV_NO_SMALL_PARTIALS, L.CONV_NO_GEMM_LAT, L.CONV_GEMM_LAT_TILES, L.CONV_GEMM_LAT_WAVES, L.CONV_X3_EXACT_ACT)
X1_BITS = (0, L.CONV_X1_HALO16, L.CONV_X1_UP2, L.CONV_X1_GEMM, L.CONV_X1_HALO16 | L.CONV_X1_UP2 | L.CONV_X1_GEMM)
# (mma, input dtype, output dtype, x1 opt-in bits)
POLICIES = [(L.MMA_F32, L.F32, L.F32, 0), (L.MMA_BF16, L.F32, L.F32, 0), (L.MMA_BF16, L.BF16, L.F32, 0), (L.MMA_BF16, L.F32, L.BF16, 0),
            (L.MMA_BF16, L.BF16, L.BF16, 0), (L.MMA_X3, L.F32, L.F32, 0)] + [(L.MMA_X1, L.F32, L.F32, b) for b in X1_BITS]
PROS = [(act, aff) for act in (L.PRO_NONE, L.PRO_SWISH, L.PRO_RELU) for aff in (0, 1)]
ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU02, L.ACT_GELU, L.ACT_SIGMOID, L.ACT_LRELU01, L.ACT_SILU)
EPILOGUES = ('none', 'res', 'res+aux')
CINS = (3, 16, 32, 48, 64, 96, 128, 256, 512, 1024, 2048)
COUTS = (3, 32, 48, 64, 96, 128)
MAPS = ((8, 32), (16, 16), (16, 64), (64, 64))
BIG = (1026, 1026)                                                  # stride 2: 513 x 513 = 263169 > 262144 output rows
ALIGNS = ('aligned', 'out_ld', 'pointers')
DEFAULTS = dict(policy=POLICIES[5], k=3, stride=1, hw=(8, 32), up=0, N=1, Cin=64, Cout=64, pro=(L.PRO_NONE, 0), act=L.ACT_NONE, epi='none',
                in2=0, ln=0, reflect=0, split=0, stats=0, amax=0, align='aligned', flags=0, bk256=0)


class Sweep:
    """Calls keep_conv2d_launch_plan on the points it is given; ``found``: launched string -> a point that gives it."""

    def __init__(self):
        self.lib = L.load(check_device=False)
        self.a, self.plan, self.out = L.ConvArgs(), L.ConvPlanOut(), L.ConvLaunchPlanOut()
        self.pa, self.pp, self.po = ctypes.byref(self.a), ctypes.byref(self.plan), ctypes.byref(self.out)
        self.found, self.points, self.refused = {}, 0, 0

    def point(self, policy, k, stride, hw, up, N, Cin, Cout, pro, act, epi, in2, ln, reflect, split, stats, amax, align, flags, bk256):
        a = self.a
        ctypes.memset(self.pa, 0, ctypes.sizeof(a))
        a.struct_size = ctypes.sizeof(a)
        mma, dt, odt, x1 = policy
        H, W = hw
        pad = k // 2
        Hv, Wv = (2 * H, 2 * W) if up else (H, W)
        a.mma, a.dtype, a.out_dtype, a.flags, a.bk256 = mma, dt, odt, flags | x1, bk256
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_t, a.pad_l = N, H, W, Cin, Cout, k, k, stride, pad, pad
        a.Ho, a.Wo = (Hv + 2 * pad - k) // stride + 1, (Wv + 2 * pad - k) // stride + 1
        a.upsample, a.pro_act, a.epi_act, a.aux_w, a.split_k = up, pro[0], act, 0.5, split
        a.pad_mode = L.PAD_REFLECT if reflect else L.PAD_ZERO
        off = 8 if align == 'pointers' else 0                      # every optional tensor 8 bytes off a 16-byte boundary
        a.inp = a.out = A + off
        a.weight = a.weight_bf16 = a.weight_x3 = A                 # (a misaligned weight pointer is refused by every form)
        a.bias = A + off
        a.x3_acc_scale = 1.0
        a.in_ld = a.in2_cin1 = 0
        a.in_ld, a.out_ld = Cin, Cout + (2 if align == 'out_ld' else 0)
        if pro[1]:
            a.pro_scale = a.pro_shift = A
        if epi != 'none':
            a.residual, a.res_ld = A + off, Cout
        if epi == 'res+aux':
            a.aux = A + off
        if in2:
            a.in2, a.in2_cin1, a.in_ld = A, 32, 32
        if ln:
            a.ln_gamma = a.ln_beta = A
            a.ln_eps = 1e-5
        if self.lib.keep_conv2d_plan(self.pa, self.pp) != 0:
            self.refused += 1
            return
        a.split_k = self.plan.split_k                              # the caller passes the plan's split-K and brings its workspace
        if self.plan.split_k > 1:
            a.workspace = A
        if stats:
            if not self.plan.stats_P:
                return
            a.stats_out, a.stats_P = A, self.plan.stats_P
        if amax:
            if not self.plan.out_amax_ok:
                return
            a.x3_out_amax, a.x3_out_amax_zeroed = A, 2 - amax      # amax = 2: not zeroed, the launch zeroes the slots first
        if self.lib.keep_conv2d_launch_plan(self.pa, self.po) != 0:
            self.refused += 1
            return
        self.points += 1
        s = self.out.kernels.decode()
        assert self.out.n_kernels == s.count(' + ') + 1, s
        if s not in self.found:
            self.found[s] = dict(policy=policy, k=k, stride=stride, hw=hw, up=up, N=N, Cin=Cin, Cout=Cout, pro=pro, act=act, epi=epi, in2=in2,
                                 ln=ln, reflect=reflect, split=split, stats=stats, amax=amax, align=align, flags=flags, bk256=bk256)

    def grid(self, **axes):
        """The full product of the given axes, every other axis at its default."""
        names = list(axes)
        base = dict(DEFAULTS)
        for values in itertools.product(*axes.values()):
            base.update(zip(names, values))
            self.point(**base)


X3_X1 = [p for p in POLICIES if p[0] in (L.MMA_X3, L.MMA_X1)]


def universe():
    """(launched string -> first point, admitted points, refused points).  The grid is the union of the products below: each takes in
    full the axes ONE launcher reads together, at every policy, and leaves the axes that launcher never reads at a default; the last
    product crosses every axis coarsely, as a net under the rest."""
    s = Sweep()
    some = [POLICIES[0], POLICIES[1], POLICIES[3], POLICIES[5], POLICIES[6], POLICIES[9], POLICIES[10]]      # f32, bf16 (out f32 / bf16), x3, x1 (0 / GEMM / all)
    aff_swish, aff_relu = (L.PRO_SWISH, 1), (L.PRO_RELU, 1)
    # 3x3 stride 1 -- the halo families (x3 / x1: x3_halo_run, the streaming kernel's PRO x AFF x X1 x EACT, TW / PRO / simple / fast of
    # the stage-barrier kernel; f32: TW x PRO; bf16: dtype x TW x simple, the v1 kernel)
    s.grid(policy=POLICIES, hw=((8, 32), (16, 16)), N=(1, 48), Cin=(32,), pro=PROS, act=ACTS, epi=EPILOGUES, reflect=(0, 1),
           flags=(0, L.CONV_X3_EXACT_ACT, L.CONV_NO_STREAM), split=(0, 2))
    s.grid(policy=POLICIES, hw=MAPS, up=(0, 1, L.UPSAMPLE_X2_PHASES), N=(1, 3, 48), Cin=(16, 32), pro=(DEFAULTS['pro'], aff_swish),
           act=(L.ACT_NONE, L.ACT_GELU), stats=(0, 1), amax=(0, 1, 2), flags=LAUNCH_FLAGS)
    # the 64-pixel blocks: chunk counts per split (NCH), prologue forms, what sends a launch there
    s.grid(policy=(POLICIES[5], POLICIES[6]), hw=MAPS, N=(1, 3, 48), Cin=CINS, Cout=(64, 96), pro=PROS, split=(0, 1, 2, 3, 4), epi=('none', 'res+aux'),
           stats=(0, 1), flags=(0, L.CONV_NO_SMALL_PARTIALS, L.CONV_NO_STREAM, L.CONV_X3_EXACT_ACT))
    # 1x1: GEMM forms (latency form, K slices by tiles or by waves, the tile and its shrink, statistics replica, the bf16 256-channel step)
    s.grid(policy=some, k=(1,), hw=MAPS + ((128, 128),), N=(1, 48), Cin=CINS, Cout=COUTS, pro=(DEFAULTS['pro'], aff_swish), split=(0, 2), stats=(0, 1),
           flags=LAUNCH_FLAGS + (L.CONV_SMALL_TILES, L.CONV_NO_PLAIN, L.CONV_NO_GATHER_X3))
    s.grid(policy=POLICIES[1:5], k=(1,), hw=MAPS, N=(1, 48), Cin=CINS, Cout=COUTS, split=(0, 2), bk256=(0, 1), flags=(0, L.CONV_NO_PLAIN))
    s.grid(policy=(POLICIES[0], POLICIES[1], POLICIES[5], POLICIES[10]), k=(1,), hw=MAPS, N=(1, 48), Cin=(64, 96, 512), Cout=(64, 128), in2=(0, 1), ln=(0, 1),
           epi=EPILOGUES, act=(L.ACT_NONE, L.ACT_GELU), align=ALIGNS, flags=LAUNCH_FLAGS)
    # im2col: k 3 / 7, stride 1 / 2, flattened K, the gather kernels' tiles and plain forms, the policy-independent small-channel kernels
    s.grid(policy=some, k=(3, 7), stride=(1, 2), hw=((8, 32), (5, 7), (64, 128)), up=(0, 1), N=(1, 48), Cin=(3, 16, 32, 48, 64, 256), Cout=(3, 32, 48, 64, 128),
           pro=(DEFAULTS['pro'], aff_relu), split=(0, 3),
           flags=(0, L.CONV_NO_PLAIN, L.CONV_SMALL_TILES, L.CONV_NO_HALO_X3, L.CONV_NO_HALO_F32, L.CONV_NO_GATHER_X3, L.CONV_NO_FLATK_F32, L.CONV_NO_COUT4, L.CONV_NO_C3))
    # ... and the one form that needs M > 262144 output rows
    s.grid(policy=POLICIES, stride=(1, 2), hw=(BIG,), Cin=(16, 32), Cout=(48, 64, 128), pro=(DEFAULTS['pro'], aff_relu), stats=(0, 1),
           flags=(0, L.CONV_NO_PLAIN, L.CONV_SMALL_TILES))
    # the net: every flag and alignment against every policy and kernel size, coarsely
    s.grid(policy=POLICIES, k=(1, 3, 7), stride=(1, 2), N=(1, 48), Cin=(3, 32, 512), Cout=(3, 64, 128), epi=('none', 'res+aux'), split=(0, 4), align=ALIGNS,
           flags=(0,) + ALL_FLAGS)
    return s.found, s.points, s.refused


def convolution(launched):
    """The convolution kernel of a launched string: without the zero-fill before it and the follow-up kernels behind it."""
    parts = [p for p in launched.split(' + ') if p != 'zero_u32_kernel' and p not in FOLLOW_UPS]
    assert len(parts) == 1, launched
    return parts[0]
