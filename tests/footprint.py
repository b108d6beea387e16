"""Memory-footprint harness: which bytes does a kernel touch?

Every tensor of a launch lives in an allocation of its own, ``[guard | payload | guard]``.  The payload keeps its real row
stride (``ld``) and channel offset, so the gap columns of a strided slice are *surroundings* like the guards.  One launch is
then judged three ways:

* **write check** -- the surroundings of every buffer are filled with a known bit pattern before the launch (``0x7FC0BEEF``, a
  quiet NaN no kernel produces, ``0xA5`` for uint8, or the read poison of the round) and compared bit for bit afterwards.  Any
  difference raises ``WriteOutside`` with the first offset relative to the payload.
* **read check** -- the launch is repeated with the surroundings of every buffer the kernel reads holding zeros, NaN and 3e38
  (``0x00`` / ``0xFF`` / ``0x7F`` for uint8, 0 / INT_MIN / INT_MAX for integers).  The outputs of the three runs must be
  bit-identical, and finite: a stray value that reaches a result -- also one that is "masked" by a multiplication with zero --
  raises ``ReadOutside``.
* **value check** -- the zero-poison output equals the plain call (exactly sized buffers, no guards) bit for bit.  Accuracy is
  the business of the value judges of the same cases (tests/test_gpu_case_values.py, tests/test_gpu_flat_values.py) and of the reference tests.

Guard size is a condition, not a measurement: at least ``GUARD_BYTES`` (64 KiB) and at least the ``tile_bytes`` a case states
for its kernel family (the largest block of memory one step of the kernel can touch).  Buffers whose size the library reports
(split-K workspace, statistics partials, amax slots) are declared at exactly that size, so the first byte behind them is guard.

What this cannot see: a stray read whose value is discarded by a select and that lands inside our own allocation is harmless
here and invisible here; it would only fault at the end of a real allocation.  This is not a sanitizer, and it must never be
used to go looking for a fault: every byte a kernel may touch, guards included, is memory the test owns.

The module is device-agnostic (``device='cpu'`` works: tests/test_host_logic.py runs it over two deliberately wrong torch
"kernels").
"""
import torch

GUARD_BYTES = 64 * 1024
BEEF = 0x7FC0BEEF                      # quiet NaN with a payload: written surroundings of float / int32 buffers
POISONS = ('zero', 'nan', 'big')

_INT_VIEW = {torch.float32: torch.int32, torch.int32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16,
             torch.int16: torch.int16, torch.uint8: torch.uint8, torch.float64: torch.int64, torch.int64: torch.int64}


class FootprintError(AssertionError):
    pass


class WriteOutside(FootprintError):
    pass


class ReadOutside(FootprintError):
    pass


class ValueMismatch(FootprintError):
    pass


def _pattern(dtype, kind):
    """The fill value (in the integer view of ``dtype``) of one kind of surroundings."""
    iv = _INT_VIEW[dtype]
    if kind == 'beef':
        return {torch.int32: BEEF, torch.int16: 0x7FCE, torch.uint8: 0xA5, torch.int64: 0x7FF8BEEFBEEFBEEF}[iv]
    if dtype.is_floating_point:
        v = {'zero': 0.0, 'nan': float('nan'), 'big': 3e38}[kind]
        return int(torch.tensor([v], dtype=dtype).view(iv)[0])
    info = torch.iinfo(dtype)
    if dtype == torch.uint8:
        return {'zero': 0x00, 'nan': 0xFF, 'big': 0x7F}[kind]
    return {'zero': 0, 'nan': info.min, 'big': info.max}[kind]


class Region:
    """One device allocation holding one or more payload windows of a row-strided buffer.

    ``rows`` rows of ``ld`` elements; window ``name`` covers columns ``[off, off + C)`` of every row.  ``role``: 'r' (only read),
    'w' (only written) or 'rw' (in place).  ``windows``: name -> (off, C, data) with ``data`` a tensor of ``rows * C`` elements
    (any shape) or None (an output: the payload starts as the BEEF pattern, so an element the kernel leaves unwritten shows up
    as non-finite).  Packed operands (q | k | v rows) are several windows of one region: each is surroundings to nobody, the
    columns outside all of them are.
    """

    def __init__(self, rows, ld, windows, dtype=torch.float32, role='r', tile_bytes=0, compare=True):
        assert role in ('r', 'w', 'rw')
        self.compare = compare          # False: scratch (split-K partials, packed K / V) -- footprint only, contents not an output
        self.rows, self.ld, self.dtype, self.role = int(rows), int(ld), dtype, role
        self.windows = {}
        for name, (off, C, data) in windows.items():
            assert 0 <= off and off + C <= ld, (name, off, C, ld)
            if data is not None:
                assert data.numel() == self.rows * C and data.dtype == dtype, (name, tuple(data.shape), data.dtype, rows, C)
            self.windows[name] = (int(off), int(C), data)
        self.item = torch.empty((), dtype=dtype).element_size()
        g = max(GUARD_BYTES, int(tile_bytes))
        self.guard = (g + 15) // 16 * 16 // self.item                 # elements; a multiple of 16 bytes keeps the alignment

    @property
    def first(self):
        return min(off for off, _, _ in self.windows.values())

    def build(self, device, embedded, poison):
        """Allocate and fill; returns (flat buffer, {name: [rows, C] strided view}, payload mask)."""
        g = self.guard if embedded else 0
        n = self.rows * self.ld
        iv = _INT_VIEW[self.dtype]
        flat = torch.empty(n + 2 * g, dtype=self.dtype, device=device)
        kind = 'beef' if self.role == 'w' else poison
        flat.view(iv).fill_(_pattern(self.dtype, kind) if embedded else 0)
        mask = torch.zeros(n + 2 * g, dtype=torch.bool, device=device)
        body = flat[g:g + n].view(self.rows, self.ld)
        mbody = mask[g:g + n].view(self.rows, self.ld)
        views = {}
        for name, (off, C, data) in self.windows.items():
            v = body[:, off:off + C]
            if data is not None:
                v.copy_(data.reshape(self.rows, C).to(device))
            else:
                v.view(iv).fill_(_pattern(self.dtype, 'beef'))
            mbody[:, off:off + C] = True
            views[name] = v
        return flat, views, mask


def single(name, data, role='r', ld=None, off=0, tile_bytes=0, C=None):
    """A region with one window: ``data`` [..., C] (rows = the leading dims) at column ``off`` of rows ``ld`` wide."""
    C = data.shape[-1] if C is None else C
    rows = data.numel() // C
    return Region(rows, C if ld is None else ld, {name: (off, C, data)}, data.dtype, role, tile_bytes)


def output(name, shape, dtype=torch.float32, ld=None, off=0, tile_bytes=0, init=None, compare=True):
    """A written region: ``shape`` [..., C]; ``init`` (a tensor) when the kernel legitimately leaves part of it unwritten."""
    C = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    if init is not None:
        assert init.numel() == rows * C
    return Region(rows, C if ld is None else ld, {name: (off, C, init)}, dtype, 'w', tile_bytes, compare)


def unaligned_u8(src, dst_bytes):
    """The regions 'src' and 'dst' of a uint8 launch whose two base pointers are not 16-byte aligned: ``src`` and the ``dst_bytes`` of the
    result as one row each, 5 and 11 bytes into a row that is 16 bytes longer (allocations, guards and exactly sized buffers all start on
    a multiple of 16).  The other 16 bytes of either row are surroundings like the guards."""
    src = src.reshape(1, -1)
    return [single('src', src, ld=src.numel() + 16, off=5), output('dst', (1, dst_bytes), torch.uint8, ld=dst_bytes + 16, off=11)]


def _first_diff(a, b):
    return int((a != b).nonzero()[0])


def _one_run(launch, regions, device, embedded, poison):
    built = [(r, *r.build(device, embedded, poison)) for r in regions]
    tensors = {}
    before = []
    for r, flat, views, mask in built:
        tensors.update(views)
        before.append(flat.view(_INT_VIEW[r.dtype])[~mask].clone() if embedded else None)
    sig = launch(tensors)
    sig = None if isinstance(sig, torch.Tensor) else sig          # (a torch in-place op used as the launch returns its tensor)
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()
    outs = {}
    for (r, flat, views, mask), was in zip(built, before):
        iv = _INT_VIEW[r.dtype]
        if embedded:
            now = flat.view(iv)[~mask]
            if not torch.equal(now, was):
                i = _first_diff(now, was)
                pos = int((~mask).nonzero()[i])                      # flat index of the first changed surrounding element
                rel = pos - (r.guard + r.first)
                raise WriteOutside(f"{'|'.join(r.windows)}: the launch changed memory outside the payload; first at element "
                                   f"{rel:+d} relative to the payload start (payload spans {r.rows} rows x ld {r.ld}, "
                                   f"poison {poison!r}): {int(was[i]):#x} -> {int(now[i]):#x}")
        if r.role != 'r' and r.compare:
            for name, v in views.items():
                outs[name] = v.contiguous().clone()
    return outs, sig


def plain(launch, regions, device):
    """One plain call -- exactly sized buffers, no guards, gap columns zero: (outputs name -> tensor, the launch's signature).  For
    the tests that judge values (tests/test_gpu_case_values.py); nothing about the footprint is checked."""
    names = [n for r in regions for n in r.windows]
    assert len(names) == len(set(names)), names
    return _one_run(launch, regions, device, False, 'zero')


def run(launch, regions, device, finite=True, canon=None):
    """``launch(tensors) -> signature``: the kernel call on the views in ``tensors`` (name -> [rows, C] view with row stride ld);
    the optional signature (e.g. the library's plan) must be the same for the plain and every embedded run.  Raises a
    ``FootprintError``; returns the outputs of the zero-poison run (name -> tensor).  ``canon``: maps the outputs of one run
    (name -> tensor) to the form that is compared -- for the few kernels whose ABI leaves an order open (rows appended in arrival
    order); everything else is compared as it is."""
    names = [n for r in regions for n in r.windows]
    assert len(names) == len(set(names)), names
    canon = canon or (lambda outs: outs)
    plain, sig0 = _one_run(launch, regions, device, False, 'zero')
    plain = canon(plain)
    got = {}
    for poison in POISONS:
        got[poison], sig = _one_run(launch, regions, device, True, poison)
        got[poison] = canon(got[poison])
        if sig != sig0:
            raise FootprintError(f"the embedded call was planned differently from the plain call: {sig!r} vs {sig0!r}")
    for name in plain:
        z = got['zero'][name]
        iv = _INT_VIEW[z.dtype]
        for poison in POISONS[1:]:
            o = got[poison][name]
            if not torch.equal(z.view(iv), o.view(iv)):
                i = _first_diff(z.view(iv).reshape(-1), o.view(iv).reshape(-1))
                raise ReadOutside(f"{name}: the result depends on memory outside the inputs' payloads: element {i} is "
                                  f"{z.reshape(-1)[i].item()!r} with zero surroundings and {o.reshape(-1)[i].item()!r} with "
                                  f"{poison!r} surroundings")
        if finite and z.dtype.is_floating_point and not bool(torch.isfinite(z.float()).all()):
            i = int((~torch.isfinite(z.float().reshape(-1))).nonzero()[0])
            raise ReadOutside(f"{name}: element {i} of the result is {z.reshape(-1)[i].item()!r} (an output the kernel left "
                              f"unwritten keeps its NaN fill)")
        if not torch.equal(z.view(iv), plain[name].view(iv)):
            i = _first_diff(z.view(iv).reshape(-1), plain[name].view(iv).reshape(-1))
            raise ValueMismatch(f"{name}: the embedded call differs from the plain call at element {i}: "
                                f"{z.reshape(-1)[i].item()!r} vs {plain[name].reshape(-1)[i].item()!r}")
    return got['zero']
