"""Lifecycle shared by the packed facelib engines (ParseNet, RetinaFace, YOLOv5-face): one packed fp32 blob on the host, ``to()`` uploads
it and activates the matrix-core policy, ``to('cpu')`` drops the device copies."""
import numpy as np
import torch

from . import hiplib as L
from . import ops
from .weights import views

# matrix-core policies of these engines: 'x3' split fp16 (fp32-grade, the default), 'fp32' exact f32, 'f16' operands rounded once to fp16
# (KEEP_MMA_X1 wherever the library's plan admits the call: an opt-in speed mode OUTSIDE bit-parity with the default -- DESIGN 4)
PRECISIONS = ('x3', 'fp32', 'f16')


class PackedEngine:
    """An engine supplies ``NET`` (its name in messages), ``x3_names()`` (the tensors that get a split-fp16 twin), the data of its 'f16'
    rule -- ``X1_BASE`` (the policy the twin rides on) and ``X1_RULE`` (``Ops.set_x1_twin``'s flags / base_kernel) -- and, where it keeps
    device state of its own, ``_uploaded()``."""
    PRECISIONS = PRECISIONS
    NET = 'engine'
    X1_BASE = L.MMA_X3
    X1_RULE = {}

    @classmethod
    def check_precision(cls, precision):
        if precision not in PRECISIONS:
            raise ValueError(f"{cls.NET} precision must be one of {PRECISIONS}, got {precision!r}")
        return precision

    def _init_packed(self, blob, index, precision):
        self._blob, self._index = blob, index
        self.precision = self.check_precision(precision)
        self.device = torch.device('cpu')
        self.w = self._dev = None
        self.o = ops.Ops()

    @classmethod
    def _rebuild(cls, blob, index, precision, **attrs):
        """The shared half of an engine's ``from_packed``: an instance around a packed blob that another process (or this one) made, with the
        attributes its constructor would have derived (``attrs``) -- no state dict, no folding, nothing uploaded yet."""
        self = cls.__new__(cls)
        for k, v in attrs.items():
            setattr(self, k, v)
        self._init_packed(np.ascontiguousarray(blob), index, precision)
        return self

    def x3_names(self):
        raise NotImplementedError

    def x1_names(self):
        """Tensors that get a hi-only twin: every matrix weight with whole 32-channel K steps (no x1 kernel takes another depth)."""
        return [n for n in self.x3_names() if self._index[n][1][-1] % 32 == 0]

    def _uploaded(self):
        """Hook: the weights moved (``self.w`` holds the new device views, or None after an offload)."""

    def to(self, device):
        device = torch.device(device)
        if device.type != 'cuda':
            self.w, self._dev = None, None
            self.o.set_precision(self.o.mma)        # drop the references to the device blobs
            self.device = device
            self._uploaded()
            return self
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        L.load(check_device=True)
        self.device = device
        self._dev = torch.from_numpy(self._blob).to(device)
        self.w = views(self._dev, self._index)
        self._uploaded()
        # the twins, then the base policy, then the x1 rule.  'f16' holds a hi-only twin beside its base's: a call runs single-fp16 wherever
        # the library's plan admits it and on the base everywhere else (a tensor without a twin -- the Cin = 3 convolutions -- always)
        base = {'x3': L.MMA_X3, 'fp32': L.MMA_F32, 'f16': self.X1_BASE}[self.precision]
        if base == L.MMA_X3:
            bx, table = ops.make_x3_blob(self._dev, self._index, self.w, self.x3_names())       # one power-of-two scale per tensor
            self.o.set_precision(L.MMA_X3, self._dev, None, bx, 1.0, x3_scales=table)
        else:
            self.o.set_precision(base, self._dev, None)
        if self.precision == 'f16':
            b1, t1 = ops.make_x1_blob(self._dev, self._index, self.w, self.x1_names())
            self.o.set_x1_twin(b1, t1, base=base, **self.X1_RULE)
        return self
