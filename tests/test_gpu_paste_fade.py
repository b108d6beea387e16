"""GPU suite (-m gpu): keep_paste_face_w (csrc/keep_paste.hip, include/keep_cv_hip.h) -- the paste-back composite with an opacity per
face -- against keep_paste_face and against the numpy restatement tests/paste_fade_ref.py, BIT FOR BIT: the opacity adds one float32
product, rounded on its own on both sides, so the bound is 0.

The case (paste_fade_ref.small_case): a 200 x 300 frame, two 512 x 512 faces mapped to boxes of about 90 px, the second cut by the frame's
right and lower edge; both mask forms -- the blurred parse mask sampled in face space, and the frame-space erosion mask
(``mask_border`` < 0)."""
import ctypes as C

import numpy as np
import pytest
import torch

import paste_fade_ref as FR
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import paste

pytestmark = pytest.mark.gpu

CORE, W = 'keep_paste_face', 'keep_paste_face_w'
FORMS = ['parse-mask', 'frame-mask']


class Case:
    """The inputs on the device, the kernel's masks in both forms and the restatement's frame-space soft masks, computed once."""

    def __init__(self):
        self.frame, self.faces, self.mats, self.classes = FR.small_case()
        self.H, self.W = self.frame.shape[:2]
        self.gp = paste.GpuPaster('cuda')
        self.faces_dev = torch.from_numpy(self.faces).cuda()
        self.frame_f32 = torch.from_numpy(self.frame.astype(np.float32)).cuda()
        self.d2s = [(C.c_double * 6)(*paste.invert_affine(M).reshape(-1).tolist()) for M in self.mats]
        self.boxes = [paste.face_box(M, 512, 512, self.W, self.H) for M in self.mats]
        assert self.boxes[1][2] == self.W and self.boxes[1][3] == self.H and self.boxes[0][2] < self.W    # the second face is cut by the edge
        self.masks = {'parse-mask': list(self.gp.soft_masks(torch.from_numpy(self.classes).cuda())),
                      'frame-mask': [self.gp.erosion_mask(d, self.H, self.W, 512, 512, 1.0) for d in self.d2s]}
        assert all(m is not None for m in self.masks['frame-mask'])
        self.soft = {'parse-mask': FR.frame_soft_masks(self.frame, list(self.faces), list(self.mats), list(self.classes)),
                     'frame-mask': FR.frame_soft_masks(self.frame, list(self.faces), list(self.mats), None)}

    def composite(self, form, opacities, entry=W):
        """The float frame behind both faces, blended by ``entry`` (opacities: per face; ignored by the core entry)."""
        acc = self.frame_f32.clone()
        border = paste.PARSE_BORDER if form == 'parse-mask' else -1
        for i in range(2):
            args = (acc, self.H, self.W, self.faces_dev[i], self.masks[form][i], 512, 512, self.d2s[i], *self.boxes[i], border)
            if entry == CORE:
                L.call(CORE, *args)
            else:
                L.call(W, *args, C.c_float(opacities[i]))
        torch.cuda.synchronize()
        return acc

    def ref(self, form, weights):
        cls = list(self.classes) if form == 'parse-mask' else None
        return torch.from_numpy(FR.composite_f32(self.frame, list(self.faces), list(self.mats), cls, weights=weights, soft=self.soft[form]))


@pytest.fixture(scope='module')
def case():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return Case()


@pytest.mark.parametrize('form', FORMS)
def test_opacity_one_is_the_core_entry(case, form):
    core = case.composite(form, None, entry=CORE)
    assert (core != case.frame_f32).any()                                            # (the faces really landed)
    assert torch.equal(case.composite(form, [1.0, 1.0]), core)
    assert torch.equal(core.cpu(), case.ref(form, [1.0, 1.0]))                       # ... and both are the restatement


@pytest.mark.parametrize('form', FORMS)
def test_opacity_zero_leaves_the_frame_bit_identical(case, form):
    assert torch.equal(case.composite(form, [0.0, 0.0]), case.frame_f32)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('opacity', [0.25, 0.5])
def test_opacity_equals_the_restatement(case, form, opacity):
    got = case.composite(form, [opacity, opacity]).cpu()
    ref = case.ref(form, [opacity, opacity])
    diff = (got - ref).abs()
    print(form, opacity, 'max abs difference', float(diff.max()), 'differing values', int((diff != 0).sum()))
    assert torch.equal(got, ref)
    assert not torch.equal(got, case.ref(form, [1.0, 1.0])) and not torch.equal(got, case.frame_f32.cpu())
    # mixed opacities, and one that is no power of two (1 / 3 as the fade computes it: float64 quotient cast to float32)
    third = float(np.float32(1.0 / 3.0))
    assert torch.equal(case.composite(form, [third, 1.0 - opacity]).cpu(), case.ref(form, [third, 1.0 - opacity]))


@pytest.mark.parametrize('form', FORMS)
def test_a_bad_opacity_is_refused_and_nothing_is_written(case, form):
    for bad in (-0.25, 1.5, float('nan'), float('inf')):
        acc = case.frame_f32.clone()
        border = paste.PARSE_BORDER if form == 'parse-mask' else -1
        with pytest.raises(L.KeepHipError) as e:
            L.call(W, acc, case.H, case.W, case.faces_dev[0], case.masks[form][0], 512, 512, case.d2s[0], *case.boxes[0], border, C.c_float(bad))
        assert e.value.code == L.EINVAL and W + ':' in str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(acc, case.frame_f32)


def test_paster_weights_equal_the_restatement_after_rounding(case, monkeypatch):
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    cls = torch.from_numpy(case.classes).cuda()
    got = case.gp.paste(case.frame, case.faces, list(case.mats), cls, weights=[1, 0.5])
    assert calls.count(CORE) == 1 and calls.count(W) == 1                            # a weight of 1.0 takes today's call
    ref = FR.paste_faces_weighted(case.frame, list(case.faces), list(case.mats), list(case.classes), weights=[1, 0.5], soft=case.soft['parse-mask'])
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref)
    # weights None / all 1.0: today's calls and today's frame
    calls.clear()
    plain = case.gp.paste(case.frame, case.faces, list(case.mats), cls)
    ones = case.gp.paste(case.frame, case.faces, list(case.mats), cls, weights=[1.0, 1.0])
    assert calls.count(CORE) == 4 and calls.count(W) == 0 and torch.equal(plain, ones) and not torch.equal(plain, got)
    # the erosion-mask form, a skipped face, and a wrong number of weights
    got = case.gp.paste(case.frame, case.faces, list(case.mats), None, 1.0, weights=[0.25, 0.5])
    ref = FR.paste_faces_weighted(case.frame, list(case.faces), list(case.mats), None, weights=[0.25, 0.5], soft=case.soft['frame-mask'])
    assert np.array_equal(got.cpu().numpy(), ref)
    got = case.gp.paste(case.frame, case.faces, [None, case.mats[1]], cls, weights=[0.25, 0.5])
    ref = FR.paste_faces_weighted(case.frame, list(case.faces), [None, case.mats[1]], list(case.classes), weights=[0.25, 0.5],
                                  soft=case.soft['parse-mask'])
    assert np.array_equal(got.cpu().numpy(), ref)
    with pytest.raises(ValueError):
        case.gp.paste(case.frame, case.faces, list(case.mats), cls, weights=[0.5])
