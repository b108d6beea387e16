"""GPU suite (-m gpu): keep_paste_face_aa (csrc/keep_paste.hip, include/keep_cv_hip.h) -- the alias-free paste-back composite, N x N
sub-samples per frame pixel -- and ``GpuPaster.paste(aa=True)`` against the numpy restatement tests/paste_aa_ref.py, BIT FOR BIT: every
sum is an integer sum and every float operation is rounded on its own on both sides, so the bound is 0.

The case: a 160 x 200 frame and three 512 x 512 faces, one per N, all rotated -- N = 2 (r = 0.55, hangs over the left and upper edge and
covers nearly all of the frame), N = 4 (r = 0.3, cut by the upper edge), N = 8 (r = 0.176, the 90 px face of paste_fade_ref.small_case, inside the frame)
-- in both mask forms: the blurred parse mask sampled in face space and supersampled, and the frame-space erosion mask
(``mask_border`` < 0), where only the face is supersampled.  The restatement's warps on the N-times finer grids and both kinds of soft
masks are computed once per module."""
import ctypes as C

import numpy as np
import pytest
import torch

import footprint as FP
import paste_aa_ref as AR
import paste_fade_ref as FR
import paste_oracle as P
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import paste

pytestmark = pytest.mark.gpu

CORE, W, AA = 'keep_paste_face', 'keep_paste_face_w', 'keep_paste_face_aa'
FORMS = ['parse-mask', 'frame-mask']
NS = [2, 4, 8]
THIRD = float(np.float32(1.0 / 3.0))
H_, W_ = 160, 200


def d2s_of(M):
    return (C.c_double * 6)(*paste.invert_affine(M).reshape(-1).tolist())


class Case:
    def __init__(self):
        rng = np.random.default_rng(11)
        self.frame = rng.integers(0, 256, (H_, W_, 3), dtype=np.uint8)
        self.faces = rng.integers(0, 256, (3, 512, 512, 3), dtype=np.uint8)
        cls = FR.small_case()[3]
        self.classes = np.stack([cls[0], cls[1], cls[0]])
        self.mats = [AR.similarity(0.55, 0.15, -60.0, -70.0), AR.similarity(0.3, 0.2, 40.0, -30.0), AR.similarity(90.0 / 512.0, 0.1, 40.3, 50.7)]
        assert [paste.aa_factor(M) for M in self.mats] == NS
        self.gp = paste.GpuPaster('cuda')
        self.faces_dev = torch.from_numpy(self.faces).cuda()
        self.frame_f32 = torch.from_numpy(self.frame.astype(np.float32)).cuda()
        self.boxes = [paste.face_box(M, 512, 512, W_, H_) for M in self.mats]
        assert self.boxes[0] == (0, 0, W_, H_) and self.boxes[1][1] == 0 and self.boxes[1][3] < H_            # cut by the edges as said above
        assert self.boxes[2][0] > 0 and self.boxes[2][1] > 0 and self.boxes[2][2] < W_ and self.boxes[2][3] < H_
        self.fine = [d2s_of(paste.ss_affine(M, n)) for M, n in zip(self.mats, NS)]
        coarse = [d2s_of(M) for M in self.mats]
        self.masks = {'parse-mask': list(self.gp.soft_masks(torch.from_numpy(self.classes).cuda())),
                      'frame-mask': [self.gp.erosion_mask(d, H_, W_, 512, 512, 1.0) for d in coarse]}
        assert all(m is not None for m in self.masks['frame-mask'])
        faces, mats = list(self.faces), list(self.mats)
        self.soft = {'parse-mask': AR.frame_soft_masks(self.frame, faces, mats, list(self.classes)),
                     'frame-mask': AR.frame_soft_masks(self.frame, faces, mats, None)}
        self.means = [AR.face_mean(f, M, n, W_, H_) for f, M, n in zip(faces, mats, NS)]

    def border(self, form):
        return paste.PARSE_BORDER if form == 'parse-mask' else -1

    def launch(self, acc, i, form, opacity, box=None, n=None):
        L.call(AA, acc, H_, W_, self.faces_dev[i], self.masks[form][i], 512, 512, self.fine[i], *(self.boxes[i] if box is None else box),
               self.border(form), NS[i] if n is None else n, C.c_float(opacity))

    def ref(self, i, form, opacity, base=None):
        """The float frame behind face i alone at ``opacity``, blended onto ``base`` (default: the frame)."""
        up = self.frame.astype(np.float32) if base is None else base
        m = (self.soft[form][i].astype(np.float32) * np.float32(opacity))[:, :, None].astype(np.float32)
        return m * self.means[i] + (np.float32(1) - m) * up


@pytest.fixture(scope='module')
def case():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return Case()


def rounded(acc):
    out = torch.empty(acc.shape, dtype=torch.uint8, device=acc.device)
    L.call('keep_f32_round_u8', acc, out, acc.numel())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('i', [0, 1, 2], ids=['N2', 'N4', 'N8'])
def test_kernel_equals_the_restatement_bit_for_bit(case, i, form):
    for opacity in (1.0, 0.5, THIRD):
        acc = case.frame_f32.clone()
        case.launch(acc, i, form, opacity)
        torch.cuda.synchronize()
        ref = case.ref(i, form, opacity)
        got = acc.cpu().numpy()
        diff = np.abs(got - ref)
        print(f"N {NS[i]} {form} opacity {opacity}: max abs difference {float(diff.max())}, differing values {int((diff != 0).sum())}")
        assert np.array_equal(got, ref)
        assert np.array_equal(rounded(acc), np.round(np.clip(ref, 0, 255)).astype(np.uint8))
        assert (got != case.frame.astype(np.float32)).any()                               # (the face really landed)
        again = case.frame_f32.clone()                                                   # two runs give equal results
        case.launch(again, i, form, opacity)
        torch.cuda.synchronize()
        assert torch.equal(again, acc)
    # ... and the supersampled face is not the single tap's
    one = case.frame_f32.clone()
    L.call(CORE, one, H_, W_, case.faces_dev[i], case.masks[form][i], 512, 512, d2s_of(case.mats[i]), *case.boxes[i], case.border(form))
    torch.cuda.synchronize()
    assert not torch.equal(one, acc)


@pytest.mark.parametrize('form', FORMS)
def test_faces_blended_one_after_the_other(case, form):
    acc, ref = case.frame_f32.clone(), None
    for i, opacity in ((0, THIRD), (1, 1.0), (2, 0.5)):
        case.launch(acc, i, form, opacity)
        ref = case.ref(i, form, opacity, ref)
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), ref)


@pytest.mark.parametrize('i', [0, 1, 2], ids=['N2', 'N4', 'N8'])
@pytest.mark.parametrize('width', [1, 3, 5, 17])
def test_box_widths_that_are_no_multiple_of_the_pixels_per_wave(case, i, width):
    """A sub-box of the face's box, ``width`` wide and 1, 3, 5 or 17 rows high: inside it the restatement, outside it the frame as it
    was -- also in the rest of the blocks' tiles."""
    x0, y0 = case.boxes[i][0] + 37, case.boxes[i][1] + 41
    box = (x0, y0, x0 + width, y0 + {1: 17, 3: 5, 5: 3, 17: 1}[width])
    for form in FORMS:
        acc = case.frame_f32.clone()
        case.launch(acc, i, form, 0.5, box=box)
        torch.cuda.synchronize()
        want = case.frame.astype(np.float32)
        full = case.ref(i, form, 0.5)
        want[box[1]:box[3], box[0]:box[2]] = full[box[1]:box[3], box[0]:box[2]]
        assert np.array_equal(acc.cpu().numpy(), want)
        assert (want != case.frame.astype(np.float32)).any()


@pytest.mark.parametrize('edge', ['left', 'top', 'right', 'bottom'])
@pytest.mark.parametrize('n', NS)
def test_boxes_cut_by_each_frame_edge(case, edge, n):
    """One face per (edge, N), all but a strip of 40 px past that edge of an 80 x 96 frame, the frame-space mask a constant 0.75, so
    that every pixel of the box -- also those whose sub-samples leave the crop, which read 0 -- shows in the result."""
    h, w = 80, 96
    r = {2: 0.5, 4: 0.25, 8: 0.125}[n] * 1.1
    side = 512 * r
    tx, ty = {'left': (40 - side, 20.3), 'top': (20.3, 40 - side), 'right': (w - 40, 10.7), 'bottom': (10.7, h - 40)}[edge]
    M = AR.similarity(r, 0.1, tx, ty)
    assert paste.aa_factor(M) == n
    box = paste.face_box(M, 512, 512, w, h)
    assert {'left': box[0] == 0, 'top': box[1] == 0, 'right': box[2] == w, 'bottom': box[3] == h}[edge]
    frame = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    soft = np.full((h, w), 0.75, np.float32)
    acc = torch.from_numpy(frame.astype(np.float32)).cuda()
    L.call(AA, acc, h, w, case.faces_dev[1], torch.from_numpy(soft).cuda(), 512, 512, d2s_of(paste.ss_affine(M, n)), *box, -1, n, C.c_float(1.0))
    torch.cuda.synchronize()
    mean = AR.face_mean(case.faces[1], M, n, w, h)
    ref = AR.composite_f32(frame, [case.faces[1]], [M], soft=[soft], means=[mean], factors=[n])
    want = frame.astype(np.float32)
    want[box[1]:box[3], box[0]:box[2]] = ref[box[1]:box[3], box[0]:box[2]]
    assert np.array_equal(acc.cpu().numpy(), want)
    # the case has what it is for: frame pixels of the box with some, but not all, of their sub-samples outside the crop
    cover = P.warp_affine_f32(np.ones((512, 512), np.float32), paste.ss_affine(M, n), n * w, n * h)
    outside = AR.cell_sums((cover == 0).astype(np.int32), n)[box[1]:box[3], box[0]:box[2]]
    assert ((outside > 0) & (outside < n * n)).any() and (outside == n * n).any() and (outside == 0).any()


@pytest.mark.parametrize('form', FORMS)
def test_bad_n_and_bad_opacity_are_refused_and_nothing_is_written(case, form):
    for kw in [dict(n=0), dict(n=1), dict(n=3), dict(n=16), dict(n=-4), dict(opacity=-0.25), dict(opacity=1.5), dict(opacity=float('nan')),
               dict(opacity=float('inf'))]:
        acc = case.frame_f32.clone()
        with pytest.raises(L.KeepHipError) as e:
            case.launch(acc, 1, form, kw.get('opacity', 0.5), n=kw.get('n'))
        assert e.value.code == L.EINVAL and AA + ':' in str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(acc, case.frame_f32)


def recorded(monkeypatch):
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def test_paster_aa_equals_the_restatement_after_rounding(case, monkeypatch):
    calls = recorded(monkeypatch)
    cls = torch.from_numpy(case.classes).cuda()
    faces, mats = list(case.faces), list(case.mats)
    got = case.gp.paste(case.frame, case.faces, mats, cls, aa=True)
    assert calls.count(AA) == 3 and calls.count(CORE) == 0 and calls.count(W) == 0 and case.gp.last_aa == NS
    ref = AR.paste_faces_aa(case.frame, faces, mats, list(case.classes), soft=case.soft['parse-mask'], means=case.means)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref)
    plain = case.gp.paste(case.frame, case.faces, mats, cls)
    assert case.gp.last_aa is None and not torch.equal(plain, got)
    assert np.array_equal(plain.cpu().numpy(), FR.paste_faces_weighted(case.frame, faces, mats, list(case.classes)))   # aa=False: today's frame
    # weights, a skipped face, the erosion-mask form
    wts = [0.5, 1, THIRD]
    got = case.gp.paste(case.frame, case.faces, [mats[0], None, mats[2]], cls, weights=wts, aa=True)
    assert case.gp.last_aa == [2, None, 8]
    ref = AR.paste_faces_aa(case.frame, faces, [mats[0], None, mats[2]], list(case.classes), weights=wts, soft=case.soft['parse-mask'],
                            means=case.means)
    assert np.array_equal(got.cpu().numpy(), ref)
    got = case.gp.paste(case.frame, case.faces, mats, None, 1.0, weights=wts, aa=True)
    ref = AR.paste_faces_aa(case.frame, faces, mats, None, weights=wts, soft=case.soft['frame-mask'], means=case.means)
    assert np.array_equal(got.cpu().numpy(), ref)
    # draw_box works as today: the same green pixels over the area-sampled frame
    boxed = case.gp.paste(case.frame, case.faces, [None, None, mats[2]], cls, draw_box=True, aa=True).cpu().numpy()
    today = case.gp.paste(case.frame, case.faces, [None, None, mats[2]], cls, draw_box=True).cpu().numpy()
    soft_aa = case.gp.paste(case.frame, case.faces, [None, None, mats[2]], cls, aa=True).cpu().numpy()
    green = (today == np.array([0, 255, 0], np.uint8)).all(axis=2) & (boxed == np.array([0, 255, 0], np.uint8)).all(axis=2)
    assert green.sum() > 50 and np.array_equal(boxed[~green], soft_aa[~green])


def test_paster_aa_on_faces_that_are_not_shrunk_makes_only_todays_calls(case, monkeypatch):
    mats = [AR.similarity(1.18, 0.1, -200.0, -150.0), AR.similarity(1.0, 0.0, -100.5, -200.25)]
    assert [paste.aa_factor(M) for M in mats] == [1, 1]
    cls = torch.from_numpy(case.classes[:2]).cuda()
    for classes, weights in ((cls, None), (cls, [0.5, 1.0]), (None, None)):
        kw = {} if weights is None else {'weights': weights}
        calls = recorded(monkeypatch)
        today = case.gp.paste(case.frame, case.faces[:2], mats, classes, **kw)
        names = list(calls)
        calls.clear()
        got = case.gp.paste(case.frame, case.faces[:2], mats, classes, aa=True, **kw)
        assert list(calls) == names and AA not in names and case.gp.last_aa == [1, 1]
        assert torch.equal(got, today) and (today.cpu().numpy() != case.frame).any()
        monkeypatch.undo()


@pytest.mark.parametrize('r,theta', [(0.25, 0.2), (0.2, 0.1), (0.6, 0.15)])
def test_checkerboard_property_on_the_device(case, r, theta):
    frame, face, M, cls = AR.checkerboard_case(r, theta)
    n = paste.aa_factor(M)
    sf = [P.parse_soft_mask(cls)]
    soft1 = AR.frame_soft_masks(frame, [face], [M], [cls], factors=[1], parse_soft=sf)
    softn = AR.frame_soft_masks(frame, [face], [M], [cls], parse_soft=sf)
    cls_dev = torch.from_numpy(cls[None]).cuda()
    default = case.gp.paste(frame, face[None], [M], cls_dev).cpu().numpy()
    aa = case.gp.paste(frame, face[None], [M], cls_dev, aa=True).cpu().numpy()
    assert case.gp.last_aa == [n]
    assert np.array_equal(aa, AR.paste_faces_aa(frame, [face], [M], [cls], soft=softn))
    sel = (soft1[0] > 0.999) & (softn[0] > 0.999)
    d, a = default[sel].astype(np.float64), aa[sel].astype(np.float64)
    print(f"r {r} theta {theta} N {n}: {int(sel.sum())} pixels; default {d.min():.0f} .. {d.max():.0f} std {d.std():.2f}; "
          f"area-sampled {a.min():.0f} .. {a.max():.0f} std {a.std():.2f}")
    assert sel.sum() > 5000 and d.min() == 0 and d.max() == 255 and d.std() > 30
    assert a.min() >= 127.5 - 14 and a.max() <= 127.5 + 14 and a.std() < 5
    assert np.array_equal(aa[softn[0] == 0], frame[softn[0] == 0])


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('form', FORMS)
def test_footprint_under_poisoned_surroundings(n, form):
    """Every buffer in an allocation of its own between guards (tests/footprint.py): a 24 x 40 frame, a 64 x 48 crop that hangs over the
    frame's left and lower edge, the box the whole frame -- most sub-samples of the box's rim leave the crop."""
    h, w, fh, fw = 24, 40, 64, 48
    r = {2: 0.6, 4: 0.3, 8: 0.15}[n]
    M = AR.similarity(r, 0.2, -5.5, 9.25)
    assert paste.aa_factor(M) == n
    g = torch.Generator().manual_seed(n)
    R = [FP.single('frame', torch.rand((h * w, 3), generator=g) * 255, role='rw'),
         FP.single('face', torch.randint(0, 256, (fh * fw, 3), generator=g, dtype=torch.uint8))]
    if form == 'frame-mask':
        R.append(FP.single('mask', torch.rand((h, w), generator=g)))
    else:
        R.append(FP.single('mask', torch.rand((fh, fw), generator=g) * 255))
    fine = d2s_of(paste.ss_affine(M, n))
    border = -1 if form == 'frame-mask' else 3
    out = FP.run(lambda t: L.call(AA, t['frame'], h, w, t['face'], t['mask'], fh, fw, fine, 0, 0, w, h, border, n, C.c_float(0.75)), R, 'cuda')
    assert set(out) == {'frame'}
