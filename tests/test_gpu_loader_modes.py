"""GPU tests of the loader modes 'resize' / 'stacking' and the reflect pad (csrc/resize.hip, the pad_mode of salt_preprocess and
salt_augment_preprocess) against the float64 restatements of tests/loader_modes_reference.py, through the C-ABI on guarded operands,
and of the Python surface built on them (StackingPreprocessor, ValidationMonitor's resized scoring, predict_tta_tiles)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_ops as O
import aug_reference as AR
import loader_modes_reference as L
import net_checks as NC
from helpers import T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'F22_loader_modes.npz')
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# (g / 255 - mean) / std in fp32: three roundings of values below 4 plus the two rounded constants: < 2e-6; one gray level is 1.7e-2
X_TOL = 2e-6


class Guarded:
    """n integers (uint8 / int32) on the device between two runs of 64 sentinel values"""

    def __init__(self, n, dtype, sentinel=113):
        self.sentinel = sentinel
        self.buf = torch.full((n + 128,), sentinel, dtype=dtype, device=DEV)
        self.win = self.buf[64:64 + n]
        self.win.fill_(77)

    def ptr(self):
        return self.win.data_ptr()

    def get(self, shape):
        b = self.buf.cpu()
        assert bool((b[:64] == self.sentinel).all()) and bool((b[-64:] == self.sentinel).all()), 'write outside an integer output'
        return b[64:-64].reshape(shape).numpy()


def one_step(got, ref64, what):
    """|got - float32(ref64)| <= 2^-24 max(|ref64|, 2^-126) on every element: the single rounding of a float64 value to fp32"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    err = np.abs(got - ref64.astype(np.float32).astype(np.float64))
    bound = 2.0 ** -24 * np.maximum(np.abs(ref64), 2.0 ** -126)
    print('%s: max err / bound %.3f, %d of %d elements differ from float32(ref)' % (what, float((err / bound).max()), int((err > 0).sum()), err.size))
    assert bool((err <= bound).all()), '%s: %d elements over one fp32 rounding step (max err %.3e)' % (what, int((err > bound).sum()), float(err.max()))


# ----------------------------------------------------------------------------- salt_stack_resize
def _stack_resize(x, layout, HW):
    """x: [B,h,w,M] numpy -> (out float64 [B,M,H,W] through guards, second run's bits)"""
    B, h, w, M = x.shape
    if layout == 'hwm':
        src, strides = x, dict(sb=h * w * M, sr=w * M, sc=M, sm=1)
    else:
        src, strides = np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2))), dict(sb=M * h * w, sr=w, sc=1, sm=h * w)
    xin = O.vec_of(torch.from_numpy(src))
    frozen = O.Frozen(x=xin.buf)
    runs = []
    for _ in range(2):
        y = O.Vec(B * M * HW[0] * HW[1])
        O.call('salt_stack_resize', x=xin.ptr(), B=B, h=h, w=w, M=M, H=HW[0], W=HW[1], y=y.ptr(), **strides)
        runs.append(y.get((B, M) + tuple(HW)))
    frozen.check('stack_resize')
    assert torch.equal(O.bits(runs[0].float()), O.bits(runs[1].float())), 'stack_resize: two runs differ'
    return runs[0].numpy()


@pytest.mark.parametrize('layout', ['hwm', 'mhw'])
@pytest.mark.parametrize('hw,HW', L.STACK_SIZES, ids=['%dx%d-%dx%d' % (a + b) for a, b in L.STACK_SIZES])
def test_stack_resize(hw, HW, layout):
    for M in L.STACK_MAPS:
        for B in L.BATCHES:
            x = L.stack_case(hw, M, B)
            got = _stack_resize(x, layout, HW)
            assert np.isfinite(got).all()
            one_step(got, L.stack_resize(x, HW), 'stack_resize %s %s->%s M=%d B=%d' % (layout, hw, HW, M, B))
            if hw == HW:
                assert np.array_equal(got.astype(np.float32), np.transpose(x, (0, 3, 1, 2)))       # integer coordinates: a transpose
    g = np.load(GOLDEN)['r1_%dx%d_%dx%d' % (hw + HW)]                               # scipy's own values for M = 5, B = 1
    got = _stack_resize(L.stack_case(hw, 5, 1), layout, HW)[0][:, L.golden_rows(HW[0])]
    assert np.abs(got - g).max() <= 2.0 ** -24 * max(np.abs(g).max(), 1e-30) + 1e-14


# ----------------------------------------------------------------------------- salt_mask_resize
def _dev_table(table):
    start, length, weights = table
    return T(start).to(DEV), T(length).to(DEV), T(weights).to(DEV)


@pytest.mark.parametrize('kind', L.MASK_KINDS)
@pytest.mark.parametrize('n,N', L.MASK_SIZES)
def test_mask_resize_is_pil(n, N, kind):
    masks = L.mask_case(n, kind)
    B = masks.shape[0]
    (rs, rl, rw), (cs, cl, cw) = _dev_table(L.pil_axis_table(n, N)), _dev_table(L.pil_axis_table(n, N))
    m = Guarded(masks.size, torch.uint8)
    m.win.copy_(T(masks).reshape(-1))
    frozen = O.Frozen(mask=m.buf, rw=rw, cw=cw, rs=rs, cs=cs, rl=rl, cl=cl)
    out = O.Vec(B * 2 * N * N)
    O.call('salt_mask_resize', mask=m.ptr(), B=B, h=n, w=n, H=N, W=N, row_start=rs.data_ptr(), row_len=rl.data_ptr(), row_w=rw.data_ptr(),
           row_taps=rw.shape[1], col_start=cs.data_ptr(), col_len=cl.data_ptr(), col_w=cw.data_ptr(), col_taps=cw.shape[1], target=out.ptr())
    got = out.get((B, 2, N, N)).numpy().astype(np.float32)
    frozen.check('mask_resize')
    assert np.array_equal(got, L.mask_target(masks, (N, N)))
    assert np.array_equal(got, np.load(GOLDEN)['pil_%d_%d_%s' % (n, N, kind)].astype(np.float32))      # PIL's own output


# ----------------------------------------------------------------------------- salt_resize_prob / threshold / iou sweep
@pytest.mark.parametrize('HW,hw', L.PROB_SIZES, ids=['%dx%d-%dx%d' % (a + b) for a, b in L.PROB_SIZES])
def test_resize_prob(HW, hw):
    for C in (1, 2):
        for B in L.BATCHES:
            p = L.prob_case(HW, C, B)
            pin = O.vec_of(torch.from_numpy(p))
            frozen = O.Frozen(p=pin.buf)
            out = O.Vec(B * C * hw[0] * hw[1])
            O.call('salt_resize_prob', prob=pin.ptr(), B=B, C=C, H=HW[0], W=HW[1], h=hw[0], w=hw[1], out=out.ptr())
            frozen.check('resize_prob')
            one_step(out.get((B, C) + tuple(hw)).numpy(), L.resize_back(p, hw), 'resize_prob %s->%s C=%d B=%d' % (HW, hw, C, B))
    g = np.load(GOLDEN)['r2_%dx%d_%dx%d' % (HW + hw)]
    p = L.prob_case(HW, 2, 1)
    pin, out = O.vec_of(torch.from_numpy(p)), O.Vec(2 * hw[0] * hw[1])
    O.call('salt_resize_prob', prob=pin.ptr(), B=1, C=2, H=HW[0], W=HW[1], h=hw[0], w=hw[1], out=out.ptr())
    got = out.get((2,) + tuple(hw)).numpy()[:, L.golden_rows(hw[0])]
    assert np.abs(got - g).max() <= 2.0 ** -24 * np.abs(g).max() + 1e-14


@pytest.mark.parametrize('C', [1, 2])
@pytest.mark.parametrize('HW,hw', L.PROB_SIZES, ids=['%dx%d-%dx%d' % (a + b) for a, b in L.PROB_SIZES])
def test_resize_threshold_and_sweep_decide_as_float64(HW, hw, C):
    """identical masks and integer counts: the case table keeps every interpolant 1e-9 away from every threshold (CPU test)"""
    cls = C - 1
    for B in L.BATCHES:
        p, gt = L.prob_case(HW, C, B), L.gt_case(hw, B)
        v64 = L.resize_back(p[:, cls], hw)
        pin = O.vec_of(torch.from_numpy(p))
        g = Guarded(gt.size, torch.uint8)
        g.win.copy_(T(gt).reshape(-1))
        frozen = O.Frozen(p=pin.buf, gt=g.buf)
        for Tn, th in L.THRESHOLDS.items():
            inter, pred, gtc = Guarded(B * Tn, torch.int32), Guarded(B * Tn, torch.int32), Guarded(B, torch.int32)
            tha = (ctypes.c_double * Tn)(*[float(t) for t in th])
            O.call('salt_resize_iou_sweep', prob=pin.ptr(), B=B, C=C, H=HW[0], W=HW[1], cls=cls, h=hw[0], w=hw[1], gt=g.ptr(), T=Tn,
                   thresholds=ctypes.cast(tha, ctypes.c_void_p).value, inter=inter.ptr(), pred=pred.ptr(), gt_count=gtc.ptr())
            ri, rp, rg = L.counts(v64, gt, th)
            assert np.array_equal(inter.get((B, Tn)), ri) and np.array_equal(pred.get((B, Tn)), rp) and np.array_equal(gtc.get((B,)), rg), (B, Tn)
        for t in L.THRESHOLDS[32][::4]:
            mask = Guarded(B * hw[0] * hw[1], torch.uint8)
            O.call('salt_resize_threshold', prob=pin.ptr(), B=B, C=C, H=HW[0], W=HW[1], cls=cls, h=hw[0], w=hw[1], threshold=float(t), mask=mask.ptr())
            assert np.array_equal(mask.get((B,) + tuple(hw)), (v64 > t).astype(np.uint8)), (B, t)
        frozen.check('resize sweep')


# ----------------------------------------------------------------------------- reflect pad
def _tiles(B, n, seed):
    r = np.random.RandomState(seed)
    img = r.randint(0, 256, (B, n, n)).astype(np.uint8)
    msk = (r.random_sample((B, n, n)) < 0.4).astype(np.uint8)
    return img, msk


def _resized(a, rn, binarize=False):
    if rn == a.shape[1]:
        return a
    out = np.stack([L.resize_cubic_u8_fixed(t, rn, rn) for t in a])
    return (out > 0).astype(np.uint8) if binarize else out


# (tile, resized tile, top, bottom, left, right): the train branch 101 -> 102 + 13, the inference 13 / 14 split, the smallest tile that
# still reflects 13 pixels
REFLECT_CASES = {'train': (101, 102, 13, 13, 13, 13), 'inference': (101, 101, 13, 14, 14, 13), 'smallest': (15, 15, 13, 13, 13, 13)}


@pytest.mark.parametrize('channels', [1, 3])
@pytest.mark.parametrize('case', sorted(REFLECT_CASES))
def test_preprocess_reflect(case, channels):
    n, rn, top, bottom, left, right = REFLECT_CASES[case]
    B = 3
    img, msk = _tiles(B, n, 5)
    H, W = rn + top + bottom, rn + left + right
    xi, mi = Guarded(img.size, torch.uint8), Guarded(msk.size, torch.uint8)
    xi.win.copy_(T(img).reshape(-1)); mi.win.copy_(T(msk).reshape(-1))
    frozen = O.Frozen(img=xi.buf, mask=mi.buf)
    res = {}
    for pad_mode in (0, 1):
        x, t = O.Vec(B * channels * H * W), O.Vec(B * 2 * H * W)
        O.call('salt_preprocess', img=xi.ptr(), img_is_u8=1, mask=mi.ptr(), B=B, h=n, w=n, resize_h=rn if rn != n else 0, resize_w=rn if rn != n else 0,
               top=top, left=left, H=H, W=W, channels=channels, mean=MEAN, std=STD, x=x.ptr(), target=t.ptr(), interpolation=2, pad_mode=pad_mode)
        res[pad_mode] = (x.get((B, channels, H, W)).numpy(), t.get((B, 2, H, W)).numpy())
    frozen.check('preprocess')
    for pad_mode, pad in ((0, L.edge_pad), (1, L.reflect_pad)):
        gray = pad(_resized(img, rn), top, bottom, left, right)
        m = pad(_resized(msk, rn, True), top, bottom, left, right).astype(np.float64)
        x, t = res[pad_mode]
        assert np.abs(x - L.normalise(gray, H, channels)).max() <= X_TOL * (2 if channels == 3 else 1), (case, pad_mode)
        assert np.array_equal(t, np.stack([1 - m, m], 1)), (case, pad_mode)
    inner = (slice(None), slice(None), slice(top, top + rn), slice(left, left + rn))
    assert np.array_equal(res[0][0][inner], res[1][0][inner]) and not np.array_equal(res[0][0], res[1][0])      # only the pad differs


@pytest.mark.parametrize('case', sorted(REFLECT_CASES))
def test_augment_preprocess_reflect_in_replay(case):
    """replayed parameters (flip + invert): the geometric stage is the one of pad_mode 0, the padded gray grid is the reflect pad of the
    resized stage, and the intensity stage runs on the padded grid"""
    n, rn, top, bottom, left, right = REFLECT_CASES[case]
    B = 2
    img, msk = _tiles(B, n, 6)
    H, W = rn + top + bottom, rn + left + right
    row = np.zeros((B, 64), np.float32)
    row[:, 1], row[:, 2], row[:, 6], row[:, 53] = 1, 1, 1, 1                         # SomeOf n = 1: Fliplr fires; Invert
    row[1, 6] = 0
    xi, mi, prm = T(img).to(DEV), T(msk).to(DEV), T(row).to(DEV)
    abi = O._abi()
    res = {}
    for pad_mode in (0, 1):
        x, t = O.Vec(B * H * W), O.Vec(B * 2 * H * W)
        gi, gm, gray = Guarded(img.size, torch.uint8), Guarded(img.size, torch.uint8), Guarded(B * H * W, torch.uint8)
        fn, S = abi.OP_FUNCS['salt_augment_preprocess']
        s = abi.fill(S(), img=xi.data_ptr(), mask=mi.data_ptr(), B=B, h=n, w=n, resize_h=rn if rn != n else 0, resize_w=rn if rn != n else 0, top=top,
                     left=left, H=H, W=W, channels=1, mean=MEAN, std=STD, x=x.ptr(), target=t.ptr(), seed=5, counter=0, params=prm.data_ptr(),
                     params_given=1, geo_img=gi.ptr(), geo_mask=gm.ptr(), gray=gray.ptr(), pad_mode=pad_mode)
        abi.check(fn(ctypes.byref(s), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'augment_preprocess')
        torch.cuda.synchronize()
        res[pad_mode] = (x.get((B, 1, H, W)).numpy(), t.get((B, 2, H, W)).numpy(), gi.get(img.shape), gm.get(img.shape), gray.get((B, H, W)))
    geo_img = np.stack([img[0][:, ::-1], img[1]])
    geo_msk = np.stack([msk[0][:, ::-1], msk[1]])
    for pad_mode, pad in ((0, L.edge_pad), (1, L.reflect_pad)):
        x, t, gi, gm, gray = res[pad_mode]
        assert np.array_equal(gi, geo_img) and np.array_equal(gm, geo_msk)
        want = 255 - pad(_resized(geo_img, rn), top, bottom, left, right)
        assert np.array_equal(gray, want), (case, pad_mode)
        m = pad(_resized(geo_msk, rn, True), top, bottom, left, right).astype(np.float64)
        assert np.array_equal(t, np.stack([1 - m, m], 1))
        assert np.abs(x[:, 0] - AR.normalise(want).astype(np.float64)).max() <= X_TOL
    inner = (slice(None), slice(top, top + rn), slice(left, left + rn))
    assert np.array_equal(res[0][4][inner], res[1][4][inner]) and not np.array_equal(res[0][4], res[1][4])      # only the pad differs


def test_device_preprocessor_modes():
    """DevicePreprocessor(loader_mode='resize') is the cubic resize to 128 without a pad in both branches (R4); pad_method='reflect'
    reaches the kernels in both branches and with augment="""
    from salt_amd.input_pipeline import AugmentConfig, DevicePreprocessor
    img, msk = _tiles(2, 101, 7)
    xi, mi = T(img).to(DEV), T(msk).to(DEV)
    gray = _resized(img, 128)
    m = _resized(msk, 128, True).astype(np.float64)
    outs = []
    for train in (True, False):
        x, t = DevicePreprocessor(train, 3, resize=128, loader_mode='resize')(xi, mi)
        assert tuple(x.shape) == (2, 3, 128, 128)
        assert np.abs(x.cpu().numpy() - L.normalise(gray, 128, 3)).max() <= 2 * X_TOL
        assert np.array_equal(t.cpu().numpy(), np.stack([1 - m, m], 1))
        outs.append(x)
    assert torch.equal(outs[0], outs[1])
    x, _ = DevicePreprocessor(False, 1, pad_method='reflect')(xi)
    assert np.abs(x.cpu().numpy() - L.normalise(L.reflect_pad(img, 13, 14, 14, 13), 128, 1)).max() <= X_TOL
    x, _ = DevicePreprocessor(True, 1, pad_method='reflect')(xi)
    assert np.abs(x.cpu().numpy() - L.normalise(L.reflect_pad(_resized(img, 102), 13, 13, 13, 13), 128, 1)).max() <= X_TOL
    xa, _ = DevicePreprocessor(True, 1, pad_method='reflect', augment=AugmentConfig.none())(xi)
    assert torch.equal(xa, x)


# ----------------------------------------------------------------------------- surface
def _first_level(n, seed, M=5, size=101):
    """n tiles of M first-level probability maps [n,size,size,M] (a disc seen through M noisy models) and their uint8 masks"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing='ij')
    masks = torch.zeros(n, size, size)
    for i in range(n):
        if i % 3 == 0:
            continue
        cy, cx, r = [int(v) for v in torch.randint(size // 4, 3 * size // 4, (3,), generator=g)]
        masks[i] = (((yy - cy) ** 2 + (xx - cx) ** 2) < max(r // 2, 6) ** 2).float()
    stacks = torch.sigmoid(4.0 * (masks[..., None] - 0.5) + torch.randn(n, size, size, M, generator=g))
    return stacks.contiguous(), masks.to(torch.uint8)


def test_stacking_preprocessor_feeds_fit_and_the_monitor_scores_resized():
    from salt_amd import callbacks as C, inference as I
    from salt_amd.input_pipeline import StackingPreprocessor
    pre = StackingPreprocessor()
    St, Mt = _first_level(8, 1)
    Sv, Mv = _first_level(4, 2)
    Xt, Tt = pre(St.to(DEV), Mt.to(DEV))
    Xv, Tv = pre(Sv.to(DEV), Mv.to(DEV))
    assert tuple(Xt.shape) == (8, 5, 128, 128) and tuple(Tt.shape) == (8, 2, 128, 128)
    one_step(Xv.cpu().numpy(), L.stack_resize(Sv.numpy(), (128, 128)), 'StackingPreprocessor X')
    assert np.array_equal(Tv.cpu().numpy(), L.mask_target(Mv.numpy(), (128, 128)))
    Xp, _ = pre(Sv.permute(0, 3, 1, 2).contiguous().to(DEV))                        # [B,M,h,w] planes: the same tensor
    assert torch.equal(Xp, Xv)
    train = ([[Xt[i:i + 4].cpu(), Tt[i:i + 4].cpu()] for i in (0, 4)], 1)           # one epoch, two steps
    valid = ([[Xv[i:i + 2].cpu(), Tv[i:i + 2].cpu()] for i in (0, 2)], 1)
    cfg = {'training_monitor': {'batch_every': 0, 'epoch_every': 1},
           'validation_monitor': {'epoch_every': 1, 'data_dir': None, 'loader_mode': 'stacking', 'use_depth': False}}
    scores = {}
    for name, meta in (('resized', Mv.numpy()), ('crop', None)):
        torch.manual_seed(0)
        m = NC.family_model('StackingFCN', 'f32', 1e-3, 1, cfg, input_model_nr=5)
        m.fit(train, valid, meta_valid=meta)
        assert m.optimizer.steps == 2 and sorted(m.validation_loss) == [0]
        val = m.validation_loss[0]
        m.model.eval()
        with torch.no_grad():
            prob = torch.sigmoid(torch.cat([m.model(b[0].to(DEV)).float() for b in valid[0]])).cpu().double().numpy()
        if name == 'resized':                                                      # float64 host computation on the same probabilities
            cnt = L.counts(L.resize_back(prob[:, 1], (101, 101)), Mv.numpy(), L.SWEEP)
        else:                                                                       # today's numbers: the batches' own targets, centre crop
            cnt = L.counts(prob[:, 1, 13:114, 14:115], Tv[:, 1, 13:114, 14:115].cpu().numpy() > 0.5, L.SWEEP)
            again = C.score_validation(m, valid)
            assert all(torch.equal(again[k], val[k]) for k in val)
        t_best, iou, iout = I.select_threshold([cnt], L.SWEEP)
        print(name, t_best, iou, iout, float(val['iou']), float(val['iout']))
        assert float(val['iou']) == np.float32(iou) and float(val['iout']) == np.float32(iout) and m.best_threshold == t_best
        scores[name] = val
    assert abs(float(scores['resized']['sum']) - float(scores['crop']['sum'])) <= 1e-4 * abs(float(scores['crop']['sum']))   # the loss is the batches' own


def test_predict_tta_tiles_in_resize_mode():
    """every variant is scaled in by the preprocessor, the aggregate comes back through resize_image: against the composition of the
    pieces (the variants' own forward passes, tta_mean) and the float64 restatement of the way back"""
    from salt_amd import architectures as A, inference as I
    from salt_amd._abi import SaltError
    from salt_amd.input_pipeline import DevicePreprocessor
    torch.manual_seed(3)
    net = A.VanillaUNet(2, in_channels=1, base_filters=8, levels=3).to(DEV).eval()
    img, _ = _tiles(2, 101, 9)
    xi = T(img).to(DEV)
    pre = DevicePreprocessor(False, 1, resize=128, loader_mode='resize')
    got = I.predict_tta_tiles(net, pre, xi, flip_ud=True, flip_lr=True, loader_mode='resize')
    assert tuple(got.shape) == (2, 2, 101, 101)
    specs = [(False, False, 0), (True, True, 0), (True, False, 0), (False, True, 0)]
    with torch.no_grad():
        logits = torch.cat([net(pre(torch.flip(xi, dims=[d for d, on in ((1, ud), (2, lr)) if on]).contiguous() if (ud or lr) else xi)[0]).float()
                            for ud, lr, _ in specs])
    prob128 = I.tta_mean(logits, specs, 2)
    one_step(got.cpu().numpy(), L.resize_back(prob128.cpu().double().numpy(), (101, 101)), 'predict_tta_tiles resize')
    assert torch.equal(I.predict_tta_tiles(net, pre, xi, flip_ud=True, flip_lr=True, loader_mode='resize', target_size=(101, 101)), got)
    v64 = L.resize_back(prob128.cpu().double().numpy(), (101, 101))
    assert np.array_equal(I.resize_threshold(prob128, (101, 101), 0.45).cpu().numpy(), (v64[:, 1] > 0.45).astype(np.uint8))
    with pytest.raises(SaltError):
        I.predict_tta_tiles(net, pre, xi)                                           # the preprocessor is a 'resize' one
    with pytest.raises(SaltError):
        I.predict_tta_tiles(net, DevicePreprocessor(False, 1), xi, target_size=(101, 101))
    with pytest.raises(SaltError):
        I.resize_image(prob128, (129, 128))
