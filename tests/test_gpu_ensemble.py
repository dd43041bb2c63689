"""GPU tests of device-side ensembling (csrc/ensemble.hip: salt_ensemble, salt_rle_encode) through the C-ABI on guarded operands, against
the numpy restatements of tests/ensemble_reference.py, and of the Python surface built on them (salt_amd.ensemble).  Every comparison
is BIT equality: the arithmetic order is fixed (tests/test_ensemble_cpu.py shows that np.mean is that order)."""
import ctypes

import numpy as np
import pytest
import torch

import abi_ops as O
import ensemble_reference as E
import loader_modes_reference as L
from helpers import T, golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
E_BADARG, E_UNSUPPORTED = -1, -2


class Guarded:
    """n integers on the device between two runs of 64 sentinel values; the window starts at ``fill``"""

    def __init__(self, n, dtype, sentinel=113, fill=77):
        self.sentinel = sentinel
        self.buf = torch.full((n + 128,), sentinel, dtype=dtype, device=DEV)
        self.win = self.buf[64:64 + n]
        self.win.fill_(fill)

    def ptr(self):
        return self.win.data_ptr()

    def get(self, shape):
        b = self.buf.cpu()
        assert bool((b[:64] == self.sentinel).all()) and bool((b[-64:] == self.sentinel).all()), 'write outside an integer output'
        return b[64:-64].reshape(shape).numpy()


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Members:
    """K member maps on the device, each between its own guards, and the HOST table of their device pointers"""

    def __init__(self, maps):
        self.vecs = [O.vec_of(torch.from_numpy(m)) for m in maps]
        self.table = (ctypes.c_void_p * len(maps))(*[v.ptr() for v in self.vecs])
        self.frozen = O.Frozen(**{'member%d' % i: v.buf for i, v in enumerate(self.vecs)})
        self.K, (self.B, self.C, self.H, self.W) = len(maps), maps[0].shape

    def args(self):
        return dict(members=ctypes.cast(self.table, ctypes.c_void_p).value, K=self.K, B=self.B, C=self.C, H=self.H, W=self.W)


def run_ensemble(mem, mode, window, acc, threshold, cls=1, want=('mean', 'mask', 'stack'), layout='mhw', M=None, m0=0):
    """one salt_ensemble launch -> {'mean': float32 [B,C,h,w], 'mask': uint8 [B,h,w], 'stack': float32 in its layout, other slots kept}"""
    top, left, h, w = window
    M = mem.K if M is None else M
    mean = O.Vec(mem.B * mem.C * h * w)
    mask = Guarded(mem.B * h * w, torch.uint8)
    stack = O.Vec(mem.B * M * h * w, fill=O.SENTINEL)
    strides = dict(sb=M * h * w, sr=w, sc=1, sm=h * w) if layout == 'mhw' else dict(sb=h * w * M, sr=w * M, sc=M, sm=1)
    O.call('salt_ensemble', mode=mode, top=top, left=left, h=h, w=w, acc=acc, cls=cls, threshold=float(threshold),
           mean=mean.ptr() if 'mean' in want else None, mask=mask.ptr() if 'mask' in want else None,
           stack=stack.ptr() if 'stack' in want else None, m0=m0, **strides, **mem.args())
    out = {}
    got_mean, got_mask = mean.get((mem.B, mem.C, h, w)), mask.get((mem.B, h, w))
    got_stack = stack.get((mem.B, M, h, w) if layout == 'mhw' else (mem.B, h, w, M))
    if 'mean' in want:
        out['mean'] = got_mean.numpy().astype(np.float32)
    else:
        assert bool(torch.isnan(got_mean).all()), 'mean written though not requested'
    if 'mask' in want:
        out['mask'] = got_mask
    else:
        assert (got_mask == 77).all(), 'mask written though not requested'
    if 'stack' in want:
        out['stack'] = got_stack.numpy().astype(np.float32)
    else:
        assert bool((got_stack == O.SENTINEL).all()), 'stack written though not requested'
    return out


def same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype == np.uint8:
        n = int((a != b).sum())
    else:
        n = int((f32_bits(a) != f32_bits(b)).sum())
    print('%s: %d of %d elements differ' % (what, n, a.size))
    assert n == 0, '%s: %d of %d elements differ' % (what, n, a.size)


# ----------------------------------------------------------------------------- salt_ensemble, crop window
@pytest.mark.parametrize('K', E.ENSEMBLE_KS)
@pytest.mark.parametrize('case', E.CROP_CASES, ids=['%dx%d-%d-%d-%dx%d' % c for c in E.CROP_CASES])
def test_ensemble_crop_equals_numpy(case, K):
    H, W, top, left, h, w = case
    window = (top, left, h, w)
    for t in E.THRESHOLDS:
        maps = E.member_maps(K, 2, 2, H, W, window, t)
        mem = Members(maps)
        crops = [E.crop(m, *window) for m in maps]
        for acc, dtype in ((0, np.float32), (1, np.float64)):
            ref = np.mean(np.array([c.astype(dtype) for c in crops]), axis=0)                 # numpy itself
            assert ref.dtype == dtype
            same_bits(E.fold_mean(crops, dtype).astype(np.float32), ref.astype(np.float32), 'restatement')
            ref_mask = (ref[:, 1] > t).astype(np.uint8)                                       # numpy's decision in the accumulator's type
            assert np.array_equal(ref_mask, E.decide(ref[:, 1], t))
            what = 'crop %s K=%d acc=%d t=%g' % (case, K, acc, t)
            got = run_ensemble(mem, 0, window, acc, t)
            same_bits(got['mean'], ref.astype(np.float32), what + ' mean')
            same_bits(got['mask'], ref_mask, what + ' mask')
            same_bits(got['stack'], E.stack([c[:, 1] for c in crops], 'mhw'), what + ' stack')
            if K == 1:                                                                        # at, below, above the threshold
                planted = got['mask'][0, 0, :3].tolist()
                assert planted == [0, 0, 1], (what, planted)                                  # float32(0.47) < 0.47 < the fp32 value above it
            if t == 0.5 and acc == 0:
                assert got['mean'][0, 1, 0, 0] == np.float32(0.5)                             # j * 0.5 is exact: the mean sits ON the threshold
            if t == E.THRESHOLDS[0]:                                                          # each output alone: the same bits
                for one in ('mean', 'mask', 'stack'):
                    same_bits(run_ensemble(mem, 0, window, acc, t, want=(one,))[one], got[one], what + ' only ' + one)
        mem.frozen.check('ensemble crop')


def test_ensemble_crop_other_class_and_tensor_of_members():
    """cls = 0 decides and stacks channel 0; the Python wrappers on a [K,B,C,H,W] tensor and on a list give the same bits"""
    from salt_amd import ensemble as EN
    H, W, top, left, h, w = E.CROP_CASES[1]
    maps = E.member_maps(3, 2, 2, H, W)
    mem = Members(maps)
    crops = [E.crop(m, top, left, h, w) for m in maps]
    got = run_ensemble(mem, 0, (top, left, h, w), 0, 0.5, cls=0)
    ref = np.mean(np.array(crops), axis=0)
    same_bits(got['mask'], (ref[:, 0] > 0.5).astype(np.uint8), 'cls 0 mask')
    same_bits(got['stack'], E.stack([c[:, 0] for c in crops], 'mhw'), 'cls 0 stack')
    dev = [T(m).to(DEV) for m in maps]
    for probs in (dev, torch.stack(dev)):
        same_bits(EN.fold_mean(probs, target_size=(h, w)).cpu().numpy(), ref, 'fold_mean')
        same_bits(EN.fold_mean(probs, target_size=(h, w), acc='f64').cpu().numpy(),
                  np.mean(np.array([c.astype(np.float64) for c in crops]), axis=0).astype(np.float32), 'fold_mean f64')
        same_bits(EN.fold_masks(probs, target_size=(h, w), threshold=0.47).cpu().numpy(), (ref[:, 1] > np.float32(0.47)).astype(np.uint8), 'fold_masks')
        same_bits(EN.first_level_stack(probs, target_size=(h, w), layout='hwm').cpu().numpy(), E.stack([c[:, 1] for c in crops], 'hwm'), 'stack hwm')
    for bad in (dict(acc='f16'), dict(loader_mode='pad'), dict(target_size=(H + 1, w)), dict(loader_mode='resize', acc='f32')):
        with pytest.raises(EN.SaltError):
            EN.fold_mean(dev, **{**dict(target_size=(h, w)), **bad})
    with pytest.raises(EN.SaltError):
        EN.fold_mean([d.cpu() for d in dev], target_size=(h, w))
    with pytest.raises(EN.SaltError):
        EN.fold_masks(dev, target_size=(h, w), cls=2)
    with pytest.raises(EN.SaltError):
        EN.first_level_stack(dev, target_size=(h, w), out=torch.empty((2, 2, h, w), device=DEV))       # 3 maps into a stack of 2


# ----------------------------------------------------------------------------- salt_ensemble, resized
@pytest.mark.parametrize('K', (1, 2, 7))
@pytest.mark.parametrize('case', E.RESIZE_CASES, ids=['%dx%d-%dx%d' % c for c in E.RESIZE_CASES])
def test_ensemble_resized_is_resize_each_then_mean(case, K):
    H, W, h, w = case
    maps = E.member_maps(K, 2, 2, H, W)
    mem = Members(maps)
    v64 = [E.resized(m, (h, w)) for m in maps]                                                # float64 [B,C,h,w] per member
    ref = E.fold_mean(v64, np.float64)
    assert ref.dtype == np.float64
    window = (0, 0, h, w)
    for t in E.THRESHOLDS:
        what = 'resized %s K=%d t=%g' % (case, K, t)
        got = run_ensemble(mem, 1, window, 1, t)
        same_bits(got['mean'], ref.astype(np.float32), what + ' mean')                        # its single rounding
        same_bits(got['mask'], (ref[:, 1] > t).astype(np.uint8), what + ' mask')
        same_bits(got['stack'], E.stack([v[:, 1] for v in v64], 'mhw'), what + ' stack')
    for one in ('mean', 'mask', 'stack'):
        same_bits(run_ensemble(mem, 1, window, 1, t, want=(one,))[one], got[one], 'resized only ' + one)
    if K == 1:                                                                                # the existing operators on the same map
        out, mask = O.Vec(2 * 2 * h * w), Guarded(2 * h * w, torch.uint8)
        O.call('salt_resize_prob', prob=mem.vecs[0].ptr(), B=2, C=2, H=H, W=W, h=h, w=w, out=out.ptr())
        O.call('salt_resize_threshold', prob=mem.vecs[0].ptr(), B=2, C=2, H=H, W=W, cls=1, h=h, w=w, threshold=float(t), mask=mask.ptr())
        same_bits(got['mean'], out.get((2, 2, h, w)).numpy().astype(np.float32), 'K = 1 against salt_resize_prob')
        same_bits(got['mask'], mask.get((2, h, w)), 'K = 1 against salt_resize_threshold')
        same_bits(got['stack'][:, 0], got['mean'][:, 1], 'K = 1: the stack is the map')
    if (H, W) == (h, w):
        same_bits(got['stack'], E.stack([m[:, 1] for m in maps], 'mhw'), 'equal size: the maps themselves')
    mem.frozen.check('ensemble resized')


# ----------------------------------------------------------------------------- the stack
@pytest.mark.parametrize('mode', (0, 1))
def test_stack_layouts_slices_and_the_stacking_preprocessor(mode):
    from salt_amd.input_pipeline import StackingPreprocessor
    H, W, h, w = 16, 12, 7, 5
    window = (0, 0, h, w) if mode else E.crop_window(H, W, (h, w)) + (h, w)
    for K, M, m0 in ((3, 8, 2), (64, 64, 0), (5, 64, 59)):
        maps = E.member_maps(K, 2, 2, H, W)
        mem = Members(maps)
        vals = [E.resized(m, (h, w))[:, 1] if mode else E.crop(m, *window)[:, 1] for m in maps]
        res = {}
        for layout in ('mhw', 'hwm'):
            got = run_ensemble(mem, mode, window, mode, 0.5, want=('stack',), layout=layout, M=M, m0=m0)['stack']
            want = np.full(got.shape, O.SENTINEL, np.float32)                                 # the other slots keep their sentinel
            if layout == 'mhw':
                want[:, m0:m0 + K] = E.stack(vals, 'mhw')
            else:
                want[..., m0:m0 + K] = E.stack(vals, 'hwm')
            same_bits(got, want, 'stack %s K=%d M=%d m0=%d mode=%d' % (layout, K, M, m0, mode))
            res[layout] = got
        same_bits(np.transpose(res['mhw'], (0, 2, 3, 1)), res['hwm'], 'the two layouts')
        if K == M:                                                                            # a full stack feeds the second-level loader
            a, _ = StackingPreprocessor(size=(16, 16), layout='mhw')(T(res['mhw']).to(DEV))
            b, _ = StackingPreprocessor(size=(16, 16), layout='hwm')(T(E.stack(vals, 'hwm')).to(DEV))          # host-stacked
            assert tuple(a.shape) == (2, 64, 16, 16) and torch.equal(O.bits(a), O.bits(b))


# ----------------------------------------------------------------------------- refusals
def test_ensemble_refusals_touch_nothing():
    maps = E.member_maps(2, 2, 2, 16, 20)
    mem = Members(maps)
    mean, mask, stack = O.Vec(2 * 2 * 9 * 11), Guarded(2 * 9 * 11, torch.uint8), O.Vec(2 * 2 * 9 * 11)
    frozen = O.Frozen(mean=mean.buf, mask=mask.buf, stack=stack.buf)
    good = dict(mode=0, top=3, left=5, h=9, w=11, acc=0, cls=1, threshold=0.5, mean=mean.ptr(), mask=mask.ptr(), stack=stack.ptr(),
                sb=2 * 99, sr=11, sc=1, sm=99, m0=0, **mem.args())
    holed = (ctypes.c_void_p * 2)(mem.vecs[0].ptr(), None)
    cases = [
        (dict(members=None), E_BADARG), (dict(K=0), E_BADARG), (dict(K=65), E_BADARG),
        (dict(members=ctypes.cast(holed, ctypes.c_void_p).value), E_BADARG),
        (dict(top=8), E_BADARG), (dict(left=10), E_BADARG), (dict(top=-1), E_BADARG), (dict(h=17, top=0), E_BADARG),
        (dict(mode=1, acc=1, h=17, top=0, left=0), E_BADARG), (dict(mode=1, acc=1, w=21, top=0, left=0), E_BADARG),
        (dict(mode=1, acc=0), E_UNSUPPORTED), (dict(mode=2), E_BADARG), (dict(acc=2), E_BADARG),
        (dict(cls=2), E_BADARG), (dict(cls=-1), E_BADARG), (dict(mean=None, mask=None, stack=None), E_BADARG),
        (dict(sm=0), E_BADARG), (dict(m0=-1), E_BADARG), (dict(B=0), E_BADARG), (dict(h=0), E_BADARG),
    ]
    for change, code in cases:
        rc = O.raw('salt_ensemble', **{**good, **change})
        assert rc == code, (change, rc)
        assert len(O._abi().lib.salt_last_error()) > 0
    frozen.check('ensemble refusals')
    mem.frozen.check('ensemble refusals')
    O.call('salt_ensemble', **good)                                                           # ... and the unchanged struct is accepted
    counts = Guarded(2, torch.int32)
    rl = dict(mask=mask.ptr(), B=2, h=9, w=11, counts=counts.ptr(), runs=stack.ptr(), cap_pairs=10, total=mean.ptr())
    frozen = O.Frozen(mean=mean.buf, mask=mask.buf, stack=stack.buf, counts=counts.buf)
    for change in (dict(mask=None), dict(counts=None), dict(runs=None), dict(total=None), dict(B=0), dict(h=0), dict(h=300, w=300), dict(cap_pairs=-1)):
        assert O.raw('salt_rle_encode', **{**rl, **change}) == E_BADARG, change
    frozen.check('rle refusals')


# ----------------------------------------------------------------------------- salt_rle_encode
def rle_device(masks, cap=None):
    """masks [B,h,w] uint8 numpy -> (counts [B], total, pairs written (flat ints), cap) through guards; two runs must agree byte for byte"""
    B, h, w = masks.shape
    worst = B * ((h * w + 1) // 2)
    cap = worst if cap is None else cap
    m = Guarded(masks.size, torch.uint8)
    m.win.copy_(T(masks).reshape(-1))
    frozen = O.Frozen(mask=m.buf)
    res = []
    for _ in range(2):
        counts, runs, total = Guarded(B, torch.int32), Guarded(2 * max(cap, 1), torch.int32, fill=-7), Guarded(1, torch.int64)
        O.call('salt_rle_encode', mask=m.ptr(), B=B, h=h, w=w, counts=counts.ptr(), runs=runs.ptr(), cap_pairs=cap, total=total.ptr())
        res.append((counts.get((B,)).copy(), int(total.get((1,))[0]), runs.get((2 * max(cap, 1),)).copy()))
    frozen.check('rle_encode')
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] and res[0][2].tobytes() == res[1][2].tobytes(), 'two runs differ'
    return res[0]


def check_rle(masks, what):
    from salt_amd import inference as I
    host = [I.run_length_encoding(m) for m in masks]
    assert host == [E.run_length_encoding(m) for m in masks]
    counts, total, runs = rle_device(masks)
    assert counts.tolist() == [len(r) // 2 for r in host], what
    assert total == sum(len(r) // 2 for r in host), what
    flat = [v for r in host for v in r]
    assert runs[:2 * total].tolist() == flat, what
    assert (runs[2 * total:] == -7).all(), '%s: pairs written behind the total' % what
    offs = np.concatenate([[0], np.cumsum(counts)]) * 2
    for b, m in enumerate(masks):
        back = I.run_length_decoding(runs[offs[b]:offs[b + 1]].tolist(), m.shape)
        assert np.array_equal(back, (m != 0).astype(np.uint8)), (what, b)
    return total


@pytest.mark.parametrize('shape', E.RLE_SHAPES, ids=['%dx%d' % s for s in E.RLE_SHAPES])
def test_rle_encode_patterns(shape):
    masks = np.stack([E.rle_mask(shape, p) for p in E.RLE_PATTERNS])
    masks[2] *= 255                                                                          # nonzero = set
    check_rle(masks, 'patterns %s' % (shape,))
    n = shape[0] * shape[1]
    counts, total, _ = rle_device(masks[4:5])
    assert counts.tolist() == [(n + 1) // 2] and total == (n + 1) // 2                       # the checkerboard fills the worst case exactly
    both = E.rle_mask(shape, 'first') | E.rle_mask(shape, 'last')
    check_rle(both[None], 'first and last %s' % (shape,))
    # five images with different counts, the random masks at three densities among them
    five = np.stack([E.rle_mask(shape, p) for p in ('random50', 'empty', 'random10', 'columns', 'random90')])
    check_rle(five, 'five %s' % (shape,))


def test_rle_encode_golden_masks():
    f12, f23 = golden('F12_rle'), golden('F23_ensemble')
    for name, masks, fx, first in (('F12', f12['masks'], f12, 0), ('F12 small', f12['small'][None], f12, len(f12['masks'])),
                                   ('F23 1x1', f23['masks_1x1'], f23, 0), ('F23 3x7', f23['masks_3x7'], f23, 5), ('F23 101', f23['masks_101'], f23, 10)):
        counts, total, runs = rle_device(np.ascontiguousarray(masks))
        offs = fx['rle_offsets']
        want = fx['rle_flat'][offs[first]:offs[first + len(masks)]].tolist()                  # what the reference's encoder said
        assert runs[:2 * total].tolist() == want, name
        assert counts.tolist() == [(offs[first + i + 1] - offs[first + i]) // 2 for i in range(len(masks))], name
        check_rle(np.ascontiguousarray(masks), name)


def test_rle_encode_respects_cap_pairs():
    shape = (64, 200)
    masks = np.stack([E.rle_mask(shape, p) for p in ('random50', 'columns', 'random10', 'checker', 'random90')])
    counts, total, full = rle_device(masks)
    for cap in (0, 1, int(counts[0]) - 1, int(counts[0]) + 3, total - 1):
        c2, t2, part = rle_device(masks, cap=cap)
        assert np.array_equal(c2, counts) and t2 == total and total > cap                    # the need is still reported
        assert part[:2 * cap].tolist() == full[:2 * cap].tolist()                            # exactly cap pairs, the guard behind them intact
        assert (part[2 * cap:] == -7).all()


def test_rle_encode_wrapper_and_submission():
    from salt_amd import ensemble as EN, inference as I
    f23 = golden('F23_ensemble')
    masks = f23['masks_101']
    dev = T(masks).to(DEV)
    lists = EN.rle_encode(dev)
    assert lists == [I.run_length_encoding(m) for m in masks]
    assert EN.rle_encode(dev[1]) == [lists[1]]                                               # one [h,w] mask
    assert EN.rle_encode(torch.zeros((3, 5, 4), dtype=torch.uint8, device=DEV)) == [[], [], []]
    ids = f23['sub_ids'].tolist()[10:13]
    rows = EN.create_submission(ids, dev)
    assert rows == list(zip(ids, f23['sub_rle'].tolist()[10:13])) == E.submission_rows(ids, masks)
    for (_, s), m in zip(rows, masks):
        assert np.array_equal(I.run_length_decoding(s, m.shape), m)
    with pytest.raises(EN.SaltError):
        EN.rle_encode(torch.zeros((1, 300, 300), dtype=torch.uint8, device=DEV))


# ----------------------------------------------------------------------------- FoldEnsemble
def _tiles(B, n, seed):
    return np.random.RandomState(seed).randint(0, 256, (B, n, n)).astype(np.uint8)


def _nets(seeds):
    from salt_amd import architectures as A
    nets = []
    for s in seeds:
        torch.manual_seed(s)
        nets.append(A.VanillaUNet(2, in_channels=1, base_filters=8, levels=3).to(DEV).eval())
    return nets


def test_fold_ensemble_crop_mode():
    from salt_amd import architectures as A, ensemble as EN, inference as I
    from salt_amd.input_pipeline import DevicePreprocessor, StackingPreprocessor
    nets = _nets((11, 12, 13))
    pre = DevicePreprocessor(False, 1)
    xi = T(_tiles(4, 101, 21)).to(DEV)
    ens = EN.FoldEnsemble(nets, pre)
    own = [I.predict_tta_tiles(n, pre, xi) for n in nets]                                     # the members' own outputs, [4,2,128,128]
    assert tuple(own[0].shape) == (4, 2, 128, 128) and not torch.equal(own[0], own[1])
    got = ens.predict(xi)
    assert tuple(got.shape) == (4, 2, 101, 101) and torch.equal(O.bits(got), O.bits(EN.fold_mean(own)))
    host = [o.cpu().numpy()[:, :, 13:114, 14:115] for o in own]
    ref = np.mean(np.array(host), axis=0)
    same_bits(got.cpu().numpy(), ref, 'FoldEnsemble.predict')
    for t in (0.5, 0.47):
        same_bits(ens.predict_masks(xi, threshold=t).cpu().numpy(), (ref[:, 1] > t).astype(np.uint8), 'FoldEnsemble.predict_masks %g' % t)
    ref64 = np.mean(np.array([h_.astype(np.float64) for h_ in host]), axis=0)
    same_bits(ens.predict(xi, acc='f64').cpu().numpy(), ref64.astype(np.float32), 'FoldEnsemble.predict f64')
    # first-level stack -> second-level loader -> second-level network, against the same network on the host-assembled stack
    stack = ens.predict_stack(xi)
    assert tuple(stack.shape) == (4, 3, 101, 101)
    same_bits(stack.cpu().numpy(), E.stack([h_[:, 1] for h_ in host], 'mhw'), 'FoldEnsemble.predict_stack')
    same_bits(ens.predict_stack(xi, layout='hwm').cpu().numpy(), E.stack([h_[:, 1] for h_ in host], 'hwm'), 'FoldEnsemble.predict_stack hwm')
    torch.manual_seed(5)
    fcn = A.StackingFCN(3, 2).to(DEV).eval()
    with torch.no_grad():
        a = fcn(StackingPreprocessor(layout='mhw')(stack)[0]).float()
        b = fcn(StackingPreprocessor(layout='hwm')(T(E.stack([h_[:, 1] for h_ in host], 'hwm')).to(DEV))[0]).float()
    assert tuple(a.shape) == (4, 2, 128, 128) and bool(torch.isfinite(a).all()) and torch.equal(O.bits(a), O.bits(b))
    # submission round trip
    masks = ens.predict_masks(xi, threshold=float(np.median(ref[:, 1])))                     # about half of the pixels set
    rows = EN.create_submission(['a', 'b', 'c', 'd'], masks)
    for (_, s), m in zip(rows, masks.cpu().numpy()):
        assert np.array_equal(I.run_length_decoding(s, m.shape), m)
    assert 0 < int(masks.sum()) < masks.numel()                                              # neither empty nor full: the round trip says something
    # refusals
    class Deep(A.VanillaUNet):
        uses_depth = True
    with pytest.raises(EN.SaltError):
        EN.FoldEnsemble([nets[0], Deep(2, in_channels=1, base_filters=8, levels=3).to(DEV).eval()], pre)
    with pytest.raises(EN.SaltError):
        EN.FoldEnsemble([], pre)
    with pytest.raises(EN.SaltError):
        EN.FoldEnsemble(nets, pre, loader_mode='resize').predict(xi)                          # the preprocessor is a resize_and_pad one


def test_fold_ensemble_resize_mode():
    from salt_amd import ensemble as EN, inference as I
    from salt_amd.input_pipeline import DevicePreprocessor
    nets = _nets((11, 12, 13))
    pre = DevicePreprocessor(False, 1, resize=128, loader_mode='resize')
    xi = T(_tiles(4, 101, 22)).to(DEV)
    ens = EN.FoldEnsemble(nets, pre, loader_mode='resize')
    own = [I.predict_tta_tiles(n, pre, xi, loader_mode='resize', resize_back=False) for n in nets]
    assert tuple(own[0].shape) == (4, 2, 128, 128)
    v64 = [L.resize_back(o.cpu().double().numpy(), (101, 101)) for o in own]
    ref = E.fold_mean(v64, np.float64)
    same_bits(ens.predict(xi).cpu().numpy(), ref.astype(np.float32), 'FoldEnsemble.predict resize')
    same_bits(ens.predict_masks(xi, threshold=0.47).cpu().numpy(), (ref[:, 1] > 0.47).astype(np.uint8), 'FoldEnsemble.predict_masks resize')
    same_bits(ens.predict_stack(xi).cpu().numpy(), E.stack([v[:, 1] for v in v64], 'mhw'), 'FoldEnsemble.predict_stack resize')
    # resize_back's default is today's behaviour: the member's own resized map is K = 1 of the ensemble
    one = I.predict_tta_tiles(nets[0], pre, xi, loader_mode='resize')
    assert torch.equal(O.bits(one), O.bits(EN.fold_mean(own[:1], 'resize')))
