"""CPU tests of the loader modes 'resize' / 'stacking' and the reflect pad: the float64 restatements (loader_modes_reference.py) against
the libraries that can be executed (scipy.ndimage for R1 / R2, PIL for R3, np.pad for R5), the fitness of the case table the GPU tests
compare on, and the host logic (geometry, refusals, which validation path is taken)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

import loader_modes_reference as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'F22_loader_modes.npz')


def _scipy(P, size_out, mode):
    h, w = P.shape
    rr, cc = np.meshgrid(L.src_coords(h, size_out[0]), L.src_coords(w, size_out[1]), indexing='ij')
    return ndimage.map_coordinates(P.astype(np.float64), [rr, cc], order=1, mode=mode, cval=0.0)


@pytest.mark.parametrize('hw,HW', L.STACK_SIZES)
def test_r1_is_scipy_grid_constant(hw, HW):
    x = L.stack_case(hw, 5, 1)
    got = L.stack_resize(x, HW)[0]
    g = np.load(GOLDEN)['r1_%dx%d_%dx%d' % (hw + HW)]
    for m in range(5):
        ref = _scipy(x[0, :, :, m], HW, 'grid-constant')
        assert np.abs(got[m] - ref).max() <= 1e-14
        assert np.array_equal(ref[L.golden_rows(HW[0])], g[m])                    # the stored vectors are scipy's
    if HW[0] > hw[0]:                                                             # an up-scale blends its border with the zero outside
        ones = L.resize_map(np.ones(hw), HW)
        assert ones[0, 0] < 0.95 and ones[HW[0] // 2, HW[1] // 2] == 1.0


@pytest.mark.parametrize('HW,hw', L.PROB_SIZES)
def test_r2_is_scipy_constant_and_stays_inside(HW, hw):
    p = L.prob_case(HW, 2, 1)
    got = L.resize_back(p, hw)[0]
    g = np.load(GOLDEN)['r2_%dx%d_%dx%d' % (HW + hw)]
    for c in range(2):
        ref = _scipy(p[0, c], hw, 'constant')
        assert np.abs(got[c] - ref).max() <= 1e-14
        assert np.array_equal(ref[L.golden_rows(hw[0])], g[c])
    for n_in, n_out in zip(HW, hw):                                               # every coordinate of a down-scale lies in the source
        r = L.src_coords(n_in, n_out)
        assert r.min() >= 0.0 and r.max() <= n_in - 1
    if HW == (128, 128):
        r = L.src_coords(128, 101)
        assert abs(r.min() - 0.1337) < 1e-4 and abs(r.max() - 126.8663) < 1e-4
    if HW == hw:                                                                  # integer coordinates: the identity, bit for bit
        assert np.array_equal(got, p[0].astype(np.float64))


def test_r2_refuses_an_upscale():
    with pytest.raises(ValueError):
        L.resize_back(np.zeros((1, 8, 8)), (9, 8))


@pytest.mark.parametrize('n,N', L.MASK_SIZES)
@pytest.mark.parametrize('kind', L.MASK_KINDS)
def test_r3_is_pil_bilinear(n, N, kind):
    g = np.load(GOLDEN)
    masks = L.mask_case(n, kind)
    assert np.array_equal(masks, g['mask_%d_%d_%s' % (n, N, kind)])
    got, sums = L.mask_target(masks, (N, N), with_sums=True)
    assert got.dtype == np.float32 and got.shape == (masks.shape[0], 2, N, N)
    for b, m in enumerate(masks):
        for k in (0, 1):
            im = Image.fromarray((m == k).astype(np.uint8)).resize((N, N), Image.BILINEAR).convert('L')
            assert np.array_equal(np.asarray(im, dtype=np.float32), got[b, k]), (n, N, kind, b, k)
    assert np.array_equal(got, g['pil_%d_%d_%s' % (n, N, kind)].astype(np.float32))
    # fitness: no weighted sum of either pass sits near a rounding tie, so summation order cannot decide a pixel
    assert L.tie_distance(sums) >= 1e-6


def test_r3_passes_are_not_one_float_pass():
    """the horizontal intermediate is rounded onto the uint8 grid: a single float pass over both axes gives other pixels"""
    masks = L.mask_case(101, 'noise')
    got = L.mask_target(masks, (128, 128))
    assert set(np.unique(got)) <= {0.0, 1.0}
    start, length, weights = L.pil_axis_table(101, 128)
    dense = np.zeros((128, 101))
    for x in range(128):
        dense[x, start[x]:start[x] + length[x]] = weights[x, :length[x]]
    one_pass = np.floor(dense @ (masks == 1).astype(np.float64) @ dense.T + 0.5)
    differ = int((one_pass != got[:, 1]).sum())
    assert 0 < differ < 0.1 * one_pass.size, differ


def test_the_wrapper_builds_the_same_tables():
    from salt_amd import input_pipeline as IP
    for n_in, n_out in [(101, 128), (101, 256), (7, 16), (5, 8), (32, 32), (128, 101), (9, 8), (256, 8)]:
        for a, b in zip(L.pil_axis_table(n_in, n_out), IP.pil_resize_table(n_in, n_out)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        start, length, weights = IP.pil_resize_table(n_in, n_out)
        assert (start >= 0).all() and (length >= 1).all() and (start + length <= n_in).all() and (length <= weights.shape[1]).all()
        assert np.abs(weights.sum(1) - 1).max() < 1e-15


@pytest.mark.parametrize('n,pads', [(102, (13, 13, 13, 13)), (101, (13, 14, 14, 13)), (15, (13, 13, 13, 13)), (14, (13, 13, 0, 1)), (1, (0, 0, 0, 0))])
def test_r5_is_numpy_reflect(n, pads):
    a = np.random.RandomState(n).randint(0, 256, (2, n, n)).astype(np.uint8)
    t, b, l, r = pads
    assert np.array_equal(L.reflect_pad(a, t, b, l, r), np.pad(a, ((0, 0), (t, b), (l, r)), mode='reflect'))
    assert np.array_equal(L.edge_pad(a, t, b, l, r), np.pad(a, ((0, 0), (t, b), (l, r)), mode='edge'))
    if n > 1:
        with pytest.raises(ValueError):
            L.reflect_pad(a, n, 0, 0, 0)


def test_probability_cases_decide_far_from_every_threshold():
    """|v64 - t| >= 1e-9 for every probability case and every threshold the GPU tests sweep (the 21 of the reference among them): a
    kernel that evaluates the pinned float64 formula cannot land on the other side."""
    assert np.array_equal(L.THRESHOLDS[21], np.linspace(0.5, 0.3, 21))
    for HW, hw in L.PROB_SIZES:
        for C in (1, 2):
            for B in L.BATCHES:
                v = L.resize_back(L.prob_case(HW, C, B), hw)
                for th in L.THRESHOLDS.values():
                    assert np.abs(v[..., None] - th).min() >= 1e-9, (HW, hw, C, B)


# ----------------------------------------------------------------------------- host logic
def test_geometry_and_refusals_of_the_preprocessor():
    from salt_amd import input_pipeline as IP
    from salt_amd._abi import SaltError
    for train in (True, False):
        pre = IP.DevicePreprocessor(train, 3, resize=128, loader_mode='resize')
        assert pre.geometry(101, 101) == (128, 128, 0, 0, 128, 128)               # R4: scaled, not padded, in both branches
        assert pre.geometry(128, 128) == (0, 0, 0, 0, 128, 128)
    assert IP.DevicePreprocessor(True, 3).geometry(101, 101) == (102, 102, 13, 13, 128, 128)
    assert IP.DevicePreprocessor(False, 3, pad_method='reflect').geometry(101, 101) == (0, 0, 13, 14, 128, 128)
    with pytest.raises(SaltError, match='loader_mode'):
        IP.DevicePreprocessor(True, 3, loader_mode='stacking')
    with pytest.raises(SaltError, match='pad_method'):
        IP.DevicePreprocessor(True, 3, pad_method='symmetric')
    pre = IP.DevicePreprocessor(False, 1, pad_method='reflect')
    pre._check_pad(15, 15, 0, 0, 13, 13, 41, 41)                                  # pad 13 on a 15-pixel tile still reflects
    with pytest.raises(SaltError, match='n - 1'):
        pre._check_pad(14, 14, 0, 0, 14, 14, 42, 42)
    with pytest.raises(SaltError, match='n - 1'):
        pre._check_pad(10, 10, 0, 0, *pre.geometry(10, 10)[2:])                   # 10 -> 64: pad 27 on each side
    IP.DevicePreprocessor(False, 1)._check_pad(10, 10, 0, 0, 27, 27, 64, 64)      # the edge pad has no such limit
    with pytest.raises(SaltError, match='GPU'):
        pre(torch.zeros(1, 101, 101, dtype=torch.uint8))
    sp = IP.StackingPreprocessor()
    assert sp.size == (128, 128)
    with pytest.raises(SaltError, match='GPU'):
        sp(torch.zeros(1, 101, 101, 5))
    with pytest.raises(SaltError, match='layout'):
        IP.StackingPreprocessor(layout='nhwc')
    assert sp._layout((2, 101, 101, 5)) == 'hwm' and sp._layout((2, 5, 101, 101)) == 'mhw'
    with pytest.raises(SaltError, match='layout'):
        sp._layout((2, 64, 64, 64))


def test_the_library_refuses_before_it_launches():
    from salt_amd import _abi as abi
    from salt_amd import inference as I
    BAD = abi.CONSTS['SALT_E_BADARG']
    P = 1 << 20                                                                   # never dereferenced: every call below is refused on the host
    assert abi.lib.salt_abi_version() >= 33
    for s in ('salt_stack_resize', 'salt_mask_resize', 'salt_resize_prob', 'salt_resize_threshold', 'salt_resize_iou_sweep'):
        assert s in abi.DECLARED_SYMBOLS and s in abi.OP_FUNCS
    call = lambda name, **kw: abi.OP_FUNCS[name][0](ctypes.byref(abi.fill(abi.OP_FUNCS[name][1](), **kw)), None)
    pre = dict(img=P, img_is_u8=1, B=1, channels=1, mean=[0.5] * 3, std=[0.25] * 3, x=P)
    assert call('salt_preprocess', h=14, w=14, top=14, left=14, H=42, W=42, pad_mode=1, **pre) == BAD
    assert b'n - 1' in abi.lib.salt_last_error()
    assert call('salt_preprocess', h=101, w=101, top=13, left=14, H=128, W=128, pad_mode=2, **pre) == BAD
    assert call('salt_preprocess', h=101, w=101, resize_h=102, resize_w=102, top=13, left=13, H=231, W=128, pad_mode=1, interpolation=2, **pre) == BAD
    aug = dict(img=P, B=1, channels=1, mean=[0.5] * 3, std=[0.25] * 3, x=P)
    assert call('salt_augment_preprocess', h=14, w=14, top=14, left=14, H=42, W=42, pad_mode=1, **aug) == BAD
    assert b'n - 1' in abi.lib.salt_last_error()
    st = dict(x=P, y=P, B=1, h=101, w=101, H=128, W=128)
    assert call('salt_stack_resize', M=65, sb=101 * 101 * 65, sr=101 * 65, sc=65, sm=1, **st) == BAD
    assert b'M <= 64' in abi.lib.salt_last_error()
    assert call('salt_stack_resize', M=0, sb=1, sr=1, sc=1, sm=1, **st) == BAD
    assert call('salt_stack_resize', M=4, sb=101 * 101 * 8, sr=101 * 8, sc=8, sm=2, **st) == BAD      # neither maps nor columns innermost
    assert call('salt_stack_resize', M=4, sb=4 * 300 * 300, sr=300, sc=1, sm=300 * 300, x=P, y=P, B=1, h=300, w=300, H=128, W=128) == BAD
    down = dict(prob=P, B=1, C=2, H=101, W=101, h=128, w=128)
    assert call('salt_resize_prob', out=P, **down) == BAD and b'up-scale' in abi.lib.salt_last_error()
    assert call('salt_resize_threshold', mask=P, cls=1, threshold=0.5, **down) == BAD and b'up-scale' in abi.lib.salt_last_error()
    th = (ctypes.c_double * 2)(0.5, 0.4)
    sweep = dict(gt=P, T=2, thresholds=ctypes.cast(th, ctypes.c_void_p).value, inter=P, pred=P, gt_count=P, cls=1)
    assert call('salt_resize_iou_sweep', **sweep, **down) == BAD and b'up-scale' in abi.lib.salt_last_error()
    assert call('salt_resize_iou_sweep', **dict(sweep, T=33), **dict(down, h=101, w=101)) == BAD
    assert call('salt_resize_threshold', mask=P, cls=2, threshold=0.5, **dict(down, h=101, w=101)) == BAD
    for fn in (I.resize_image, I.resize_threshold):
        with pytest.raises(abi.SaltError, match='GPU'):
            fn(torch.zeros(1, 2, 128, 128), (101, 101))
    with pytest.raises(abi.SaltError, match='GPU'):
        I.iou_counts_resized(torch.zeros(1, 2, 128, 128), torch.zeros(1, 101, 101, dtype=torch.uint8), [0.5])


class _Net:
    training = False
    uses_depth = False

    def eval(self):
        return self

    def train(self):
        return self

    def __call__(self, X):
        return X[:, :2] * 4 - 2


class _Transformer:
    def __init__(self):
        self.model, self.optimizer, self.validation_loss = _Net(), None, {}
        self.loss_function = [('mask', lambda logits, target: (logits - target).abs().mean(), 1.0)]
        self.output_names = ['mask']

    def _to_device(self):
        return torch.device('cpu')


def test_score_validation_takes_the_resized_path_only_with_original_size_masks(monkeypatch):
    """loader_mode 'stacking' / 'resize' AND original-size masks -> the probabilities are resized back and swept against those masks;
    every other combination is the path of before (the batches' own targets on the centre crop)."""
    from salt_amd import callbacks as C
    from salt_amd import inference as I
    calls = []

    def crop(prob, gt, thresholds, cls=1):
        calls.append(('crop', tuple(gt.shape)))
        return L.counts(prob[:, cls, 13:13 + gt.shape[1], 14:14 + gt.shape[2]].double().numpy(), gt.numpy(), thresholds)

    def resized(prob, gt, thresholds, cls=1):
        calls.append(('resized', tuple(gt.shape)))
        return L.counts(L.resize_back(prob[:, cls].double().numpy(), gt.shape[1:]), gt.numpy(), thresholds)

    monkeypatch.setattr(I, 'iou_counts', crop)
    monkeypatch.setattr(I, 'iou_counts_resized', resized)
    g = torch.Generator().manual_seed(3)
    X = [torch.rand(2, 5, 128, 128, generator=g) for _ in range(2)]
    T = [(torch.rand(2, 2, 128, 128, generator=g) < 0.4).float() for _ in range(2)]
    datagen = lambda: (iter(list(zip(X, T))), 1)
    y_true = L.gt_case((101, 101), 4)
    tr = _Transformer()
    before = C.score_validation(tr, datagen())
    assert calls == [('crop', (2, 101, 101))] * 2
    for kw in ({'loader_mode': 'stacking'}, {'loader_mode': 'resize'}, {'loader_mode': 'resize_and_pad', 'y_true': y_true}, {'loader_mode': None}):
        del calls[:]
        again = C.score_validation(tr, datagen(), **kw)
        assert calls == [('crop', (2, 101, 101))] * 2, kw
        assert all(torch.equal(before[k], again[k]) for k in before), kw
    for mode in C.RESIZED_MODES:
        for masks in (y_true, torch.from_numpy(y_true)):
            del calls[:]
            val = C.score_validation(tr, datagen(), loader_mode=mode, y_true=masks)
            assert calls == [('resized', (2, 101, 101))] * 2
            prob = torch.sigmoid(torch.cat([tr.model(x) for x in X]))
            cnt = L.counts(L.resize_back(prob[:, 1].double().numpy(), (101, 101)), y_true, L.SWEEP)
            t_best, iou, iout = I.select_threshold([cnt], L.SWEEP)
            assert abs(float(val['iou']) - iou) < 1e-6 and abs(float(val['iout']) - iout) < 1e-6 and tr.best_threshold == t_best
            assert torch.equal(val['sum'], before['sum'])                        # the loss is the batches' own either way
    with pytest.raises(C.SaltError):
        C.score_validation(tr, datagen(), loader_mode='stacking', y_true=y_true[:3])          # fewer masks than validation tiles
    with pytest.raises(C.SaltError):
        C.score_validation(tr, datagen(), loader_mode='stacking', y_true=y_true.astype(np.float32))
    # the monitor hands the masks to the transformer, which every callback's shared validation pass goes through
    for mode, meta, want in (('stacking', y_true, True), ('resize', torch.from_numpy(y_true), True), ('stacking', None, False),
                             ('stacking', 'meta.csv', False), ('resize_and_pad', y_true, False), (None, y_true, False)):
        tr = _Transformer()
        C.ValidationMonitor(loader_mode=mode).set_params(tr, validation_datagen=None, meta_valid=meta)
        assert (tr.validation_masks is not None) == want, (mode, type(meta))
        if want:
            assert tr.validation_masks[0] == mode and tuple(tr.validation_masks[1].shape) == (4, 101, 101)
