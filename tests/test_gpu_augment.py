"""GPU tests of the on-device training augmentation (DevicePreprocessor(augment=...), salt_augment_preprocess) against the numpy
restatement in tests/aug_reference.py."""
import numpy as np
import pytest
import torch

import aug_reference as R
from helpers import T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _tiles(B, seed=0, h=101, w=101):
    """smooth gray tiles with texture + blob masks: what salt tiles look like"""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((B, h, w), np.uint8)
    msk = np.zeros((B, h, w), np.uint8)
    for b in range(B):
        f = 120 + 60 * np.sin(xx / r.uniform(4, 15) + r.uniform(0, 6)) * np.cos(yy / r.uniform(4, 15)) + r.normal(0, 8, (h, w))
        img[b] = np.clip(f, 0, 255).astype(np.uint8)
        if b % 4:
            msk[b] = (((yy - r.uniform(0, h)) / r.uniform(10, 50)) ** 2 + ((xx - r.uniform(0, w)) / r.uniform(10, 50)) ** 2 <= 1)
    return img, msk


def _pre(cfg, **kw):
    from salt_amd.input_pipeline import DevicePreprocessor
    return DevicePreprocessor(True, kw.pop('channels', 3), augment=cfg, **kw)


def _none(*ops):
    from salt_amd.input_pipeline import AugmentConfig
    return AugmentConfig.none(enable=tuple(ops))


@pytest.mark.parametrize('channels', [1, 3])
@pytest.mark.parametrize('B', [1, 5, 257])
def test_every_op_disabled_is_the_plain_preprocessing_bit_for_bit(channels, B):
    from salt_amd.input_pipeline import DevicePreprocessor
    img, msk = _tiles(B, 1)
    xi, mi = T(img).to(DEV), T(msk).to(DEV)
    x0, t0 = DevicePreprocessor(True, channels)(xi, mi)
    x1, t1 = _pre(_none(), channels=channels)(xi, mi)
    assert torch.equal(x0, x1) and torch.equal(t0, t1)
    x2, t2 = _pre(_none(), channels=channels)(xi)
    assert t2 is None and torch.equal(x2, x0)


def _replay(rows, img, msk, cfg=None, seed=5, counter=0):
    from salt_amd.input_pipeline import AugmentConfig
    pre = _pre(cfg or AugmentConfig(), seed=seed)
    pre.counter = counter
    x, t, dbg = pre(T(img).to(DEV), T(msk).to(DEV), params=T(rows).to(DEV), debug=True)
    return x.cpu().numpy(), t.cpu().numpy(), {k: v.cpu().numpy() for k, v in dbg.items()}


def _row(**kv):
    p = np.zeros(64, np.float32)
    slots = {'order': 0, 'n': 1, 'flip': 6, 'angle': 7, 'shift': 8, 'pw': 9, 'ps': 43, 'invert': 53, 'contrast': 54, 'alpha': 55, 'op': 56, 'value': 57}
    for k, v in kv.items():
        if k == 'chosen':
            p[2 + v] = 1
        elif k == 'jitter':
            p[11:43] = np.asarray(v, np.float32).reshape(32)
        elif k == 'corners':
            p[45:53] = np.asarray(v, np.float32).reshape(8)
        else:
            p[slots[k]] = v
    return p


def _check_geo(rows, img, msk, exact):
    x, t, dbg = _replay(rows, img, msk)
    bad_img, n_img = 0, 0
    for b in range(len(rows)):
        gi, gm, bands = R.geometric(img[b], msk[b], rows[b])
        if exact:
            assert np.array_equal(dbg['geo_img'][b], gi), b
            assert np.array_equal(dbg['geo_mask'][b], gm), b
        else:
            d = np.abs(dbg['geo_img'][b].astype(int) - gi.astype(int))
            assert d.max() <= 1, (b, int(d.max()))
            bad_img += int((d > 0).sum()); n_img += d.size
            near = np.zeros(gm.shape, bool)
            for mv in bands[-1:]:
                near |= np.abs(mv - 0.5) < 1e-3
            assert np.array_equal(dbg['geo_mask'][b][~near], gm[~near]), b
    if not exact:
        assert bad_img <= 1e-3 * n_img, (bad_img, n_img)
    return x, t, dbg


def test_flip_sharpen_emboss_are_exact_in_replay():
    img, msk = _tiles(6, 2)
    rows = np.stack([_row(n=1, chosen=0, flip=1), _row(n=1, chosen=0, flip=0), _row(n=1, chosen=1), _row(n=1, chosen=2),
                     _row(n=2, chosen=0, flip=1) + _row(chosen=2), _row(n=2, chosen=1) + _row(chosen=2)])
    _check_geo(rows, img, msk, exact=True)


def test_warps_match_the_restatement_in_replay():
    img, msk = _tiles(6, 3)
    r = np.random.RandomState(3)
    rows = [_row(n=1, chosen=3, angle=7.3, shift=0.031), _row(n=1, chosen=3, angle=-9.9, shift=-0.05),
            _row(pw=1, jitter=r.normal(0, 0.06, 32)), _row(pw=1, jitter=r.normal(0, 0.04, 32)),
            _row(ps=1, corners=np.mod(np.abs(r.normal(0, 0.08, 8)), 1)), _row(ps=1, corners=np.mod(np.abs(r.normal(0, 0.1, 8)), 1))]
    _check_geo(np.stack(rows), img, msk, exact=False)


def test_whole_sequences_in_every_stage_order():
    img, msk = _tiles(6, 4)
    r = np.random.RandomState(4)
    rows = []
    for order in range(6):
        p = _row(order=order, n=2, chosen=0, flip=1, pw=1, jitter=r.normal(0, 0.05, 32), ps=1, corners=np.mod(np.abs(r.normal(0, 0.07, 8)), 1))
        p[2 + (1 + order % 3)] = 1                                          # + Sharpen / Emboss / Affine
        p[7], p[8] = 5.0, 0.02
        rows.append(p)
    x, t, dbg = _replay(np.stack(rows), img, msk)
    for b in range(6):
        gi, gm, _ = R.geometric(img[b], msk[b], rows[b])
        d = np.abs(dbg['geo_img'][b].astype(int) - gi.astype(int))
        assert (d > 1).mean() < 0.01 and (d > 0).mean() < 0.05, b          # three warps in a row: differences may carry on
        assert (dbg['geo_mask'][b] != gm).mean() < 0.01, b


@pytest.mark.parametrize('op,value', [('invert', None), ('contrast', 0.62), ('contrast', 1.43), ('add', -7), ('add', 10), ('add_elementwise', None),
                                      ('multiply', 1.037), ('multiply', 0.951), ('multiply_elementwise', None), ('all', 1.21)])
def test_intensity_ops_are_exact_in_replay(op, value):
    img, msk = _tiles(4, 5)
    kw = {'invert': dict(invert=1), 'contrast': dict(contrast=1, alpha=value or 0), 'add': dict(op=1, value=value or 0),
          'add_elementwise': dict(op=2), 'multiply': dict(op=3, value=value or 0), 'multiply_elementwise': dict(op=4),
          'all': dict(invert=1, contrast=1, alpha=value or 0, op=4)}[op]
    rows = np.stack([_row(**kw)] * 4)
    x, t, dbg = _replay(rows, img, msk, seed=11, counter=3)
    for b in range(4):
        g = R.intensity(R.resize_pad(img[b]), rows[b], 11, 3, b)
        assert np.array_equal(dbg['gray'][b], g), (op, b, int((dbg['gray'][b] != g).sum()))
        assert np.array_equal(x[b, 0], R.normalise(g)), b


def test_draw_then_replay_is_bit_identical():
    from salt_amd.input_pipeline import AugmentConfig
    img, msk = _tiles(64, 6)
    xi, mi = T(img).to(DEV), T(msk).to(DEV)
    pre = _pre(AugmentConfig(), seed=21, record_params=True)
    x, t, dbg = pre(xi, mi, debug=True)
    rec = pre.last_params(raw=True).clone()
    rep = _pre(AugmentConfig(), seed=21)
    x2, t2, dbg2 = rep(xi, mi, params=rec, debug=True)
    assert torch.equal(x, x2) and torch.equal(t, t2)
    for k in dbg:
        assert torch.equal(dbg[k], dbg2[k]), k


def test_fused_output_equals_plain_preprocessing_of_the_debug_tiles():
    from salt_amd.input_pipeline import AugmentConfig, DevicePreprocessor, AUG_OPS
    img, msk = _tiles(32, 7)
    xi, mi = T(img).to(DEV), T(msk).to(DEV)
    geo_only = AugmentConfig(enable=AUG_OPS[:6], p_piecewise=0.6, p_perspective=0.6)
    x, t, dbg = _pre(geo_only, seed=3)(xi, mi, debug=True)
    xp, tp = DevicePreprocessor(True, 3)(dbg['geo_img'], dbg['geo_mask'])
    assert torch.equal(t, tp) and torch.equal(x, xp)
    pre = _pre(AugmentConfig(p_invert=0.5, p_contrast=0.5), seed=4, record_params=True)
    x, t, dbg = pre(xi, mi, debug=True)
    rows = pre.last_params(raw=True).cpu().numpy()
    xp, tp = DevicePreprocessor(True, 3)(dbg['geo_img'], dbg['geo_mask'])
    assert torch.equal(t, tp)
    xc, gray, geo = x.cpu().numpy(), dbg['gray'].cpu().numpy(), dbg['geo_img'].cpu().numpy()
    for b in range(32):
        assert np.array_equal(xc[b, 0], R.normalise(gray[b])), b
        assert np.array_equal(gray[b], R.intensity(R.resize_pad(geo[b]), rows[b], 4, 0, b)), b


def test_distributions_of_the_drawn_parameters():
    from salt_amd.input_pipeline import AugmentConfig
    B = 8192
    img, msk = _tiles(8, 8)
    xi, mi = T(np.repeat(img, B // 8, 0)).to(DEV), T(np.repeat(msk, B // 8, 0)).to(DEV)
    pre = _pre(AugmentConfig(), seed=99, record_params=True)
    x, t, dbg = pre(xi, mi, debug=True)
    d = pre.last_params()

    def near(k, p, n=B):
        assert abs(k - n * p) <= 4 * np.sqrt(n * p * (1 - p)) + 1, (k, n, p)
    for o in range(6):
        near(int((d['order'] == o).sum()), 1 / 6)
    near(int((d['n'] == 1).sum()), 0.5)
    assert set(np.unique(d['n'])) == {1, 2} and np.array_equal(d['chosen'].sum(1), d['n'])
    for c in range(4):
        near(int(d['chosen'][:, c].sum()), 3 / 8)
    ch = d['chosen'][:, 0]
    near(int(d['flip'][ch].sum()), 0.5, int(ch.sum()))
    near(int(d['flip'].sum()), 3 / 16)
    assert not d['flip'][~ch].any()
    for k in ('piecewise', 'perspective', 'invert', 'contrast'):
        near(int(d[k].sum()), 0.3)
    near(int((d['intensity_op'] == 0).sum()), 0.5)
    for o in range(1, 5):
        near(int((d['intensity_op'] == o).sum()), 1 / 8)
    aff = d['chosen'][:, 3]
    a, s = d['angle'][aff], d['shift'][aff]
    assert a.min() >= -10 and a.max() <= 10 and abs(a.mean()) < 4 * 20 / np.sqrt(12 * len(a))
    assert s.min() >= -0.05 and s.max() <= 0.05 and abs(s.mean()) < 4 * 0.1 / np.sqrt(12 * len(s))
    ps = d['piecewise_scale'][d['piecewise']]
    assert ps.min() >= 0.04 and ps.max() <= 0.08 and abs(ps.mean() - 0.06) < 4 * 0.04 / np.sqrt(12 * len(ps))
    jit = d['piecewise_jitter'][d['piecewise']].reshape(len(ps), -1) / ps[:, None]
    assert abs(jit.mean()) < 0.01 and abs(jit.std() - 1) < 0.02                          # N(0, s)
    pp = d['perspective_scale'][d['perspective']]
    assert pp.min() >= 0.05 and pp.max() <= 0.1 and abs(pp.mean() - 0.075) < 4 * 0.05 / np.sqrt(12 * len(pp))
    cr = d['perspective_corners'][d['perspective']]
    assert cr.min() >= 0 and cr.max() < 1
    al = d['contrast_alpha'][d['contrast']]
    assert al.min() >= 0.5 and al.max() <= 1.5 and abs(al.mean() - 1) < 4 / np.sqrt(12 * len(al))
    av = d['value'][d['intensity_op'] == 1]
    assert np.array_equal(av, np.round(av)) and av.min() == -10 and av.max() == 10
    mv = d['value'][d['intensity_op'] == 3]
    assert mv.min() >= 0.95 and mv.max() <= 1.05 and abs(mv.mean() - 1) < 4 * 0.1 / np.sqrt(12 * len(mv))
    assert not d['value'][np.isin(d['intensity_op'], (0, 2, 4))].any()
    # per-pixel noise bounds: AddElementwise moves a pixel by at most 10 levels, MultiplyElementwise by at most 5 % (+ rounding)
    raw = pre.last_params(raw=True)
    for op in (2, 4):
        sel = np.nonzero((d['intensity_op'][:64] == op) & ~d['invert'][:64] & ~d['contrast'][:64])[0]
        if len(sel) == 0:
            continue
        rows = raw[:64].cpu().numpy()
        for b in sel[:4]:
            g0 = R.intensity(R.resize_pad(dbg['geo_img'][b].cpu().numpy()), rows[b], 99, 0, b)
            assert np.array_equal(dbg['gray'][b].cpu().numpy(), g0)
            ref = R.resize_pad(dbg['geo_img'][b].cpu().numpy()).astype(int)
            diff = dbg['gray'][b].cpu().numpy().astype(int) - ref
            if op == 2:
                assert np.abs(diff).max() <= 10 and len(np.unique(diff[(ref >= 10) & (ref <= 245)])) == 21
            else:
                assert np.all(np.abs(diff) <= np.ceil(ref * 0.05) + 1)
    m = dbg['geo_mask']
    assert int(((m != 0) & (m != 1)).sum()) == 0
    assert torch.equal(t[:, 0], 1 - t[:, 1]) and set(torch.unique(t).tolist()) <= {0.0, 1.0}


def test_determinism_and_seeding():
    img, msk = _tiles(16, 9)
    xi, mi = T(img).to(DEV), T(msk).to(DEV)
    a = _pre(True, seed=5)
    b = _pre(True, seed=5)
    c = _pre(True, seed=6)
    xa, ta = a(xi, mi)
    xb, tb = b(xi, mi)
    xc, tc = c(xi, mi)
    xa2, ta2 = a(xi, mi)
    assert torch.equal(xa, xb) and torch.equal(ta, tb)
    assert not torch.equal(xa, xc) and not torch.equal(xa, xa2)
    assert a.counter == 2
    for t in (ta, tc, ta2):
        assert set(torch.unique(t).tolist()) <= {0.0, 1.0} and torch.equal(t[:, 0], 1 - t[:, 1])


def test_errors():
    from salt_amd import SaltError
    img, msk = _tiles(2, 10)
    pre = _pre(True)
    with pytest.raises(SaltError):
        pre(T(img), T(msk))                                                 # CPU tensors
    with pytest.raises(SaltError):
        pre(T(img.astype(np.float32) / 255).to(DEV))                         # float tiles
    with pytest.raises(SaltError):
        pre(torch.zeros((2, 129, 129), dtype=torch.uint8, device=DEV))      # over-size tiles
    with pytest.raises(SaltError):
        pre(T(img).to(DEV), params=torch.zeros((2, 63), device=DEV))
    with pytest.raises(SaltError):
        _pre(True).last_params()


def test_fit_trains_on_augmented_tiles(deterministic_sums):
    from salt_amd.models import SegmentationModel
    from salt_amd.input_pipeline import DevicePreprocessor
    img, msk = _tiles(64, 11)
    pre = DevicePreprocessor(True, 3, augment=True, seed=1234)
    calls = []

    class Batches:
        def __iter__(self):
            for i in range(0, 64, 8):
                calls.append(i)
                yield list(pre(T(img[i:i + 8]).to(DEV), T(msk[i:i + 8]).to(DEV)))

    losses = []

    from salt_amd.callbacks import Callback

    class Rec(Callback):
        def on_batch_end(self, metrics, *a, **k):
            losses.append(float(metrics['sum']))
    arch = {'model_params': {'architecture': 'UNetResNet', 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
            'optimizer_params': {'lr': 1e-3}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    torch.manual_seed(0)
    m = SegmentationModel(arch, {'epochs': 3}, {'callbacks': [Rec()]})
    fused = []
    orig = m._fused_step
    m._fused_step = lambda *a, **k: (fused.append(a[2]), orig(*a, **k))[1]
    m.fit((Batches(), 7))
    assert len(losses) == 24 and all(np.isfinite(losses)) and fused and set(fused) == {'lovasz'}
    assert pre.counter == 24
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
