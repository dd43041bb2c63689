"""GPU tests of the depth-conditioned network (UNetResNetWithDepth / SegmentationModelWithDepth): the gate kernels of csrc/depth.hip
against the reference's F14 fixtures, the whole network against the reference, factored vs materialised hypercolumn, the depth input
through the fused step (bound in place, copied, replayed as a hipGraph), the trainer / TTA surface, and the unchanged non-depth path."""
import numpy as np
import pytest
import torch
from torch import nn

from helpers import golden, T, assert_close
import net_checks as NC
from net_checks import fill_closed_form

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL32 = 5e-5                    # tests/test_gpu_blocks.py: fp32 block bound
# bf16: the bounds tests/test_gpu_blocks.py applies to the F4 scSE block (test_scse_kernels_vs_channel_and_spatial_se_goldens)
TOLBF_Y, TOLBF_GX, TOLBF_GP = 1e-2, 3e-2, 6e-2


class _Gate(nn.Module):
    def __init__(self, C):
        super().__init__()
        from salt_amd import architectures as A
        self.dce = A.DepthChannelExcitation(C)


def _gate_run(fx_or_x, d, sd, dtype, layout, gy):
    """The gate over an NCHW input through Graph.depth_gate / channel_gate in one of three layouts -> (y, gx, {param: grad})
    copy: gated copy of the whole view; inplace: in place; halves: two channel halves of the interleaved buffer, each with its own
    c0 (pixel stride > C); planar: the halves as dense planes of a planar buffer, gated in place."""
    from gpu_harness import BlockRun
    x = fx_or_x
    C = x.shape[1]
    m = _Gate(C)
    m.load_state_dict({'dce.' + k: v for k, v in sd.items()})

    def emit(g, a):
        dbuf = g.alloc(tuple(d.shape), torch.float32)
        dbuf.copy_(d)
        gate = g.depth_gate(dbuf, m.dce.fc[0])
        if layout == 'copy':
            return g.channel_gate(a, gate, 0)
        if layout == 'inplace':
            return g.channel_gate(a, gate, 0, out=a)
        h = C // 2
        if layout == 'halves':
            out = g.new_act(a.B, a.H, a.W, C, 'out')
            for c0 in (0, h):
                g.channel_gate(a.slice(c0, h), gate, c0, out=out.slice(c0, h))
            return out
        assert layout == 'planar'
        p = g.new_act(a.B, a.H, a.W, C, 'planar', planes=h)
        out = g.new_act(a.B, a.H, a.W, C, 'out')
        for c0 in (0, h):
            g.copy(a.slice(c0, h), p.slice(c0, h))
            g.channel_gate(p.slice(c0, h), gate, c0, out=p.slice(c0, h))
            g.copy(p.slice(c0, h), out.slice(c0, h))
        return out
    run = BlockRun(m, [x], emit, train=True, dtype=dtype)
    y = run.forward()
    gx, grads = run.backward(gy.to(DEV))
    return y, gx[0], grads


def _torch_gate(x, d, sd, gy):
    w, b = sd['fc.0.weight'].clone().requires_grad_(True), sd['fc.0.bias'].clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    y = xr * torch.sigmoid(torch.nn.functional.linear(d, w, b))[:, :, None, None]
    y.backward(gy)
    return y.detach(), xr.grad, {'dce.fc.0.weight': w.grad, 'dce.fc.0.bias': b.grad}


@pytest.mark.parametrize('layout', ['copy', 'inplace'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_gate_block_vs_reference_golden(dtype, layout):
    """F14 block (C = 20, 5 x 7 pixels): forward, gx, dw, db.  fp32 against the golden itself; bf16 (storage rounds x, y, gy, gx) against
    the same block in torch on the bf16-rounded input, at the bounds of the F4 scSE block test."""
    fx = golden('F14_depth_channel_excitation_train')
    sd = {k[2:]: T(v) for k, v in fx.items() if k.startswith('s:')}
    x, d, gy = T(fx['x']), T(fx['d']), T(fx['gy'])
    if dtype == 'bf16':
        x, gy = x.bfloat16().float(), gy.bfloat16().float()
    y, gx, grads = _gate_run(x, d, sd, dtype, layout, gy)
    yr, gxr, gr = _torch_gate(x, d, sd, gy)
    errs = {'y': assert_close(y, yr, TOL32 if dtype == 'f32' else TOLBF_Y, 'y'),
            'gx': assert_close(gx, gxr, TOL32 if dtype == 'f32' else TOLBF_GX, 'gx')}
    for k in gr:
        errs[k] = assert_close(grads[k], gr[k], TOL32 if dtype == 'f32' else TOLBF_GP, k)
    print('gate block', dtype, layout, errs)
    if dtype == 'f32':
        assert_close(y, fx['y'], TOL32, 'y vs golden')
        assert_close(gx, fx['gx'], TOL32, 'gx vs golden')
        assert_close(grads['dce.fc.0.weight'], fx['g:fc.0.weight'], TOL32, 'dw vs golden')
        assert_close(grads['dce.fc.0.bias'], fx['g:fc.0.bias'], TOL32, 'db vs golden')


@pytest.mark.parametrize('layout', ['halves', 'planar'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('mode', ['shards', 'fixed'])
def test_gate_views_and_reduction_modes(dtype, layout, mode, monkeypatch):
    """Channel slices of an interleaved buffer (pixel stride 2 C) and dense planes of a planar buffer, each gated by its own columns of
    one [B, 32] gate; 16-byte vector path (16 channels per half), enough pixels for several parts per image.  Both dL/ds protocols;
    the fixed-order one twice, bit for bit."""
    if mode == 'fixed':
        monkeypatch.setenv('SALT_BN_FIN', '0')
        monkeypatch.setenv('SALT_SE_SHARDS', '0')
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 3, 32, 37, 41
    x = torch.randn(B, C, H, W, generator=g)
    gy = torch.randn(B, C, H, W, generator=g)
    d = torch.tensor([[0.1], [0.5], [0.9]])
    sd = {'fc.0.weight': torch.randn(C, 1, generator=g) * 1.3, 'fc.0.bias': torch.randn(C, generator=g) * 0.1}
    if dtype == 'bf16':
        x, gy = x.bfloat16().float(), gy.bfloat16().float()
    y, gx, grads = _gate_run(x, d, sd, dtype, layout, gy)
    yr, gxr, gr = _torch_gate(x, d, sd, gy)
    assert_close(y, yr, TOL32 if dtype == 'f32' else TOLBF_Y, 'y')
    assert_close(gx, gxr, TOL32 if dtype == 'f32' else TOLBF_GX, 'gx')
    for k in gr:
        assert_close(grads[k], gr[k], TOL32 if dtype == 'f32' else TOLBF_GP, k)
    if mode == 'fixed':
        y2, gx2, grads2 = _gate_run(x, d, sd, dtype, layout, gy)
        assert torch.equal(y, y2) and torch.equal(gx, gx2)
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), k


def _depth_net(hyper, depth=34):
    from salt_amd import architectures as A
    return A.UNetResNetWithDepth(depth, 2, dropout_2d=0.0, pretrained=False, use_hypercolumn=hyper)


@pytest.mark.parametrize('tag,hyper', [('hyper', True), ('nohyper', False)])
def test_eval_logits_and_masks_match_reference(tag, hyper):
    fx = golden('F14_unet_resnet34_depth_' + tag)
    net = fill_closed_form(_depth_net(hyper)).to(DEV)
    net.eval()
    with torch.no_grad():
        logits = net(T(fx['x']).to(DEV), T(fx['d']).to(DEV)).cpu()
    e = assert_close(logits, fx['eval_logits'], 1e-3, 'eval logits')
    guard = 4 * float(fx['ref_f32_vs_f64_maxabs'])
    safe = np.abs(fx['eval_logits'][:, 1]) > guard
    under = int((~safe).sum())
    mine = (logits[:, 1] > 0).numpy().astype(np.uint8)
    print('depth eval', tag, 'rel err %.3e' % e, 'pixels under the guard', under, 'mask differences', int((mine != fx['eval_mask']).sum()))
    assert under <= 2
    assert np.array_equal(mine[safe], fx['eval_mask'][safe])
    # no full-resolution 5d-channel tensor: with the default factoring the hypercolumn buffer holds dec1 and up2(dec2) only
    if hyper:
        g = net.engine().net((2, 3, 64, 64), False).g
        shapes = [tuple(t.shape) for t in g.keep if t.dim() >= 4]
        assert not any(s[-1] >= 320 and s[-3:-1] == (64, 64) for s in shapes), [s for s in shapes if s[-1] >= 320]


@pytest.mark.parametrize('tag,hyper', [('hyper', True), ('nohyper', False)])
def test_one_training_step_matches_reference(tag, hyper):
    """zero_grad -> forward(X, D) -> lovasz -> backward -> Adam(lr 1e-4, L2 1e-4) as models.py:222-253; tolerances of
    tests/test_gpu_models.py::test_one_training_step_matches_reference; the two gate parameters' gradients elementwise.  Prologue,
    full gradients and the post-step checks by the procedures of tests/net_checks.py."""
    fx = golden('F14_unet_resnet34_depth_' + tag)
    net = fill_closed_form(_depth_net(hyper)).to(DEV)
    net.train()
    opt, out, eng, own, idx = NC.train_step_prologue(net, [T(fx['x']).to(DEV), T(fx['d']).to(DEV)], fx, logits_tol=2e-3, loss_tol=2e-3)
    dead = set(net.dead_parameter_names())
    checked, worst, worst_sum = 0, (0.0, ''), (0.0, '')
    gmax = float(fx['grad_norm'].max())
    for k, p in own.items():
        i = idx[k]
        has = bool(fx['param_has_grad'][i])
        assert has == (k not in dead), k
        if has and fx['grad_norm'][i] > 1e-4:
            off, n = eng.grad_range(p)
            g = eng.grads[off:off + n].double()
            worst = max(worst, (abs(float(g.norm()) - fx['grad_norm'][i]) / fx['grad_norm'][i], k))
            # sums cancel: bounded relative to the tensor's own gradient norm times sqrt(numel) (what |sum| can reach)
            worst_sum = max(worst_sum, (abs(float(g.sum()) - fx['grad_sum'][i]) / (fx['grad_norm'][i] * n ** 0.5), k))
            checked += 1
    print('depth train', tag, 'checked', checked, 'worst grad norm', worst, 'worst grad sum', worst_sum, 'gmax', gmax)
    assert checked > 100 and worst[0] < 1e-2, (checked, worst)
    assert worst_sum[0] < 1e-2, worst_sum
    NC.check_full_grads(eng, own, fx, [k[9:] for k in fx if k.startswith('fullgrad:')], tol=2e-2, verbose=True)
    assert 'fullgrad:depth_channel_excitation.fc.0.weight' in fx and 'fullgrad:depth_channel_excitation.fc.0.bias' in fx
    NC.check_after_adam(opt, net, own, idx, fx, norm_tol=1e-4, sum_tol=1e-4, bn_tol=1e-3, skip_bn=None)


def test_factored_equals_materialised_hypercolumn_with_depth(monkeypatch):
    """SALT_HYPER_FACTOR=0 (every level up-sampled into the hypercolumn, gated before the up-sampling) against the default (levels
    x4 .. x16 gated at their own resolution and factored through the tap GEMM): fp32, eval and one training step.  Bound: the 1e-4
    tests/test_gpu_hyper_factor.py applies to the factored block in fp32 (2e-4 for parameter gradients there); whole-network
    gradients are compared in L2 over the flat gradient buffer."""
    fx = golden('F14_unet_resnet34_depth_hyper')
    x, d, t = T(fx['x']).to(DEV), T(fx['d']).to(DEV), T(fx['t']).to(DEV)
    res = {}
    for mode in ('factored', 'materialised'):
        if mode == 'materialised':
            monkeypatch.setenv('SALT_HYPER_FACTOR', '0')
        from salt_amd import losses
        net = fill_closed_form(_depth_net(True)).to(DEV)
        net.eval()
        with torch.no_grad():
            ye = net(x, d).cpu()
        n_st = sum(1 for name, _, _ in net.engine().net((2, 3, 64, 64), False).fwd.ops if name == 'hyper_stencil')
        assert n_st == (1 if mode == 'factored' else 0)
        net.train()
        out = net(x, d)
        losses.lovasz_loss(out, t).backward()
        torch.cuda.synchronize()
        res[mode] = (ye, out.detach().cpu(), net.engine().grads.clone())
    a, b = res['factored'], res['materialised']
    e0, e1 = assert_close(a[0], b[0], 1e-4, 'eval logits'), assert_close(a[1], b[1], 1e-4, 'train logits')
    l2 = float((a[2] - b[2]).norm() / b[2].norm())
    print('factored vs materialised: eval %.3e train %.3e grads L2 %.3e' % (e0, e1, l2))
    assert l2 <= 2e-4


def test_swapped_depths_change_the_logits():
    fx = golden('F14_unet_resnet34_depth_hyper')
    net = fill_closed_form(_depth_net(True)).to(DEV)
    net.eval()
    x, d = T(fx['x']).to(DEV), T(fx['d']).to(DEV)
    with torch.no_grad():
        a = net(x, d).cpu()
        b = net(x, d.flip(0).contiguous()).cpu()
        c = net(x, d).cpu()
    assert torch.equal(a, c)
    assert float((a - b).abs().max()) > 1.0
    from salt_amd._abi import SaltError
    from salt_amd import architectures as A
    with pytest.raises(SaltError):
        net(x)
    with pytest.raises(SaltError):
        net(x, d.view(-1))
    plain = A.UNetResNet(34, 2, use_hypercolumn=True).to(DEV).eval()
    with pytest.raises(SaltError):
        plain(x, d)


def _depth_model(loss='lovasz', dtype='bf16', lr=1e-3, cfg=None, epochs=1):
    return NC.family_model('UNetResNetWithDepth', dtype, lr, epochs, cfg, loss=loss)


def _steps(mode):
    """3 _fit_loop steps, a different X, D and target each.  bound: every tensor resident, contiguous, 16-byte aligned - read in place
    (CompiledNet.bind); views: batch-sliced views of larger tensors (D slices of 4 floats start off the 16-byte grid every other step,
    X as float64) - copied into the static buffers; graph: the step replayed as a hipGraph (inputs copied into the static buffers)."""
    torch.manual_seed(11)
    m = _depth_model()
    m.step_graph = mode == 'graph'
    m._to_device()
    m.model.train()
    g = torch.Generator().manual_seed(5)
    B = 4
    X = torch.randn(3 * B, 3, 128, 128, generator=g)
    M = (torch.rand(3 * B, 1, 128, 128, generator=g) > 0.6).float()
    Tt = torch.cat([1 - M, M], 1)
    D = torch.rand(3 * B + 1, 1, generator=g)
    ls = []
    for i in range(3):
        sl = slice(i * B, (i + 1) * B)
        if mode == 'views':
            Xd, Dd, Td = X.double().to(DEV)[sl], D.to(DEV)[1 + i * B:1 + (i + 1) * B], Tt.to(DEV)[sl]
            assert Dd.data_ptr() % 16 != 0
            Dref = D[1 + i * B:1 + (i + 1) * B]
        else:
            Xd, Td = X[sl].clone().to(DEV), Tt[sl].clone().to(DEV)
            Dref = D[1 + i * B:1 + (i + 1) * B]
            Dd = Dref.clone().to(DEV)
        assert torch.equal(Dd.cpu(), Dref)
        ls.append(float(m._fit_loop([Xd, Dd, Td])['sum']))
    torch.cuda.synchronize()
    eng = m.model.engine()
    fc = m.model.depth_channel_excitation.fc[0]
    off, n = eng.grad_range(fc.weight)
    return ls, eng.grads.clone(), eng.flat.clone(), eng.grads[off:off + n].clone()


def test_depth_flows_through_the_fused_step(deterministic_sums):
    """The per-step depth really reaches the kernels on all three routes of the fused step: bound in place, copied into the static
    buffer, and copied + replayed as a hipGraph - bit-equal losses, gradients and weights under the fixed summation order.  (The
    bound-vs-copied pair is the A/B the former SALT_STEP_ZERO_COPY switch selected; the switch itself no longer exists.)"""
    a, b, c = _steps('bound'), _steps('views'), _steps('graph')
    print('losses', a[0], b[0], c[0])
    assert len(set(a[0])) == 3
    assert float(a[3].abs().max()) > 0
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[0] == c[0] and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])


def test_fit_transform_persist_load_and_tta(tmp_path):
    """SegmentationModelWithDepth.fit + transform on synthetic tiles with the callback stack (use_depth=True), persist -> load -> same
    outputs, predict_tta(depth=D) = mean of the four flips done by hand."""
    from salt_amd import inference as I
    from gpu_harness import _data
    ck = str(tmp_path / 'ck' / 'best.torch')
    cfg = {'model_checkpoint': {'filepath': ck, 'epoch_every': 1, 'metric_name': 'iout', 'minimize': False},
           'training_monitor': {'batch_every': 0, 'epoch_every': 1}, 'experiment_timing': {'batch_every': 0, 'epoch_every': 1},
           'validation_monitor': {'epoch_every': 1, 'data_dir': None, 'loader_mode': 'resize_and_pad', 'use_depth': True},
           'early_stopping': {'patience': 20, 'metric_name': 'iout', 'minimize': False}}
    torch.manual_seed(0)
    m = _depth_model(dtype='f32', lr=1e-3, cfg=cfg, epochs=2)
    Xt, Mt = _data(16, 1)
    Xv, Mv = _data(8, 2)
    Xt, Xv = Xt.repeat(1, 3, 1, 1), Xv.repeat(1, 3, 1, 1)
    g = torch.Generator().manual_seed(4)
    Dt, Dv = torch.rand(16, 1, generator=g), torch.rand(8, 1, generator=g)
    train = ([[Xt[i:i + 4], Dt[i:i + 4], Mt[i:i + 4]] for i in range(0, 16, 4)], 3)
    valid = ([[Xv[i:i + 4], Dv[i:i + 4], Mv[i:i + 4]] for i in range(0, 8, 4)], 1)
    m.fit(train, valid)
    assert sorted(m.validation_loss) == [0, 1]
    for v in m.validation_loss.values():
        assert set(v) == {'sum', 'iou', 'iout'} and all(torch.isfinite(x).all() for x in v.values())
    m.persist(ck)
    out = m.transform(valid)['mask_prediction']
    assert len(out) == 8 and out[0].shape == (2, 128, 128)
    m2 = _depth_model(dtype='f32').load(ck)
    out2 = m2.transform(valid)['mask_prediction']
    for p, q in zip(out, out2):
        assert np.array_equal(p, q)
    # transform really used the depths: the same tiles with shuffled depths give other probabilities
    shuffled = ([[Xv[i:i + 4], Dv[i:i + 4].flip(0), Mv[i:i + 4]] for i in range(0, 8, 4)], 1)
    assert not np.array_equal(m.transform(shuffled)['mask_prediction'][0], out[0])
    # TTA
    net = m.model.eval()
    X, D = Xv[:4].to(DEV), Dv[:4].to(DEV)
    prob = I.predict_tta(net, X, flip_ud=True, flip_lr=True, depth=D, depth_channels=False).cpu()
    acc = torch.zeros_like(prob)
    with torch.no_grad():
        for ud, lr in I.tta_variants(True, True):
            dims = [k for k, f in ((2, ud), (3, lr)) if f]
            xb = torch.flip(X, dims).contiguous() if dims else X
            p = torch.sigmoid(net(xb, D).float())
            acc += (torch.flip(p, dims) if dims else p).cpu()
    assert_close(prob, acc / 4, 1e-5, 'predict_tta(depth=D)')


def test_resnet152_without_hypercolumn_runs_one_eval_batch():
    net = _depth_net(False, depth=152).to(DEV).eval()
    g = torch.Generator().manual_seed(2)
    x, d = torch.randn(2, 3, 64, 64, generator=g).to(DEV), torch.tensor([[0.3], [0.7]]).to(DEV)
    with torch.no_grad():
        y = net(x, d)
        y2 = net(x, d.flip(0).contiguous())
    assert tuple(y.shape) == (2, 2, 64, 64) and bool(torch.isfinite(y).all()) and not torch.equal(y, y2)
    for depth in (18, 50):
        n = _depth_net(True, depth=depth).to(DEV).eval()
        with torch.no_grad():
            assert bool(torch.isfinite(n(x, d)).all())


# Operator-name sequences of UNetResNet(34, hypercolumn) at [2,3,64,64] fp32 under the default switches, recorded from the commit
# before the depth network was added, run-length encoded as (name, count): the hook UNetResNet.emit gained must emit nothing.
PARENT_PROGRAMS = {
    'train_fwd': [('zero', 1), ('s2d', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), 
        ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('affine_act', 1), ('avgpool2', 1), ('bilinear', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('scse', 1), ('conv', 1), ('bilinear', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('scse', 1), 
        ('conv', 1), ('bilinear', 1), ('conv', 1), ('affine_act', 1), ('conv', 1), ('scse', 1), ('conv', 1), ('bilinear', 1), ('conv', 1), 
        ('affine_act', 1), ('conv', 1), ('scse', 1), ('bilinear', 2), ('conv', 1), ('affine_act', 1), ('conv', 1), ('scse', 1), ('conv', 1), 
        ('hyper_stencil', 1), ('head_bn', 1)],
    'train_bwd': [('zero', 1), ('head_bn_bwd', 1), ('hyper_stencil', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('scse_bwd', 1), 
        ('scse_fc_grads', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), 
        ('wgrad_reduce', 1), ('conv', 1), ('bilinear', 2), ('scse_bwd', 1), ('scse_fc_grads', 1), ('bn_bwd', 1), ('conv_wgrad', 1), 
        ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bilinear', 1), ('conv_wgrad', 1), 
        ('wgrad_reduce', 1), ('conv', 1), ('scse_bwd', 1), ('scse_fc_grads', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bilinear', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('scse_bwd', 1), ('scse_fc_grads', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), 
        ('wgrad_reduce', 1), ('conv', 1), ('bilinear', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('scse_bwd', 1), 
        ('scse_fc_grads', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), 
        ('wgrad_reduce', 1), ('conv', 1), ('bilinear', 1), ('avgpool2', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv', 1), 
        ('bn_bwd', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('conv_wgrad', 1), ('wgrad_reduce', 1), ('stem_grad_unfold', 1)],
    'eval_fwd': [('s2d', 1), ('conv', 38), ('avgpool2', 1), ('bilinear', 1), ('conv', 2), ('scse', 1), ('conv', 1), ('bilinear', 1), ('conv', 2), 
        ('scse', 1), ('conv', 1), ('bilinear', 1), ('conv', 2), ('scse', 1), ('conv', 1), ('bilinear', 1), ('conv', 2), ('scse', 1), ('bilinear', 2), 
        ('conv', 2), ('scse', 1), ('conv', 1), ('hyper_stencil', 1)],
}


def _rle(names):
    out = []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return [(n, c) for n, c in out]


def _unet_programs():
    from salt_amd import architectures as A
    net = A.UNetResNet(34, 2, use_hypercolumn=True).to(DEV)
    eng = net.engine()
    tr, ev = eng.net((2, 3, 64, 64), True), eng.net((2, 3, 64, 64), False)
    return {'train_fwd': [o[0] for o in tr.fwd.ops], 'train_bwd': [o[0] for o in tr.bwd.ops], 'eval_fwd': [o[0] for o in ev.fwd.ops]}


def test_plain_unet_programs_are_unchanged():
    progs = _unet_programs()
    for k, want in PARENT_PROGRAMS.items():
        assert len(progs[k]) == sum(c for _, c in want), (k, len(progs[k]))
        assert _rle(progs[k]) == [tuple(w) for w in want], k
    assert not any(n in ('depth_gate', 'channel_gate') for v in progs.values() for n in v)
