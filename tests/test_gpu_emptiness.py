"""GPU tests of the emptiness classifier (EmptinessClassifier on csrc/classifier.hip): the pooled 1x1 head through the C-ABI against the
plain fp64 reference of emptiness_op_reference.py (every placement, guard patterns, both dtypes), the reference's own F15 fixtures
through the graph and through the whole network (eval, one training step), the trainer surface with the AUC monitor, and the fused /
autograd-bridge / hipGraph steps on [B,2,1,1] logits."""

import numpy as np
import pytest
import torch

from helpers import golden, T, assert_close
import closed_form as CF
import emptiness_op_reference as ER
from emptiness_op_reference import Placed, VIEW_CASES, VARIANTS
import net_checks as NC
from abi_ops import Vec, raw, call, close, code, gen, rnd, _abi, DEV, F64, SENTINEL

pytestmark = pytest.mark.gpu
TOL32 = 5e-5                    # tests/test_gpu_blocks.py: fp32 block bound

# (B, H, W, C, K): one window / several / ragged rows and columns / C that is no multiple of 16 / the workload's C = 512 (four pixel
# rows per workgroup) / 2048 channels (more pieces than threads in f32) / C > 256 pieces off, K = 8
SHAPES = [(1, 8, 8, 16, 1), (2, 8, 8, 64, 2), (3, 12, 20, 96, 3), (2, 9, 8, 40, 2), (2, 16, 16, 512, 2), (1, 8, 8, 2048, 2), (2, 24, 8, 520, 8)]


def placement(variant, C, dtype):
    """op_reference.VARIANTS 'a' / 'b' / 'c' carried over to C channels: contiguous; a 16-byte aligned slice of a wider buffer; a slice
    that starts 8 bytes past a 16-byte boundary (scalar path)."""
    return {'a': (0, C, C), 'b': (8, C, C + 24), 'c': (2 if dtype == 'f32' else 4, C, C + 24)}[variant]


def head_case(dtype, shape, vx, vdx, with_bias, accumulate, what):
    """forward (training and eval form) + backward (with and without dx) of one placement against the fp64 reference"""
    from salt_amd.engine import shaped_view
    B, H, W, C, K = shape
    OH, OW = H // 8, W // 8
    g = gen('pool_head', dtype, shape, vx, vdx, with_bias, accumulate)
    x = rnd((B, H, W, C), g, dtype)
    w = ER.round_to(torch.randn(K, C, generator=g, dtype=F64) * 0.3, 'f32')
    bias = ER.round_to(torch.randn(K, generator=g, dtype=F64), 'f32') if with_bias else None
    dl = ER.round_to(torch.randn(B, K, OH, OW, generator=g, dtype=F64), 'f32')
    wd, dld = w.float().to(DEV), dl.float().to(DEV)
    bd = bias.float().to(DEV) if with_bias else None
    px = Placed((B, H, W), vx, dtype, DEV, x)
    before = px.buf.clone()
    logits, pooled, logits_eval = Vec(B * K * OH * OW), Vec(B * OH * OW * C), Vec(B * K * OH * OW)
    fields = dict(dtype=code(dtype), x=px.view, w=wd.data_ptr(), bias=bd.data_ptr() if with_bias else None, K=K)
    call('salt_pool_head', logits_nchw=logits.ptr(), pooled=pooled.ptr(), **fields)
    call('salt_pool_head', logits_nchw=logits_eval.ptr(), pooled=None, **fields)
    px.check(what + ' x')
    assert torch.equal(px.buf.view(torch.int16 if dtype == 'bf16' else torch.int32), before.view(torch.int16 if dtype == 'bf16' else torch.int32))
    rp, rl = ER.pool_head(x, w, bias)
    got_l = logits.get((B, K, OH, OW))
    close(got_l, rl, 'f32', what + ' logits')
    close(pooled.get((B, OH, OW, C)), rp, 'f32', what + ' pooled')
    assert torch.equal(got_l, logits_eval.get((B, K, OH, OW))), what + ': eval logits (pooled = NULL) differ from the training form'
    # backward
    sc = (B, H, W, C)
    old = rnd(sc, g, dtype) if accumulate else torch.full(sc, float('nan'), dtype=F64)
    pdx = Placed((B, H, W), vdx, dtype, DEV, old)
    gw, gb = Vec(K * C), Vec(K)
    bw = dict(dtype=code(dtype), w=wd.data_ptr(), K=K, dlogits_nchw=dld.data_ptr(), pooled=pooled.ptr(), accumulate=accumulate)
    call('salt_pool_head_bwd', dx=pdx.view, gw=gw.ptr(), gb=gb.ptr() if with_bias else None, **bw)
    pdx.check(what + ' dx')
    rdx, rgw, rgb = ER.pool_head_bwd(dl, w, rp, H, W, old if accumulate else None, bool(accumulate))
    got_dx = pdx.get()
    close(got_dx, rdx, dtype, what + ' dx')
    outside = ~ER.in_window_mask(H, W)
    if bool(outside.any()):
        want = old[:, outside] if accumulate else torch.zeros_like(old[:, outside])
        assert torch.equal(got_dx[:, outside], want), what + ': pixels outside every window'
    got_gw, got_gb = gw.get((K, C)), gb.get((K,))
    close(got_gw, rgw, 'f32', what + ' gw')
    if with_bias:
        close(got_gb, rgb, 'f32', what + ' gb')
    else:
        assert bool(torch.isnan(got_gb).all()), what + ': gb written although NULL was passed'
    # dx.p == NULL: no data gradient, the same parameter gradients, bit for bit (and run to run)
    gw2, gb2 = Vec(K * C), Vec(K)
    call('salt_pool_head_bwd', dx=shaped_view(None, B, H, W, C, C), gw=gw2.ptr(), gb=gb2.ptr() if with_bias else None, **bw)
    assert torch.equal(got_gw, gw2.get((K, C))), what + ': gw is not reproducible'
    if with_bias:
        assert torch.equal(got_gb, gb2.get((K,))), what + ': gb is not reproducible'


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(str(v) for v in s) for s in SHAPES])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_pool_head_vs_fp64_reference(dtype, shape):
    C = shape[3]
    n = 0
    for vin, vout in VIEW_CASES:
        if 'd' in (vin, vout):                 # the ragged 13-channel variant has its own C: test_pool_head_view_cases
            continue
        for with_bias, accumulate in ((1, 0), (0, 1), (1, 1), (0, 0)):
            head_case(dtype, shape, placement(vin, C, dtype), placement(vout, C, dtype), with_bias, accumulate,
                      'pool_head %s %s->%s bias=%d acc=%d' % (shape, vin, vout, with_bias, accumulate))
            n += 1
    assert n == 24


@pytest.mark.parametrize('views', VIEW_CASES, ids=['%s-%s' % v for v in VIEW_CASES])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_pool_head_view_cases(dtype, views):
    """op_reference.VIEW_CASES as they are (16 channels; 13 for the ragged variant), x placed by the first and dx by the second, on a
    map with a ragged row and ragged columns."""
    vin, vout = views
    C = VARIANTS[vin][dtype][1]
    assert VARIANTS[vout][dtype][1] == C
    for with_bias, accumulate in ((1, 0), (0, 1)):
        head_case(dtype, (2, 9, 19, C, 3), vin, vout, with_bias, accumulate, 'pool_head views %s-%s bias=%d acc=%d' % (vin, vout, with_bias, accumulate))


def test_bad_arguments_are_refused_and_launch_nothing():
    abi = _abi()
    from salt_amd.engine import shaped_view
    B, H, W, C, K = 2, 8, 8, 16, 2
    x = torch.randn(B, H, W, C, device=DEV)
    w, bias = torch.randn(K, C, device=DEV), torch.randn(K, device=DEV)
    logits, pooled = Vec(B * 8, fill=SENTINEL), Vec(B * C, fill=SENTINEL)
    okf = dict(dtype=0, x=shaped_view(x.data_ptr(), B, H, W, C), w=w.data_ptr(), bias=bias.data_ptr(), K=K, logits_nchw=logits.ptr(), pooled=pooled.ptr())
    for what, bad in (('K=0', dict(K=0)), ('K=9', dict(K=9)), ('H=7', dict(x=shaped_view(x.data_ptr(), B, 7, W, C))),
                      ('W=7', dict(x=shaped_view(x.data_ptr(), B, H, 7, C))), ('NULL x', dict(x=shaped_view(None, B, H, W, C))),
                      ('NULL w', dict(w=None)), ('dtype', dict(dtype=7))):
        rc = raw('salt_pool_head', **dict(okf, **bad))
        assert rc == abi.CONSTS['SALT_E_BADARG'], (what, rc)
        assert abi.lib.salt_last_error()
        assert bool((logits.get((B * 8,)) == SENTINEL).all()) and bool((pooled.get((B * C,)) == SENTINEL).all()), what
    dl = torch.randn(B, K, 1, 1, device=DEV)
    dx = torch.full((B, H, W, C), SENTINEL, device=DEV)
    gw, gb = Vec(K * C, fill=SENTINEL), Vec(K, fill=SENTINEL)
    pooled_ok = torch.randn(B, 1, 1, C, device=DEV)
    ok = dict(dtype=0, dx=shaped_view(dx.data_ptr(), B, H, W, C), w=w.data_ptr(), K=K, dlogits_nchw=dl.data_ptr(), pooled=pooled_ok.data_ptr(),
              accumulate=0, gw=gw.ptr(), gb=gb.ptr())
    for what, bad in (('K=0', dict(K=0)), ('K=9', dict(K=9)), ('H=7', dict(dx=shaped_view(dx.data_ptr(), B, 7, W, C))),
                      ('NULL pooled', dict(pooled=None)), ('NULL dlogits', dict(dlogits_nchw=None)), ('NULL gw', dict(gw=None))):
        rc = raw('salt_pool_head_bwd', **dict(ok, **bad))
        assert rc == abi.CONSTS['SALT_E_BADARG'], (what, rc)
        assert bool((dx == SENTINEL).all()) and bool((gw.get((K * C,)) == SENTINEL).all()) and bool((gb.get((K,)) == SENTINEL).all()), what
    # the same structs with nothing wrong are accepted (the refusals above were about the one bad field)
    assert raw('salt_pool_head', **okf) == 0 and raw('salt_pool_head_bwd', **ok) == 0
    assert not bool((logits.get((B * 8,))[:B * K] == SENTINEL).any()) and not bool((gw.get((K * C,)) == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ the head through the graph
class _Head(torch.nn.Module):
    def __init__(self, C, K):
        super().__init__()
        self.classifier = torch.nn.Sequential(torch.nn.AvgPool2d(8), torch.nn.Conv2d(C, K, kernel_size=1, padding=0))


def _head_run(x, sd, gy, dtype='f32', train=True):
    """g.pool_head behind from_nchw, as gpu_harness.BlockRun builds its graphs (pool_head writes NCHW logits itself: no to_nchw)"""
    from gpu_harness import BlockRun

    class HeadRun(BlockRun):
        def __init__(self, module, x):
            from salt_amd.engine import Graph
            from salt_amd.runtime import Engine
            self.module = module.to(DEV)
            self.eng = Engine(self.module, torch.device(DEV), dtype)
            g = self.g = Graph(self.eng, train)
            self.xs = [g.alloc(tuple(x.shape), torch.float32)]
            self.xs[0].copy_(x)
            a = g.from_nchw(self.xs[0])
            K = module.classifier[1].weight.shape[0]
            self.out = g.alloc((a.B, K, a.H // 8, a.W // 8), torch.float32)
            g.pool_head(a, module.classifier[1], self.out)
            if train:
                g.build_backward()
            g.finalize()
    m = _Head(x.shape[1], sd['1.weight'].shape[0])
    m.load_state_dict({'classifier.' + k: v for k, v in sd.items()})
    run = HeadRun(m, x)
    y = run.forward()
    if not train:
        return y, None, None, run
    gx, grads = run.backward(gy.to(DEV))
    return y, gx[0], grads, run


def test_pool_head_block_vs_reference_golden():
    """F15_pool_head (the reference's own Sequential on [2,20,12,20], K = 3) through Graph.pool_head: y, gx, g:weight, g:bias at the
    fp32 block bound of tests/test_gpu_blocks.py."""
    fx = golden('F15_pool_head')
    sd = {k[2:]: T(v) for k, v in fx.items() if k.startswith('s:')}
    y, gx, grads, run = _head_run(T(fx['x']), sd, T(fx['gy']))
    errs = {'y': assert_close(y, fx['y'], TOL32, 'y'), 'gx': assert_close(gx, fx['gx'], TOL32, 'gx'),
            'g:weight': assert_close(grads['classifier.1.weight'], fx['g:weight'], TOL32, 'g:weight'),
            'g:bias': assert_close(grads['classifier.1.bias'], fx['g:bias'], TOL32, 'g:bias')}
    print('pool_head block', errs)
    assert bool((gx[:, :, 8:] == 0).all())
    names = lambda prog: [o[0] for o in prog.ops if o[0] != 'zero']          # ('zero': the statistics arena's clear, 0 bytes here)
    assert names(run.g.fwd) == ['layout', 'pool_head'] and names(run.g.bwd) == ['pool_head_bwd', 'layout']
    ye, _, _, run_e = _head_run(T(fx['x']), sd, None, train=False)
    args = lambda r: [o[2] for o in r.g.fwd.ops if o[0] == 'pool_head'][0]
    assert torch.equal(ye, y) and not args(run_e).pooled and args(run).pooled    # eval keeps no pooled tensor


# ------------------------------------------------------------------------------------------------ whole network
NETS = [('F15_emptiness_resnet18_128', 18), ('F15_emptiness_resnet18_256', 18), ('F15_emptiness_resnet34_128', 34)]


def fixture_input(fx):
    return CF.input_for('f15', tuple(int(v) for v in fx['x_shape']))


def _net(depth, dtype='f32'):
    from salt_amd import architectures as A
    return NC.fill_closed_form(A.EmptinessClassifier(2, depth)).set_compute_dtype(dtype).to(DEV)


@pytest.mark.parametrize('name,depth', NETS)
def test_eval_logits_and_decisions_match_reference(name, depth):
    fx = golden(name)
    x = fixture_input(fx).to(DEV)
    net = _net(depth).eval()
    with torch.no_grad():
        logits = net(x).cpu()
    e = assert_close(logits, fx['eval_logits'], 1e-3, 'eval logits')
    ref = fx['eval_logits'][:, 1]
    safe = np.abs(ref) > 4 * float(fx['ref_f32_vs_f64_maxabs'])
    print('emptiness eval', name, 'rel err %.3e' % e, 'decisions under the guard', int((~safe).sum()))
    assert int((~safe).sum()) == 0
    assert np.array_equal((logits[:, 1] > 0).numpy()[safe], (ref > 0)[safe])
    ops = [o[0] for o in net.engine().net(tuple(x.shape), False).fwd.ops]
    assert ops[-1] == 'pool_head' and ops.count('pool_head') == 1 and 'head1x1' not in ops and 'head_bn' not in ops
    # bf16 storage: finite, and the same decisions as the fp32 run wherever the fp32 logit clears what bf16 storage costs the oracle
    net16 = _net(depth, 'bf16').eval()
    with torch.no_grad():
        l16 = net16(x).cpu()
    assert bool(torch.isfinite(l16).all())
    guard = 4 * float(fx['ref_bf16_storage_vs_f32_maxabs'])
    safe16 = (logits[:, 1].abs() > guard).numpy()
    print('emptiness eval bf16', name, 'max |bf16 - f32| %.3e' % float((l16 - logits).abs().max()), 'guard %.3e' % guard,
          'decisions under the guard', int((~safe16).sum()))
    assert np.array_equal((l16[:, 1] > 0).numpy()[safe16], (logits[:, 1] > 0).numpy()[safe16])


@pytest.mark.parametrize('name', [n for n, _ in NETS[:2]])
def test_one_training_step_matches_reference(name):
    """zero_grad -> forward -> lovasz -> backward -> Adam(lr 1e-4, L2 1e-4) as models.py:105-136; prologue, full gradients and the
    post-step checks by the procedures of tests/net_checks.py, tolerances of
    tests/test_gpu_depth.py::test_one_training_step_matches_reference.  Every live tensor is checked: 62 for ResNet18 (60 of the encoder
    plus the classifier's weight and bias)."""
    fx = golden(name)
    assert float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3             # the reference's own error: a quarter of the 1e-2 below
    net = _net(18)
    net.train()
    opt, out, eng, own, idx = NC.train_step_prologue(net, [fixture_input(fx).to(DEV)], fx, logits_tol=2e-3, loss_tol=2e-3)
    dead = set(net.dead_parameter_names())
    checked, worst, worst_sum = 0, (0.0, ''), (0.0, '')
    for k, p in own.items():
        i = idx[k]
        has = bool(fx['param_has_grad'][i])
        assert has == (k not in dead), k
        if has and fx['grad_norm'][i] > 1e-4:
            off, n = eng.grad_range(p)
            g = eng.grads[off:off + n].double()
            worst = max(worst, (abs(float(g.norm()) - fx['grad_norm'][i]) / fx['grad_norm'][i], k))
            worst_sum = max(worst_sum, (abs(float(g.sum()) - fx['grad_sum'][i]) / (fx['grad_norm'][i] * n ** 0.5), k))
            checked += 1
    print('emptiness train', name, 'checked', checked, 'worst grad norm', worst, 'worst grad sum', worst_sum)
    assert checked == len(eng.live_params) == 62, (checked, len(eng.live_params))
    assert worst[0] < 1e-2, worst
    assert worst_sum[0] < 1e-2, worst_sum
    NC.check_full_grads(eng, own, fx, ['classifier.1.weight', 'classifier.1.bias'], tol=2e-2, verbose=True)
    NC.check_after_adam(opt, net, own, idx, fx, norm_tol=1e-4, sum_tol=1e-4, bn_tol=1e-3, skip_bn=None)


# ------------------------------------------------------------------------------------------------ trainer
def _model(loss='lovasz', dtype='bf16', lr=1e-3, cfg=None, epochs=1):
    return NC.family_model('EmptinessClassifier', dtype, lr, epochs, cfg, loss=loss)


def _tiles(n, seed):
    """n 128x128 tiles, every second one noise plus a bright blob ("not empty"), the others noise alone -> (X [n,3,128,128], flags [n])"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(128), torch.arange(128), indexing='ij')
    X = torch.randn(n, 1, 128, 128, generator=g) * 0.3
    flags = torch.zeros(n, dtype=torch.long)
    for i in range(1, n, 2):
        cy, cx, r = [int(v) for v in torch.randint(30, 98, (3,), generator=g)]
        X[i, 0] += 1.5 * (((yy - cy) ** 2 + (xx - cx) ** 2) < (16 + r // 4) ** 2).float()
        flags[i] = 1
    return X.repeat(1, 3, 1, 1), flags


def test_fit_transform_persist_load_with_the_auc_monitor(tmp_path):
    from salt_amd import callbacks as C, input_pipeline as IP
    rec = NC.Losses()
    ck = str(tmp_path / 'ck' / 'best.torch')
    cfg = {'callbacks': [rec],
           'model_checkpoint': {'filepath': ck, 'epoch_every': 1, 'metric_name': 'auc', 'minimize': False},
           'reduce_lr_on_plateau_scheduler': {'metric_name': 'auc', 'minimize': False, 'reduce_factor': 0.1, 'reduce_patience': 10, 'min_lr': 1e-7},
           'training_monitor': {'batch_every': 0, 'epoch_every': 1}, 'experiment_timing': {'batch_every': 0, 'epoch_every': 1},
           'validation_monitor': {'epoch_every': 1, 'data_dir': None, 'loader_mode': 'resize_and_pad', 'use_depth': False, 'emptiness': True},
           'early_stopping': {'patience': 20, 'metric_name': 'auc', 'minimize': False}}
    torch.manual_seed(0)
    m = _model(cfg=cfg, epochs=2)
    assert any(type(c) is C.ValidationMonitorEmptiness for c in m.callbacks.callbacks)
    Xt, ft = _tiles(64, 1)
    Xv, fv = _tiles(16, 2)
    Tt, Tv = IP.emptiness_target(ft), IP.emptiness_target(fv)
    train = ([[Xt[i:i + 8], Tt[i:i + 8]] for i in range(0, 64, 8)], 7)
    valid = ([[Xv[i:i + 8], Tv[i:i + 8]] for i in range(0, 16, 8)], 1)
    m.fit(train, valid, meta_valid='accepted and ignored')
    assert sorted(m.validation_loss) == [0, 1]
    for e in (0, 1):
        v = m.validation_loss[e]
        assert set(v) == {'sum', 'auc'} and all(torch.isfinite(x).all() for x in v.values())
        assert 0.0 <= float(v['auc']) <= 1.0
    steps = [float(v) for v in rec.values]
    print('emptiness fit: losses', ['%.4f' % s for s in steps], 'auc', [float(m.validation_loss[e]['auc']) for e in (0, 1)])
    assert len(steps) == 16 and all(np.isfinite(steps))
    assert sum(steps[-4:]) / 4 < sum(steps[:4]) / 4
    es = [c for c in m.callbacks.callbacks if type(c) is C.EarlyStopping][0]
    mc = [c for c in m.callbacks.callbacks if type(c) is C.ModelCheckpoint][0]
    assert es.best_score is not None and mc.best_score is not None and m.optimizer.param_groups[0]['lr'] == 1e-3
    m.persist(ck)
    out = m.transform(valid)['mask_prediction']
    assert len(out) == 16 and all(p.shape == (2,) and np.all((p >= 0) & (p <= 1)) for p in out)
    sd = torch.load(ck, map_location='cpu')
    assert list(sd.keys()) == ['module.' + k for k in golden('F15_emptiness_resnet18_128')['keys'].tolist()]
    out2 = _model().load(ck).transform(valid)['mask_prediction']
    for p, q in zip(out, out2):
        assert np.array_equal(p, q)


class _Bridge:
    """a torch-side wrapper of a native loss WITHOUT native_kind: _fit_loop takes the autograd bridge"""

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, output, target):
        return self.fn(output, target)


def _steps(mode, loss='lovasz', n=3):
    """n _fit_loop steps on [B,2,1,1] targets, a different batch each.  fused: resident, aligned tensors read in place (CompiledNet.bind);
    views: the 32-byte target batches are slices that start 4 bytes off the 16-byte grid and X is float64 - both copied into the static
    buffers; bridge: forward -> torch-side loss -> autograd backward; graph: the step replayed as a hipGraph."""
    from salt_amd import input_pipeline as IP
    torch.manual_seed(11)
    m = _model(loss=loss)
    m.step_graph = mode == 'graph'
    if mode == 'bridge':
        name, fn, weight = m.loss_function[0]
        m.loss_function = [(name, _Bridge(fn), weight)]
        assert getattr(m.loss_function[0][1], 'native_kind', None) is None
    m._to_device()
    m.model.train()
    B = 4
    X, flags = _tiles(n * B, 5)
    Tt = IP.emptiness_target(flags)
    flat = torch.cat([torch.zeros(1), Tt.reshape(-1)]).to(DEV)
    ls = []
    for i in range(n):
        sl = slice(i * B, (i + 1) * B)
        if mode == 'views':
            Xd = X.double().to(DEV)[sl]
            Td = flat[1 + i * 2 * B:1 + (i + 1) * 2 * B].view(B, 2, 1, 1)
            assert Td.data_ptr() % 16 != 0 and Td.is_contiguous() and torch.equal(Td.cpu(), Tt[sl])
        else:
            Xd, Td = X[sl].clone().to(DEV), Tt[sl].clone().to(DEV)
            assert Td.numel() * 4 == 32
        ls.append(float(m._fit_loop([Xd, Td])['sum']))
    torch.cuda.synchronize()
    eng = m.model.engine()
    net = eng.net((B, 3, 128, 128), True)
    assert tuple(net.logits.shape) == (B, 2, 1, 1) and tuple(net.target.shape) == (B, 2, 1, 1)
    return ls, eng.grads.clone(), eng.flat.clone()


@pytest.mark.parametrize('loss', ['lovasz', 'bce_dice'])
def test_fused_bridge_and_graph_steps_agree(loss, deterministic_sums):
    """[B,2,1,1] logits through every route of the training step: bit-equal losses, gradients and weights under the fixed summation
    order (as tests/test_gpu_depth.py::test_depth_flows_through_the_fused_step compares its routes)."""
    a, b, c, d = _steps('fused', loss), _steps('views', loss), _steps('bridge', loss), _steps('graph', loss)
    print('losses', loss, a[0], b[0], c[0], d[0])
    assert all(np.isfinite(a[0])) and len(set(a[0])) == 3 and float(a[1].abs().max()) > 0
    for other, what in ((b, 'copied inputs'), (c, 'autograd bridge'), (d, 'hipGraph')):
        assert a[0] == other[0], what
        assert torch.equal(a[1], other[1]), what + ': gradients'
        assert torch.equal(a[2], other[2]), what + ': weights'
