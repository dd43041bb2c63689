"""The softmax head through the public surface: SegmentationModel with model_params['activation'] = 'softmax' trains (fused step, step
graph, autograd bridge), and its probabilities reach test-time augmentation and the validation score.

Tolerances: the operator bars of test_gpu_softmax_loss.py for the step's loss and dlogits against the float64 reference evaluated on the
step's own logits; the whole-network gradient statistics of test_gpu_fused_step.py::test_fit_loop_fused_step_matches_oracle_step
(relative L2 under 5e-2 per tensor, cosine over 0.9999) between the fused step and the autograd bridge; 2e-6 absolute for probabilities
(test_gpu_inference.py::test_tta_mean_vs_oracle)."""
import numpy as np
import pytest
import torch

import net_checks as NC
import softmax_loss_reference as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
LOSSES = ['lovasz_softmax', 'dice_ce']


def _model(loss, lr=1e-4, cfg=None):
    return NC.family_model('UNetResNet', 'f32', lr, 1, cfg, activation='softmax', loss=loss)


def _reference(kind, logits, target):
    """float64 loss and d loss / d logits of the step's own logits"""
    B, K, H, W = logits.shape
    z, t = logits.double().cpu().reshape(B, K, H * W), target.double().cpu().reshape(B, K, H * W)
    if kind == 'dice_ce':
        loss, dz, _ = SR.dice_ce(z, t)
        return loss, dz.reshape(B, K, H, W), 5e-5
    p = SR.softmax(z)
    loss, dp, _ = SR.lovasz_softmax(p, t)
    return loss, SR.softmax_bwd(p, dp).reshape(B, K, H, W), 5e-3


@pytest.mark.parametrize('kind', LOSSES)
def test_one_fused_step(kind):
    from salt_amd import losses
    torch.manual_seed(3)
    m = _model(kind)
    m._to_device()
    m.model.train()
    X, Tt = NC.noise_batch(7, 2, 64)
    Xd, Td = X.to(DEV), Tt.to(DEV)
    eng = m.model.engine()
    own = dict(m.model.named_parameters())

    # the autograd bridge: model(X), loss(out, t).backward()
    fn = {'lovasz_softmax': losses.lovasz_softmax_loss, 'dice_ce': losses.mixed_dice_cross_entropy_loss}[kind]
    m.optimizer.zero_grad()
    out = m.model(Xd)
    loss_b = fn(out, Td)
    loss_b.backward()
    torch.cuda.synchronize()
    bridge = {}
    for k, p in own.items():
        if id(p) in eng._off:
            off, n = eng.grad_range(p)
            bridge[k] = eng.grads[off:off + n].view(p.shape).cpu().clone()

    # the fused step on the same weights
    metrics = m._fit_loop([X, Tt])
    torch.cuda.synchronize()
    net = eng.net(tuple(X.shape), True)
    logits, dlogits, loss = net.logits.clone(), net.dlogits.clone(), float(metrics['sum'])
    assert tuple(logits.shape) == (2, 2, 64, 64) and bool(torch.isfinite(dlogits).all())

    # ... equals the operator-level call on the step's own logits bit for bit
    loss_op, dl_op = losses.native_loss(logits, Td, kind, want_grad=True, loss_scale=1.0)
    assert float(loss_op) == loss and torch.equal(dl_op, dlogits)

    # ... and sits within the operator bars of the float64 reference on those logits
    lref, gref, gtol = _reference(kind, logits, Tt)
    err = float((dlogits.double().cpu() - gref).abs().max())
    print('%s: loss %.8f ref %.8f | dlogits max err %.3e, max|ref| %.3e | bridge loss %.8f' % (kind, loss, lref, err, float(gref.abs().max()),
                                                                                           float(loss_b.detach())))
    assert abs(loss - lref) <= 2e-5 * max(1.0, abs(lref)), (loss, lref)
    assert err <= gtol * float(gref.abs().max())

    # the two paths give the same parameter gradients
    assert abs(float(loss_b.detach()) - loss) <= 2e-5 * max(1.0, abs(loss))
    worst, cos, n = NC.grad_report(m.model, bridge)
    print('%s: fused vs bridge gradients: worst relative L2 %.3e (%s), cosine %.7f, %d tensors' % (kind, worst[0], worst[1], cos, n))
    assert n > 120 and worst[0] < 5e-2 and cos > 0.9999, (worst, cos, n)


def test_dice_ce_loss_params_reach_the_fused_step():
    """model_params['loss_params'] select the weights of the fused path's loss program"""
    from salt_amd import losses
    torch.manual_seed(3)
    m = NC.family_model('UNetResNet', 'f32', 1e-4, 1, None, activation='softmax', loss='dice_ce',
                        loss_params={'dice_weight': 0.2, 'cross_entropy_weight': 0.9, 'smooth': 1.0})
    m._to_device()
    m.model.train()
    X, Tt = NC.noise_batch(7, 2, 64)
    loss = float(m._fit_loop([X, Tt])['sum'])
    torch.cuda.synchronize()
    net = m.model.engine().net(tuple(X.shape), True)
    logits = net.logits.clone()
    weighted, dl = losses.native_loss(logits, Tt.to(DEV), 'dice_ce', params=m.loss_params)
    default, _ = losses.native_loss(logits, Tt.to(DEV), 'dice_ce')
    assert float(weighted) == loss and torch.equal(dl, net.dlogits) and abs(float(default) - loss) > 1e-3
    B, K, H, W = logits.shape
    lref, _, _ = SR.dice_ce(logits.double().cpu().reshape(B, K, H * W), Tt.double().reshape(B, K, H * W), 0.2, 0.9, 1.0)
    assert abs(loss - lref) <= 2e-5 * max(1.0, abs(lref))


def test_step_graph_replay_equals_eager_steps(deterministic_sums):
    """net_checks.step_graph_equals_eager with the three-launch Lovasz-softmax program inside the captured step"""
    NC.step_graph_equals_eager(lambda: _model('lovasz_softmax', lr=1e-3), lambda: NC.noise_batch(5, 2, 64), steps=4)


@pytest.mark.parametrize('kind', LOSSES)
def test_it_learns(kind):
    """20 steps on one batch of 4 squares: the mean loss of the last 5 steps is below the mean of the first 5"""
    from salt_amd import architectures as A
    (X0, T0), (X1, T1) = NC.square_batch(3), NC.square_batch(4)
    batch = (torch.cat([X0, X1]), torch.cat([T0, T1]))
    m, values = NC.fit_steps(lambda cfg: _model(kind, lr=1e-3, cfg=cfg), A.UNetResNet, batch, 20)
    print('%s losses' % kind, ['%.4f' % v for v in values])
    assert np.mean(values[-5:]) < np.mean(values[:5])


@pytest.mark.parametrize('shape', [(2, 2, 16, 24), (3, 3, 17, 23), (1, 4, 64, 64)])
def test_class_probabilities(shape):
    from salt_amd import inference as I
    z = torch.randn(shape, generator=SR.gen('class_probabilities', shape)) * 3
    got = I.class_probabilities(z.to(DEV), 'softmax').cpu().double()
    ref = SR.softmax(z.double().reshape(shape[0], shape[1], -1)).reshape(shape)
    assert float((got - ref).abs().max()) <= 2e-6
    assert torch.equal(I.class_probabilities(z.to(DEV), 'sigmoid'), torch.sigmoid(z.to(DEV)))
    assert torch.equal(I.class_probabilities(z.to(DEV)), torch.sigmoid(z.to(DEV)))


@pytest.mark.parametrize('method', ['mean', 'gmean'])
def test_tta_mean_softmax(method):
    """softmax -> inverse flips -> aggregate over all four flip combinations against a numpy restatement; logits ~ N(0, 2^2), so
    |log p| stays of order 10 and an fp32 logarithm (relative error ~1e-7) keeps the geometric mean inside the 2e-6 bar"""
    from salt_amd import inference as I
    variants = I.tta_variants(True, True)
    assert sorted(variants) == [(False, False), (False, True), (True, False), (True, True)]
    V, B = len(variants), 3
    z = torch.randn(V * B, 2, 16, 24, generator=SR.gen('tta softmax')) * 2
    got = I.tta_mean(z.to(DEV), variants, B, method, activation='softmax').cpu().double().numpy()
    p = SR.softmax(z.double().reshape(V * B, 2, -1)).reshape(V, B, 2, 16, 24).numpy()
    back = []
    for v, (ud, lr) in enumerate(variants):
        q = p[v]
        if lr:
            q = q[..., ::-1]
        if ud:
            q = q[..., ::-1, :]
        back.append(q)
    back = np.stack(back)
    ref = back.mean(0) if method == 'mean' else np.exp(np.log(back).mean(0))
    assert got.shape == ref.shape == (B, 2, 16, 24)
    assert float(np.abs(got - ref).max()) <= 2e-6
    # today's calls are untouched: the sigmoid default is the call without the argument, bit for bit
    zd = z.to(DEV)
    assert torch.equal(I.tta_mean(zd, variants, B, method, activation='sigmoid'), I.tta_mean(zd, variants, B, method))


def test_score_validation_with_a_softmax_model():
    """score_validation's iou / iout equal the host computation from the float64 softmax of the same logits.  The head's 1x1 convolution
    is scaled by 4096 so that the class-1 probabilities sit away from the 21 thresholds; that no probability lies within 1e-5 of a
    threshold is asserted on the host, so no pixel is left out of the comparison."""
    from salt_amd import inference as I
    from oracle import metrics as OM
    torch.manual_seed(9)
    m = _model('lovasz_softmax')
    with torch.no_grad():
        m.model.final[1].weight.mul_(4096.0)
        m.model.final[1].bias.mul_(4096.0)
    m._to_device()
    batches = [list(NC.noise_batch(s, 2, 64)) for s in (21, 22)]
    res = m.score_validation((batches, 1))
    assert set(res) == {'sum', 'iou', 'iout'} and bool(torch.isfinite(res['sum']).all())
    m.model.eval()
    with torch.no_grad():
        logits = torch.cat([m.model(X.to(DEV)).float() for X, _ in batches]).cpu()
    p1 = SR.softmax(logits.double().reshape(4, 2, -1))[:, 1].reshape(4, 64, 64).numpy()
    thresholds = np.linspace(0.5, 0.3, 21)
    assert float(np.abs(p1[None] - thresholds[:, None, None, None]).min()) > 1e-5
    gts = [T[b, 1].numpy().astype(np.uint8) for _, T in batches for b in range(2)]
    assert 0 < sum(int(g.sum()) for g in gts) < 4 * 64 * 64
    best, t_best, scores = 0.0, 0.5, None
    for th in thresholds:                                               # callbacks.py:503-513: walk while IOUT improves
        preds = [(p1[b] > th).astype(np.uint8) for b in range(4)]
        iou, iout = OM.intersection_over_union(gts, preds), OM.intersection_over_union_thresholds(gts, preds)
        if scores is None:
            scores = (iou, iout)                                        # nothing beats 0.0: the default threshold 0.5 is scored
        if iout > best:
            best, t_best, scores = iout, float(th), (iou, iout)
        else:
            break
    print('softmax validation: threshold %.3f iou %.6f iout %.6f' % (t_best, scores[0], scores[1]))
    assert m.best_threshold == t_best
    assert abs(float(res['iou']) - scores[0]) < 1e-6 and abs(float(res['iout']) - scores[1]) < 1e-6
