"""The Lovasz options through the public surface: model_params['loss_params'] of 'lovasz' ({'per_image': False, 'ignore': 255}) and of
'lovasz_softmax' ({'only_present': True, 'ignore': 255}) reach the fused step, the autograd bridge, the captured step and the
validation score.  Batches are [4,3,64,64]; the targets carry a void border of 4 pixels (255 in every channel).

Tolerances: the fused step equals the operator-level call on the step's own logits bit for bit; against the float64 closed form on those
logits the operator bars of test_gpu_lovasz_options.py (loss 2e-5 max(1, |ref|); the batch-flat row here has 32768 elements)."""
import pytest
import torch

import lovasz_options_reference as LR
import net_checks as NC
import softmax_loss_reference as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = {'lovasz': ('sigmoid', {'per_image': False, 'ignore': 255}), 'lovasz_softmax': ('softmax', {'only_present': True, 'ignore': 255})}


def _model(kind, lr=1e-4, params='case'):
    activation, lp = CASES[kind]
    extra = {} if params is None else {'loss_params': lp if params == 'case' else params}
    return NC.family_model('UNetResNet', 'f32', lr, 1, None, activation=activation, loss=kind, **extra)


def _batch(seed=7):
    X, Tt = NC.noise_batch(seed, 4, 64)
    Tt = Tt.clone()
    border = torch.ones(64, 64, dtype=torch.bool)
    border[4:-4, 4:-4] = False
    Tt[:, :, border] = 255.0
    return X, Tt, border


def _reference(kind, logits, target):
    B, K, H, W = logits.shape
    z, t = logits.double().cpu().reshape(B, K, H * W), target.double().cpu().reshape(B, K, H * W)
    if kind == 'lovasz':
        return LR.hinge(z.reshape(B, -1), t.reshape(B, -1), per_image=False, ignore=255.0)[0]
    return LR.softmax(SR.softmax(z), t, only_present=True, per_image=True, ignore=255.0)[0]


@pytest.mark.parametrize('kind', sorted(CASES))
def test_one_fused_step_with_options(kind):
    from salt_amd import losses
    torch.manual_seed(3)
    m = _model(kind)
    assert m.loss_params == CASES[kind][1]
    m._to_device()
    m.model.train()
    X, Tt, border = _batch()
    Xd, Td = X.to(DEV), Tt.to(DEV)

    # the autograd bridge with the model's own loss function (a partial that carries the options)
    m.optimizer.zero_grad()
    loss_b = m.loss_function[0][1](m.model(Xd), Td)
    loss_b.backward()

    loss = float(m._fit_loop([X, Tt])['sum'])
    torch.cuda.synchronize()
    net = m.model.engine().net(tuple(X.shape), True)
    logits, dlogits = net.logits.clone(), net.dlogits.clone()
    loss_op, dl_op = losses.native_loss(logits, Td, kind, params=m.loss_params)
    assert float(loss_op) == loss and torch.equal(dl_op, dlogits), 'the fused step is the operator on its own logits'
    plain, _ = losses.native_loss(logits, torch.where(Td == 255, torch.zeros_like(Td), Td), kind)
    assert abs(float(plain) - loss) > 1e-4, 'the options change the loss'
    assert bool((dlogits[:, :, border.to(DEV)] == 0).all()), 'void pixels receive a gradient'
    assert bool((dlogits[:, :, ~border.to(DEV)] != 0).any())
    lref = _reference(kind, logits, Tt)
    print('%s %s: fused loss %.8f float64 %.8f bridge %.8f' % (kind, m.loss_params, loss, lref, float(loss_b)))
    assert abs(loss - lref) <= 2e-5 * max(1.0, abs(lref)), (loss, lref)
    assert abs(float(loss_b.detach()) - loss) <= 2e-5 * max(1.0, abs(loss)), 'the autograd bridge gives the same first-step loss'


@pytest.mark.parametrize('kind', sorted(CASES))
def test_step_graph_replay_equals_eager_steps_with_options(kind, deterministic_sums):
    NC.step_graph_equals_eager(lambda: _model(kind, lr=1e-3), lambda: _batch(5)[:2], steps=4)


@pytest.mark.parametrize('kind', sorted(CASES))
def test_loss_params_are_part_of_the_loss_key(kind):
    from salt_amd._abi import SaltError
    keys = []
    for params in (None, 'case', {'ignore': 7}):
        m = _model(kind, params=params)
        m._to_device()
        eng = m.model.engine()
        eng.loss_params = m.loss_params
        keys.append(eng.net((4, 3, 64, 64), True).loss_key(kind, 1.0))
    assert len(set(keys)) == 3 and all(k[:2] == (kind, 1.0) for k in keys), keys
    with pytest.raises(SaltError) as ei:
        _model(kind, params={'per_batch': True})
    assert 'per_image' in str(ei.value)


def test_score_validation_uses_the_options():
    m = _model('lovasz_softmax')
    m._to_device()
    batches = [list(_batch(s)[:2]) for s in (21, 22)]
    res = m.score_validation((batches, 1))
    assert bool(torch.isfinite(res['sum']).all()) and float(res['sum']) > 0


def test_batch_flat_refuses_data_parallel():
    from salt_amd._abi import SaltError
    m = _model('lovasz')
    m._to_device()
    m.model.train()
    X, Tt, _ = _batch()
    m.dp.world = 2                                               # data parallel active
    with pytest.raises(SaltError, match='per_image=False'):
        m._fit_loop([X, Tt])
    m.dp.world = 1
    assert torch.isfinite(m._fit_loop([X, Tt])['sum'])
