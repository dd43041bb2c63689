"""CPU tests of the emptiness classifier: the comparator tests/emptiness_oracle.py and the operator reference
tests/emptiness_op_reference.py against the F15 fixtures the reference produced, the host surface (state_dict layout, registry, error
paths, callback construction, validation scoring on a stand-in network) and the numpy ROC-AUC."""
import numpy as np
import pytest
import torch

from helpers import golden, T, assert_close
import closed_form as CF
import emptiness_oracle as EO
import emptiness_op_reference as ER
from oracle import losses as OL, specs as OS

NETS = [('F15_emptiness_resnet18_128', 18, True), ('F15_emptiness_resnet18_256', 18, True), ('F15_emptiness_resnet34_128', 34, False)]


def fixture_input(fx):
    x = CF.input_for('f15', tuple(int(v) for v in fx['x_shape']))
    if 'x' in fx:
        assert np.array_equal(x.numpy(), fx['x'])
    return x


# ------------------------------------------------------------------------------------------------ fixtures vs comparators
def test_op_reference_and_oracle_head_reproduce_the_reference_block():
    """F15_pool_head is the reference's own nn.Sequential(AvgPool2d(8), Conv2d(20, 3, 1)) on [2,20,12,20] (rows 8..11 in no window)."""
    fx = golden('F15_pool_head')
    w, b = CF.tensor_for('1.weight', fx['s:1.weight'].shape), CF.tensor_for('1.bias', fx['s:1.bias'].shape)
    assert np.array_equal(w.numpy(), fx['s:1.weight']) and fx['y'].shape == (2, 3, 1, 2)
    x = T(fx['x']).requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = EO.pool_head(x, wr, br)
    assert_close(y, fx['y'], 2e-5, 'y')
    y.backward(T(fx['gy']))
    assert_close(x.grad, fx['gx'], 2e-5, 'gx')
    assert_close(wr.grad, fx['g:weight'], 2e-5, 'g:weight')
    assert_close(br.grad, fx['g:bias'], 2e-5, 'g:bias')
    # the plain fp64 operator reference the GPU test compares the kernel with
    x64 = T(fx['x']).double().permute(0, 2, 3, 1).contiguous()
    pooled, logits = ER.pool_head(x64, w.double().reshape(3, 20), b.double())
    assert_close(logits.float(), fx['y'], 2e-6, 'op reference logits')
    dx, gw, gb = ER.pool_head_bwd(T(fx['gy']).double(), w.double().reshape(3, 20), pooled, 12, 20)
    assert_close(dx.permute(0, 3, 1, 2).float(), fx['gx'], 2e-6, 'op reference dx')
    assert_close(gw.reshape(3, 20, 1, 1).float(), fx['g:weight'], 2e-6, 'op reference gw')
    assert_close(gb.float(), fx['g:bias'], 2e-6, 'op reference gb')
    assert bool((dx[:, 8:] == 0).all()) and not bool(ER.in_window_mask(12, 20)[8:].any())
    old = torch.full_like(dx, 3.0)
    dx1, _, _ = ER.pool_head_bwd(T(fx['gy']).double(), w.double().reshape(3, 20), pooled, 12, 20, old=old, accumulate=True)
    assert bool((dx1[:, 8:] == 3.0).all()) and torch.equal(dx1[:, :8], dx[:, :8] + 3.0)


@pytest.mark.parametrize('name,depth,trains', NETS)
def test_emptiness_oracle_reproduces_reference_network(name, depth, trains):
    """Same checks and tolerances as tests/test_depth_cpu.py applies to the F14 networks."""
    fx = golden(name)
    spec = EO.spec_emptiness_classifier(depth, with_fc=True)
    assert set(EO.expand_aliases({k: None for k in spec})) == set(fx['keys'].tolist())
    sd = CF.state_for((k, s) for k, (s, _) in spec.items())
    x = fixture_input(fx)
    with torch.no_grad():
        logits = EO.emptiness_classifier(sd, x, False, depth=depth)
    assert tuple(logits.shape) == (2, 2, x.shape[2] // 128, x.shape[3] // 128)
    assert_close(logits, fx['eval_logits'], 1e-4, 'eval logits')
    assert np.array_equal((logits[:, 1] > 0).numpy(), fx['eval_logits'][:, 1] > 0)
    if not trains:
        assert 'train_loss' not in fx
        return
    t = T(fx['t'])
    assert t[0, :, 0, 0].tolist() == [0.0, 1.0] and t[1, :, 0, 0].tolist() == [1.0, 0.0]
    train_keys = [k for k in OS.trainable_keys(spec) if not k.startswith('encoder.fc.')]
    for k in train_keys:
        sd[k].requires_grad_(True)
    out = EO.emptiness_classifier(sd, x, True, depth=depth)
    assert_close(out, fx['train_logits'], 1e-4, 'train logits')
    loss = OL.lovasz_loss(out, t)
    loss.backward()
    assert abs(float(loss) - float(fx['train_loss'])) < 1e-4 * max(1.0, abs(float(fx['train_loss'])))
    idx = {n: i for i, n in enumerate(fx['param_names'].tolist())}
    assert int(fx['param_has_grad'].sum()) == len(train_keys) == 62
    assert not fx['param_has_grad'][idx['encoder.fc.weight']] and not fx['param_has_grad'][idx['encoder.fc.bias']]
    checked = 0
    for k in train_keys:
        i = idx[k]
        assert bool(fx['param_has_grad'][i]) and fx['grad_norm'][i] > 1e-4, k          # no tensor falls under the skip rule
        gn = float(sd[k].grad.double().norm())
        assert abs(gn - fx['grad_norm'][i]) <= 2e-3 * fx['grad_norm'][i], (k, gn, fx['grad_norm'][i])
        checked += 1
    assert checked == 62
    for k in ('classifier.1.weight', 'classifier.1.bias'):
        assert_close(sd[k].grad, fx['fullgrad:' + k], 2e-3, k)
    params = [sd[k] for k in train_keys]
    with torch.no_grad():
        ps = [p.detach() for p in params]
        OL.adam_l2_step(ps, [p.grad for p in params], [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], 1)
    for k, p in zip(train_keys, params):
        i = idx[k]
        assert abs(float(p.detach().double().norm()) - fx['post_norm'][i]) <= 1e-5 * max(fx['post_norm'][i], 1e-3), k
    for k, s in zip(fx['bn_keys'].tolist(), fx['bn_sum'].tolist()):
        assert abs(float(sd[k].double().sum()) - s) <= 1e-4 * max(1.0, abs(s)), k


def test_fixture_guards_are_the_references_own_error():
    """The GPU tests' guards: 4 x the fp32 reference's distance from float64 on the decisions (no decision of these fixtures sits under
    it), a quarter of the gradient-norm tolerance on the training step."""
    for name, depth, trains in NETS:
        fx = golden(name)
        guard = 4 * float(fx['ref_f32_vs_f64_maxabs'])
        assert 0 < guard < 5e-4 and int((np.abs(fx['eval_logits'][:, 1]) <= guard).sum()) == 0
        assert 0 < float(fx['ref_bf16_storage_vs_f32_maxabs']) < 1.0
        if trains:
            assert 0 < float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3
            assert float(fx['grad_norm'][fx['param_has_grad']].min()) > 1e-4


# ------------------------------------------------------------------------------------------------ host surface
def test_registry_entry_is_the_references():
    from salt_amd import architectures as A, models
    assert models.ARCHITECTURES['EmptinessClassifier'] == {'model': A.EmptinessClassifier,
                                                           'model_config': {'encoder_depth': 18, 'pretrained': False},
                                                           'init_weights': False}


def test_state_dict_layout_matches_reference():
    from salt_amd import architectures as A
    for name, depth, _ in NETS[1:]:
        net = A.EmptinessClassifier(2, depth)
        assert list(net.state_dict().keys()) == golden(name)['keys'].tolist()
    net = A.EmptinessClassifier(2, 18)
    sd = net.state_dict()
    assert list(sd.keys())[-2:] == ['classifier.1.weight', 'classifier.1.bias']
    assert tuple(sd['classifier.1.weight'].shape) == (2, 512, 1, 1)
    assert sd['conv1.0.weight'].data_ptr() == sd['encoder.conv1.weight'].data_ptr()
    assert sd['encoder5.1.bn2.weight'].data_ptr() == sd['encoder.layer4.1.bn2.weight'].data_ptr()
    assert isinstance(net.classifier[0], torch.nn.AvgPool2d) and net.classifier[0].kernel_size == 8
    for depth, bottom in ((18, 512), (34, 512), (50, 2048), (101, 2048), (152, 2048)):
        assert A.EmptinessClassifier(3, depth).classifier[1].weight.shape == (3, bottom, 1, 1)


def test_dead_parameters_output_shape_and_error_paths():
    from salt_amd import architectures as A
    from salt_amd._abi import SaltError
    net = A.EmptinessClassifier(2, 18)
    assert net.is_classifier and not net.uses_depth
    assert net.dead_parameter_names() == ['encoder.fc.weight', 'encoder.fc.bias']
    assert net.output_shape((4, 3, 128, 128)) == (4, 2, 1, 1)
    assert net.output_shape((2, 3, 256, 384)) == (2, 2, 2, 3)
    with pytest.raises(NotImplementedError, match='only 18, 34, 50, 101, 152 version of Resnet are implemented'):
        A.EmptinessClassifier(2, 20)
    with pytest.raises(SaltError, match='128x128'):
        net.output_shape((2, 3, 64, 64))
    with pytest.raises(SaltError, match='128x128'):
        net.output_shape((2, 3, 128, 127))
    with pytest.raises(SaltError, match='download'):
        A.EmptinessClassifier(2, 18, pretrained=True)
    with pytest.raises(SaltError):
        net(torch.zeros(1, 3, 128, 128))                  # CPU tensor: no fallback


def _arch(loss='lovasz'):
    return {'model_params': {'architecture': 'EmptinessClassifier', 'out_channels': 2, 'activation': 'sigmoid', 'loss': loss},
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}


def test_callbacks_network_builds_the_right_monitor():
    from salt_amd import callbacks as C, models, architectures as A
    from salt_amd._abi import SaltError
    vm = {'epoch_every': 1, 'data_dir': None, 'loader_mode': 'resize_and_pad'}
    for flag, cls in ((True, C.ValidationMonitorEmptiness), (False, C.ValidationMonitor)):
        cfg = {'validation_monitor': dict(vm, emptiness=flag), 'training_monitor': {'batch_every': 0, 'epoch_every': 1}}
        cbs = C.callbacks_network(cfg).callbacks
        mon = [c for c in cbs if isinstance(c, C.ValidationMonitor)]
        assert len(mon) == 1 and type(mon[0]) is cls
        assert cfg['validation_monitor']['emptiness'] is flag             # the caller's config is not edited
    assert type(C.callbacks_network({'validation_monitor': vm}).callbacks[0]) is C.ValidationMonitor
    m = models.SegmentationModel(_arch(), {'epochs': 1}, {'validation_monitor': dict(vm, emptiness=True)})
    assert isinstance(m.model, A.EmptinessClassifier)
    assert isinstance(m.callbacks.callbacks[0], C.ValidationMonitorEmptiness)
    m.callbacks.set_params(m, validation_datagen=None, meta_valid='ignored')
    ids = {id(p) for p in m.optimizer.param_groups[0]['params']}
    assert id(m.model.classifier[1].weight) in ids and id(m.model.classifier[1].bias) in ids
    unet = models.SegmentationModel(dict(_arch(), model_params=dict(_arch()['model_params'], architecture='UNetResNet')), {'epochs': 1}, {})
    with pytest.raises(SaltError):
        C.ValidationMonitorEmptiness().set_params(unet, validation_datagen=None)
    mon = C.ValidationMonitorEmptiness(data_dir='d', loader_mode='m', epoch_every=0, batch_every=2, use_depth=False)
    assert (mon.data_dir, mon.loader_mode, mon.epoch_every, mon.batch_every, mon.use_depth) == ('d', 'm', False, 2, False)


class _StandIn:
    """What score_validation_emptiness touches of a transformer, around a fixed logit table (no GPU)."""

    def __init__(self, logits_by_batch):
        outs = iter(logits_by_batch)

        class Net(torch.nn.Module):
            is_classifier = True

            def forward(self, x):
                return next(outs)
        self.model = Net()
        self.loss_function = [('mask', OL.lovasz_loss, 1.0)]

    def _to_device(self):
        return torch.device('cpu')


def test_score_validation_emptiness_on_a_stand_in_network():
    from salt_amd import callbacks as C, input_pipeline as IP, inference as I, models
    from salt_amd._abi import SaltError
    z = torch.tensor([2.0, -1.0, 0.5, -3.0, 0.25, 0.5, -0.5, 4.0])
    y = [1, 0, 0, 0, 1, 1, 0, 1]
    logits = torch.stack([-z, z], 1).reshape(8, 2, 1, 1)
    tgt = IP.emptiness_target(y)
    batches = [[torch.zeros(4, 3, 128, 128), tgt[:4]], [torch.zeros(4, 3, 128, 128), tgt[4:]]]
    tr = _StandIn([logits[:4], logits[4:]])
    tr.model.train()
    val = C.score_validation_emptiness(tr, (batches, 1))
    assert set(val) == {'sum', 'auc'} and all(v.dtype == torch.float32 and tuple(v.shape) == (1,) for v in val.values())
    assert tr.model.training
    assert abs(float(val['auc']) - I.roc_auc(y, torch.sigmoid(z).numpy())) < 1e-7 and 0.5 < float(val['auc']) < 1.0
    want = (float(OL.lovasz_loss(logits[:4], tgt[:4])) + float(OL.lovasz_loss(logits[4:], tgt[4:]))) / 2
    assert abs(float(val['sum']) - want) < 1e-6
    # Model.score_validation dispatches on the network's is_classifier
    tr2 = _StandIn([logits[:4], logits[4:]])
    assert set(models.Model.score_validation(tr2, (batches, 1))) == {'sum', 'auc'}
    with pytest.raises(SaltError, match='1, 1|1x1|2,1,1'):                       # a 2x2 output has no single score per tile
        C.score_validation_emptiness(_StandIn([logits[:4].expand(4, 2, 2, 2)]), ([[batches[0][0], tgt[:4].expand(4, 2, 2, 2)]], 0))
    one = IP.emptiness_target([1, 1, 1, 1])
    with pytest.raises(ValueError, match='Only one class present'):
        C.score_validation_emptiness(_StandIn([logits[:4]]), ([[batches[0][0], one]], 0))


# ------------------------------------------------------------------------------------------------ helpers
def test_roc_auc_hand_cases():
    from salt_amd.inference import roc_auc
    assert abs(roc_auc([0, 0, 1, 1, 1, 0], [.1, .4, .4, .8, .35, .35]) - 7.0 / 9.0) < 1e-12
    assert roc_auc([0, 0, 1, 1], [0.1, 0.2, 0.3, 0.9]) == 1.0
    assert roc_auc([1, 1, 0, 0], [0.1, 0.2, 0.3, 0.9]) == 0.0
    assert roc_auc([0, 1, 0, 1, 1], [0.5] * 5) == 0.5
    assert roc_auc(np.array([[0.0], [1.0]]), np.array([[0.2], [0.7]], np.float32)) == 1.0
    for y in ([1, 1, 1], [0, 0]):
        with pytest.raises(ValueError, match='Only one class present'):
            roc_auc(y, [0.1 * i for i in range(len(y))])


def test_roc_auc_equals_sklearn_on_quantised_scores():
    metrics = pytest.importorskip('sklearn.metrics')
    from salt_amd.inference import roc_auc
    r = np.random.RandomState(7)
    for case in range(200):
        n = r.randint(2, 60)
        y = r.randint(0, 2, n)
        if y.min() == y.max():
            y[0] = 1 - y[0]
        s = np.round(r.rand(n) * r.choice([3, 10, 100])) / 10.0           # quantised: many ties
        assert abs(roc_auc(y, s) - metrics.roc_auc_score(y, s)) < 1e-12, case


def test_emptiness_target_and_resize_match_the_references_arithmetic():
    from salt_amd import input_pipeline as IP, inference as I
    for flags in ([0, 1, 1, 0], np.array([1]), torch.tensor([0, 0, 1])):
        got = IP.emptiness_target(flags)
        want = []
        for x in np.asarray(flags).reshape(-1):                           # loaders.py:778-783, per tile
            x_ = np.zeros((2, 1, 1))
            x_[0, :, :] = int(x == 0)
            x_[1, :, :] = x
            want.append(x_)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(want), 2, 1, 1)
        assert np.array_equal(got.numpy(), np.stack(want).astype(np.float32))
    img = np.array([0.3, 0.7]).reshape(2, 1, 1)
    out = I.resize_emptiness_predictions(img, (5, 4))                     # postprocessing.py:46-61
    want = np.zeros((2, 5, 4))
    want[0, :, :] = img[0]
    want[1, :, :] = img[1]
    assert out.shape == (2, 5, 4) and out.dtype == np.float64 and np.array_equal(out, want)
