#!/usr/bin/env python
"""Generate the F18 fixtures (UNetSeResNetXt) by EXECUTING THE REFERENCE'S OWN architectures/unet.py.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_seresnext.py
Everything that is not specific to the grouped bottleneck comes from make_golden_seresnet.py (SEModule, the gate-spread probe, the
block writer with its companion files) and the conventions are that file's.

The reference builds its SE-ResNeXt encoders from ``pretrainedmodels.__dict__['se_resnext50_32x4d' | 'se_resnext101_32x4d']``
(architectures/encoders.py:86-118).  That package is not available here, so this file puts BUILD-AUTHORED factories with the package's
public layout (senet.py: SENet / SEResNeXtBottleneck / SEModule, groups 32, base width 4, reduction 16, inplanes 64, input_3x3 False,
1x1 downsample without padding, no dropout) into the stub module.  The layout is RESTATED, not executed from the package; the stub is
the pin: whoever has the package should compare key lists before loading a real checkpoint.

  F18_sx_bottleneck_{train,eval}     SEResNeXtBottleneck(64 -> 256, planes 64, groups 32, stride 1, with downsample) on [2,64,6,10]
  F18_sx_bottleneck_s2_{train,eval}  SEResNeXtBottleneck(256 -> 512, planes 128, stride 2) on [2,256,6,10]; x and gy are rebuilt by the
                                     tests, gradients above 40 000 elements go to the companion files _g1, _g2, ..
  F18_unet_seresnext50_hyper         unet.UNetSeResNetXt(50, 2, use_hypercolumn=True) at [2,3,64,64]: eval logits plus one training step
                                     as SegmentationModel._fit_loop runs it, in the F17 layout
  F18_unet_seresnext101_hyper        depth 101, eval only

The generator REFUSES to write unless the reference alone meets the F17 guards: at least half of the SE gates of every stage in
[0.1, 0.9]; at most 0.1 % of the pixels with |logit[1]| < 10 x its own f32-vs-f64 error; its f32-vs-f64 gradient-norm figures within a
quarter of the GPU test's bounds (1e-2 relative for tensors of 16 elements and more, 1e-6 of the largest norm below)."""
import copy
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: seresnext_oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root: oracle
import closed_form as CF          # noqa: E402
import ref_import as R            # noqa: E402
from make_golden import canonical_fn, save, ONLY          # noqa: E402
from make_golden_emptiness import lovasz_loss_any_dtype, grad_norms          # noqa: E402
from make_golden_seresnet import SEModule, FC2_SCALES, scale_fc2, gate_fractions, block_fixture          # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


# --------------------------------------------------------------------------- pretrainedmodels stub (build-authored, plain torch)
class SEResNeXtBottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, groups, reduction, stride=1, downsample=None, base_width=4):
        super().__init__()
        width = math.floor(planes * (base_width / 64)) * groups
        self.conv1 = nn.Conv2d(inplanes, width, kernel_size=1, bias=False, stride=1)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.se_module = SEModule(planes * 4, reduction=reduction)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        residual = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            residual = self.downsample(x)
        return self.relu(self.se_module(out) + residual)


class SENeXt(nn.Module):
    def __init__(self, counts, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.layer0 = nn.Sequential(OrderedDict([('conv1', nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)),
                                                 ('bn1', nn.BatchNorm2d(64)), ('relu1', nn.ReLU(inplace=True)),
                                                 ('pool', nn.MaxPool2d(3, stride=2, ceil_mode=True))]))
        self.layer1 = self._make(64, counts[0], 1)
        self.layer2 = self._make(128, counts[1], 2)
        self.layer3 = self._make(256, counts[2], 2)
        self.layer4 = self._make(512, counts[3], 2)
        self.avg_pool = nn.AvgPool2d(7, stride=1)
        self.dropout = None
        self.last_linear = nn.Linear(512 * 4, num_classes)

    def _make(self, planes, n, stride):
        down = None
        if stride != 1 or self.inplanes != planes * 4:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, kernel_size=1, stride=stride, padding=0, bias=False),
                                 nn.BatchNorm2d(planes * 4))
        layers = [SEResNeXtBottleneck(self.inplanes, planes, 32, 16, stride, down)]
        self.inplanes = planes * 4
        layers += [SEResNeXtBottleneck(self.inplanes, planes, 32, 16) for _ in range(1, n)]
        return nn.Sequential(*layers)


def _factory(counts):
    def make(num_classes=1000, pretrained=None):
        if pretrained:
            raise RuntimeError('no network: pretrained weights unavailable')
        return SENeXt(counts, num_classes)
    return make


def install_senext_stub():
    R.install_stubs()
    pm = sys.modules['pretrainedmodels']
    for name, counts in (('se_resnext50_32x4d', [3, 4, 6, 3]), ('se_resnext101_32x4d', [3, 4, 23, 3])):
        setattr(pm, name, _factory(counts))            # encoders.py reads pretrainedmodels.__dict__[name]


def network_fixture(unet, models, name, depth, train_step):
    """make_golden_seresnet.network_fixture for unet.UNetSeResNetXt, tags 'f18..', with the gradient-norm guard asserted here."""
    import seresnext_oracle as SX
    from oracle import blocks as OB
    shape = (2, 3, 64, 64)

    def build(scale):
        net = unet.UNetSeResNetXt(encoder_depth=depth, num_classes=2, dropout_2d=0.0, pretrained=False, use_hypercolumn=True, pool0=False)
        canon = canonical_fn(net)
        CF.fill_module(net, canonical=canon)
        scale_fc2(net, scale)
        return net, canon
    enc = lambda net: [[b.se_module for b in getattr(net.encoders.encoder, 'layer%d' % i)] for i in (1, 2, 3, 4)]
    def attempt(picked):
        tag, scale, X, net, canon, logits, err, margin, fr_eval = picked
        out = OrderedDict(x_shape=np.array(X.shape), x=X, input_tag=np.array(tag), fc2_scale=np.float32(scale), gate_frac_mid_eval=np.array(fr_eval),
                          eval_logits=logits, ref_f32_vs_f64_maxabs=err, margin_pixels=margin)
        out['keys'] = np.array(list(net.state_dict().keys()))
        out['key_shapes'] = np.array(['x'.join(str(d) for d in v.shape) for v in net.state_dict().values()])
        sd = {k: v.clone() for k, v in net.state_dict().items() if canon(k) == k}
        with torch.no_grad():
            o32 = SX.unet_seresnext(sd, X, False, depth=depth)
            with OB.bf16_storage():
                o16 = SX.unet_seresnext(sd, X, False, depth=depth)
        assert float((o32 - logits).abs().max()) <= 1e-3 * float(logits.abs().max()), 'test-side oracle does not reproduce the reference'
        out['ref_bf16_storage_vs_f32_maxabs'] = float((o16.double() - o32.double()).abs().max())
        msg = '  %s: max|logit| %.2f  bf16 storage %.2e' % (name, float(logits.abs().max()), out['ref_bf16_storage_vs_f32_maxabs'])
        if train_step:
            T = CF.mask_for('f18', (2, 64, 64))
            out['t'] = T
            net.train()
            n64 = copy.deepcopy(net).double()
            lovasz_loss_any_dtype(n64(X.double()), T.double()).backward()
            g64 = grad_norms(n64)
            fr_train = gate_fractions(n64, enc(n64), lambda: n64(X.double()))
            if min(fr_train) < 0.5:
                print('  %s: input %s refused: train-mode gates saturate: %s' % (name, tag, fr_train))
                return None
            out['gate_frac_mid_train'] = np.array(fr_train)
            del n64
            # one training step exactly as SegmentationModel._fit_loop (models.py:105-136)
            params = [p for p in net.parameters() if p.requires_grad]
            opt = torch.optim.Adam([{'params': params, 'weight_decay': 1e-4}], lr=1e-4)
            opt.zero_grad()
            o = net(X)
            loss = models.lovasz_loss(o, T) * 1.0
            loss.backward()
            out['train_logits'] = o
            out['train_loss'] = loss
            g32 = grad_norms(net)
            assert list(g32) == list(g64)
            numel = {k: p.numel() for k, p in net.named_parameters()}
            gmax = max(g64.values())
            out['ref_f32_vs_f64_gradnorm_rel'] = max(abs(g32[k] - g64[k]) / g64[k] for k in g64 if g64[k] > 1e-4 and numel[k] >= 16)
            out['ref_f32_vs_f64_small_abs'] = max(abs(g32[k] - g64[k]) / gmax for k in g64 if g64[k] > 1e-4 and numel[k] < 16)
            out['ref_f32_vs_f64_small_rel'] = max(abs(g32[k] - g64[k]) / g64[k] for k in g64 if g64[k] > 1e-4 and numel[k] < 16)
            # a quarter of the GPU test's bounds, or nothing is written
            if not (out['ref_f32_vs_f64_gradnorm_rel'] <= 2.5e-3 and out['ref_f32_vs_f64_small_abs'] <= 2.5e-7):
                print('  %s: input %s refused: gradient norms f32 vs f64 %.2e (>= 16 elements), %.2e of the largest norm (< 16)' % (
                    name, tag, out['ref_f32_vs_f64_gradnorm_rel'], out['ref_f32_vs_f64_small_abs']))
                return None
            names, gnorm, gsum, has_grad = [], [], [], []
            for k, p in net.named_parameters():
                names.append(k)
                has_grad.append(p.grad is not None)
                g = p.grad if p.grad is not None else torch.zeros_like(p)
                gnorm.append(float(g.double().norm()))
                gsum.append(float(g.double().sum()))
            named = dict(net.named_parameters())
            for k in ('final.1.weight', 'final.1.bias', 'encoders.encoder.layer1.0.conv2.weight', 'encoders.encoder.layer2.0.conv2.weight',
                      'encoders.encoder.layer1.0.se_module.fc1.bias', 'encoders.encoder.layer1.0.se_module.fc2.bias',
                      'encoders.encoder.layer4.2.se_module.fc1.bias', 'encoders.encoder.layer4.2.se_module.fc2.bias'):
                out['fullgrad:' + k] = named[k].grad.clone()
            opt.step()
            out['param_names'] = np.array(names)
            out['param_has_grad'] = np.array(has_grad)
            out['grad_norm'] = np.array(gnorm)
            out['grad_sum'] = np.array(gsum)
            out['post_norm'] = np.array([float(p.detach().double().norm()) for _, p in net.named_parameters()])
            out['post_sum'] = np.array([float(p.detach().double().sum()) for _, p in net.named_parameters()])
            sd2 = net.state_dict()
            bn_keys = [k for k in sd2 if (k.endswith('running_mean') or k.endswith('running_var')) and canon(k) == k]
            out['bn_keys'] = np.array(bn_keys)
            out['bn_sum'] = np.array([float(sd2[k].double().sum()) for k in bn_keys])
            msg += '  loss %.5f  grad-norm f32 vs f64 %.2e (small tensors: %.2e of the largest norm, %.2e relative)  min checked grad norm %.2e  live tensors %d' % (
                float(loss.detach()), out['ref_f32_vs_f64_gradnorm_rel'], out['ref_f32_vs_f64_small_abs'], out['ref_f32_vs_f64_small_rel'],
                min(v for v, h in zip(gnorm, has_grad) if h and v > 1e-4), sum(has_grad))
        return out, msg

    def eval_guards(tag):
        """-> the eval half of the fixture at input ``tag``, or None where the gates saturate / the mask margin is not kept"""
        X = CF.input_for(tag, shape)
        for scale in FC2_SCALES:
            net, canon = build(scale)
            net.eval()
            with torch.no_grad():
                fr_eval = gate_fractions(net, enc(net), lambda: net(X))
            if min(fr_eval) >= 0.5:
                break
        else:
            return None
        net.eval()
        with torch.no_grad():
            logits = net(X)
            logits64 = copy.deepcopy(net).double()(X.double())
        err = float((logits.double() - logits64).abs().max())
        margin = int((logits[:, 1].abs() < 10 * err).sum())
        print('  %s: input %s fc2 scale %g  gates %s  f32 vs f64 %.2e  pixels under 10x %d of %d' % (
            name, tag, scale, ['%.2f' % f for f in fr_eval], err, margin, logits[:, 1].numel()))
        return (tag, scale, X, net, canon, logits, err, margin, fr_eval) if margin <= 0.001 * logits[:, 1].numel() else None

    # the input tag is changed until the reference alone keeps every guard (recorded as `input_tag`)
    for tag in ['f18'] + ['f18:%d' % i for i in range(1, 16)]:
        picked = eval_guards(tag)
        res = attempt(picked) if picked is not None else None
        if res is not None:
            save(name, **res[0])
            print(res[1])
            return
    raise AssertionError('%s: no input keeps the guards' % name)


def main():
    assert R.reference_available(), 'reference not mounted'
    install_senext_stub()
    unet = R.load('architectures.unet')
    models = R.load_models_module()
    down = lambda cin, cout, s: nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, stride=s, padding=0, bias=False), nn.BatchNorm2d(cout))
    want = lambda name: not ONLY or any(o.startswith(name) for o in ONLY)
    if want('F18_sx_bottleneck'):
        block_fixture('F18_sx_bottleneck', lambda: SEResNeXtBottleneck(64, 64, 32, 16, 1, down(64, 256, 1)), CF.input_for('f18a', (2, 64, 6, 10)), True, False)
    if want('F18_sx_bottleneck_s2'):
        block_fixture('F18_sx_bottleneck_s2', lambda: SEResNeXtBottleneck(256, 128, 32, 16, 2, down(256, 512, 2)), CF.input_for('f18b', (2, 256, 6, 10)), False, True)
    if want('F18_unet_seresnext50_hyper'):
        network_fixture(unet, models, 'F18_unet_seresnext50_hyper', 50, True)
    if want('F18_unet_seresnext101_hyper'):
        network_fixture(unet, models, 'F18_unet_seresnext101_hyper', 101, False)


if __name__ == '__main__':
    main()
