#!/usr/bin/env python
"""Generate the F19 fixtures (UNetDenseNet) by EXECUTING THE REFERENCE'S OWN architectures/unet.py.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_densenet.py

The reference builds its DenseNet encoders from ``pretrainedmodels.__dict__['densenet121']`` (architectures/encoders.py:121-164).  That
package is not available here, so this file installs a BUILD-AUTHORED ``pretrainedmodels`` module into sys.modules BEFORE
ref_import.install_stubs() (which uses setdefault and therefore keeps it).  The module carries a plain-torch DenseNet with the public
torchvision / pretrainedmodels layout (growth 32, bn_size 4, block config (6, 12, 24, 16), 64 initial features, bias-free convolutions,
BatchNorm eps 1e-5, AvgPool2d(2, 2) in transitions, drop rate 0, ``last_linear`` for the classifier) under the MODERN module names -
torchvision 0.2.0's 'norm.1' ... cannot be registered in current torch.  The layout is RESTATED, not executed from the package; the stub
is the pin: whoever has the package should compare key lists before loading a real checkpoint.

  F19_dense_layer_{train,eval} one _DenseLayer(96 -> 32) on [3,96,9,7]: a 96-channel prefix of the 128-wide buffer it returns
  F19_dense_block_{train,eval} denseblock1 + transition1 of depth 121 (the stub's modules) on [2,64,10,6]: outputs, gradients, running statistics
  F19_unet_densenet121_hyper   unet.UNetDenseNet(121, 2, use_hypercolumn=True) at [2,3,64,64] with closed-form weights: eval logits plus one
                               training step as SegmentationModel._fit_loop runs it, in the F18 layout.  No weights are stored.

The generator REFUSES to write unless the reference alone meets the guards the tests re-assert: at most 0.1 % of the pixels with
|logit[1]| < 10 x its own f32-vs-f64 error; both classes in the eval masks; the norm1 ReLU of the middle layer of each dense block
passes 20 .. 80 % of its elements (eval and train); its f32-vs-f64 gradient-norm figures within a quarter of the GPU test's bounds.  Full
gradients are recorded for a fixed list of tensors; an input at which the reference's own f32-vs-f64 element error of any of them
exceeds a quarter of the GPU test's 2e-2 is refused."""
import copy
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: densenet_oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root: oracle

torch.manual_seed(0)
torch.set_num_threads(8)


# --------------------------------------------------------------------------- pretrainedmodels stub (build-authored, plain torch)
class _DenseLayer(nn.Module):
    def __init__(self, nin, growth, bn_size):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(nin)
        self.relu1 = nn.ReLU(inplace=False)
        self.conv1 = nn.Conv2d(nin, bn_size * growth, kernel_size=1, stride=1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(bn_size * growth, growth, kernel_size=3, stride=1, padding=1, bias=False)

    def forward(self, x):
        return torch.cat([x, self.conv2(self.relu2(self.norm2(self.conv1(self.relu1(self.norm1(x))))))], 1)


class _Transition(nn.Sequential):
    def __init__(self, nin, nout):
        super().__init__()
        self.add_module('norm', nn.BatchNorm2d(nin))
        self.add_module('relu', nn.ReLU(inplace=True))
        self.add_module('conv', nn.Conv2d(nin, nout, kernel_size=1, stride=1, bias=False))
        self.add_module('pool', nn.AvgPool2d(kernel_size=2, stride=2))


class DenseNet(nn.Module):
    def __init__(self, cfg, growth=32, bn_size=4, init=64, num_classes=1000):
        super().__init__()
        self.features = nn.Sequential(OrderedDict([('conv0', nn.Conv2d(3, init, kernel_size=7, stride=2, padding=3, bias=False)),
                                                   ('norm0', nn.BatchNorm2d(init)), ('relu0', nn.ReLU(inplace=True)),
                                                   ('pool0', nn.MaxPool2d(kernel_size=3, stride=2, padding=1))]))
        n = init
        for i, layers in enumerate(cfg):
            block = nn.Sequential()
            for l in range(layers):
                block.add_module('denselayer%d' % (l + 1), _DenseLayer(n + l * growth, growth, bn_size))
            self.features.add_module('denseblock%d' % (i + 1), block)
            n += layers * growth
            if i != len(cfg) - 1:
                self.features.add_module('transition%d' % (i + 1), _Transition(n, n // 2))
                n //= 2
        self.features.add_module('norm5', nn.BatchNorm2d(n))
        self.last_linear = nn.Linear(n, num_classes)

    def forward(self, x):
        y = F.relu(self.features(x), inplace=True)
        return self.last_linear(F.avg_pool2d(y, kernel_size=7, stride=1).view(y.size(0), -1))


def _factory(cfg):
    def make(num_classes=1000, pretrained=None):
        if pretrained:
            raise RuntimeError('no network: pretrained weights unavailable')
        return DenseNet(cfg, num_classes=num_classes)
    return make


def install_densenet_stub():
    """BEFORE ref_import.install_stubs(): its setdefault keeps this module"""
    pm = types.ModuleType('pretrainedmodels')
    pm.densenet121 = _factory((6, 12, 24, 16))
    sys.modules['pretrainedmodels'] = pm
    import ref_import as R
    R.install_stubs()
    assert sys.modules['pretrainedmodels'] is pm
    return R


E = 'encoders.encoder.features.'
# The tensors whose gradient is recorded IN FULL: a FIXED, REQUIRED list (each at most 33 000 elements, the file stays under 1 MiB) - the
# head, the first conv1 of three blocks, norm1 of the last layer of every block, the first transition's convolution and every
# transition's norm.  An input at which the reference's own fp32 gradient of ANY of them is more than 5e-3 (a quarter of the GPU test's
# 2e-2) from its float64 gradient is refused as a whole; nothing is dropped per tensor.  (denseblock2.denselayer12.norm1.weight is not on
# the list: the reference's own error on it was 5.5e-3 .. 7.4e-3 at every input tried; its bias is.)
FULL_REQUIRED = (['final.1.weight', 'final.1.bias'] + [E + 'denseblock%d.denselayer1.conv1.weight' % b for b in (1, 2, 3)]
                 + [E + 'denseblock1.denselayer6.norm1.weight', E + 'denseblock1.denselayer6.norm1.bias', E + 'denseblock2.denselayer12.norm1.bias']
                 + [E + 'denseblock%d.denselayer%d.norm1.%s' % (b, n, leaf) for b, n in ((3, 24), (4, 16)) for leaf in ('weight', 'bias')]
                 + [E + 'transition1.conv.weight'] + [E + 'transition%d.norm.%s' % (t, leaf) for t in (1, 2, 3) for leaf in ('weight', 'bias')])


# With the plain closed-form fill 99.7 % of the eval pixels land in one class (logit[1] has its median at +0.43 against a head bias of
# -0.008): 'both classes occur' holds, but only just.  The allowed remedy was tried - final.1.bias times 52 gives 50 % - and at none of the
# 16 inputs did the reference then keep its own gradient guards below, so the plain fill stands and the masks stay lopsided.


def relu_pass_fractions(net, run):
    """pass fraction of the norm1 ReLU of the middle layer of each dense block during ``run()``"""
    fr, hooks = [], []
    f = net.encoders.encoder.features
    for i in (1, 2, 3, 4):
        block = getattr(f, 'denseblock%d' % i)
        mid = getattr(block, 'denselayer%d' % (len(block) // 2 + 1))
        hooks.append(mid.relu1.register_forward_hook(lambda m, a, out: fr.append(float((out > 0).double().mean()))))
    try:
        run()
    finally:
        for h in hooks:
            h.remove()
    return fr


def network_fixture(unet, models, name):
    import closed_form as CF
    import densenet_oracle as DO
    from oracle import blocks as OB
    from make_golden import canonical_fn, save
    from make_golden_emptiness import lovasz_loss_any_dtype, grad_norms
    shape = (2, 3, 64, 64)

    def build():
        net = unet.UNetDenseNet(encoder_depth=121, num_classes=2, dropout_2d=0.0, pretrained=False, use_hypercolumn=True, pool0=False)
        canon = canonical_fn(net)
        CF.fill_module(net, canonical=canon)
        return net, canon

    for tag in ['f19'] + ['f19:%d' % i for i in range(1, 16)]:
        X = CF.input_for(tag, shape)
        net, canon = build()
        net.eval()
        with torch.no_grad():
            fr_eval = relu_pass_fractions(net, lambda: net(X))
            logits = net(X)
            logits64 = copy.deepcopy(net).double()(X.double())
        err = float((logits.double() - logits64).abs().max())
        margin = int((logits[:, 1].abs() < 10 * err).sum())
        pos = float((logits[:, 1] > 0).float().mean())
        print('  %s: input %s  relu pass %s  f32 vs f64 %.2e  pixels under 10x %d of %d  positive %.3f' % (
            name, tag, ['%.2f' % f for f in fr_eval], err, margin, logits[:, 1].numel(), pos))
        if margin > 0.001 * logits[:, 1].numel() or not (0.0 < pos < 1.0) or not all(0.2 <= f <= 0.8 for f in fr_eval):
            continue
        out = OrderedDict(x_shape=np.array(X.shape), x=X, input_tag=np.array(tag), relu_pass_mid_eval=np.array(fr_eval), eval_logits=logits,
                          ref_f32_vs_f64_maxabs=err, margin_pixels=margin, eval_positive_fraction=pos)
        out['keys'] = np.array(list(net.state_dict().keys()))
        out['key_shapes'] = np.array(['x'.join(str(d) for d in v.shape) for v in net.state_dict().values()])
        sd = {k: v.clone() for k, v in net.state_dict().items() if canon(k) == k}
        with torch.no_grad():
            o32 = DO.unet_densenet(sd, X, False)
            with OB.bf16_storage():
                o16 = DO.unet_densenet(sd, X, False)
        assert float((o32 - logits).abs().max()) <= 1e-3 * float(logits.abs().max()), 'test-side oracle does not reproduce the reference'
        out['ref_bf16_storage_vs_f32_maxabs'] = float((o16.double() - o32.double()).abs().max())
        T = CF.mask_for('f19', (2, 64, 64))
        out['t'] = T
        net.train()
        n64 = copy.deepcopy(net).double()
        fr_train = relu_pass_fractions(n64, lambda: lovasz_loss_any_dtype(n64(X.double()), T.double()).backward())
        g64 = grad_norms(n64)
        full64 = {k: p.grad.clone() for k, p in n64.named_parameters() if k in FULL_REQUIRED}
        del n64
        if not all(0.2 <= f <= 0.8 for f in fr_train):
            print('  %s: input %s refused: train-mode relu pass %s' % (name, tag, fr_train))
            continue
        out['relu_pass_mid_train'] = np.array(fr_train)
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
        if not (out['ref_f32_vs_f64_gradnorm_rel'] <= 2.5e-3 and out['ref_f32_vs_f64_small_abs'] <= 2.5e-7):
            print('  %s: input %s refused: gradient norms f32 vs f64 %.2e (>= 16 elements), %.2e of the largest norm (< 16)' % (
                name, tag, out['ref_f32_vs_f64_gradnorm_rel'], out['ref_f32_vs_f64_small_abs']))
            continue
        names, gnorm, gsum, has_grad = [], [], [], []
        for k, p in net.named_parameters():
            names.append(k)
            has_grad.append(p.grad is not None)
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            gnorm.append(float(g.double().norm()))
            gsum.append(float(g.double().sum()))
        # full gradients: the fixed list above, every tensor of it within a quarter of the GPU test's 2e-2 in the reference's OWN
        # f32-vs-f64 deviation (largest element error over the largest element) - the rule of the gradient-norm guard above - or the
        # input is refused.  In this network the early encoder gradients of the reference itself are off by up to 1.3e-2 in fp32 at
        # most inputs (transition1.conv.weight); such an input cannot hold anybody to 2e-2
        named = dict(net.named_parameters())
        errs = {k: float((named[k].grad.double() - full64[k]).abs().max() / full64[k].abs().max()) for k in FULL_REQUIRED}
        kept = list(FULL_REQUIRED)
        print('  full gradients (own f32 vs f64):', {k.replace(E, ''): '%.1e' % v for k, v in errs.items()})
        if max(errs.values()) > 5e-3:
            print('  %s: input %s refused: a required full gradient is ill-conditioned in the reference itself' % (name, tag))
            continue
        for k in kept:
            out['fullgrad:' + k] = named[k].grad.clone()
        out['fullgrad_keys'] = np.array(kept)
        out['fullgrad_ref_f32_vs_f64'] = np.array([errs[k] for k in kept])
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
        save(name, **out)
        print('  %s: max|logit| %.2f  bf16 storage %.2e  loss %.5f  grad-norm f32 vs f64 %.2e (small tensors %.2e of the largest norm)  live tensors %d' % (
            name, float(logits.abs().max()), out['ref_bf16_storage_vs_f32_maxabs'], float(loss.detach()), out['ref_f32_vs_f64_gradnorm_rel'],
            out['ref_f32_vs_f64_small_abs'], sum(has_grad)))
        return
    raise AssertionError('%s: no input keeps the guards' % name)


class DenseBlockT(nn.Module):
    """denseblock1 + transition1 of depth 121: six layers on 64 channels share one statistics table, then 256 -> 128 and the pool"""

    def __init__(self):
        super().__init__()
        self.block = nn.Sequential()
        for l in range(6):
            self.block.add_module('denselayer%d' % (l + 1), _DenseLayer(64 + 32 * l, 32, 4))
        self.transition = _Transition(256, 128)

    def forward(self, x):
        return self.transition(self.block(x))


def block_fixture(name, make, tag, shape):
    """make_golden.block_fixture without weights: expected outputs, gradients and (train) the running statistics AFTER the pass; the
    tests rebuild x = closed_form.input_for(tag, shape), gy and the weights from the closed form"""
    import closed_form as CF
    from make_golden import run_block, save
    x = CF.input_for(tag, shape)
    for train in (True, False):
        mod = make()
        CF.fill_module(mod)
        out = run_block(mod, x, train)
        # (a committed file stays under 1 MiB: eval keeps y and gx; train keeps every gradient in full except conv2.weight of the
        #  layers 2 .. 5, recorded as norm and sum under 'gn:' / 'gs:')
        brief = lambda k: k.endswith('conv2.weight') and 'denselayer' in k and not any('denselayer%d.' % l in k for l in (1, 6))
        keep = OrderedDict((k, v) for k, v in out.items() if k in ('y', 'gx') or (train and k.startswith('g:') and not brief(k))
                           or (train and k.startswith('s:') and k.endswith(('running_mean', 'running_var'))))
        if train:
            for k, v in out.items():
                if k.startswith('g:') and brief(k):
                    keep['gn:' + k[2:]], keep['gs:' + k[2:]] = float(v.double().norm()), float(v.double().sum())
        keep['x_shape'], keep['input_tag'] = np.array(shape), np.array(tag)
        save('%s_%s' % (name, 'train' if train else 'eval'), **keep)


def main():
    R = install_densenet_stub()
    assert R.reference_available(), 'reference not mounted'
    unet = R.load('architectures.unet')
    models = R.load_models_module()
    from make_golden import ONLY
    want = lambda name: not ONLY or any(o.startswith(name) for o in ONLY)
    if want('F19_dense_layer'):
        # one layer on a 96-channel prefix of a 128-wide buffer (the layer's output IS that buffer: the input and 32 new channels);
        # 189 pixels: two pixel tiles, the second ragged
        block_fixture('F19_dense_layer', lambda: _DenseLayer(96, 32, 4), 'f19a', (3, 96, 9, 7))
    if want('F19_dense_block'):
        block_fixture('F19_dense_block', DenseBlockT, 'f19b', (2, 64, 10, 6))
    if want('F19_unet_densenet121_hyper'):
        network_fixture(unet, models, 'F19_unet_densenet121_hyper')


if __name__ == '__main__':
    main()
