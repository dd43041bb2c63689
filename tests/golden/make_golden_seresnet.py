#!/usr/bin/env python
"""Generate the F17 fixtures (UNetSeResNet) by EXECUTING THE REFERENCE'S OWN architectures/unet.py.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_seresnet.py
Same conventions as make_golden_emptiness.py: closed-form weights keyed by state-dict name (closed_form.py), the reference's sources
imported through the stubs of ref_import.py, only .npz data is written.

The reference builds its SE-ResNet encoders from ``pretrainedmodels.__dict__['se_resnet50' | 'se_resnet101' | 'se_resnet152']``
(architectures/encoders.py:48-83).  That package is not available here, so - exactly as ref_import.py does for torchvision's ResNets -
this file puts BUILD-AUTHORED factories with the package's public layout (senet.py: SENet / SEResNetBottleneck / SEModule, groups 1,
reduction 16, inplanes 64, input_3x3 False, 1x1 downsample without padding, no dropout) into the stub module.  The layout is RESTATED,
not executed from the package: whoever has the package should compare key lists before loading a real checkpoint.

  F17_se_bottleneck_{train,eval}     SEResNetBottleneck(64 -> 256, planes 64, stride 1, with downsample) on [2,64,6,10]: x, y, gy, gx,
                                     (train) every parameter gradient and the BatchNorm running statistics after the pass
  F17_se_bottleneck_s2_{train,eval}  SEResNetBottleneck(256 -> 512, planes 128, stride 2) on [2,256,6,10].  No committed file may pass
                                     1 MiB and this block's gradients alone are 1.6 MB, so: the block has its own files, its closed-form
                                     x and gy are rebuilt by the tests (CF.input_for), and the three gradients above 40 000 elements are
                                     stored IN FULL in the companion files F17_se_bottleneck_s2_train_g1 (conv2.weight) and _g2
                                     (conv3.weight, downsample.0.weight); `companions` in the main file counts them
  F17_unet_seresnet50_hyper          unet.UNetSeResNet(50, 2, use_hypercolumn=True) at [2,3,64,64]: eval logits plus one training step as
                                     SegmentationModel._fit_loop runs it (lovasz_loss, Adam lr 1e-4 + L2 1e-4), laid out like the F14 /
                                     F15 network fixtures, with the reference's own error figures (see make_golden_emptiness.py)
  F17_unet_seresnet101_hyper         depth 101, eval only

The generator REFUSES to write a fixture unless the reference alone satisfies:
  gate spread    in every encoder stage at least half of the SE gates lie in [0.1, 0.9] (a saturated gate would hide a wrong FC);
                 the closed-form fill of every se_module.fc2.weight is multiplied by `fc2_scale` (recorded) until it does
  mask margin    pixels with |logit[1]| < 10 x ref_f32_vs_f64_maxabs are at most 0.1 % of the map; the input tag is changed until the
                 reference stays within it (recorded as `input_tag`; the pixels' count as `margin_pixels`)
"""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: seresnet_oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root: oracle
import closed_form as CF          # noqa: E402
import ref_import as R            # noqa: E402
from make_golden import canonical_fn, save, run_block, ONLY          # noqa: E402
from make_golden_emptiness import lovasz_loss_any_dtype, grad_norms          # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)

FC2_SCALES = (1.0, 0.5, 0.25, 0.125, 0.0625, 2.0, 4.0)
BIG = 40000
COMPANION_BYTES = 800 * 1024          # a committed file stays under 1 MiB (1 048 576 bytes), the repository's limit for new files


# --------------------------------------------------------------------------- pretrainedmodels stub (build-authored, plain torch)
class SEModule(nn.Module):
    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, channels // reduction, kernel_size=1, padding=0)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(channels // reduction, channels, kernel_size=1, padding=0)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        s = self.sigmoid(self.fc2(self.relu(self.fc1(self.avg_pool(x)))))
        return x * s


class SEResNetBottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, groups, reduction, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False, stride=stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
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


class SENet(nn.Module):
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
        layers = [SEResNetBottleneck(self.inplanes, planes, 1, 16, stride, down)]
        self.inplanes = planes * 4
        layers += [SEResNetBottleneck(self.inplanes, planes, 1, 16) for _ in range(1, n)]
        return nn.Sequential(*layers)


def _factory(counts):
    def make(num_classes=1000, pretrained=None):
        if pretrained:
            raise RuntimeError('no network: pretrained weights unavailable')
        return SENet(counts, num_classes)
    return make


def install_senet_stub():
    R.install_stubs()
    pm = sys.modules['pretrainedmodels']
    for name, counts in (('se_resnet50', [3, 4, 6, 3]), ('se_resnet101', [3, 4, 23, 3]), ('se_resnet152', [3, 8, 36, 3])):
        setattr(pm, name, _factory(counts))            # encoders.py reads pretrainedmodels.__dict__[name]


# --------------------------------------------------------------------------- helpers
def scale_fc2(module, scale):
    for k, p in module.named_parameters():
        if k.endswith('se_module.fc2.weight'):
            p.data.mul_(scale)


def gate_fractions(module, stages, run):
    """fraction of SE gates in [0.1, 0.9] per stage while ``run()`` executes; ``stages`` = [[SEModule, ..], ..]"""
    seen = [[] for _ in stages]
    hooks = [m.sigmoid.register_forward_hook(lambda mod, i, o, b=seen[si]: b.append(o.detach().reshape(-1)))
             for si, st in enumerate(stages) for m in st]
    try:
        run()
    finally:
        for h in hooks:
            h.remove()
    out = []
    for b in seen:
        g = torch.cat(b)
        out.append(float(((g >= 0.1) & (g <= 0.9)).float().mean()))
    return out


def block_fixture(name, make, x, store_inputs, split_big):
    chosen = None
    for scale in FC2_SCALES:
        ok = True
        for train in (True, False):
            mod = make()
            CF.fill_module(mod)
            scale_fc2(mod, scale)
            mod.train(train)
            fr = gate_fractions(mod, [[mod.se_module]], lambda: mod(x))          # (a throw-away module: the pass moves the running statistics)
            ok = ok and fr[0] >= 0.5
        if ok:
            chosen = scale
            break
    assert chosen is not None, '%s: no fc2 scale spreads the gates' % name
    for train in (True, False):
        mod = make()
        CF.fill_module(mod)
        scale_fc2(mod, chosen)
        mod.train(train)
        probe = copy.deepcopy(mod)
        fr = gate_fractions(probe, [[probe.se_module]], lambda: probe(x))
        r = run_block(mod, x, train)
        out = OrderedDict(fc2_scale=np.float32(chosen), gate_frac_mid=np.array(fr), x_shape=np.array(x.shape))
        big = OrderedDict()
        for k, v in r.items():
            if k in ('x', 'gy') and not store_inputs:
                continue
            if k.startswith('g:'):
                if not train:
                    continue
                if split_big and v.numel() > BIG:
                    big[k] = v
                    continue
            if k.startswith('s:'):
                if not (train and k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))):
                    continue
            out[k] = v
        # the gradients above BIG elements go to companion files, filled in order up to COMPANION_BYTES each
        groups, size = [], COMPANION_BYTES + 1
        for k, v in big.items():
            if size + v.numel() * 4 > COMPANION_BYTES:
                groups.append(OrderedDict())
                size = 0
            groups[-1][k] = v
            size += v.numel() * 4
        out['companions'] = np.array(len(groups))
        for i, g in enumerate(groups):
            save('%s_%s_g%d' % (name, 'train' if train else 'eval', i + 1), **g)
        save('%s_%s' % (name, 'train' if train else 'eval'), **out)
    print('  %s: fc2 scale %g, gates in [0.1, 0.9] %.2f' % (name, chosen, fr[0]))


def network_fixture(unet, models, name, depth, train_step):
    import seresnet_oracle as SO
    from oracle import blocks as OB
    shape = (2, 3, 64, 64)

    def build(scale):
        net = unet.UNetSeResNet(encoder_depth=depth, num_classes=2, dropout_2d=0.0, pretrained=False, use_hypercolumn=True, pool0=False)
        canon = canonical_fn(net)
        CF.fill_module(net, canonical=canon)
        scale_fc2(net, scale)
        return net, canon
    enc = lambda net: [[b.se_module for b in getattr(net.encoders.encoder, 'layer%d' % i)] for i in (1, 2, 3, 4)]
    picked = None
    for tag in ['f17'] + ['f17:%d' % i for i in range(1, 16)]:
        X = CF.input_for(tag, shape)
        for scale in FC2_SCALES:
            net, canon = build(scale)
            net.eval()
            with torch.no_grad():
                fr_eval = gate_fractions(net, enc(net), lambda: net(X))
            if min(fr_eval) >= 0.5:
                break
        else:
            continue
        net.eval()
        with torch.no_grad():
            logits = net(X)
            logits64 = copy.deepcopy(net).double()(X.double())
        err = float((logits.double() - logits64).abs().max())
        margin = int((logits[:, 1].abs() < 10 * err).sum())
        print('  %s: input %s fc2 scale %g  gates %s  f32 vs f64 %.2e  pixels under 10x %d of %d' % (
            name, tag, scale, ['%.2f' % f for f in fr_eval], err, margin, logits[:, 1].numel()))
        if margin <= 0.001 * logits[:, 1].numel():
            picked = (tag, scale, X, net, canon, logits, err, margin, fr_eval)
            break
    assert picked is not None, '%s: no input keeps the mask margin' % name
    tag, scale, X, net, canon, logits, err, margin, fr_eval = picked
    out = OrderedDict(x_shape=np.array(X.shape), x=X, input_tag=np.array(tag), fc2_scale=np.float32(scale), gate_frac_mid_eval=np.array(fr_eval),
                      eval_logits=logits, ref_f32_vs_f64_maxabs=err, margin_pixels=margin)
    out['keys'] = np.array(list(net.state_dict().keys()))
    out['key_shapes'] = np.array(['x'.join(str(d) for d in v.shape) for v in net.state_dict().values()])
    sd = {k: v.clone() for k, v in net.state_dict().items() if canon(k) == k}
    with torch.no_grad():
        o32 = SO.unet_seresnet(sd, X, False, depth=depth)
        with OB.bf16_storage():
            o16 = SO.unet_seresnet(sd, X, False, depth=depth)
    assert float((o32 - logits).abs().max()) <= 1e-3 * float(logits.abs().max()), 'test-side oracle does not reproduce the reference'
    out['ref_bf16_storage_vs_f32_maxabs'] = float((o16.double() - o32.double()).abs().max())
    msg = '  %s: max|logit| %.2f  bf16 storage %.2e' % (name, float(logits.abs().max()), out['ref_bf16_storage_vs_f32_maxabs'])
    if train_step:
        T = CF.mask_for('f17', (2, 64, 64))
        out['t'] = T
        net.train()
        n64 = copy.deepcopy(net).double()
        lovasz_loss_any_dtype(n64(X.double()), T.double()).backward()
        g64 = grad_norms(n64)
        fr_train = gate_fractions(n64, enc(n64), lambda: n64(X.double()))
        assert min(fr_train) >= 0.5, 'train-mode gates saturate: %s' % fr_train
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
        # (tensors under the tests' skip rule - convolution biases in front of a train-mode BatchNorm, analytically zero - have no relative error;
        # and tensors of fewer than 16 elements - the one-element spatial-SE biases, sums over every pixel that cancel almost completely -
        # are measured absolutely, relative to the largest gradient norm, as tests/test_gpu_models.py:139-144 bounds them)
        numel = {k: p.numel() for k, p in net.named_parameters()}
        gmax = max(g64.values())
        out['ref_f32_vs_f64_gradnorm_rel'] = max(abs(g32[k] - g64[k]) / g64[k] for k in g64 if g64[k] > 1e-4 and numel[k] >= 16)
        out['ref_f32_vs_f64_small_abs'] = max(abs(g32[k] - g64[k]) / gmax for k in g64 if g64[k] > 1e-4 and numel[k] < 16)
        out['ref_f32_vs_f64_small_rel'] = max(abs(g32[k] - g64[k]) / g64[k] for k in g64 if g64[k] > 1e-4 and numel[k] < 16)
        names, gnorm, gsum, has_grad = [], [], [], []
        for k, p in net.named_parameters():
            names.append(k)
            has_grad.append(p.grad is not None)
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            gnorm.append(float(g.double().norm()))
            gsum.append(float(g.double().sum()))
        named = dict(net.named_parameters())
        for k in ('final.1.weight', 'final.1.bias', 'encoders.encoder.layer1.0.se_module.fc1.weight', 'encoders.encoder.layer1.0.se_module.fc1.bias',
                  'encoders.encoder.layer1.0.se_module.fc2.weight', 'encoders.encoder.layer1.0.se_module.fc2.bias',
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
            float(loss.detach()), out['ref_f32_vs_f64_gradnorm_rel'], out['ref_f32_vs_f64_small_abs'], out['ref_f32_vs_f64_small_rel'], min(v for v, h in zip(gnorm, has_grad) if h and v > 1e-4), sum(has_grad))
    save(name, **out)
    print(msg)


def main():
    assert R.reference_available(), 'reference not mounted'
    install_senet_stub()
    unet = R.load('architectures.unet')
    models = R.load_models_module()
    down = lambda cin, cout, s: nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, stride=s, padding=0, bias=False), nn.BatchNorm2d(cout))
    want = lambda name: not ONLY or any(o.startswith(name) for o in ONLY)          # `make_golden_seresnet.py F17_se_bottleneck_train ..`: only those
    if want('F17_se_bottleneck'):
        block_fixture('F17_se_bottleneck', lambda: SEResNetBottleneck(64, 64, 1, 16, 1, down(64, 256, 1)), CF.input_for('f17a', (2, 64, 6, 10)), True, False)
    if want('F17_se_bottleneck_s2'):
        block_fixture('F17_se_bottleneck_s2', lambda: SEResNetBottleneck(256, 128, 1, 16, 2, down(256, 512, 2)), CF.input_for('f17b', (2, 256, 6, 10)), False, True)
    if want('F17_unet_seresnet50_hyper'):
        network_fixture(unet, models, 'F17_unet_seresnet50_hyper', 50, True)
    if want('F17_unet_seresnet101_hyper'):
        network_fixture(unet, models, 'F17_unet_seresnet101_hyper', 101, False)


if __name__ == '__main__':
    main()
