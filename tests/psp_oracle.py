"""Comparator for PSPNet (TEST INFRASTRUCTURE ONLY): architectures/pspnet.py on the ResNet encoders of architectures/encoders.py:6-45,
as pure functions over a flat state dict, composed from the oracle's blocks (stem, layers, final block) plus the pyramid module and the
up-sampling block in plain torch.  Written from the layout the reference's state dict and forward define - psp.stages.{0..3}.1
(bias-free 1x1 behind AdaptiveAvgPool2d(s)), psp.bottleneck (1x1 with bias over [stage 0 .. stage 3 | feats]), up{4..1}.conv.{0,1,2}
(3x3 zero-padded convolution with bias, BatchNorm2d, PReLU with one slope), final.{0,1} - in the CONCATENATED form the reference
runs, so that the factored HIP path is held to the unfactored arithmetic.  tests/golden/make_golden_psp.py executes the reference
itself; the F20 fixtures pin the two to each other."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import helpers
from oracle import blocks as B
from oracle import specs as OS

SIZES = (1, 2, 3, 6)
ALIASES = OS.alias_map('UNetResNet')            # ResNetEncoders registers the stem and the four layers a second time


def psp_module(sd, p, x, sizes=SIZES, passed=None):
    """PSPModule.forward.  ``passed``: a list that receives the fraction of the bottleneck ReLU that passes."""
    h, w = x.shape[2], x.shape[3]
    priors = []
    for i, s in enumerate(sizes):
        t = B._st(F.conv2d(B._st(F.adaptive_avg_pool2d(x, s)), B._w(sd['%sstages.%d.1.weight' % (p, i)])))
        priors.append(F.interpolate(t, size=(h, w), mode='bilinear', align_corners=B.ALIGN_CORNERS))
    y = F.conv2d(torch.cat(priors + [x], 1), B._w(sd[p + 'bottleneck.weight']), sd[p + 'bottleneck.bias'])
    if passed is not None:
        passed.append(float((y > 0).double().mean()))
    return B._st(F.relu(y))


def psp_upsample(sd, p, x, train, passed=None):
    """PSPUpsample.forward.  ``passed``: a list that receives the fraction of the PReLU's inputs that are NEGATIVE."""
    y = B._st(F.conv2d(B.upsample_bilinear(x, 2), B._w(sd[p + 'conv.0.weight']), sd[p + 'conv.0.bias'], padding=1))
    u = B.batch_norm(sd, p + 'conv.1.', y, train)
    if passed is not None:
        passed.append(float((u < 0).double().mean()))
    return B._st(F.prelu(u, sd[p + 'conv.2.weight']))


def pspnet(sd, x, train, depth=34, p='', passed=None):
    """PSPNet.forward with use_hypercolumn=True, pool0=False; F.dropout2d is an identity (dropout_2d = 0 in the generator).
    ``passed``: receives [bottleneck ReLU pass fraction, negative fraction of the PReLU inputs of up4, up3, up2, up1]."""
    e = p + 'encoders.encoder.'
    y = B.resnet_stem(sd, e, x, train, False)
    for i in (1, 2, 3, 4):
        y = B.resnet_layer(sd, e, y, train, depth, i)
    y = psp_module(sd, p + 'psp.', y, passed=passed)
    u4 = psp_upsample(sd, p + 'up4.', y, train, passed)
    u3 = psp_upsample(sd, p + 'up3.', u4, train, passed)
    u2 = psp_upsample(sd, p + 'up2.', u3, train, passed)
    u1 = psp_upsample(sd, p + 'up1.', u2, train, passed)
    hyper = torch.cat([u1, B.upsample_bilinear(u2, 2), B.upsample_bilinear(u3, 4), B.upsample_bilinear(u4, 8)], 1)
    y = B.conv2d_bn_relu(sd, p + 'final.0.', hyper, train)
    return F.conv2d(y, sd[p + 'final.1.weight'], sd[p + 'final.1.bias'])


def _psp_module(spec, p, features, out_features, sizes=SIZES):
    for i in range(len(sizes)):
        spec['%sstages.%d.1.weight' % (p, i)] = ((features, features, 1, 1), 'conv_w')
    spec[p + 'bottleneck.weight'] = ((out_features, features * (len(sizes) + 1), 1, 1), 'conv_w')
    spec[p + 'bottleneck.bias'] = ((out_features,), 'conv_b')


def _psp_upsample(spec, p, cin, cout):
    spec[p + 'conv.0.weight'] = ((cout, cin, 3, 3), 'conv_w')
    spec[p + 'conv.0.bias'] = ((cout,), 'conv_b')
    OS._bn(spec, p + 'conv.1.', cout)
    spec[p + 'conv.2.weight'] = ((1,), 'prelu_w')


def spec_psp_module(features=64, out_features=128):
    s = OrderedDict()
    _psp_module(s, '', features, out_features)
    return s


def spec_psp_upsample(cin=32, cout=16):
    s = OrderedDict()
    _psp_upsample(s, '', cin, cout)
    return s


def spec_pspnet(depth=34, num_classes=2, deep=1024):
    """State-dict spec {key: (shape, kind)} under the canonical spellings, in the module tree's order."""
    s = OrderedDict()
    b = OS._resnet(s, 'encoders.encoder.', depth, 3, True)
    _psp_module(s, 'psp.', b, deep)
    for n, c in ((4, deep), (3, deep // 2), (2, deep // 4), (1, deep // 8)):
        _psp_upsample(s, 'up%d.' % n, c, c // 2)
    OS._conv2d_bn_relu(s, 'final.0.', 15 * b // 8, b // 8)
    s['final.1.weight'] = ((num_classes, b // 8, 1, 1), 'conv_w')
    s['final.1.bias'] = ((num_classes,), 'conv_b')
    return s


def expand_aliases(sd):
    return helpers.expand_aliases(sd, ALIASES)


def closed_form_state(spec):
    import closed_form as CF
    return CF.state_for((k, s) for k, (s, _) in spec.items())
