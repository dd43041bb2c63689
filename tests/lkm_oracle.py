"""Comparator for LargeKernelMatters (TEST INFRASTRUCTURE ONLY): architectures/large_kernel_matters.py with the blocks of
architectures/base.py:152-197 on the ResNet encoders of architectures/encoders.py:6-45, as pure functions over a flat state dict,
composed from the oracle's blocks (stem, layers, Conv2dBnRelu, DeconvConv2dBnRelu).  Written from the layout the reference's state dict
and forward define - gcn{2..5}.conv{1,2}.{0,1}.{batch_norm,conv}, {enc,dec}_br{..}.conv.{0,1}, deconv{5..2}.{batch_norm,deconv}, final -
with every Conv2dBnRelu on its own padded copy, as the reference runs them: the paired HIP path is held to the unpaired arithmetic.
tests/golden/make_golden_lkm.py executes the reference itself; the F21 fixtures pin the two to each other."""
from collections import OrderedDict

import torch.nn.functional as F

import helpers
from oracle import blocks as B
from oracle import specs as OS

ALIASES = OS.alias_map('UNetResNet')            # ResNetEncoders registers the stem and the four layers a second time


def gcn(sd, p, x, train, use_relu=False, passed=None):
    """GlobalConvolutionalNetwork.forward.  ``passed``: receives the pass fraction of each of the four ReLUs (use_relu only)."""
    def cbr(q, t):
        y = B.conv2d_bn_relu(sd, p + q, t, train, use_relu=use_relu)
        if passed is not None and use_relu:
            passed.append(float((y > 0).double().mean()))
        return y
    return B._st(cbr('conv1.1.', cbr('conv1.0.', x)) + cbr('conv2.1.', cbr('conv2.0.', x)))


def boundary_refinement(sd, p, x, train, passed=None):
    """BoundaryRefinement.forward.  ``passed``: receives the pass fraction of the inner ReLU."""
    y = B.conv2d_bn_relu(sd, p + 'conv.0.', x, train)
    if passed is not None:
        passed.append(float((y > 0).double().mean()))
    return B._st(x + B.conv2d_bn_relu(sd, p + 'conv.1.', y, train, use_relu=False))


def lkm(sd, x, train, depth=34, use_relu=True, p='', passed=None):
    """LargeKernelMatters.forward with pool0=False; F.dropout2d is an identity (dropout_2d = 0)."""
    e = p + 'encoders.encoder.'
    y = B.resnet_stem(sd, e, x, train, False)
    enc = []
    for i in (1, 2, 3, 4):
        y = B.resnet_layer(sd, e, y, train, depth, i)
        enc.append(y)
    g = [boundary_refinement(sd, '%senc_br%d.' % (p, n), gcn(sd, '%sgcn%d.' % (p, n), t, train, use_relu, passed), train, passed)
         for n, t in zip((2, 3, 4, 5), enc)]
    br = lambda n, t: boundary_refinement(sd, '%sdec_br%d.' % (p, n), t, train, passed)
    up = lambda n, t: B.deconv_conv2d_bn_relu(sd, '%sdeconv%d.' % (p, n), t, train)
    d5 = up(5, g[3])
    d4 = up(4, br(4, B._st(d5 + g[2])))
    d3 = up(3, br(3, B._st(d4 + g[1])))
    d2 = br(1, up(2, br(2, B._st(d3 + g[0]))))
    return F.conv2d(d2, sd[p + 'final.weight'], sd[p + 'final.bias'])


def _gcn(spec, p, cin, cout, k):
    OS._conv2d_bn_relu(spec, p + 'conv1.0.', cin, cout, (k, 1))
    OS._conv2d_bn_relu(spec, p + 'conv1.1.', cout, cout, (1, k))
    OS._conv2d_bn_relu(spec, p + 'conv2.0.', cin, cout, (1, k))
    OS._conv2d_bn_relu(spec, p + 'conv2.1.', cout, cout, (k, 1))


def _br(spec, p, c, k=3):
    OS._conv2d_bn_relu(spec, p + 'conv.0.', c, c, (k, k))
    OS._conv2d_bn_relu(spec, p + 'conv.1.', c, c, (k, k))


def spec_gcn(cin=64, cout=21, k=9):
    s = OrderedDict()
    _gcn(s, '', cin, cout, k)
    return s


def spec_br(c=21, k=3):
    s = OrderedDict()
    _br(s, '', c, k)
    return s


def spec_lkm(depth=34, num_classes=2, k=9, c=21):
    """State-dict spec {key: (shape, kind)} under the canonical spellings, in the module tree's order."""
    s = OrderedDict()
    b = OS._resnet(s, 'encoders.encoder.', depth, 3, True)
    for n, cin in ((2, b // 8), (3, b // 4), (4, b // 2), (5, b)):
        _gcn(s, 'gcn%d.' % n, cin, c, k)
    for name in ('enc_br2', 'enc_br3', 'enc_br4', 'enc_br5', 'dec_br1', 'dec_br2', 'dec_br3', 'dec_br4'):
        _br(s, name + '.', c)
    for n in (5, 4, 3, 2):
        OS._bn(s, 'deconv%d.batch_norm.' % n, c)
        s['deconv%d.deconv.weight' % n] = ((c, c, 3, 3), 'convT_w')
        s['deconv%d.deconv.bias' % n] = ((c,), 'convT_b')
    s['final.weight'] = ((num_classes, c, 1, 1), 'conv_w')
    s['final.bias'] = ((num_classes,), 'conv_b')
    return s


def expand_aliases(sd):
    return helpers.expand_aliases(sd, ALIASES)


def closed_form_state(spec):
    import closed_form as CF
    return CF.state_for((k, s) for k, (s, _) in spec.items())
