"""Comparator for UNetDenseNet (TEST INFRASTRUCTURE ONLY): architectures/unet.py:238-307 on the DenseNet encoders of
architectures/encoders.py:121-164, composed from the oracle's blocks (stem, decoder, final block) plus the dense layer and the
transition in plain torch.  The encoder layout (torchvision / pretrainedmodels densenet.py as densenet121 builds it: growth 32, bn_size 4,
64 initial features, bias-free convolutions, AvgPool2d(2, 2) transitions, modern module names) is RESTATED from the public source, not
executed: tests/golden/make_golden_densenet.py holds the same restatement as the stub the reference's own unet.py ran on, and the F19
fixtures pin the two to each other."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import helpers
from oracle import blocks as B
from oracle import specs as OS

CFG = {121: (6, 12, 24, 16), 169: (6, 12, 32, 32), 201: (6, 12, 48, 32)}
WIDTHS = {121: [256, 512, 1024, 1024], 169: [256, 512, 1280, 1664], 201: [256, 512, 1792, 1920]}
GROWTH, BN_SIZE, INIT = 32, 4, 64
ENC = 'encoders.encoder.'
FEAT = ENC + 'features.'
# {alias prefix: canonical prefix}: DenseNetEncoders registers the stem, the blocks and the transitions a second time (encoders.py:137-153)
ALIASES = OrderedDict([('encoders.conv1.0.', FEAT + 'conv0.'), ('encoders.conv1.1.', FEAT + 'norm0.'),
                       ('encoders.encoder2.', FEAT + 'denseblock1.'), ('encoders.transition1.', FEAT + 'transition1.'),
                       ('encoders.encoder3.', FEAT + 'denseblock2.'), ('encoders.transition2.', FEAT + 'transition2.'),
                       ('encoders.encoder4.', FEAT + 'denseblock3.'), ('encoders.transition3.', FEAT + 'transition3.'),
                       ('encoders.encoder5.', FEAT + 'denseblock4.')])


def dense_layer(sd, p, x, train, passed=None):
    """-> the 32 new channels: conv2(relu(norm2(conv1(relu(norm1(x))))));  relu(norm1(x)) is an operand of the HIP kernel, rounded to the
    storage type like a stored activation.  ``passed``: a list that receives the fraction of norm1's ReLU that passes."""
    a = F.relu(B.batch_norm(sd, p + 'norm1.', x, train))
    if passed is not None:
        passed.append(float((a > 0).double().mean()))
    y = B._st(F.conv2d(B._st(a), B._w(sd[p + 'conv1.weight'])))
    y = B._st(F.relu(B.batch_norm(sd, p + 'norm2.', y, train)))
    return B._st(F.conv2d(y, B._w(sd[p + 'conv2.weight']), None, padding=1))


def dense_block(sd, p, x, train, n, passed=None):
    for i in range(n):
        x = torch.cat([x, dense_layer(sd, '%sdenselayer%d.' % (p, i + 1), x, train, passed if i == n // 2 else None)], 1)
    return x


def transition(sd, p, x, train):
    y = B._st(F.conv2d(B._st(F.relu(B.batch_norm(sd, p + 'norm.', x, train))), B._w(sd[p + 'conv.weight'])))
    return B._st(F.avg_pool2d(y, 2, 2))


def unet_densenet(sd, x, train, depth=121, use_hypercolumn=True, p='', passed=None):
    """``passed``: a list that receives, per dense block, the pass fraction of the middle layer's norm1 ReLU."""
    f = p + FEAT
    y = B._st(F.conv2d(B._st(x), B._w(sd[f + 'conv0.weight']), None, stride=2, padding=3))
    y = B._st(F.relu(B.batch_norm(sd, f + 'norm0.', y, train)))
    es = []
    for i, n in enumerate(CFG[depth]):
        y = dense_block(sd, '%sdenseblock%d.' % (f, i + 1), y, train, n, passed)
        es.append(y)
        if i < 3:
            y = transition(sd, '%stransition%d.' % (f, i + 1), y, train)
    e2, e3, e4, e5 = es
    c = B.conv2d_bn_relu(sd, p + 'center.0.', e5, train)
    c = B.conv2d_bn_relu(sd, p + 'center.1.', c, train)
    c = B._st(F.avg_pool2d(c, 2, 2))
    d5 = B.decoder_block(sd, p + 'dec5.', c, e5, train)
    d4 = B.decoder_block(sd, p + 'dec4.', d5, e4, train)
    d3 = B.decoder_block(sd, p + 'dec3.', d4, e3, train)
    d2 = B.decoder_block(sd, p + 'dec2.', d3, e2, train)
    d1 = B.decoder_block(sd, p + 'dec1.', d2, None, train)
    if use_hypercolumn:
        d1 = torch.cat([d1, B.upsample_bilinear(d2, 2), B.upsample_bilinear(d3, 4), B.upsample_bilinear(d4, 8), B.upsample_bilinear(d5, 16)], 1)
    y = B.conv2d_bn_relu(sd, p + 'final.0.', d1, train)
    return F.conv2d(y, sd[p + 'final.1.weight'], sd[p + 'final.1.bias'])


def _densenet(spec, p, depth):
    f = p + 'features.'
    spec[f + 'conv0.weight'] = ((INIT, 3, 7, 7), 'conv_w')
    OS._bn(spec, f + 'norm0.', INIT)
    n = INIT
    for i, layers in enumerate(CFG[depth]):
        for l in range(layers):
            q = '%sdenseblock%d.denselayer%d.' % (f, i + 1, l + 1)
            OS._bn(spec, q + 'norm1.', n + l * GROWTH)
            spec[q + 'conv1.weight'] = ((BN_SIZE * GROWTH, n + l * GROWTH, 1, 1), 'conv_w')
            OS._bn(spec, q + 'norm2.', BN_SIZE * GROWTH)
            spec[q + 'conv2.weight'] = ((GROWTH, BN_SIZE * GROWTH, 3, 3), 'conv_w')
        n += layers * GROWTH
        if i < 3:
            q = '%stransition%d.' % (f, i + 1)
            OS._bn(spec, q + 'norm.', n)
            spec[q + 'conv.weight'] = ((n // 2, n, 1, 1), 'conv_w')
            n //= 2
    OS._bn(spec, f + 'norm5.', n)
    spec[p + 'last_linear.weight'] = ((1000, n), 'lin_w')
    spec[p + 'last_linear.bias'] = ((1000,), 'lin_b')


def spec_unet_densenet(depth=121, num_classes=2, use_hypercolumn=True):
    """State-dict spec {key: (shape, kind)} under the canonical spellings, in the module tree's order."""
    s = OrderedDict()
    _densenet(s, ENC, depth)
    e = WIDTHS[depth]
    b = e[3]
    OS._conv2d_bn_relu(s, 'center.0.', b, b)
    OS._conv2d_bn_relu(s, 'center.1.', b, e[2])
    OS._decoder_block(s, 'dec5.', b + e[2], b, b // 8)
    OS._decoder_block(s, 'dec4.', e[2] + b // 8, b // 2, b // 8)
    OS._decoder_block(s, 'dec3.', e[1] + b // 8, b // 4, b // 8)
    OS._decoder_block(s, 'dec2.', e[0] + b // 8, b // 8, b // 8)
    OS._decoder_block(s, 'dec1.', b // 8, b // 16, b // 8)
    OS._conv2d_bn_relu(s, 'final.0.', (5 if use_hypercolumn else 1) * b // 8, b // 8)
    s['final.1.weight'] = ((num_classes, b // 8, 1, 1), 'conv_w')
    s['final.1.bias'] = ((num_classes,), 'conv_b')
    return s


def expand_aliases(sd):
    return helpers.expand_aliases(sd, ALIASES)


def closed_form_state(spec):
    import closed_form as CF
    return CF.state_for((k, s) for k, (s, _) in spec.items())
