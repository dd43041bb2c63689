"""Comparator for UNetSeResNetXt (TEST INFRASTRUCTURE ONLY): architectures/unet.py:175-235 on the SE-ResNeXt encoders of
architectures/encoders.py:86-118, built on tests/seresnet_oracle.py - the stem, the SE gate, the decoder and the final block are that
file's; only the bottleneck differs.  The encoder layout (pretrainedmodels senet.py: SENet / SEResNeXtBottleneck / SEModule as
se_resnext50_32x4d / se_resnext101_32x4d build them: groups 32, base width 4, the grouped 3x3 conv2 carries the stride, conv1 is a plain
1x1) is RESTATED from the package's public source, not executed: tests/golden/make_golden_seresnext.py holds the same restatement as
the stub the reference's own unet.py ran on, and the F18 fixtures pin the two to each other."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import blocks as B
from oracle import specs as OS
import seresnet_oracle as SO
from seresnet_oracle import ENC, ALIASES, expand_aliases, closed_form_state, block_fixture, se_gate          # noqa: F401  (re-exported)

COUNTS = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3]}
GROUPS, BASE_WIDTH = 32, 4


def width_of(planes):
    return planes * BASE_WIDTH // 64 * GROUPS


def sx_bottleneck(sd, p, x, train, stride, gates=None):
    """SEResNeXtBottleneck: conv1 1x1 stride 1, conv2 3x3 groups 32 with the stride; out = relu(bn3(conv3) * gate + shortcut)"""
    y = B._st(F.relu(B.batch_norm(sd, p + 'bn1.', B._st(F.conv2d(x, B._w(sd[p + 'conv1.weight']))), train)))
    y = B._st(F.relu(B.batch_norm(sd, p + 'bn2.', B._st(F.conv2d(y, B._w(sd[p + 'conv2.weight']), None, stride=stride, padding=1, groups=GROUPS)), train)))
    z = B.batch_norm(sd, p + 'bn3.', B._st(F.conv2d(y, B._w(sd[p + 'conv3.weight']))), train)
    if (p + 'downsample.0.weight') in sd:
        x = B._st(F.conv2d(x, B._w(sd[p + 'downsample.0.weight']), None, stride=stride))
        x = B._st(B.batch_norm(sd, p + 'downsample.1.', x, train))
    g = se_gate(sd, p + 'se_module.', z)
    if gates is not None:
        gates.append(g.detach())
    return B._st(F.relu(z * g + x))


def sx_layer(sd, p, x, train, depth, idx, gates=None):
    for b in range(COUNTS[depth][idx - 1]):
        x = sx_bottleneck(sd, '%slayer%d.%d.' % (p, idx, b), x, train, 2 if (b == 0 and idx > 1) else 1, gates)
    return x


def unet_seresnext(sd, x, train, depth=50, use_hypercolumn=True, p='', gates=None):
    """``gates``: a list that receives one list of gate tensors per encoder stage."""
    e = p + ENC
    y = B.resnet_stem(sd, e + 'layer0.', x, train, False)
    es = []
    for i in (1, 2, 3, 4):
        stage = [] if gates is not None else None
        y = sx_layer(sd, e, y, train, depth, i, stage)
        es.append(y)
        if gates is not None:
            gates.append(stage)
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


def block_shapes(cin, planes, cout):
    """{state-dict key: shape} of one SEResNeXtBottleneck with a projection shortcut, in the module's order."""
    w = width_of(planes)
    shapes = OrderedDict([('conv1.weight', (w, cin, 1, 1)), ('conv2.weight', (w, w // GROUPS, 3, 3)), ('conv3.weight', (cout, w, 1, 1)),
                          ('se_module.fc1.weight', (cout // 16, cout, 1, 1)), ('se_module.fc1.bias', (cout // 16,)),
                          ('se_module.fc2.weight', (cout, cout // 16, 1, 1)), ('se_module.fc2.bias', (cout,)),
                          ('downsample.0.weight', (cout, cin, 1, 1))])
    for p, ch in (('bn1.', w), ('bn2.', w), ('bn3.', cout), ('downsample.1.', cout)):
        for leaf in ('weight', 'bias', 'running_mean', 'running_var'):
            shapes[p + leaf] = (ch,)
        shapes[p + 'num_batches_tracked'] = ()
    return shapes


def _senext(spec, p, depth, with_last_linear):
    spec[p + 'layer0.conv1.weight'] = ((64, 3, 7, 7), 'conv_w')
    OS._bn(spec, p + 'layer0.bn1.', 64)
    inpl = 64
    for li, (planes, n) in enumerate(zip([64, 128, 256, 512], COUNTS[depth]), start=1):
        w = width_of(planes)
        for b in range(n):
            q = '%slayer%d.%d.' % (p, li, b)
            C = planes * 4
            spec[q + 'conv1.weight'] = ((w, inpl, 1, 1), 'conv_w'); OS._bn(spec, q + 'bn1.', w)
            spec[q + 'conv2.weight'] = ((w, w // GROUPS, 3, 3), 'conv_w'); OS._bn(spec, q + 'bn2.', w)
            spec[q + 'conv3.weight'] = ((C, w, 1, 1), 'conv_w'); OS._bn(spec, q + 'bn3.', C)
            spec[q + 'se_module.fc1.weight'] = ((C // 16, C, 1, 1), 'conv_w'); spec[q + 'se_module.fc1.bias'] = ((C // 16,), 'conv_b')
            spec[q + 'se_module.fc2.weight'] = ((C, C // 16, 1, 1), 'conv_w'); spec[q + 'se_module.fc2.bias'] = ((C,), 'conv_b')
            if b == 0:
                spec[q + 'downsample.0.weight'] = ((C, inpl, 1, 1), 'conv_w')
                OS._bn(spec, q + 'downsample.1.', C)
            inpl = C
    if with_last_linear:
        spec[p + 'last_linear.weight'] = ((1000, 2048), 'lin_w')
        spec[p + 'last_linear.bias'] = ((1000,), 'lin_b')


def spec_unet_seresnext(depth=50, num_classes=2, use_hypercolumn=True, with_last_linear=False):
    """State-dict spec {key: (shape, kind)} under the canonical spellings, in the module tree's order: the encoder of this file, the
    rest (center, decoder, final block) exactly as tests/seresnet_oracle.py lays it out."""
    s = OrderedDict()
    _senext(s, ENC, depth, with_last_linear)
    for k, v in SO.spec_unet_seresnet(50, num_classes, use_hypercolumn).items():
        if not k.startswith(ENC):
            s[k] = v
    return s
