"""Comparator for UNetSeResNet (TEST INFRASTRUCTURE ONLY): architectures/unet.py:112-172 on the SE-ResNet encoders of
architectures/encoders.py:48-83, composed from the oracle's blocks (stem, decoder, final block) plus the SE bottleneck in plain torch.
The encoder layout (pretrainedmodels senet.py: SENet / SEResNetBottleneck / SEModule as se_resnet50 / 101 / 152 build them) is
RESTATED from the package's public source, not executed: tests/golden/make_golden_seresnet.py holds the same restatement as the stub
the reference's own unet.py ran on, and the F17 fixtures pin the two to each other."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import helpers
from oracle import blocks as B
from oracle import specs as OS

COUNTS = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3], 152: [3, 8, 36, 3]}
ENC = 'encoders.encoder.'
# {alias prefix: canonical prefix}: SeResNetEncoders registers the stem and the layers a second time (encoders.py:61-74)
ALIASES = OrderedDict([('encoders.conv1.0.', ENC + 'layer0.conv1.'), ('encoders.conv1.1.', ENC + 'layer0.bn1.'),
                       ('encoders.encoder2.', ENC + 'layer1.'), ('encoders.encoder3.', ENC + 'layer2.'),
                       ('encoders.encoder4.', ENC + 'layer3.'), ('encoders.encoder5.', ENC + 'layer4.')])


def se_gate(sd, p, z):
    """SEModule's gate [B,C,1,1]: sigmoid(fc2(relu(fc1(avg_pool(z))))); pooled vector, FC and gate stay fp32 on the HIP path"""
    s = z.mean(dim=(2, 3), keepdim=True)
    s = F.relu(F.conv2d(s, sd[p + 'fc1.weight'], sd[p + 'fc1.bias']))
    return torch.sigmoid(F.conv2d(s, sd[p + 'fc2.weight'], sd[p + 'fc2.bias']))


def se_bottleneck(sd, p, x, train, stride, gates=None):
    """SEResNetBottleneck: the 1x1 conv1 carries the stride; out = relu(bn3(conv3) * gate + shortcut)"""
    y = B._st(F.relu(B.batch_norm(sd, p + 'bn1.', B._st(F.conv2d(x, B._w(sd[p + 'conv1.weight']), None, stride=stride)), train)))
    y = B._st(F.relu(B.batch_norm(sd, p + 'bn2.', B._st(F.conv2d(y, B._w(sd[p + 'conv2.weight']), None, padding=1)), train)))
    z = B.batch_norm(sd, p + 'bn3.', B._st(F.conv2d(y, B._w(sd[p + 'conv3.weight']))), train)
    if (p + 'downsample.0.weight') in sd:
        x = B._st(F.conv2d(x, B._w(sd[p + 'downsample.0.weight']), None, stride=stride))
        x = B._st(B.batch_norm(sd, p + 'downsample.1.', x, train))
    g = se_gate(sd, p + 'se_module.', z)
    if gates is not None:
        gates.append(g.detach())
    return B._st(F.relu(z * g + x))


def se_layer(sd, p, x, train, depth, idx, gates=None):
    for b in range(COUNTS[depth][idx - 1]):
        x = se_bottleneck(sd, '%slayer%d.%d.' % (p, idx, b), x, train, 2 if (b == 0 and idx > 1) else 1, gates)
    return x


def unet_seresnet(sd, x, train, depth=50, use_hypercolumn=True, p='', gates=None):
    """``gates``: a list that receives one list of gate tensors per encoder stage."""
    e = p + ENC
    c1 = B.resnet_stem(sd, e + 'layer0.', x, train, False)
    es = []
    y = c1
    for i in (1, 2, 3, 4):
        stage = [] if gates is not None else None
        y = se_layer(sd, e, y, train, depth, i, stage)
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


def _senet(spec, p, depth, with_last_linear):
    spec[p + 'layer0.conv1.weight'] = ((64, 3, 7, 7), 'conv_w')
    OS._bn(spec, p + 'layer0.bn1.', 64)
    inpl = 64
    for li, (planes, n) in enumerate(zip([64, 128, 256, 512], COUNTS[depth]), start=1):
        for b in range(n):
            q = '%slayer%d.%d.' % (p, li, b)
            C = planes * 4
            spec[q + 'conv1.weight'] = ((planes, inpl, 1, 1), 'conv_w'); OS._bn(spec, q + 'bn1.', planes)
            spec[q + 'conv2.weight'] = ((planes, planes, 3, 3), 'conv_w'); OS._bn(spec, q + 'bn2.', planes)
            spec[q + 'conv3.weight'] = ((C, planes, 1, 1), 'conv_w'); OS._bn(spec, q + 'bn3.', C)
            spec[q + 'se_module.fc1.weight'] = ((C // 16, C, 1, 1), 'conv_w'); spec[q + 'se_module.fc1.bias'] = ((C // 16,), 'conv_b')
            spec[q + 'se_module.fc2.weight'] = ((C, C // 16, 1, 1), 'conv_w'); spec[q + 'se_module.fc2.bias'] = ((C,), 'conv_b')
            if b == 0:
                spec[q + 'downsample.0.weight'] = ((C, inpl, 1, 1), 'conv_w')
                OS._bn(spec, q + 'downsample.1.', C)
            inpl = C
    if with_last_linear:
        spec[p + 'last_linear.weight'] = ((1000, 2048), 'lin_w')
        spec[p + 'last_linear.bias'] = ((1000,), 'lin_b')


def spec_unet_seresnet(depth=50, num_classes=2, use_hypercolumn=True, with_last_linear=False):
    """State-dict spec {key: (shape, kind)} under the canonical spellings, in the module tree's order."""
    s = OrderedDict()
    _senet(s, ENC, depth, with_last_linear)
    b = 2048
    OS._conv2d_bn_relu(s, 'center.0.', b, b)
    OS._conv2d_bn_relu(s, 'center.1.', b, b // 2)
    OS._decoder_block(s, 'dec5.', b + b // 2, b, b // 8)
    OS._decoder_block(s, 'dec4.', b // 2 + b // 8, b // 2, b // 8)
    OS._decoder_block(s, 'dec3.', b // 4 + b // 8, b // 4, b // 8)
    OS._decoder_block(s, 'dec2.', b // 8 + b // 8, b // 8, b // 8)
    OS._decoder_block(s, 'dec1.', b // 8, b // 16, b // 8)
    OS._conv2d_bn_relu(s, 'final.0.', (5 if use_hypercolumn else 1) * b // 8, b // 8)
    s['final.1.weight'] = ((num_classes, b // 8, 1, 1), 'conv_w')
    s['final.1.bias'] = ((num_classes,), 'conv_b')
    return s


def expand_aliases(sd):
    return helpers.expand_aliases(sd, ALIASES)


FC2_KEY = 'se_module.fc2.weight'


def closed_form_state(spec, fc2_scale=1.0):
    """The closed-form state of tests/golden/closed_form.py with every ``se_module.fc2.weight`` multiplied by ``fc2_scale`` (the F17
    generator scales the fill until the SE gates spread, and records the factor in the fixture)."""
    import closed_form as CF
    sd = CF.state_for((k, s) for k, (s, _) in spec.items())
    for k in sd:
        if k.endswith(FC2_KEY):
            sd[k] = sd[k] * fc2_scale
    return sd


def block_fixture(golden, name):
    """A bottleneck fixture with the gradients of its companion files (tests/golden/make_golden_seresnet.py: a committed file stays under
    1 MiB) merged in; ``golden`` = helpers.golden."""
    fx = golden(name)
    for i in range(int(fx.get('companions', 0))):
        fx.update(golden('%s_g%d' % (name, i + 1)))
    return fx
