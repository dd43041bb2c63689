"""Comparator for the emptiness classifier (TEST INFRASTRUCTURE ONLY): architectures/misc.py:39-81 composed from the oracle's ResNet
blocks plus the AvgPool2d(8) + 1x1 convolution head in plain torch."""
from collections import OrderedDict

import torch.nn.functional as F

import helpers
from oracle import blocks as B
from oracle import specs as OS

# {alias prefix: canonical prefix}: the reference registers the encoder's stem and layers a second time (misc.py:61-68)
ALIASES = OrderedDict([('conv1.0.', 'encoder.conv1.'), ('conv1.1.', 'encoder.bn1.'), ('encoder2.', 'encoder.layer1.'),
                       ('encoder3.', 'encoder.layer2.'), ('encoder4.', 'encoder.layer3.'), ('encoder5.', 'encoder.layer4.')])


def pool_head(x, weight, bias, k=8):
    """nn.Sequential(nn.AvgPool2d(k), nn.Conv2d(C, K, 1)): the pooled vector and the weight stay fp32 on the HIP path (no storage
    rounding between the two)."""
    return F.conv2d(F.avg_pool2d(x, k), weight, bias)


def emptiness_classifier(sd, x, train, depth=18, p=''):
    e = p + 'encoder.'
    y = B.resnet_stem(sd, e, x, train, False)
    for i in (1, 2, 3, 4):
        y = B.resnet_layer(sd, e, y, train, depth, i)
    return pool_head(y, sd[p + 'classifier.1.weight'], sd[p + 'classifier.1.bias'])


def spec_emptiness_classifier(depth=18, num_classes=2, with_fc=False):
    """State-dict spec {key: (shape, kind)} under the canonical spellings (``expand_aliases`` adds the reference's second names)."""
    s = OrderedDict()
    bottom = OS._resnet(s, 'encoder.', depth, with_fc=with_fc)
    s['classifier.1.weight'] = ((num_classes, bottom, 1, 1), 'conv_w')
    s['classifier.1.bias'] = ((num_classes,), 'conv_b')
    return s


def expand_aliases(sd):
    return helpers.expand_aliases(sd, ALIASES)
