"""Comparator for the depth-conditioned network (TEST INFRASTRUCTURE ONLY): architectures/models_with_depth.py:56-76 composed from the
oracle's blocks plus the depth gate (architectures/base.py:120-131) in plain torch."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import blocks as B
from oracle import specs as OS


def depth_gate(sd, d, p='depth_channel_excitation.'):
    """sigmoid(nn.Linear(1, C)(d)) -> [B, C]"""
    return torch.sigmoid(F.linear(d, sd[p + 'fc.0.weight'], sd[p + 'fc.0.bias']))


def unet_resnet_with_depth(sd, x, d, train, depth=34, use_hypercolumn=True, p=''):
    e = p + 'encoders.encoder.'
    c1 = B.resnet_stem(sd, e, x, train, False)
    e2 = B.resnet_layer(sd, e, c1, train, depth, 1)
    e3 = B.resnet_layer(sd, e, e2, train, depth, 2)
    e4 = B.resnet_layer(sd, e, e3, train, depth, 3)
    e5 = B.resnet_layer(sd, e, e4, train, depth, 4)
    c = B.conv2d_bn_relu(sd, p + 'center.0.', e5, train)
    c = B.conv2d_bn_relu(sd, p + 'center.1.', c, train)
    c = B._st(F.avg_pool2d(c, 2, 2))
    d5 = B.decoder_block(sd, p + 'dec5.', c, e5, train)
    d4 = B.decoder_block(sd, p + 'dec4.', d5, e4, train)
    d3 = B.decoder_block(sd, p + 'dec3.', d4, e3, train)
    d2 = B.decoder_block(sd, p + 'dec2.', d3, e2, train)
    d1 = B.decoder_block(sd, p + 'dec1.', d2, None, train)
    if use_hypercolumn:
        d1 = torch.cat([d1, B.upsample_bilinear(d2, 2), B.upsample_bilinear(d3, 4),
                        B.upsample_bilinear(d4, 8), B.upsample_bilinear(d5, 16)], 1)
    s = depth_gate(sd, d, p + 'depth_channel_excitation.')
    y = B.conv2d_bn_relu(sd, p + 'final.0.', d1 * s[:, :, None, None], train)
    return F.conv2d(y, sd[p + 'final.1.weight'], sd[p + 'final.1.bias'])


def spec_unet_resnet_with_depth(depth=34, num_classes=2, use_hypercolumn=True, with_fc=False):
    """State-dict spec {key: (shape, kind)}: UNetResNet's, then the two gate parameters (the position the reference registers them in)."""
    s = OrderedDict(OS.spec_unet_resnet(depth=depth, num_classes=num_classes, use_hypercolumn=use_hypercolumn, with_fc=with_fc))
    bottom = 512 if depth in (18, 34) else 2048
    C = (5 if use_hypercolumn else 1) * bottom // 8
    s['depth_channel_excitation.fc.0.weight'] = ((C, 1), 'fc_w')
    s['depth_channel_excitation.fc.0.bias'] = ((C,), 'fc_b')
    return s
