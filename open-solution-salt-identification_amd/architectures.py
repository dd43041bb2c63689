"""Host-side mirror of the reference's network classes for the U-Net hot path.

Each class keeps the reference's constructor signature, attribute names and therefore ``state_dict()``
keys/shapes (checked against the reference's own key lists in tests/), but instead of a torch
``forward`` it has ``emit(graph, ...)``, which appends hand-written HIP operators to a static program
(engine.py).  The torch ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.Linear`` objects inside are used ONLY
as parameter containers (names, shapes, default initialisation); their ``forward`` is never called.

Reference classes mirrored (paths relative to the reference's common_blocks/):
  unet_models.py:21-30 ConvBnRelu · :38-50 DecoderBlockV1 · :53-75 DecoderBlockV2 · :78-151 UNetResNet
  (-> TernausUNetResNet here, exported under its reference name in unet_models.py) · :154-189 SaltUNet ·
  :192-233 SaltLinkNet
  architectures/base.py:7-37 Conv2dBnRelu · :40-57 DeconvConv2dBnRelu · :65-86 DecoderBlock ·
  :89-104 ChannelSELayer · :107-117 SpatialSELayer
  architectures/encoders.py:6-45 ResNetEncoders;  architectures/unet.py:22-109 UNetResNet
  architectures/misc.py:39-81 EmptinessClassifier
  architectures/encoders.py:48-83 SeResNetEncoders;  architectures/unet.py:112-172 UNetSeResNet
  pretrainedmodels senet.py (un-vendored dependency, layout RESTATED from its public source, not executed): SENet / SEResNetBottleneck /
  SEModule as se_resnet50 / 101 / 152 build them; SEResNeXtBottleneck as se_resnext50_32x4d / se_resnext101_32x4d build it
  architectures/encoders.py:86-118 SeResNetXtEncoders;  architectures/unet.py:175-235 UNetSeResNetXt
  torchvision 0.2.0 models/resnet.py (un-vendored dependency): ResNet / BasicBlock / Bottleneck layout
  torchvision / pretrainedmodels densenet.py (un-vendored dependency, layout RESTATED from the public source, not executed): DenseNet /
  _DenseBlock / _DenseLayer / _Transition as densenet121 / 169 / 201 build them
  architectures/encoders.py:121-164 DenseNetEncoders;  architectures/unet.py:238-307 UNetDenseNet
  architectures/pspnet.py:9-28 PSPModule · :31-42 PSPUpsample · :45-105 PSPNet
  architectures/base.py:152-178 GlobalConvolutionalNetwork · :181-197 BoundaryRefinement;  architectures/large_kernel_matters.py:8-98 LargeKernelMatters
"""
import math

import torch
from torch import nn

from . import switches
from ._abi import SaltError
from .runtime import Engine


class EmitOnly(nn.Module):
    """Sub-modules are parameter containers + emitters; only whole networks are callable."""

    def forward(self, *a, **k):
        raise SaltError('%s is executed as part of a compiled network (HIP program); call the enclosing network'
                        % type(self).__name__)


# ----------------------------------------------------------------------------- TernausNet-style blocks
class ConvBnRelu(EmitOnly):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_channels, out_channels, 3, padding=1), nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))

    def emit(self, g, x, out=None):
        return g.conv(x, self.conv[0], self.conv[1], relu=True, out=out, name='ConvBnRelu')


class DecoderBlockV1(EmitOnly):
    def __init__(self, in_channels, middle_channels, out_channels):
        super().__init__()
        self.block = nn.Sequential(ConvBnRelu(in_channels, middle_channels),
                                   nn.ConvTranspose2d(middle_channels, out_channels, kernel_size=3, stride=2, padding=1, output_padding=1),
                                   nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))

    def emit(self, g, x, out=None):
        return g.conv_transpose(self.block[0].emit(g, x), self.block[1], self.block[2], relu=True, out=out, name='DecoderBlockV1')


class DecoderBlockV2(EmitOnly):
    def __init__(self, in_channels, middle_channels, out_channels, is_deconv=True):
        super().__init__()
        self.is_deconv = is_deconv
        self.deconv = nn.Sequential(ConvBnRelu(in_channels, middle_channels),
                                    nn.ConvTranspose2d(middle_channels, out_channels, kernel_size=4, stride=2, padding=1),
                                    nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))
        self.upsample = nn.Sequential(ConvBnRelu(in_channels, out_channels), nn.Upsample(scale_factor=2, mode='bilinear'))

    def emit(self, g, x, out=None):
        if self.is_deconv:
            return g.conv_transpose(self.deconv[0].emit(g, x), self.deconv[1], self.deconv[2], relu=True, out=out, name='DecoderBlockV2')
        return g.upsample(self.upsample[0].emit(g, x), 2, out=out, name='DecoderBlockV2.up')

    def dead_prefix(self):
        return 'upsample.' if self.is_deconv else 'deconv.'


# ----------------------------------------------------------------------------- architectures/base.py blocks
class Conv2dBnRelu(EmitOnly):
    def __init__(self, in_channels, out_channels, kernel_size=(3, 3), use_relu=True, use_batch_norm=True, use_padding=True,
                 padding_method='replication'):
        super().__init__()
        if padding_method != 'replication' or not use_padding:
            raise NotImplementedError('only the replication-padded variant is on the U-Net hot path')
        self.use_relu, self.use_batch_norm, self.use_padding = use_relu, use_batch_norm, use_padding
        self.batch_norm = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.padding = nn.ReplicationPad2d(padding=(0, kernel_size[1] - 1, kernel_size[0] - 1, 0))
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=0)

    def emit(self, g, x, out=None):
        return g.conv(x, self.conv, self.batch_norm if self.use_batch_norm else None, relu=self.use_relu, out=out, replicate=True, name='Conv2dBnRelu')


class DeconvConv2dBnRelu(EmitOnly):
    def __init__(self, in_channels, out_channels, use_relu=True, use_batch_norm=True):
        super().__init__()
        self.use_relu, self.use_batch_norm = use_relu, use_batch_norm
        self.batch_norm = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.deconv = nn.ConvTranspose2d(in_channels, out_channels, kernel_size=3, stride=2, padding=1, output_padding=1)

    def emit(self, g, x, out=None):
        return g.conv_transpose(x, self.deconv, self.batch_norm if self.use_batch_norm else None, relu=self.use_relu, out=out, name='DeconvConv2dBnRelu')


class ChannelSELayer(EmitOnly):
    def __init__(self, channel, reduction=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction), nn.ReLU(inplace=True),
                                nn.Linear(channel // reduction, channel), nn.Sigmoid())


class SpatialSELayer(EmitOnly):
    def __init__(self, channels):
        super().__init__()
        self.fc = nn.Conv2d(channels, 1, kernel_size=1)
        self.sigmoid = nn.Sigmoid()


class DecoderBlock(EmitOnly):
    def __init__(self, in_channels, middle_channels, out_channels):
        super().__init__()
        self.conv1 = Conv2dBnRelu(in_channels, middle_channels)
        self.conv2 = Conv2dBnRelu(middle_channels, out_channels)
        self.upsample = nn.Upsample(scale_factor=2, mode='bilinear')
        self.relu = nn.ReLU(inplace=True)
        self.channel_se = ChannelSELayer(out_channels, reduction=16)
        self.spatial_se = SpatialSELayer(out_channels)

    def emit(self, g, x, e=None, cat=None, out=None):
        """``cat``: optional pre-allocated [up(x) | e] buffer whose tail slice IS ``e`` (concat-free skip)."""
        if e is None:
            xin = g.upsample(x, 2, name='DecoderBlock.up')
        else:
            if cat is None:
                cat = g.new_act(x.B, 2 * x.H, 2 * x.W, x.C + e.C, 'DecoderBlock.cat')
                g.copy(e, cat.slice(x.C, e.C))
            else:
                assert e.buf is cat.buf and e.c0 == cat.c0 + x.C and cat.C == x.C + e.C
            g.upsample(x, 2, out=cat.slice(0, x.C))
            xin = cat
        y = self.conv2.emit(g, self.conv1.emit(g, xin))
        return g.scse(y, self.channel_se, self.spatial_se, out=out, name='DecoderBlock.scse')


# ----------------------------------------------------------------------------- torchvision-layout ResNet (parameter layout only)
class BasicBlock(EmitOnly):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def emit(self, g, x, out=None):
        idt = x
        if self.downsample is not None:          # the projection shortcut is independent of conv1 -> conv2: side stream, joined at the add
            with g.side():
                idt = g.conv(x, self.downsample[0], self.downsample[1], relu=False, name='down')
        n0 = len(g.tape)
        a = g.conv(x, self.conv1, self.bn1, relu=True, name='block.conv1')
        y = g.conv(a, self.conv2, self.bn2, relu=True, res=idt, out=out, name='block.conv2')
        _shortcut_gradient_first(g, n0, self.downsample)
        return y


def _shortcut_gradient_first(g, n0, downsample):
    """Backward order inside a residual block with a projection shortcut (torchvision layout through architectures/encoders.py:38-45):
    the tape runs in reverse, so by default the shortcut's closure - emitted first - runs LAST and its stride-2 1x1 data gradient
    (every other pixel of the block input) is the last writer of dL/dx.  Moving it in front of the main branch's first convolution
    makes that convolution's data gradient - a full-coverage launch - the last writer, which can then carry the BatchNorm-backward
    sums of x's producer (Graph._bn_train_bwd) and saves that layer's reduction pass.  ``n0`` = tape length BEFORE the main branch was
    emitted; the shortcut's closure sits at n0 - 1."""
    if downsample is None or not g.train or switches.get('SALT_NO_SHORTCUT_FIRST') or n0 < 1 or len(g.tape) < n0 + 2:
        return
    g.tape.insert(n0, g.tape.pop(n0 - 1))        # [.., down, conv1, ..] -> [.., conv1, down, ..]: backward runs .., down, conv1


class Bottleneck(EmitOnly):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def emit(self, g, x, out=None):
        idt = x
        if self.downsample is not None:
            with g.side():
                idt = g.conv(x, self.downsample[0], self.downsample[1], relu=False, name='down')
        n0 = len(g.tape)
        a = g.conv(x, self.conv1, self.bn1, relu=True, name='bneck.conv1')
        a = g.conv(a, self.conv2, self.bn2, relu=True, name='bneck.conv2')
        y = g.conv(a, self.conv3, self.bn3, relu=True, res=idt, out=out, name='bneck.conv3')
        _shortcut_gradient_first(g, n0, self.downsample)
        return y


class ResNet(EmitOnly):
    CFG = {18: (BasicBlock, [2, 2, 2, 2]), 34: (BasicBlock, [3, 4, 6, 3]), 50: (Bottleneck, [3, 4, 6, 3]),
           101: (Bottleneck, [3, 4, 23, 3]), 152: (Bottleneck, [3, 8, 36, 3])}

    def __init__(self, depth, in_channels=3):
        super().__init__()
        block, counts = self.CFG[depth]
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make(block, 64, counts[0], 1)
        self.layer2 = self._make(block, 128, counts[1], 2)
        self.layer3 = self._make(block, 256, counts[2], 2)
        self.layer4 = self._make(block, 512, counts[3], 2)
        self.avgpool = nn.AvgPool2d(7, stride=1)
        self.fc = nn.Linear(512 * block.expansion, 1000)        # present in the reference state_dict, never used
        for m in self.modules():                                 # torchvision 0.2.0 initialisation
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make(self, block, planes, n, stride):
        down = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                                 nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, down)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, n)]
        return nn.Sequential(*layers)


def emit_blocks(g, blocks, x, out=None):
    blocks = list(blocks)
    for i, b in enumerate(blocks):
        x = b.emit(g, x, out=out if i == len(blocks) - 1 else None)
    return x


def resnet(depth, pretrained=False):
    if pretrained:
        raise SaltError('pretrained ImageNet weights need a download; load a state_dict instead')
    return ResNet(depth)


class ResNetEncoders(EmitOnly):
    def __init__(self, encoder_depth, pretrained=False, pool0=False):
        super().__init__()
        if encoder_depth not in ResNet.CFG:
            raise NotImplementedError('only 18, 34, 50, 101, 152 version of Resnet are implemented')
        # pool0: the stem is followed by torchvision's MaxPool2d(3, 2, 1) (encoders.py:23-27).  The reference's decoder has no
        # compensating up-sampling, so the logits then come out at HALF the input resolution (unet.py:89-109); the registry never
        # sets it (models.py:15-19) - reproduced as is
        self.pool0 = pool0
        self.encoder = resnet(encoder_depth, pretrained)
        if pool0:
            self.conv1 = nn.Sequential(self.encoder.conv1, self.encoder.bn1, self.encoder.relu, self.encoder.maxpool)
        else:
            self.conv1 = nn.Sequential(self.encoder.conv1, self.encoder.bn1, self.encoder.relu)
        self.encoder2 = self.encoder.layer1
        self.encoder3 = self.encoder.layer2
        self.encoder4 = self.encoder.layer3
        self.encoder5 = self.encoder.layer4


# ----------------------------------------------------------------------------- pretrainedmodels-layout SE-ResNet (parameter layout only)
class SEModule(EmitOnly):
    """senet.py SEModule: x * sigmoid(fc2(relu(fc1(avg_pool(x))))), fc1 / fc2 1x1 convolutions with bias."""

    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, channels // reduction, kernel_size=1, padding=0)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(channels // reduction, channels, kernel_size=1, padding=0)
        self.sigmoid = nn.Sigmoid()


class SEResNetBottleneck(EmitOnly):
    """senet.py SEResNetBottleneck: the Caffe-style bottleneck - the 1x1 conv1 carries the stride - with an SEModule on bn3's output
    before the shortcut add.  conv3 -> bn3 is emitted without ReLU and Graph.se_res (csrc/se_res.hip) is its only reader."""
    expansion = 4

    def __init__(self, inplanes, planes, groups, reduction, stride=1, downsample=None):
        super().__init__()
        if groups != 1:
            raise SaltError('SEResNetBottleneck: grouped convolutions (SE-ResNeXt) are not built')
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

    def emit(self, g, x, out=None):
        idt = x
        if self.downsample is not None:          # the projection shortcut stays on the side stream, joined at the SE tail
            with g.side():
                idt = g.conv(x, self.downsample[0], self.downsample[1], relu=False, name='down')
        n0 = len(g.tape)
        a = g.conv(x, self.conv1, self.bn1, relu=True, name='sebneck.conv1')
        a = g.conv(a, self.conv2, self.bn2, relu=True, name='sebneck.conv2')
        z = g.conv(a, self.conv3, self.bn3, relu=False, name='sebneck.conv3')
        y = g.se_res(z, self.bn3, self.se_module, idt, out=out, name='sebneck.se')
        _shortcut_gradient_first(g, n0, self.downsample)
        return y


class SEResNeXtBottleneck(EmitOnly):
    """senet.py SEResNeXtBottleneck: the ResNeXt type-C bottleneck with an SEModule - conv1 is a plain 1x1, the grouped 3x3 conv2
    carries the stride.  conv2 -> bn2 runs on Graph.gconv (csrc/conv_group.hip); everything else is SEResNetBottleneck.emit."""
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

    def emit(self, g, x, out=None):
        idt = x
        if self.downsample is not None:          # the projection shortcut stays on the side stream, joined at the SE tail
            with g.side():
                idt = g.conv(x, self.downsample[0], self.downsample[1], relu=False, name='down')
        n0 = len(g.tape)
        a = g.conv(x, self.conv1, self.bn1, relu=True, name='sxbneck.conv1')
        a = g.gconv(a, self.conv2, self.bn2, relu=True, name='sxbneck.conv2')
        z = g.conv(a, self.conv3, self.bn3, relu=False, name='sxbneck.conv3')
        y = g.se_res(z, self.bn3, self.se_module, idt, out=out, name='sxbneck.se')
        _shortcut_gradient_first(g, n0, self.downsample)
        return y


class SENet(EmitOnly):
    """senet.py SENet as se_resnet50 / 101 / 152 (SEResNetBottleneck, groups 1) and se_resnext50_32x4d / se_resnext101_32x4d
    (``block`` = SEResNeXtBottleneck, groups 32) configure it - reduction 16, inplanes 64, input_3x3 False, 1x1 downsample without
    padding, no dropout: layer0 = Sequential(conv1 7x7 s2 p3, bn1, relu1, pool), layer1 .. layer4, avg_pool, last_linear."""
    CFG = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3], 152: [3, 8, 36, 3]}

    def __init__(self, depth, num_classes=1000, block=SEResNetBottleneck, groups=1):
        super().__init__()
        from collections import OrderedDict
        counts = self.CFG[depth]
        self.block, self.groups = block, groups
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
        self.last_linear = nn.Linear(512 * block.expansion, num_classes)      # present in the state_dict, never used

    def _make(self, planes, n, stride):
        exp = self.block.expansion
        down = None
        if stride != 1 or self.inplanes != planes * exp:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes * exp, kernel_size=1, stride=stride, padding=0, bias=False),
                                 nn.BatchNorm2d(planes * exp))
        layers = [self.block(self.inplanes, planes, self.groups, 16, stride, down)]
        self.inplanes = planes * exp
        layers += [self.block(self.inplanes, planes, self.groups, 16) for _ in range(1, n)]
        return nn.Sequential(*layers)


class SeResNetEncoders(EmitOnly):
    def __init__(self, encoder_depth, pretrained=False, pool0=False):
        super().__init__()
        if encoder_depth not in SENet.CFG:
            raise NotImplementedError('only 50, 101, 152 version of Resnet are implemented')
        if pretrained:
            raise SaltError('pretrained ImageNet weights need a download; load a state_dict instead')
        if pool0:
            # encoders.py:61-65 reads layer0.pool0 for it; the ceil_mode pool changes every map size downstream - out of scope
            raise SaltError('SeResNetEncoders: pool0=True is not built')
        self.pool0 = False
        self.encoder = SENet(encoder_depth)
        self.conv1 = nn.Sequential(self.encoder.layer0.conv1, self.encoder.layer0.bn1, self.encoder.layer0.relu1)
        self.encoder2 = self.encoder.layer1
        self.encoder3 = self.encoder.layer2
        self.encoder4 = self.encoder.layer3
        self.encoder5 = self.encoder.layer4


class SeResNetXtEncoders(EmitOnly):
    def __init__(self, encoder_depth, pretrained=False, pool0=False):
        super().__init__()
        if encoder_depth not in (50, 101):
            raise NotImplementedError('only 50, 101 version of Resnet are implemented')
        if pretrained:
            raise SaltError('pretrained ImageNet weights need a download; load a state_dict instead')
        if pool0:
            # encoders.py:97-101 reads layer0.pool0 for it, as SeResNetEncoders does - out of scope in the same way
            raise SaltError('SeResNetXtEncoders: pool0=True is not built')
        self.pool0 = False
        self.encoder = SENet(encoder_depth, block=SEResNeXtBottleneck, groups=32)
        self.conv1 = nn.Sequential(self.encoder.layer0.conv1, self.encoder.layer0.bn1, self.encoder.layer0.relu1)
        self.encoder2 = self.encoder.layer1
        self.encoder3 = self.encoder.layer2
        self.encoder4 = self.encoder.layer3
        self.encoder5 = self.encoder.layer4



# ----------------------------------------------------------------------------- DenseNet (public torchvision / pretrainedmodels layout, restated)
class _DenseLayer(EmitOnly):
    """norm1 -> relu1 -> conv1 (1x1, bn_size * growth) -> norm2 -> relu2 -> conv2 (3x3, growth); the output is concatenated behind the
    input.  Module names are the modern ones (torchvision 0.2.0 registered 'norm.1' ...; UNetDenseNet.load_state_dict translates)."""

    def __init__(self, num_input_features, growth_rate, bn_size, drop_rate):
        super().__init__()
        if drop_rate:
            raise SaltError('_DenseLayer: drop_rate > 0 is not built')
        self.norm1 = nn.BatchNorm2d(num_input_features)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = nn.Conv2d(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth_rate)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False)
        self.growth_rate = growth_rate

    def emit(self, g, block, c, table):
        """``block``: the concatenation buffer; reads its prefix [0, c), writes the slice [c, c + growth) - no copy.  conv2's launch
        also reports the statistics of its 32 raw channels, which every later norm1 of the block shares (``table``)."""
        a = g.dense_conv(block.slice(0, c), self.norm1, self.conv1, self.norm2, relu=True, table=table, name='denselayer.conv1')
        fill = (lambda st, cnt, n: g.dense_table_fill(table, c, self.growth_rate, st, cnt, n)) if g.train else None
        return g.conv(a, self.conv2, None, relu=False, out=block.slice(c, self.growth_rate), name='denselayer.conv2', raw_stats=fill)


class _DenseBlock(nn.Sequential):
    def __init__(self, num_layers, num_input_features, bn_size, growth_rate, drop_rate):
        super().__init__()
        for i in range(num_layers):
            self.add_module('denselayer%d' % (i + 1), _DenseLayer(num_input_features + i * growth_rate, growth_rate, bn_size, drop_rate))

    def forward(self, *a, **k):
        return EmitOnly.forward(self, *a, **k)


class _Transition(EmitOnly):
    def __init__(self, num_input_features, num_output_features):
        super().__init__()
        self.norm = nn.BatchNorm2d(num_input_features)
        self.relu = nn.ReLU(inplace=True)
        self.conv = nn.Conv2d(num_input_features, num_output_features, kernel_size=1, stride=1, bias=False)
        self.pool = nn.AvgPool2d(kernel_size=2, stride=2)

    def emit(self, g, block, table, out):
        return g.avgpool2(g.dense_conv(block, self.norm, self.conv, None, relu=False, table=table, name='transition.conv'), out=out, name='transition.pool')


class DenseNet(EmitOnly):
    """densenet121 / 169 / 201: growth 32, bn_size 4, 64 initial features, bias-free convolutions, BatchNorm eps 1e-5, AvgPool2d(2, 2) in
    the transitions, drop rate 0.  features = conv0, norm0, relu0, pool0, denseblock1, transition1, ..., denseblock4, norm5; the
    classifier is pretrainedmodels' ``last_linear``.  norm5 and last_linear are in the state_dict and never used by the U-Net."""
    CFG = {121: (6, 12, 24, 16), 169: (6, 12, 32, 32), 201: (6, 12, 48, 32)}
    GROWTH, BN_SIZE, INIT = 32, 4, 64

    def __init__(self, depth, num_classes=1000):
        super().__init__()
        from collections import OrderedDict
        cfg = self.CFG[depth]
        self.features = nn.Sequential(OrderedDict([('conv0', nn.Conv2d(3, self.INIT, kernel_size=7, stride=2, padding=3, bias=False)),
                                                   ('norm0', nn.BatchNorm2d(self.INIT)), ('relu0', nn.ReLU(inplace=True)),
                                                   ('pool0', nn.MaxPool2d(kernel_size=3, stride=2, padding=1))]))
        n = self.INIT
        self.widths = []
        for i, layers in enumerate(cfg):
            self.features.add_module('denseblock%d' % (i + 1), _DenseBlock(layers, n, self.BN_SIZE, self.GROWTH, 0))
            n += layers * self.GROWTH
            self.widths.append(n)
            if i != len(cfg) - 1:
                self.features.add_module('transition%d' % (i + 1), _Transition(n, n // 2))
                n //= 2
        self.features.add_module('norm5', nn.BatchNorm2d(n))
        self.last_linear = nn.Linear(n, num_classes)


class DenseNetEncoders(EmitOnly):
    BUILT = (121,)

    def __init__(self, encoder_depth, pretrained=False, pool0=False):
        super().__init__()
        if encoder_depth == 161:
            raise NotImplementedError('DenseNetEncoders: depth 161 (growth 48, 96 initial features) is not built; 121 is')
        if encoder_depth in DenseNet.CFG and encoder_depth not in self.BUILT:
            # the encoders themselves share every shape class with 121; the U-Net's decoder is enc[3] // 8 = 208 / 240 channels wide, and
            # the first layer that refuses that is dec5's scSE block: salt_scse takes power-of-two widths only (csrc/se.hip)
            d = {169: 208, 201: 240}[encoder_depth]
            raise NotImplementedError('DenseNetEncoders: depth %d is not built: the decoder is %d channels wide and dec5.channel_se / spatial_se '
                                      '(salt_scse) refuses it: C=%d must be a power of two' % (encoder_depth, d, d))
        if encoder_depth not in DenseNet.CFG:
            raise NotImplementedError('only 121, 161, 169, 201 version of Densenet are implemented')
        if pretrained:
            raise SaltError('pretrained ImageNet weights need a download; load a state_dict instead')
        if pool0:
            raise SaltError('DenseNetEncoders: pool0=True is not built')
        self.pool0 = False
        self.encoder = DenseNet(encoder_depth)
        f = self.encoder.features
        self.conv1 = nn.Sequential(f.conv0, f.norm0, f.relu0)
        self.encoder2 = f.denseblock1
        self.transition1 = f.transition1
        self.encoder3 = f.denseblock2
        self.transition2 = f.transition2
        self.encoder4 = f.denseblock3
        self.transition3 = f.transition3
        self.encoder5 = f.denseblock4


# ----------------------------------------------------------------------------- whole networks
class HipNetwork(nn.Module):
    """Base of the callable networks: owns the Engine, dispatches forward to the compiled HIP program."""

    compute_dtype = switches.get('SALT_DTYPE')
    # nn.Upsample / F.upsample(mode='bilinear') (base.py:70, unet.py:103-106).  False: torch >= 0.4 semantics, what the oracle and the
    # goldens executed (torch 2.10).  True: how torch 0.3.1 - the version the reference pins, environment.yml:17 - evaluated the very
    # same calls; a checkpoint TRAINED in the reference's environment saw these features, so evaluate / fine-tune it with True
    align_corners = False

    def __init__(self):
        super().__init__()
        self._engine = None

    # -- engine management -------------------------------------------------------------------------
    def engine(self, device=None):
        if self._engine is None:
            if device is None:
                device = next(self.parameters()).device
            self._engine = Engine(self, torch.device(device), self.compute_dtype)
        return self._engine

    def set_compute_dtype(self, dtype):
        if dtype != self.compute_dtype:
            self.compute_dtype = dtype
            self._drop_engine()
        return self

    def set_align_corners(self, flag):
        flag = bool(flag)
        if flag != self.align_corners:
            self.align_corners = flag
            self._drop_engine()
        return self

    def _drop_engine(self):
        if self._engine is not None:
            self._engine.release_step_graphs()
            for p in self.parameters():       # detach parameters from the flat buffers before they go away
                p.data = p.data.clone()
                p.grad = None
            self._engine = None

    def _apply(self, fn, *a, **k):
        self._drop_engine()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = {k: v for k, v in state_dict.items()}
        own = self.state_dict()
        for k in own:                          # torch 0.3.1 checkpoints have no num_batches_tracked
            if k.endswith('num_batches_tracked') and k not in sd:
                sd[k] = own[k]
        r = super().load_state_dict(sd, strict=strict, **kw)
        if self._engine is not None:
            self._engine.touch()
        return r

    def dead_parameter_names(self):
        return []

    # -- execution -----------------------------------------------------------------------------------
    uses_depth = False          # True: forward(x, d) with the tiles' depths d [B,1] (UNetResNetWithDepth)

    def _check_depth(self, x, d):
        if not self.uses_depth:
            if d is not None:
                raise SaltError('%s takes no depth input' % type(self).__name__)
            return None
        if not isinstance(d, torch.Tensor) or tuple(d.shape) != (x.shape[0], 1):
            raise SaltError('%s needs the depth input d of shape [%d, 1] (got %s)'
                            % (type(self).__name__, x.shape[0], 'none' if d is None else tuple(getattr(d, 'shape', ()))))
        return d.to(x.device).contiguous().float()

    def forward(self, x, d=None):
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise SaltError('expected a [B,C,H,W] tensor')
        if x.device.type != 'cuda':
            raise SaltError('%s runs only as hand-written HIP kernels on a GPU; got a %s tensor (no CPU/PyTorch fallback)'
                            % (type(self).__name__, x.device.type))
        eng = self.engine(x.device)
        x = x.contiguous().float()
        d = self._check_depth(x, d)
        if self.training and torch.is_grad_enabled():
            from .autograd import HipNetFunction
            return HipNetFunction.apply(self, x, d, *eng.live_params)
        net = eng.forward(x, self.training, d=d)
        return net.logits.clone()


class UNetResNet(HipNetwork):
    """architectures.unet.UNetResNet — the hypercolumn scSE U-Net that main.py trains (models.py:15-19)."""

    def __init__(self, encoder_depth, num_classes, dropout_2d=0.0, pretrained=False, use_hypercolumn=False, pool0=False):
        super().__init__()
        # F.dropout2d(encoder5, p=self.dropout_2d) (unet.py:91): the reference environment pins torch==0.3.1 (environment.yml:17), whose
        # F.dropout2d defaults to training=False - the call is an identity for every p there, and the registry passes p = 0 anyway
        self.num_classes, self.dropout_2d, self.use_hypercolumn = num_classes, dropout_2d, use_hypercolumn
        self.encoders, b = self._make_encoders(encoder_depth, pretrained, pool0)
        e = self._encoder_widths(b)
        self.center = nn.Sequential(Conv2dBnRelu(b, b), Conv2dBnRelu(b, e[2]), nn.AvgPool2d(kernel_size=2, stride=2))
        self.dec5 = DecoderBlock(b + e[2], b, b // 8)
        self.dec4 = DecoderBlock(e[2] + b // 8, b // 2, b // 8)
        self.dec3 = DecoderBlock(e[1] + b // 8, b // 4, b // 8)
        self.dec2 = DecoderBlock(e[0] + b // 8, b // 8, b // 8)
        self.dec1 = DecoderBlock(b // 8, b // 16, b // 8)
        self.final = nn.Sequential(Conv2dBnRelu((5 if use_hypercolumn else 1) * b // 8, b // 8),
                                   nn.Conv2d(b // 8, num_classes, kernel_size=1, padding=0))
        self.bottom = b

    def _make_encoders(self, encoder_depth, pretrained, pool0):
        """Hook: -> (the encoders module, bottom_channel_nr).  UNetSeResNet builds SeResNetEncoders here."""
        return ResNetEncoders(encoder_depth, pretrained=pretrained, pool0=pool0), 512 if encoder_depth in (18, 34) else 2048

    def _encoder_widths(self, b):
        """Hook: the channels of encoder2 .. encoder5 (the last one is the bottom width ``b``).  The ResNet families halve them level by
        level; UNetDenseNet returns the reference's encoder_channel_nr."""
        return [b // 8, b // 4, b // 2, b]

    def _emit_encoders(self, g, c1, slots):
        """Hook: emit encoder2 .. encoder5 behind the stem output ``c1``, each straight into its slot of the decoder's concatenation
        buffers."""
        enc = self.encoders.encoder
        e2 = emit_blocks(g, enc.layer1, c1, out=slots[0])
        e3 = emit_blocks(g, enc.layer2, e2, out=slots[1])
        e4 = emit_blocks(g, enc.layer3, e3, out=slots[2])
        e5 = emit_blocks(g, enc.layer4, e4, out=slots[3])
        return e2, e3, e4, e5

    def _stem(self):
        """Hook: the stem's (convolution, BatchNorm) inside ``self.encoders.encoder``."""
        return self.encoders.encoder.conv1, self.encoders.encoder.bn1

    def dead_parameter_names(self):
        return ['encoders.encoder.fc.weight', 'encoders.encoder.fc.bias']

    def output_shape(self, shape):
        B, _, H, W = shape
        s = 2 if self.encoders.pool0 else 1
        return (B, self.num_classes, H // s, W // s)

    def _hyper_in(self, g, x, c0, last=False):
        """Hook: ``x`` is about to enter the final block as channels [c0, c0 + x.C) of the (possibly factored) hypercolumn, at its own
        resolution.  ``last``: dec1, whose only consumer is the final block.  UNetResNetWithDepth gates here."""
        return x

    def emit(self, g, x_nchw, logits):
        B, _, H, W = x_nchw.shape
        b, d = self.bottom, self.bottom // 8
        ew = self._encoder_widths(b)
        c1 = g.conv_first(x_nchw, *self._stem(), relu=True, name='stem')
        if self.encoders.pool0:
            c1 = g.maxpool3s2(c1, name='stem.pool')
            H, W = H // 2, W // 2                    # everything downstream runs at half the resolution
        # concat-free skips: the encoder writes each feature map straight into the decoder's input buffer
        cat5 = g.new_act(B, H // 16, W // 16, ew[2] + b, 'cat5')                    # [up(center) | e5]
        cat4 = g.new_act(B, H // 8, W // 8, d + ew[2], 'cat4')                       # [up(dec5)   | e4]
        cat3 = g.new_act(B, H // 4, W // 4, d + ew[1], 'cat3')                       # [up(dec4)   | e3]
        cat2 = g.new_act(B, H // 2, W // 2, d + ew[0], 'cat2')                       # [up(dec3)   | e2]
        e2, e3, e4, e5 = self._emit_encoders(g, c1, [cat2.slice(d, ew[0]), cat3.slice(d, ew[1]), cat4.slice(d, ew[2]), cat5.slice(ew[2], b)])
        c = self.center[1].emit(g, self.center[0].emit(g, e5))
        c = g.avgpool2(c, name='center.pool')
        # FACTORED hypercolumn (round 5; DESIGN 4, saltnet.h salt_hyper_stencil): the levels up-sampled by R >= SALT_HYPER_FACTOR (default 4;
        # 0 = off) are never up-sampled, stored or convolved at full resolution.  A 1x1 contraction commutes with the bilinear
        # interpolation and the tap shift, so each such level enters the final convolution as z_k = [W_tap] dec_k - ONE 1x1 launch at the
        # level's own resolution - plus a separable stencil that adds sum_tap shift_tap(up(z_k[tap])) to the convolution over the
        # remaining full-resolution channels [dec1 | up2(dec2)]
        fmin = switches.get('SALT_HYPER_FACTOR')
        levels = [(16, 4), (8, 3), (4, 2), (2, 1)]          # (R, channel block of the hypercolumn)
        fact = [(R, k) for R, k in levels if fmin and R >= fmin] if self.use_hypercolumn else []
        if fact and not g.hyper_factor_ok(B, H, W, d, [R for R, _ in fact]):
            fact = []
        nfull = 5 - len(fact)                               # channel blocks that stay at full resolution (contiguous from block 0)
        if fact and sorted(k for _, k in fact) != list(range(nfull, 5)):
            raise SaltError('factored hypercolumn levels must be the deepest ones')
        zs = {}
        if self.use_hypercolumn:
            # PLANAR hypercolumn where the kernels allow it (bf16, conv_ls / conv_ws eligible): five dense [B,H,W,64] planes instead of
            # 320-channel rows.  Every producer (dec1's scSE, the four up-samplings) and every gradient consumer then streams ONE dense
            # tensor instead of 128-byte pieces at a 640-byte pitch (0.6 TB/s at the C4 size); the final convolution, its data gradient
            # and its weight gradient address the planes themselves (salt_conv_args.x_plane / y_plane, salt_conv_wgrad_args.q_plane)
            planes = d if (nfull > 1 and g.planar_ok(B, H, W, nfull * d, d, self.final[0].conv)) else 0
            hyper = g.new_act(B, H, W, nfull * d, 'hypercolumn', planes=planes)
        # the hypercolumn up-samplings only feed the final convolution: each one goes to the side stream as soon as its decoder
        # level exists and overlaps the remaining decoder levels; the final convolution joins
        def hyper_up(x, R, k):
            if (R, k) in fact:
                with g.side():
                    zs[k] = g.hyper_level(self._hyper_in(g, x, k * d), self.final[0].conv, k * d, name='hyper.z%d' % k)
            elif self.use_hypercolumn:
                with g.side():
                    g.upsample(self._hyper_in(g, x, k * d), R, out=hyper.slice(k * d, d))
        d5 = self.dec5.emit(g, c, e5, cat=cat5)
        hyper_up(d5, 16, 4)
        d4 = self.dec4.emit(g, d5, e4, cat=cat4)
        hyper_up(d4, 8, 3)
        d3 = self.dec3.emit(g, d4, e3, cat=cat3)
        hyper_up(d3, 4, 2)
        d2 = self.dec2.emit(g, d3, e2, cat=cat2)
        hyper_up(d2, 2, 1)
        if self.use_hypercolumn:
            d1 = self._hyper_in(g, self.dec1.emit(g, d2, None, out=hyper.slice(0, d)), 0, last=True)
            g.join()
            if fact:
                ks = sorted(zs)
                # eval: the 1x1 logit head is the block's only consumer - the stencil's epilogue applies it
                fuse_head = g.head_bn_ok(d, self.final[1]) if g.train else g.hyper_head_ok(d, self.final[1])
                f = g.conv_hyper(hyper, [zs[k] for k in ks], [dict((k_, R_) for R_, k_ in fact)[k] for k in ks], self.final[0].conv,
                                 self.final[0].batch_norm, relu=self.final[0].use_relu, head=(self.final[1], logits) if fuse_head else None)
                if fuse_head:
                    return
            else:
                f = self.final[0].emit(g, hyper)
        else:
            d1 = self._hyper_in(g, self.dec1.emit(g, d2, None), 0, last=True)
            f = self.final[0].emit(g, d1)
        g.head(f, self.final[1], logits)


class UNetSeResNet(UNetResNet):
    """architectures.unet.UNetSeResNet (unet.py:112-172): UNetResNet's decoder, hypercolumn and head (the two classes differ in the
    ``encoders`` line and nothing else) on SE-ResNet50 / 101 / 152 encoders with 2048 bottom channels."""

    def _make_encoders(self, encoder_depth, pretrained, pool0):
        return SeResNetEncoders(encoder_depth, pretrained=pretrained, pool0=pool0), 2048

    def _stem(self):
        return self.encoders.encoder.layer0.conv1, self.encoders.encoder.layer0.bn1

    def dead_parameter_names(self):
        return ['encoders.encoder.last_linear.weight', 'encoders.encoder.last_linear.bias']


class UNetSeResNetXt(UNetSeResNet):
    """architectures.unet.UNetSeResNetXt (unet.py:175-235): the same decoder, hypercolumn and head once more, on SE-ResNeXt50 / 101
    (32x4d) encoders - the grouped 3x3 of every bottleneck runs on csrc/conv_group.hip."""

    def _make_encoders(self, encoder_depth, pretrained, pool0):
        return SeResNetXtEncoders(encoder_depth, pretrained=pretrained, pool0=pool0), 2048


class UNetDenseNet(UNetResNet):
    """architectures.unet.UNetDenseNet (unet.py:238-307): UNetResNet's decoder, hypercolumn and head on DenseNet-121 encoders.  The
    decoder widths come from the four encoder widths [256, 512, 1024, 1024] (center[1] outputs enc[2], dec5 takes enc[3] + enc[2]).
    A dense block IS its slot of the decoder's concatenation buffer: layer l reads the prefix [0, C0 + 32 l) through Graph.dense_conv
    (csrc/dense.hip) and its conv2 writes the slice behind it; a transition is dense_conv -> avgpool2 into the next block's first
    channels.  In training every block keeps ONE table of batch statistics that all of its layers' norm1 and its transition share."""
    WIDTHS = {121: [256, 512, 1024, 1024], 169: [256, 512, 1280, 1664], 201: [256, 512, 1792, 1920]}

    def _make_encoders(self, encoder_depth, pretrained, pool0):
        enc = DenseNetEncoders(encoder_depth, pretrained=pretrained, pool0=pool0)
        self._widths = self.WIDTHS[encoder_depth]
        assert enc.encoder.widths == self._widths
        return enc, self._widths[3]

    def _encoder_widths(self, b):
        return list(self._widths)

    def _stem(self):
        return self.encoders.encoder.features.conv0, self.encoders.encoder.features.norm0

    def dead_parameter_names(self):
        return ['encoders.encoder.features.norm5.weight', 'encoders.encoder.features.norm5.bias',
                'encoders.encoder.last_linear.weight', 'encoders.encoder.last_linear.bias']

    @classmethod
    def translate_keys(cls, state_dict, dotted=False):
        """torchvision 0.2.0 (what the reference pins) registered a dense layer's modules as 'norm.1', 'conv.1', 'norm.2', 'conv.2'; current
        torch forbids dots in module names.  -> the same state_dict under the modern names (``dotted``: the other way round)."""
        import re
        if dotted:
            return {re.sub(r'(denselayer\d+)\.(norm|conv)([12])\.', r'\1.\2.\3.', k): v for k, v in state_dict.items()}
        return {re.sub(r'(denselayer\d+)\.(norm|conv)\.([12])\.', r'\1.\2\3.', k): v for k, v in state_dict.items()}

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super().load_state_dict(self.translate_keys(state_dict), strict=strict, **kw)

    def _emit_encoders(self, g, c1, slots):
        f = self.encoders.encoder.features
        x = c1
        for i, block in enumerate(slots):
            c = x.C
            if i == 0:
                g.copy(x, block.slice(0, c))             # the stem output opens denseblock1 (one salt_add launch)
            table = g.dense_table(block, f.norm0.eps) if g.train else None
            if g.train:
                g.dense_moments(block.slice(0, c), table, 0)
            for layer in getattr(f, 'denseblock%d' % (i + 1)).children():
                layer.emit(g, block, c, table)
                c += layer.growth_rate
            assert c == block.C
            if i < 3:
                x = getattr(f, 'transition%d' % (i + 1)).emit(g, block, table, slots[i + 1].slice(0, c // 2))
        return slots


class PSPModule(EmitOnly):
    """architectures/pspnet.py:9-28: per pyramid size AdaptiveAvgPool2d(s) -> bias-free 1x1 convolution -> bilinear resize back to (h, w);
    the results and the input concatenated; 1x1 ``bottleneck`` with bias; ReLU.  Executed by Graph.psp without the concatenation."""

    def __init__(self, features, out_features=1024, sizes=(1, 2, 3, 6)):
        super().__init__()
        self.stages = nn.ModuleList([self._make_stage(features, size) for size in sizes])
        self.bottleneck = nn.Conv2d(features * (len(sizes) + 1), out_features, kernel_size=1)
        self.relu = nn.ReLU()

    def _make_stage(self, features, size):
        return nn.Sequential(nn.AdaptiveAvgPool2d(output_size=(size, size)), nn.Conv2d(features, features, kernel_size=1, bias=False))

    def emit(self, g, x):
        return g.psp(x, self, name='PSPModule')


class PSPUpsample(EmitOnly):
    """architectures/pspnet.py:31-42: bilinear x2, then Conv2d(3x3, padding 1) -> BatchNorm2d -> nn.PReLU() (one slope)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_channels, out_channels, 3, padding=1), nn.BatchNorm2d(out_channels), nn.PReLU())

    def emit(self, g, x, out=None):
        return g.conv_bn_prelu(g.upsample(x, 2, name='PSPUpsample.up'), self.conv[0], self.conv[1], self.conv[2], out=out, name='PSPUpsample')


class PSPNet(HipNetwork):
    """architectures.pspnet.PSPNet (pspnet.py:45-105): ResNet18 / 34 encoders without the stem pool, PSPModule on encoder5 (a /16 map),
    four PSPUpsamples 1024 -> 512 -> 256 -> 128 -> 64 back to the input resolution, the hypercolumn [up1 | up2 x2 | up3 x4 | up4 x8] (960
    channels, materialised) and UNetResNet's final block.  F.dropout2d is an identity as everywhere in this file (torch 0.3.1 defaults to
    training=False): ``dropout_2d`` is accepted and ignored."""

    def __init__(self, encoder_depth, num_classes=2, sizes=(1, 2, 3, 6), deep_features_size=1024, dropout_2d=0.2, pretrained=False,
                 use_hypercolumn=False, pool0=False):
        super().__init__()
        if encoder_depth in (50, 101, 152):
            # pspnet.py:77-78 sizes ``final`` for 15 * 2048 // 8 = 3840 channels while the four PSPUpsamples still deliver 960: the
            # reference itself cannot run these depths
            raise NotImplementedError('PSPNet: depth %d is not built: the reference sizes final for 3840 hypercolumn channels and its '
                                      'up-sampling path delivers 960' % encoder_depth)
        if encoder_depth not in (18, 34):
            raise NotImplementedError('only 18, 34, 50, 101, 152 version of Resnet are implemented')
        if not use_hypercolumn:
            # pspnet.py:101-103 hands up4 (deep_features_size // 2 channels at 1/8 resolution) to a final block built for 64
            raise SaltError('PSPNet: use_hypercolumn=False does not run in the reference either (final expects 64 channels and gets up4\'s %d)'
                            % (deep_features_size // 2))
        if pool0:
            raise SaltError('PSPNet: pool0=True is not built')
        if tuple(sizes) != (1, 2, 3, 6) or deep_features_size != 1024:
            raise SaltError('PSPNet: sizes %s / deep_features_size %d are not built ((1, 2, 3, 6) and 1024 are: final expects 960 channels)'
                            % (tuple(sizes), deep_features_size))
        self.num_classes, self.dropout_2d, self.use_hypercolumn = num_classes, dropout_2d, use_hypercolumn
        self.encoders = ResNetEncoders(encoder_depth, pretrained=pretrained, pool0=pool0)
        b = 512
        self.psp = PSPModule(b, deep_features_size, sizes)
        self.up4 = PSPUpsample(deep_features_size, deep_features_size // 2)
        self.up3 = PSPUpsample(deep_features_size // 2, deep_features_size // 4)
        self.up2 = PSPUpsample(deep_features_size // 4, deep_features_size // 8)
        self.up1 = PSPUpsample(deep_features_size // 8, deep_features_size // 16)
        self.final = nn.Sequential(Conv2dBnRelu(15 * b // 8, b // 8), nn.Conv2d(b // 8, num_classes, kernel_size=1, padding=0))

    def dead_parameter_names(self):
        return ['encoders.encoder.fc.weight', 'encoders.encoder.fc.bias']

    def output_shape(self, shape):
        B, _, H, W = shape
        if H % 16 or W % 16 or H > 512 or W > 512:
            raise SaltError('PSPNet needs tiles whose sides are multiples of 16 up to 512 (got %dx%d): encoder5 is the /16 map and '
                            'salt_psp_pool takes at most 32x32 pixels' % (H, W))
        return (B, self.num_classes, H, W)

    def emit(self, g, x_nchw, logits):
        B, _, H, W = self.output_shape(tuple(x_nchw.shape))
        enc = self.encoders.encoder
        x = g.conv_first(x_nchw, enc.conv1, enc.bn1, relu=True, name='stem')
        for layer in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
            x = emit_blocks(g, layer, x)
        u4 = self.up4.emit(g, self.psp.emit(g, x))
        u3 = self.up3.emit(g, u4)
        u2 = self.up2.emit(g, u3)
        d = u2.C // 2
        hyper = g.new_act(B, H, W, d + u2.C + u3.C + u4.C, 'hypercolumn')
        # the reference computes up x2(up2) twice, inside up1 and for the hypercolumn: here the hypercolumn's slice IS up1's input
        up2x = g.upsample(u2, 2, out=hyper.slice(d, u2.C))
        g.conv_bn_prelu(up2x, self.up1.conv[0], self.up1.conv[1], self.up1.conv[2], out=hyper.slice(0, d), name='PSPUpsample')
        g.upsample(u3, 4, out=hyper.slice(d + u2.C, u3.C))
        g.upsample(u4, 8, out=hyper.slice(d + u2.C + u3.C, u4.C))
        g.head(self.final[0].emit(g, hyper), self.final[1], logits)


class GlobalConvolutionalNetwork(EmitOnly):
    """architectures/base.py:152-178: conv1 = (K x 1) -> (1 x K), conv2 = (1 x K) -> (K x 1), four Conv2dBnRelu with the one-sided replicate
    pad; the sum of the two branches.  conv1[0] and conv2[0] read the same wide map: Graph.gcn_pair runs them as one launch."""

    def __init__(self, in_channels, out_channels, kernel_size, use_relu=False):
        super().__init__()
        if not 2 <= kernel_size <= 9 or not 1 <= out_channels <= 32:
            raise SaltError('GlobalConvolutionalNetwork: kernel_size %d / %d output channels (salt_gcn_pair: kernel sizes 2 .. 9, at most 32 '
                            'output channels)' % (kernel_size, out_channels))
        k = kernel_size
        self.conv1 = nn.Sequential(Conv2dBnRelu(in_channels, out_channels, kernel_size=(k, 1), use_relu=use_relu, use_padding=True),
                                   Conv2dBnRelu(out_channels, out_channels, kernel_size=(1, k), use_relu=use_relu, use_padding=True))
        self.conv2 = nn.Sequential(Conv2dBnRelu(in_channels, out_channels, kernel_size=(1, k), use_relu=use_relu, use_padding=True),
                                   Conv2dBnRelu(out_channels, out_channels, kernel_size=(k, 1), use_relu=use_relu, use_padding=True))

    def emit(self, g, x, out=None, paired=None):
        """``paired``: None - Graph.gcn_pair with its measured shape rule (the default); True - the paired launch whatever the rule says;
        False - the composed route spelled out, conv1[0] and conv2[0] as two Graph.conv launches.  A keyword, not an environment switch."""
        v, h = self.conv1[0], self.conv2[0]
        if paired is False:
            av, ah = v.emit(g, x), h.emit(g, x)
        else:
            av, ah = g.gcn_pair(x, v.conv, v.batch_norm, h.conv, h.batch_norm, relu=v.use_relu, name='gcn', force=bool(paired))
        return g.add(self.conv1[1].emit(g, av), self.conv2[1].emit(g, ah), out=out, name='gcn.sum')


class BoundaryRefinement(EmitOnly):
    """architectures/base.py:181-197: x + Conv2dBnRelu(no ReLU)(Conv2dBnRelu(x)), both K x K with the replicate pad."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        k = (kernel_size, kernel_size)
        self.conv = nn.Sequential(Conv2dBnRelu(in_channels, out_channels, kernel_size=k, use_relu=True, use_padding=True),
                                  Conv2dBnRelu(in_channels, out_channels, kernel_size=k, use_relu=False, use_padding=True))

    def emit(self, g, x, out=None):
        last = self.conv[1]
        return g.conv(self.conv[0].emit(g, x), last.conv, last.batch_norm, relu=False, res=x, out=out, replicate=True, name='BoundaryRefinement')


class LargeKernelMatters(HipNetwork):
    """architectures.large_kernel_matters.LargeKernelMatters (large_kernel_matters.py:8-98): ResNet encoders without the stem pool, a
    GlobalConvolutionalNetwork + BoundaryRefinement on each of the /2, /4, /8 and /16 maps, and a 21-channel decoder of transposed
    convolutions, sums and BoundaryRefinements back to the tile's own size.  F.dropout2d is an identity as everywhere in this file:
    ``dropout_2d`` is accepted and ignored."""

    def __init__(self, encoder_depth, num_classes, kernel_size=9, internal_channels=21, use_relu=False, pretrained=False, dropout_2d=0.0,
                 pool0=False):
        super().__init__()
        if pool0:
            raise SaltError('LargeKernelMatters: pool0=True is not built (the reference then returns half-resolution logits)')
        if not 2 <= kernel_size <= 9 or not 1 <= internal_channels <= 32:
            raise SaltError('LargeKernelMatters: kernel_size %d / internal_channels %d (salt_gcn_pair: kernel sizes 2 .. 9, at most 32 output '
                            'channels)' % (kernel_size, internal_channels))
        self.num_classes, self.dropout_2d = num_classes, dropout_2d
        self.encoders = ResNetEncoders(encoder_depth, pretrained=pretrained, pool0=pool0)
        b, c = (512 if encoder_depth in (18, 34) else 2048), internal_channels
        self.gcn2 = GlobalConvolutionalNetwork(b // 8, c, kernel_size, use_relu=use_relu)
        self.gcn3 = GlobalConvolutionalNetwork(b // 4, c, kernel_size, use_relu=use_relu)
        self.gcn4 = GlobalConvolutionalNetwork(b // 2, c, kernel_size, use_relu=use_relu)
        self.gcn5 = GlobalConvolutionalNetwork(b, c, kernel_size, use_relu=use_relu)
        for name in ('enc_br2', 'enc_br3', 'enc_br4', 'enc_br5', 'dec_br1', 'dec_br2', 'dec_br3', 'dec_br4'):
            setattr(self, name, BoundaryRefinement(c, c, 3))
        for name in ('deconv5', 'deconv4', 'deconv3', 'deconv2'):
            setattr(self, name, DeconvConv2dBnRelu(c, c))
        self.final = nn.Conv2d(c, num_classes, kernel_size=1, padding=0)
        self.paired = None           # GlobalConvolutionalNetwork.emit's keyword for all four blocks (None: the shape rule decides); set before the first forward

    def dead_parameter_names(self):
        return ['encoders.encoder.fc.weight', 'encoders.encoder.fc.bias']

    def output_shape(self, shape):
        B, _, H, W = shape
        if H % 16 or W % 16:
            raise SaltError('LargeKernelMatters needs tiles whose sides are multiples of 16 (got %dx%d): encoder5 is the /16 map and every '
                            'decoder level doubles it' % (H, W))
        return (B, self.num_classes, H, W)

    def emit(self, g, x_nchw, logits):
        self.output_shape(tuple(x_nchw.shape))
        enc = self.encoders.encoder
        x = g.conv_first(x_nchw, enc.conv1, enc.bn1, relu=True, name='stem')
        e2 = emit_blocks(g, enc.layer1, x)
        e3 = emit_blocks(g, enc.layer2, e2)
        e4 = emit_blocks(g, enc.layer3, e3)
        e5 = emit_blocks(g, enc.layer4, e4)
        gcn2 = self.enc_br2.emit(g, self.gcn2.emit(g, e2, paired=self.paired))
        gcn3 = self.enc_br3.emit(g, self.gcn3.emit(g, e3, paired=self.paired))
        gcn4 = self.enc_br4.emit(g, self.gcn4.emit(g, e4, paired=self.paired))
        gcn5 = self.enc_br5.emit(g, self.gcn5.emit(g, e5, paired=self.paired))
        d5 = self.deconv5.emit(g, gcn5)
        d4 = self.deconv4.emit(g, self.dec_br4.emit(g, g.add(d5, gcn4, name='dec4.sum')))
        d3 = self.deconv3.emit(g, self.dec_br3.emit(g, g.add(d4, gcn3, name='dec3.sum')))
        d2 = self.dec_br1.emit(g, self.deconv2.emit(g, self.dec_br2.emit(g, g.add(d3, gcn2, name='dec2.sum'))))
        g.head(d2, self.final, logits)


class DepthChannelExcitation(EmitOnly):
    """architectures/base.py:120-131: x * sigmoid(Linear(1, C)(d))[:, :, None, None]."""

    def __init__(self, channels):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(1, channels), nn.Sigmoid())


class UNetResNetWithDepth(UNetResNet):
    """architectures.models_with_depth.UNetResNetWithDepth: UNetResNet whose hypercolumn (or dec1 alone) is scaled per image and
    channel by a gate computed from the tile's depth ``d`` [B,1] before the final block.  The scale commutes with the bilinear
    up-sampling, so every level is gated at its own resolution (Graph.channel_gate) and the factored / planar hypercolumn paths of
    UNetResNet.emit are used as they are: dec5 .. dec2 also feed the next decoder and get a gated copy, dec1 is gated in place (the
    scSE backward that produced it reads its output for the ReLU mask only, and the gate is positive)."""

    uses_depth = True

    def __init__(self, encoder_depth, num_classes, dropout_2d=0.0, pretrained=False, use_hypercolumn=False):
        super().__init__(encoder_depth, num_classes, dropout_2d=dropout_2d, pretrained=pretrained, use_hypercolumn=use_hypercolumn)
        self.depth_channel_excitation = DepthChannelExcitation((5 if use_hypercolumn else 1) * self.bottom // 8)

    def emit(self, g, x_nchw, logits):
        if 'd' not in g.step_inputs:
            raise SaltError('UNetResNetWithDepth needs the graph\'s depth input (CompiledNet allocates it)')
        # first operator of the main stream: the side-stream level gates and the in-place gate of dec1 are all ordered behind it
        self._gate = g.depth_gate(g.step_inputs['d'], self.depth_channel_excitation.fc[0])
        try:
            super().emit(g, x_nchw, logits)
        finally:
            self._gate = None

    def _hyper_in(self, g, x, c0, last=False):
        return g.channel_gate(x, self._gate, c0, out=x if last else None, name='depth_gate.c%d' % c0)


class EmptinessClassifier(HipNetwork):
    """architectures.misc.EmptinessClassifier (misc.py:39-81), the per-tile "any salt at all" classifier empty_vs_non_empty.py trains:
    ResNet stem without max-pool, layer1..4, then AvgPool2d(8) + 1x1 convolution on the /16 map (Graph.pool_head).  A 128x128 tile
    gives [B, num_classes, 1, 1] logits."""

    is_classifier = True        # Model.score_validation: ROC-AUC of the 1x1 output instead of the mask metrics

    def __init__(self, num_classes=2, encoder_depth=18, pretrained=False):
        super().__init__()
        if encoder_depth not in ResNet.CFG:
            raise NotImplementedError('only 18, 34, 50, 101, 152 version of Resnet are implemented')
        self.num_classes = num_classes
        self.encoder = resnet(encoder_depth, pretrained)
        self.bottom = 512 if encoder_depth in (18, 34) else 2048
        self.conv1 = nn.Sequential(self.encoder.conv1, self.encoder.bn1, self.encoder.relu)
        self.encoder2 = self.encoder.layer1
        self.encoder3 = self.encoder.layer2
        self.encoder4 = self.encoder.layer3
        self.encoder5 = self.encoder.layer4
        self.classifier = nn.Sequential(nn.AvgPool2d(8), nn.Conv2d(self.bottom, num_classes, kernel_size=1, padding=0))

    def dead_parameter_names(self):
        return ['encoder.fc.weight', 'encoder.fc.bias']

    def output_shape(self, shape):
        B, _, H, W = shape
        if H < 128 or W < 128:
            raise SaltError('EmptinessClassifier needs tiles of at least 128x128 (got %dx%d): the layer4 map is smaller than the 8x8 pool window'
                            % (H, W))
        return (B, self.num_classes, H // 128, W // 128)

    def emit(self, g, x_nchw, logits):
        self.output_shape(tuple(x_nchw.shape))
        enc = self.encoder
        x = g.conv_first(x_nchw, enc.conv1, enc.bn1, relu=True, name='stem')
        for layer in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
            x = emit_blocks(g, layer, x)
        g.pool_head(x, self.classifier[1], logits)


class StackingFCN(HipNetwork):
    """architectures.misc.StackingFCN (misc.py:8-20), the second-level network of main.py's SECOND_LEVEL switch: one replicate-padded
    3x3 Conv2dBnRelu over the ``input_model_nr`` stacked out-of-fold probability maps and a 1x1 logit head.  The input is the fp32
    [B, input_model_nr, H, W] tensor the stacking loader emits; eval is ONE launch (Graph.stack_conv).  F.dropout2d(p=dropout_2d) is
    an identity here as everywhere else in this file (torch 0.3.1 defaults to training=False, and the registry passes 0)."""

    def __init__(self, input_model_nr, num_classes, filter_nr=32, dropout_2d=0.0):
        super().__init__()
        from .engine import stack_conv_parts
        stack_conv_parts(1, input_model_nr, 1, 1, filter_nr)          # SaltError for a shape the kernel does not run
        if not 1 <= num_classes <= 4:
            raise SaltError('%s: %d classes (the fused 1x1 head takes 1 .. 4)' % (type(self).__name__, num_classes))
        self.input_model_nr, self.num_classes, self.dropout_2d = input_model_nr, num_classes, dropout_2d
        self.conv = nn.Sequential(Conv2dBnRelu(input_model_nr, filter_nr, kernel_size=(3, 3)))
        self._more_modules(filter_nr)
        self.final = nn.Sequential(nn.Conv2d(filter_nr, num_classes, kernel_size=1, padding=0))

    def _more_modules(self, filter_nr):
        """Hook: modules the reference registers between ``conv`` and ``final`` (state_dict order)."""

    def output_shape(self, shape):
        B, M, H, W = shape
        if M != self.input_model_nr:
            raise SaltError('%s was built for %d stacked maps, the batch has %d' % (type(self).__name__, self.input_model_nr, M))
        return (B, self.num_classes, H, W)

    def dead_parameter_names(self):
        return []

    def _gate(self, g):
        return None

    def emit(self, g, x_nchw, logits):
        self.output_shape(tuple(x_nchw.shape))
        blk = self.conv[0]
        gate = self._gate(g)
        if not g.train:
            g.stack_conv(x_nchw, blk.conv, blk.batch_norm, relu=blk.use_relu, head=self.final[0], gate=gate, logits=logits)
            return
        a = g.stack_conv(x_nchw, blk.conv, blk.batch_norm, relu=blk.use_relu)
        if gate is not None:
            a = g.channel_gate(a, gate, 0, name='depth_gate')
        g.head(a, self.final[0], logits)


class StackingFCNWithDepth(StackingFCN):
    """architectures.misc.StackingFCNWithDepth (misc.py:23-36): the same with DepthChannelExcitation between the block and the head."""

    uses_depth = True

    def _more_modules(self, filter_nr):
        self.depth_channel_excitation = DepthChannelExcitation(filter_nr)

    def _gate(self, g):
        if 'd' not in g.step_inputs:
            raise SaltError('StackingFCNWithDepth needs the graph\'s depth input (CompiledNet allocates it)')
        return g.depth_gate(g.step_inputs['d'], self.depth_channel_excitation.fc[0])


class TernausUNetResNet(HipNetwork):
    """unet_models.UNetResNet — TernausNet-style decoder (DecoderBlockV2), exported as unet_models.UNetResNet."""

    def __init__(self, encoder_depth, num_classes, num_filters=32, dropout_2d=0.2, pretrained=False, is_deconv=False):
        super().__init__()
        if dropout_2d != 0.0:
            # the reference environment pins torch==0.3.1 (environment.yml:17) where F.dropout2d(x, p) defaults to
            # training=False, i.e. the call at unet_models.py:150 is an identity there.  We keep that behaviour.
            pass
        if encoder_depth not in (34, 101, 152):
            raise NotImplementedError('only 34, 101, 152 version of Resnet are implemented')
        self.num_classes, self.dropout_2d, self.is_deconv = num_classes, dropout_2d, is_deconv
        self.encoder = resnet(encoder_depth, pretrained)
        b = 512 if encoder_depth == 34 else 2048
        self.pool = nn.MaxPool2d(2, 2)
        self.relu = nn.ReLU(inplace=True)
        self.input_adjust = nn.Sequential(self.encoder.conv1, self.encoder.bn1, self.encoder.relu)
        self.conv1, self.conv2, self.conv3, self.conv4 = self.encoder.layer1, self.encoder.layer2, self.encoder.layer3, self.encoder.layer4
        nf = num_filters
        self.dec4 = DecoderBlockV2(b, nf * 8 * 2, nf * 8, is_deconv)
        self.dec3 = DecoderBlockV2(b // 2 + nf * 8, nf * 8 * 2, nf * 8, is_deconv)
        self.dec2 = DecoderBlockV2(b // 4 + nf * 8, nf * 4 * 2, nf * 2, is_deconv)
        self.dec1 = DecoderBlockV2(b // 8 + nf * 2, nf * 2 * 2, nf * 2 * 2, is_deconv)
        self.final = nn.Conv2d(nf * 2 * 2, num_classes, kernel_size=1)
        self.bottom, self.nf = b, nf

    def dead_parameter_names(self):
        dead = ['encoder.fc.weight', 'encoder.fc.bias']
        for n in ('dec4', 'dec3', 'dec2', 'dec1'):
            blk = getattr(self, n)
            dead += ['%s.%s' % (n, k) for k, _ in blk.named_parameters() if k.startswith(blk.dead_prefix())]
        return dead

    def emit(self, g, x_nchw, logits):
        enc = self.encoder
        B, _, H, W = x_nchw.shape
        b, nf = self.bottom, self.nf
        a = g.conv_first(x_nchw, enc.conv1, enc.bn1, relu=True, name='stem')
        cat3 = g.new_act(B, H // 8, W // 8, nf * 8 + b // 2, 'cat3')        # [dec4 | conv3]
        cat2 = g.new_act(B, H // 4, W // 4, nf * 8 + b // 4, 'cat2')        # [dec3 | conv2]
        cat1 = g.new_act(B, H // 2, W // 2, nf * 2 + b // 8, 'cat1')        # [dec2 | conv1]
        c1 = emit_blocks(g, enc.layer1, a, out=cat1.slice(nf * 2, b // 8))
        c2 = emit_blocks(g, enc.layer2, c1, out=cat2.slice(nf * 8, b // 4))
        c3 = emit_blocks(g, enc.layer3, c2, out=cat3.slice(nf * 8, b // 2))
        ce = emit_blocks(g, enc.layer4, c3)
        self.dec4.emit(g, ce, out=cat3.slice(0, nf * 8))
        self.dec3.emit(g, cat3, out=cat2.slice(0, nf * 8))
        self.dec2.emit(g, cat2, out=cat1.slice(0, nf * 2))
        d1 = self.dec1.emit(g, cat1)
        g.head(d1, self.final, logits)


class _SaltResNet34Stub(HipNetwork):
    """Shared plumbing of SaltUNet / SaltLinkNet: a whole torchvision-layout resnet34 is constructed (its unused blocks stay in
    ``state_dict()`` and ``parameters()`` exactly like the reference) but only a few BasicBlocks are on the path."""

    used_blocks = ()

    def _make(self, num_classes, dropout_2d, pretrained):
        self.num_classes, self.dropout_2d = num_classes, dropout_2d
        self.encoder = resnet(34, pretrained)
        self.relu = nn.ReLU(inplace=True)
        self.input_adjust = nn.Sequential(self.encoder.conv1, self.encoder.bn1, self.encoder.relu)

    def dead_parameter_names(self):
        live = ['encoder.conv1.', 'encoder.bn1.'] + ['encoder.%s.' % b for b in self.used_blocks]
        dead = [k for k, _ in self.encoder.named_parameters(prefix='encoder') if not any(k.startswith(l) for l in live)]
        for n in self.decoders:
            blk = getattr(self, n)
            dead += ['%s.%s' % (n, k) for k, _ in blk.named_parameters() if k.startswith(blk.dead_prefix())]
        return dead


class SaltUNet(_SaltResNet34Stub):
    """unet_models.SaltUNet (unet_models.py:154-189): stem, layer1[1], layer1[2], layer2[0], layer2[1]; DecoderBlockV2 / ConvBnRelu
    decoders over concatenated skips; 1x1 head.  layer1[0] and everything after layer2[1] is constructed but never called."""

    used_blocks = ('layer1.1', 'layer1.2', 'layer2.0', 'layer2.1')
    decoders = ('dec3', 'dec1')

    def __init__(self, num_classes, dropout_2d=0.2, pretrained=False, is_deconv=False):
        super().__init__()
        self._make(num_classes, dropout_2d, pretrained)
        self.conv1 = self.encoder.layer1[1]
        self.conv2 = self.encoder.layer1[2]
        self.conv3 = self.encoder.layer2[0]
        self.conv4 = self.encoder.layer2[1]
        self.dec3 = DecoderBlockV2(256, 512, 256, is_deconv)
        self.dec2 = ConvBnRelu(256 + 64, 256)
        self.dec1 = DecoderBlockV2(256 + 64, (256 + 64) * 2, 256, is_deconv)
        self.final = nn.Conv2d(256, num_classes, kernel_size=1)

    def emit(self, g, x_nchw, logits):
        enc = self.encoder
        B, _, H, W = x_nchw.shape
        a = g.conv_first(x_nchw, enc.conv1, enc.bn1, relu=True, name='stem')
        cat1 = g.new_act(B, H // 2, W // 2, 256 + 64, 'cat1')            # [dec2 | conv1]
        cat2 = g.new_act(B, H // 2, W // 2, 256 + 64, 'cat2')            # [dec3 | conv2]
        cat3 = g.new_act(B, H // 4, W // 4, 128 + 128, 'cat3')           # [center | conv3]
        c1 = self.conv1.emit(g, a, out=cat1.slice(256, 64))
        c2 = self.conv2.emit(g, c1, out=cat2.slice(256, 64))
        c3 = self.conv3.emit(g, c2, out=cat3.slice(128, 128))
        self.conv4.emit(g, c3, out=cat3.slice(0, 128))
        self.dec3.emit(g, cat3, out=cat2.slice(0, 256))
        self.dec2.emit(g, cat2, out=cat1.slice(0, 256))
        d1 = self.dec1.emit(g, cat1)
        g.head(d1, self.final, logits)


class SaltLinkNet(_SaltResNet34Stub):
    """unet_models.SaltLinkNet (unet_models.py:192-233): block outputs of layer1[1..2] and layer2[0..3] are summed per stage."""

    used_blocks = ('layer1.1', 'layer1.2', 'layer2.0', 'layer2.1', 'layer2.2', 'layer2.3')
    decoders = ('dec2', 'dec1')

    def __init__(self, num_classes, dropout_2d=0.2, pretrained=False, is_deconv=False):
        super().__init__()
        self._make(num_classes, dropout_2d, pretrained)
        self.conv1_1 = self.encoder.layer1[1]
        self.conv1_2 = self.encoder.layer1[2]
        self.conv2_0 = self.encoder.layer2[0]
        self.conv2_1 = self.encoder.layer2[1]
        self.conv2_2 = self.encoder.layer2[2]
        self.conv2_3 = self.encoder.layer2[3]
        self.dec2 = DecoderBlockV2(128, 256, 256, is_deconv=is_deconv)
        self.dec1 = DecoderBlockV2(256 + 64, 512, 256, is_deconv=is_deconv)
        self.final = nn.Conv2d(256, num_classes, kernel_size=1)

    def emit(self, g, x_nchw, logits):
        enc = self.encoder
        B, _, H, W = x_nchw.shape
        a = g.conv_first(x_nchw, enc.conv1, enc.bn1, relu=True, name='stem')
        c11 = self.conv1_1.emit(g, a)
        c12 = self.conv1_2.emit(g, c11)
        c20 = self.conv2_0.emit(g, c12)
        c21 = self.conv2_1.emit(g, c20)
        c22 = self.conv2_2.emit(g, c21)
        c23 = self.conv2_3.emit(g, c22)
        cat1 = g.new_act(B, H // 2, W // 2, 256 + 64, 'cat1')            # [dec2 | conv1_sum]
        g.add(c11, c12, out=cat1.slice(256, 64), name='conv1_sum')
        s2 = g.add(g.add(g.add(c20, c21), c22), c23, name='conv2_sum')   # left-to-right like the reference expression
        self.dec2.emit(g, s2, out=cat1.slice(0, 256))
        d1 = self.dec1.emit(g, cat1)
        g.head(d1, self.final, logits)


class VanillaUNet(HipNetwork):
    """BASELINE C0/C1 "vanilla 4-level U-Net": the reference has no in-tree definition; it is
    assembled from the reference's own blocks: per level 2 x ConvBnRelu + MaxPool2d(2,2); centre 2 x ConvBnRelu;
    per level DeconvConv2dBnRelu (ConvT k3 s2 p1 op1 + BN + ReLU), concat skip, 2 x ConvBnRelu; 1x1 head."""

    def __init__(self, num_classes=2, in_channels=1, base_filters=16, levels=4):
        super().__init__()
        self.num_classes, self.levels = num_classes, levels
        c = in_channels
        for i in range(1, levels + 1):
            f = base_filters * 2 ** (i - 1)
            setattr(self, 'enc%d' % i, nn.Sequential(ConvBnRelu(c, f), ConvBnRelu(f, f)))
            c = f
        f = base_filters * 2 ** levels
        self.center = nn.Sequential(ConvBnRelu(c, f), ConvBnRelu(f, f))
        c = f
        for i in range(levels, 0, -1):
            f = base_filters * 2 ** (i - 1)
            setattr(self, 'up%d' % i, DeconvConv2dBnRelu(c, f))
            setattr(self, 'dec%d' % i, nn.Sequential(ConvBnRelu(2 * f, f), ConvBnRelu(f, f)))
            c = f
        self.final = nn.Conv2d(c, num_classes, kernel_size=1)
        self.base = base_filters

    def emit(self, g, x_nchw, logits):
        B, _, H, W = x_nchw.shape
        L = self.levels
        cats = {}
        x = None
        for i in range(1, L + 1):
            f = self.base * 2 ** (i - 1)
            h, w = H >> (i - 1), W >> (i - 1)
            cats[i] = g.new_act(B, h, w, 2 * f, 'cat%d' % i)                 # [up_i | enc_i]
            enc = getattr(self, 'enc%d' % i)
            if i == 1:
                c0 = enc[0].conv
                a = g.conv_first(x_nchw, c0[0], c0[1], relu=True, name='enc1.0')
            else:
                a = enc[0].emit(g, x)
            skip = enc[1].emit(g, a, out=cats[i].slice(f, f))
            x = g.maxpool2(skip, name='pool%d' % i)
        x = self.center[1].emit(g, self.center[0].emit(g, x))
        for i in range(L, 0, -1):
            f = self.base * 2 ** (i - 1)
            getattr(self, 'up%d' % i).emit(g, x, out=cats[i].slice(0, f))
            dec = getattr(self, 'dec%d' % i)
            x = dec[1].emit(g, dec[0].emit(g, cats[i]))
        g.head(x, self.final, logits)
