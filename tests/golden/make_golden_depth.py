#!/usr/bin/env python
"""Generate the F14 fixtures (depth-conditioned network) by EXECUTING THE REFERENCE'S OWN MODULES.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_depth.py
Same conventions as make_golden.py: closed-form weights keyed by state-dict name (closed_form.py), the reference's
sources imported through the stubs of ref_import.py, only .npz data is written.

  F14_depth_channel_excitation_{train,eval}  base.DepthChannelExcitation on a small odd-sized block (C = 20): x, d, y, gy, gx and the
                                             gradients of fc.0.weight / fc.0.bias
  F14_unet_resnet34_depth_{hyper,nohyper}    models_with_depth.UNetResNetWithDepth at 64x64, B = 2, D = [[0.2], [0.6]], laid out like
                                             the F8 fixtures, plus `d` and `ref_f32_vs_f64_maxabs` (largest absolute deviation of the
                                             fp32 reference's eval logits from the same module run in float64)
"""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import closed_form as CF          # noqa: E402
import ref_import as R            # noqa: E402
from make_golden import canonical_fn, save          # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def main():
    assert R.reference_available(), 'reference not mounted'
    base = R.load('architectures.base')
    wd = R.load('architectures.models_with_depth')
    models = R.load_models_module()

    # ---- block: odd sizes, C not a multiple of 16
    x = CF.input_for('f14', (2, 20, 5, 7))
    d = torch.tensor([[0.35], [0.8]])
    for train in (True, False):
        mod = base.DepthChannelExcitation(20)
        CF.fill_module(mod)
        mod.train(train)
        xv = x.clone().requires_grad_(True)
        y = mod(xv, d)
        gy = CF.input_for('gy:%s' % (tuple(y.shape),), y.shape)
        y.backward(gy)
        out = OrderedDict(x=x, d=d, y=y, gy=gy, gx=xv.grad)
        for k, p in mod.named_parameters():
            out['g:' + k] = p.grad
        for k, v in mod.state_dict().items():
            out['s:' + k] = v
        save('F14_depth_channel_excitation_%s' % ('train' if train else 'eval'), **out)

    # ---- whole networks
    X = CF.input_for('f8', (2, 3, 64, 64))
    T = CF.mask_for('f8', (2, 64, 64))
    D = torch.tensor([[0.2], [0.6]])
    for tag, hyper in (('hyper', True), ('nohyper', False)):
        net = wd.UNetResNetWithDepth(34, 2, dropout_2d=0.0, pretrained=False, use_hypercolumn=hyper)
        canon = canonical_fn(net)
        CF.fill_module(net, canonical=canon)
        net.eval()
        with torch.no_grad():
            logits = net(X, D)
            logits64 = copy.deepcopy(net).double()(X.double(), D.double())
        out = OrderedDict(x=X, d=D, t=T, eval_logits=logits, eval_mask=(logits[:, 1] > 0).to(torch.uint8))
        out['ref_f32_vs_f64_maxabs'] = float((logits.double() - logits64).abs().max())
        out['ref_f32_mask_flips_vs_f64'] = int(((logits[:, 1] > 0) != (logits64[:, 1] > 0)).sum())
        out['keys'] = np.array(list(net.state_dict().keys()))
        # one training step exactly as SegmentationModelWithDepth._fit_loop (models.py:222-253)
        net.train()
        params = [p for p in net.parameters() if p.requires_grad]
        opt = torch.optim.Adam([{'params': params, 'weight_decay': 1e-4}], lr=1e-4)
        opt.zero_grad()
        o = net(X, D)
        loss = models.lovasz_loss(o, T) * 1.0
        loss.backward()
        out['train_logits'] = o
        out['train_loss'] = loss
        names, gnorm, gsum, has_grad = [], [], [], []
        for k, p in net.named_parameters():
            names.append(k)
            has_grad.append(p.grad is not None)
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            gnorm.append(float(g.double().norm()))
            gsum.append(float(g.double().sum()))
        named = dict(net.named_parameters())
        for k in [n for n in names if n.endswith('final.1.weight') or n.endswith('encoder.conv1.weight')
                  or n.startswith('depth_channel_excitation.')]:
            out['fullgrad:' + k] = named[k].grad.clone()
        opt.step()
        out['param_names'] = np.array(names)
        out['param_has_grad'] = np.array(has_grad)
        out['grad_norm'] = np.array(gnorm)
        out['grad_sum'] = np.array(gsum)
        out['post_norm'] = np.array([float(p.detach().double().norm()) for _, p in net.named_parameters()])
        out['post_sum'] = np.array([float(p.detach().double().sum()) for _, p in net.named_parameters()])
        sd = net.state_dict()
        bn_keys = [k for k in sd if k.endswith('running_mean') or k.endswith('running_var')]
        bn_keys = [k for k in bn_keys if canon(k) == k]
        out['bn_keys'] = np.array(bn_keys)
        out['bn_sum'] = np.array([float(sd[k].double().sum()) for k in bn_keys])
        save('F14_unet_resnet34_depth_' + tag, **out)
        gate = torch.sigmoid(sd['depth_channel_excitation.fc.0.weight'] @ D.t() + sd['depth_channel_excitation.fc.0.bias'][:, None])
        print('  %s: gate %.3f..%.3f  max|logit| %.1f  min|logit[1]| %.2e  f32 vs f64 %.2e  flips %d' % (
            tag, float(gate.min()), float(gate.max()), float(logits.abs().max()), float(logits[:, 1].abs().min()),
            out['ref_f32_vs_f64_maxabs'], out['ref_f32_mask_flips_vs_f64']))


if __name__ == '__main__':
    main()
