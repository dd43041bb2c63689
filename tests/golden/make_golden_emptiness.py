#!/usr/bin/env python
"""Generate the F15 fixtures (emptiness classifier) by EXECUTING THE REFERENCE'S OWN MODULES.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_emptiness.py
Same conventions as make_golden.py / make_golden_depth.py: closed-form weights keyed by state-dict name (closed_form.py), the
reference's sources imported through the stubs of ref_import.py, only .npz data is written.

  F15_pool_head                      the bare `classifier` Sequential (nn.AvgPool2d(8) + nn.Conv2d(C, K, 1)) of misc.EmptinessClassifier
                                     on [2,20,12,20]: odd C, a ragged 12-row map (rows 8..11 belong to no window), OW = 2, K = 3;
                                     x, y, gy, gx, g:weight, g:bias
  F15_emptiness_resnet18_128         misc.EmptinessClassifier(2, 18) at [2,3,128,128] ([B,2,1,1] logits): eval logits plus one training
                                     step as SegmentationModel._fit_loop runs it (lovasz_loss, Adam lr 1e-4 + L2 1e-4), laid out like the
                                     F14 network fixtures.  The input is CF.input_for('f15', x_shape); `x` itself is stored where it is
                                     small.  Training targets: image 0 [0,1] (not empty), image 1 [1,0] (empty)
  F15_emptiness_resnet18_256         the same at [2,3,256,256]: a 2x2 output, the targets broadcast to [B,2,2,2].  A TEST CONSTRUCTION so
                                     that more than one pool window runs through the whole network; the reference's loader never makes it
  F15_emptiness_resnet34_128         depth 34, eval only

Every network fixture also records the reference's own numerical error, which the GPU tests' guards are derived from:
  ref_f32_vs_f64_maxabs              largest absolute deviation of the fp32 eval logits from the same module run in float64
  ref_f32_vs_f64_gradnorm_rel        (fixtures with a training step) worst per-tensor relative deviation of the fp32 gradient norms from
                                     the float64 run's.  The reference's lovasz_hinge does not run in double (torch.dot dtype error), so
                                     the float64 leg alone uses the dtype-generic restatement below
  ref_bf16_storage_vs_f32_maxabs     eval logits of the test-side oracle (tests/emptiness_oracle.py) under oracle.blocks.bf16_storage
                                     against the same oracle in fp32: what bf16 activation storage costs an independent implementation
"""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: emptiness_oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root: oracle
import closed_form as CF          # noqa: E402
import ref_import as R            # noqa: E402
from make_golden import canonical_fn, save          # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def lovasz_loss_any_dtype(output, target):
    """models.py:326-328 + lovasz_losses.py:81-115 (per image, F.elu variant) with the labels cast to the logits' dtype."""
    vals = []
    for lg, lb in zip(output, target):
        lg, lb = lg.reshape(-1), lb.reshape(-1).to(lg.dtype)
        err = 1.0 - lg * (2.0 * lb - 1.0)
        es, perm = torch.sort(err, dim=0, descending=True)
        gt = lb[perm]
        total = gt.sum()
        jac = 1.0 - (total - gt.cumsum(0)) / (total + (1.0 - gt).cumsum(0))
        if gt.numel() > 1:
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        vals.append(torch.dot(F.elu(es), jac))
    return sum(vals) / len(vals)


def grad_norms(net):
    return OrderedDict((k, float(p.grad.double().norm())) for k, p in net.named_parameters() if p.grad is not None)


def network_fixture(misc, models, name, depth, size, train_step):
    import emptiness_oracle as EO
    from oracle import blocks as OB
    X = CF.input_for('f15', (2, 3, size, size))
    net = misc.EmptinessClassifier(num_classes=2, encoder_depth=depth, pretrained=False)
    canon = canonical_fn(net)
    CF.fill_module(net, canonical=canon)
    net.eval()
    with torch.no_grad():
        logits = net(X)
        logits64 = copy.deepcopy(net).double()(X.double())
    out = OrderedDict(x_shape=np.array(X.shape), eval_logits=logits)
    if X.numel() * 4 <= 512 * 1024:           # the 256x256 input alone would pass the size limit of a committed file: it is closed-form,
        out['x'] = X                          # the tests rebuild it from x_shape (CF.input_for('f15', x_shape))
    out['ref_f32_vs_f64_maxabs'] = float((logits.double() - logits64).abs().max())
    out['keys'] = np.array(list(net.state_dict().keys()))
    sd = {k: v.clone() for k, v in net.state_dict().items() if canon(k) == k}
    with torch.no_grad():
        o32 = EO.emptiness_classifier(sd, X, False, depth=depth)
        with OB.bf16_storage():
            o16 = EO.emptiness_classifier(sd, X, False, depth=depth)
    assert float((o32 - logits).abs().max()) <= 1e-3 * float(logits.abs().max()), 'test-side oracle does not reproduce the reference'
    out['ref_bf16_storage_vs_f32_maxabs'] = float((o16.double() - o32.double()).abs().max())
    msg = '  %s: logits %s  max|logit| %.2f  min|logit[1]| %.2e  f32 vs f64 %.2e  bf16 storage %.2e' % (
        name, tuple(logits.shape), float(logits.abs().max()), float(logits[:, 1].abs().min()), out['ref_f32_vs_f64_maxabs'],
        out['ref_bf16_storage_vs_f32_maxabs'])
    if train_step:
        oh = logits.shape[2]
        T = torch.tensor([[0.0, 1.0], [1.0, 0.0]]).reshape(2, 2, 1, 1).expand(2, 2, oh, oh).contiguous()
        out['t'] = T
        # float64 leg first (a deep copy: the fp32 module below starts from the same state)
        net.train()
        n64 = copy.deepcopy(net).double()
        lovasz_loss_any_dtype(n64(X.double()), T.double()).backward()
        g64 = grad_norms(n64)
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
        out['ref_f32_vs_f64_gradnorm_rel'] = max(abs(g32[k] - g64[k]) / g64[k] for k in g64)
        names, gnorm, gsum, has_grad = [], [], [], []
        for k, p in net.named_parameters():
            names.append(k)
            has_grad.append(p.grad is not None)
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            gnorm.append(float(g.double().norm()))
            gsum.append(float(g.double().sum()))
        named = dict(net.named_parameters())
        for k in ('classifier.1.weight', 'classifier.1.bias'):
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
        msg += '  grad-norm f32 vs f64 %.2e  min grad norm %.2e  live tensors %d' % (
            out['ref_f32_vs_f64_gradnorm_rel'], min(v for v, h in zip(gnorm, has_grad) if h), sum(has_grad))
    save(name, **out)
    print(msg)


def main():
    assert R.reference_available(), 'reference not mounted'
    misc = R.load('architectures.misc')
    models = R.load_models_module()

    # ---- the bare head: odd C, ragged rows, two windows across, K = 3
    cls = misc.EmptinessClassifier(num_classes=3, encoder_depth=18, pretrained=False).classifier
    cls[1] = torch.nn.Conv2d(20, 3, kernel_size=1, padding=0)
    CF.fill_module(cls)
    x = CF.input_for('f15', (2, 20, 12, 20)).requires_grad_(True)
    y = cls(x)
    gy = CF.input_for('gy:%s' % (tuple(y.shape),), y.shape)
    y.backward(gy)
    out = OrderedDict(x=x, y=y, gy=gy, gx=x.grad)
    for k, p in cls.named_parameters():
        out['g:' + k[2:]] = p.grad
    for k, v in cls.state_dict().items():
        out['s:' + k] = v
    save('F15_pool_head', **out)

    network_fixture(misc, models, 'F15_emptiness_resnet18_128', 18, 128, True)
    network_fixture(misc, models, 'F15_emptiness_resnet18_256', 18, 256, True)
    network_fixture(misc, models, 'F15_emptiness_resnet34_128', 34, 128, False)


if __name__ == '__main__':
    main()
