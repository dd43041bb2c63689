#!/usr/bin/env python
"""Generate the F21 fixtures (LargeKernelMatters) by EXECUTING THE REFERENCE'S OWN architectures/large_kernel_matters.py and base.py.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_lkm.py

  F21_gcn_{train,eval}      base.GlobalConvolutionalNetwork(64, 21, 9, use_relu=True) on [2,64,6,10] (H < K - 1 < W): output, input
                            gradient, every parameter gradient, the running statistics after the pass, the pass fraction of each ReLU
  F21_gcn_norelu_train      the same block with the class default use_relu=False
  F21_br_{train,eval}       base.BoundaryRefinement(21, 21, 3) on [2,21,5,7]
  F21_lkm34                 LargeKernelMatters(34, 2) with the registry's model_config (kernel_size 9, internal_channels 21, use_relu,
                            pool0 off; pretrained off) at [2,3,64,64] - encoder5 is 4x4, every vertical tap of gcn5 clamps onto row 0 -
                            with closed-form weights: eval logits plus one training step as SegmentationModel._fit_loop runs it, in
                            the F19 / F20 layout.  No weights are stored, except the two values of final.bias where the class-1 bias
                            had to be moved so that both classes occur.
  F21_lkm34_gcn5_grads      the two first-layer weight gradients of gcn5 (2 x 96 768 values) of that same step: a file of their own,
                            so that every file stays under 1 MiB

The generator REFUSES to write unless the reference alone meets the guards the tests re-assert (the rule set of make_golden_psp.py): at
most 0.1 % of the pixels with |logit[1]| < 10 x its own f32-vs-f64 error; both classes in the eval masks; 20 .. 80 % of every ReLU's
inputs pass in the new blocks (eval and train); its f32-vs-f64 gradient-norm figures within a quarter of the GPU test's bounds (1e-2
relative for tensors of 16 elements and more, 1e-6 of the largest norm under 16); the f32-vs-f64 element error of every full gradient
within a quarter of the GPU test's 2e-2; the Adam step stable under fp32-sized input noise to a quarter of the post-step bounds (see
network_fixture: 21-element tensors leave no room for one gradient element that rounding can carry across zero)."""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: lkm_oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root: oracle

torch.manual_seed(0)
torch.set_num_threads(8)

CONFIG = dict(encoder_depth=34, num_classes=2, kernel_size=9, internal_channels=21, use_relu=True, pretrained=False, dropout_2d=0.0, pool0=False)
BIG = ['gcn5.conv1.0.conv.weight', 'gcn5.conv2.0.conv.weight']      # 96 768 values each: F21_lkm34_gcn5_grads
# The tensors whose gradient is recorded IN FULL: the head, the first layers of gcn5 (the paired weight gradients at the 4x4 map where every
# vertical tap is clamped), their BatchNorms, the thin first layers of gcn2, and the last encoder BatchNorm, whose gradient has passed
# through the paired data gradient
FULL_REQUIRED = (['final.weight', 'final.bias'] + BIG
                 + ['gcn5.conv%d.0.batch_norm.%s' % (b, leaf) for b in (1, 2) for leaf in ('weight', 'bias')]
                 + ['gcn2.conv1.0.conv.weight', 'gcn2.conv2.0.conv.weight', 'enc_br5.conv.1.batch_norm.weight', 'dec_br1.conv.1.batch_norm.weight',
                    'deconv2.batch_norm.weight', 'encoders.encoder.layer4.2.bn2.weight', 'encoders.encoder.layer4.2.bn2.bias'])


def relu_fractions(mod, run, prefixes=None):
    """pass fraction of every ReLU that runs during ``run()`` in the sub-modules whose name starts with one of ``prefixes`` (all if None),
    in call order"""
    fr, hooks = [], []
    for name, m in mod.named_modules():
        if isinstance(m, torch.nn.ReLU) and (prefixes is None or name.startswith(prefixes)):
            hooks.append(m.register_forward_hook(lambda mm, a, out: fr.append(float((out > 0).double().mean()))))
    try:
        run()
    finally:
        for h in hooks:
            h.remove()
    return fr


def block_fixture(name, make, tag, shape, modes=(True, False)):
    """make_golden.block_fixture without weights: expected output, gradients and (train) the running statistics AFTER the pass; the tests
    rebuild x = closed_form.input_for(tag, shape), gy and the weights from the closed form."""
    import closed_form as CF
    from make_golden import run_block, save
    x = CF.input_for(tag, shape)
    for train in modes:
        mod = make()
        CF.fill_module(mod)
        res = {}
        fr = relu_fractions(mod, lambda: res.update(run_block(mod, x, train)))
        assert all(0.2 <= f <= 0.8 for f in fr), (name, train, fr)
        keep = OrderedDict((k, v) for k, v in res.items() if k in ('y', 'gx') or k.startswith('g:')
                           or (train and k.startswith('s:') and k.endswith(('running_mean', 'running_var'))))
        keep['x_shape'], keep['input_tag'], keep['fractions'] = np.array(shape), np.array(tag), np.array(fr, dtype=np.float64)
        # the reference's own f32-vs-f64 error of the output: the tests' 5e-5 must be at least four times that
        m64 = copy.deepcopy(mod).double()
        m64.train(train)
        with torch.no_grad():
            y64 = m64(x.double())
        keep['ref_f32_vs_f64'] = float((res['y'].detach().double() - y64).abs().max() / y64.abs().max())
        assert keep['ref_f32_vs_f64'] <= 5e-5 / 4, (name, keep['ref_f32_vs_f64'])
        print('  %s %s: relu pass fractions %s  f32 vs f64 %.2e' % (name, 'train' if train else 'eval', ['%.2f' % f for f in fr], keep['ref_f32_vs_f64']))
        save('%s_%s' % (name, 'train' if train else 'eval'), **keep)


NEW_BLOCKS = ('gcn', 'enc_br', 'dec_br', 'deconv')


def network_fixture(lkm, models, name):
    import closed_form as CF
    import lkm_oracle as LO
    from oracle import blocks as OB
    from make_golden import canonical_fn, save
    from make_golden_emptiness import lovasz_loss_any_dtype, grad_norms
    shape = (2, 3, 64, 64)

    def build():
        net = lkm.LargeKernelMatters(**CONFIG)
        canon = canonical_fn(net)
        CF.fill_module(net, canonical=canon)
        return net, canon

    refused = []          # (input tag, why): recorded in the fixture, so that the data the GPU test is judged on shows how it was chosen
    for tag in ['f21'] + ['f21:%d' % i for i in range(1, 16)]:
        X = CF.input_for(tag, shape)
        net, canon = build()
        net.eval()
        with torch.no_grad():
            pos0 = float((net(X)[:, 1] > 0).float().mean())
            if not 0.2 <= pos0 <= 0.8:
                # the remedy of F20: the head's bias for class 1 is moved to minus the median of logit[1] at this input (one decimal), which
                # splits the mask in half; the tests read the two bias values from the fixture, every other weight stays closed-form
                net.final.bias.data[1] = round(float(net.final.bias.data[1] - net(X)[:, 1].median()), 1)
            fr_eval = relu_fractions(net, lambda: net(X), NEW_BLOCKS)
            logits = net(X)
            logits64 = copy.deepcopy(net).double()(X.double())
        err = float((logits.double() - logits64).abs().max())
        margin = int((logits[:, 1].abs() < 10 * err).sum())
        pos = float((logits[:, 1] > 0).float().mean())
        print('  %s: input %s  relu pass %.2f .. %.2f (%d)  f32 vs f64 %.2e  pixels under 10x %d of %d  positive %.3f' % (
            name, tag, min(fr_eval), max(fr_eval), len(fr_eval), err, margin, logits[:, 1].numel(), pos))
        if margin > 0.001 * logits[:, 1].numel() or not (0.0 < pos < 1.0) or not all(0.2 <= f <= 0.8 for f in fr_eval):
            refused.append((tag, 'eval guards: %d pixels under the margin, positive fraction %.3f, relu pass %.2f .. %.2f' % (margin, pos, min(fr_eval), max(fr_eval))))
            continue
        out = OrderedDict(x_shape=np.array(X.shape), x=X, input_tag=np.array(tag), fractions_eval=np.array(fr_eval), eval_logits=logits,
                          ref_f32_vs_f64_maxabs=err, margin_pixels=margin, eval_positive_fraction=pos)
        out['final_bias'] = net.final.bias.data.clone()
        out['keys'] = np.array(list(net.state_dict().keys()))
        out['key_shapes'] = np.array(['x'.join(str(d) for d in v.shape) for v in net.state_dict().values()])
        sd = {k: v.clone() for k, v in net.state_dict().items() if canon(k) == k}
        with torch.no_grad():
            o32 = LO.lkm(sd, X, False)
            with OB.bf16_storage():
                o16 = LO.lkm(sd, X, False)
        assert float((o32 - logits).abs().max()) <= 1e-3 * float(logits.abs().max()), 'test-side oracle does not reproduce the reference'
        out['ref_bf16_storage_vs_f32_maxabs'] = float((o16.double() - o32.double()).abs().max())
        T = CF.mask_for('f21', (2, 64, 64))
        out['t'] = T
        net.train()
        n64 = copy.deepcopy(net).double()
        fr_train = relu_fractions(n64, lambda: lovasz_loss_any_dtype(n64(X.double()), T.double()).backward(), NEW_BLOCKS)
        g64 = grad_norms(n64)
        full64 = {k: p.grad.clone() for k, p in n64.named_parameters() if k in FULL_REQUIRED}
        del n64
        if not all(0.2 <= f <= 0.8 for f in fr_train):
            print('  %s: input %s refused: train-mode fractions %s' % (name, tag, fr_train))
            refused.append((tag, 'train-mode relu pass fractions %.2f .. %.2f' % (min(fr_train), max(fr_train))))
            continue
        out['fractions_train'] = np.array(fr_train)
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
        numel = {k: p.numel() for k, p in net.named_parameters()}
        gmax = max(g64.values())
        out['ref_f32_vs_f64_gradnorm_rel'] = max(abs(g32[k] - g64[k]) / g64[k] for k in g64 if g64[k] > 1e-4 and numel[k] >= 16)
        out['ref_f32_vs_f64_small_abs'] = max(abs(g32[k] - g64[k]) / gmax for k in g64 if numel[k] < 16)
        if not (out['ref_f32_vs_f64_gradnorm_rel'] <= 2.5e-3 and out['ref_f32_vs_f64_small_abs'] <= 2.5e-7):
            print('  %s: input %s refused: gradient norms f32 vs f64 %.2e (>= 16 elements), %.2e of the largest norm (< 16)' % (
                name, tag, out['ref_f32_vs_f64_gradnorm_rel'], out['ref_f32_vs_f64_small_abs']))
            refused.append((tag, 'gradient norms f32 vs f64 %.2e / %.2e' % (out['ref_f32_vs_f64_gradnorm_rel'], out['ref_f32_vs_f64_small_abs'])))
            continue
        names, gnorm, gsum, has_grad = [], [], [], []
        for k, p in net.named_parameters():
            names.append(k)
            has_grad.append(p.grad is not None)
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            gnorm.append(float(g.double().norm()))
            gsum.append(float(g.double().sum()))
        named = dict(net.named_parameters())
        errs = {k: float((named[k].grad.double() - full64[k]).abs().max() / full64[k].abs().max()) for k in FULL_REQUIRED}
        print('  full gradients (own f32 vs f64):', {k: '%.1e' % v for k, v in errs.items()})
        if max(errs.values()) > 5e-3:
            print('  %s: input %s refused: a required full gradient is ill-conditioned in the reference itself' % (name, tag))
            refused.append((tag, 'a full gradient f32 vs f64 at %.2e' % max(errs.values())))
            continue
        # The Adam step divides every gradient element by its own magnitude: an element that fp32 rounding alone can carry across zero moves
        # its parameter by 2 lr, which is more than the post-step bound of a 21-element tensor allows.  Such an input cannot be reproduced
        # by ANY fp32 implementation with another summation order, so it is refused here, on the reference alone: the same step on the
        # input scaled by (1 + 2e-6 noise) - the size of the reference's own f32-vs-f64 logit error - must leave every tensor's post-step
        # norm and sum within a quarter of the GPU test's 1e-4 bounds (net_checks.check_after_adam's formula).
        def post_step(net_, X_):
            n_ = copy.deepcopy(net_)
            o_ = torch.optim.Adam([{'params': [p for p in n_.parameters() if p.requires_grad], 'weight_decay': 1e-4}], lr=1e-4)
            o_.zero_grad()
            (models.lovasz_loss(n_(X_), T) * 1.0).backward()
            o_.step()
            return [(float(p.detach().double().norm()), float(p.detach().double().sum()), p.numel()) for _, p in n_.named_parameters()]
        noise = torch.randn(X.shape, generator=torch.Generator().manual_seed(21))
        base, moved = post_step(net, X), post_step(net, X * (1 + 2e-6 * noise))
        worst = max(max(abs(a[0] - b[0]) / max(a[0], 1e-3), abs(a[1] - b[1]) / max(a[0] * a[2] ** 0.5, 1e-3)) for a, b in zip(base, moved))
        out['ref_post_step_stability'] = worst
        if worst > 0.25e-4:
            print('  %s: input %s refused: the Adam step is not stable under fp32-sized input noise (%.2e of a 1e-4 bound)' % (name, tag, worst))
            refused.append((tag, 'Adam step under (1 + 2e-6 noise) input: post-step norm / sum moved by %.2e of a 1e-4 bound (allowed 0.25e-4)' % worst))
            continue
        big = OrderedDict()
        for k in FULL_REQUIRED:
            (big if k in BIG else out)['fullgrad:' + k] = named[k].grad.clone()
        out['fullgrad_keys'] = np.array(FULL_REQUIRED)
        out['fullgrad_ref_f32_vs_f64'] = np.array([errs[k] for k in FULL_REQUIRED])
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
        out['refused_tags'] = np.array([t for t, _ in refused], dtype=str)
        out['refused_why'] = np.array([w for _, w in refused], dtype=str)
        save(name, **out)
        save(name + '_gcn5_grads', **big)
        print('  %s: max|logit| %.2f  bf16 storage %.2e  loss %.5f  grad-norm f32 vs f64 %.2e (small tensors %.2e of the largest norm)  live tensors %d' % (
            name, float(logits.abs().max()), out['ref_bf16_storage_vs_f32_maxabs'], float(loss.detach()), out['ref_f32_vs_f64_gradnorm_rel'],
            out['ref_f32_vs_f64_small_abs'], sum(has_grad)))
        return
    raise AssertionError('%s: no input keeps the guards' % name)


def main():
    import ref_import as R
    R.install_stubs()
    assert R.reference_available(), 'reference not mounted'
    base = R.load('architectures.base')
    lkm = R.load('architectures.large_kernel_matters')
    models = R.load_models_module()
    from make_golden import ONLY
    want = lambda name: not ONLY or any(o.startswith(name) for o in ONLY)
    if want('F21_gcn'):
        block_fixture('F21_gcn', lambda: base.GlobalConvolutionalNetwork(64, 21, 9, use_relu=True), 'f21a', (2, 64, 6, 10))
        block_fixture('F21_gcn_norelu', lambda: base.GlobalConvolutionalNetwork(64, 21, 9), 'f21a', (2, 64, 6, 10), modes=(True,))
    if want('F21_br'):
        block_fixture('F21_br', lambda: base.BoundaryRefinement(21, 21, 3), 'f21b', (2, 21, 5, 7))
    if want('F21_lkm34'):
        network_fixture(lkm, models, 'F21_lkm34')


if __name__ == '__main__':
    main()
