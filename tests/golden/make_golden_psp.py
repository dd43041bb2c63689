#!/usr/bin/env python
"""Generate the F20 fixtures (PSPNet) by EXECUTING THE REFERENCE'S OWN architectures/pspnet.py.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_psp.py

  F20_psp_module_{train,eval}    pspnet.PSPModule(64, 128) on [2,64,8,8]: output, input gradient, every parameter gradient (the
                                 bottleneck's bias gradient among them) and the pass fraction of the bottleneck ReLU
  F20_psp_upsample_{train,eval}  pspnet.PSPUpsample(32, 16) on [2,32,5,7] with the PReLU slope set to ALPHA (not 0, 1 or torch's 0.25):
                                 output, gradients (the slope's among them), the running statistics after the pass, the fraction of
                                 negative PReLU inputs
  F20_pspnet34_hyper             pspnet.PSPNet(34, 2, use_hypercolumn=True, dropout_2d=0.0) at [2,3,64,64] - encoder5 is 4x4, so the s = 6
                                 stage has repeated bins - with closed-form weights: eval logits plus one training step as
                                 SegmentationModel._fit_loop runs it, in the F19 layout.  No weights are stored, except the two values
                                 of final.1.bias: the class-1 bias is moved so that both classes occur (see network_fixture).

dropout_2d: the class default is 0.2 and the registry does not override it; under the torch the reference pins F.dropout2d is an identity
(training=False by default), under a modern torch it would drop channels at random - the generator builds the network with 0.0.

The generator REFUSES to write unless the reference alone meets the guards the tests re-assert: at most 0.1 % of the pixels with
|logit[1]| < 10 x its own f32-vs-f64 error; both classes in the eval masks; 20 .. 80 % of the bottleneck ReLU passes and 20 .. 80 % of
every PReLU's inputs are negative (eval and train); its f32-vs-f64 gradient-norm figures within a quarter of the GPU test's bounds (1e-2
relative for tensors of 16 elements and more, 1e-6 of the largest norm under 16).  Full gradients are recorded for FULL_REQUIRED; an
input at which the reference's own f32-vs-f64 element error of any of them exceeds a quarter of the GPU test's 2e-2 is refused."""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: psp_oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root: oracle

torch.manual_seed(0)
torch.set_num_threads(8)

ALPHA = 0.4
UPS = ('up4', 'up3', 'up2', 'up1')
# The tensors whose gradient is recorded IN FULL (each at most 33 000 elements, the file stays under 1 MiB): the head, the bottleneck's
# bias (its gradient comes out of the merge's adjoint), BatchNorm and PReLU of every PSPUpsample, and the last encoder BatchNorm, whose
# gradient has passed through the pooling adjoint and the data gradient of the feats block together.
FULL_REQUIRED = (['final.1.weight', 'final.1.bias', 'psp.bottleneck.bias'] + ['%s.conv.%s' % (u, leaf) for u in UPS for leaf in ('1.weight', '1.bias', '2.weight')]
                 + ['encoders.encoder.layer4.2.bn2.weight', 'encoders.encoder.layer4.2.bn2.bias'])


def fractions(net, run):
    """[pass fraction of the bottleneck ReLU, negative fraction of the PReLU inputs of up4, up3, up2, up1] during ``run()``"""
    fr, hooks = {}, []
    hooks.append(net.psp.relu.register_forward_hook(lambda m, a, out: fr.__setitem__('psp', float((out > 0).double().mean()))))
    for u in UPS:
        hooks.append(getattr(net, u).conv[2].register_forward_hook(lambda m, a, out, u=u: fr.__setitem__(u, float((a[0] < 0).double().mean()))))
    try:
        run()
    finally:
        for h in hooks:
            h.remove()
    return [fr[k] for k in ('psp',) + UPS]


def network_fixture(pspnet, models, name):
    import closed_form as CF
    import psp_oracle as PO
    from oracle import blocks as OB
    from make_golden import canonical_fn, save
    from make_golden_emptiness import lovasz_loss_any_dtype, grad_norms
    shape = (2, 3, 64, 64)

    def build():
        net = pspnet.PSPNet(encoder_depth=34, num_classes=2, dropout_2d=0.0, pretrained=False, use_hypercolumn=True, pool0=False)
        canon = canonical_fn(net)
        CF.fill_module(net, canonical=canon)
        return net, canon

    for tag in ['f20'] + ['f20:%d' % i for i in range(1, 16)]:
        X = CF.input_for(tag, shape)
        net, canon = build()
        net.eval()
        with torch.no_grad():
            # With the plain closed-form fill every eval pixel lands in class 0 at all 16 inputs (logit[1] between -630 and -20: the
            # PReLU slopes come out near 1 and nothing bounds the activations).  The remedy: the head's bias for class 1 is moved to
            # minus the median of logit[1] at this input (one decimal), which splits the mask in half; the tests read the two bias
            # values from the fixture ('final_1_bias'), every other weight stays closed-form.
            net.final[1].bias.data[1] = round(float(net.final[1].bias.data[1] - net(X)[:, 1].median()), 1)
            fr_eval = fractions(net, lambda: net(X))
            logits = net(X)
            logits64 = copy.deepcopy(net).double()(X.double())
        err = float((logits.double() - logits64).abs().max())
        margin = int((logits[:, 1].abs() < 10 * err).sum())
        pos = float((logits[:, 1] > 0).float().mean())
        print('  %s: input %s  relu pass / prelu negative %s  f32 vs f64 %.2e  pixels under 10x %d of %d  positive %.3f' % (
            name, tag, ['%.2f' % f for f in fr_eval], err, margin, logits[:, 1].numel(), pos))
        if margin > 0.001 * logits[:, 1].numel() or not (0.0 < pos < 1.0) or not all(0.2 <= f <= 0.8 for f in fr_eval):
            continue
        out = OrderedDict(x_shape=np.array(X.shape), x=X, input_tag=np.array(tag), fractions_eval=np.array(fr_eval), eval_logits=logits,
                          ref_f32_vs_f64_maxabs=err, margin_pixels=margin, eval_positive_fraction=pos)
        out['final_1_bias'] = net.final[1].bias.data.clone()
        out['keys'] = np.array(list(net.state_dict().keys()))
        out['key_shapes'] = np.array(['x'.join(str(d) for d in v.shape) for v in net.state_dict().values()])
        sd = {k: v.clone() for k, v in net.state_dict().items() if canon(k) == k}
        with torch.no_grad():
            o32 = PO.pspnet(sd, X, False)
            with OB.bf16_storage():
                o16 = PO.pspnet(sd, X, False)
        assert float((o32 - logits).abs().max()) <= 1e-3 * float(logits.abs().max()), 'test-side oracle does not reproduce the reference'
        out['ref_bf16_storage_vs_f32_maxabs'] = float((o16.double() - o32.double()).abs().max())
        T = CF.mask_for('f20', (2, 64, 64))
        out['t'] = T
        net.train()
        n64 = copy.deepcopy(net).double()
        fr_train = fractions(n64, lambda: lovasz_loss_any_dtype(n64(X.double()), T.double()).backward())
        g64 = grad_norms(n64)
        full64 = {k: p.grad.clone() for k, p in n64.named_parameters() if k in FULL_REQUIRED}
        del n64
        if not all(0.2 <= f <= 0.8 for f in fr_train):
            print('  %s: input %s refused: train-mode fractions %s' % (name, tag, fr_train))
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
            continue
        for k in FULL_REQUIRED:
            out['fullgrad:' + k] = named[k].grad.clone()
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
        save(name, **out)
        print('  %s: max|logit| %.2f  bf16 storage %.2e  loss %.5f  grad-norm f32 vs f64 %.2e (small tensors %.2e of the largest norm)  live tensors %d' % (
            name, float(logits.abs().max()), out['ref_bf16_storage_vs_f32_maxabs'], float(loss.detach()), out['ref_f32_vs_f64_gradnorm_rel'],
            out['ref_f32_vs_f64_small_abs'], sum(has_grad)))
        return
    raise AssertionError('%s: no input keeps the guards' % name)


def block_fixture(name, make, tag, shape, fraction, alpha=None):
    """make_golden.block_fixture without weights: expected output, gradients and (train) the running statistics AFTER the pass; the
    tests rebuild x = closed_form.input_for(tag, shape), gy and the weights from the closed form (and set the slope to ``alpha``).
    ``fraction(mod, run)`` -> the guarded fraction, which must lie in 20 .. 80 %."""
    import closed_form as CF
    from make_golden import run_block, save
    x = CF.input_for(tag, shape)
    for train in (True, False):
        mod = make()
        CF.fill_module(mod)
        if alpha is not None:
            mod.conv[2].weight.data.fill_(alpha)
        res = {}
        fr = fraction(mod, lambda: res.update(run_block(mod, x, train)))
        assert 0.2 <= fr <= 0.8, (name, train, fr)
        keep = OrderedDict((k, v) for k, v in res.items() if k in ('y', 'gx') or k.startswith('g:')
                           or (train and k.startswith('s:') and k.endswith(('running_mean', 'running_var'))))
        keep['x_shape'], keep['input_tag'], keep['fraction'] = np.array(shape), np.array(tag), fr
        if alpha is not None:
            keep['alpha'] = alpha
        # the reference's own f32-vs-f64 error of the output: the tests' 5e-5 must be at least four times that
        m64 = copy.deepcopy(mod).double()
        m64.train(train)
        with torch.no_grad():
            y64 = m64(x.double())
        keep['ref_f32_vs_f64'] = float((res['y'].detach().double() - y64).abs().max() / y64.abs().max())
        assert keep['ref_f32_vs_f64'] <= 5e-5 / 4, (name, keep['ref_f32_vs_f64'])
        save('%s_%s' % (name, 'train' if train else 'eval'), **keep)


def _hooked(get_module, value):
    def fraction(mod, run):
        got = []
        h = get_module(mod).register_forward_hook(lambda m, a, out: got.append(value(a, out)))
        try:
            run()
        finally:
            h.remove()
        return got[0]
    return fraction


def main():
    import ref_import as R
    R.install_stubs()
    assert R.reference_available(), 'reference not mounted'
    pspnet = R.load('architectures.pspnet')
    models = R.load_models_module()
    from make_golden import ONLY
    want = lambda name: not ONLY or any(o.startswith(name) for o in ONLY)
    if want('F20_psp_module'):
        block_fixture('F20_psp_module', lambda: pspnet.PSPModule(64, 128), 'f20a', (2, 64, 8, 8),
                      _hooked(lambda m: m.relu, lambda a, out: float((out > 0).double().mean())))
    if want('F20_psp_upsample'):
        block_fixture('F20_psp_upsample', lambda: pspnet.PSPUpsample(32, 16), 'f20b', (2, 32, 5, 7),
                      _hooked(lambda m: m.conv[2], lambda a, out: float((a[0] < 0).double().mean())), alpha=ALPHA)
    if want('F20_pspnet34_hyper'):
        network_fixture(pspnet, models, 'F20_pspnet34_hyper')


if __name__ == '__main__':
    main()
