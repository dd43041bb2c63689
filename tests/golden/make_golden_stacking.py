#!/usr/bin/env python
"""Generate the F16 fixtures (second-level / stacking networks) by EXECUTING THE REFERENCE'S OWN MODULES.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_stacking.py
Same conventions as make_golden_depth.py / make_golden_emptiness.py: closed-form weights keyed by state-dict name (closed_form.py), the
reference's sources imported through the stubs of ref_import.py, only .npz data is written.

  F16_stacking_fcn          misc.StackingFCN(5, 2, 32) on [2,5,19,37]: eval logits plus one training step as SegmentationModel._fit_loop
                            runs it (lovasz_loss, Adam lr 1e-4 + L2 1e-4).  The network is tiny, so EVERY parameter's full gradient
                            ('fullgrad:<key>'), its value after the step ('post:<key>') and the BatchNorm running statistics after the
                            step ('bn:<key>') are stored, and 'train_dy', the gradient that reached the raw convolution output
  F16_stacking_fcn_depth    misc.StackingFCNWithDepth, the same with D = [[0.2], [0.6]]
  F16_stacking_fcn_m32      misc.StackingFCN(32, 2, 32) (the registry's model_config) on [2,32,32,32]

The stacked maps are probabilities: x = sigmoid(1.5 * CF.input_for(tag, shape)).  Every fixture records, like F15:
  ref_f32_vs_f64_maxabs              largest deviation of the fp32 eval logits from the same module run in float64
  ref_f32_vs_f64_gradnorm_rel        worst per-tensor relative deviation of the fp32 gradient norms from the float64 run's (the float64 leg
                                     uses the dtype-generic lovasz restatement of tests/stacking_oracle.py: the reference's does not run
                                     in double), over the tensors whose exact gradient is not zero ('zero_grad_names' lists the others)
  wgrad_f64_from_train_dy            the reference's ReplicationPad2d + Conv2d run in float64 on x with 'train_dy' as the upstream gradient:
                                     the weight gradient free of fp32 summation error; ref_wgrad_f32_vs_f64_maxrel is the distance of the
                                     module's fp32 gradient from it, relative to its largest element
  ref_bf16_storage_vs_f32_maxabs     eval logits of tests/stacking_oracle.py with bf16 storage against the same oracle in fp32
  near_zero_share / near_zero_thr    share of pixels with |logit[1]| < 1e-3 max|logit| (asserted <= 0.1 % here): the only pixels a
                                     mask-equality check may leave out
"""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: stacking_oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root
import closed_form as CF          # noqa: E402
import ref_import as R            # noqa: E402
from make_golden import save          # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def stack_input(tag, shape):
    return torch.sigmoid(1.5 * CF.input_for(tag, shape))


def grad_norms(net):
    return OrderedDict((k, float(p.grad.double().norm())) for k, p in net.named_parameters())


def fixture(misc, models, name, tag, M, H, W, with_depth):
    import stacking_oracle as SO
    X = stack_input(tag, (2, M, H, W))
    T = CF.mask_for(tag, (2, H, W))
    D = torch.tensor([[0.2], [0.6]]) if with_depth else None
    net = (misc.StackingFCNWithDepth if with_depth else misc.StackingFCN)(M, 2, filter_nr=32, dropout_2d=0.0)
    CF.fill_module(net)
    args = (X, D) if with_depth else (X,)
    args64 = tuple(a.double() for a in args)
    net.eval()
    with torch.no_grad():
        logits = net(*args)
        logits64 = copy.deepcopy(net).double()(*args64)
    out = OrderedDict(x=X, t=T, eval_logits=logits)
    if with_depth:
        out['d'] = D
    out['keys'] = np.array(list(net.state_dict().keys()))
    out['ref_f32_vs_f64_maxabs'] = float((logits.double() - logits64).abs().max())
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        o32 = SO.stacking_fcn(sd, X, False, d=D)
        o16 = SO.stacking_fcn(sd, X, False, d=D, bf16=True)
    assert float((o32 - logits).abs().max()) <= 1e-4 * float(logits.abs().max()), 'test-side oracle does not reproduce the reference'
    out['ref_bf16_storage_vs_f32_maxabs'] = float((o16.double() - o32.double()).abs().max())
    thr = 1e-3 * float(logits.abs().max())
    share = float((logits[:, 1].abs() < thr).float().mean())
    assert share <= 1e-3, '%s: %.3f %% of the pixels are near-zero logits: pick another input tag' % (name, 100 * share)
    out['near_zero_thr'], out['near_zero_share'] = thr, share
    # float64 leg of the training step first (a deep copy: the fp32 module below starts from the same state)
    net.train()
    n64 = copy.deepcopy(net).double()
    SO.lovasz_loss(n64(*args64), T.double()).backward()
    g64 = grad_norms(n64)
    # one training step exactly as SegmentationModel._fit_loop / SegmentationModelWithDepth._fit_loop (models.py:105-136, 222-253)
    params = [p for p in net.parameters() if p.requires_grad]
    opt = torch.optim.Adam([{'params': params, 'weight_decay': 1e-4}], lr=1e-4)
    opt.zero_grad()
    raw = []

    def keep_raw(mod, inp, res):
        res.retain_grad()
        raw.append(res)
    hook = net.conv[0].conv.register_forward_hook(keep_raw)
    o = net(*args)
    hook.remove()
    loss = models.lovasz_loss(o, T) * 1.0
    loss.backward()
    out['train_logits'], out['train_loss'] = o, loss
    out['train_dy'] = raw[0].grad.clone()       # dL/d(raw convolution output): what the weight gradient contracts with the input
    assert abs(float(SO.lovasz_loss(o.detach(), T)) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach())), 'lovasz restatement'
    # the same contraction by the reference's own padding + convolution modules in float64: torch's fp32 weight gradient sums 2 H W
    # cancelling terms per element (dL/dy behind a BatchNorm sums to zero) and is itself off by several 1e-6 of its maximum
    c64 = copy.deepcopy(net.conv[0]).double()
    c64.zero_grad()
    c64.conv(c64.padding(X.double())).backward(out['train_dy'].double())
    out['wgrad_f64_from_train_dy'] = c64.conv.weight.grad.clone()
    gw32 = net.conv[0].conv.weight.grad.double()
    out['ref_wgrad_f32_vs_f64_maxrel'] = float((gw32 - c64.conv.weight.grad).abs().max() / c64.conv.weight.grad.abs().max())
    g32 = grad_norms(net)
    # conv.0.conv.bias feeds a train-mode BatchNorm: its gradient is zero in exact arithmetic (1e-17 in float64, rounding noise in fp32) and
    # has no relative error; such tensors are listed in 'zero_grad_names' and only bounded in absolute terms by the tests
    live = [k for k in g64 if g64[k] > 1e-9 * max(g64.values())]
    out['zero_grad_names'] = np.array([k for k in g64 if k not in live])
    assert out['zero_grad_names'].tolist() == ['conv.0.conv.bias']
    out['ref_f32_vs_f64_gradnorm_rel'] = max(abs(g32[k] - g64[k]) / g64[k] for k in live)
    out['param_names'] = np.array([k for k, _ in net.named_parameters()])
    for k, p in net.named_parameters():
        out['fullgrad:' + k] = p.grad.clone()
    opt.step()
    for k, p in net.named_parameters():
        out['post:' + k] = p.detach().clone()
    for k, v in net.state_dict().items():
        if k.endswith('running_mean') or k.endswith('running_var'):
            out['bn:' + k] = v.clone()
    save(name, **out)
    print('  %s: max|logit| %.2f  near-zero share %.4f %%  f32 vs f64 %.2e  bf16 storage %.2e  grad-norm f32 vs f64 %.2e  loss %.6f' % (
        name, float(logits.abs().max()), 100 * share, out['ref_f32_vs_f64_maxabs'], out['ref_bf16_storage_vs_f32_maxabs'],
        out['ref_f32_vs_f64_gradnorm_rel'], float(loss)))


def main():
    assert R.reference_available(), 'reference not mounted'
    misc = R.load('architectures.misc')
    models = R.load_models_module()
    fixture(misc, models, 'F16_stacking_fcn', 'f16', 5, 19, 37, False)
    fixture(misc, models, 'F16_stacking_fcn_depth', 'f16', 5, 19, 37, True)
    fixture(misc, models, 'F16_stacking_fcn_m32', 'f16m32', 32, 32, 32, False)


if __name__ == '__main__':
    main()
