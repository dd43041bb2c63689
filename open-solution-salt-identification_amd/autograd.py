"""torch.autograd bridge: lets reference-style code (``out = model(X); loss = fn(out, t); loss.backward()``,
models.py:121-134) drive the compiled HIP programs.  The fused path in models.SegmentationModel._fit_loop
does not go through autograd at all; this exists so that the nn.Module surface stays a drop-in."""
import torch

from ._abi import SaltError


class HipNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, d, *params):
        eng = module.engine(x.device)
        net = eng.forward(x, True, d=d)          # d: the depth input of a depth-conditioned network (no gradient), else None
        ctx.net, ctx.eng = net, eng
        return net.logits.clone()

    @staticmethod
    def backward(ctx, dlogits):
        net, eng = ctx.net, ctx.eng
        if net.dlogits is None:
            raise SaltError('network was compiled without a backward program')
        net.dlogits.copy_(dlogits)
        net.bwd.run(side=eng.side_stream)
        grads = []
        for p in eng.live_params:
            off, n = eng.grad_range(p)
            view = eng.grads[off:off + n].view(p.shape)
            # gradients are already in place when p.grad still aliases the flat gradient buffer
            grads.append(None if (p.grad is not None and p.grad.data_ptr() == view.data_ptr()) else view.clone())
        return (None, None, None) + tuple(grads)


class _NativeLoss(torch.autograd.Function):
    """Hand-written HIP loss kernels as differentiable torch functions of fp32 NCHW logits."""

    @staticmethod
    def forward(ctx, logits, target, kind, *weights):
        """``weights``: nothing, or the (dice_weight, cross_entropy_weight, smooth) tuple of 'dice_ce' / the lovasz_params tuple of
        'lovasz' and 'lovasz_softmax'"""
        from . import losses
        names = losses.LOVASZ_DEFAULTS.get(kind, losses.DICE_CE_DEFAULTS)
        params = dict(zip(names, weights[0])) if weights else None
        loss, dl = losses.native_loss(logits.detach(), target, kind, want_grad=True, params=params)
        ctx.save_for_backward(dl)
        ctx.n_inputs = 3 + len(weights)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl * g,) + (None,) * (ctx.n_inputs - 1)
