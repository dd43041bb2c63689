"""Loss functions of the reference's training loop as hand-written HIP kernels.

  lovasz_loss          <- models.py:326-328  (lovasz_losses.py:81-115, per-image, F.elu variant)
  mixed_dice_bce_loss  <- models.py:331-340  (defaults dice 0.2 / bce 0.9, sigmoid dice, batch-wide sums)
  lovasz_softmax_loss  <- lovasz_losses.py:173-210 (per image, all classes) on softmax(logits); 2 .. 4 channels
  mixed_dice_cross_entropy_loss <- models.py:343-388 (defaults dice 0.5 / cross entropy 0.5; target WITH its background channel)

All accept what the reference passes (fp32 logits [B,C,H,W], float one-hot target [B,C,H,W]) and return
a differentiable 0-dim tensor.  They run only on GPU tensors; there is no CPU fallback."""
import ctypes

import torch

from ._abi import CONSTS, SaltError, STRUCTS, fill, lib, check

_ws = {}


def _workspace(key, n, dtype, device):
    t = _ws.get(key)
    if t is None or t.numel() < n or t.device != device:
        t = torch.empty(n, dtype=dtype, device=device)
        _ws[key] = t
    return t


DICE_CE_DEFAULTS = {'dice_weight': 0.5, 'cross_entropy_weight': 0.5, 'smooth': 0.0}       # models.py:343


def dice_ce_params(params):
    """(dice_weight, cross_entropy_weight, smooth) of a 'dice_ce' loss from a dict that may name any of them (None: the defaults)"""
    params = dict(params or {})
    unknown = set(params) - set(DICE_CE_DEFAULTS)
    if unknown:
        raise SaltError('dice_ce: unknown loss parameter(s) %s (%s)' % (sorted(unknown), ' | '.join(DICE_CE_DEFAULTS)))
    return tuple(float(params.get(k, v)) for k, v in DICE_CE_DEFAULTS.items())


# the options of the two Lovasz losses, in the order lovasz_params returns them (this project's defaults: per image, every class)
LOVASZ_DEFAULTS = {'lovasz': {'per_image': True, 'ignore': None},
                   'lovasz_softmax': {'only_present': False, 'per_image': True, 'ignore': None}}


def lovasz_params(kind, params):
    """The options of a 'lovasz' -> (per_image, ignore) or 'lovasz_softmax' -> (only_present, per_image, ignore) loss from a dict that
    may name any of them (None: the defaults).  ``ignore`` is None or the void value of the target, a real number."""
    if kind not in LOVASZ_DEFAULTS:
        raise SaltError('lovasz_params: kind %r (%s)' % (kind, ' | '.join(LOVASZ_DEFAULTS)))
    defaults = LOVASZ_DEFAULTS[kind]
    params = dict(params or {})
    unknown = set(params) - set(defaults)
    if unknown:
        raise SaltError('%s: unknown loss parameter(s) %s (%s)' % (kind, sorted(unknown), ' | '.join(defaults)))
    out = []
    for k, v in defaults.items():
        v = params.get(k, v)
        if k == 'ignore':
            if v is not None:
                if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
                    raise SaltError('%s: ignore must be None or a number that is not NaN, got %r' % (kind, v))
                v = float(v)
        elif not isinstance(v, bool):
            raise SaltError('%s: %s must be True or False, got %r' % (kind, k, v))
        out.append(v)
    return tuple(out)


def lovasz_launch_shape(kind, params, B, C, HW):
    """(flags, ignore, rows, N) of the launch of a Lovasz loss over [B,C,HW]: the sort runs over ``rows`` rows of ``N`` elements, which
    sizes ws_split (rows * salt_lovasz_split_words(N)) and ws_flat (rows * salt_lovasz_flat_words(N))."""
    opts = dict(zip(LOVASZ_DEFAULTS[kind], lovasz_params(kind, params)))
    flat = not opts['per_image']
    flags = ((CONSTS['SALT_LOVASZ_BATCH_FLAT'] if flat else 0) | (CONSTS['SALT_LOVASZ_ONLY_PRESENT'] if opts.get('only_present') else 0)
             | (CONSTS['SALT_LOVASZ_HAS_IGNORE'] if opts['ignore'] is not None else 0))
    if kind == 'lovasz':
        rows, n = (1, B * C * HW) if flat else (B, C * HW)
    else:
        rows, n = (C, B * HW) if flat else (B * C, HW)
    return flags, (opts['ignore'] if opts['ignore'] is not None else 0.0), rows, n


def native_loss(logits, target, kind, want_grad=True, loss_scale=1.0, params=None):
    """``params``: the weights of 'dice_ce' (see dice_ce_params) or the options of 'lovasz' / 'lovasz_softmax' (see lovasz_params);
    'bce_dice' takes none."""
    if logits.device.type != 'cuda':
        raise SaltError('native losses run on the GPU only (got %s)' % logits.device)
    logits = logits.contiguous().float()
    target = target.contiguous().float()
    if target.shape[1] != logits.shape[1]:
        target = target[:, :logits.shape[1]].contiguous()
    B, C, H, W = logits.shape
    dev = logits.device
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if want_grad else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if kind == 'lovasz':
        P = C * H * W
        # sort scratch is cached per (device, stream): kernels of ONE stream run in order, so two losses may share it; losses
        # enqueued on different streams (two models on one device) get their own
        sid = torch.cuda.current_stream().cuda_stream
        wk = _workspace(('k', dev, sid), 2 * B * P, torch.int32, dev)
        wv = _workspace(('v', dev, sid), 2 * B * P, torch.int32, dev)
        lpi = torch.empty(B, dtype=torch.float32, device=dev)
        flags, ignore, rows, n = lovasz_launch_shape(kind, params, B, C, H * W)
        sw = int(lib.salt_lovasz_split_words(n)) if n < 2 ** 31 else 0    # > 0: several workgroups per row (segments of the sort)
        ws = _workspace(('s', dev, sid), rows * sw, torch.int32, dev) if sw else None
        fw = int(lib.salt_lovasz_flat_words(n))                  # > 0: a long row, histograms in global memory
        wf = _workspace(('f', dev, sid), rows * fw, torch.int32, dev) if fw else None
        a = STRUCTS['salt_lovasz_args']()
        fill(a, logits=logits.data_ptr(), target=target.data_ptr(), B=B, P=P, ws_keys=wk.data_ptr(), ws_vals=wv.data_ptr(),
             loss_per_image=lpi.data_ptr(), loss=loss.data_ptr(), dlogits=dl.data_ptr() if want_grad else None, loss_scale=loss_scale,
             ws_split=ws.data_ptr() if ws is not None else None, flags=flags, ignore=ignore, ws_flat=wf.data_ptr() if wf is not None else None)
        check(lib.salt_lovasz_hinge(ctypes.byref(a), st), 'lovasz_hinge')
    elif kind == 'bce_dice':
        a = STRUCTS['salt_bce_dice_args']()
        fill(a, B=B, C=C, HW=H * W)
        nparts = lib.salt_bce_dice_parts(ctypes.byref(a))
        parts = torch.empty(nparts * 4, dtype=torch.float32, device=dev)
        sums = torch.empty(3 * C + 1, dtype=torch.float32, device=dev)
        fill(a, logits=logits.data_ptr(), target=target.data_ptr(), dice_weight=0.2, bce_weight=0.9, partials=parts.data_ptr(), nparts=nparts,
             sums=sums.data_ptr(), loss=loss.data_ptr(), dlogits=dl.data_ptr() if want_grad else None, loss_scale=loss_scale)
        check(lib.salt_bce_dice(ctypes.byref(a), st), 'bce_dice')
    elif kind == 'lovasz_softmax':
        # softmax -> row loss (gradient with respect to the probabilities into a workspace) -> softmax Jacobian into dlogits
        HW = H * W
        sid = torch.cuda.current_stream().cuda_stream
        wk = _workspace(('k', dev, sid), 2 * B * C * HW, torch.int32, dev)
        wv = _workspace(('v', dev, sid), 2 * B * C * HW, torch.int32, dev)
        probas = _workspace(('p', dev, sid), B * C * HW, torch.float32, dev)
        lpr = torch.empty(B * C, dtype=torch.float32, device=dev)
        flags, ignore, rows, n = lovasz_launch_shape(kind, params, B, C, HW)
        sw = int(lib.salt_lovasz_split_words(n)) if n < 2 ** 31 else 0
        ws = _workspace(('s', dev, sid), rows * sw, torch.int32, dev) if sw else None
        fw = int(lib.salt_lovasz_flat_words(n))
        wf = _workspace(('f', dev, sid), rows * fw, torch.int32, dev) if fw else None
        wp = _workspace(('n', dev, sid), B * C, torch.int32, dev)
        a = STRUCTS['salt_softmax_args']()
        fill(a, x=logits.data_ptr(), y=probas.data_ptr(), B=B, C=C, HW=HW)
        check(lib.salt_softmax(ctypes.byref(a), st), 'softmax')
        a = STRUCTS['salt_lovasz_softmax_args']()
        fill(a, probas=probas.data_ptr(), target=target.data_ptr(), B=B, C=C, HW=HW, ws_keys=wk.data_ptr(), ws_vals=wv.data_ptr(),
             loss_per_row=lpr.data_ptr(), loss=loss.data_ptr(), dprobas=dl.data_ptr() if want_grad else None, loss_scale=loss_scale,
             ws_split=ws.data_ptr() if ws is not None else None, flags=flags, ignore=ignore,
             ws_flat=wf.data_ptr() if wf is not None else None, ws_present=wp.data_ptr())
        check(lib.salt_lovasz_softmax(ctypes.byref(a), st), 'lovasz_softmax')
        if want_grad:
            a = STRUCTS['salt_softmax_bwd_args']()
            fill(a, p=probas.data_ptr(), dp=dl.data_ptr(), dz=dl.data_ptr(), B=B, C=C, HW=HW)        # in place: dprobas -> dlogits
            check(lib.salt_softmax_bwd(ctypes.byref(a), st), 'softmax_bwd')
    elif kind == 'dice_ce':
        dw, cw, smooth = dice_ce_params(params)
        a = STRUCTS['salt_dice_ce_args']()
        fill(a, B=B, C=C, HW=H * W)
        nparts = lib.salt_dice_ce_parts(ctypes.byref(a))
        if nparts < 1:
            raise SaltError('dice_ce: %d output channels (the softmax losses take 2 .. 4)' % C)
        parts = torch.empty(nparts * (3 * C + 1), dtype=torch.float32, device=dev)
        sums = torch.empty(3 * C + 1, dtype=torch.float32, device=dev)
        fill(a, logits=logits.data_ptr(), target=target.data_ptr(), dice_weight=dw, cross_entropy_weight=cw, smooth=smooth,
             partials=parts.data_ptr(), nparts=nparts, sums=sums.data_ptr(), loss=loss.data_ptr(),
             dlogits=dl.data_ptr() if want_grad else None, loss_scale=loss_scale)
        check(lib.salt_dice_ce(ctypes.byref(a), st), 'dice_ce')
    else:
        raise SaltError('unknown loss %r' % kind)
    return loss[0], dl


def lovasz_loss(output, target, per_image=True, ignore=None):
    """lovasz_hinge(output, target, per_image, ignore) of lovasz_losses.py:81-115 (F.elu variant) on logits and a {0,1} target of the same
    shape.  ``per_image=False``: one sort over the whole batch.  ``ignore``: a target value that marks void elements, which are left out
    of the loss and get a gradient of exactly 0."""
    from .autograd import _NativeLoss
    opts = lovasz_params('lovasz', {'per_image': per_image, 'ignore': ignore})
    return _NativeLoss.apply(output, target, 'lovasz') if opts == (True, None) else _NativeLoss.apply(output, target, 'lovasz', opts)


def mixed_dice_bce_loss(output, target, dice_weight=0.2, dice_loss=None, bce_weight=0.9, bce_loss=None, smooth=0, dice_activation='sigmoid'):
    if dice_weight != 0.2 or bce_weight != 0.9 or smooth != 0 or dice_activation != 'sigmoid' or dice_loss is not None or bce_loss is not None:
        raise NotImplementedError('only the reference defaults (0.2 dice + 0.9 BCE, sigmoid) have a HIP kernel')
    from .autograd import _NativeLoss
    return _NativeLoss.apply(output, target, 'bce_dice')


def lovasz_softmax_loss(output, target, only_present=False, per_image=True, ignore=None):
    """lovasz_softmax(softmax(output), labels, only_present, per_image, ignore) of lovasz_losses.py:173-210 on logits [B,C,H,W] and the
    one-hot target [B,C,H,W] (channel 0 the background), 2 <= C <= 4.  The defaults are this project's behaviour so far - per image,
    every class: the mean over the B*C (image, class) rows - NOT the reference function's, which are only_present=False,
    per_image=False.  ``only_present``: classes without a pixel in the image (per_image=False: in the batch) are left out of the mean.
    ``ignore``: a void pixel carries this value in EVERY channel of the target (a one-hot target has no label plane to mark it in); it
    is left out of every class and its logits get a gradient of exactly 0."""
    from .autograd import _NativeLoss
    opts = lovasz_params('lovasz_softmax', {'only_present': only_present, 'per_image': per_image, 'ignore': ignore})
    if opts == (False, True, None):
        return _NativeLoss.apply(output, target, 'lovasz_softmax')
    return _NativeLoss.apply(output, target, 'lovasz_softmax', opts)


def mixed_dice_cross_entropy_loss(output, target, dice_weight=0.5, dice_loss=None, cross_entropy_weight=0.5, cross_entropy_loss=None, smooth=0,
                                  dice_activation='softmax'):
    """dice_weight * mean over the foreground classes of the soft Dice loss of softmax(output) + cross_entropy_weight * cross entropy
    (models.py:343-388), batch-wide sums, on logits [B,C,H,W] and the one-hot target [B,C,H,W] WITH its background channel 0.

    The reference function pairs ``target[:, class_nr]`` with output channel ``class_nr + 1`` (models.py:346-351), which assumes a target
    without a background channel; with this project's [background, foreground] targets that would swap the classes, so it is not
    reproduced: class c of the output is compared with channel c of the target, and the label is the target's argmax."""
    if dice_activation != 'softmax' or dice_loss is not None or cross_entropy_loss is not None:
        raise NotImplementedError('only the softmax Dice + cross entropy pair has a HIP kernel')
    from .autograd import _NativeLoss
    return _NativeLoss.apply(output, target, 'dice_ce', (float(dice_weight), float(cross_entropy_weight), float(smooth)))


lovasz_loss.native_kind = 'lovasz'
mixed_dice_bce_loss.native_kind = 'bce_dice'
lovasz_softmax_loss.native_kind = 'lovasz_softmax'
mixed_dice_cross_entropy_loss.native_kind = 'dice_ce'
