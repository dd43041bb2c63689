"""Plain float64 references of the streaming, BatchNorm, loss and optimizer operators, plus the view helpers the operator tests share.

Everything here is the textbook definition of an operation (loops over windows / pixels, torch arithmetic in double), NOT a
transcription of a kernel: no vector pieces, no partial sums, no folded coefficients.  Activations are NHWC ``torch.float64``.
``test_op_reference_cpu.py`` pins every function against torch autograd / ``torch.optim`` on the CPU, so the references can be
trusted on a machine without a GPU; the ``test_gpu_ops_*`` files compare the HIP kernels with them through the C-ABI."""
import math

import torch

F64 = torch.float64


def round_to(x, dtype):
    """fp64 values as the storage dtype holds them ('bf16' / 'f32'), back in fp64."""
    return x.to(torch.bfloat16 if dtype == 'bf16' else torch.float32).to(F64)


# ---------------------------------------------------------------- elementwise
def affine_act(y, scale, shift, res, relu):
    a = y.clone() if scale is None else y * scale + shift
    if res is not None:
        a = a + res
    return a.clamp_min(0) if relu else a


def relu_bwd(da, a, old, accumulate):
    dy = da.clone() if a is None else torch.where(a > 0, da, torch.zeros_like(da))
    return dy + old if accumulate else dy


def add(a, b, old, accumulate):
    y = a.clone() if b is None else a + b
    return y + old if accumulate else y


def nchw_to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------- pooling
def _windows(H, W, k, stride, pad, OH, OW):
    """[(oy, ox, [(iy, ix), ...] in row-major window order, padding left out)]"""
    out = []
    for oy in range(OH):
        for ox in range(OW):
            pos = [(stride * oy - pad + ky, stride * ox - pad + kx) for ky in range(k) for kx in range(k)]
            out.append((oy, ox, [(iy, ix) for iy, ix in pos if 0 <= iy < H and 0 <= ix < W]))
    return out


def _maxpool(x, k, stride, pad, OH, OW):
    B, H, W, C = x.shape
    y = torch.empty(B, OH, OW, C, dtype=x.dtype)
    for oy, ox, pos in _windows(H, W, k, stride, pad, OH, OW):
        y[:, oy, ox] = torch.stack([x[:, iy, ix] for iy, ix in pos]).max(0).values
    return y


def _maxpool_bwd(x, dy, k, stride, pad, old, accumulate):
    B, H, W, C = x.shape
    dx = torch.zeros_like(x)
    for oy, ox, pos in _windows(H, W, k, stride, pad, dy.shape[1], dy.shape[2]):
        best = x[:, pos[0][0], pos[0][1]].clone()
        arg = torch.zeros(B, C, dtype=torch.long)
        for n, (iy, ix) in enumerate(pos[1:], 1):
            better = x[:, iy, ix] > best                          # strictly greater: the FIRST maximum keeps the window
            best = torch.where(better, x[:, iy, ix], best)
            arg = torch.where(better, torch.full_like(arg, n), arg)
        for n, (iy, ix) in enumerate(pos):
            dx[:, iy, ix] += torch.where(arg == n, dy[:, oy, ox], torch.zeros_like(best))
    return dx + old if accumulate else dx


def maxpool2(x):
    return _maxpool(x, 2, 2, 0, x.shape[1] // 2, x.shape[2] // 2)


def maxpool2_bwd(x, dy, old=None, accumulate=False):
    return _maxpool_bwd(x, dy, 2, 2, 0, old, accumulate)


def maxpool3s2(x):
    return _maxpool(x, 3, 2, 1, (x.shape[1] + 1) // 2, (x.shape[2] + 1) // 2)


def maxpool3s2_bwd(x, dy, old=None, accumulate=False):
    return _maxpool_bwd(x, dy, 3, 2, 1, old, accumulate)


def avgpool2(x):
    B, H, W, C = x.shape
    y = torch.empty(B, H // 2, W // 2, C, dtype=x.dtype)
    for oy, ox, pos in _windows(H, W, 2, 2, 0, H // 2, W // 2):
        y[:, oy, ox] = sum(x[:, iy, ix] for iy, ix in pos) / 4
    return y


def avgpool2_bwd(dy, H, W, old=None, accumulate=False):
    B, OH, OW, C = dy.shape
    dx = torch.zeros(B, H, W, C, dtype=dy.dtype)
    for oy, ox, pos in _windows(H, W, 2, 2, 0, OH, OW):
        for iy, ix in pos:
            dx[:, iy, ix] += dy[:, oy, ox] / 4
    return dx + old if accumulate else dx


# ---------------------------------------------------------------- replicate-pad adjoint
def pad_fold(xp, top, bottom, left, right, old=None, accumulate=False):
    """Adjoint of replicate padding: every pixel of the extended gradient goes to the interior pixel it was copied from."""
    B, Hp, Wp, C = xp.shape
    H, W = Hp - top - bottom, Wp - left - right
    x = torch.zeros(B, H, W, C, dtype=xp.dtype)
    for py in range(Hp):
        for px in range(Wp):
            x[:, min(max(py - top, 0), H - 1), min(max(px - left, 0), W - 1)] += xp[:, py, px]
    return x + old if accumulate else x


def fold_ring_pixels(H, W, top, bottom, left, right):
    """Extended-grid coordinates (py, px) of the pad ring in strip order: the rows above the interior whole, then the rows below it
    whole, then for every interior row its `left` columns followed by its `right` columns."""
    Wp = W + left + right
    ring = [(py, px) for py in range(top) for px in range(Wp)]
    ring += [(top + H + r, px) for r in range(bottom) for px in range(Wp)]
    for r in range(H):
        ring += [(top + r, px) for px in range(left)] + [(top + r, left + W + k) for k in range(right)]
    return ring


def ring_from_padded(xp, top, bottom, left, right):
    """[B, ring, C]: the pad ring of an extended gradient in strip layout."""
    H, W = xp.shape[1] - top - bottom, xp.shape[2] - left - right
    ring = fold_ring_pixels(H, W, top, bottom, left, right)
    if not ring:
        return torch.zeros(xp.shape[0], 0, xp.shape[3], dtype=xp.dtype)
    return torch.stack([xp[:, py, px] for py, px in ring], 1)


def pad_fold_strip(strip, x, top, bottom, left, right):
    """x (the interior of the extended gradient, already in place) += the fold of the ring alone."""
    B, H, W, C = x.shape
    out = x.clone()
    for n, (py, px) in enumerate(fold_ring_pixels(H, W, top, bottom, left, right)):
        out[:, min(max(py - top, 0), H - 1), min(max(px - left, 0), W - 1)] += strip[:, n]
    return out


# ---------------------------------------------------------------- BatchNorm
def _bn_from_moments(mean, m2, n, gamma, beta, running_mean, running_var, momentum, eps):
    var = m2 / n if n > 0 else torch.zeros_like(m2)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    out = {'mean': mean, 'invstd': invstd, 'scale': scale, 'shift': beta - mean * scale}
    if running_mean is not None:
        unbiased = m2 / (n - 1) if n > 1 else var
        out['running_mean'] = (1 - momentum) * running_mean + momentum * mean
        out['running_var'] = (1 - momentum) * running_var + momentum * unbiased
    return out


def bn_finalize(partials, counts, gamma, beta, running_mean, running_var, momentum, eps):
    """partials [nparts, 2, C] = (sum, M2 about the partial's own mean), counts [nparts]: exact merge of (sum, M2, n)."""
    n = float(counts.sum())
    mean = partials[:, 0].sum(0) / n if n > 0 else torch.zeros_like(partials[0, 0])
    m2 = torch.zeros_like(mean)
    for k in range(partials.shape[0]):
        if counts[k] > 0:
            m2 = m2 + partials[k, 1] + counts[k] * (partials[k, 0] / counts[k] - mean) ** 2
    return _bn_from_moments(mean, m2, n, gamma, beta, running_mean, running_var, momentum, eps)


def bn_finalize_shards(shards, gamma, beta, running_mean, running_var, momentum, eps):
    """shards [8, 2 C + 1] = (sum [C], sum of squares [C], count)."""
    C = (shards.shape[1] - 1) // 2
    n = float(shards[:, 2 * C].sum())
    s, q = shards[:, :C].sum(0), shards[:, C:2 * C].sum(0)
    mean = s / n if n > 0 else torch.zeros_like(s)
    m2 = (q - n * mean * mean).clamp_min(0)
    return _bn_from_moments(mean, m2, n, gamma, beta, running_mean, running_var, momentum, eps)


def bn_fold(gamma, beta, running_mean, running_var, eps):
    scale = gamma / torch.sqrt(running_var + eps)
    return scale, beta - running_mean * scale


def bn_bwd(da, a, y, relu, mean, invstd, gamma, beta, da_bias=None, old_dres=None, accumulate_dres=False,
           old_dgamma=None, old_dbeta=None, accumulate_param_grads=False, sums=None):
    """Backward of a = relu?(bn(y) (+ res)) in train mode -> dy, dres, dgamma, dbeta, coef [3, C].
    a is None with relu: the mask is recomputed from y (a = relu(bn(y)), no residual).  da_bias [B, C] is added to da wherever it is
    read.  mean / invstd are the operator's arguments, not necessarily the batch statistics of y.  ``sums`` = (sum gg, sum gg xhat)
    replaces the sums of this call (the operator's partials_ready modes, where the caller supplies them)."""
    B, H, W, C = y.shape
    M = B * H * W
    g = da if da_bias is None else da + da_bias.reshape(B, 1, 1, C)
    xhat = (y - mean) * invstd
    if not relu:
        mask = torch.ones_like(y)
    elif a is not None:
        mask = (a > 0).to(F64)
    else:
        mask = ((y - mean) * invstd * gamma + beta > 0).to(F64)
    gg = mask * g
    s1, s2 = (gg.sum((0, 1, 2)), (gg * xhat).sum((0, 1, 2))) if sums is None else sums
    c1, c2 = s1 / M, s2 / M
    k = gamma * invstd
    dy = k * (gg - c1 - xhat * c2)
    dres = gg + old_dres if accumulate_dres else gg
    dgamma = s2 + old_dgamma if accumulate_param_grads else s2
    dbeta = s1 + old_dbeta if accumulate_param_grads else s1
    return dy, dres, dgamma, dbeta, torch.stack([k, c1, c2])


# ---------------------------------------------------------------- loss / optimizer
def bce_dice(z, t, dice_w, bce_w, scale):
    """z, t NCHW-like [B, C, HW] fp64 -> (loss, dz, sums [3 C + 1] = per channel (sum p t, sum p, sum t), then the BCE sum)."""
    from oracle import losses as OL
    import torch.nn.functional as F
    zz = z.detach().clone().to(F64).requires_grad_(True)
    # oracle.losses.mixed_dice_bce_loss term by term: the function itself casts the target to fp32, after which torch evaluates the
    # BCE term in single precision (4e-8 off) - here the target stays double (test_op_reference_cpu.py compares the two)
    loss = (dice_w * OL.multiclass_dice_loss(zz, t.to(F64)) + bce_w * F.binary_cross_entropy_with_logits(zz, t.to(F64))) * scale
    loss.backward()
    p = torch.sigmoid(z.to(F64))
    C = z.shape[1]
    sums = torch.zeros(3 * C + 1, dtype=F64)
    for c in range(C):
        sums[3 * c], sums[3 * c + 1], sums[3 * c + 2] = (p[:, c] * t[:, c]).sum(), p[:, c].sum(), t[:, c].sum()
    zd = z.to(F64)
    sums[3 * C] = (zd.clamp_min(0) - zd * t + torch.log1p(torch.exp(-zd.abs()))).sum()
    return float(loss.detach()), zz.grad, sums


def tick(beta1, beta2, t):
    """Adam's bias corrections after t steps."""
    return 1.0 - beta1 ** t, 1.0 - beta2 ** t


def adam(p, g, m, v, hyper):
    """hyper = (lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale) -> (p, m, v) after one step of Adam with the
    weight decay added to the (scaled) gradient."""
    lr, b1, b2, eps, wd, bc1, bc2, gs = [float(h) for h in hyper]
    gr = g * gs + wd * p
    m1 = b1 * m + (1 - b1) * gr
    v1 = b2 * v + (1 - b2) * gr * gr
    return p - (lr / bc1) * m1 / (torch.sqrt(v1) / math.sqrt(bc2) + eps), m1, v1


# ---------------------------------------------------------------- views and guards
GUARD = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FA5, torch.float64: 0x7FF8A5A5A5A5A5A5}     # NaN payloads: a read shows too
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}

# view variants of the operator tests: name -> dtype -> (c0, C, cs)
VARIANTS = {
    'a': {'f32': (0, 16, 16), 'bf16': (0, 16, 16)},        # contiguous, 16-byte pieces
    'b': {'f32': (8, 16, 40), 'bf16': (8, 16, 40)},        # channel slice of a wider buffer, 16-byte pieces
    'c': {'f32': (2, 16, 40), 'bf16': (4, 16, 40)},        # slice whose first element is 8 bytes past a 16-byte boundary: scalar
    'd': {'f32': (0, 13, 13), 'bf16': (0, 13, 13)},        # ragged: scalar
}
# (inputs, outputs): the mixed pairs make vec_ok of ONE view decide the path
VIEW_CASES = [('a', 'a'), ('b', 'b'), ('c', 'c'), ('d', 'd'), ('a', 'c'), ('c', 'b'), ('b', 'a')]


def torch_dtype(dtype):
    return torch.bfloat16 if dtype == 'bf16' else torch.float32


def guard_fill(buf):
    """Fill a whole [B, H, W, cs] buffer with a fixed bit pattern (a NaN, so that a stray READ of a gap channel shows as well)."""
    buf.view(_INT[buf.dtype]).fill_(GUARD[buf.dtype])
    return buf


def guard_check(buf, c0, C, what=''):
    """Every element outside channels [c0, c0 + C) still holds the pattern (compared as integers)."""
    bits = buf.view(_INT[buf.dtype]).cpu()
    pat = torch.tensor(GUARD[buf.dtype], dtype=bits.dtype)
    left, right = bits[..., :c0], bits[..., c0 + C:]
    assert bool((left == pat).all()) and bool((right == pat).all()), \
        '%s: %d gap elements of the output buffer were overwritten' % (what, int((left != pat).sum() + (right != pat).sum()))


def make_view(buf, c0, C):
    """buf [B, H, W, cs] -> (salt_view of channels [c0, c0 + C), that window as a tensor view)."""
    from salt_amd.engine import shaped_view
    B, H, W, cs = buf.shape
    assert buf.is_contiguous() and 0 <= c0 and c0 + C <= cs
    return shaped_view(buf.data_ptr() + c0 * buf.element_size(), B, H, W, C, cs), buf[..., c0:c0 + C]


class Placed:
    """A guard-filled [B, H, W, cs] buffer on `device` with a C-channel window: .view (salt_view), .win (tensor view), .check()."""

    def __init__(self, shape_bhw, variant, dtype, device, values=None):
        self.c0, self.C, cs = VARIANTS[variant][dtype] if isinstance(variant, str) else variant
        B, H, W = shape_bhw
        self.buf = guard_fill(torch.empty(B, H, W, cs, dtype=torch_dtype(dtype), device=device))
        self.view, self.win = make_view(self.buf, self.c0, self.C)
        if values is not None:
            self.win.copy_(values.to(self.buf.dtype))

    def get(self):
        return self.win.to(F64).cpu()

    def check(self, what=''):
        guard_check(self.buf, self.c0, self.C, what)


def avoid_zero_crossings(y, pre_fn, margin, dtype='f32'):
    """Move every element of y whose fp64 pre-activation pre_fn(y) lies within `margin` of zero away from zero (y is rounded to the
    storage dtype first and after every move; the check is done on the rounded values) and assert that none remain."""
    y = round_to(y, dtype)
    for step in range(1, 33):
        pre = pre_fn(y)
        bad = pre.abs() < margin
        if not bool(bad.any()):
            break
        sign = torch.where(pre >= 0, torch.ones_like(pre), -torch.ones_like(pre))
        y = round_to(torch.where(bad, y + sign * 0.0625 * step, y), dtype)
    assert not bool((pre_fn(y).abs() < margin).any()), 'pre-activations within %g of zero remain' % margin
    return y
