"""The fp64 operator references of op_reference.py against an independent CPU evaluation (torch autograd / torch.optim in float64), so
that the references the GPU operator tests rely on are validated without a GPU.  Arithmetic agrees to 1e-12 relative; selections and
permutations agree exactly."""
import math

import pytest
import torch
import torch.nn.functional as F

import op_reference as R

F64 = torch.float64
SHAPES = [(2, 6, 8, 5), (3, 7, 5, 3), (1, 1, 1, 2), (2, 2, 2, 4), (2, 7, 9, 3)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, ref, what=''):
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    assert got.shape == ref.shape and err <= 1e-12 * max(1.0, float(ref.abs().max()) if ref.numel() else 0.0), (what, err)


def _ints(shape, g, lo=-2, hi=3):
    return torch.randint(lo, hi, shape, generator=g).to(F64)          # many ties


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


@pytest.mark.parametrize('shape,kind', [(s, k) for s in SHAPES for k in ('2', '3s2') if k == '3s2' or s[1] >= 2])
def test_maxpool_matches_torch(shape, kind):
    B, H, W, C = shape
    g = _gen(H * 10 + W)
    x = _ints(shape, g)
    fwd, bwd, kw = (R.maxpool2, R.maxpool2_bwd, dict(kernel_size=2, stride=2)) if kind == '2' else \
        (R.maxpool3s2, R.maxpool3s2_bwd, dict(kernel_size=3, stride=2, padding=1))
    xt = _nchw(x).clone().requires_grad_(True)
    yt = F.max_pool2d(xt, **kw)
    y = fwd(x)
    assert torch.equal(y, _nhwc(yt.detach()))
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    yt.backward(_nchw(dy))
    assert torch.equal(bwd(x, dy), _nhwc(xt.grad))                     # a selection: exact, first maximum of tied windows
    old = torch.randn(shape, generator=g, dtype=F64)
    assert torch.equal(bwd(x, dy, old, True), _nhwc(xt.grad) + old)
    if kind == '2' and (H % 2 or W % 2):                               # the row / column no window covers gets no gradient
        assert float(bwd(x, dy)[:, H - H % 2:].abs().sum() + bwd(x, dy)[:, :, W - W % 2:].abs().sum()) == 0.0


def test_maxpool_tie_goes_to_first_maximum():
    x = torch.zeros(1, 2, 2, 1, dtype=F64)
    dy = torch.ones(1, 1, 1, 1, dtype=F64)
    assert R.maxpool2_bwd(x, dy).reshape(-1).tolist() == [1.0, 0.0, 0.0, 0.0]
    x3 = torch.zeros(1, 3, 3, 1, dtype=F64)
    dy3 = torch.ones(1, 2, 2, 1, dtype=F64)
    assert R.maxpool3s2_bwd(x3, dy3).reshape(-1).tolist() == [1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[1] >= 2])
def test_avgpool_matches_torch(shape):
    B, H, W, C = shape
    g = _gen(H + W)
    x = torch.randn(shape, generator=g, dtype=F64)
    xt = _nchw(x).clone().requires_grad_(True)
    yt = F.avg_pool2d(xt, 2, 2)
    _close(R.avgpool2(x), _nhwc(yt.detach()), 'avgpool2')
    dy = torch.randn(yt.shape, generator=g, dtype=F64)
    yt.backward(dy)
    _close(R.avgpool2_bwd(_nhwc(dy), H, W), _nhwc(xt.grad), 'avgpool2 backward')
    old = torch.randn(shape, generator=g, dtype=F64)
    _close(R.avgpool2_bwd(_nhwc(dy), H, W, old, True), _nhwc(xt.grad) + old, 'avgpool2 backward accumulate')


PADS = [(2, 0, 0, 2), (0, 2, 2, 0), (1, 2, 3, 1), (0, 0, 0, 0)]


@pytest.mark.parametrize('pads', PADS)
@pytest.mark.parametrize('shape', [(2, 5, 4, 3), (1, 1, 1, 2), (2, 2, 7, 3)])
def test_pad_fold_is_adjoint_of_replicate_pad(pads, shape):
    top, bottom, left, right = pads
    B, H, W, C = shape
    g = _gen(sum(pads) + H)
    xt = torch.randn(B, C, H, W, generator=g, dtype=F64).requires_grad_(True)
    xpt = F.pad(xt, (left, right, top, bottom), mode='replicate')
    gp = torch.randn(xpt.shape, generator=g, dtype=F64)
    xpt.backward(gp)
    _close(R.pad_fold(_nhwc(gp), *pads), _nhwc(xt.grad), 'pad_fold')
    old = torch.randn(B, H, W, C, generator=g, dtype=F64)
    _close(R.pad_fold(_nhwc(gp), *pads, old, True), _nhwc(xt.grad) + old, 'pad_fold accumulate')
    # strip form: ring + interior = the whole fold; the ring has salt_fold_strip_pixels entries, each extended pixel once
    ring = R.fold_ring_pixels(H, W, *pads)
    assert len(ring) == (top + bottom) * (W + left + right) + H * (left + right) and len(set(ring)) == len(ring)
    interior = {(top + r, left + c) for r in range(H) for c in range(W)}
    assert not (set(ring) & interior) and len(ring) + len(interior) == (H + top + bottom) * (W + left + right)
    strip = R.ring_from_padded(_nhwc(gp), *pads)
    inner = _nhwc(gp)[:, top:top + H, left:left + W].contiguous()
    _close(R.pad_fold_strip(strip, inner, *pads), _nhwc(xt.grad), 'pad_fold_strip')


def test_elementwise_and_layout():
    g = _gen(3)
    a, b, old = (torch.randn(2, 3, 4, 5, generator=g, dtype=F64) for _ in range(3))
    assert torch.equal(R.add(a, None, None, False), a) and torch.equal(R.add(a, b, old, True), a + b + old)
    assert torch.equal(R.add(a, None, old, True), a + old)
    at = a.clone().requires_grad_(True)
    torch.relu(at).backward(b)
    assert torch.equal(R.relu_bwd(b, torch.relu(a), None, False), at.grad)
    assert torch.equal(R.relu_bwd(b, None, old, True), b + old)
    x = torch.randn(2, 5, 3, 4, generator=g, dtype=F64)                # NCHW
    assert torch.equal(R.nchw_to_nhwc(x), x.permute(0, 2, 3, 1)) and torch.equal(R.nhwc_to_nchw(R.nchw_to_nhwc(x)), x)
    assert R.nchw_to_nhwc(x).is_contiguous()


def _bn_problem(shape, seed, relu, with_res):
    B, H, W, C = shape
    g = _gen(seed)
    y = torch.randn(shape, generator=g, dtype=F64) * 1.5 + torch.linspace(-1, 1, C, dtype=F64)
    gamma = torch.rand(C, generator=g, dtype=F64) + 0.5
    beta = torch.randn(C, generator=g, dtype=F64) * 0.3
    res = torch.randn(shape, generator=g, dtype=F64) if with_res else None
    da = torch.randn(shape, generator=g, dtype=F64)
    return y, gamma, beta, res, da


@pytest.mark.parametrize('shape', [(3, 5, 7, 4), (2, 4, 8, 3), (1, 1, 1, 2), (1, 2, 3, 2)])
@pytest.mark.parametrize('relu,with_res', [(0, False), (1, False), (1, True), (0, True)])
def test_bn_forward_and_backward_match_torch(shape, relu, with_res):
    B, H, W, C = shape
    M = B * H * W
    y, gamma, beta, res, da = _bn_problem(shape, M + relu, relu, with_res)
    rm, rv = torch.randn(C, dtype=F64, generator=_gen(1)), torch.rand(C, dtype=F64, generator=_gen(2)) + 0.5
    yt, gt, bt = _nchw(y).clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rt = _nchw(res).clone().requires_grad_(True) if with_res else None
    rmt, rvt = rm.clone(), rv.clone()
    if M > 1:
        out = F.batch_norm(yt, rmt, rvt, gt, bt, training=True, momentum=0.1, eps=1e-5)
    else:                                                           # torch refuses one value per channel; N == 1: var = 0, running_var keeps var
        out = (yt - yt.detach()) / math.sqrt(1e-5) * gt.reshape(1, C, 1, 1) + bt.reshape(1, C, 1, 1)
        rmt, rvt = 0.9 * rm + 0.1 * y.reshape(C), 0.9 * rv
    if with_res:
        out = out + rt
    if relu:
        out = torch.relu(out)
    # forward: split the pixels into unequal partials (first and last smaller), exact merge
    flat = y.reshape(M, C)
    cuts = sorted(set([0, 1, M // 3, M - 1, M]))
    parts = [flat[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    partials = torch.stack([torch.stack([p.sum(0), ((p - p.mean(0)) ** 2).sum(0)]) for p in parts])
    counts = torch.tensor([float(len(p)) for p in parts], dtype=F64)
    f = R.bn_finalize(partials, counts, gamma, beta, rm, rv, 0.1, 1e-5)
    a = R.affine_act(y, f['scale'], f['shift'], res, relu)
    _close(a, _nhwc(out.detach()), 'bn forward')
    _close(f['running_mean'], rmt, 'running_mean')
    _close(f['running_var'], rvt, 'running_var')
    _close(f['mean'], flat.mean(0), 'mean')
    # shard form (sum, sum of squares, count): same result
    shards = torch.zeros(8, 2 * C + 1, dtype=F64)
    for k, p in enumerate(parts):
        s = (3 * k + 1) % 8
        shards[s, :C] += p.sum(0); shards[s, C:2 * C] += (p * p).sum(0); shards[s, 2 * C] += len(p)
    f2 = R.bn_finalize_shards(shards, gamma, beta, rm, rv, 0.1, 1e-5)
    for k in f:
        assert float((f[k] - f2[k]).abs().max()) <= 1e-10 * max(1.0, float(f[k].abs().max())), k      # sum of squares cancels a few digits
    if M == 1:
        return
    # backward
    out.backward(_nchw(da))
    dy, dres, dgamma, dbeta, coef = R.bn_bwd(da, a if relu else None, y, relu, f['mean'], f['invstd'], gamma, beta)
    _close(dy, _nhwc(yt.grad), 'dy')
    _close(dgamma, gt.grad, 'dgamma')
    _close(dbeta, bt.grad, 'dbeta')
    if with_res:
        _close(dres, _nhwc(rt.grad), 'dres')
    else:
        dy2 = R.bn_bwd(da, None, y, relu, f['mean'], f['invstd'], gamma, beta)[0]        # mask recomputed from y
        _close(dy2, _nhwc(yt.grad), 'dy (mask from y)')
    _close(coef[0], gamma * f['invstd'], 'coef k')
    # accumulate flags and da_bias = da shifted per image and channel
    bias = torch.randn(B, C, dtype=F64, generator=_gen(5))
    od, og, ob = torch.randn(shape, dtype=F64, generator=_gen(6)), torch.randn(C, dtype=F64, generator=_gen(7)), torch.randn(C, dtype=F64, generator=_gen(8))
    ref = R.bn_bwd(da + bias.reshape(B, 1, 1, C), a if relu else None, y, relu, f['mean'], f['invstd'], gamma, beta)
    got = R.bn_bwd(da, a if relu else None, y, relu, f['mean'], f['invstd'], gamma, beta, bias, od, True, og, ob, True)
    _close(got[0], ref[0], 'dy with da_bias')
    _close(got[1], ref[1] + od, 'dres accumulate')
    _close(got[2], ref[2] + og, 'dgamma accumulate')
    _close(got[3], ref[3] + ob, 'dbeta accumulate')


def test_bn_fold_matches_eval_batch_norm():
    g = _gen(4)
    C = 5
    x = torch.randn(2, C, 3, 3, generator=g, dtype=F64)
    gamma, beta, rm = (torch.randn(C, generator=g, dtype=F64) for _ in range(3))
    rv = torch.rand(C, generator=g, dtype=F64) + 0.2
    scale, shift = R.bn_fold(gamma, beta, rm, rv, 1e-5)
    _close(R.affine_act(_nhwc(x), scale, shift, None, 0), _nhwc(F.batch_norm(x, rm, rv, gamma, beta, training=False, eps=1e-5)), 'bn_fold')


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 2, 255), (3, 2, 4097)])
@pytest.mark.parametrize('scale', [1.0, 0.25])
def test_bce_dice_matches_definition(shape, scale):
    g = _gen(shape[2])
    z = torch.randn(shape, generator=g, dtype=F64) * 3
    t = (torch.rand(shape, generator=g) < 0.3).to(F64)
    loss, dz, sums = R.bce_dice(z, t, 0.2, 0.9, scale)
    zt = z.clone().requires_grad_(True)
    p = torch.sigmoid(zt)
    dice = sum(1 - 2 * (p[:, c] * t[:, c]).sum() / (p[:, c].sum() + t[:, c].sum() + 1e-7) for c in range(shape[1])) / shape[1]
    ref = (0.2 * dice + 0.9 * F.binary_cross_entropy_with_logits(zt, t)) * scale
    ref.backward()
    assert abs(loss - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
    _close(dz, zt.grad, 'dlogits')
    from oracle import losses as OL
    assert abs(loss - scale * float(OL.mixed_dice_bce_loss(z, t))) <= 1e-6 * max(1.0, abs(loss))      # its BCE term runs with an fp32 target
    _close(sums[3 * shape[1]], F.binary_cross_entropy_with_logits(z, t, reduction='sum'), 'bce sum')
    _close(sums[1], torch.sigmoid(z[:, 0]).sum(), 'sum p')


@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('n', [1, 5])
def test_adam_matches_torch_optim(wd, n):
    g = _gen(n)
    p0 = (torch.rand(n, generator=g, dtype=F64) - 0.5) * 0.2
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    q, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for t in range(1, 5):
        gr = torch.randn(n, generator=g, dtype=F64) * 0.1
        p.grad = gr.clone()
        opt.step()
        bc1, bc2 = R.tick(0.9, 0.999, t)
        q, m, v = R.adam(q, gr * 64, m, v, (1e-2, 0.9, 0.999, 1e-8, wd, bc1, bc2, 1 / 64))      # grad_scale undoes a scaled gradient
        _close(q, p.detach(), 'param step %d' % t)
        st = opt.state[p]
        _close(m, st['exp_avg'], 'exp_avg')
        _close(v, st['exp_avg_sq'], 'exp_avg_sq')
    assert R.tick(0.9, 0.999, 1) == (1.0 - 0.9, 1.0 - 0.999)


def test_guard_and_zero_crossing_helpers():
    for dt in (torch.float32, torch.bfloat16):
        buf = R.guard_fill(torch.empty(2, 3, 2, 10, dtype=dt))
        buf[..., 2:7] = 1.0
        R.guard_check(buf, 2, 5)
        buf[1, 2, 1, 7] = 0.0
        with pytest.raises(AssertionError):
            R.guard_check(buf, 2, 5)
    y = torch.linspace(-1, 1, 4001, dtype=F64).reshape(1, 1, 4001, 1)
    for dtype in ('f32', 'bf16'):
        pre = lambda v: v * 0.7 + 0.01
        out = R.avoid_zero_crossings(y, pre, 1e-3, dtype)
        assert float(pre(out).abs().min()) >= 1e-3 and torch.equal(out, R.round_to(out, dtype))
        assert float((out - R.round_to(y, dtype)).abs().max()) <= 0.5
