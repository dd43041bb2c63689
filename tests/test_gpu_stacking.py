"""GPU tests of the second-level (stacking) networks: salt_stack_conv / salt_stack_grad_unfold of csrc/stacking.hip through the C-ABI
against the float64 operator reference tests/stacking_op_reference.py, StackingFCN / StackingFCNWithDepth against the F16 fixtures the
reference's own modules produced, and the trainer / inference surface.

Operator tolerances are close() of abi_ops.py on inputs already rounded to the compute dtype (f32: 5e-5 max|ref|;
bf16: 2^-8 |ref| + 5e-5 max|ref|).  The BatchNorm statistics are defined on the STORED y (saltnet.h), so they are compared - at the fp32
bound in both dtypes - with the float64 statistics of the y the kernel wrote; y itself is compared with the reference."""
import ctypes

import numpy as np
import pytest
import torch

import closed_form as CF
import stacking_op_reference as SR
from helpers import golden, T, assert_close
from op_reference import round_to
import net_checks as NC
from abi_ops import _abi, call, close, code, gen, DEV, F64, TDT

pytestmark = pytest.mark.gpu
DTYPES = ['f32', 'bf16']
# (B, M, F, K, H, W): smaller than a tile | ragged both ways, several tiles, padded channels | exact tiles | ... ; the last one is the
# largest supported case, the only one where fp32 stages the weights in two channel chunks (M > 48 with F = 64)
SHAPES = [(1, 1, 16, 1, 8, 8), (2, 5, 32, 2, 19, 37), (2, 16, 16, 2, 16, 64), (1, 20, 32, 2, 33, 17), (2, 32, 32, 2, 32, 32),
          (1, 40, 64, 4, 9, 70), (1, 64, 32, 2, 16, 16), (1, 64, 64, 2, 9, 20)]
GUARD = 64                       # sentinel elements on both sides of every output window (a multiple of 16 bytes in both dtypes)
SENT = 1024.0                    # exact in bf16


class Window:
    """n elements of ``tdt`` on the device with GUARD sentinels before and after; check() proves the launch stayed inside"""

    def __init__(self, n, tdt, fill=float('nan')):
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=tdt, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def check(self, what):
        assert bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all()), '%s: wrote outside its window' % what

    def get(self, shape):
        return self.t.reshape(shape).to(F64).cpu()


def view(ptr, B, H, W, C, cs=None):
    v = _abi().STRUCTS['salt_view']()
    v.p, v.B, v.H, v.W, v.C, v.cs = ptr, B, H, W, C, (C if cs is None else cs)
    return v


def operands(shape, dtype, *seed):
    B, M, F_, K, H, W = shape
    g = gen('stack', shape, dtype, *seed)
    x = round_to(torch.rand((B, M, H, W), generator=g, dtype=F64), dtype)                 # probabilities
    w = round_to(torch.randn((F_, M, 3, 3), generator=g, dtype=F64) * (1.6 / (9 * M)) ** 0.5, dtype)
    bias = torch.randn(F_, generator=g, dtype=F64).float().to(F64) * 0.1
    return x, w, bias


def dev32(t):
    return t.to(torch.float32).contiguous().to(DEV)


def run_train(shape, dtype, x, w, bias):
    """-> (y [B,H,W,F] f64, xs [B,H,W,Mpad] f64, stats (sum, M2, count) per tile, the device tensors kept for the weight gradient)"""
    abi = _abi()
    B, M, F_, K, H, W = shape
    Mpad = (M + 15) // 16 * 16
    xd, wd, bd = dev32(x), dev32(w), dev32(bias)
    x0 = xd.clone()
    S = abi.fill(abi.STRUCTS['salt_stack_conv_args'](), B=B, M=M, H=H, W=W, F=F_)
    nparts = abi.lib.salt_stack_conv_stats_parts(ctypes.byref(S))
    assert nparts == B * ((H + 7) // 8) * ((W + 15) // 16)
    nst = int(abi.lib.salt_bn_stats_floats(nparts, F_))
    assert nst >= nparts * 2 * F_
    yw, xw = Window(B * H * W * F_, TDT[dtype]), Window(B * H * W * Mpad, TDT[dtype])
    st, cnt = Window(nst, torch.float32), Window(nparts, torch.float32)
    call('salt_stack_conv', dtype=code(dtype), x=xd.data_ptr(), B=B, M=M, H=H, W=W, w=wd.data_ptr(), bias=bd.data_ptr(), F=F_,
         y=view(yw.t.data_ptr(), B, H, W, F_), xs=view(xw.t.data_ptr(), B, H, W, Mpad), stats=st.t.data_ptr(), stats_cnt=cnt.t.data_ptr())
    for wdw, what in ((yw, 'y'), (xw, 'xs'), (st, 'stats'), (cnt, 'stats_cnt')):
        wdw.check(what)
    assert torch.equal(xd, x0), 'the input batch was written'
    parts = st.get((nst,))[:nparts * 2 * F_].reshape(nparts, 2, F_)
    return yw.get((B, H, W, F_)), xw.get((B, H, W, Mpad)), (parts[:, 0], parts[:, 1], cnt.get((nparts,))), (xd, x0, xw, yw)


def merge_partials(sums, m2s, cnts):
    """per-tile (sum, M2 about the tile mean, count) -> (mean, biased variance), Chan's parallel formula in float64"""
    n = cnts.sum()
    mean = sums.sum(0) / n
    tile_mean = sums / cnts[:, None]
    m2 = m2s.sum(0) + (cnts[:, None] * (tile_mean - mean[None]) ** 2).sum(0)
    return mean, m2 / n


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dtype', DTYPES)
def test_train_form_y_statistics_and_xs(dtype, shape):
    B, M, F_, K, H, W = shape
    x, w, bias = operands(shape, dtype)
    y, xs, (sums, m2s, cnts), _ = run_train(shape, dtype, x, w, bias)
    ref = SR.conv(x, w, bias).permute(0, 2, 3, 1)
    close(y, ref, dtype, 'y')
    Mpad = xs.shape[-1]
    assert torch.equal(xs, SR.xs_nhwc(x, Mpad)), 'xs is a copy (inputs are representable): every pixel once, pad channels zero'
    assert float(cnts.sum()) == B * H * W and float(cnts.max()) <= 128
    mean, var = merge_partials(sums, m2s, cnts)
    rmean, rvar, _ = SR.stats(y.permute(0, 3, 1, 2))
    close(mean, rmean, 'f32', 'mean of the stored y')
    close(var, rvar, 'f32', 'biased variance of the stored y')


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dtype', DTYPES)
def test_eval_form_with_and_without_gate(dtype, shape):
    B, M, F_, K, H, W = shape
    x, w, bias = operands(shape, dtype)
    g = gen('stack-eval', shape, dtype)
    scale = (1.0 + 0.2 * torch.randn(F_, generator=g, dtype=F64)).float().to(F64)
    shift = (0.3 * torch.randn(F_, generator=g, dtype=F64)).float().to(F64)
    hw = (torch.randn((K, F_), generator=g, dtype=F64) * F_ ** -0.5).float().to(F64)
    hb = (0.1 * torch.randn(K, generator=g, dtype=F64)).float().to(F64)
    gate = torch.sigmoid(torch.randn((B, F_), generator=g, dtype=F64)).float().to(F64)
    yref = SR.conv(x, w, bias)
    xd, wd, bd, scd, shd, hwd, hbd, gd = (dev32(t) for t in (x, w, bias, scale, shift, hw, hb, gate))
    x0 = xd.clone()
    for with_gate in (False, True):
        for relu in (1, 0):
            lw = Window(B * K * H * W, torch.float32)
            call('salt_stack_conv', dtype=code(dtype), x=xd.data_ptr(), B=B, M=M, H=H, W=W, w=wd.data_ptr(), bias=bd.data_ptr(), F=F_,
                 scale=scd.data_ptr(), shift=shd.data_ptr(), relu=relu, gate=gd.data_ptr() if with_gate else None, gate_cs=F_,
                 head_w=hwd.data_ptr(), head_b=hbd.data_ptr(), K=K, logits_nchw=lw.t.data_ptr())
            lw.check('logits')
            ref = SR.eval_head(yref, scale, shift, relu, gate if with_gate else None, hw, hb)
            close(lw.get((B, K, H, W)), ref, dtype, 'logits gate=%d relu=%d' % (with_gate, relu))
    assert torch.equal(xd, x0), 'the input batch was written'


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dtype', DTYPES)
def test_weight_gradient_drops_the_padded_channels(dtype, shape):
    """P = dL/dy, Q = the xs the train form wrote, through salt_conv_wgrad / salt_wgrad_reduce (pad_mode 1, the replicate taps) and, where
    Mpad != M, salt_stack_grad_unfold - the operator sequence Graph.stack_conv emits - into an [F,M,3,3] buffer."""
    abi = _abi()
    B, M, F_, K, H, W = shape
    x, w, bias = operands(shape, dtype)
    _, _, _, (xd, x0, xw, _) = run_train(shape, dtype, x, w, bias)
    Mpad = (M + 15) // 16 * 16
    g = gen('stack-wgrad', shape, dtype)
    dy = round_to(torch.randn((B, F_, H, W), generator=g, dtype=F64), dtype)
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(TDT[dtype]).to(DEV)
    ref = SR.wgrad(dy, x)
    td = [(kh - 2, kw) for kh in range(3) for kw in range(3)]
    wg = dict(dtype=code(dtype), p=view(dyd.data_ptr(), B, H, W, F_), q=view(xw.t.data_ptr(), B, H, W, Mpad), ntaps=9,
              tap_dy=[t[0] for t in td], tap_dx=[t[1] for t in td], q_step=1, pad_mode=1)
    ns = abi.lib.salt_conv_wgrad_nsplit(ctypes.byref(abi.fill(abi.STRUCTS['salt_conv_wgrad_args'](), **wg)))
    assert ns >= 1, abi.lib.salt_last_error()
    partials = torch.empty(ns * 9 * F_ * Mpad, dtype=torch.float32, device=DEV)
    for accumulate in (0, 1):
        old = torch.randn((F_, M, 3, 3), generator=g, dtype=F64).float().to(F64) if accumulate else torch.full((F_, M, 3, 3), float('nan'), dtype=F64)
        gw = Window(F_ * M * 9, torch.float32)
        gw.t.copy_(old.reshape(-1))
        call('salt_conv_wgrad', partials=partials.data_ptr(), nsplit=ns, **wg)
        red = dict(partials=partials.data_ptr(), nsplit=ns, ntaps=9, Ca=F_, Cb=Mpad, KH=3, KW=3, tap_kh=[t // 3 for t in range(9)],
                   tap_kw=[t % 3 for t in range(9)])
        if Mpad == M:
            call('salt_wgrad_reduce', grad=gw.t.data_ptr(), accumulate=accumulate, **red)
        else:
            gpad = Window(F_ * Mpad * 9, torch.float32)
            call('salt_wgrad_reduce', grad=gpad.t.data_ptr(), accumulate=0, **red)
            gpad.check('padded gradient')
            pad = gpad.get((F_, Mpad, 3, 3))
            assert bool((pad[:, M:] == 0).all()), 'the zero channels of xs give zero gradient'
            call('salt_stack_grad_unfold', gpad=gpad.t.data_ptr(), F=F_, M=M, Mpad=Mpad, grad=gw.t.data_ptr(), accumulate=accumulate)
        gw.check('weight gradient')
        want = ref + old if accumulate else ref
        close(gw.get((F_, M, 3, 3)), want, dtype, 'weight gradient accumulate=%d' % accumulate)
    assert torch.equal(xd, x0), 'the input batch was written'


@pytest.mark.parametrize('dtype', DTYPES)
def test_single_tap_integer_operands_are_exact(dtype):
    """Integer-valued maps and weights with ONE non-zero tap at a time: every product and sum is exact in both dtypes (|y| <= 5 x 6 x 4 =
    120 < 256), so y and the logits must EQUAL the reference - at the image border (the clamp) and at the top rows / right columns of the
    interior tile boundaries (x = 16, 32; y = 8, 16), where a halo that clamped to the TILE instead of the image would differ.  The
    weights differ per (f, m) and the map per (b, m, y, x) with unequal row / column periods: a kh / kw or a row / column swap fails."""
    B, M, F_, K, H, W = 2, 5, 32, 2, 19, 37
    bb, mm, yy, xx = torch.meshgrid(torch.arange(B), torch.arange(M), torch.arange(H), torch.arange(W), indexing='ij')
    x = ((yy * 7 + xx * 3 + mm * 5 + bb) % 13 - 6).to(F64)
    ff, m2 = torch.meshgrid(torch.arange(F_), torch.arange(M), indexing='ij')
    wtap = ((ff * 3 + m2) % 9 - 4).to(F64)
    hw = ((torch.arange(K)[:, None] + torch.arange(F_)[None, :]) % 3 - 1).to(F64)
    ones, zeros = torch.ones(F_, dtype=F64), torch.zeros(F_, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            w = torch.zeros((F_, M, 3, 3), dtype=F64)
            w[:, :, kh, kw] = wtap
            y, xs, _, (xd, x0, _, _) = run_train((B, M, F_, K, H, W), dtype, x, w, zeros)
            ref = SR.conv(x, w)
            assert float(ref.abs().max()) <= 120
            assert torch.equal(y, ref.permute(0, 2, 3, 1)), 'tap (%d, %d)' % (kh, kw)
            wd, hwd = dev32(w), dev32(hw)
            lw = Window(B * K * H * W, torch.float32)
            call('salt_stack_conv', dtype=code(dtype), x=xd.data_ptr(), B=B, M=M, H=H, W=W, w=wd.data_ptr(), bias=None, F=F_,
                 scale=None, shift=None, relu=0, gate=None, gate_cs=0, head_w=hwd.data_ptr(), head_b=None, K=K, logits_nchw=lw.t.data_ptr())
            lw.check('logits')
            assert torch.equal(lw.get((B, K, H, W)), SR.eval_head(ref, ones, zeros, 0, None, hw, None)), 'logits, tap (%d, %d)' % (kh, kw)


def test_unsupported_arguments_are_refused():
    abi = _abi()
    x = torch.zeros(1, 5, 8, 8, device=DEV)
    w = torch.zeros(32, 5, 3, 3, device=DEV)
    out = torch.zeros(1, 5, 8, 8, device=DEV)
    base = dict(dtype=0, x=x.data_ptr(), B=1, M=5, H=8, W=8, w=w.data_ptr(), F=32, head_w=w.data_ptr(), K=2, logits_nchw=out.data_ptr())
    for bad in (dict(K=5), dict(M=65), dict(F=48), dict(logits_nchw=None), dict(dtype=2)):
        with pytest.raises(abi.SaltError):
            call('salt_stack_conv', **dict(base, **bad))


# ------------------------------------------------------------------------------------------------ networks vs the reference's fixtures
FIXTURES = [('F16_stacking_fcn', False), ('F16_stacking_fcn_depth', True), ('F16_stacking_fcn_m32', False)]


def _net(fx, with_depth, dtype='f32'):
    from salt_amd import architectures as A
    net = (A.StackingFCNWithDepth if with_depth else A.StackingFCN)(int(fx['x'].shape[1]), 2, filter_nr=32, dropout_2d=0.0)
    CF.fill_module(net)
    return net.set_compute_dtype(dtype).to(DEV)


def _inputs(fx):
    return [T(fx['x']).to(DEV)] + ([T(fx['d']).to(DEV)] if 'd' in fx else [])


@pytest.mark.parametrize('name,with_depth', FIXTURES)
def test_eval_logits_and_masks_match_reference(name, with_depth):
    fx = golden(name)
    net = _net(fx, with_depth).eval()
    with torch.no_grad():
        logits = net(*_inputs(fx)).cpu()
    ops = [o[0] for o in net.engine().net(tuple(fx['x'].shape), False).fwd.ops]
    assert ops == (['depth_gate'] if with_depth else []) + ['stack_conv'], ops            # the eval network is ONE launch (+ the gate vector)
    e = assert_close(logits, fx['eval_logits'], 1e-3, 'eval logits')
    safe = np.abs(fx['eval_logits'][:, 1]) >= float(fx['near_zero_thr'])
    assert (~safe).mean() <= 1e-3
    print(name, 'eval rel err %.3e, near-zero pixels %d' % (e, int((~safe).sum())))
    assert np.array_equal((logits[:, 1] > 0).numpy()[safe], (fx['eval_logits'][:, 1] > 0)[safe])


def _train_step(fx, with_depth, dtype='f32'):
    from salt_amd.optim import FusedAdam, weight_regularization
    from salt_amd import losses
    net = _net(fx, with_depth, dtype)
    net.train()
    opt = FusedAdam(weight_regularization(net, True, 1e-4), lr=1e-4, model=net)
    out = net(*_inputs(fx))
    loss = losses.lovasz_loss(out, T(fx['t']).to(DEV)) * 1.0
    loss.backward()
    torch.cuda.synchronize()
    eng = net.engine()
    grads = {}
    for k, p in net.named_parameters():
        off, n = eng.grad_range(p)
        grads[k] = eng.grads[off:off + n].view(p.shape).cpu().clone()
    opt.step()
    torch.cuda.synchronize()
    post = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    return out.detach().cpu(), float(loss), grads, post


@pytest.mark.parametrize('det', [False, True], ids=['default_sums', 'deterministic_sums'])
@pytest.mark.parametrize('name,with_depth', FIXTURES)
def test_one_training_step_matches_reference(name, with_depth, det, request):
    """zero_grad -> forward -> lovasz -> backward -> Adam(lr 1e-4, L2 1e-4) as models.py:105-136 / 222-253, fp32.  Loss 2e-5.  Gradients:
    the project's bounds (tests/test_gpu_depth.py, test_gpu_emptiness.py) - per-tensor norm within 1e-2, four times the largest error the
    fixtures may record for the reference itself against float64, and every element within 2e-2 of the tensor's maximum; a tensor whose
    exact gradient is zero (conv.0.conv.bias, in front of a BatchNorm) is bounded by 1e-4 of the largest gradient element.  After Adam's
    first step every element has moved by +-lr unless its gradient is tiny, so a parameter may differ by at most 2 lr = 2e-4 anywhere
    and its norm by 1e-4 relative (test_gpu_depth.py).  Under the deterministic setting two runs are bit-identical."""
    if det:
        request.getfixturevalue('deterministic_sums')
    fx = golden(name)
    assert float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3
    out, loss, grads, post = _train_step(fx, with_depth)
    assert_close(out, fx['train_logits'], 1e-3, 'train logits')
    ref = float(fx['train_loss'])
    print(name, 'loss', loss, 'reference', ref)
    assert abs(loss - ref) <= 2e-5 * abs(ref), (loss, ref)
    names = fx['param_names'].tolist()
    assert list(grads) == names
    gmax = max(float(np.abs(fx['fullgrad:' + k]).max()) for k in names)
    for k in names:
        want = fx['fullgrad:' + k]
        if k in fx['zero_grad_names'].tolist():
            print('  %-40s max |g| %.3e (exact value 0)' % (k, float(grads[k].abs().max())))
            assert float(grads[k].abs().max()) <= 1e-4 * gmax, k
            continue
        n_rel = abs(float(grads[k].double().norm()) - float(np.linalg.norm(want.astype(np.float64)))) / float(np.linalg.norm(want.astype(np.float64)))
        e = assert_close(grads[k], want, 2e-2, 'grad ' + k)
        print('  %-40s norm rel %.3e  max rel %.3e' % (k, n_rel, e))
        assert n_rel <= 1e-2, (k, n_rel)
    for k in names:
        want = T(fx['post:' + k]).double()
        got = post[k].double()
        assert float((got - want).abs().max()) <= 2e-4, k
        assert abs(float(got.norm()) - float(want.norm())) <= 1e-4 * max(float(want.norm()), 1e-3), k
    for k in ('conv.0.batch_norm.running_mean', 'conv.0.batch_norm.running_var'):
        assert_close(post[k], fx['bn:' + k], 2e-5, k)
    assert int(post['conv.0.batch_norm.num_batches_tracked']) == 1
    if det:
        out2, loss2, grads2, post2 = _train_step(fx, with_depth)
        assert torch.equal(out, out2) and loss == loss2
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), k
        for k in post:
            assert torch.equal(post[k], post2[k]), k


# bf16: eval logits against the fixture's fp32 reference logits.  Allowance = MARGIN x ref_bf16_storage_vs_f32_maxabs, the deviation of
# the test-side oracle under bf16 storage of the same network.  The margin is the 2x the kernel is allowed for rounding the input maps
# and weights as well as the activations; measured once on an MI355X: err / recorded = 0.53 (M = 5), 0.57 (depth), 0.63 (M = 32) - the
# fused eval launch rounds only the maps and the weights and keeps the activation in fp32, so it stays below the oracle's own figure.
BF16_MARGIN = 2.0
BF16_MEASURED = {'F16_stacking_fcn': 0.53, 'F16_stacking_fcn_depth': 0.57, 'F16_stacking_fcn_m32': 0.63}


@pytest.mark.parametrize('name,with_depth', FIXTURES)
def test_bf16_eval_logits_within_the_recorded_storage_error(name, with_depth):
    fx = golden(name)
    net = _net(fx, with_depth, 'bf16').eval()
    with torch.no_grad():
        logits = net(*_inputs(fx)).float().cpu()
    err = float((logits.double() - T(fx['eval_logits']).double()).abs().max())
    allow = float(fx['ref_bf16_storage_vs_f32_maxabs'])
    print(name, 'bf16 eval max abs err %.3e, recorded storage error %.3e, ratio %.2f' % (err, allow, err / allow))
    assert err <= BF16_MARGIN * allow, (err, allow)


@pytest.mark.parametrize('name,with_depth', FIXTURES[:2])
def test_bf16_training_step_runs_and_tracks_fp32(name, with_depth, deterministic_sums):
    """bf16 storage of x, y, the activation and its gradient: the loss stays within 1e-2 of the reference's (the bound
    test_gpu_fused_step.py applies to a whole U-Net in bf16), every live gradient points the reference's way (cosine > 0.99), and two runs
    under the fixed summation order are bit-identical."""
    fx = golden(name)
    out, loss, grads, post = _train_step(fx, with_depth, 'bf16')
    ref = float(fx['train_loss'])
    assert abs(loss - ref) <= 1e-2 * max(1.0, abs(ref)), (loss, ref)
    for k in fx['param_names'].tolist():
        if k in fx['zero_grad_names'].tolist():
            continue
        a, b = grads[k].double().reshape(-1), T(fx['fullgrad:' + k]).double().reshape(-1)
        cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
        print('  %-40s cosine %.5f' % (k, cos))
        assert cos > 0.99, (k, cos)
    out2, loss2, grads2, _ = _train_step(fx, with_depth, 'bf16')
    assert torch.equal(out, out2) and loss == loss2 and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ------------------------------------------------------------------------------------------------ trainer / inference surface
def _model(with_depth, dtype='f32', lr=1e-3, cfg=None, epochs=1, **extra):
    return NC.family_model('StackingFCNWithDepth' if with_depth else 'StackingFCN', dtype, lr, epochs, cfg, **dict({'input_model_nr': 5}, **extra))


def _stacks(n, seed, size=32):
    """n synthetic stacks of 5 first-level probability maps: a disc mask seen through five noisy 'models' -> (X [n,5,s,s], T [n,2,s,s])"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing='ij')
    M = torch.zeros(n, 1, size, size)
    for i in range(n):
        if i % 3 == 0:
            continue
        cy, cx, r = [int(v) for v in torch.randint(size // 4, 3 * size // 4, (3,), generator=g)]
        M[i, 0] = (((yy - cy) ** 2 + (xx - cx) ** 2) < max(r // 2, 3) ** 2).float()
    X = torch.sigmoid(4.0 * (M - 0.5) + torch.randn(n, 5, size, size, generator=g))
    return X, torch.cat([1 - M, M], 1)


@pytest.mark.parametrize('with_depth', [False, True], ids=['StackingFCN', 'StackingFCNWithDepth'])
def test_fit_transform_persist_load(with_depth, tmp_path):
    ck = str(tmp_path / 'ck' / 'best.torch')
    cfg = {'model_checkpoint': {'filepath': ck, 'epoch_every': 1, 'metric_name': 'iout', 'minimize': False},
           'training_monitor': {'batch_every': 0, 'epoch_every': 1}, 'experiment_timing': {'batch_every': 0, 'epoch_every': 1},
           'validation_monitor': {'epoch_every': 1, 'data_dir': None, 'loader_mode': 'stacking', 'use_depth': with_depth},
           'early_stopping': {'patience': 20, 'metric_name': 'iout', 'minimize': False}}
    torch.manual_seed(0)
    m = _model(with_depth, cfg=cfg, epochs=2)
    Xt, Mt = _stacks(8, 1)
    Xv, Mv = _stacks(4, 2)
    g = torch.Generator().manual_seed(4)
    Dt, Dv = torch.rand(8, 1, generator=g), torch.rand(4, 1, generator=g)

    def batches(X, D, M):
        return [[X[i:i + 4]] + ([D[i:i + 4]] if with_depth else []) + [M[i:i + 4]] for i in range(0, X.shape[0], 4)]
    train, valid = (batches(Xt, Dt, Mt), 1), (batches(Xv, Dv, Mv), 0)          # 2 epochs x 2 steps
    m.fit(train, valid)
    assert m.optimizer.steps == 4 and sorted(m.validation_loss) == [0, 1]
    for v in m.validation_loss.values():
        assert set(v) == {'sum', 'iou', 'iout'} and all(torch.isfinite(x).all() for x in v.values())
    m.persist(ck)
    out = m.transform(valid)['mask_prediction']
    assert len(out) == 4 and out[0].shape == (2, 32, 32) and all(0.0 <= float(p.min()) and float(p.max()) <= 1.0 for p in out)
    m2 = _model(with_depth).load(ck)
    for p, q in zip(out, m2.transform(valid)['mask_prediction']):
        assert np.array_equal(p, q)
    if with_depth:
        other = ([[Xv, Dv.flip(0), Mv]], 0)
        assert not np.array_equal(m.transform(other)['mask_prediction'][0], out[0])


@pytest.mark.parametrize('with_depth', [False, True], ids=['StackingFCN', 'StackingFCNWithDepth'])
def test_step_graph_replay_equals_eager_steps(with_depth, deterministic_sums):
    """tests/test_gpu_fused_step.py::test_step_graph_replay_equals_eager_steps on the stacking networks: the same comparison (with the
    state dicts and the step count, which tests/net_checks.py::step_graph_equals_eager does not compare), bit for bit."""
    results = {}
    for mode in ('eager', 'graph'):
        torch.manual_seed(11)
        m = _model(with_depth, dtype='bf16')
        m.step_graph = mode == 'graph'
        m._to_device()
        m.model.train()
        X, Tt = _stacks(4, 5)
        D = torch.tensor([[0.1], [0.4], [0.6], [0.9]])
        ls = [float(m._fit_loop([X * (1 - 0.05 * i)] + ([D] if with_depth else []) + [Tt])['sum']) for i in range(3)]
        torch.cuda.synchronize()
        eng = m.model.engine()
        sd = {k: v.detach().clone() for k, v in m.model.state_dict().items()}
        results[mode] = (ls, eng.flat.clone(), eng.grads.clone(), sd, m.optimizer.steps,
                         sum(len(n.__dict__.get('_step_graphs', {})) for n in eng.nets.values()))
    assert results['graph'][5] == 1 and results['eager'][5] == 0
    assert results['eager'][4] == results['graph'][4] == 3
    assert len(set(results['eager'][0])) == 3 and results['eager'][0] == results['graph'][0]
    assert torch.equal(results['eager'][2], results['graph'][2]) and torch.equal(results['eager'][1], results['graph'][1])
    for k, v in results['eager'][3].items():
        assert torch.equal(v, results['graph'][3][k]), k


def test_fused_step_reads_a_resident_batch_in_place(deterministic_sums):
    """the op's input pointer is re-pointed by CompiledNet.bind like conv_first's: a resident contiguous batch and a batch-sliced view
    (copied into the static buffer) give the same bits"""
    res = []
    for mode in ('bound', 'views'):
        torch.manual_seed(3)
        m = _model(False)
        m._to_device()
        m.model.train()
        X, Tt = _stacks(8, 7)
        ls = []
        for i in range(2):
            sl = slice(4 * i, 4 * i + 4)
            Xd = X.double().to(DEV)[sl] if mode == 'views' else X[sl].clone().to(DEV)
            ls.append(float(m._fit_loop([Xd, Tt[sl].clone().to(DEV)])['sum']))
        net = m.model.engine().net((4, 5, 32, 32), True)
        assert len(net.slots('x')) >= 1
        res.append((ls, m.model.engine().flat.clone()))
    assert res[0][0] == res[1][0] and len(set(res[0][0])) == 2 and torch.equal(res[0][1], res[1][1])


def test_predict_tta_takes_an_m_channel_batch():
    from salt_amd import inference as I
    fx = golden('F16_stacking_fcn')
    net = _net(fx, False).eval()
    X = T(fx['x']).to(DEV)
    prob = I.predict_tta(net, X, flip_lr=True).cpu()
    with torch.no_grad():
        a = torch.sigmoid(net(X).float())
        b = torch.flip(torch.sigmoid(net(torch.flip(X, [3]).contiguous()).float()), [3])
    assert tuple(prob.shape) == (2, 2, 19, 37)
    assert float((prob - ((a + b) / 2).cpu()).abs().max()) <= 1e-6
