"""GPU parity tests (through the C-ABI): HIP blocks vs the golden vectors the reference produced, and vs the
oracle on seeded inputs.  Tolerance: fp32 outputs/gradients <= 1e-3 relative to the tensor's max magnitude
(north_star's forward tolerance; measured errors are ~1e-6); bf16 compute <= 3e-2."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, T, assert_close, rel_err, state_from_fixture
from gpu_harness import BLOCKS, _fixture_state, _mods

pytestmark = pytest.mark.gpu

TOL32 = 5e-5
TOLBF = 4e-2


def _emulated_bf16_grads(name, fx):
    """gradients of the ORACLE block with bf16 storage emulated (inputs, activations, their gradients, packed weights) on a fixture's
    inputs and closed-form state: {'gx': .., 'ge0': .., 'g:<param>': ..} - the yardstick of the bf16 backward bound below"""
    from helpers import ORACLE_BLOCKS as OBLOCKS, oracle_run as orun
    from oracle import blocks as OB
    sd = state_from_fixture(fx)
    extras = [T(fx['e0'])] if 'e0' in fx else []
    with OB.bf16_storage():
        fn = OBLOCKS[name](sd, True)
        x, ex, leaves, y = orun(lambda *a: fn(*[OB._st(t) for t in a]), sd, T(fx['x']), extras)
        y.backward(T(fx['gy']))
    out = {'gx': x.grad}
    for i, e in enumerate(ex):
        out['ge%d' % i] = e.grad
    for k, v in leaves.items():
        out['g:' + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return out


@pytest.mark.parametrize('name', sorted(BLOCKS))
@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_block_vs_reference_golden(name, mode, dtype):
    from gpu_harness import BlockRun, load_into
    A = _mods()
    fx = golden('%s_%s' % (name, mode))
    make, emit = BLOCKS[name]
    m = make(A)
    load_into(m, _fixture_state(fx, m))
    inputs = [T(fx['x'])] + ([T(fx['e0'])] if 'e0' in fx else [])
    train = mode == 'train'
    m.train(train)
    run = BlockRun(m, inputs, emit(m), train=True if train else False, dtype=dtype)
    tol = TOL32 if dtype == 'f32' else TOLBF
    y = run.forward()
    assert_close(y, fx['y'], tol, 'y')
    if not train:
        return
    gx, grads = run.backward(T(fx['gy']).to('cuda:0'))
    if dtype == 'f32':
        gtol, emu = tol * 2, None
    else:
        # bf16: these fixtures are tiny (<= 200 samples per BatchNorm channel), the BN backward's cancellations
        # amplify storage rounding - so the bound is EARNED per tensor: the oracle re-run with bf16 storage emulated at the HIP path's
        # tensor boundaries (oracle.blocks.bf16_storage) sits e_emu from the golden; the HIP path may sit at most 1.5 e_emu + 2e-2
        gtol, emu = None, _emulated_bf16_grads(name, fx)

    def check(got, ref, key, f32_tol):
        if emu is None:
            assert_close(got, ref, f32_tol, key)
        else:
            e_hip, e_emu = rel_err(got, ref), rel_err(emu[key], ref)
            assert e_hip <= 1.5 * e_emu + 2e-2, '%s: HIP bf16 %.3e from the golden, bf16-storage emulation %.3e' % (key, e_hip, e_emu)
    check(gx[0], fx['gx'], 'gx', gtol)
    if 'e0' in fx:
        check(gx[1], fx['ge0'], 'ge0', gtol)
    gscale = max(float(np.abs(fx['g:' + k]).max()) for k in grads)
    for k, g in grads.items():
        ref = fx['g:' + k]
        if float(g.abs().max()) == 0.0:
            # conv / deconv bias in front of train-mode BN: analytically zero; the reference holds rounding noise
            assert np.abs(ref).max() < 1e-4 * gscale, (k, np.abs(ref).max(), gscale)
        else:
            check(g, ref, 'g:' + k, tol * 3)
    sd = m.state_dict()
    for k in sd:
        if k.endswith(('running_mean', 'running_var')):
            assert_close(sd[k].cpu(), fx['s:' + k], tol, k)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


CONV_CASES = [
    # (B, Cin, H, W, Cout, k, stride, pad)   dense nn.Conv2d as used by the ResNet encoders / decoders
    (2, 16, 9, 11, 24, 3, 1, 1),
    (2, 64, 16, 16, 64, 3, 1, 1),
    (1, 40, 33, 17, 72, 3, 1, 1),
    (2, 32, 16, 16, 64, 3, 2, 1),
    (2, 32, 15, 13, 48, 3, 2, 1),
    (2, 64, 8, 8, 128, 1, 2, 0),
    (2, 96, 8, 8, 32, 1, 1, 0),
    (2, 128, 8, 8, 64, 1, 1, 0),      # 1x1 with Cin a multiple of 4 chunks: virtual-tap path (Bottleneck convs of ResNet101/152)
    (2, 256, 9, 7, 96, 1, 1, 0),
    (1, 512, 20, 12, 40, 1, 1, 0),
    (3, 128, 4, 4, 256, 3, 1, 1),
    (4, 256, 2, 2, 128, 3, 1, 1),
    (2, 13, 7, 5, 10, 3, 1, 1),       # ragged channels: scalar load path
    (2, 96, 33, 17, 96, 3, 1, 1),     # whole 64-byte chunks (conv_glds_kernel eligible fwd + dgrad), ragged grid, Cout = 1.5 channel tiles
    (5, 160, 8, 8, 64, 3, 1, 1),      # 8x8 maps: several images per pixel tile, partial batch tile
]


@pytest.mark.parametrize('case', CONV_CASES)
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('cfg', [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_conv_fwd_dgrad_wgrad_vs_torch(case, dtype, cfg):
    """Raw conv (no BN): forward, data gradient and weight gradient vs torch CPU fp32, every tile config."""
    from gpu_harness import BlockRun
    from torch import nn
    B, Cin, H, W, Cout, k, s, p = case
    if cfg == 2 and s == 2:
        pytest.skip('256-pixel tiles are not used for stride 2')
    conv = nn.Conv2d(Cin, Cout, k, s, p, bias=False)
    bn = nn.BatchNorm2d(Cout)
    mod = nn.Sequential(conv, bn)
    with torch.no_grad():
        conv.weight.copy_(_rand(conv.weight.shape, 1, (2.0 / (Cin * k * k)) ** 0.5))
        bn.weight.copy_(1 + 0.1 * _rand((Cout,), 2)); bn.bias.copy_(0.1 * _rand((Cout,), 3))
    x = _rand((B, Cin, H, W), 4)
    if dtype == 'bf16':
        x = x.bfloat16().float()

    def emit(g, a):
        # force the tile config through the plan override
        orig = g._conv_launch

        def launch(*args, **kw):
            kw.setdefault('cfg', cfg)
            return orig(*args, **kw)
        g._conv_launch = launch
        orig_parts = g._conv_parts
        g._conv_parts = lambda *a_, **k_: orig_parts(*a_, cfg=cfg, **k_)
        return g.conv(a, conv, bn, relu=True)

    mod.train()
    try:
        run = BlockRun(mod, [x], emit, train=True, dtype=dtype)
    except Exception as e:
        if 'too large' in str(e) or 'LDS' in str(e):
            pytest.skip(str(e))
        raise
    y = run.forward()
    # oracle
    ref_conv = nn.Conv2d(Cin, Cout, k, s, p, bias=False)
    ref_bn = nn.BatchNorm2d(Cout)
    with torch.no_grad():
        w = conv.weight.detach().cpu()
        ref_conv.weight.copy_(w.bfloat16().float() if dtype == 'bf16' else w)
        ref_bn.weight.copy_(bn.weight.detach().cpu()); ref_bn.bias.copy_(bn.bias.detach().cpu())
    xr = x.clone().requires_grad_(True)
    yr = F.relu(ref_bn(ref_conv(xr)))
    tol = TOL32 if dtype == 'f32' else TOLBF
    assert_close(y, yr, tol, 'y')
    gy = _rand(tuple(yr.shape), 5)
    yr.backward(gy)
    gx, grads = run.backward(gy.to('cuda:0'))
    if dtype == 'f32':
        assert_close(gx[0], xr.grad, tol * 2, 'dgrad')
    else:
        # bf16 rounding of y flips the ReLU mask of the few outputs that sit within 2^-8 of zero; each flip moves one pixel's
        # gradient by O(|g w|), which a max-norm over a large tensor always catches.  The L2 norm is the meaningful statistic.
        d, r = gx[0].double(), xr.grad.double()
        l2 = float((d - r).norm() / r.norm())
        assert l2 <= tol, 'dgrad: rel-L2 %.3e > %.1e' % (l2, tol)
    if dtype == 'f32':
        assert_close(grads['0.weight'], ref_conv.weight.grad, tol * 3, 'wgrad')
    else:
        d, r = grads['0.weight'].double(), ref_conv.weight.grad.double()
        l2 = float((d - r).norm() / r.norm())
        assert l2 <= tol, 'wgrad: rel-L2 %.3e > %.1e' % (l2, tol)
    assert_close(grads['1.weight'], ref_bn.weight.grad, tol * 3, 'dgamma')
    assert_close(grads['1.bias'], ref_bn.bias.grad, tol * 3, 'dbeta')


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_pool_and_upsample_vs_golden(dtype):
    from gpu_harness import BlockRun
    from torch import nn
    fx = golden('F5_pool_upsample')
    tol = 1e-6 if dtype == 'f32' else 1e-2
    dummy = nn.Linear(1, 1)
    x = T(fx['x'])
    for tag, op in (('max2', 'maxpool2'), ('avg2', 'avgpool2')):
        run = BlockRun(dummy, [x], lambda g, a, op=op: getattr(g, op)(a), train=True, dtype=dtype)
        assert_close(run.forward(), fx[tag + '_y'], tol, tag)
        gx, _ = run.backward(T(fx[tag + '_gy']).to('cuda:0'))
        assert_close(gx[0], fx[tag + '_gx'], max(tol, 1e-6), tag + ' grad')
    for r in (2, 4, 8, 16):
        run = BlockRun(dummy, [T(fx['xb'])], lambda g, a, r=r: g.upsample(a, r), train=True, dtype=dtype)
        assert_close(run.forward(), fx['up%d_y' % r], max(tol, 2e-6), 'up%d' % r)
        gx, _ = run.backward(T(fx['up%d_gy' % r]).to('cuda:0'))
        assert_close(gx[0], fx['up%d_gx' % r], max(tol, 1e-5), 'up%d grad' % r)


def test_first_layer_conv_vs_torch():
    """salt_conv_first (+BN+ReLU) and its weight gradient: ResNet stem 7x7 s2 p3 and a 1-channel 3x3."""
    from gpu_harness import DEV
    from salt_amd.engine import Graph
    from salt_amd.runtime import Engine
    from torch import nn
    for (B, Cin, H, W, Cout, K, s, p) in [(2, 3, 32, 32, 64, 7, 2, 3), (2, 1, 19, 21, 16, 3, 1, 1), (1, 3, 40, 24, 64, 7, 2, 3)]:
        conv = nn.Conv2d(Cin, Cout, K, s, p, bias=(K == 3))
        bn = nn.BatchNorm2d(Cout)
        mod = nn.Sequential(conv, bn).to(DEV)
        eng = Engine(mod, torch.device(DEV), 'f32')
        g = Graph(eng, True)
        x = _rand((B, Cin, H, W), 7)
        xd = g.alloc(tuple(x.shape), torch.float32); xd.copy_(x)
        a = g.conv_first(xd, conv, bn, relu=True)
        out = g.alloc((a.B, a.C, a.H, a.W), torch.float32)
        g.to_nchw(a, out)
        g.build_backward(); g.finalize()
        eng.refresh(True); g.fwd.run()
        rc, rb = nn.Conv2d(Cin, Cout, K, s, p, bias=(K == 3)), nn.BatchNorm2d(Cout)
        rc.load_state_dict({k: v.cpu() for k, v in conv.state_dict().items()})
        yr = F.relu(rb(rc(x)))
        assert_close(out.cpu(), yr, TOL32, 'conv_first y')
        gy = _rand(tuple(yr.shape), 8)
        yr.backward(gy)
        g.dlogits.copy_(gy); g.bwd.run(); torch.cuda.synchronize()
        off, n = eng.grad_range(conv.weight)
        assert_close(eng.grads[off:off + n].view(conv.weight.shape).cpu(), rc.weight.grad, 3e-3, 'conv_first wgrad')
        assert_close(bn.running_var.cpu(), rb.running_var, 1e-4, 'running_var')


@pytest.mark.parametrize('case', [(2, 16, 20, 24, 24), (1, 64, 16, 16, 64), (3, 32, 8, 8, 40), (2, 24, 33, 19, 16), (5, 32, 2, 2, 16), (3, 16, 4, 3, 24),
                                  (3, 16, 9, 18, 24)])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('replicate', [True, False])
@pytest.mark.parametrize('fin', [2, 1, 0])
def test_two_conv_bn_relu_layers_vs_torch(case, dtype, replicate, fin, monkeypatch):
    """fin (SALT_BN_FIN): 2 = fp64 shard atomics in the producing launch, finalized by the consumer (salt_affine_act / the apply pass of
    salt_bn_bwd); 1 = the same shards finalized in the producing launch by the last-arriving workgroup (salt_conv_args.fin / bnb_fin);
    0 = per-tile partials and separate salt_bn_finalize / bn_bwd finalize launches.
    Two stacked 3x3 conv + BN + ReLU layers against torch CPU fp32: forward, data gradient, weight and BN gradients.
    replicate: the reference's replicate top/right padding (architectures/base.py:21-27) - fold-mode data gradient and the
    pipelined weight-gradient kernel's clamp loader on ragged tiles.  Zero padding: the second layer's data gradient is the only
    writer of dL/d(first activation), so its epilogue must also produce the first layer's BatchNorm-backward sums
    (salt_conv_args.bnb_*; checked on the emitted program)."""
    from gpu_harness import BlockRun
    from torch import nn
    monkeypatch.setenv('SALT_BN_FIN', str(fin))
    B, Cin, H, W, Cmid = case
    Cout = Cmid + 8
    c1, b1, c2, b2 = nn.Conv2d(Cin, Cmid, 3, 1, 0, bias=False), nn.BatchNorm2d(Cmid), nn.Conv2d(Cmid, Cout, 3, 1, 0, bias=False), nn.BatchNorm2d(Cout)
    mod = nn.Sequential(c1, b1, c2, b2)
    with torch.no_grad():
        c1.weight.copy_(_rand(c1.weight.shape, 11, (2.0 / (Cin * 9)) ** 0.5)); c2.weight.copy_(_rand(c2.weight.shape, 12, (2.0 / (Cmid * 9)) ** 0.5))
        for i, b in enumerate((b1, b2)):
            b.weight.copy_(1 + 0.1 * _rand(b.weight.shape, 13 + i)); b.bias.copy_(0.1 * _rand(b.bias.shape, 15 + i))
    x = _rand((B, Cin, H, W), 17)
    if dtype == 'bf16':
        x = x.bfloat16().float()
    ref = nn.Sequential(nn.Conv2d(Cin, Cmid, 3, 1, 0, bias=False), nn.BatchNorm2d(Cmid), nn.Conv2d(Cmid, Cout, 3, 1, 0, bias=False), nn.BatchNorm2d(Cout))
    ref.load_state_dict({k: v.clone() for k, v in mod.state_dict().items()})
    if dtype == 'bf16':
        with torch.no_grad():
            ref[0].weight.copy_(ref[0].weight.bfloat16().float()); ref[2].weight.copy_(ref[2].weight.bfloat16().float())

    if not replicate:
        c1.padding = c2.padding = (1, 1)

    def emit(g, a):
        h = g.conv(a, c1, b1, relu=True, replicate=replicate)
        return g.conv(h, c2, b2, relu=True, replicate=replicate)

    mod.train()
    run = BlockRun(mod, [x], emit, train=True, dtype=dtype)
    y = run.forward()
    xr = x.clone().requires_grad_(True)
    pad = (lambda t: F.pad(t, (0, 2, 2, 0), mode='replicate')) if replicate else (lambda t: F.pad(t, (1, 1, 1, 1)))   # l, r, t, b
    hr = F.relu(ref[1](ref[0](pad(xr))))
    yr = F.relu(ref[3](ref[2](pad(hr))))
    tol = TOL32 if dtype == 'f32' else TOLBF
    assert_close(y, yr, tol * (1 if dtype == 'f32' else 2), 'y')
    gy = _rand(tuple(yr.shape), 18)
    yr.backward(gy)
    gx, grads = run.backward(gy.to('cuda:0'))
    ready = [int(st.partials_ready) for name, _, st in run.g.bwd.ops if name == 'bn_bwd']
    # the data-gradient launch of layer 2 completes dL/d(a1) - also for the replicate-padded variant, whose pad-ring fold is fused
    # into the launch's epilogue - so it carries layer 1's BatchNorm-backward sums whenever the channel pieces are whole
    fusable = Cmid % (4 if dtype == 'f32' else 8) == 0
    assert ready == [0, {2: 3, 1: 2, 0: 1}[fin] if fusable else 0], ready  # backward order: layer 2, then layer 1
    assert sum(1 for name, _, _ in run.g.fwd.ops if name == 'bn_finalize') == (0 if fin else 2)
    pairs = [('dgrad', gx[0], xr.grad)] + [(k, grads[k], dict(ref.named_parameters())[k].grad) for k in grads]
    for name, got, want in pairs:
        if dtype == 'f32':
            assert_close(got, want, tol * 4, name)
        else:
            l2 = float((got.double() - want.double()).norm() / want.double().norm())
            assert l2 <= 2 * tol, '%s: rel-L2 %.3e' % (name, l2)
    for i, b in ((1, b1), (3, b2)):                                  # running statistics (the in-launch finalize writes them too)
        assert_close(b.running_mean.cpu(), ref[i].running_mean, tol * (1 if dtype == 'f32' else 2), 'running_mean')
        assert_close(b.running_var.cpu(), ref[i].running_var, tol * (1 if dtype == 'f32' else 2), 'running_var')
        assert int(b.num_batches_tracked) == 1
    # a second forward through the same program: the accumulators and tickets were left zero
    y2 = run.forward()
    assert torch.equal(y2, y) or float((y2.float() - y.float()).abs().max()) <= 1e-6 * float(y.float().abs().max())


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 16, 12, 10), (1, 8, 7, 9), (3, 5, 16, 16)])
def test_maxpool3s2_with_ties_vs_torch(dtype, shape):
    """nn.MaxPool2d(3, 2, 1) (the pool0 stem pool): forward and the first-maximum gradient routing through overlapping windows, on
    small-integer inputs (many ties) and odd sizes."""
    from gpu_harness import BlockRun
    from torch import nn
    B, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
    mod = nn.Sequential(nn.Conv2d(1, 1, 1))                      # BlockRun wants a module with parameters
    run = BlockRun(mod, [x], lambda gr, a: gr.maxpool3s2(a), train=True, dtype=dtype)
    y = run.forward()
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    assert torch.equal(y, yr.detach())
    gy = torch.randint(-3, 4, tuple(yr.shape), generator=g).float()
    yr.backward(gy)
    gx, _ = run.backward(gy.to('cuda:0'))
    assert torch.equal(gx[0], xr.grad)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_scse_kernels_vs_channel_and_spatial_se_goldens(dtype):
    """se.hip alone: the fused cSE + sSE + ReLU operator against the reference's STANDALONE ChannelSELayer / SpatialSELayer
    goldens (architectures/base.py:89-117, fixtures F4_channel_se / F4_spatial_se share their input).  Forward: the fused output must be
    relu(y_cSE + y_sSE) of the two golden outputs.  Backward: the reference holds the two Jacobians at its own upstream gradient, not
    at the ReLU-masked one, so the gradients are compared with the oracle's composition of the two layers, which
    tests/test_oracle_golden.py pins against the very same fixtures (forward and backward)."""
    from torch import nn
    from gpu_harness import BlockRun
    from oracle import blocks as OB
    A = _mods()
    fc, fs = golden('F4_channel_se_train'), golden('F4_spatial_se_train')
    assert np.array_equal(fc['x'], fs['x'])
    C = fc['x'].shape[1]

    class Both(nn.Module):
        def __init__(self):
            super().__init__()
            self.channel_se = A.ChannelSELayer(C, reduction=16)
            self.spatial_se = A.SpatialSELayer(C)
    m = Both()
    sd = {'channel_se.' + k[2:]: T(v) for k, v in fc.items() if k.startswith('s:')}
    sd.update({'spatial_se.' + k[2:]: T(v) for k, v in fs.items() if k.startswith('s:')})
    m.load_state_dict(sd)
    x = T(fc['x'])
    if dtype == 'bf16':
        x = x.bfloat16().float()
    run = BlockRun(m, [x], lambda g, a: g.scse(a, m.channel_se, m.spatial_se), train=True, dtype=dtype)
    y = run.forward()
    tol = TOL32 if dtype == 'f32' else 1e-2
    if dtype == 'f32':
        assert_close(y, np.maximum(fc['y'] + fs['y'], 0.0), tol, 'y vs the two goldens')
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    yr = torch.relu(OB.channel_se(leaves, 'channel_se.', xr) + OB.spatial_se(leaves, 'spatial_se.', xr))
    assert_close(y, yr.detach(), tol, 'y vs oracle')
    gy = T(fc['gy'])
    yr.backward(gy)
    gx, grads = run.backward(gy.to('cuda:0'))
    gtol = tol * 2 if dtype == 'f32' else 3e-2
    assert_close(gx[0], xr.grad, gtol, 'gx')
    for k, g in grads.items():
        assert_close(g, leaves[k].grad, gtol * 2, 'g:' + k)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_backward_program_is_idempotent_without_a_fresh_forward(dtype):
    """the BatchNorm-backward fp64 shards are accumulate-only and cleared by the FORWARD program's salt_zero; a backward
    program that runs twice behind ONE forward pass (loss.backward(retain_graph=True) through autograd.py, a second loss, the timed /
    debug runs of the tools) must clear its own half first (Graph.finalize: 'backward shards dirty' flag) instead of doubling the sums."""
    from gpu_harness import BlockRun, load_into
    A = _mods()
    fx = golden('F4_decoderblock_skip_train')
    make, emit = BLOCKS['F4_decoderblock_skip']
    m = make(A)
    load_into(m, _fixture_state(fx, m))
    m.train(True)
    run = BlockRun(m, [T(fx['x']), T(fx['e0'])], emit(m), train=True, dtype=dtype)
    run.forward()
    gy = T(fx['gy']).to('cuda:0')
    tol = 1e-4 if dtype == 'f32' else 2e-2          # (a doubled sum is an O(1) error; the fp64 atomics' arrival order is last bits)
    gx1, g1 = run.backward(gy)
    st = run.g._shard_state
    assert st is not None and st['dirty'] and st['rezeroed'] == 0
    gx2, g2 = run.backward(gy)                       # no forward in between
    assert st['rezeroed'] == 1
    timed = run.g.bwd.run_timed()                    # the tools' path
    torch.cuda.synchronize()
    assert st['rezeroed'] == 2 and len(timed) == len(run.g.bwd)
    gx3 = [t.cpu() for t in run.g.input_grads]
    for a, b, c in zip(gx1, gx2, gx3):
        assert_close(b, a, tol, 'dx after a second backward')
        assert_close(c, a, tol, 'dx after a timed backward')
    for k in g1:
        assert_close(g2[k], g1[k], tol, k)
    run.forward()
    assert not st['dirty']
    gx4, _ = run.backward(gy)
    assert st['rezeroed'] == 2
    assert_close(gx4[0], gx1[0], tol, 'dx after forward + backward')


@pytest.mark.parametrize('B', [51, 64, 130])
def test_scse_backward_batch_tiles_c256(B):
    """se_fc_bwd_kernel is ONE workgroup whose per-image vectors had to fit 160 KB of LDS - C = 256 (the ResNet101 / 152
    decoders, architectures/base.py:82-117) failed with SALT_E_LDS above 51 images per GPU, i.e. at BASELINE C3's batch 64.  Round 6
    walks the batch in tiles of (160 KiB - 2 R C 4) / ((3 C + 2 R + 1) 4) = 40 images at C = 256, R = 16 (launch_se_fc); 51 still runs as
    ONE tile (the old path), 64 as 40 + 24, 130 as four tiles (40 + 40 + 40 + 10) - all against the oracle's
    composition of ChannelSELayer and SpatialSELayer (pinned by fixtures F4_channel_se / F4_spatial_se in tests/test_oracle_golden.py)."""
    from torch import nn
    from gpu_harness import BlockRun
    from oracle import blocks as OB
    A = _mods()
    C = 256

    class Both(nn.Module):
        def __init__(self):
            super().__init__()
            self.channel_se = A.ChannelSELayer(C, reduction=16)
            self.spatial_se = A.SpatialSELayer(C)
    torch.manual_seed(B)
    m = Both()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = _rand((B, C, 8, 8), 31)
    run = BlockRun(m, [x], lambda g, a: g.scse(a, m.channel_se, m.spatial_se), train=True, dtype='f32')
    y = run.forward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    yr = torch.relu(OB.channel_se(leaves, 'channel_se.', xr) + OB.spatial_se(leaves, 'spatial_se.', xr))
    assert_close(y, yr.detach(), TOL32, 'y vs oracle')
    gy = _rand(tuple(yr.shape), 32)
    yr.backward(gy)
    gx, grads = run.backward(gy.to('cuda:0'))
    assert_close(gx[0], xr.grad, TOL32 * 2, 'gx')
    for k, g in grads.items():
        assert_close(g, leaves[k].grad, TOL32 * 4, 'g:' + k)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 16, 16, 16, 32), (3, 32, 8, 12, 64)])
def test_projection_block_input_gradient_carries_bn_backward_sums(dtype, shape, monkeypatch):
    """layerN.0 of the ResNet encoders (torchvision BasicBlock with a 1x1 stride-2 projection shortcut, architectures/encoders.py:38-45)
    behind a Conv-BN-ReLU producer.  Round 6: the shortcut's backward is emitted BEFORE conv1's, so the LAST writer of dL/dx is conv1's
    phase-fused stride-2 data gradient - every pixel once - and it carries the BatchNorm-backward sums of x's producer
    (salt_conv_args.bnb_* on an nphase = 4 launch): that layer's bn_bwd runs without its reduction pass.  Values against torch autograd;
    SALT_NO_SHORTCUT_FIRST=1 restores round 5's order (reduction pass in bn_bwd) and must give the same gradients."""
    from gpu_harness import BlockRun
    from torch import nn
    A = _mods()
    B, Cin, H, W, planes = shape
    torch.manual_seed(7)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv0 = nn.Conv2d(Cin, Cin, 3, 1, 1, bias=False)
            self.bn0 = nn.BatchNorm2d(Cin)
            down = nn.Sequential(nn.Conv2d(Cin, planes, 1, 2, bias=False), nn.BatchNorm2d(planes))
            self.block = A.BasicBlock(Cin, planes, 2, down)
    m = Net()
    with torch.no_grad():
        for p_ in m.parameters():
            if p_.dim() == 1:
                p_.copy_(1 + 0.2 * torch.randn_like(p_))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = _rand((B, Cin, H, W), 41)
    gy = _rand((B, planes, H // 2, W // 2), 42)
    results = {}
    for mode in ('shortcut_first', 'round5'):
        if mode == 'round5':
            monkeypatch.setenv('SALT_NO_SHORTCUT_FIRST', '1')
        m.load_state_dict(sd)
        m.train()

        def emit(g, a):
            h = g.conv(a, m.conv0, m.bn0, relu=True)
            return m.block.emit(g, h)
        run = BlockRun(m, [x], emit, train=True, dtype=dtype)
        y = run.forward()
        gx, grads = run.backward(gy.to('cuda:0'))
        ready = [int(st.partials_ready) for name, _, st in run.g.bwd.ops if name == 'bn_bwd']
        nph = [int(st.nphase) for name, _, st in run.g.bwd.ops if name == 'conv' and st.bnb_y.p]
        results[mode] = (y, gx[0], grads, ready, nph)
    fusable = Cin % (4 if dtype == 'f32' else 8) == 0
    # backward order of the bn_bwd operators: block.bn2 (reduce: its da comes from the harness' layout op), [downsample.bn | block.bn1], bn0
    assert results['shortcut_first'][3][-1] == (3 if fusable else 0) and results['round5'][3][-1] == 0, (results['shortcut_first'][3], results['round5'][3])
    assert (4 in results['shortcut_first'][4]) == fusable and 4 not in results['round5'][4]
    # torch reference (fp32)
    ref = nn.ModuleDict(dict(conv0=nn.Conv2d(Cin, Cin, 3, 1, 1, bias=False), bn0=nn.BatchNorm2d(Cin), c1=nn.Conv2d(Cin, planes, 3, 2, 1, bias=False), b1=nn.BatchNorm2d(planes),
                             c2=nn.Conv2d(planes, planes, 3, 1, 1, bias=False), b2=nn.BatchNorm2d(planes), d=nn.Conv2d(Cin, planes, 1, 2, bias=False), db=nn.BatchNorm2d(planes)))
    mp = {'conv0': 'conv0', 'bn0': 'bn0', 'c1': 'block.conv1', 'b1': 'block.bn1', 'c2': 'block.conv2', 'b2': 'block.bn2', 'd': 'block.downsample.0', 'db': 'block.downsample.1'}
    ref.load_state_dict({a_ + k[len(b_):]: v for a_, b_ in mp.items() for k, v in sd.items() if k.startswith(b_ + '.')})
    ref.train()
    xr = x.clone().requires_grad_(True)
    h = F.relu(ref['bn0'](ref['conv0'](xr)))
    yr = F.relu(ref['b2'](ref['c2'](F.relu(ref['b1'](ref['c1'](h))))) + ref['db'](ref['d'](h)))
    yr.backward(gy)
    tol = TOL32 if dtype == 'f32' else TOLBF
    for mode in results:
        y, gx, grads = results[mode][:3]
        assert_close(y, yr, tol * (1 if dtype == 'f32' else 2), 'y ' + mode)
        if dtype == 'f32':
            assert_close(gx, xr.grad, tol * 8, 'dx ' + mode)
        else:
            l2 = float((gx.double() - xr.grad.double()).norm() / xr.grad.double().norm())
            assert l2 <= 3 * tol, (mode, l2)
    a, b = results['shortcut_first'], results['round5']
    for k in a[2]:
        if float(b[2][k].abs().max()) > 0:
            l2 = float((a[2][k].double() - b[2][k].double()).norm() / b[2][k].double().norm())
            assert l2 <= (1e-4 if dtype == 'f32' else 3e-2), (k, l2)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_projection_shortcut_bn_backward_sums_ride_on_the_main_branch_apply_pass(dtype, monkeypatch):
    """salt_bn_bwd_args.sec_* (round 6): in a residual block with a projection shortcut (torchvision BasicBlock, architectures/encoders.py:38-45)
    the shortcut BatchNorm's dL/da IS the masked gradient the main branch's bn_bwd stores as dres - so that apply pass also takes the
    shortcut layer's (sum, sum xhat) and the shortcut's bn_bwd loses its reduction pass.  Needs the main branch's sums to come from a
    convolution (a layer behind the block), as in the encoders.  Against torch autograd and against SALT_BNB_SEC=0."""
    from gpu_harness import BlockRun
    from torch import nn
    A = _mods()
    B, Cin, H, W, planes = 3, 16, 16, 16, 32
    torch.manual_seed(9)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            down = nn.Sequential(nn.Conv2d(Cin, planes, 1, 2, bias=False), nn.BatchNorm2d(planes))
            self.block = A.BasicBlock(Cin, planes, 2, down)
            self.tail = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
            self.tail_bn = nn.BatchNorm2d(planes)
    m = Net()
    with torch.no_grad():
        for p_ in m.parameters():
            if p_.dim() == 1:
                p_.copy_(1 + 0.2 * torch.randn_like(p_))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = _rand((B, Cin, H, W), 51)
    gy = _rand((B, planes, H // 2, W // 2), 52)
    results = {}
    for mode in ('sec', 'plain'):
        monkeypatch.setenv('SALT_BNB_SEC', '1' if mode == 'sec' else '0')
        m.load_state_dict(sd)
        m.train()
        run = BlockRun(m, [x], lambda g, a: g.conv(m.block.emit(g, a), m.tail, m.tail_bn, relu=True), train=True, dtype=dtype)
        y = run.forward()
        gx, grads = run.backward(gy.to('cuda:0'))
        bnb = [st for name, _, st in run.g.bwd.ops if name == 'bn_bwd']
        # backward order: tail_bn (reduce), block.bn2 (apply-only, sums from tail's data gradient), downsample.bn, block.bn1
        assert int(bnb[1].partials_ready) == 3 and bool(bnb[1].sec_acc) == (mode == 'sec'), [int(b.partials_ready) for b in bnb]
        assert int(bnb[2].partials_ready) == (3 if mode == 'sec' else 0)
        results[mode] = (y, gx[0], grads)
    ref = nn.ModuleDict(dict(c1=nn.Conv2d(Cin, planes, 3, 2, 1, bias=False), b1=nn.BatchNorm2d(planes), c2=nn.Conv2d(planes, planes, 3, 1, 1, bias=False),
                             b2=nn.BatchNorm2d(planes), d=nn.Conv2d(Cin, planes, 1, 2, bias=False), db=nn.BatchNorm2d(planes),
                             t=nn.Conv2d(planes, planes, 3, 1, 1, bias=False), tb=nn.BatchNorm2d(planes)))
    mp = {'c1': 'block.conv1', 'b1': 'block.bn1', 'c2': 'block.conv2', 'b2': 'block.bn2', 'd': 'block.downsample.0', 'db': 'block.downsample.1', 't': 'tail', 'tb': 'tail_bn'}
    ref.load_state_dict({a_ + k[len(b_):]: v for a_, b_ in mp.items() for k, v in sd.items() if k.startswith(b_ + '.')})
    ref.train()
    xr = x.clone().requires_grad_(True)
    blk = F.relu(ref['b2'](ref['c2'](F.relu(ref['b1'](ref['c1'](xr))))) + ref['db'](ref['d'](xr)))
    yr = F.relu(ref['tb'](ref['t'](blk)))
    yr.backward(gy)
    tol = TOL32 if dtype == 'f32' else TOLBF
    inv = {v: k for k, v in mp.items()}
    for mode, (y, gx, grads) in results.items():
        assert_close(y, yr, tol * (1 if dtype == 'f32' else 2), 'y ' + mode)
        l2 = float((gx.double() - xr.grad.double()).norm() / xr.grad.double().norm())
        assert l2 <= (1e-4 if dtype == 'f32' else 3 * tol), (mode, l2)
        for k, g_ in grads.items():
            mod_name, _, pname = k.rpartition('.')
            want = dict(ref[inv[mod_name]].named_parameters())[pname].grad
            if float(want.abs().max()) > 1e-6:
                l2 = float((g_.double() - want.double()).norm() / want.double().norm())
                assert l2 <= (2e-4 if dtype == 'f32' else 4 * tol), (mode, k, l2)
