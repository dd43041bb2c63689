"""conv_wgrad_ls_kernel (csrc/conv_wgrad_ls.hip: loader-specialised, row-streaming bf16 weight gradient) through the C-ABI
(tests/wgrad_abi.py): salt_conv_wgrad + salt_wgrad_reduce against torch's float64 weight gradient of the same bf16-rounded operands,
and against the kernels it replaced by default (csrc/conv_wgrad.hip, one child process with SALT_WGRAD_LS=0).  Replaces autograd of
common_blocks/models.py:133 over architectures/base.py:7-37 / unet_models.py:21-30."""
import os

import pytest
import torch
import torch.nn.functional as F

import wgrad_abi
from wgrad_abi import mk as _mk, wgrad_hip as _wgrad_hip

pytestmark = pytest.mark.gpu


def _ref(p, q, replicate):
    """p [B,Ca,H,W], q [B,Cb,H,W] fp32 (bf16-representable) -> dW [Ca][Cb][3][3] of the zero-pad-1 conv, or of the reference's
    ReplicationPad2d((0, 2, 2, 0)) + valid conv (architectures/base.py:21-27)."""
    w = torch.zeros(p.shape[1], q.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    qq = q.double()
    if replicate:
        y = F.conv2d(F.pad(qq, (0, 2, 2, 0), mode='replicate'), w)
    else:
        y = F.conv2d(qq, w, padding=1)
    (y * p.double()).sum().backward()
    return w.grad.float()


CASES = [
    # B, H, W, Ca, Cb
    (2, 16, 16, 64, 64),
    (1, 64, 64, 64, 64),       # one 64-row strip per column block
    (3, 33, 17, 72, 40),       # ragged rows / columns / channel blocks
    (2, 32, 32, 128, 192),     # several channel blocks: the XCD triple map
    (4, 8, 8, 128, 64),        # two images side by side in a k-step
    (5, 8, 8, 160, 72),        # ... odd batch, ragged channels
    (4, 4, 4, 64, 128),        # maps narrower than 8
    (3, 2, 2, 256, 64),
    (2, 128, 16, 32, 64),      # half-empty a-block, long strips
    (1, 9, 40, 64, 32),
]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('replicate', [False, True])
@pytest.mark.parametrize('ku', [4, 8])
def test_wgrad_ls_vs_torch(case, replicate, ku, monkeypatch):
    monkeypatch.setenv('SALT_WL_KU', str(ku))
    B, H, W, Ca, Cb = case
    p, q = _mk(B, Ca, H, W, 1), _mk(B, Cb, H, W, 2)
    taps = [(dy - 2, dx) for dy in range(3) for dx in range(3)] if replicate else [(dy - 1, dx - 1) for dy in range(3) for dx in range(3)]
    pd = p.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    qd = q.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    ref = _ref(p, q, replicate)
    got, ns = _wgrad_hip(pd, qd, taps, 1 if replicate else 0)
    err = float((got.double() - ref.double()).norm() / ref.double().norm())
    assert torch.isfinite(got).all()
    assert err <= 2e-5, 'rel-L2 %.3e (nsplit %d)' % (err, ns)          # exact products, fp32 accumulation in another order


@pytest.mark.parametrize('nsplit', [1, 3, 7, 40])
@pytest.mark.parametrize('ku', [4, 8])
def test_wgrad_ls_split_starts_mid_strip(nsplit, ku, monkeypatch):
    """Any split count: splits that begin inside a strip open with their own two-halo-row entry; splits beyond the last unit write
    zero slabs."""
    monkeypatch.setenv('SALT_WL_KU', str(ku))
    B, H, W, Ca, Cb = 2, 40, 24, 64, 64
    p, q = _mk(B, Ca, H, W, 3), _mk(B, Cb, H, W, 4)
    taps = [(dy - 1, dx - 1) for dy in range(3) for dx in range(3)]
    pd = p.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    qd = q.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    ref = _ref(p, q, False)
    got, _ = _wgrad_hip(pd, qd, taps, 0, nsplit=nsplit)
    err = float((got.double() - ref.double()).norm() / ref.double().norm())
    assert err <= 2e-5, 'rel-L2 %.3e' % err


@pytest.mark.parametrize('replicate', [False, True])
def test_wgrad_ls_strided_views_and_planar_q(replicate):
    """Channel slices of wider buffers (concat-free skips: pixel stride > channels) and the planar hypercolumn as Q."""
    B, H, W = 2, 32, 32
    Ca, Cb = 64, 128
    p, q = _mk(B, Ca, H, W, 5), _mk(B, Cb, H, W, 6)
    taps = [(dy - 2, dx) for dy in range(3) for dx in range(3)] if replicate else [(dy - 1, dx - 1) for dy in range(3) for dx in range(3)]
    ref = _ref(p, q, replicate)
    # strided: P lives in channels [16, 80) of a 96-channel buffer, Q in channels [8, 136) of a 160-channel buffer
    pbuf = torch.randn(B, H, W, 96).bfloat16().cuda()
    qbuf = torch.randn(B, H, W, 160).bfloat16().cuda()
    pbuf[..., 16:80] = p.permute(0, 2, 3, 1).bfloat16().cuda()
    qbuf[..., 8:136] = q.permute(0, 2, 3, 1).bfloat16().cuda()
    got, _ = _wgrad_hip(pbuf[..., 16:], qbuf[..., 8:], taps, 1 if replicate else 0, Ca=Ca, Cb=Cb)
    err = float((got.double() - ref.double()).norm() / ref.double().norm())
    assert err <= 2e-5, 'strided: rel-L2 %.3e' % err
    # planar: Q as two dense [B,H,W,64] planes
    planes = torch.stack([q[:, 0:64].permute(0, 2, 3, 1), q[:, 64:128].permute(0, 2, 3, 1)]).contiguous().bfloat16().cuda()
    pd = p.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    got, _ = _wgrad_hip(pd, planes.view(2 * B, H, W, 64)[:B], taps, 1 if replicate else 0, q_planar=True, Cb=Cb)
    err = float((got.double() - ref.double()).norm() / ref.double().norm())
    assert err <= 2e-5, 'planar: rel-L2 %.3e' % err


CASES_S2 = [
    # B, QH, QW, Ca (= cout), Cb (= cin): nn.Conv2d(Cb, Ca, 3, stride 2, padding 1) - ResNet layer2-4 conv1
    (2, 32, 32, 128, 64),
    (2, 16, 16, 256, 128),     # P is 8 x 8: two images side by side in a k-step
    (3, 8, 8, 512, 256),       # P is 4 x 4
    (3, 17, 9, 72, 40),        # odd input sizes, ragged channel blocks
    (1, 64, 64, 128, 64),
    (5, 15, 13, 48, 32),
]


@pytest.mark.parametrize('case', CASES_S2)
@pytest.mark.parametrize('nsplit', [None, 3])
def test_wgrad_ls_stride2_vs_torch(case, nsplit):
    """The stride-2 variant (Q de-interleaved into even / odd column planes by the loader): dW of nn.Conv2d(k3, s2, p1)."""
    B, QH, QW, Ca, Cb = case
    PH, PW = (QH + 2 - 3) // 2 + 1, (QW + 2 - 3) // 2 + 1
    p, q = _mk(B, Ca, PH, PW, 11), _mk(B, Cb, QH, QW, 12)
    w = torch.zeros(Ca, Cb, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(q.double(), w, stride=2, padding=1) * p.double()).sum().backward()
    ref = w.grad.float()
    taps = [(dy - 1, dx - 1) for dy in range(3) for dx in range(3)]
    got, ns = _wgrad_hip(p.permute(0, 2, 3, 1).contiguous().bfloat16().cuda(), q.permute(0, 2, 3, 1).contiguous().bfloat16().cuda(), taps, 0,
                         nsplit=nsplit, q_step=2)
    err = float((got.double() - ref.double()).norm() / ref.double().norm())
    assert torch.isfinite(got).all()
    assert err <= 2e-5, 'rel-L2 %.3e (nsplit %d)' % (err, ns)


def test_wgrad_ls_is_the_kernel_that_runs_and_matches_previous_kernels(tmp_path):
    """The plan hands aligned bf16 raster 3x3 launches to conv_wgrad_ls_kernel, and its results equal the float64 reference and the
    previous kernels' (conv_wgrad_fast8_kernel, conv_wgrad_fast_kernel<9, 8> / <9, 4>: ONE child process with SALT_WGRAD_LS=0 - the
    library reads the switch once - computes wgrad_abi.PREVIOUS_KERNEL_SHAPES) to fp32 summation-order noise."""
    import subprocess
    import sys
    code = 'import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); import wgrad_abi; torch.save(wgrad_abi.run_previous_shapes(wgrad_abi.FAST), sys.argv[1])' % (
        os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = str(tmp_path / 'previous.pt')
    subprocess.run([sys.executable, '-c', code, out], check=True, env=dict(os.environ, SALT_WGRAD_LS='0'), timeout=600)
    prev = torch.load(out)
    assert os.environ.get('SALT_WGRAD_LS', '1') != '0'
    new = wgrad_abi.run_previous_shapes(wgrad_abi.LS)
    assert len(prev) == len(new) == len(wgrad_abi.PREVIOUS_KERNEL_SHAPES)
    for i, shape in enumerate(wgrad_abi.PREVIOUS_KERNEL_SHAPES):
        p, q, taps = wgrad_abi.previous_shape_operands(shape, i)
        ref = wgrad_abi.wgrad_ref(p, q, taps, shape[5], shape[6]).permute(1, 2, 0).reshape(p.shape[1], q.shape[1], 3, 3)
        for name, got in (('previous', prev[i]), ('ls', new[i])):
            assert torch.isfinite(got).all(), (name, shape)
            err = wgrad_abi.rel_l2(got, ref)
            assert err <= 2e-5, '%s vs float64 %s: rel-L2 %.3e' % (name, shape, err)
        d = wgrad_abi.rel_l2(new[i], prev[i])
        assert d <= 2e-5, (shape, d)
