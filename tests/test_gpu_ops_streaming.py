"""Operator-level parity of the streaming kernels of csrc/elementwise.hip (and salt_zero) through the C-ABI against the plain fp64
references of op_reference.py: every view variant (contiguous / channel slice / misaligned slice / ragged, mixed between inputs and
outputs so that one view alone selects the scalar kernel), guard patterns around every output window, both accumulate settings,
odd sizes, all four pad sides, and the grid-stride loops of affine_act.

Tolerances (none measured on the kernels): selections / permutations exact; f32 5e-5 of max|ref| (TOL32 of test_gpu_blocks.py); bf16
one rounding of an fp32 result: 2**-8 |ref| + 5e-5 max|ref| per element; bilinear as in test_gpu_bilinear_rows.py."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import op_reference as R
from op_reference import Placed, VIEW_CASES, VARIANTS
from abi_ops import _abi, call, code, gen, rnd, close, shape_c, out_buf, null_view, DEV, F64, NAN, VIEWS_IDS

pytestmark = pytest.mark.gpu
DTYPES = ['f32', 'bf16']
SHAPES = [(2, 6, 8), (3, 7, 5), (1, 1, 1), (2, 2, 2)]


def ints(shape, g):
    return torch.randint(-3, 4, shape, generator=g).to(F64)            # small integers: exact in bf16, many ties


# ---------------------------------------------------------------- relu_bwd / add / layout
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_relu_bwd(dtype, views, shape):
    vin, vout = views
    for accumulate in (0, 1):
        for with_mask in (1, 0):
            g = gen('relu_bwd', dtype, vin, vout, shape, accumulate, with_mask)
            sc = shape_c(shape, vin, dtype)
            da, a = rnd(sc, g, dtype), rnd(sc, g, dtype).clamp_min(0)
            pda, pa = Placed(shape, vin, dtype, DEV, da), Placed(shape, vin, dtype, DEV, a)
            pdy, old = out_buf(shape, vout, dtype, accumulate, g)
            call('salt_relu_bwd', dtype=code(dtype), da=pda.view, a=pa.view if with_mask else null_view(),
                 dy=pdy.view, accumulate=accumulate)
            ref = R.relu_bwd(da, a if with_mask else None, old, accumulate)
            pdy.check('relu_bwd')
            if accumulate:
                close(pdy.get(), ref, dtype, 'relu_bwd accumulate')
            else:
                assert torch.equal(pdy.get(), ref), 'relu_bwd is a selection'


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_add(dtype, views, shape):
    vin, vout = views
    null = null_view()
    for accumulate in (0, 1):
        for with_b in (1, 0):
            g = gen('add', dtype, vin, vout, shape, accumulate, with_b)
            sc = shape_c(shape, vin, dtype)
            a, b = rnd(sc, g, dtype), rnd(sc, g, dtype)
            pa, pb = Placed(shape, vin, dtype, DEV, a), Placed(shape, vin, dtype, DEV, b)
            py, old = out_buf(shape, vout, dtype, accumulate, g)
            call('salt_add', dtype=code(dtype), a=pa.view, b=pb.view if with_b else null, y=py.view, accumulate=accumulate)
            ref = R.add(a, b if with_b else None, old, accumulate)
            py.check('add')
            if not with_b and not accumulate:
                assert torch.equal(py.get(), a), 'same-dtype copy through add'
            else:
                close(py.get(), ref, dtype, 'add b=%d accumulate=%d' % (with_b, accumulate))


@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
def test_add_rounds_f32_sum_once_to_bf16(views):
    """bf16 view: the stored value is the fp32 sum a + b rounded ONCE (not a sum of rounded partial results)."""
    vin, vout = views
    shape = (2, 6, 8)
    g = gen('add cast', vin, vout)
    sc = shape_c(shape, vin, 'bf16')
    a, b = rnd(sc, g, 'bf16'), rnd(sc, g, 'bf16', 2.0 ** -6)
    pa, pb = Placed(shape, vin, 'bf16', DEV, a), Placed(shape, vin, 'bf16', DEV, b)
    py, _ = out_buf(shape, vout, 'bf16', 0, g)
    call('salt_add', dtype=1, a=pa.view, b=pb.view, y=py.view, accumulate=0)
    py.check('add cast')
    assert torch.equal(py.get(), (a.float() + b.float()).to(torch.bfloat16).to(F64))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('variant', list('abcd'))
@pytest.mark.parametrize('dtype', DTYPES)
def test_layout(dtype, variant, shape):
    g = gen('layout', dtype, variant, shape)
    B, H, W = shape
    C = VARIANTS[variant][dtype][1]
    x = rnd((B, C, H, W), g, dtype)                                    # representable in the view's dtype: both directions exact
    nchw = x.float().to(DEV).contiguous()
    pv = Placed(shape, variant, dtype, DEV)
    call('salt_layout', dtype=code(dtype), nchw=nchw.data_ptr(), nhwc=pv.view, to_nhwc=1)
    pv.check('layout to nhwc')
    assert torch.equal(pv.get(), R.nchw_to_nhwc(x))
    back = torch.full((B, C, H, W), NAN, dtype=torch.float32, device=DEV)
    call('salt_layout', dtype=code(dtype), nchw=back.data_ptr(), nhwc=pv.view, to_nhwc=0)
    assert torch.equal(back.cpu().to(F64), R.nhwc_to_nchw(R.nchw_to_nhwc(x)))
    if dtype == 'bf16':                                                # fp32 values that bf16 cannot hold: one rounding on the way in
        y = torch.randn(B, C, H, W, generator=g)
        pv2 = Placed(shape, variant, dtype, DEV)
        call('salt_layout', dtype=1, nchw=y.to(DEV).data_ptr(), nhwc=pv2.view, to_nhwc=1)
        pv2.check('layout cast')
        assert torch.equal(pv2.get(), R.nchw_to_nhwc(y.to(torch.bfloat16).to(F64)))


# ---------------------------------------------------------------- pooling
POOL_SHAPES = [s for s in SHAPES if s[1] >= 2]


@pytest.mark.parametrize('shape', POOL_SHAPES + [(2, 7, 9)])
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_maxpool2(dtype, views, shape):
    vin, vout = views
    B, H, W = shape
    g = gen('maxpool2', dtype, vin, vout, shape)
    x = ints(shape_c(shape, vin, dtype), g)
    px = Placed(shape, vin, dtype, DEV, x)
    oshape = (B, H // 2, W // 2)
    py, _ = out_buf(oshape, vout, dtype, 0, g)
    call('salt_maxpool2', dtype=code(dtype), x=px.view, y=py.view)
    py.check('maxpool2')
    assert torch.equal(py.get(), R.maxpool2(x))
    for accumulate in (0, 1):
        dy = rnd(shape_c(oshape, vin, dtype), g, dtype)
        pdy = Placed(oshape, vin, dtype, DEV, dy)
        pdx, old = out_buf(shape, vout, dtype, accumulate, g)
        call('salt_maxpool2_bwd', dtype=code(dtype), x=px.view, dy=pdy.view, dx=pdx.view, accumulate=accumulate)
        pdx.check('maxpool2_bwd')
        ref = R.maxpool2_bwd(x, dy, old, accumulate)
        got = pdx.get()
        if accumulate:
            close(got, ref, dtype, 'maxpool2_bwd accumulate')
            assert torch.equal(got[:, H - H % 2:], old[:, H - H % 2:]) and torch.equal(got[:, :, W - W % 2:], old[:, :, W - W % 2:]), \
                'the uncovered last row / column is left unchanged'
        else:
            assert torch.equal(got, ref), 'maxpool2_bwd is a selection (first maximum; zero where no window covers)'


@pytest.mark.parametrize('shape', SHAPES + [(2, 7, 9)])
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_maxpool3s2(dtype, views, shape):
    vin, vout = views
    B, H, W = shape
    g = gen('maxpool3s2', dtype, vin, vout, shape)
    x = ints(shape_c(shape, vin, dtype), g)
    px = Placed(shape, vin, dtype, DEV, x)
    oshape = (B, (H + 1) // 2, (W + 1) // 2)
    py, _ = out_buf(oshape, vout, dtype, 0, g)
    call('salt_maxpool3s2', dtype=code(dtype), x=px.view, y=py.view)
    py.check('maxpool3s2')
    assert torch.equal(py.get(), R.maxpool3s2(x))
    for accumulate in (0, 1):
        dy = ints(shape_c(oshape, vin, dtype), g)                      # integers: the up-to-four gathered gradients add exactly
        pdy = Placed(oshape, vin, dtype, DEV, dy)
        pdx, old = out_buf(shape, vout, dtype, accumulate, g)
        if accumulate:
            old = ints(old.shape, g)
            pdx.win.copy_(old.to(pdx.buf.dtype))
        call('salt_maxpool3s2_bwd', dtype=code(dtype), x=px.view, dy=pdy.view, dx=pdx.view, accumulate=accumulate)
        pdx.check('maxpool3s2_bwd')
        assert torch.equal(pdx.get(), R.maxpool3s2_bwd(x, dy, old, accumulate)), 'maxpool3s2_bwd accumulate=%d' % accumulate


@pytest.mark.parametrize('shape', POOL_SHAPES)
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_avgpool2(dtype, views, shape):
    vin, vout = views
    B, H, W = shape
    oshape = (B, H // 2, W // 2)
    g = gen('avgpool2', dtype, vin, vout, shape)
    x = rnd(shape_c(shape, vin, dtype), g, dtype)
    px = Placed(shape, vin, dtype, DEV, x)
    py, _ = out_buf(oshape, vout, dtype, 0, g)
    call('salt_avgpool2', dtype=code(dtype), x=px.view, y=py.view, backward=0, accumulate=0)
    py.check('avgpool2')
    close(py.get(), R.avgpool2(x), dtype, 'avgpool2')
    for accumulate in (0, 1):
        dy = rnd(shape_c(oshape, vin, dtype), g, dtype)
        pdy = Placed(oshape, vin, dtype, DEV, dy)
        pdx, old = out_buf(shape, vout, dtype, accumulate, g)
        call('salt_avgpool2', dtype=code(dtype), x=pdx.view, y=pdy.view, backward=1, accumulate=accumulate)
        pdx.check('avgpool2 backward')
        got = pdx.get()
        close(got, R.avgpool2_bwd(dy, H, W, old, accumulate), dtype, 'avgpool2 backward accumulate=%d' % accumulate)
        edge_ref = old if accumulate else torch.zeros_like(old)
        assert torch.equal(got[:, H - H % 2:], edge_ref[:, H - H % 2:]) and torch.equal(got[:, :, W - W % 2:], edge_ref[:, :, W - W % 2:]), \
            'the uncovered last row / column is zero (unchanged under accumulate)'


# ---------------------------------------------------------------- replicate-pad adjoint
PADS = [(2, 0, 0, 2), (0, 2, 2, 0), (1, 2, 3, 1), (0, 0, 0, 0)]


@pytest.mark.parametrize('pads', PADS)
@pytest.mark.parametrize('shape', [(2, 5, 4), (1, 1, 1)])
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_pad_fold(dtype, views, shape, pads):
    vin, vout = views
    top, bottom, left, right = pads
    B, H, W = shape
    pshape = (B, H + top + bottom, W + left + right)
    for accumulate in (0, 1):
        g = gen('pad_fold', dtype, vin, vout, shape, pads, accumulate)
        xp = rnd(shape_c(pshape, vin, dtype), g, dtype)
        pxp = Placed(pshape, vin, dtype, DEV, xp)
        px, old = out_buf(shape, vout, dtype, accumulate, g)
        call('salt_pad_fold', dtype=code(dtype), xp=pxp.view, top=top, bottom=bottom, left=left, right=right, x=px.view, accumulate=accumulate)
        px.check('pad_fold')
        close(px.get(), R.pad_fold(xp, top, bottom, left, right, old, accumulate), dtype, 'pad_fold %s accumulate=%d' % (pads, accumulate))


@pytest.mark.parametrize('pads', PADS)
@pytest.mark.parametrize('shape', [(2, 5, 4), (2, 2, 7), (1, 1, 1)])
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_pad_fold_strip(dtype, views, shape, pads):
    """The strip is a [B * ring, strip_cs] buffer with strip_cs > C; `views` = (strip variant, x variant)."""
    vin, vout = views
    top, bottom, left, right = pads
    B, H, W = shape
    abi = _abi()
    npx = int(abi.lib.salt_fold_strip_pixels(H, W, top, bottom, left, right))
    assert npx == len(R.fold_ring_pixels(H, W, top, bottom, left, right))
    g = gen('pad_fold_strip', dtype, vin, vout, shape, pads)
    c0, C, cs = VARIANTS[vin][dtype]
    if cs == C:
        cs = C + (8 if vin == 'a' else 3)                              # strip_cs > C: 'a' keeps 16-byte pieces, 'd' stays ragged
    xp = rnd((B, H + top + bottom, W + left + right, C), g, dtype)
    strip = R.ring_from_padded(xp, top, bottom, left, right)           # [B, ring, C]
    x0 = rnd(shape + (VARIANTS[vout][dtype][1],), g, dtype)
    px = Placed(shape, vout, dtype, DEV, x0)
    ps = Placed((1, B, max(npx, 1)), (c0, C, cs), dtype, DEV, strip.reshape(1, B, npx, C) if npx else None)
    call('salt_pad_fold_strip', dtype=code(dtype), strip=ps.view.p, strip_cs=cs, top=top, bottom=bottom, left=left, right=right, x=px.view)
    px.check('pad_fold_strip')
    close(px.get(), R.pad_fold_strip(strip, x0, top, bottom, left, right), dtype, 'pad_fold_strip %s' % (pads,))


# ---------------------------------------------------------------- affine + activation
def _affine_case(dtype, vin, vout, shape_bhwc, with_scale, with_res, relu, seed):
    B, H, W, C = shape_bhwc
    shape = (B, H, W)
    g = gen('affine', dtype, vin, vout, shape_bhwc, with_scale, with_res, relu, seed)
    y = rnd(shape_bhwc, g, dtype)
    res = rnd(shape_bhwc, g, dtype) if with_res else None
    scale = (torch.rand(C, generator=g) + 0.5).to(F64) if with_scale else None
    shift = torch.randn(C, generator=g).to(F64) if with_scale else None
    py = Placed(shape, vin, dtype, DEV, y)
    pr = Placed(shape, vin, dtype, DEV, res) if with_res else None
    pa = Placed(shape, vout, dtype, DEV, torch.full(shape_bhwc, NAN, dtype=F64))
    sc_d = scale.float().to(DEV) if with_scale else None
    sh_d = shift.float().to(DEV) if with_scale else None
    null = null_view()
    call('salt_affine_act', dtype=code(dtype), y=py.view, scale=sc_d.data_ptr() if with_scale else None, shift=sh_d.data_ptr() if with_scale else None,
         res=pr.view if with_res else null, relu=relu, a=pa.view, fin=None, fin_acc=None)
    pa.check('affine_act')
    close(pa.get(), R.affine_act(y, scale, shift, res, relu), dtype, 'affine_act scale=%d res=%d relu=%d' % (with_scale, with_res, relu))


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('with_res', [0, 1])
@pytest.mark.parametrize('with_scale', [0, 1])
@pytest.mark.parametrize('views', VIEW_CASES, ids=VIEWS_IDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_affine_act(dtype, views, with_scale, with_res, relu):
    vin, vout = views
    _affine_case(dtype, vin, vout, (2, 6, 8, VARIANTS[vin][dtype][1]), with_scale, with_res, relu, 0)


@pytest.mark.parametrize('shape_bhwc', [(2, 192, 192, 16),      # 4 pieces per pixel, 294912 units > 2 x 512 x 256: several unrolled trips, live tail
                                        (1, 160, 160, 24)])     # 6 pieces per pixel do not divide the grid stride: generic path, several trips
@pytest.mark.parametrize('with_res', [0, 1])
def test_affine_act_grid_stride_loops(shape_bhwc, with_res):
    C = shape_bhwc[3]
    _affine_case('f32', (0, C, C), (0, C, C), shape_bhwc, 1, with_res, 1, 1)


def test_affine_act_grid_stride_loop_strided_output():
    _affine_case('f32', (0, 16, 16), (8, 16, 40), (2, 192, 192, 16), 1, 1, 0, 2)


# ---------------------------------------------------------------- bilinear through strided views
@pytest.mark.parametrize('R_', [2, 4])
@pytest.mark.parametrize('variant', ['b', 'c'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bilinear_strided_views(dtype, variant, R_):
    """Tolerances of test_gpu_bilinear_rows.py (1e-5 f32 / 1e-2 bf16 of max(1, max|ref|), x2 for the two-pass bf16 adjoint, x3 under
    accumulate); the point here is the pixel stride, the misaligned slice and the gap channels."""
    shape, oshape = (2, 3, 5), (2, 3 * R_, 5 * R_)
    g = gen('bilinear', dtype, variant, R_)
    C = VARIANTS[variant][dtype][1]
    x, gy = rnd(shape + (C,), g, dtype), rnd(oshape + (C,), g, dtype)
    xr = R.nhwc_to_nchw(x).requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=R_, mode='bilinear', align_corners=False)
    yr.backward(R.nhwc_to_nchw(gy))
    yref, dxref = R.nchw_to_nhwc(yr.detach()), R.nchw_to_nhwc(xr.grad)
    tol = 1e-2 if dtype == 'bf16' else 1e-5
    px = Placed(shape, variant, dtype, DEV, x)
    py, _ = out_buf(oshape, variant, dtype, 0, g)
    call('salt_bilinear', dtype=code(dtype), x=px.view, y=py.view, R=R_, backward=0, accumulate=0, tmp=None, align_corners=0)
    py.check('bilinear')
    assert float((py.get() - yref).abs().max()) <= tol * max(1.0, float(yref.abs().max()))
    pg = Placed(oshape, variant, dtype, DEV, gy)
    tmp = torch.empty(2 * 3 * R_ * 5 * 16, dtype=R.torch_dtype(dtype), device=DEV)
    for accumulate in (0, 1):
        pdx, old = out_buf(shape, variant, dtype, accumulate, g)
        call('salt_bilinear', dtype=code(dtype), x=pdx.view, y=pg.view, R=R_, backward=1, accumulate=accumulate, tmp=tmp.data_ptr(), align_corners=0)
        pdx.check('bilinear adjoint')
        ref = dxref + old if accumulate else dxref
        bound = tol * max(1.0, float(dxref.abs().max())) * (3 if accumulate else (2 if R_ >= 4 and dtype == 'bf16' else 1))
        assert float((pdx.get() - ref).abs().max()) <= bound, (accumulate, float((pdx.get() - ref).abs().max()), bound)


# ---------------------------------------------------------------- salt_zero
@pytest.mark.parametrize('nbytes', [0, 4, 60, 4100])
def test_zero_stays_inside_its_range(nbytes):
    words = nbytes // 4
    buf = torch.full((words + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    call('salt_zero', p=buf.data_ptr() + 16, bytes=nbytes)
    got = buf.cpu()
    assert bool((got[:4] == 0x5A5A5A5A).all()) and bool((got[4 + words:] == 0x5A5A5A5A).all()), 'guard words'
    assert bool((got[4:4 + words] == 0).all())


def test_zero_rejects_a_size_that_is_no_multiple_of_four():
    abi = _abi()
    buf = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    fn, S = abi.OP_FUNCS['salt_zero']
    rc = fn(ctypes.byref(abi.fill(S(), p=buf.data_ptr(), bytes=6)), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == abi.CONSTS['SALT_E_BADARG']                           # rejected on the host, before any launch
    torch.cuda.synchronize()
    assert bool((buf.cpu() == 0x5A5A5A5A).all())
