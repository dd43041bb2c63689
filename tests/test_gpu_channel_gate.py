"""Operator-level GPU tests of salt_channel_gate (csrc/depth.hip) through the C-ABI on guarded operands, for the paths the block tests
of tests/test_gpu_depth.py do not reach: the element-wise kernels (C = 5; C = 24 in rows of 27), lanes-per-pixel that do not divide the
workgroup so that its last threads idle (bf16 C = 24: 85 pixel rows of 3 lanes; f32 C = 40: 25 rows of 10), several ragged pixel parts,
both dL/ds protocols, accumulate, the inplace backward, a gate wider than the level (sC > C, c0 > 0) - and what happens when x allows
16-byte pieces and dx does not, where salt_channel_gate_parts (which sees x alone) and the launch (which looks at every view) plan
differently.

The operation: y = x s[b][c0 + c];  dx = dy s (+ old);  ds[b][c0 + c] = sum over the image of dy x - with inplace = 1 the kernel is given
the STORED y in place of x and divides the sum by s, and the reference does the same on the same stored values.  Bounds as in
tests/test_gpu_scse.py (abi_ops.within): 4 e32 + 1e-6 max|ref| with e32 the error of a float32 torch evaluation of the same case, plus
2**-8 |ref| per element for activations stored in bf16 (one rounding each)."""
import ctypes

import pytest
import torch

from abi_ops import Act, Vec, Frozen, raw, call, _abi, code, rnd, gen, DEV, F64, NAN
from abi_ops import within as bound_within

pytestmark = pytest.mark.gpu
RATIOS = {}

# name: (dtype, (B, H, W, C), layout (c0, cs) or None for contiguous, pieces per pixel row N the launch must pick, parts it must plan)
CASES = {
    'scalar-c5-f32': ('f32', (2, 17, 19, 5), None, 1, 2),              # 51 pixel rows of 5 lanes, thread 255 idles; 162 + 161 pixels
    'scalar-c5-bf16': ('bf16', (2, 17, 19, 5), None, 1, 2),
    'scalar-c24-rows27-f32': ('f32', (3, 9, 11, 24), (2, 27), 1, 3),   # rows of 27 elements: no 16-byte piece; 10 pixel rows, 16 threads idle
    'scalar-c24-rows27-bf16': ('bf16', (3, 9, 11, 24), (2, 27), 1, 3),
    'idle-c24-bf16': ('bf16', (2, 23, 31, 24), None, 8, 3),            # 3 lanes per pixel: 85 rows, thread 255 idles; 238 + 238 + 237 pixels
    'idle-c40-f32': ('f32', (2, 17, 19, 40), None, 4, 4),              # 10 lanes per pixel: 25 rows, 6 threads idle; 81 + 81 + 81 + 80
    'sliced-c64-bf16': ('bf16', (2, 17, 19, 64), (32, 160), 8, 3),     # 16-byte pieces inside a wider buffer
}


def within(got, ref64, ev32, what, case, key, allowance=None):
    bound_within(got, ref64, ev32, what, RATIOS, case, key, allowance)


def plan(B, hw, C, N):
    """gate_plan of csrc/depth.hip -> nparts"""
    R = 256 // (C // N)
    np_ = max(1, min(-(-1024 // B), -(-hw // (R * 4)), 64))
    per = -(-hw // np_)
    return -(-hw // per)


def operands(name):
    dtype, (B, H, W, C), layout, N, nparts = CASES[name]
    g = gen('channel_gate', name)
    sC, c0 = C + 7, 3
    c = dict(x=rnd((B, H, W, C), g, dtype), dy=rnd((B, H, W, C), g, dtype), old=rnd((B, H, W, C), g, dtype))
    c['s'] = torch.sigmoid(torch.randn(B, sC, generator=g, dtype=F64)).float().double()
    c['sw'] = c['s'][:, c0:c0 + C]
    assert plan(B, H * W, C, N) == nparts
    return c, sC, c0


def run(name, acc_path, accumulate, inplace):
    abi = _abi()
    dtype, (B, H, W, C), layout, N, nparts = CASES[name]
    c, sC, c0 = operands(name)
    what = 'channel_gate %s acc_path=%d accumulate=%d inplace=%d' % (name, acc_path, accumulate, inplace)
    bf = dtype == 'bf16'
    s = c['s'].float().to(DEV)
    x = Act(c['x'], dtype, False, layout)
    y = Act(torch.full((B, H, W, C), NAN, dtype=F64), dtype, False, layout)
    probe = abi.fill(abi.STRUCTS['salt_channel_gate_args'](), dtype=code(dtype), x=x.view)
    assert abi.lib.salt_channel_gate_parts(ctypes.byref(probe)) == nparts
    frozen = Frozen(x=x.buf, s=s)
    call('salt_channel_gate', dtype=code(dtype), x=x.view, y=y.view, s=s.data_ptr(), sC=sC, c0=c0)
    frozen.check(what + ' forward')
    y.check(what + ' y')
    got_y = y.get()
    sw = c['sw'][:, None, None, :]
    ref_y = c['x'] * sw
    within(got_y, ref_y, c['x'].float() * sw.float(), what, name, 'y', 2.0 ** -8 * ref_y.abs() if bf else None)
    # backward: with inplace the kernel is given the stored y instead of x
    dy = Act(c['dy'], dtype, False, layout)
    xin = y if inplace else x
    dx = dy if inplace else Act(c['old'] if accumulate else torch.full((B, H, W, C), NAN, dtype=F64), dtype, False, layout)
    ds = Vec(B * sC)
    parts = Vec(B * nparts * C)
    ds_acc = Vec(B * sC, fill=0.0, dtype=F64)
    frozen = Frozen(x=xin.buf, s=s, **({} if inplace else {'dy': dy.buf}))
    call('salt_channel_gate', dtype=code(dtype), backward=1, x=xin.view, y=dy.view, dx=dx.view, s=s.data_ptr(), sC=sC, c0=c0, accumulate=accumulate,
         inplace=inplace, ds=None if acc_path else ds.ptr(), partials=None if acc_path else parts.ptr(), nparts=nparts, ds_acc=ds_acc.ptr() if acc_path else None)
    frozen.check(what + ' backward')
    dx.check(what + ' dx')
    ref_dx = c['dy'] * sw + (c['old'] if accumulate else 0.0)
    ev_dx = c['dy'].float() * sw.float() + (c['old'].float() if accumulate else 0.0)
    within(dx.get(), ref_dx, ev_dx, what, name, 'dx', 2.0 ** -8 * ref_dx.abs() if bf else None)
    seen = got_y if inplace else c['x']
    ref_ds = (c['dy'] * seen).sum(dim=(1, 2)) / (c['sw'] if inplace else 1.0)
    ev_ds = (c['dy'].float() * seen.float()).sum(dim=(1, 2)) / (c['sw'].float() if inplace else 1.0)
    full_ds, full_acc = ds.get((B, sC)), ds_acc.get((B, sC))
    if acc_path:
        got_ds = full_acc[:, c0:c0 + C]
        assert bool((full_acc[:, :c0] == 0).all()) and bool((full_acc[:, c0 + C:] == 0).all()), what + ': ds_acc outside [c0, c0 + C)'
        assert bool(torch.isnan(full_ds).all()) and bool(torch.isnan(parts.get((-1,))).all()), what + ': the fixed-order workspaces were touched'
    else:
        got_ds = full_ds[:, c0:c0 + C]
        assert bool(torch.isnan(full_ds[:, :c0]).all()) and bool(torch.isnan(full_ds[:, c0 + C:]).all()), what + ': ds outside [c0, c0 + C)'
        assert bool((full_acc == 0).all()), what + ': ds_acc was touched on the fixed-order path'
    within(got_ds, ref_ds, ev_ds, what, name, 'ds')
    return dict(y=got_y, dx=dx.get(), ds=got_ds)


@pytest.mark.parametrize('name', list(CASES))
def test_channel_gate_vs_fp64_reference(name):
    for acc_path, accumulate, inplace in ((0, 0, 0), (1, 1, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)):
        run(name, acc_path, accumulate, inplace)
    print('RATIOS', name, {k: round(v, 3) for k, v in sorted(RATIOS[name].items())})


@pytest.mark.parametrize('name', ['scalar-c5-f32', 'idle-c24-bf16'])
def test_fixed_order_path_is_bit_identical_between_runs(name):
    a, b = run(name, 0, 0, 0), run(name, 0, 0, 0)
    for k in a:
        assert torch.equal(a[k], b[k]), (name, k)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_x_in_16_byte_pieces_and_dx_not(dtype):
    """salt_channel_gate_parts plans from x alone: 16-byte pieces.  The launch takes pieces only if EVERY view allows them; with a dx whose
    rows are no multiple of 16 bytes it runs element-wise, with more pixel rows per workgroup and so another number of parts.  Pinned:
    the fixed-order path REFUSES the planner's nparts before any launch (the error names the number it wants, with which it then runs),
    and the atomics path, which has no workspace to size, runs - both against the reference."""
    abi = _abi()
    B, H, W, C = 2, 23, 31, 8
    ve = 8 if dtype == 'bf16' else 4
    g = gen('gate mismatch', dtype)
    x, dyv, old = rnd((B, H, W, C), g, dtype), rnd((B, H, W, C), g, dtype), rnd((B, H, W, C), g, dtype)
    s64 = torch.sigmoid(torch.randn(B, C, generator=g, dtype=F64)).float().double()
    s = s64.float().to(DEV)
    X, DY = Act(x, dtype, False), Act(dyv, dtype, False)
    planned = abi.lib.salt_channel_gate_parts(ctypes.byref(abi.fill(abi.STRUCTS['salt_channel_gate_args'](), dtype=code(dtype), x=X.view)))
    wanted = plan(B, H * W, C, 1)
    assert planned == plan(B, H * W, C, ve) and planned != wanted
    ref_dx, ev_dx = dyv * s64[:, None, None, :] + old, dyv.float() * s64.float()[:, None, None, :] + old.float()
    ref_ds, ev_ds = (dyv * x).sum(dim=(1, 2)), (dyv.float() * x.float()).sum(dim=(1, 2))
    for acc_path, nparts in ((0, planned), (0, wanted), (1, 0)):
        DX = Act(old, dtype, False, (1, C + 3))
        ds, parts, ds_acc = Vec(B * C), Vec(B * max(planned, wanted) * C), Vec(B * C, fill=0.0, dtype=F64)
        before = Frozen(dx=DX.buf, x=X.buf, dy=DY.buf)
        rc = raw('salt_channel_gate', dtype=code(dtype), backward=1, x=X.view, y=DY.view, dx=DX.view, s=s.data_ptr(), sC=C, c0=0, accumulate=1,
                 ds=None if acc_path else ds.ptr(), partials=None if acc_path else parts.ptr(), nparts=nparts, ds_acc=ds_acc.ptr() if acc_path else None)
        what = 'gate mismatch %s acc_path=%d nparts=%d' % (dtype, acc_path, nparts)
        if not acc_path and nparts == planned:
            msg = abi.lib.salt_last_error().decode()
            assert rc == abi.CONSTS['SALT_E_BADARG'] and 'expected %d' % wanted in msg, (rc, msg)
            before.check(what)
            assert bool(torch.isnan(ds.get((B, C))).all()) and bool(torch.isnan(parts.get((-1,))).all())
            continue
        assert rc == 0, (what, rc, abi.lib.salt_last_error().decode())
        DX.check(what + ' dx')
        within(DX.get(), ref_dx, ev_dx, what, 'mismatch-' + dtype, 'dx', 2.0 ** -8 * ref_dx.abs() if dtype == 'bf16' else None)
        within(ds_acc.get((B, C)) if acc_path else ds.get((B, C)), ref_ds, ev_ds, what, 'mismatch-' + dtype, 'ds')
