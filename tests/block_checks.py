"""The block rule of the GPU tests that hold a module, emitted through the graph, to a fixture the reference produced: forward, input
gradient, every parameter gradient and the running statistics with the bounds of tests/test_gpu_blocks.py::test_block_vs_reference_golden
(5e-5 f32, 2x / 3x for input / parameter gradients; bf16 4e-2 forward and the 1.5 e_emu + 2e-2 rule against the bf16-storage emulation
of the test-side oracle backward).  Fixtures in the layout of tests/golden/make_golden_lkm.py::block_fixture ('fractions': the guarded
ReLU pass fractions).

Importable without a GPU and without the built library."""
import torch

from abi_ops import DEV

TOL32, TOLBF = 5e-5, 4e-2                   # tests/test_gpu_blocks.py: the F2 / F4 block bounds


def block_state(m):
    import closed_form as CF
    return {k: CF.tensor_for(k, v.shape).to(v.dtype) for k, v in m.state_dict().items()}


def emulated(fn, sd, x, gy):
    """the test-side oracle block with bf16 storage emulated: the yardstick of the bf16 backward bound (tests/test_gpu_blocks.py)"""
    from oracle import blocks as OB
    s2 = {k: v.clone() for k, v in sd.items()}
    leaves = [k for k, v in s2.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))]
    for k in leaves:
        s2[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    with OB.bf16_storage():
        fn(s2, OB._st(xr)).backward(gy)
    out = {'gx': xr.grad}
    for k in leaves:
        out['g:' + k] = s2[k].grad if s2[k].grad is not None else torch.zeros_like(s2[k])
    return out


def block_vs_golden(fxname, make, emit, oracle, mode, dtype, zero_grads=()):
    """forward, input gradient, parameter gradients and running statistics with the bounds of
    tests/test_gpu_blocks.py::test_block_vs_reference_golden (5e-5 f32, 2x / 3x for input / parameter gradients; bf16 4e-2 forward and
    the 1.5 e_emu + 2e-2 rule against the bf16-storage emulation backward) -> the BlockRun"""
    import numpy as np
    import closed_form as CF
    from gpu_harness import BlockRun
    from helpers import golden, assert_close, rel_err
    fx = golden('%s_%s' % (fxname, mode))
    assert all(0.2 <= f <= 0.8 for f in fx['fractions'].tolist()) and float(fx['ref_f32_vs_f64']) <= TOL32 / 4
    m = make()
    sd = block_state(m)
    m.load_state_dict(sd)
    x = CF.input_for(str(fx['input_tag']), tuple(int(v) for v in fx['x_shape']))
    gy = CF.input_for('gy:%s' % (tuple(fx['y'].shape),), fx['y'].shape)
    train = mode == 'train'
    m.train(train)
    run = BlockRun(m, [x], lambda g, a: emit(m, g, a), train=train, dtype=dtype)
    tol = TOL32 if dtype == 'f32' else TOLBF
    e = assert_close(run.forward(), fx['y'], tol, 'y')
    print('  %s %s %s y: %.2e of %.1e' % (fxname, mode, dtype, e, tol))
    if not train:
        return run
    gx, grads = run.backward(gy.to(DEV))
    emu = None if dtype == 'f32' else emulated(lambda s, a: oracle(s, a, True), sd, x, gy)

    def check(got, ref, key, f32_tol):
        if emu is None:
            e = assert_close(got, ref, f32_tol, key)
            print('  %s %s %s: %.2e of %.1e' % (fxname, dtype, key, e, f32_tol))
        else:
            e_hip, e_emu = rel_err(got, ref), rel_err(emu[key], ref)
            print('  %s %s %s: HIP %.2e, emulation %.2e' % (fxname, dtype, key, e_hip, e_emu))
            assert e_hip <= 1.5 * e_emu + 2e-2, '%s: HIP bf16 %.3e from the golden, bf16-storage emulation %.3e' % (key, e_hip, e_emu)
    check(gx[0], fx['gx'], 'gx', tol * 2)
    assert set(grads) == {k for k, _ in m.named_parameters()} == {k[2:] for k in fx if k.startswith('g:')}
    gscale = max(float(np.abs(fx['g:' + k]).max()) for k in grads)
    for k, g in grads.items():
        if float(g.abs().max()) == 0.0:      # a convolution's bias in front of a train-mode BatchNorm: analytically zero, rounding noise in the fixture
            assert k.endswith('conv.bias') and np.abs(fx['g:' + k]).max() < 1e-4 * gscale, k
        elif emu is None and k in zero_grads:
            # ``zero_grads``: parameters whose gradient is analytically zero although the kernels do not write exact zeros (the caller says
            # why): the fixture and the kernels both hold rounding noise, which has no relative error - both must be noise (bf16: the
            # emulation rule below covers it, its noise is the yardstick)
            assert np.abs(fx['g:' + k]).max() < 1e-4 * gscale and float(g.abs().max()) < 1e-4 * gscale, k
        else:
            check(g, fx['g:' + k], 'g:' + k, tol * 3)
    sd2 = m.state_dict()
    for k in sd2:
        if k.endswith(('running_mean', 'running_var')):
            assert_close(sd2[k].cpu(), fx['s:' + k], tol, k)
    return run
