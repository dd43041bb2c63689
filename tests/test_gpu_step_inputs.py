"""The step inputs of a compiled instance (batch `x`, depth `d`, `target`, the `loss` scalar) as recorded slots: the emitters that read
one say so (engine.StepInput -> Program.slots) and CompiledNet.bind re-points exactly those fields.  The records are compared against
the by-value search bind used to do (net_checks._ptr_fields), and the one stem no other test binds - VanillaUNet's direct first
convolution, whose BACKWARD program reads the batch too - is trained in place against the copied route."""
import pytest
import torch

import net_checks as NC

pytestmark = pytest.mark.gpu
DEV = NC.DEV

# the smallest shapes the suite trains each network at: the s2d stem, the direct stem (x read by forward AND backward), stack_conv + d,
# the depth gate of the U-Net
CASES = [('UNetResNet', 'lovasz', (2, 3, 64, 64), {}), ('VanillaUNet', 'bce_dice', (2, 1, 64, 64), {}),
         ('StackingFCNWithDepth', 'lovasz', (4, 5, 32, 32), {'input_model_nr': 5}), ('UNetResNetWithDepth', 'lovasz', (2, 3, 64, 64), {})]


@pytest.mark.parametrize('arch,loss,shape,extra', CASES, ids=[c[0] for c in CASES])
def test_recorded_slots_equal_the_search_by_value(arch, loss, shape, extra):
    """A training instance with its loss program built, everything on the static buffers: for every key the recorded (struct, field)
    set equals the set of pointer fields that hold the static buffer's address."""
    torch.manual_seed(0)
    m = NC.family_model(arch, 'f32', 1e-3, 1, None, loss=loss, **extra)
    m._to_device()
    m.model.train()
    net = m.model.engine().net(shape, True)
    net.loss_program(loss, 1.0)
    assert (net.d is not None) == arch.endswith('WithDepth')
    for which in ('x', 'target', 'loss') + (('d',) if net.d is not None else ()):
        recorded, searched, in_bwd = NC.recorded_and_searched_slots(net, which)
        print(arch, which, len(recorded), 'recorded', len(searched), 'searched')
        assert recorded and recorded == searched, (which, recorded ^ searched)
        assert len(recorded) == len(net.slots(which))
        if arch == 'VanillaUNet' and which == 'x':
            assert any(addr in in_bwd for addr, _ in recorded)


def test_direct_stem_reads_a_resident_batch_in_place(deterministic_sums):
    """VanillaUNet's conv_first and its conv_first_wgrad (backward) both read the batch: two steps on resident contiguous tensors (bound
    in place) against the same steps on batch-sliced float64 views (copied into the static buffer) - the same bits."""
    g = torch.Generator().manual_seed(9)
    X = torch.randn(4, 1, 64, 64, generator=g)
    M = (torch.rand(4, 1, 64, 64, generator=g) > 0.6).float()
    Tt = torch.cat([1 - M, M], 1)
    res = []
    for mode in ('bound', 'views'):
        torch.manual_seed(3)
        m = NC.segmentation_model('VanillaUNet', 'bce_dice', 'f32', 1e-3)
        m._to_device()
        m.model.train()
        ls = []
        for i in range(2):
            sl = slice(2 * i, 2 * i + 2)
            Xd = X.double().to(DEV)[sl] if mode == 'views' else X[sl].clone().to(DEV)
            Td = Tt.to(DEV)[sl] if mode == 'views' else Tt[sl].clone().to(DEV)
            ls.append(float(m._fit_loop([Xd, Td])['sum']))
        torch.cuda.synchronize()
        eng = m.model.engine()
        res.append((ls, eng.grads.clone(), eng.flat.clone()))
    print('losses', res[0][0], res[1][0])
    assert res[0][0] == res[1][0] and len(set(res[0][0])) == 2
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
