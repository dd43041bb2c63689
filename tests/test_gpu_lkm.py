"""GPU tests of LargeKernelMatters: GlobalConvolutionalNetwork and BoundaryRefinement through the graph against the F21 block fixtures
(train and eval, f32 and bf16: outputs, input gradient, every parameter gradient, running statistics; the GCN block on the paired route
AND on the composed route, both held to the fixture), and LargeKernelMatters(34) against the F21 network fixture the reference produced
(eval logits and masks, hipGraph replay, bf16 storage, one training step, the step graph, the trainer) - on the route the shape rule
of Graph.gcn_pair ships (today the composed one at every shape) AND with the pair forced at all four levels (``net.paired = True``), so
that the kernel is driven through the whole graph; depth 50 in eval against tests/lkm_oracle.py; which composed data gradients take the
fused fold and which the strip.

The bounds are the ones tests/test_gpu_psp.py passes for F20 (tests/test_gpu_blocks.py's block rule; tests/net_checks.py's procedures).
The yardstick is always the fixture (or the oracle), never the composed GPU path."""
import pytest
import torch

from abi_ops import DEV

import block_checks as BC

pytestmark = pytest.mark.gpu

GCN_BLOCKS = [('F21_gcn', True, 'train'), ('F21_gcn', True, 'eval'), ('F21_gcn_norelu', False, 'train')]


@pytest.mark.parametrize('paired', [True, False], ids=['paired', 'composed'])
@pytest.mark.parametrize('fxname,use_relu,mode', GCN_BLOCKS, ids=['%s_%s' % (b[0], b[2]) for b in GCN_BLOCKS])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_gcn_block_vs_golden(dtype, fxname, use_relu, mode, paired):
    """F21_gcn / F21_gcn_norelu: GlobalConvolutionalNetwork(64, 21, 9) on [2,64,6,10] (H < K - 1 < W) - one paired launch for the two first
    layers, one paired data gradient that writes dL/dx once; the composed route (two convolutions, two fold-ring data gradients) is held
    to the same fixture with the same bounds"""
    import lkm_oracle as LO
    from salt_amd import architectures as A
    # use_relu=False: the BatchNorm shift of a first layer reaches the next train-mode BatchNorm through a convolution alone (a constant per
    # channel stays a constant per channel under the replicate pad): its gradient is analytically zero
    zero = () if use_relu else ('conv1.0.batch_norm.bias', 'conv2.0.batch_norm.bias')
    run = BC.block_vs_golden(fxname, lambda: A.GlobalConvolutionalNetwork(64, 21, 9, use_relu=use_relu), lambda m, g, a: m.emit(g, a, paired=paired),
                             lambda s, a, tr: LO.gcn(s, '', a, tr, use_relu), mode, dtype, zero_grads=zero)
    ops = [o[0] for o in run.g.fwd.ops]
    assert ops.count('gcn_pair') == int(paired) and ops.count('conv') == (2 if paired else 4) and ops.count('add') == 1
    if paired and mode == 'eval':
        assert 'bn_finalize' not in ops and 'affine_act' not in ops                           # ONE launch with both folded epilogues
    if mode == 'train':
        bops = [o[0] for o in run.g.bwd.ops]
        assert bops.count('gcn_pair_dgrad') == int(paired) and bops.count('bn_bwd') == 4
        if paired:
            assert ops.count('bn_finalize') >= 2 and ops.count('affine_act') == 4            # the pair: per-tile partials + bn_finalize per branch in every SALT_BN_FIN mode
            dg = [s for (o, _, s) in run.g.bwd.ops if o == 'gcn_pair_dgrad'][0]
            assert dg.accumulate == 0 and dg.K == 9 and 'pad_fold_strip' not in bops[bops.index('gcn_pair_dgrad'):]


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_boundary_refinement_vs_golden(mode, dtype):
    """F21_br: BoundaryRefinement(21, 21, 3) on [2,21,5,7] - the residual BatchNorm without ReLU on salt_conv's ragged 21-channel path"""
    import lkm_oracle as LO
    from salt_amd import architectures as A
    BC.block_vs_golden('F21_br', lambda: A.BoundaryRefinement(21, 21, 3), lambda m, g, a: m.emit(g, a),
                        lambda s, a, tr: LO.boundary_refinement(s, '', a, tr), mode, dtype)


# ------------------------------------------------------------------------------------------------ whole network (F21, closed-form weights)
NET_FX = 'F21_lkm34'


def _fixture():
    from helpers import golden
    fx = golden(NET_FX)
    fx.update(golden(NET_FX + '_gcn5_grads'))
    return fx


def _net(fx, dtype='f32', paired=None):
    import net_checks as NC
    from helpers import T
    from salt_amd import architectures as A, models
    net = NC.fill_closed_form(A.LargeKernelMatters(num_classes=2, **models.ARCHITECTURES['LargeKernelMatters']['model_config']))
    net.final.bias.data.copy_(T(fx['final_bias']))           # the class-1 bias the generator may have moved so that both classes occur
    net.paired = paired          # None: the shipped rule decides; True: the pair at every level
    return net.set_compute_dtype(dtype).to(DEV)


ROUTES = pytest.mark.parametrize('paired', [None, True], ids=['shipped', 'pair_forced'])


@ROUTES
def test_eval_logits_and_masks_match_reference(paired):
    import net_checks as NC
    from helpers import T
    fx = _fixture()
    x = T(fx['x']).to(DEV)
    net = _net(fx, paired=paired).eval()
    with torch.no_grad():
        logits = net(x).cpu()
    ref = NC.check_eval_masks(logits, fx, 'lkm eval', logits_tol=1e-3)
    assert 0.2 <= ref.mean() <= 0.8
    cn = net.engine().net(tuple(x.shape), False)
    ops = [o[0] for o in cn.fwd.ops]
    assert 'bn_finalize' not in ops
    pairs = [s for (o, _, s) in cn.fwd.ops if o == 'gcn_pair']
    if paired:
        assert [(s.x.H, s.x.W, s.x.C) for s in pairs] == [(32, 32, 64), (16, 16, 128), (8, 8, 256), (4, 4, 512)]     # 4x4: every vertical tap clamps onto row 0
        assert all(s.K == 9 and s.yv.C == 21 and s.relu_v == 1 and s.relu_h == 1 for s in pairs)
    else:
        assert pairs == []          # the measured rule: the composed route at every shape (tests/test_lkm_cpu.py holds it to the table)
    NC.check_eval_graph_replay(cn, x, logits)
    NC.check_bf16_eval_guard(_net(fx, 'bf16', paired).eval(), x, logits, fx, 'lkm eval bf16', guard_factor=4)


@ROUTES
def test_one_training_step_matches_reference(paired):
    """zero_grad -> forward -> lovasz -> backward -> Adam(lr 1e-4, L2 1e-4) as models.py:105-136, by the procedures of
    tests/net_checks.py with the bounds tests/test_gpu_psp.py uses for F20: gradient norms (and sums) of tensors with 16 elements and
    more within 1e-2 relative, tensors under 16 elements within 1e-6 of the largest gradient norm, full gradients at 2e-2."""
    import net_checks as NC
    from helpers import T
    fx = _fixture()
    assert float(fx['ref_f32_vs_f64_gradnorm_rel']) <= 2.5e-3 and float(fx['ref_f32_vs_f64_small_abs']) <= 2.5e-7
    assert float(fx['ref_post_step_stability']) <= 0.25e-4          # the reference's own Adam step is stable under fp32-sized noise (make_golden_lkm.py)
    net = _net(fx, paired=paired)
    net.train()
    opt, out, eng, own, idx = NC.train_step_prologue(net, [T(fx['x']).to(DEV)], fx, logits_tol=2e-3, loss_tol=2e-3)
    cn = eng.net(tuple(fx['x'].shape), True)
    ops, bops = [o[0] for o in cn.fwd.ops], [o[0] for o in cn.bwd.ops]
    n = 4 if paired else 0          # forced: exactly four of each; shipped: the measured rule sends every level to the composed route
    assert ops.count('gcn_pair') == n and bops.count('gcn_pair_dgrad') == n
    assert 'head_bn' not in ops and 'head_bn_bwd' not in bops                         # the head follows a residual BatchNorm: never fused
    # under 16 elements: the two-element head bias
    NC.check_grad_tally(net, eng, own, idx, fx, 'lkm train:', include_small_below_norm_floor=True, min_checked=120, n_small=1,
                        norm_tol=1e-2, sum_tol=1e-2, small_tol=1e-6, verbose=True)
    full = fx['fullgrad_keys'].tolist()
    assert len(full) == 15 and float(fx['fullgrad_ref_f32_vs_f64'].max()) <= 5e-3
    for k in ('gcn5.conv1.0.conv.weight', 'gcn5.conv2.0.conv.weight', 'encoders.encoder.layer4.2.bn2.weight'):
        assert k in full, k
    NC.check_full_grads(eng, own, fx, full, tol=2e-2, verbose=True)
    sd = NC.check_after_adam(opt, net, own, idx, fx, norm_tol=1e-4, sum_tol=1e-4, bn_tol=1e-3, skip_bn=None)
    assert int(sd['gcn5.conv1.0.batch_norm.num_batches_tracked']) == 1 and int(sd['gcn5.conv2.0.batch_norm.num_batches_tracked']) == 1


def _model(dtype='bf16', lr=1e-3, cfg=None, paired=None):
    import net_checks as NC
    m = NC.family_model('LargeKernelMatters', dtype, lr, 1, cfg)
    m.model.paired = paired
    return m


@ROUTES
def test_step_graph_replay_equals_eager_steps(deterministic_sums, paired):
    """the procedure of tests/net_checks.py::step_graph_equals_eager at [2,3,64,64]: the training step captured into ONE hipGraph and
    replayed reproduces the eagerly launched steps bit for bit under the fixed summation order"""
    import net_checks as NC
    NC.step_graph_equals_eager(lambda: _model(paired=paired), lambda: NC.noise_batch(5, 2, 64), steps=4)


@ROUTES
def test_fit_two_steps(paired):
    """SegmentationModel.fit for two steps at [2,3,64,64]: the unchanged trainer (fused step) on the new architecture"""
    import net_checks as NC
    from salt_amd import architectures as A
    m, values = NC.fit_steps(lambda cfg: _model(cfg=cfg, paired=paired), A.LargeKernelMatters, NC.square_batch(3), 2)
    print('lkm fit losses', values)


def test_depth50_eval_matches_oracle():
    """LargeKernelMatters(50) at [1,3,32,32] (GCN inputs 256 .. 2048 channels wide, encoder5 2x2) in fp32 against tests/lkm_oracle.py, at
    the eval-logit bound; the pair forced at every level"""
    import net_checks as NC
    import lkm_oracle as LO
    from helpers import assert_close
    from salt_amd import architectures as A
    net = NC.fill_closed_form(A.LargeKernelMatters(50, 2, use_relu=True))
    net.paired = True
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(50))
    with torch.no_grad():
        ref = LO.lkm(sd, x, False, depth=50)
    net = net.set_compute_dtype('f32').to(DEV).eval()
    with torch.no_grad():
        logits = net(x.to(DEV)).cpu()
    e = assert_close(logits, ref, 1e-3, 'depth 50 eval logits')
    print('lkm50 eval rel err %.3e' % e)
    pairs = [s for (o, _, s) in net.engine().net(tuple(x.shape), False).fwd.ops if o == 'gcn_pair']
    assert [s.x.C for s in pairs] == [256, 512, 1024, 2048]


def test_composed_route_at_a_benchmark_tile_and_its_fold_kinds():
    """[8,3,128,128] on the shipped route (composed at every level): eval logits in fp32 against tests/lkm_oracle.py at the eval-logit
    bound, and one training step that leaves finite gradients.  The data gradients of the eight long line convolutions on the wide maps
    (pad 8) are pinned: the fused fold where the plan's tiles are larger than the pad, the strip fold where the plan refuses it
    (Graph._dgrad asks salt_conv_stats_parts; tests/test_lkm_cpu.py pins the host side of that question)."""
    import ctypes
    import net_checks as NC
    import lkm_oracle as LO
    from helpers import assert_close
    from salt_amd import architectures as A
    from salt_amd import losses
    from salt_amd._abi import lib
    from salt_amd.optim import FusedAdam, weight_regularization
    net = NC.fill_closed_form(A.LargeKernelMatters(34, 2, use_relu=True))
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x, t = NC.noise_batch(8, 8, 128)
    with torch.no_grad():
        ref = LO.lkm(sd, x, False)
    net = net.set_compute_dtype('f32').to(DEV).eval()
    with torch.no_grad():
        logits = net(x.to(DEV)).cpu()
    e = assert_close(logits, ref, 1e-3, 'composed route eval logits')
    print('lkm34 [8,3,128,128] eval rel err %.3e' % e)
    assert 'gcn_pair' not in [o[0] for o in net.engine().net(tuple(x.shape), False).fwd.ops]
    net.train()
    opt = FusedAdam(weight_regularization(net, True, 1e-4), lr=1e-4, model=net)
    out = net(x.to(DEV))
    losses.lovasz_loss(out, t.to(DEV)).backward()
    eng = net.engine()
    cn = eng.net(tuple(x.shape), True)
    assert 'gcn_pair' not in [o[0] for o in cn.fwd.ops] and 'gcn_pair_dgrad' not in [o[0] for o in cn.bwd.ops]
    wide = [s for (o, _, s) in cn.bwd.ops if o == 'conv' and max(s.fold_top, s.fold_right) == 8 and s.y.C >= 64]
    assert len(wide) == 8                                             # a (9, 1) and a (1, 9) data gradient per level
    for s in wide:
        # what the launch took must be what the plan says about the fused fold of these arguments: no strip where it accepts them
        fused = not s.strip
        probe = type(s).from_buffer_copy(s)
        probe.strip, probe.strip_cs = None, 0
        assert fused == (lib.salt_conv_stats_parts(ctypes.byref(probe)) >= 0), (s.y.H, s.y.W, s.y.C, s.fold_top, s.fold_right)
    kinds = {(s.y.H, s.fold_top): not s.strip for s in wide}
    print('fused fold by (map side, fold_top):', kinds)
    assert any(kinds.values())                                        # the larger maps keep the fused fold they had
    assert bool(torch.isfinite(eng.grads).all()) and float(eng.grads.abs().max()) > 0
    opt.step()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
