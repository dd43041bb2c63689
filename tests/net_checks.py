"""Whole-network fixtures and trainer procedures shared by the GPU tests of the architecture families: closed-form weights, the
SegmentationModel factories, and the pieces of the eval and one-training-step comparisons against a fixture the reference produced.

Every tolerance, count and switch of a procedure is an argument without a default: the numbers stand in the test that owns them.
Fixed here is only what defines the compared step itself (Adam lr 1e-4 with L2 1e-4, models.py:105-136), the 1e-4 gradient-norm floor
below which a tensor is not compared relatively, and the 16 elements below which a tensor counts as small.

Importable without a GPU and without the built library: salt_amd is imported inside the functions."""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

import closed_form as CF
from helpers import T, assert_close

DEV = 'cuda:0'


def fill_closed_form(net):
    first = {}
    sd = net.state_dict()
    for k, v in sd.items():
        first.setdefault(v.data_ptr() if v.numel() else ('e', k), k)
    new = OrderedDict()
    for k, v in sd.items():
        ck = first[v.data_ptr() if v.numel() else ('e', k)]
        new[k] = CF.tensor_for(ck, v.shape).to(v.dtype)
    net.load_state_dict(new)
    return net


def grad_report(net, ref_grads):
    """Per-parameter relative L2 error and global cosine of the HIP gradients vs reference gradients.

    Whole-network gradients are only piecewise continuous: one ReLU / max-pool decision that flips under fp32
    summation-order noise moves a conv weight gradient by ~1/sqrt(pixels) ~ 1e-3..1e-2 (torch's own fp32 result is
    that far from its float64 result, measured in round 1), so the element-wise 1e-7 agreement of the block
    tests cannot hold here; L2 / cosine measures are the meaningful whole-net statistics."""
    eng = net.engine()
    worst, dots, n1, n2, n = (0.0, ''), 0.0, 0.0, 0.0, 0
    gmax = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
    for k, p in net.named_parameters():
        gr = ref_grads.get(k)
        if gr is None or float(gr.abs().max()) < 1e-7:
            continue
        off, cnt = eng.grad_range(p)
        mine = eng.grads[off:off + cnt].view(p.shape).cpu().double()
        gr = gr.double()
        if float(mine.abs().max()) == 0.0:
            # conv / deconv bias in front of train-mode BatchNorm: analytically zero (sum of the BN input gradient);
            # the HIP path writes exact zeros, the reference holds rounding noise
            assert float(gr.abs().max()) < 1e-3 * gmax, (k, float(gr.abs().max()), gmax)
            continue
        e = float((mine - gr).norm() / gr.norm())
        worst = max(worst, (e, k))
        dots += float((mine * gr).sum()); n1 += float((mine * mine).sum()); n2 += float((gr * gr).sum())
        n += 1
    return worst, dots / (n1 ** 0.5 * n2 ** 0.5), n


def family_model(arch_name, dtype, lr, epochs, cfg, **extra):
    """SegmentationModel (SegmentationModelWithDepth for a '...WithDepth' architecture) with the reference's regulariser settings and
    the Lovasz loss; ``extra`` adds to or overrides model_params."""
    from salt_amd import models
    cls = models.SegmentationModelWithDepth if arch_name.endswith('WithDepth') else models.SegmentationModel
    arch = {'model_params': dict({'architecture': arch_name, 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': dtype},
                                 **extra),
            'optimizer_params': {'lr': lr}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    return cls(arch, {'epochs': epochs}, cfg or {})


def segmentation_model(architecture, loss='lovasz', dtype='f32', lr=1e-4):
    return family_model(architecture, dtype, lr, 1, None, loss=loss)


def Losses():
    """a callback that records every step's loss"""
    from salt_amd import callbacks as C

    class Losses(C.Callback):
        def __init__(self):
            super().__init__()
            self.values = []

        def on_batch_end(self, metrics, *a, **k):
            self.values.append(float(metrics['sum']))
            self.batch_id += 1
    return Losses()


# ------------------------------------------------------------------------------------------------ eval
def margin_mask(fx):
    """pixels whose reference logit clears 10 x the reference's own fp32-vs-float64 error: where a mask decision is defined"""
    ref = fx['eval_logits'][:, 1]
    under = np.abs(ref) < 10 * float(fx['ref_f32_vs_f64_maxabs'])
    assert int(under.sum()) == int(fx['margin_pixels']) <= 0.001 * ref.size
    return ~under


def check_eval_masks(logits, fx, tag, logits_tol):
    """eval logits within logits_tol of the fixture's and equal masks wherever margin_mask allows -> the reference mask"""
    e = assert_close(logits, fx['eval_logits'], logits_tol, 'eval logits')
    safe = margin_mask(fx)
    mine, ref = (logits[:, 1] > 0).numpy(), fx['eval_logits'][:, 1] > 0
    print(tag, 'rel err %.3e' % e, 'pixels left out', int((~safe).sum()), 'mask differences', int((mine != ref).sum()))
    assert np.array_equal(mine[safe], ref[safe])
    return ref


def check_bf16_eval_guard(net16, x, logits, fx, tag, guard_factor):
    """bf16 storage: within guard_factor x what bf16 storage costs the test-side oracle, and the same masks wherever the fp32 logit
    clears that"""
    with torch.no_grad():
        l16 = net16(x).float().cpu()
    assert bool(torch.isfinite(l16).all())
    guard = guard_factor * float(fx['ref_bf16_storage_vs_f32_maxabs'])
    err16 = float((l16 - logits).abs().max())
    safe16 = (logits[:, 1].abs() > guard).numpy()
    print(tag, 'max |bf16 - f32| %.3e' % err16, 'guard %.3e' % guard, 'pixels under the guard', int((~safe16).sum()))
    assert err16 <= guard
    assert np.array_equal((l16[:, 1] > 0).numpy()[safe16], (logits[:, 1] > 0).numpy()[safe16])


def check_eval_graph_replay(cn, x, logits):
    """hipGraph replay of the eval program equals the eager run"""
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    cn.fwd.capture(st)
    with torch.cuda.stream(st):
        cn.logits.zero_()
        cn.x.copy_(x)
        cn.fwd.replay(st)
    st.synchronize()
    assert torch.equal(cn.logits.cpu(), logits)
    cn.fwd.release_graph()


# ------------------------------------------------------------------------------------------------ one training step
def train_step_prologue(net, inputs, fx, logits_tol, loss_tol):
    """FusedAdam(lr 1e-4, L2 1e-4) -> forward(*inputs) -> train logits -> lovasz -> backward -> loss, against the fixture
    -> (opt, out, eng, own, idx)"""
    from salt_amd.optim import FusedAdam, weight_regularization
    from salt_amd import losses
    opt = FusedAdam(weight_regularization(net, True, 1e-4), lr=1e-4, model=net)
    out = net(*inputs)
    assert_close(out.detach().cpu(), fx['train_logits'], logits_tol, 'train logits')
    loss = losses.lovasz_loss(out, T(fx['t']).to(DEV)) * 1.0
    loss.backward()
    ref = float(fx['train_loss'])
    assert abs(float(loss.detach()) - ref) < loss_tol * max(1.0, abs(ref)), (float(loss.detach()), ref)
    idx = {n: i for i, n in enumerate(fx['param_names'].tolist())}
    return opt, out, net.engine(), dict(net.named_parameters()), idx


def check_grad_tally(net, eng, own, idx, fx, tag, include_small_below_norm_floor, min_checked, n_small, norm_tol, sum_tol, small_tol, verbose):
    """Gradient norm and sum of every live tensor against the fixture: tensors of 16 elements and more relative to their own norm
    (norm_tol, sum_tol; more than min_checked of them), tensors under 16 elements relative to the largest gradient norm (small_tol;
    exactly n_small of them).  Tensors whose reference norm is under 1e-4 are left out, except that the small ones among them enter
    the tally with include_small_below_norm_floor."""
    dead = set(net.dead_parameter_names())
    gmax = float(fx['grad_norm'][fx['param_has_grad']].max())
    checked, small, worst, worst_sum, worst_small = 0, 0, (0.0, ''), (0.0, ''), (0.0, '')
    for k, p in own.items():
        i = idx[k]
        has = bool(fx['param_has_grad'][i])
        assert has == (k not in dead), k
        if has and (fx['grad_norm'][i] > 1e-4 or (include_small_below_norm_floor and p.numel() < 16)):
            off, n = eng.grad_range(p)
            g = eng.grads[off:off + n].double()
            if n < 16:
                e = max(abs(float(g.norm()) - fx['grad_norm'][i]), abs(float(g.sum()) - fx['grad_sum'][i])) / gmax
                if verbose:
                    print('  small tensor %s: %.3e of the largest norm (%.3e relative)' % (k, e, e * gmax / fx['grad_norm'][i]))
                worst_small = max(worst_small, (e, k))
                small += 1
                continue
            worst = max(worst, (abs(float(g.norm()) - fx['grad_norm'][i]) / fx['grad_norm'][i], k))
            worst_sum = max(worst_sum, (abs(float(g.sum()) - fx['grad_sum'][i]) / (fx['grad_norm'][i] * n ** 0.5), k))
            checked += 1
    print(tag, 'checked', checked, '+', small, 'small of', len(eng.live_params), 'worst grad norm', worst, 'worst grad sum', worst_sum,
          'worst small tensor', worst_small)
    assert checked > min_checked and small == n_small and worst[0] < norm_tol, (checked, small, worst)
    assert worst_sum[0] < sum_tol, worst_sum
    assert worst_small[0] < small_tol, worst_small


def check_full_grads(eng, own, fx, keys, tol, verbose):
    """the whole gradient of every parameter in keys against the fixture's 'fullgrad:<key>', max-norm relative"""
    for k in keys:
        p = own[k]
        off, n = eng.grad_range(p)
        e = assert_close(eng.grads[off:off + n].view(p.shape).cpu(), fx['fullgrad:' + k], tol, 'fullgrad:' + k)
        if verbose:
            print('  ', 'fullgrad:' + k, '%.3e' % e)


def check_after_adam(opt, net, own, idx, fx, norm_tol, sum_tol, bn_tol, skip_bn):
    """opt.step(), then every compared tensor's norm (and, unless sum_tol is None, sum) and the sums of the BatchNorm running
    statistics against the fixture; skip_bn: a substring of the statistics keys to leave out, or None -> the state dict"""
    opt.step()
    torch.cuda.synchronize()
    for k, p in own.items():
        i = idx[k]
        if fx['param_has_grad'][i] and fx['grad_norm'][i] > 1e-4:
            pn, ps = float(p.detach().double().norm()), float(p.detach().double().sum())
            assert abs(pn - fx['post_norm'][i]) <= norm_tol * max(fx['post_norm'][i], 1e-3), (k, pn, fx['post_norm'][i])
            if sum_tol is not None:
                assert abs(ps - fx['post_sum'][i]) <= sum_tol * max(fx['post_norm'][i] * p.numel() ** 0.5, 1e-3), (k, ps, fx['post_sum'][i])
    sd = net.state_dict()
    for k, s in zip(fx['bn_keys'].tolist(), fx['bn_sum'].tolist()):
        if skip_bn is not None and skip_bn in k:
            continue
        assert abs(float(sd[k].double().sum()) - s) <= bn_tol * max(1.0, abs(s)), k
    return sd


# ------------------------------------------------------------------------------------------------ step inputs
def _ptr_fields(struct, ptr, out):
    """(struct, field) of every pointer field of an argument struct (nested views / arrays included) that holds ``ptr``: the by-value
    search CompiledNet.bind used before the emitters recorded their step-input slots, kept as the oracle of those records"""
    for name, ct in struct._fields_:
        v = getattr(struct, name)
        if isinstance(v, ctypes.Structure):
            _ptr_fields(v, ptr, out)
        elif isinstance(v, ctypes.Array):
            for e in v:
                if isinstance(e, ctypes.Structure):
                    _ptr_fields(e, ptr, out)
        elif ct is ctypes.c_void_p and v == ptr:
            out.append((struct, name))
    return out


def recorded_and_searched_slots(net, which):
    """-> (recorded, searched, addresses of bwd's structs): the slots the programs of a CompiledNet recorded for step input ``which``
    and the fields that hold its static buffer's address by value, each as a set of (address of the holding struct, field).  A ctypes
    struct is identified by its address: a nested one gets a fresh Python object on every access."""
    progs = [net.fwd, net.bwd] + list(net._loss_progs.values())
    recorded, searched = set(), set()
    for prog in progs:
        for st, path, off in prog.slots.get(which, ()):
            assert off == 0
            for a in path[:-1]:
                st = getattr(st, a)
            recorded.add((ctypes.addressof(st), path[-1]))
        for _, _, st in prog.ops:
            searched |= {(ctypes.addressof(h), f) for h, f in _ptr_fields(st, getattr(net, which).data_ptr(), [])}
    return recorded, searched, {ctypes.addressof(st) for _, _, st in net.bwd.ops}


# ------------------------------------------------------------------------------------------------ trainer
def noise_batch(seed, B, size):
    """[B,3,size,size] noise with a random two-channel target"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, 3, size, size, generator=g)
    M = (torch.rand(B, 1, size, size, generator=g) > 0.6).float()
    return X, torch.cat([1 - M, M], 1)


def square_batch(seed):
    """[2,3,64,64] noise over a bright square, with the square as the target"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(2, 3, 64, 64, generator=g)
    M = torch.zeros(2, 1, 64, 64)
    M[:, :, 16:48, 8:40] = 1.0
    X = X * 0.3 + M
    return X, torch.cat([1 - M, M], 1)


def step_graph_equals_eager(make_model, batch_fn, steps):
    """the training step captured into ONE hipGraph (two-stream forward and backward, loss, Adam) and replayed reproduces the eagerly
    launched steps bit for bit under the fixed summation order: step 0 eager, step 1 captures, 2.. replay"""
    results = {}
    for mode in ('eager', 'graph'):
        torch.manual_seed(11)
        m = make_model()
        m.step_graph = mode == 'graph'
        m._to_device()
        m.model.train()
        X, Tt = batch_fn()
        ls = [float(m._fit_loop([X + 0.01 * i, Tt])['sum']) for i in range(steps)]
        torch.cuda.synchronize()
        eng = m.model.engine()
        results[mode] = (ls, eng.flat.clone(), eng.grads.clone(), sum(len(n.__dict__.get('_step_graphs', {})) for n in eng.nets.values()))
    assert results['graph'][3] == 1 and results['eager'][3] == 0
    assert results['eager'][0] == results['graph'][0] and all(np.isfinite(results['eager'][0]))
    assert torch.equal(results['eager'][2], results['graph'][2]) and torch.equal(results['eager'][1], results['graph'][1])


def fit_steps(make_model, arch_cls, batch, n):
    """SegmentationModel.fit for n steps on one batch (the fused step, unchanged trainer): n finite losses -> (model, the losses)"""
    torch.manual_seed(0)
    rec = Losses()
    m = make_model({'callbacks': [rec]})
    assert isinstance(m.model, arch_cls)
    X, Tt = batch
    m.fit(([[X, Tt]] * n, n))
    assert len(rec.values) == n and all(np.isfinite(rec.values))
    return m, rec.values
