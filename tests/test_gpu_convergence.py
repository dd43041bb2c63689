"""Driver-visible convergence parity of the headline model (VERDICT r3 next #6b): the ResNet34 hypercolumn U-Net trained for 20 Lovasz +
Adam steps (common_blocks/models.py:105-136; metrics.py:21-34,53-59 for the IoU) from IDENTICAL weights on IDENTICAL minibatches by
   the CPU oracle (fp32)  |  the HIP path in fp32  |  the HIP path in bf16 (the dtype bench.py's value is quoted on).
Train-mode BatchNorm through 50 layers amplifies fp32 summation-order noise, so two correct fp32 implementations drift apart step by
step; the yardstick is the oracle against ITSELF with another torch thread count (another partitioning of the same sums), measured
here, not quoted.  Round 3 only had a builder-run file (profiles/r03_convergence.json) for this."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, K, VAL = 8, 20, 128


def _oracle_run(X, T, sd0, spec, threads, val=None):
    from oracle import nets as ON, specs as OS, losses as OL
    torch.set_num_threads(threads)
    sd = {k: v.detach().clone() for k, v in sd0.items()}
    keys = [k for k in OS.trainable_keys(spec) if k not in ('encoders.encoder.fc.weight', 'encoders.encoder.fc.bias')]
    for k in keys:
        sd[k].requires_grad_(True)
    params = [sd[k] for k in keys]
    m_ = [torch.zeros_like(q) for q in params]
    v_ = [torch.zeros_like(q) for q in params]
    losses = []
    for it in range(K):
        for q in params:
            q.grad = None
        l = OL.LOSSES['lovasz'](ON.unet_resnet(sd, X[it * B:(it + 1) * B], True), T[it * B:(it + 1) * B])
        l.backward()
        with torch.no_grad():
            OL.adam_l2_step([q.data for q in params], [q.grad for q in params], m_, v_, it + 1, lr=1e-4)
        losses.append(float(l.detach()))
    iou = None
    if val is not None:
        with torch.no_grad():
            iou = val(lambda x: ON.unet_resnet(sd, x, False))
    return np.array(losses), iou


def test_r34_hypercolumn_20_steps_hip_f32_and_bf16_track_the_oracle():
    import bench
    from oracle import specs as OS
    from net_checks import segmentation_model
    img, msk = bench.synth_tiles(B * K, seed=4321)
    X, T = bench.preprocess(img, msk, True, 3)
    vi, vm = bench.synth_tiles(VAL, seed=999)
    Xv, _ = bench.preprocess(vi, vm, False, 3)
    gt = vm > 0.5

    def val_iou(forward_eval):
        preds = []
        for i in range(0, VAL, 32):
            lg = forward_eval(Xv[i:i + 32])
            preds.append((lg[:, 1, 13:114, 14:115] > 0).numpy())
        return bench.iou_metric(np.concatenate(preds), gt)

    spec = OS.SPECS['UNetResNet'](with_fc=True)
    sd0 = OS.init_state(spec, seed=7)
    ncpu = os.cpu_count() or 8
    t_main, t_ctrl = min(32, ncpu), max(2, min(8, ncpu // 2))
    prev = torch.get_num_threads()
    try:
        cpu, iou_cpu = _oracle_run(X, T, sd0, spec, t_main, val_iou)
        ctrl, _ = _oracle_run(X, T, sd0, spec, t_ctrl)
    finally:
        torch.set_num_threads(prev)
    envelope = float((np.abs(cpu - ctrl) / np.maximum(np.abs(cpu), 1e-6)).max())

    curves, ious = {}, {}
    for dtype in ('f32', 'bf16'):
        m = segmentation_model('UNetResNet', 'lovasz', dtype=dtype, lr=1e-4)
        m.model.load_state_dict({k: sd0[k] for k in m.model.state_dict() if k in sd0}, strict=False)
        m._to_device()
        m.model.train()
        ls = [float(m._fit_loop([X[it * B:(it + 1) * B], T[it * B:(it + 1) * B]])['sum']) for it in range(K)]
        m.model.eval()
        with torch.no_grad():
            ious[dtype] = val_iou(lambda x: m.model(x.to(DEV)).float().cpu())
        curves[dtype] = np.array(ls)
        del m
        torch.cuda.empty_cache()
    rel = {d: np.abs(curves[d] - cpu) / np.maximum(np.abs(cpu), 1e-6) for d in curves}
    print('convergence, R34 hypercolumn B=%d, %d steps: oracle(%d threads) vs oracle(%d threads) max rel dloss %.2e | HIP fp32 vs oracle %.2e '
          '(first 3 steps %.2e) | HIP bf16 vs oracle %.2e | val IoU after %d steps: oracle %.4f, HIP fp32 %.4f, HIP bf16 %.4f'
          % (B, K, t_main, t_ctrl, envelope, rel['f32'].max(), rel['f32'][:3].max(), rel['bf16'].max(), K, iou_cpu, ious['f32'], ious['bf16']))
    from helpers import record_parity
    record_parity('convergence_r34_hyper_b8_20steps', oracle_control_max_rel_dloss=envelope, hip_f32_max_rel_dloss=float(rel['f32'].max()),
                  hip_bf16_max_rel_dloss=float(rel['bf16'].max()), val_iou_cpu_oracle=float(iou_cpu), val_iou_hip_f32=float(ious['f32']),
                  val_iou_hip_bf16=float(ious['bf16']), oracle_threads=t_main, control_threads=t_ctrl)
    # fp32: identical to 1e-3 while rounding noise has not been amplified yet, inside the oracle's own envelope afterwards
    assert rel['f32'][:3].max() <= 2e-3, rel['f32'][:3]
    assert rel['f32'].max() <= max(3.0 * envelope, 1.2e-2), (rel['f32'].max(), envelope)
    # bf16 storage: a few percent per step (round 3's builder run: 2.7e-2), and the same place after 20 steps
    assert rel['bf16'].max() <= 8e-2, rel['bf16'].max()
    assert abs(ious['f32'] - iou_cpu) <= 0.03 and abs(ious['bf16'] - iou_cpu) <= 0.03, (iou_cpu, ious)
    assert cpu[-5:].mean() < cpu[:5].mean() and curves['bf16'][-5:].mean() < curves['bf16'][:5].mean()        # it learns
