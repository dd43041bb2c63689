#!/usr/bin/env python
"""Timings of the second-level (stacking) network, one process, one GPU, StackingFCN at
B = 32, M = 32, F = 32, K = 2, 128 x 128, in bf16 and fp32:

  * eval_program_ms      the fused eval forward: the compiled forward program (ONE salt_stack_conv launch) run --inner times between two
                         events on the stream, per run; median / min over --reps such windows after --warmup windows
  * eval_call_ms         the same through StackingFCN.__call__ (adds the host path and the clone of the logits)
  * train_step_ms        the full training step (SegmentationModel._fit_loop: forward, Lovasz, backward, Adam), an event pair per step
  * torch_eval_ms        tests/stacking_oracle.py (plain torch, the same network from the same state dict) in eval mode on the same
                         GPU in torch eager, timed like eval_program_ms.  bf16: the fp32 batch is cast to torch.bfloat16 inside the
                         timed region (the loader hands over fp32) and the layers run in torch's own bf16

plus the algorithmic bytes (eval: the fp32 input once + the fp32 logits; training: also y, xs and dL/dy written and read once each, the
activation and its gradient written and read once each, and the logits' gradient) and the fraction of the 8.0 TB/s HBM rate
(MI355X data sheet) those bytes over the measured time amount to.  Every measurement has a wall-clock limit (--limit seconds): a window
that would pass it ends the measurement with the windows it has, fewer than three is an error.

usage: python tools/stacking_bench.py [--reps 20] [--warmup 5] [--inner 20] [--out profiles/stacking_bench.json] [--commit HASH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch
import salt_amd                     # noqa: F401
from salt_amd import models
import stacking_oracle as SO

HBM_PEAK = 8.0e12


def windows(fn, inner, reps, warmup, limit):
    """median / min time of one fn() call in ms: `inner` calls between two events, `reps` windows after `warmup` windows"""
    t0 = time.time()
    out = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b) / inner)
        if time.time() - t0 > limit:
            break
    if len(out) < 3:
        raise RuntimeError('measurement passed its %d s limit after %d windows' % (limit, len(out)))
    return {'median_ms': statistics.median(out), 'min_ms': min(out), 'windows': len(out), 'inner': inner}


def algorithmic_bytes(B, M, F, K, H, W, es):
    px = B * H * W
    Mpad = (M + 15) // 16 * 16
    ev = px * M * 4 + px * K * 4
    tr = ev + 2 * px * F * es + 2 * px * Mpad * es + 2 * px * F * es + 4 * px * F * es + px * K * 4
    return ev, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--limit', type=int, default=60)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--commit', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stacking_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stacking_bench needs the GPU: there is nothing to time without one')
    B, M, F, K, H, W = args.batch, 32, 32, 2, args.size, args.size
    g = torch.Generator().manual_seed(1)
    X = torch.rand(B, M, H, W, generator=g).cuda()
    Mk = (torch.rand(B, 1, H, W, generator=g) > 0.6).float()
    T = torch.cat([1 - Mk, Mk], 1).cuda()
    doc = {'commit': args.commit, 'device': torch.cuda.get_device_name(0), 'shape': [B, M, H, W], 'filters': F, 'classes': K,
           'hbm_peak_bytes_per_s': HBM_PEAK, 'reps': args.reps, 'warmup': args.warmup, 'dtypes': {}}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)

    for dtype, es in (('bf16', 2), ('f32', 4)):
        cfg = {'model_params': {'architecture': 'StackingFCN', 'out_channels': K, 'activation': 'sigmoid', 'loss': 'lovasz',
                                'compute_dtype': dtype, 'input_model_nr': M, 'filter_nr': F},
               'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
        torch.manual_seed(0)
        m = models.SegmentationModel(cfg, {'epochs': 1}, {})
        m._to_device()
        net = m.model
        ev_bytes, tr_bytes = algorithmic_bytes(B, M, F, K, H, W, es)
        d = doc['dtypes'][dtype] = {'eval_bytes': ev_bytes, 'train_bytes': tr_bytes}
        # ---- fused eval forward
        net.eval()
        with torch.no_grad():
            ref = net(X).float()
        eng = net.engine()
        cnet = eng.net(tuple(X.shape), False)
        assert [o[0] for o in cnet.fwd.ops] == ['stack_conv']
        d['eval_program'] = windows(lambda: cnet.fwd.run(), args.inner, args.reps, args.warmup, args.limit)
        with torch.no_grad():
            d['eval_call'] = windows(lambda: net(X), args.inner, args.reps, args.warmup, args.limit)
        # ---- torch eager on the same box, same state
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        if dtype == 'bf16':
            sdt = {k: (v.bfloat16() if v.is_floating_point() else v) for k, v in sd.items()}
            eager = lambda: SO.stacking_fcn(sdt, X.bfloat16(), False)
        else:
            eager = lambda: SO.stacking_fcn(sd, X, False)
        with torch.no_grad():
            got = eager().float()
            d['torch_vs_hip_eval_maxabs'] = float((got - ref).abs().max())
            d['torch_eval'] = windows(eager, args.inner, args.reps, args.warmup, args.limit)
        d['eval_speedup_vs_torch_eager'] = d['torch_eval']['median_ms'] / d['eval_program']['median_ms']
        d['eval_call_speedup_vs_torch_eager'] = d['torch_eval']['median_ms'] / d['eval_call']['median_ms']
        d['eval_hbm_fraction'] = ev_bytes / (d['eval_program']['median_ms'] * 1e-3) / HBM_PEAK
        save()
        # ---- full training step
        net.train()
        d['train_step'] = windows(lambda: m._fit_loop([X, T]), 1, max(args.reps, 30), args.warmup, args.limit)
        d['train_hbm_fraction'] = tr_bytes / (d['train_step']['median_ms'] * 1e-3) / HBM_PEAK
        tn = eng.net(tuple(X.shape), True)
        d['entries_fwd'], d['entries_bwd'] = len(tn.fwd.ops), len(tn.bwd.ops)
        per = {}
        for _ in range(10):
            eng.refresh(True)
            for prog in (tn.fwd, tn.bwd):
                for name, _, ms in prog.run_timed():
                    per.setdefault(('fwd.' if prog is tn.fwd else 'bwd.') + name, []).append(ms)
            torch.cuda.synchronize()
        d['train_entries_us'] = {k: 1e3 * statistics.median(v) for k, v in per.items()}
        save()
        print(dtype, json.dumps(d))
        if d['eval_speedup_vs_torch_eager'] <= 1.0:
            raise SystemExit('the fused eval forward (%s) is not faster than torch eager: %.3f ms vs %.3f ms'
                             % (dtype, d['eval_program']['median_ms'], d['torch_eval']['median_ms']))
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
