#!/usr/bin/env python
"""Two numbers for the emptiness classifier, neither of them a gate:

  * the median training-step time of EmptinessClassifier(ResNet18) at [32,3,128,128] bf16 (Lovasz + Adam through
    SegmentationModel._fit_loop): every step bracketed by events on the stream, device-synchronised before the first and after the last,
    median over --steps steps after --warmup warm-up steps;
  * the time of the two new launches (salt_pool_head forward, salt_pool_head_bwd) inside that step's programs, from Program.run_timed
    (an event pair around every entry), median over --timed runs of each program.

usage: python tools/emptiness_step.py [--steps 50] [--warmup 10] [--batch 32] [--out profiles/emptiness_step.json] [--commit HASH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import salt_amd                     # noqa: F401
from salt_amd import input_pipeline, models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--timed', type=int, default=20)
    ap.add_argument('--commit', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'emptiness_step.json'))
    args = ap.parse_args()
    cfg = {'model_params': {'architecture': 'EmptinessClassifier', 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
           'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    torch.manual_seed(0)
    m = models.SegmentationModel(cfg, {'epochs': 1}, {})
    m._to_device()
    m.model.train()
    g = torch.Generator().manual_seed(1)
    X = torch.randn(args.batch, 3, 128, 128, generator=g).cuda()
    T = input_pipeline.emptiness_target(torch.randint(0, 2, (args.batch,), generator=g)).cuda()
    for _ in range(args.warmup):
        m._fit_loop([X, T])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(args.steps):
        m._fit_loop([X, T])
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]
    eng = m.model.engine()
    net = eng.net(tuple(X.shape), True)
    ops = {'pool_head': [], 'pool_head_bwd': []}
    for _ in range(args.timed):
        eng.refresh(True)
        for prog in (net.fwd, net.bwd):
            for name, _, ms in prog.run_timed():
                if name in ops:
                    ops[name].append(ms)
        torch.cuda.synchronize()
    doc = {'commit': args.commit, 'device': torch.cuda.get_device_name(0), 'shape': list(X.shape), 'dtype': 'bf16', 'loss': 'lovasz',
           'steps': args.steps, 'warmup': args.warmup, 'median_step_ms': statistics.median(per), 'min_step_ms': min(per),
           'entries_fwd': len(net.fwd.ops), 'entries_bwd': len(net.bwd.ops),
           'pool_head_fwd_us': 1e3 * statistics.median(ops['pool_head']), 'pool_head_bwd_us': 1e3 * statistics.median(ops['pool_head_bwd']),
           'timed_runs': args.timed}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
