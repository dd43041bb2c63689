#!/usr/bin/env python
"""What the depth gate costs: the C2 training step ([32,3,128,128], bf16, Lovasz, Adam through SegmentationModel._fit_loop) of UNetResNet
and of UNetResNetWithDepth, timed in ONE process on one GPU - interleaved blocks of steps, so both see the same clocks - plus the
operator counts of the two compiled training instances.  Per model: warm-up, then the median over the per-step times (each step
bracketed by events on the stream; the host stays ahead of the device) and the block-mean (wall time of a block / its steps).

usage: python tools/bench_depth.py [--steps 60] [--warmup 15] [--blocks 3] [--out profiles/depth_bench.json]
       [--bench-json FILE ...]   headline lines of `python bench.py` runs to record next to it (label=path, e.g. parent=/tmp/p.json)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import salt_amd                     # noqa: F401
from salt_amd import models


def build(arch, with_depth, batch):
    cfg = {'model_params': {'architecture': arch, 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
           'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    torch.manual_seed(0)
    m = (models.SegmentationModelWithDepth if with_depth else models.SegmentationModel)(cfg, {'epochs': 1}, {})
    m._to_device()
    m.model.train()
    g = torch.Generator().manual_seed(1)
    X = torch.randn(batch, 3, 128, 128, generator=g).cuda()
    M = (torch.rand(batch, 1, 128, 128, generator=g) > 0.6).float()
    T = torch.cat([1 - M, M], 1).cuda()
    D = torch.rand(batch, 1, generator=g).cuda()
    return m, ([X, D, T] if with_depth else [X, T])


def block(m, data, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    for i in range(steps):
        m._fit_loop(data)
        ev[i + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)], wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=15)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'depth_bench.json'))
    ap.add_argument('--bench-json', nargs='*', default=[])
    args = ap.parse_args()
    nets = {'UNetResNet': build('UNetResNet', False, args.batch), 'UNetResNetWithDepth': build('UNetResNetWithDepth', True, args.batch)}
    for m, data in nets.values():
        block(m, data, args.warmup)
    per, walls = {k: [] for k in nets}, {k: [] for k in nets}
    for _ in range(args.blocks):
        for k, (m, data) in nets.items():
            ms, wall = block(m, data, args.steps // args.blocks)
            per[k] += ms
            walls[k].append(wall)
    doc = {'shape': [args.batch, 3, 128, 128], 'dtype': 'bf16', 'loss': 'lovasz', 'device': torch.cuda.get_device_name(0),
           'steps_per_model': len(per['UNetResNet']), 'warmup': args.warmup, 'blocks': args.blocks}
    for k, (m, data) in nets.items():
        net = m.model.engine().net(tuple(data[0].shape), True)
        names = [o[0] for o in net.fwd.ops + net.bwd.ops]
        doc[k] = {'median_step_ms': statistics.median(per[k]), 'min_step_ms': min(per[k]), 'block_wall_ms': walls[k],
                  'entries_fwd': len(net.fwd.ops), 'entries_bwd': len(net.bwd.ops),
                  'gate_entries': sum(1 for n in names if n in ('depth_gate', 'channel_gate'))}
    doc['depth_minus_plain_median_ms'] = doc['UNetResNetWithDepth']['median_step_ms'] - doc['UNetResNet']['median_step_ms']
    doc['bench_py'] = {}
    for item in args.bench_json:
        label, path = item.split('=', 1)
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith('{')]
        doc['bench_py'].setdefault(label, []).append(json.loads(lines[-1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({k: doc[k] for k in ('UNetResNet', 'UNetResNetWithDepth', 'depth_minus_plain_median_ms')}))


if __name__ == '__main__':
    main()
