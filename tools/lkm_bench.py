#!/usr/bin/env python
"""Timings of LargeKernelMatters, one process, one GPU, bf16:

  * block           GlobalConvolutionalNetwork(C, 21, 9, use_relu=True) compiled alone in training mode at the shapes of depth 34 at a
                    128 x 128 tile ([B,64,64,64] .. [B,512,8,8]), of depth 152's encoder5 ([B,2048,8,8]) and of a [2,3,64,64] batch ([2,64,32,32] .. [2,512,4,4]): the PAIRED route (Graph.gcn_pair:
                    one salt_gcn_pair launch, one salt_gcn_pair_dgrad) against the COMPOSED route (two Graph.conv launches, two fold-ring data
                    gradients) - both graphs built first, then timed alternately (--rounds rounds of paired, composed), forward and
                    forward + backward as whole programs (event pairs, median of --reps windows).  The spread of a figure is the
                    difference between its rounds; the per-entry times of the pair's own launches come from Program.run_timed.
  * train_step_ms   the full training step (SegmentationModel._fit_loop) and eval_forward_ms of LargeKernelMatters(34) as shipped (the
                    shape rule of Graph.gcn_pair decides the route of every GCN block), of the same network with the pair forced at every
                    level ('lkm34_pair_everywhere') and of UNetResNet(34), at [B,3,128,128], an event pair per call, median over --reps
                    calls after --warmup, --rounds alternating rounds over the three networks (every round is recorded)

Every measured step runs under --limit seconds of its own.

usage: python tools/lkm_bench.py --commit HASH [--reps 20] [--warmup 5] [--rounds 2] [--out profiles/lkm_bench.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import salt_amd                     # noqa: F401
from salt_amd import architectures as A
from salt_amd.engine import Graph
from salt_amd.runtime import Engine
from seresnet_bench import windows, build

SHAPES = [(64, 64), (128, 32), (256, 16), (512, 8), (2048, 8)]          # (channels, side) at --batch
SMALL = [(64, 32), (128, 16), (256, 8), (512, 4)]                       # depth 34 at a 64 x 64 tile, batch 2: the shapes of the F21 fixture


def block_graph(m, B, C, h, paired):
    dev = torch.device('cuda:0')
    eng = Engine(m, dev, 'bf16')
    g = Graph(eng, True)
    x = g.alloc((B, C, h, h), torch.float32)
    x.copy_(torch.randn(B, C, h, h, generator=torch.Generator().manual_seed(2)))
    y = m.emit(g, g.from_nchw(x), paired=paired)          # True forces the pair whatever Graph.gcn_pair_composed says: the A/B is what that rule is drawn from
    out = g.alloc((y.B, y.C, y.H, y.W), torch.float32)
    g.to_nchw(y, out)
    g.build_backward()
    g.finalize()
    g.dlogits.copy_(torch.randn(tuple(g.dlogits.shape), generator=torch.Generator().manual_seed(3)))
    eng.refresh(True)
    return eng, g


def entries(g, names, reps, warmup, limit):
    per, t0 = {}, time.time()
    for i in range(warmup + reps):
        if time.time() - t0 > limit:
            raise RuntimeError('per-entry timing passed its %d s limit' % limit)
        seen = {}
        for tag, prog in (('fwd', g.fwd), ('bwd', g.bwd)):
            for op, _, ms in prog.run_timed():
                if op in names:
                    seen[tag + ':' + op] = seen.get(tag + ':' + op, 0.0) + ms
        torch.cuda.synchronize()
        if i >= warmup:
            for k, v in seen.items():
                per.setdefault(k, []).append(v)
    return {k: round(statistics.median(v), 4) for k, v in sorted(per.items())}


def block_row(B, C, h, args):
    torch.manual_seed(h)
    m = A.GlobalConvolutionalNetwork(C, 21, 9, use_relu=True).to('cuda:0').train()
    sides = {name: block_graph(copy.deepcopy(m), B, C, h, name == 'paired') for name in ('paired', 'composed')}      # an Engine owns its module's parameters
    row = {'shape': [B, C, h, h]}
    rounds = {k: [] for k in ('paired_fwd_ms', 'paired_fwd_bwd_ms', 'composed_fwd_ms', 'composed_fwd_bwd_ms')}
    for _ in range(args.rounds):
        for name, (eng, g) in sides.items():
            side = eng.side_stream
            rounds[name + '_fwd_ms'].append(windows(lambda: g.fwd.run(side=side), 1, args.reps, args.warmup, args.limit)['median_ms'])
            rounds[name + '_fwd_bwd_ms'].append(windows(lambda: (g.fwd.run(side=side), g.bwd.run(side=side)), 1, args.reps, args.warmup, args.limit)['median_ms'])
    for k, v in rounds.items():
        row[k] = round(statistics.median(v), 4)
        row[k.replace('_ms', '_spread_ms')] = round(max(v) - min(v), 4)
    row['entries_ms'] = dict(paired=entries(sides['paired'][1], ('gcn_pair', 'gcn_pair_dgrad'), args.reps, args.warmup, args.limit),
                             composed=entries(sides['composed'][1], ('conv', 'pad_fold_strip'), args.reps, args.warmup, args.limit))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--limit', type=int, default=60)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--commit', required=True, help='the commit the measured tree stands on')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lkm_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lkm_bench needs the GPU: there is nothing to time without one')
    B = args.batch
    doc = {'commit': args.commit, 'device': torch.cuda.get_device_name(0), 'dtype': 'bf16', 'block': []}
    for Bb, shapes in ((B, SHAPES), (2, SMALL)):
        for C, h in shapes:
            row = block_row(Bb, C, h, args)
            doc['block'].append(row)
            print(row, flush=True)
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B, 3, 128, 128, generator=g).cuda()
    Mk = (torch.rand(B, 1, 128, 128, generator=g) > 0.6).float()
    T = torch.cat([1 - Mk, Mk], 1).cuda()
    nets = {'lkm34': build('LargeKernelMatters', {}), 'lkm34_pair_everywhere': build('LargeKernelMatters', {}), 'unet_resnet34': build('UNetResNet', {})}
    nets['lkm34_pair_everywhere'].model.paired = True          # the shipped default ('lkm34') follows the shape rule
    # alternating rounds over the networks, as for the blocks: the first network a process measures has run slower than the same network
    # measured later, so one pass in a fixed order does not compare them
    per = {name: {'train': [], 'eval': []} for name in nets}
    for _ in range(args.rounds):
        for name, mdl in nets.items():
            mdl.model.train()
            per[name]['train'].append(windows(lambda: mdl._fit_loop([X, T]), 1, args.reps, args.warmup, args.limit)['median_ms'])
            mdl.model.eval()
            with torch.no_grad():
                per[name]['eval'].append(windows(lambda: mdl.model(X), 1, args.reps, args.warmup, args.limit)['median_ms'])
    doc['train_step_ms'] = {name: statistics.median(v['train']) for name, v in per.items()}
    doc['eval_forward_ms'] = {name: statistics.median(v['eval']) for name, v in per.items()}
    doc['train_step_rounds_ms'] = {name: v['train'] for name, v in per.items()}
    doc['eval_forward_rounds_ms'] = {name: v['eval'] for name, v in per.items()}
    print({'train_step_rounds_ms': doc['train_step_rounds_ms'], 'eval_forward_rounds_ms': doc['eval_forward_rounds_ms']}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
