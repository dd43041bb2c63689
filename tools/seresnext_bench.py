#!/usr/bin/env python
"""Timings of UNetSeResNetXt(50) beside UNetSeResNet(50), one process, one GPU, [32,3,128,128], bf16:

  * train_step_ms   the full training step (SegmentationModel._fit_loop), an event pair per step, median over --reps steps after
                    --warmup steps; the two networks are measured in turn, --rounds times, and the medians of the rounds are reported
  * stages          per stage shape of the SE-ResNeXt50 encoder at that input, the grouped layer conv2 -> bn2 -> relu compiled alone
                    (Graph.gconv: salt_gconv, salt_gconv_dgrad, salt_gconv_wgrad) next to THE SAME LAYER run as a dense convolution
                    with block-diagonal weights (Graph.conv: salt_conv, its data gradient, salt_conv_wgrad + salt_wgrad_reduce) - the
                    dense stand-in is this A/B's baseline.  Event pairs around every program entry (Program.run_timed), median of
                    --reps runs; bytes/s = the tensors an operator has to touch once (bf16) over its time.

usage: python tools/seresnext_bench.py [--reps 20] [--warmup 5] [--rounds 2] [--out profiles/seresnext_bench.json] [--commit HASH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from torch import nn
import salt_amd                     # noqa: F401
from salt_amd import models
from salt_amd.engine import Graph
from salt_amd.runtime import Engine
from seresnet_bench import windows, build

# (width, H = W of the layer's input, stride) of conv2 in layer1, layer2[0], layer2[1:], layer3[0], layer3[1:], layer4[0], layer4[1:]
STAGES = [(128, 64, 1), (256, 64, 2), (256, 32, 1), (512, 32, 2), (512, 16, 1), (1024, 16, 2), (1024, 8, 1)]


class Layer(nn.Module):
    def __init__(self, width, stride, groups):
        super().__init__()
        self.conv = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn = nn.BatchNorm2d(width)


def dense_of(grouped):
    """the same layer as a dense convolution: block-diagonal weights, 31 zeros for every useful product"""
    C, Cg = grouped.conv.weight.shape[:2]
    d = Layer(C, grouped.conv.stride[0], 1)
    with torch.no_grad():
        d.conv.weight.zero_()
        for g in range(32):
            d.conv.weight[g * Cg:(g + 1) * Cg, g * Cg:(g + 1) * Cg] = grouped.conv.weight[g * Cg:(g + 1) * Cg]
    return d


def layer_times(layer, B, H, reps, warmup):
    """{program entry name: median ms} of the layer compiled alone in training mode (forward + backward programs)"""
    dev = torch.device('cuda:0')
    layer = layer.to(dev).train()
    eng = Engine(layer, dev, 'bf16')
    g = Graph(eng, True)
    C = layer.conv.weight.shape[0]
    x = g.alloc((B, C, H, H), torch.float32)
    x.copy_(torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(2)))
    a = g.from_nchw(x)
    y = g.gconv(a, layer.conv, layer.bn) if layer.conv.groups > 1 else g.conv(a, layer.conv, layer.bn, relu=True)
    out = g.alloc((y.B, y.C, y.H, y.W), torch.float32)
    g.to_nchw(y, out)
    g.build_backward()
    g.finalize()
    g.dlogits.copy_(torch.randn(tuple(g.dlogits.shape), generator=torch.Generator().manual_seed(3)))
    per = {}
    for i in range(warmup + reps):
        eng.refresh(True)
        seen = {}
        for tag, prog in (('fwd', g.fwd), ('bwd', g.bwd)):
            for op, _, ms in prog.run_timed():
                seen[tag + ':' + op] = seen.get(tag + ':' + op, 0.0) + ms
        torch.cuda.synchronize()
        if i >= warmup:
            for k, v in seen.items():
                per.setdefault(k, []).append(v)
    return {k: statistics.median(v) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--limit', type=int, default=60)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--commit', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seresnext_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('seresnext_bench needs the GPU: there is nothing to time without one')
    B, H, W = args.batch, args.size, args.size
    doc = {'commit': args.commit, 'device': torch.cuda.get_device_name(0), 'shape': [B, 3, H, W], 'dtype': 'bf16', 'rounds': [], 'stages': []}
    scale = H / 128.0
    for width, h, stride in STAGES:
        h = max(int(h * scale), 1)
        torch.manual_seed(width + h)
        grouped = Layer(width, stride, 32)
        tg, td = layer_times(grouped, B, h, args.reps, args.warmup), layer_times(dense_of(grouped), B, h, args.reps, args.warmup)
        oh = (h - 1) // stride + 1
        nbytes = 2 * B * width * (h * h + oh * oh)
        row = {'width': width, 'H': h, 'stride': stride, 'tensor_bytes': nbytes,
               'gconv_ms': tg['fwd:gconv'], 'gconv_dgrad_ms': tg['bwd:gconv_dgrad'], 'gconv_wgrad_ms': tg['bwd:gconv_wgrad'],
               'dense_conv_ms': td['fwd:conv'], 'dense_dgrad_ms': td['bwd:conv'], 'dense_wgrad_ms': td['bwd:conv_wgrad'] + td.get('bwd:wgrad_reduce', 0.0)}
        for k in ('gconv', 'gconv_dgrad', 'gconv_wgrad'):
            row[k + '_GBps'] = nbytes / (row[k + '_ms'] * 1e-3) / 1e9
        doc['stages'].append(row)
        print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}, flush=True)
    doc['stages_where_the_grouped_kernel_loses'] = [
        {'width': r['width'], 'H': r['H'], 'stride': r['stride'], 'operator': k}
        for r in doc['stages'] for k, d in (('gconv', 'dense_conv'), ('gconv_dgrad', 'dense_dgrad'), ('gconv_wgrad', 'dense_wgrad')) if r[k + '_ms'] > r[d + '_ms']]
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B, 3, H, W, generator=g).cuda()
    Mk = (torch.rand(B, 1, H, W, generator=g) > 0.6).float()
    T = torch.cat([1 - Mk, Mk], 1).cuda()
    nets = {'sext': build('UNetSeResNetXt', {}), 'se': build('UNetSeResNet', {})}
    for r in range(args.rounds):
        row = {}
        for name, m in nets.items():
            m.model.train()
            row[name] = windows(lambda: m._fit_loop([X, T]), 1, args.reps, args.warmup, args.limit)
        doc['rounds'].append(row)
        print('round', r, {k: round(v['median_ms'], 3) for k, v in row.items()}, flush=True)
    doc['train_step_ms'] = {name: statistics.median(row[name]['median_ms'] for row in doc['rounds']) for name in nets}
    eng = nets['sext'].model.engine()
    tn = eng.net(tuple(X.shape), True)
    per = {}
    for _ in range(5):
        eng.refresh(True)
        for prog in (tn.fwd, tn.bwd):
            for op, _, ms in prog.run_timed():
                per.setdefault(op, []).append(ms)
        torch.cuda.synchronize()
    total = {k: sum(v) / 5 for k, v in per.items()}
    doc['sext_entries_ms_total'] = sum(total.values())
    doc['sext_entries_ms'] = {k: total[k] for k in ('gconv', 'gconv_dgrad', 'gconv_wgrad', 'se_res', 'se_res_bwd', 'conv', 'conv_wgrad') if k in total}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
