#!/usr/bin/env python
"""Timings of UNetDenseNet(121), one process, one GPU, [32,3,128,128], bf16:

  * layers          per dense-layer shape of denseblock1 / denseblock3 (and the transitions), norm1 -> relu -> conv1 (-> norm2 -> relu)
                    compiled alone in training mode.  FUSED: Graph.dense_conv (salt_dense_conv, salt_dense_conv_dgrad with norm1's backward
                    inside, salt_dense_conv_wgrad).  COMPOSED from existing operators: salt_affine_act into a normalised copy of the prefix,
                    then Graph.conv (salt_conv 1x1, its data gradient, salt_conv_wgrad + salt_wgrad_reduce); the composed side has NO backward
                    of norm1 (a salt_bn_bwd pass over the prefix it would still need), which favours it.  Event pairs around every program
                    entry (Program.run_timed), median of --reps runs, both sides in this one process.
  * train_step_ms   the full training step (SegmentationModel._fit_loop) and eval_forward_ms, an event pair per call, median over --reps
                    calls after --warmup, UNetDenseNet(121) and UNetSeResNet(50) in turn, --rounds times
  * activation_bytes what the training program of UNetDenseNet(121) allocates (Graph.bytes)

usage: python tools/densenet_bench.py [--reps 20] [--warmup 5] [--rounds 2] [--out profiles/densenet_bench.json] [--commit HASH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
from torch import nn
import salt_amd                     # noqa: F401
from salt_amd.engine import Graph
from salt_amd.runtime import Engine
from seresnet_bench import windows, build

# (name, Cin, Cout, H = W of the block at a 128 x 128 input, norm2 behind the convolution)
LAYERS = [('denseblock1.first', 64, 128, 64, True), ('denseblock1.last', 224, 128, 64, True), ('transition1', 256, 128, 64, False),
          ('denseblock3.first', 256, 128, 16, True), ('denseblock3.mid', 640, 128, 16, True), ('denseblock3.last', 992, 128, 16, True),
          ('transition3', 1024, 512, 16, False)]


class Layer(nn.Module):
    def __init__(self, cin, cout, norm2):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, cout, 1, bias=False)
        self.norm2 = nn.BatchNorm2d(cout) if norm2 else None


def layer_times(layer, fused, B, H, reps, warmup):
    """{program entry: median ms} of the layer compiled alone in training mode; the composed form's prefix copy is 'fwd:prefix_copy'"""
    dev = torch.device('cuda:0')
    layer = layer.to(dev).train()
    eng = Engine(layer, dev, 'bf16')
    g = Graph(eng, True)
    C = layer.conv1.weight.shape[1]
    x = g.alloc((B, C, H, H), torch.float32)
    x.copy_(torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(2)))
    a = g.from_nchw(x)
    copy_entry = None
    if fused:
        table = g.dense_table(a)
        g.dense_moments(a, table, 0)
        y = g.dense_conv(a, layer.norm1, layer.conv1, layer.norm2, table=table)
    else:
        w = eng.bn_work(layer.norm1)
        w['scale'].fill_(1.0)
        n = g.new_act(B, H, H, C, 'prefix_copy')
        copy_entry = g.fwd.add('affine_act', dtype=g.dt, y=a.view(), scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(), relu=1, a=n.view())
        y = g.conv(n, layer.conv1, layer.norm2, relu=layer.norm2 is not None)
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
            for op, s, ms in prog.run_timed():
                key = 'fwd:prefix_copy' if s is copy_entry else tag + ':' + op
                seen[key] = seen.get(key, 0.0) + ms
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'densenet_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('densenet_bench needs the GPU: there is nothing to time without one')
    B, H, W = args.batch, args.size, args.size
    doc = {'commit': args.commit, 'device': torch.cuda.get_device_name(0), 'shape': [B, 3, H, W], 'dtype': 'bf16', 'rounds': [], 'layers': []}
    for name, cin, cout, h, norm2 in LAYERS:
        h = max(int(h * H / 128.0), 1)
        torch.manual_seed(cin + h)
        tf = layer_times(Layer(cin, cout, norm2), True, B, h, args.reps, args.warmup)
        tc = layer_times(Layer(cin, cout, norm2), False, B, h, args.reps, args.warmup)
        row = {'layer': name, 'Cin': cin, 'Cout': cout, 'H': h, 'input_bytes': 2 * B * h * h * cin,
               'dense_conv_ms': tf['fwd:dense_conv'], 'dense_conv_dgrad_ms': tf['bwd:dense_conv_dgrad'], 'dense_conv_wgrad_ms': tf['bwd:dense_conv_wgrad'],
               'composed_fwd_ms': tc['fwd:prefix_copy'] + tc['fwd:conv'], 'composed_prefix_copy_ms': tc['fwd:prefix_copy'],
               'composed_dgrad_ms': tc['bwd:conv'], 'composed_wgrad_ms': tc['bwd:conv_wgrad'] + tc.get('bwd:wgrad_reduce', 0.0)}
        doc['layers'].append(row)
        print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}, flush=True)
    doc['where_the_fused_operator_loses'] = [
        {'layer': r['layer'], 'operator': k} for r in doc['layers']
        for k, d in (('dense_conv', 'composed_fwd'), ('dense_conv_dgrad', 'composed_dgrad'), ('dense_conv_wgrad', 'composed_wgrad')) if r[k + '_ms'] > r[d + '_ms']]
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B, 3, H, W, generator=g).cuda()
    Mk = (torch.rand(B, 1, H, W, generator=g) > 0.6).float()
    T = torch.cat([1 - Mk, Mk], 1).cuda()
    nets = {'densenet121': build('UNetDenseNet', {}), 'seresnet50': build('UNetSeResNet', {})}
    for r in range(args.rounds):
        row = {}
        for name, m in nets.items():
            m.model.train()
            row[name] = windows(lambda: m._fit_loop([X, T]), 1, args.reps, args.warmup, args.limit)
        doc['rounds'].append(row)
        print('round', r, {k: round(v['median_ms'], 3) for k, v in row.items()}, flush=True)
    doc['train_step_ms'] = {name: statistics.median(row[name]['median_ms'] for row in doc['rounds']) for name in nets}
    doc['eval_forward_ms'] = {}
    for name, m in nets.items():
        m.model.eval()
        with torch.no_grad():
            doc['eval_forward_ms'][name] = windows(lambda: m.model(X), 1, args.reps, args.warmup, args.limit)['median_ms']
    eng = nets['densenet121'].model.engine()
    tn = eng.net(tuple(X.shape), True)
    doc['activation_bytes'] = {name: int(m.model.engine().net(tuple(X.shape), True).g.bytes) for name, m in nets.items()}
    per = {}
    for _ in range(5):
        eng.refresh(True)
        for prog in (tn.fwd, tn.bwd):
            for op, _, ms in prog.run_timed():
                per.setdefault(op, []).append(ms)
        torch.cuda.synchronize()
    total = {k: sum(v) / 5 for k, v in per.items()}
    doc['densenet_entries_ms_total'] = sum(total.values())
    doc['densenet_entries_ms'] = {k: round(v, 4) for k, v in sorted(total.items(), key=lambda kv: -kv[1])[:14]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
