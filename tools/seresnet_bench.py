#!/usr/bin/env python
"""Timings of UNetSeResNet(50) beside UNetResNet(50), one process, one GPU, [32,3,128,128], bf16:

  * train_step_ms     the full training step (SegmentationModel._fit_loop: forward, Lovasz, backward, Adam), an event pair per step,
                      median / min over --reps steps after --warmup steps; the three networks are measured in turn, --rounds times,
                      so that a drift of the box shows up as a difference between the rounds and not between the networks
  * eval_forward_ms   the compiled eval forward program, --inner runs between two events
  * se_res entries    event pairs around every program entry (Program.run_timed): the time and the share of the salt_se_res /
                      salt_se_res_bwd / salt_se_res_fc_grads entries (and of the salt_affine_act entries) in the training programs

networks: 'se' = UNetSeResNet(50) as built by default (the SE tail applies bn3 to the raw convolution output itself), 'se_stored' = the
same with SALT_SE_RES_IN_BN=0 (bn3's salt_affine_act stores the activation, the tail reads it), 'plain' = UNetResNet(50).

usage: python tools/seresnet_bench.py [--reps 30] [--warmup 8] [--rounds 2] [--out profiles/seresnet_bench.json] [--commit HASH]"""
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


def windows(fn, inner, reps, warmup, limit):
    """median / min time of one fn() call in ms: `inner` calls between two events, `reps` windows after `warmup` windows"""
    t0, out = time.time(), []
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


def build(arch, env):
    cfg = {'model_params': {'architecture': arch, 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
           'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    torch.manual_seed(0)
    m = models.SegmentationModel(cfg, {'epochs': 1}, {})
    m._to_device()
    m.bench_env = env
    return m


def with_env(env, fn):
    """the switches are read while a graph is BUILT (first step of a shape): set them around every call of that network"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--limit', type=int, default=60)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--commit', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seresnet_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('seresnet_bench needs the GPU: there is nothing to time without one')
    B, H, W = args.batch, args.size, args.size
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B, 3, H, W, generator=g).cuda()
    Mk = (torch.rand(B, 1, H, W, generator=g) > 0.6).float()
    T = torch.cat([1 - Mk, Mk], 1).cuda()
    # UNetResNet at depth 50: the registry's entry with the other depth, for this process only
    models.ARCHITECTURES['UNetResNet50'] = dict(models.ARCHITECTURES['UNetResNet'],
                                                model_config=dict(models.ARCHITECTURES['UNetResNet']['model_config'], encoder_depth=50))
    nets = {'se': build('UNetSeResNet', {}), 'se_stored': build('UNetSeResNet', {'SALT_SE_RES_IN_BN': '0'}), 'plain': build('UNetResNet50', {})}
    doc = {'commit': args.commit, 'device': torch.cuda.get_device_name(0), 'shape': [B, 3, H, W], 'dtype': 'bf16', 'rounds': [], 'networks': {}}
    for r in range(args.rounds):
        row = {}
        for name, m in nets.items():
            m.model.train()
            row[name] = with_env(m.bench_env, lambda: windows(lambda: m._fit_loop([X, T]), 1, args.reps, args.warmup, args.limit))
        doc['rounds'].append(row)
        print('round', r, {k: round(v['median_ms'], 3) for k, v in row.items()}, flush=True)
    for name, m in nets.items():
        d = doc['networks'][name] = {'train_step_ms': statistics.median(row[name]['median_ms'] for row in doc['rounds'])}
        eng = m.model.engine()
        tn = eng.net(tuple(X.shape), True)
        d['entries_fwd'], d['entries_bwd'] = len(tn.fwd.ops), len(tn.bwd.ops)
        per = {}
        for _ in range(5):
            eng.refresh(True)
            for prog in (tn.fwd, tn.bwd):
                for op, _, ms in prog.run_timed():
                    per.setdefault(op, []).append(ms)
            torch.cuda.synchronize()
        total = {k: sum(v) / 5 for k, v in per.items()}
        d['entries_ms_total'] = sum(total.values())
        d['entries_ms'] = {k: total[k] for k in ('se_res', 'se_res_bwd', 'se_res_fc_grads', 'affine_act', 'bn_bwd') if k in total}
        d['se_res_share_of_entries'] = sum(total.get(k, 0.0) for k in ('se_res', 'se_res_bwd', 'se_res_fc_grads')) / d['entries_ms_total']
        m.model.eval()
        with torch.no_grad():
            with_env(m.bench_env, lambda: m.model(X))
        en = eng.net(tuple(X.shape), False)
        d['eval_forward'] = windows(lambda: en.fwd.run(side=eng.side_stream), args.inner, max(args.reps // 2, 5), 3, args.limit)
    se, st, pl = (doc['networks'][k] for k in ('se', 'se_stored', 'plain'))
    doc['train_step_se_minus_plain_ms'] = se['train_step_ms'] - pl['train_step_ms']
    doc['train_step_stored_minus_taken_ms'] = st['train_step_ms'] - se['train_step_ms']
    doc['eval_forward_se_minus_plain_ms'] = se['eval_forward']['median_ms'] - pl['eval_forward']['median_ms']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
