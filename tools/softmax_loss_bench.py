"""The two softmax loss programs next to the Lovasz hinge program, timed on the same device in one call.

    python tools/softmax_loss_bench.py [--runs 200] [--out profiles/softmax_loss_bench.json]

Logits and target [32,2,128,128] (the workload's shape), seeded.  The programs are CompiledNet.loss_program's - the launches the fused
step and the step graph enqueue: 'lovasz' (hinge: one row of 2*128*128 per image), 'lovasz_softmax' (softmax, 64 rows of 128*128 through
the same sort, softmax Jacobian) and 'dice_ce' (partial sums, finalize, gradient).  Each run is bracketed by device events on the
stream; the three programs alternate run by run, and the median / p10 / p90 of --runs (>= 100) runs after warm-up are reported.  A
loss program is tens of microseconds of kernels, so these are times of launch chains on an otherwise idle stream, not kernel times."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
B, C, N = 32, 2, 128
KINDS = ('lovasz', 'lovasz_softmax', 'dice_ce')


def stats(ms):
    v = np.asarray(ms)
    return {'median_ms': round(float(np.median(v)), 4), 'p10_ms': round(float(np.percentile(v, 10)), 4), 'p90_ms': round(float(np.percentile(v, 90)), 4),
            'n': int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'softmax_loss_bench.json'))
    args = ap.parse_args()
    if args.runs < 100:
        ap.error('--runs must be at least 100')
    if not torch.cuda.is_available():
        raise SystemExit('softmax_loss_bench needs a GPU: there is nothing to time without one')
    from salt_amd import architectures as A
    dev = torch.device('cuda:0')
    module = A.VanillaUNet(num_classes=C, in_channels=1, base_filters=16, levels=4).to(dev).train()      # only its logits buffers are used
    net = module.engine(dev).net((B, 1, N, N), True)
    g = torch.Generator().manual_seed(0)
    net.logits.copy_((torch.randn(B, C, N, N, generator=g) * 3).to(dev))
    m = (torch.rand(B, 1, N, N, generator=g) < 0.4).float()
    net.target.copy_(torch.cat([1 - m, m], 1).to(dev))
    progs = {k: net.loss_program(k, 1.0) for k in KINDS}
    losses = {}
    for _ in range(args.warmup):
        for k in KINDS:
            progs[k].run()
            losses[k] = float(net.loss[0])
    ms = {k: [] for k in KINDS}
    for _ in range(args.runs):
        for k in KINDS:                                                # alternate: the three see the same device state over time
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            progs[k].run()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = {'shape': [B, C, N, N], 'device': torch.cuda.get_device_name(0), 'runs': args.runs,
           'programs': {k: dict(stats(ms[k]), entries=len(progs[k]), loss=losses[k]) for k in KINDS}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
