"""The batch-flat Lovasz hinge program next to the two routes it is measured against, timed on the same device in one call.

    python tools/lovasz_flat_bench.py [--runs 200] [--out profiles/lovasz_flat_bench.json]

Logits and target [32,2,128,128] (the workload's shape), seeded.  Three programs alternate run by run, each bracketed by device events:
  flat        CompiledNet.loss_program('lovasz') with loss_params {'per_image': False}: one row of 1 048 576 elements through the
              long-row sort (histograms in global memory, 512 segments)
  one_wg      the same row through the only route there was before: salt_lovasz_hinge(B=1, P=1 048 576) without ws_split / ws_flat,
              one workgroup on one CU
  per_image   the default program: 32 rows of 32 768 through the split sort
and the median / p10 / p90 of --runs (>= 200) runs after warm-up are reported with the ratios one_wg / flat and flat / per_image."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
B, C, N = 32, 2, 128
KINDS = ('flat', 'one_wg', 'per_image')


def stats(ms):
    v = np.asarray(ms)
    return {'median_ms': round(float(np.median(v)), 4), 'p10_ms': round(float(np.percentile(v, 10)), 4), 'p90_ms': round(float(np.percentile(v, 90)), 4),
            'n': int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lovasz_flat_bench.json'))
    args = ap.parse_args()
    if args.runs < 200:
        ap.error('--runs must be at least 200')
    if not torch.cuda.is_available():
        raise SystemExit('lovasz_flat_bench needs a GPU: there is nothing to time without one')
    from salt_amd import _abi, architectures as A
    dev = torch.device('cuda:0')
    module = A.VanillaUNet(num_classes=C, in_channels=1, base_filters=16, levels=4).to(dev).train()      # only its logits buffers are used
    eng = module.engine(dev)
    net = eng.net((B, 1, N, N), True)
    g = torch.Generator().manual_seed(0)
    net.logits.copy_((torch.randn(B, C, N, N, generator=g) * 3).to(dev))
    m = (torch.rand(B, 1, N, N, generator=g) < 0.4).float()
    net.target.copy_(torch.cat([1 - m, m], 1).to(dev))
    eng.loss_params = None
    per_image = net.loss_program('lovasz', 1.0)
    eng.loss_params = {'per_image': False}
    flat = net.loss_program('lovasz', 1.0)
    eng.loss_params = None
    # the one-workgroup route: the same buffers as one row, no segment workspaces
    P = B * C * N * N
    wk = torch.empty(2 * P, dtype=torch.int32, device=dev)
    wv = torch.empty(2 * P, dtype=torch.int32, device=dev)
    row_loss = torch.empty(1, dtype=torch.float32, device=dev)
    fn, S = _abi.OP_FUNCS['salt_lovasz_hinge']
    one = _abi.fill(S(), logits=net.logits.data_ptr(), target=net.target.data_ptr(), B=1, P=P, ws_keys=wk.data_ptr(), ws_vals=wv.data_ptr(),
                    loss_per_image=row_loss.data_ptr(), loss=net.loss.data_ptr(), dlogits=net.dlogits.data_ptr(), loss_scale=1.0)

    def run_one():
        _abi.check(fn(ctypes.byref(one), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'lovasz_hinge')
    run = {'flat': flat.run, 'one_wg': run_one, 'per_image': per_image.run}
    losses, grads = {}, {}
    for _ in range(args.warmup):
        for k in KINDS:
            run[k]()
            losses[k] = float(net.loss[0])
            grads[k] = net.dlogits.clone()
    assert torch.equal(grads['flat'], grads['one_wg']), 'the long-row form and the one-workgroup kernel give different gradients'
    ms = {k: [] for k in KINDS}
    for _ in range(args.runs):
        for k in KINDS:                                                # alternate: the three see the same device state over time
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    st = {k: dict(stats(ms[k]), loss=losses[k]) for k in KINDS}
    res = {'shape': [B, C, N, N], 'device': torch.cuda.get_device_name(0), 'runs': args.runs, 'programs': st,
           'one_wg_over_flat': round(st['one_wg']['median_ms'] / st['flat']['median_ms'], 2),
           'flat_over_per_image': round(st['flat']['median_ms'] / st['per_image']['median_ms'], 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res, sort_keys=True))
    if not st['flat']['median_ms'] < st['one_wg']['median_ms']:
        raise SystemExit('the long-row form is not faster than one workgroup: it is broken')


if __name__ == '__main__':
    main()
