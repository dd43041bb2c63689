#!/usr/bin/env python
"""Timings of PSPNet, one process, one GPU, bf16:

  * module          PSPModule(512, 1024) compiled alone in training mode at [B,512,8,8] and [B,512,16,16] (encoder5 of 128 x 128 and
                    256 x 256 tiles): the FACTORED path (Graph.psp: salt_psp_pool, 4 stage + 5 slice convolutions, salt_psp_merge and their
                    backward), entry by entry (Program.run_timed, event pairs) and as whole forward / forward + backward programs; next to
                    the SAME module composed from torch's own GPU operators (adaptive_avg_pool2d, conv2d, interpolate, cat, conv2d, relu;
                    bf16 parameters and activations, autograd for the backward), both sides in this one process, median of --reps windows
  * prelu           salt_bn_prelu / salt_bn_prelu_bwd on the output of up1 ([B,128,128,64])
  * train_step_ms   the full training step (SegmentationModel._fit_loop) and eval_forward_ms of PSPNet(34) and UNetResNet(34) at
                    [B,3,128,128], an event pair per call, median over --reps calls after --warmup

usage: python tools/psp_bench.py [--reps 20] [--warmup 5] [--out profiles/psp_bench.json] [--commit HASH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
import torch.nn.functional as F
import salt_amd                     # noqa: F401
from salt_amd import architectures as A
from salt_amd.engine import Graph
from salt_amd.runtime import Engine
from seresnet_bench import windows, build

SIZES = (1, 2, 3, 6)


def factored(B, C, Cout, h, reps, warmup, limit):
    """-> (per-entry median ms, forward program ms, forward + backward ms) of PSPModule compiled alone in training mode"""
    dev = torch.device('cuda:0')
    torch.manual_seed(h)
    m = A.PSPModule(C, Cout).to(dev).train()
    eng = Engine(m, dev, 'bf16')
    g = Graph(eng, True)
    x = g.alloc((B, C, h, h), torch.float32)
    x.copy_(torch.randn(B, C, h, h, generator=torch.Generator().manual_seed(2)))
    y = m.emit(g, g.from_nchw(x))
    out = g.alloc((y.B, y.C, y.H, y.W), torch.float32)
    g.to_nchw(y, out)
    g.build_backward()
    g.finalize()
    g.dlogits.copy_(torch.randn(tuple(g.dlogits.shape), generator=torch.Generator().manual_seed(3)))
    eng.refresh(True)
    per = {}
    for i in range(warmup + reps):
        seen = {}
        for tag, prog in (('fwd', g.fwd), ('bwd', g.bwd)):
            for op, _, ms in prog.run_timed():
                if op != 'layout':
                    seen[tag + ':' + op] = seen.get(tag + ':' + op, 0.0) + ms
        torch.cuda.synchronize()
        if i >= warmup:
            for k, v in seen.items():
                per.setdefault(k, []).append(v)
    side = eng.side_stream
    fwd = windows(lambda: g.fwd.run(side=side), 1, reps, warmup, limit)['median_ms']
    both = windows(lambda: (g.fwd.run(side=side), g.bwd.run(side=side)), 1, reps, warmup, limit)['median_ms']
    return {k: statistics.median(v) for k, v in per.items()}, fwd, both, m


def composed(m, B, C, h, reps, warmup, limit):
    """the same module from torch's own GPU operators, bf16, NCHW as torch prefers it -> (forward ms, forward + backward ms)"""
    ws = [st[1].weight.detach().clone().bfloat16().requires_grad_(True) for st in m.stages]
    wb = m.bottleneck.weight.detach().clone().bfloat16().requires_grad_(True)
    bb = m.bottleneck.bias.detach().clone().bfloat16().requires_grad_(True)
    x = torch.randn(B, C, h, h, generator=torch.Generator().manual_seed(2)).cuda().bfloat16().requires_grad_(True)
    gy = torch.randn(B, wb.shape[0], h, h, generator=torch.Generator().manual_seed(3)).cuda().bfloat16()

    def fwd():
        pri = [F.interpolate(F.conv2d(F.adaptive_avg_pool2d(x, s), w), size=(h, h), mode='bilinear', align_corners=False) for s, w in zip(SIZES, ws)]
        return F.relu(F.conv2d(torch.cat(pri + [x], 1), wb, bb))

    def both():
        for t in ws + [wb, bb, x]:
            t.grad = None
        fwd().backward(gy)
    with torch.no_grad():
        f = windows(fwd, 1, reps, warmup, limit)['median_ms']
    return f, windows(both, 1, reps, warmup, limit)['median_ms']


def prelu_times(B, H, C, reps, warmup):
    from salt_amd._abi import OP_FUNCS, fill, lib
    from salt_amd.engine import shaped_view
    import ctypes
    y = torch.randn(B, H, H, C, device='cuda').bfloat16()
    da, a = torch.randn_like(y), torch.empty_like(y)
    sc, sh, al, dal = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda'), torch.full((1,), 0.25, device='cuda'), torch.zeros(1, device='cuda')
    v = lambda t: shaped_view(t.data_ptr(), B, H, H, C)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn, S = OP_FUNCS['salt_bn_prelu']
    f = fill(S(), dtype=1, y=v(y), scale=sc.data_ptr(), shift=sh.data_ptr(), alpha=al.data_ptr(), a=v(a))
    fb, Sb = OP_FUNCS['salt_bn_prelu_bwd']
    b = fill(Sb(), dtype=1, da=v(da), y=v(y), scale=sc.data_ptr(), shift=sh.data_ptr(), alpha=al.data_ptr(), du=v(da), dalpha=dal.data_ptr())
    b.nparts = lib.salt_bn_prelu_bwd_parts(ctypes.byref(b))
    part = torch.zeros(b.nparts, device='cuda')
    b.partials = part.data_ptr()
    return {'bn_prelu_ms': windows(lambda: fn(ctypes.byref(f), st), 10, reps, warmup, 30)['median_ms'],
            'bn_prelu_bwd_ms': windows(lambda: fb(ctypes.byref(b), st), 10, reps, warmup, 30)['median_ms'], 'bytes_per_pass': 2 * y.numel() * 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--limit', type=int, default=60)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--commit', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'psp_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('psp_bench needs the GPU: there is nothing to time without one')
    B = args.batch
    doc = {'commit': args.commit, 'device': torch.cuda.get_device_name(0), 'dtype': 'bf16', 'module': []}
    for h in (8, 16):
        per, f, both, m = factored(B, 512, 1024, h, args.reps, args.warmup, args.limit)
        tf, tb = composed(m, B, 512, h, args.reps, args.warmup, args.limit)
        row = {'shape': [B, 512, h, h], 'factored_fwd_ms': f, 'factored_fwd_bwd_ms': both, 'torch_fwd_ms': tf, 'torch_fwd_bwd_ms': tb,
               'entries_ms': {k: round(v, 4) for k, v in sorted(per.items())}}
        doc['module'].append(row)
        print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}, flush=True)
    doc['prelu'] = prelu_times(B, 128, 64, args.reps, args.warmup)
    print(doc['prelu'], flush=True)
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B, 3, 128, 128, generator=g).cuda()
    Mk = (torch.rand(B, 1, 128, 128, generator=g) > 0.6).float()
    T = torch.cat([1 - Mk, Mk], 1).cuda()
    nets = {'pspnet34': build('PSPNet', {}), 'unet_resnet34': build('UNetResNet', {})}
    doc['train_step_ms'], doc['eval_forward_ms'] = {}, {}
    for name, mdl in nets.items():
        mdl.model.train()
        doc['train_step_ms'][name] = windows(lambda: mdl._fit_loop([X, T]), 1, args.reps, args.warmup, args.limit)['median_ms']
        mdl.model.eval()
        with torch.no_grad():
            doc['eval_forward_ms'][name] = windows(lambda: mdl.model(X), 1, args.reps, args.warmup, args.limit)['median_ms']
    print({'train_step_ms': doc['train_step_ms'], 'eval_forward_ms': doc['eval_forward_ms']}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
