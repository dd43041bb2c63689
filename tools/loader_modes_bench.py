"""Cost of the loader-mode kernels (csrc/resize.hip) against the host path a user has without them.

    python tools/loader_modes_bench.py [--calls 200] [--out profiles/loader_modes_bench.json]

1. salt_stack_resize on [32,101,101,M] -> [32,M,128,128], M = 5 / 32 / 64, both input layouts: device events around every launch after
   warm-up, median / p10 / p90 in microseconds, and the effective GB/s over the algorithmic bytes (input read once + output written once).
2. salt_mask_resize on [32,101,101] -> [32,2,128,128], the same way.
3. A 25-batch validation pass (B = 32, [B,2,128,128] probabilities, 21 thresholds) through salt_resize_iou_sweep, wall time with the
   counts copied back per batch as score_validation does; salt_iou_sweep on the centre crop is the kernel-time yardstick.
Host legs: the float64 numpy restatement (tests/loader_modes_reference.py) split over 16 threads, plus the copy to (or from) the device."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
THREADS = 16


def stats(ms):
    v = np.asarray(ms) * 1e3
    return {'median_us': round(float(np.median(v)), 2), 'p10_us': round(float(np.percentile(v, 10)), 2), 'p90_us': round(float(np.percentile(v, 90)), 2),
            'n': int(len(v))}


def device_leg(fn, calls):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


def host_leg(fn, reps=5):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {'median_ms': round(float(np.median(ms)), 2), 'min_ms': round(float(np.min(ms)), 2), 'n': reps, 'threads': THREADS}


def chunks(n):
    step = max(1, n // THREADS)
    return [slice(i, min(i + step, n)) for i in range(0, n, step)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('loader_modes_bench needs a GPU')
    import loader_modes_reference as L
    from salt_amd import inference as I
    from salt_amd.input_pipeline import StackingPreprocessor
    dev = torch.device('cuda:0')
    pool = ThreadPoolExecutor(THREADS)
    B, h, H = 32, 101, 128
    r = np.random.RandomState(1)
    res = {'what': 'salt_stack_resize / salt_mask_resize launches (device events, us) and a 25-batch resized validation sweep (ms) against the '
                   'float64 numpy restatement on %d host threads + the copy' % THREADS, 'device': torch.cuda.get_device_name(0), 'batch': B}
    pre = StackingPreprocessor((H, H))
    for M in (5, 32, 64):
        x = r.random_sample((B, h, h, M)).astype(np.float32)
        xd = torch.from_numpy(x).to(dev)
        xp = xd.permute(0, 3, 1, 2).contiguous()
        nbytes = 4 * B * M * (h * h + H * H)
        leg = {'algorithmic_MB': round(nbytes / 1e6, 2)}
        for name, t in (('hwm', xd), ('mhw', xp)):
            s = device_leg(lambda: pre(t), a.calls)
            s['GBps'] = round(nbytes / (s['median_us'] * 1e-6) / 1e9, 1)
            leg[name] = s

        def host():
            parts = list(pool.map(lambda sl: L.stack_resize(x[sl], (H, H)).astype(np.float32), chunks(B)))
            torch.from_numpy(np.concatenate(parts)).to(dev)
            torch.cuda.synchronize()
        leg['host'] = host_leg(host)
        res['stack_resize_M%d' % M] = leg
    masks = (r.random_sample((B, h, h)) < 0.4).astype(np.uint8)
    md = torch.from_numpy(masks).to(dev)
    x5 = torch.from_numpy(r.random_sample((B, h, h, 5)).astype(np.float32)).to(dev)
    both = device_leg(lambda: pre(x5, md), a.calls)
    only = device_leg(lambda: pre(x5), a.calls)
    res['mask_resize'] = {'stack_M5_and_mask': both, 'stack_M5_only': only, 'mask_added_median_us': round(both['median_us'] - only['median_us'], 2)}

    def host_mask():
        parts = list(pool.map(lambda sl: L.mask_target(masks[sl], (H, H)), chunks(B)))
        torch.from_numpy(np.concatenate(parts)).to(dev)
        torch.cuda.synchronize()
    res['mask_resize']['host'] = host_leg(host_mask)
    # ---- validation pass
    nb = 25
    probs = [torch.from_numpy(r.random_sample((B, 2, H, H)).astype(np.float32)).to(dev) for _ in range(nb)]
    gts = [torch.from_numpy((r.random_sample((B, h, h)) < 0.4).astype(np.uint8)).to(dev) for _ in range(nb)]
    th = np.linspace(0.5, 0.3, 21)

    def sweep(fn):
        def run():
            for p, g in zip(probs, gts):
                fn(p, g, th)
            torch.cuda.synchronize()
        return run
    res['validation_25_batches'] = {'resize_iou_sweep': host_leg(sweep(I.iou_counts_resized), 9), 'iou_sweep_crop': host_leg(sweep(I.iou_counts), 9)}
    for k in ('resize_iou_sweep', 'iou_sweep_crop'):
        del res['validation_25_batches'][k]['threads']
    res['validation_25_batches']['resize_iou_sweep_one_batch'] = device_leg(lambda: I.iou_counts_resized(probs[0], gts[0], th), 50)
    res['validation_25_batches']['iou_sweep_crop_one_batch'] = device_leg(lambda: I.iou_counts(probs[0], gts[0], th), 50)

    def host_valid():
        for p, g in zip(probs, gts):
            pn, gn = p[:, 1].cpu().numpy(), g.cpu().numpy()
            list(pool.map(lambda sl: L.counts(L.resize_back(pn[sl], (h, h)), gn[sl], th), chunks(B)))
    res['validation_25_batches']['host'] = host_leg(host_valid, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
