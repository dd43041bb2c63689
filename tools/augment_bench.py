"""Cost of the on-device training augmentation (DevicePreprocessor(augment=True), csrc/augment.hip).

    python tools/augment_bench.py [--calls 200] [--steps 100] [--out FILE] [--no-train]

1. DevicePreprocessor over [B,101,101] uint8 tiles + masks already on the GPU, augment off / on at B = 32 and 64, the legs alternating
   in one process: device events around every call, warm-up first; median and spread (p10 / p90) in microseconds.
2. A fused training loop (ResNet34 hypercolumn U-Net, bf16, Lovasz, B = 32) with the preprocessing inside the loop, off / on: ms per
   step over `--steps` steps after warm-up (device synchronise around the timed region).
The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (`--no-train`)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tiles(n, seed=1234):
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:101, 0:101].astype(np.float64)
    img = np.empty((n, 101, 101), np.uint8)
    msk = np.zeros((n, 101, 101), np.uint8)
    for b in range(n):
        img[b] = np.clip(120 + 60 * np.sin(xx / r.uniform(4, 15)) * np.cos(yy / r.uniform(4, 15)) + r.normal(0, 8, (101, 101)), 0, 255)
        msk[b] = (((yy - r.uniform(0, 101)) / r.uniform(10, 50)) ** 2 + ((xx - r.uniform(0, 101)) / r.uniform(10, 50)) ** 2 <= 1)
    return img, msk


def stats(v):
    v = np.asarray(v)
    return {'median_us': round(float(np.median(v)) * 1e3, 2), 'p10_us': round(float(np.percentile(v, 10)) * 1e3, 2),
            'p90_us': round(float(np.percentile(v, 90)) * 1e3, 2), 'n': int(len(v))}


def preprocess_legs(calls, dev):
    from salt_amd.input_pipeline import DevicePreprocessor
    out = {}
    for B in (32, 64):
        img, msk = tiles(B)
        xi, mi = torch.from_numpy(img).to(dev), torch.from_numpy(msk).to(dev)
        pres = {'off': DevicePreprocessor(True, 3), 'on': DevicePreprocessor(True, 3, augment=True, seed=1)}
        times = {k: [] for k in pres}
        for _ in range(20):
            for p in pres.values():
                p(xi, mi)
        torch.cuda.synchronize()
        for _ in range(calls):
            for k, p in pres.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); p(xi, mi); e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        out['B%d' % B] = {k: stats(v) for k, v in times.items()}
        out['B%d' % B]['added_median_us'] = round(out['B%d' % B]['on']['median_us'] - out['B%d' % B]['off']['median_us'], 2)
    return out


def train_legs(steps, dev):
    from salt_amd.models import SegmentationModel
    from salt_amd.input_pipeline import DevicePreprocessor
    B = 32
    img, msk = tiles(8 * B)
    xi, mi = torch.from_numpy(img).to(dev), torch.from_numpy(msk).to(dev)
    arch = {'model_params': {'architecture': 'UNetResNet', 'out_channels': 2, 'activation': 'sigmoid', 'loss': 'lovasz', 'compute_dtype': 'bf16'},
            'optimizer_params': {'lr': 1e-4}, 'regularizer_params': {'regularize': True, 'weight_decay_conv2d': 1e-4}}
    torch.manual_seed(0)
    model = SegmentationModel(arch, {'epochs': 1}, {})
    model._to_device(); model.model.train()
    pres = {'off': DevicePreprocessor(True, 3), 'on': DevicePreprocessor(True, 3, augment=True, seed=1)}
    out = {}
    for rnd in range(2):                                   # off, on, off, on: the second pass is reported
        for k, p in pres.items():
            for i in range(10):
                model._fit_loop(list(p(xi[(i % 8) * B:(i % 8 + 1) * B], mi[(i % 8) * B:(i % 8 + 1) * B])))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                model._fit_loop(list(p(xi[(i % 8) * B:(i % 8 + 1) * B], mi[(i % 8) * B:(i % 8 + 1) * B])))
            torch.cuda.synchronize()
            out.setdefault(k, []).append(round(1e3 * (time.perf_counter() - t0) / steps, 3))
    return {'batch': B, 'steps': steps, 'ms_per_step_off': out['off'], 'ms_per_step_on': out['on'],
            'added_ms_per_step': round(out['on'][-1] - out['off'][-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-train', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench needs a GPU')
    import salt_amd  # noqa: F401
    dev = torch.device('cuda:0')
    res = {'what': 'DevicePreprocessor augment off / on, device events per call (us); fused R34-hypercolumn bf16 training loop with '
                   'preprocessing inside, ms per step', 'device': torch.cuda.get_device_name(0), 'preprocess': preprocess_legs(a.calls, dev)}
    if not a.no_train:
        res['train'] = train_legs(a.steps, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
