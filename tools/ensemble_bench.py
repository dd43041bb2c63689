"""Two routes from K member maps on the device to the B run lists of a submission, timed in one call.

    python tools/ensemble_bench.py [--calls 50] [--out profiles/ensemble_bench.json]

K = 6 members, B = 32 tiles, [B,2,128,128] fp32 probabilities each, centre crop to 101 x 101, threshold 0.5.
  host route     K device-to-host copies of the full maps, np.mean(np.array(crops), axis=0), threshold, inference.run_length_encoding per
                 mask: what a user has without csrc/ensemble.hip
  device route   ensemble.fold_masks (one salt_ensemble launch), ensemble.rle_encode (salt_rle_encode: two launches; counts + total, then
                 runs[:total], cross to the host)
Both are wall time from members-on-device to Python lists (perf_counter around the route, the device idle before and after), median /
p10 / p90 over --calls after warm-up; the two routes must give identical lists.  The bytes each route copies to the host are reported
beside the times."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
K, B, C, N, TARGET = 6, 32, 2, 128, (101, 101)


def stats(ms):
    v = np.asarray(ms)
    return {'median_ms': round(float(np.median(v)), 4), 'p10_ms': round(float(np.percentile(v, 10)), 4), 'p90_ms': round(float(np.percentile(v, 90)), 4),
            'n': int(len(v))}


def timed(fn, calls, warm=5):
    for _ in range(warm):
        out = fn()
    ms = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, stats(ms)


def members(dev):
    """six noisy views of one disc per tile; every third tile is empty, as a third of the dataset is"""
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(N), torch.arange(N), indexing='ij')
    truth = torch.zeros(B, N, N)
    for b in range(B):
        if b % 3:
            cy, cx, r = [int(v) for v in torch.randint(N // 4, 3 * N // 4, (3,), generator=g)]
            truth[b] = (((yy - cy) ** 2 + (xx - cx) ** 2) < max(r // 2, 8) ** 2).float()
    out = []
    for _ in range(K):
        p1 = torch.sigmoid(4.0 * (truth - 0.5) + 0.7 * torch.randn(B, N, N, generator=g))
        out.append(torch.stack([1 - p1, p1], 1).contiguous().to(dev))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ensemble_bench.json'))
    args = ap.parse_args()
    from salt_amd import ensemble as EN, inference as I
    dev = torch.device('cuda:0')
    probs = members(dev)
    top, left = I.crop_window(N, N, TARGET)

    def host_route():
        maps = [p.cpu().numpy() for p in probs]                                   # K copies of the full maps
        mean = np.mean(np.array([m[:, :, top:top + TARGET[0], left:left + TARGET[1]] for m in maps]), axis=0)
        masks = (mean[:, 1] > 0.5).astype(np.uint8)
        return [I.run_length_encoding(m) for m in masks]

    def device_route():
        return EN.rle_encode(EN.fold_masks(probs, target_size=TARGET, threshold=0.5))

    def device_kernels():                                                         # the launches alone, nothing crosses to the host
        m = EN.fold_masks(probs, target_size=TARGET, threshold=0.5)
        fn, S = EN.OP_FUNCS['salt_rle_encode']
        EN.check(fn(EN.ctypes.byref(EN.fill(S(), mask=m.data_ptr(), B=B, h=TARGET[0], w=TARGET[1], counts=scratch.data_ptr() + 8,
                                            runs=scratch.data_ptr() + 8 + 4 * B, cap_pairs=cap, total=scratch.data_ptr())), EN._stream()), 'rle')

    cap = B * ((TARGET[0] * TARGET[1] + 1) // 2)
    scratch = torch.empty((2 + B + 2 * cap,), dtype=torch.int32, device=dev)
    host_lists, host = timed(host_route, args.calls)
    dev_lists, device = timed(device_route, args.calls)
    _, kernels = timed(device_kernels, args.calls)
    assert host_lists == dev_lists, 'the two routes disagree'
    total_pairs = sum(len(r) // 2 for r in dev_lists)
    res = {'K': K, 'B': B, 'shape': [B, C, N, N], 'target': list(TARGET), 'runs_total': total_pairs,
           'host_route': dict(host, bytes_to_host=K * B * C * N * N * 4),
           'device_route': dict(device, bytes_to_host=8 + 4 * (B + (B & 1)) + 8 * total_pairs),
           'device_launches_only': kernels,
           'speedup_median': round(host['median_ms'] / device['median_ms'], 1),
           'device': torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
