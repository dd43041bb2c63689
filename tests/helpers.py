"""Shared helpers for the test-suite (golden loading, closed-form state, comparisons)."""
import os
from collections import OrderedDict

import numpy as np
import torch

import closed_form as CF
from oracle import blocks as OB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def golden(name):
    with np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def state_from_fixture(fx, canonical=None):
    """Closed-form state BEFORE the pass for every 's:<key>' entry of a block fixture."""
    sd = OrderedDict()
    for k, v in fx.items():
        if k.startswith('s:'):
            key = k[2:]
            ck = canonical(key) if canonical else key
            sd[key] = CF.tensor_for(ck, v.shape)
    return sd


def expand_aliases(sd, aliases):
    """sd plus, for every {alias prefix: canonical prefix}, the canonical entries once more under the alias"""
    out = OrderedDict(sd)
    for a, c in aliases.items():
        for k, v in sd.items():
            if k.startswith(c):
                out[a + k[len(c):]] = v
    return out


def oracle_run(fn, sd, x, extras=()):
    x = x.clone().requires_grad_(True)
    extras = [e.clone().requires_grad_(True) for e in extras]
    leaves = {k: v for k, v in sd.items() if v.dtype.is_floating_point and not k.endswith(('running_mean', 'running_var'))}
    for v in leaves.values():
        v.requires_grad_(True)
    y = fn(x, *extras)
    return x, extras, leaves, y


# the oracle's restatement of the F1 - F4 block fixtures: name -> (state, train) -> forward
ORACLE_BLOCKS = {
    'F1_conv2dbnrelu_k33': lambda sd, tr: (lambda x: OB.conv2d_bn_relu(sd, '', x, tr)),
    'F1_conv2dbnrelu_k31': lambda sd, tr: (lambda x: OB.conv2d_bn_relu(sd, '', x, tr)),
    'F1_conv2dbnrelu_k13': lambda sd, tr: (lambda x: OB.conv2d_bn_relu(sd, '', x, tr)),
    'F2_convbnrelu': lambda sd, tr: (lambda x: OB.conv_bn_relu(sd, '', x, tr)),
    'F3_decoderv1': lambda sd, tr: (lambda x: OB.decoder_block_v1(sd, '', x, tr)),
    'F3_decoderv2_deconv': lambda sd, tr: (lambda x: OB.decoder_block_v2(sd, '', x, tr, True)),
    'F3_decoderv2_upsample': lambda sd, tr: (lambda x: OB.decoder_block_v2(sd, '', x, tr, False)),
    'F3_deconvconv2dbnrelu': lambda sd, tr: (lambda x: OB.deconv_conv2d_bn_relu(sd, '', x, tr)),
    'F4_decoderblock_skip': lambda sd, tr: (lambda x, e: OB.decoder_block(sd, '', x, e, tr)),
    'F4_decoderblock_noskip': lambda sd, tr: (lambda x: OB.decoder_block(sd, '', x, None, tr)),
    'F4_channel_se': lambda sd, tr: (lambda x: OB.channel_se(sd, '', x)),
    'F4_spatial_se': lambda sd, tr: (lambda x: OB.spatial_se(sd, '', x)),
}


def record_parity(name, **values):
    """SALT_PARITY_COUNTS=<file.json>: the parity tests of the BASELINE configs append their decision counts (mask pixels that differ from
    the oracle, totals, agreement) to that file - tools/r03_evidence.sh commits it as profiles/rNN_parity_counts.json."""
    path = os.environ.get('SALT_PARITY_COUNTS')
    if not path:
        return
    import json
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[name] = {k: (float(v) if isinstance(v, float) else int(v) if isinstance(v, (int, np.integer)) else v) for k, v in values.items()}
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def assert_close(a, b, tol, what=''):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().float().numpy()
    if isinstance(b, torch.Tensor):
        b = b.detach().cpu().float().numpy()
    assert a.shape == b.shape, '%s: shape %s vs %s' % (what, a.shape, b.shape)
    e = rel_err(a, b)
    assert e <= tol, '%s: max-rel err %.3e > %.1e' % (what, e, tol)
    return e
