"""Run a block (or a hand-built operator chain) of the HIP path on cuda:0 and hand back NCHW fp32 results; the seeded operands, the
forced convolution config and the block table several GPU test modules share.

Importable without a GPU and without the built library: salt_amd is imported inside the functions."""
import ctypes
from collections import OrderedDict

import torch

import closed_form as CF

DEV = 'cuda:0'


class BlockRun:
    """Compile ``emit_fn(g, *acts) -> act`` over NCHW inputs; forward + backward with upstream grad ``gy``."""

    def __init__(self, module, inputs, emit_fn, train=True, dtype='f32', backward=True):
        from salt_amd.engine import Graph
        from salt_amd.runtime import Engine
        self.module = module.to(DEV)
        self.eng = Engine(self.module, torch.device(DEV), dtype)
        g = Graph(self.eng, train)
        self.g = g
        self.xs = [g.alloc(tuple(x.shape), torch.float32) for x in inputs]
        for t, x in zip(self.xs, inputs):
            t.copy_(x)
        acts = [g.from_nchw(t) for t in self.xs]
        y = emit_fn(g, *acts)
        self.out = g.alloc((y.B, y.C, y.H, y.W), torch.float32)
        g.to_nchw(y, self.out)
        if train and backward:
            g.build_backward()
        elif train:
            g._resolve_lazies()                 # forward-only graph (SALT_FWD_BN_FOLD): what build_backward would have done to the forward program
        g.finalize()

    def forward(self):
        self.eng.refresh(self.g.train)
        self.g.fwd.run(side=self.eng.side_stream)
        torch.cuda.synchronize()
        return self.out.cpu()

    def backward(self, gy):
        self.g.dlogits.copy_(gy)
        self.g.bwd.run(side=self.eng.side_stream)
        torch.cuda.synchronize()
        gx = [t.cpu() for t in self.g.input_grads]
        grads = OrderedDict()
        for name, p in self.module.named_parameters():
            if id(p) in self.eng._off:
                off, n = self.eng.grad_range(p)
                grads[name] = self.eng.grads[off:off + n].view(p.shape).cpu()
        return gx, grads


def load_into(module, sd):
    """Load a {key: tensor} dict (reference key names) into a module built from salt_amd classes."""
    own = module.state_dict()
    missing = [k for k in own if k not in sd]
    assert not missing, missing[:5]
    module.load_state_dict({k: sd[k] for k in own})
    return module


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _force_cfg(g, cfg):
    orig = g._conv_launch

    def launch(*args, **kw):
        kw.setdefault('cfg', cfg)
        return orig(*args, **kw)
    g._conv_launch = launch
    orig_parts = g._conv_parts
    g._conv_parts = lambda *a_, **k_: orig_parts(*a_, cfg=cfg, **k_)


def _kernel_ids(prog):
    from salt_amd._abi import lib
    return [lib.salt_conv_kernel_id(ctypes.byref(s)) for name, _, s in prog.ops if name == 'conv']


def _data(n, seed):
    """n 128x128 one-channel tiles, two of every three noise plus a disc, with the disc as the target"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(128), torch.arange(128), indexing='ij')
    X = torch.randn(n, 1, 128, 128, generator=g) * 0.3
    M = torch.zeros(n, 1, 128, 128)
    for i in range(n):
        if i % 3 == 0:
            continue
        cy, cx, r = [int(v) for v in torch.randint(30, 98, (3,), generator=g)]
        M[i, 0] = (((yy - cy) ** 2 + (xx - cx) ** 2) < (r // 2) ** 2).float()
    X = X + 0.9 * M
    return X, torch.cat([1 - M, M], 1)


def _mods():
    from salt_amd import architectures as A
    return A


def _fixture_state(fx, module):
    sd = {}
    for k, v in module.state_dict().items():
        sd[k] = CF.tensor_for(k, v.shape).to(v.dtype)
    return sd


# the F1 - F4 block fixtures: name -> (module from the package's architectures, its emit function)
BLOCKS = {
    'F1_conv2dbnrelu_k33': (lambda A: A.Conv2dBnRelu(3, 8), lambda m: (lambda g, x: m.emit(g, x))),
    'F1_conv2dbnrelu_k31': (lambda A: A.Conv2dBnRelu(3, 8, kernel_size=(3, 1)), lambda m: (lambda g, x: m.emit(g, x))),
    'F1_conv2dbnrelu_k13': (lambda A: A.Conv2dBnRelu(3, 8, kernel_size=(1, 3)), lambda m: (lambda g, x: m.emit(g, x))),
    'F2_convbnrelu': (lambda A: A.ConvBnRelu(3, 8), lambda m: (lambda g, x: m.emit(g, x))),
    'F3_decoderv1': (lambda A: A.DecoderBlockV1(6, 8, 4), lambda m: (lambda g, x: m.emit(g, x))),
    'F3_decoderv2_deconv': (lambda A: A.DecoderBlockV2(6, 8, 4, is_deconv=True), lambda m: (lambda g, x: m.emit(g, x))),
    'F3_decoderv2_upsample': (lambda A: A.DecoderBlockV2(6, 8, 4, is_deconv=False), lambda m: (lambda g, x: m.emit(g, x))),
    'F3_deconvconv2dbnrelu': (lambda A: A.DeconvConv2dBnRelu(6, 4), lambda m: (lambda g, x: m.emit(g, x))),
    'F4_decoderblock_skip': (lambda A: A.DecoderBlock(13, 16, 32), lambda m: (lambda g, x, e: m.emit(g, x, e))),
    'F4_decoderblock_noskip': (lambda A: A.DecoderBlock(8, 16, 32), lambda m: (lambda g, x: m.emit(g, x))),
}
