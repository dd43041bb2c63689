"""Engine: owns the flat parameter/gradient/optimizer buffers of one model, the packed compute copies of
its convolution weights, the BatchNorm work vectors, and the compiled (static) programs per batch shape.

Design notes (MI355X-first):
  * fp32 master parameters live in ONE flat buffer in the reference's own tensor layouts, so
    ``state_dict()`` is the reference's; gradients live in a second flat buffer of the same layout, so
    the optimizer is one fused kernel over 30 M floats and data-parallel all-reduce works on contiguous
    byte ranges (buckets) without gather/scatter copies.
  * convolution kernels read PACKED copies ([chunk][tap][n][64 B], bf16 or f32; plus the transposed copy
    the data-gradient needs) that a tiny pack program refreshes after every optimizer step.
  * a training step = pack -> forward -> loss -> backward (in bucket segments, all-reduce on a side
    stream) -> fused Adam; each is one call into the native executor.
"""
import ctypes

import torch

from . import _abi
from ._abi import SaltError, lib
from .engine import Graph, Program, StepInput, set_path, DT_CODE, TORCH_DT
from .losses import LOVASZ_DEFAULTS, dice_ce_params, lovasz_launch_shape, lovasz_params


def _require_gpu(device):
    if device.type != 'cuda':
        raise SaltError('the HIP path needs a GPU tensor/device (got %s); there is no CPU fallback' % device)


class CompiledNet:
    """One static instance: input/target/logits buffers + forward/backward programs for fixed (B,C,H,W)."""

    def __init__(self, engine, shape, train, num_classes):
        B, C, H, W = shape
        self.engine, self.shape, self.train = engine, shape, train
        g = Graph(engine, train)
        self.g = g
        self.x = g.alloc((B, C, H, W), torch.float32)
        oshape = engine.module.output_shape(shape) if hasattr(engine.module, 'output_shape') else (B, num_classes, H, W)
        self.logits = g.alloc(tuple(oshape), torch.float32)
        # second network input of a depth-conditioned network: the tiles' depths [B,1], static like x
        self.d = g.alloc((B, 1), torch.float32) if getattr(engine.module, 'uses_depth', False) else None
        g.step_inputs = {k: t for k, t in (('x', self.x), ('d', self.d)) if t is not None}
        engine.module.emit(g, self.x, self.logits)
        self.dlogits = g.dlogits
        self.target = self.loss = None   # static target / loss scalar of a training instance: written below, read by bind() and the loss programs
        if train:
            self.target = g.alloc(tuple(oshape), torch.float32)
            self.loss = g.alloc((1,), torch.float32)
            self.loss_per_image = g.alloc((B,), torch.float32)
            g.build_backward()
        g.finalize()
        self.fwd, self.bwd = g.fwd, g.bwd
        self._loss_progs = {}
        self._step_graphs = {}         # loss key -> (optimizer, hipGraph executable, pack generation): Engine.step_graph writes, release_step_graphs clears
        for which, name, needed in (('x', 'batch', train), ('d', 'depth', self.d is not None)):
            if needed and not self.slots(which):
                raise SaltError('no operator of this instance reads the %s input' % name)

    # ------------------------------------------------------------------ zero-copy step inputs (round 6)
    def slots(self, which):
        """(struct, path, byte offset) of the pointer fields of this instance's programs that read the static input / target buffer or
        write the loss scalar, as their emitters recorded them (engine.StepInput -> Program.slots).  The executor reads an argument
        struct when it ENQUEUES the launch, so re-pointing such a field between two runs of a program is a host-side store and nothing
        else: the fused step (models.SegmentationModel._fused_step) points them at the caller's resident batch / target for its enqueue
        calls instead of copying 6 MB + 4 MB into the static buffers first, and puts them back (hipGraph captures bake pointers in)."""
        return [s for prog in [self.fwd, self.bwd] + list(self._loss_progs.values()) for s in prog.slots.get(which, ())]

    def bind(self, **tensors):
        """bind(x=t, d=t1, target=t2, loss=t3): point the programs at these device tensors.  ``key=None`` points that key back at its static
        buffer, a key that is not given is left as it is, and a bare ``bind()`` resets all of them.  A loss program built later starts on
        the static addresses.  The caller keeps the tensors alive until the step's launches are enqueued on the stream it later frees /
        overwrites them on."""
        static = dict(x=self.x, d=self.d, target=self.target, loss=self.loss)
        for which, t in (tensors or dict.fromkeys(static)).items():
            if which not in static:
                raise SaltError('bind(): unknown key %r' % which)
            buf = static[which]
            if buf is None:
                continue
            if t is not None and not self.bindable(t, buf):
                raise SaltError('bind(%s): needs a contiguous %s tensor of shape %s on %s' % (which, buf.dtype, tuple(buf.shape), buf.device))
            ptr = (buf if t is None else t).data_ptr()
            for st, path, off in self.slots(which):
                set_path(st, path, ptr + off)

    @staticmethod
    def bindable(t, buf):
        return (t.dtype == buf.dtype and tuple(t.shape) == tuple(buf.shape) and t.is_contiguous() and t.device == buf.device
                and t.data_ptr() % 16 == 0)

    def loss_key(self, kind, loss_scale):
        """Cache key of a loss program (and of a captured step that contains it): the kind, the scale, and for 'dice_ce' the weights /
        for 'lovasz' and 'lovasz_softmax' the options the engine holds (Engine.loss_params, from model_params['loss_params'])."""
        if kind == 'dice_ce':
            return (kind, float(loss_scale)) + dice_ce_params(self.engine.loss_params)
        if kind in LOVASZ_DEFAULTS:
            return (kind, float(loss_scale)) + lovasz_params(kind, self.engine.loss_params)
        return (kind, float(loss_scale))

    def loss_program(self, kind, loss_scale):
        key = self.loss_key(kind, loss_scale)
        if key in self._loss_progs:
            return self._loss_progs[key]
        g = self.g
        B, K, H, W = self.logits.shape
        p = Program('loss:' + kind)
        if kind == 'lovasz':
            P = K * H * W
            wk = g.alloc((2, B, P), torch.int32, zero=False)
            wv = g.alloc((2, B, P), torch.int32, zero=False)
            flags, ignore, rows, n = lovasz_launch_shape(kind, self.engine.loss_params, B, K, H * W)
            sw = int(lib.salt_lovasz_split_words(n)) if n < 2 ** 31 else 0    # > 0: several workgroups per row (segments of the sort)
            ws = g.alloc((rows * sw,), torch.int32, zero=False) if sw else None
            fw = int(lib.salt_lovasz_flat_words(n))              # > 0: a long row (batch-flat, or an image above 131072 elements)
            wf = g.alloc((rows * fw,), torch.int32, zero=False) if fw else None
            p.add('lovasz_hinge', logits=self.logits.data_ptr(), target=StepInput('target', self.target.data_ptr()), B=B, P=P, ws_keys=wk.data_ptr(),
                  ws_vals=wv.data_ptr(), loss_per_image=self.loss_per_image.data_ptr(), loss=StepInput('loss', self.loss.data_ptr()),
                  dlogits=self.dlogits.data_ptr(), loss_scale=loss_scale, ws_split=ws.data_ptr() if ws is not None else None,
                  flags=flags, ignore=ignore, ws_flat=wf.data_ptr() if wf is not None else None)
        elif kind == 'bce_dice':
            S = _abi.STRUCTS['salt_bce_dice_args']()
            _abi.fill(S, B=B, C=K, HW=H * W)
            nparts = lib.salt_bce_dice_parts(ctypes.byref(S))
            parts = g.alloc((nparts * 4,), torch.float32)
            sums = g.alloc((3 * K + 1,), torch.float32)
            p.add('bce_dice', logits=self.logits.data_ptr(), target=StepInput('target', self.target.data_ptr()), B=B, C=K, HW=H * W, dice_weight=0.2, bce_weight=0.9,
                  partials=parts.data_ptr(), nparts=nparts, sums=sums.data_ptr(), loss=StepInput('loss', self.loss.data_ptr()), dlogits=self.dlogits.data_ptr(),
                  loss_scale=loss_scale)
        elif kind == 'lovasz_softmax':
            # softmax -> rows (b, c) of H*W probabilities through the hinge's sort with the absolute-error policy, d loss / d probas
            # into dlogits -> softmax Jacobian in place
            HW = H * W
            probas = g.alloc((B, K, HW), torch.float32, zero=False)
            wk = g.alloc((2, B * K, HW), torch.int32, zero=False)
            wv = g.alloc((2, B * K, HW), torch.int32, zero=False)
            rows = g.alloc((B * K,), torch.float32)
            flags, ignore, nrows, n = lovasz_launch_shape(kind, self.engine.loss_params, B, K, HW)
            sw = int(lib.salt_lovasz_split_words(n)) if n < 2 ** 31 else 0
            ws = g.alloc((nrows * sw,), torch.int32, zero=False) if sw else None
            fw = int(lib.salt_lovasz_flat_words(n))
            wf = g.alloc((nrows * fw,), torch.int32, zero=False) if fw else None
            wp = g.alloc((B * K,), torch.int32, zero=False) if flags & _abi.CONSTS['SALT_LOVASZ_ONLY_PRESENT'] else None
            p.add('softmax', x=self.logits.data_ptr(), y=probas.data_ptr(), B=B, C=K, HW=HW)
            p.add('lovasz_softmax', probas=probas.data_ptr(), target=StepInput('target', self.target.data_ptr()), B=B, C=K, HW=HW, ws_keys=wk.data_ptr(),
                  ws_vals=wv.data_ptr(), loss_per_row=rows.data_ptr(), loss=StepInput('loss', self.loss.data_ptr()), dprobas=self.dlogits.data_ptr(),
                  loss_scale=loss_scale, ws_split=ws.data_ptr() if ws is not None else None, flags=flags, ignore=ignore,
                  ws_flat=wf.data_ptr() if wf is not None else None, ws_present=wp.data_ptr() if wp is not None else None)
            p.add('softmax_bwd', p=probas.data_ptr(), dp=self.dlogits.data_ptr(), dz=self.dlogits.data_ptr(), B=B, C=K, HW=HW)
        elif kind == 'dice_ce':
            dw, cw, smooth = key[2:]
            S = _abi.STRUCTS['salt_dice_ce_args']()
            _abi.fill(S, B=B, C=K, HW=H * W)
            nparts = lib.salt_dice_ce_parts(ctypes.byref(S))
            if nparts < 1:
                raise SaltError('dice_ce: %d output channels (the softmax losses take 2 .. 4)' % K)
            parts = g.alloc((nparts * (3 * K + 1),), torch.float32)
            sums = g.alloc((3 * K + 1,), torch.float32)
            p.add('dice_ce', logits=self.logits.data_ptr(), target=StepInput('target', self.target.data_ptr()), B=B, C=K, HW=H * W, dice_weight=dw,
                  cross_entropy_weight=cw, smooth=smooth, partials=parts.data_ptr(), nparts=nparts, sums=sums.data_ptr(),
                  loss=StepInput('loss', self.loss.data_ptr()), dlogits=self.dlogits.data_ptr(), loss_scale=loss_scale)
        else:
            raise SaltError('unknown native loss %r' % kind)
        p.finalize()
        if not (p.slots.get('target') and p.slots.get('loss')):
            raise SaltError('loss program %r does not read the target or does not write the loss scalar through a recorded slot' % kind)
        self._loss_progs[key] = p
        return p


class WeightPacks:
    """The packed compute copies of an engine's convolution weights ([chunk][tap][n][64 B], bf16 or f32; plus the transposed copies the
    data gradients read), the jobs that write them and the one rule for when they are stale.  Jobs are registered while the networks
    are emitted (``dense`` / ``tapgemm`` / ``phases`` / ``stem``, all through ``_register``); two batched launches run them in
    registration order: the copies the forward pass reads on the caller's stream, the backward-only copies on the side stream.
    ``refresh`` brings them up to a weight version; the step graph and FusedAdam use the members at the end."""

    def __init__(self, engine):
        self.engine = engine
        self.tensors = {}               # pack key -> packed tensor
        self._ops = Program('pack')     # the salt_pack_conv_weight jobs, registration order (never run itself: _build batches them)
        self._keys, self._is_bwd = [], {}       # their keys in _ops order; True = only backward reads it
        self._misc = Program('pack_misc')       # pack launches of other kinds (the stem's): run behind the forward batch
        self._built = False             # the batched programs below cover every job of _ops: _register clears, _build sets
        self._fwd = self._rest = self._bwd = None    # batched programs (all forward jobs / those Adam does not write / backward-only jobs)
        self._tables = []               # the device tables the batched programs point into
        self._adam_jobs = []            # forward jobs FusedAdam can write while it updates the weights: _build writes
        self._version = self._bwd_version = -1       # weight version the forward / the backward-only copies hold
        self._adam_version = None       # weight version whose forward packs FusedAdam wrote itself: note_adam_packed writes, refresh reads
        self.generation = 0             # bumped by _build; step_graph() recaptures an executable of an older generation
        self._fork = None               # the backward batch again, tagged for the side stream (the executor forks with an event): _build writes

    def _register(self, key, sub, bwd, t=None, op='pack_conv_weight', **job):
        """Pack job ``key + sub`` (``job``: its fields; none: the job exists and only changes to ``bwd``) into tensor ``t`` = tensors[key].
        THE place that says what a new or changed job makes stale: both packed versions, and the batched programs."""
        if job:
            batched = op == 'pack_conv_weight'
            (self._ops if batched else self._misc).add(op, dtype=DT_CODE[self.engine.dtype], **job)
            self._keys += [key + sub] if batched else []
            self.tensors[key] = t
        self._is_bwd[key + sub] = bool(bwd)
        self._version = self._bwd_version = -1
        self._built = False

    def _zeros(self, elems):
        return torch.zeros(elems, dtype=TORCH_DT[self.engine.dtype], device=self.engine.device)

    def dense(self, conv, taps_khkw, transposed, bwd=False, d1=None):
        """Packed copy of a convolution weight.  ``bwd``: only the backward program reads it (data-gradient packs): such copies are
        refreshed on the side stream while the forward pass runs.  ``d1`` = (first, count): only that slice of the weight's SECOND axis
        (the input channels of an nn.Conv2d) - the full-resolution part of the factored hypercolumn convolution (Graph.conv_hyper)."""
        key = (id(conv), tuple(taps_khkw), bool(transposed)) + ((tuple(d1),) if d1 else ())
        if key in self.tensors:
            if not bwd and self._is_bwd[key]:
                self._register(key, (), False)           # a forward reader of what was a backward-only copy
            return self.tensors[key]
        D0, D1, KH, KW = conv.weight.shape
        c1 = d1[1] if d1 else D1
        n, c = (c1, D0) if transposed else (D0, c1)
        t = self._zeros(lib.salt_packed_weight_elems(DT_CODE[self.engine.dtype], len(taps_khkw), n, c))
        self._register(key, (), bwd, t, w=conv.weight.data_ptr() + (4 * d1[0] * KH * KW if d1 else 0), D0=D0, D1=D1, KH=KH, KW=KW,
                       ntaps=len(taps_khkw), tap_kh=[a for a, _ in taps_khkw], tap_kw=[b for _, b in taps_khkw], transpose=int(transposed),
                       wp=t.data_ptr(), d1_cnt=(d1[1] if d1 else 0))
        return t

    def tapgemm(self, conv, c0, cn, transposed, bwd=False):
        """The KH x KW tap matrices W[:, c0 : c0 + cn, kh, kw] of a convolution weight as ONE packed 1x1 weight: forward
        (transposed=False) cn -> KH KW Cout output channels, channel t Cout + o = tap t of output channel o; transposed: the 1x1 data
        gradient KH KW Cout -> cn.  One pack job per tap into the shared tensor (salt_pack_conv_weight_args.n_off / chunk_off).  The
        low-resolution half of the factored hypercolumn convolution (Graph.hyper_level, saltnet.h salt_hyper_stencil)."""
        key = (id(conv), 'tapgemm', c0, cn, bool(transposed))
        if key in self.tensors:
            return self.tensors[key]
        D0, D1, KH, KW = conv.weight.shape
        nt = KH * KW
        kce = 16 if self.engine.dtype == 'f32' else 32
        if transposed and D0 % kce:
            raise SaltError('tap GEMM: %d output channels are not a multiple of the %d-channel pack chunk' % (D0, kce))
        n, c = (cn, nt * D0) if transposed else (nt * D0, cn)
        t = self._zeros(lib.salt_packed_weight_elems(DT_CODE[self.engine.dtype], 1, n, c))
        for tap in range(nt):
            self._register(key, (tap,), bwd, t, w=conv.weight.data_ptr() + 4 * c0 * KH * KW, D0=D0, D1=D1, KH=KH, KW=KW, ntaps=1,
                           tap_kh=[tap // KW], tap_kw=[tap % KW], transpose=int(transposed), wp=t.data_ptr(), d1_cnt=cn,
                           n_off=0 if transposed else tap * D0, n_total=n, chunk_off=(tap * D0 // kce) if transposed else 0)
        return t

    def phases(self, conv, phase_taps, transposed, bwd=False):
        """Packed weights of a phase-fused stride-2 launch: one block of len(phase_taps[0]) taps per output-parity phase, contiguous;
        ``phase_taps[p][t]`` is (kh, kw) or None (a tap that phase does not have: packed as zeros).  -> (tensor, elements per phase)"""
        key = (id(conv), tuple(tuple(t) for t in phase_taps), bool(transposed), 'phases')
        D0, D1, KH, KW = conv.weight.shape
        n, c = (D1, D0) if transposed else (D0, D1)
        nt = len(phase_taps[0])
        elems = lib.salt_packed_weight_elems(DT_CODE[self.engine.dtype], nt, n, c)
        if key in self.tensors:
            return self.tensors[key], elems
        t = self._zeros(elems * len(phase_taps))
        for ph, taps in enumerate(phase_taps):
            self._register(key, (ph,), bwd, t, w=conv.weight.data_ptr(), D0=D0, D1=D1, KH=KH, KW=KW, ntaps=nt,
                           tap_kh=[(tp[0] if tp is not None else -1) for tp in taps], tap_kw=[(tp[1] if tp is not None else 0) for tp in taps],
                           transpose=int(transposed), wp=t.data_ptr() + ph * elems * t.element_size())
        return t, elems

    def stem(self, conv):
        key = (id(conv), 'stem')
        if key in self.tensors:
            return self.tensors[key]
        Cout, Cin, K, _ = conv.weight.shape
        TT = (K + 1) // 2
        t = self._zeros(lib.salt_packed_weight_elems(DT_CODE[self.engine.dtype], TT * TT, Cout, 16))
        self._register(key, (), False, t, op='pack_stem_weight', w=conv.weight.data_ptr(), Cout=Cout, Cin=Cin, K=K, wp=t.data_ptr())
        return t

    def _build(self):
        """Two launches pack every convolution weight (per-job argument structs live in device tables): the copies the forward
        pass reads on the main stream, the data-gradient copies on the side stream (they are not needed before backward)."""
        import numpy as np
        eng = self.engine
        jobs = [s for _, _, s in self._ops.ops]
        assert len(jobs) == len(self._keys)
        self._tables = []

        def batch(sel, name, misc=False):
            prog = Program(name)
            if sel:
                raw = b''.join(bytes(s) for s in sel)
                blocks = [lib.salt_pack_job_blocks(ctypes.byref(s)) for s in sel]
                pref = np.concatenate([[0], np.cumsum(blocks)]).astype(np.int32)
                table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(eng.device)
                pref_t = torch.from_numpy(pref).to(eng.device)
                self._tables += [table, pref_t]
                prog.add('pack_batched', jobs=table.data_ptr(), job_block0=pref_t.data_ptr(), njobs=len(sel), total_blocks=int(pref[-1]),
                         dtype=DT_CODE[eng.dtype])
            if misc:
                prog.extend(self._misc)
            return prog.finalize()
        fwd_jobs = [s for s, k in zip(jobs, self._keys) if not self._is_bwd[k]]
        self._fwd = batch(fwd_jobs, 'pack', misc=True)
        # the forward packs FusedAdam writes itself while it updates the weights (salt_adam_pack): vector-path jobs, one per weight, whose
        # master lives in the flat buffer; `_rest` = what a refresh right behind such an optimizer step still has to run
        lo, hi = eng.flat.data_ptr(), eng.flat.data_ptr() + 4 * eng.n_live
        seen, self._adam_jobs = set(), []
        for s in fwd_jobs:
            if lib.salt_pack_job_is_vec(ctypes.byref(s)) and lo <= s.w < hi and s.w not in seen:
                seen.add(s.w)
                self._adam_jobs.append(s)
        ids = {id(s) for s in self._adam_jobs}
        self._rest = batch([s for s in fwd_jobs if id(s) not in ids], 'pack_rest', misc=True)
        self._adam_version = None                        # (new / moved pack tensors: the next refresh runs every job)
        self._bwd = batch([s for s, k in zip(jobs, self._keys) if self._is_bwd[k]], 'pack_bwd')
        self._fork = Program('pack_fork')
        self._fork.ops, self._fork.streams = self._bwd.ops, [1] * len(self._bwd)
        self._built = True
        # a captured step graph bakes the device pointers of THESE tables in: every rebuild starts a new generation, and step_graph()
        # recaptures an executable of an older one instead of replaying it against freed tables
        self.generation += 1

    def ensure_built(self):
        """Rebuild the batched programs if jobs were registered since they were built."""
        if not self._built:
            self._build()

    def refresh(self, train, wver, side_stream):
        """Bring the packed copies up to weight version ``wver``: the forward copies on the current stream, and for a training step the
        backward-only copies on ``side_stream``."""
        self.ensure_built()
        if self._version != wver:
            # the optimizer step that produced this weight version wrote the vector-path forward packs itself (FusedAdam -> salt_adam_pack)
            (self._rest if self._adam_version == wver else self._fwd).run()
            self._version = wver
        if train and self._bwd_version != wver and len(self._bwd):
            # ordered after the optimizer step on the main stream; the backward program's first data-gradient joins (engine.py)
            side_stream.wait_stream(torch.cuda.current_stream())
            self._bwd.run(stream=side_stream)
            self._bwd_version = wver

    # ------------------------------------------------------------------ for the step graph (Engine.step_graph) and the tests
    def programs(self):
        """-> (forward batch, backward-only batch, the latter as the one-entry fork program), rebuilt if jobs were added"""
        self.ensure_built()
        return self._fwd, self._bwd, self._fork

    def note_packed(self, wver):
        """A replayed step graph packed every copy from the weights of version ``wver``."""
        self._version = self._bwd_version = wver

    # ------------------------------------------------------------------ for FusedAdam (with ensure_built)
    def adam_jobs(self):
        """-> (generation, the forward jobs an optimizer step can write itself: vector path, one per weight of the flat buffer)"""
        return self.generation, self._adam_jobs

    def note_adam_packed(self, wver):
        """The optimizer step that produced weight version ``wver`` wrote the jobs of ``adam_jobs`` itself: refresh runs only the rest."""
        self._adam_version = wver


class Engine:
    def __init__(self, module, device, dtype='f32'):
        _require_gpu(device)
        if dtype not in DT_CODE:
            raise SaltError('dtype must be f32 or bf16')
        self.module, self.device, self.dtype = module, device, dtype
        self._flatten()
        self.packs = WeightPacks(self)  # packed compute copies of the convolution weights
        self._bn = {}
        self._fold_ops = Program('bn_fold')
        self.nets = {}
        self.wver = 0                   # bumped whenever master weights change
        self.sver = 0                   # bumped whenever BN running statistics change
        self._folded_version = None
        self.world = 1
        self.side_stream = torch.cuda.Stream(device=device)     # weight-gradient kernels overlap the data-gradient chain
        self._graph_stream = None       # capture / replay stream of the step graphs: step_graph creates it, run_step_graph reads
        self.eager_done = set()          # (shape, loss kind) whose first training step already ran eagerly (models.SegmentationModel._fused_step)
        self.loss_params = None          # weights of the 'dice_ce' / options of the Lovasz loss programs (model_params['loss_params']): SegmentationModel._fused_step writes, CompiledNet.loss_key reads

    # ------------------------------------------------------------------ flat parameter storage
    def _flatten(self):
        m = self.module
        dead = set(m.dead_parameter_names()) if hasattr(m, 'dead_parameter_names') else set()
        seen = {}
        live = []
        for name, p in m.named_parameters():
            if id(p) in seen:
                continue
            seen[id(p)] = name
            if p.requires_grad and name not in dead:
                live.append((name, p))
        total = sum(((p.numel() + 3) // 4) * 4 for _, p in live)
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._off = {}
        self.live_names = []
        off = 0
        for name, p in live:
            n = p.numel()
            view = self.flat[off:off + n].view(p.shape)
            view.copy_(p.data.to(self.device, torch.float32))
            p.data = view
            p.grad = self.grads[off:off + n].view(p.shape)
            self._off[id(p)] = (off, n)
            self.live_names.append(name)
            off += ((n + 3) // 4) * 4
        self.n_live = total
        self.live_params = [p for _, p in live]
        for name, p in m.named_parameters():              # dead parameters just move to the device
            if id(p) not in self._off and p.device != self.device:
                p.data = p.data.to(self.device)
        for name, b in m.named_buffers():
            if b.device != self.device:
                b.data = b.data.to(self.device)

    def grad_ptr(self, param):
        off, _ = self._off[id(param)]
        return self.grads.data_ptr() + 4 * off

    def grad_range(self, param):
        return self._off[id(param)]

    def bn_work(self, bn):
        if id(bn) in self._bn:
            return self._bn[id(bn)]
        C = bn.num_features
        w = {k: torch.zeros(C, dtype=torch.float32, device=self.device) for k in ('mean', 'invstd', 'scale', 'shift')}
        self._fold_ops.add('bn_fold', C=C, gamma=bn.weight.data_ptr(), beta=bn.bias.data_ptr(), running_mean=bn.running_mean.data_ptr(),
                           running_var=bn.running_var.data_ptr(), eps=bn.eps, scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr())
        self._fold_ops._entries = None
        self._bn[id(bn)] = w
        self._folded_version = None
        return w

    def touch(self, weights=True, stats=True):
        """Master weights / BN statistics changed: packed copies / folded BN are stale."""
        if weights:
            self.wver += 1
        if stats:
            self.sver += 1

    def refresh(self, train):
        """Bring the packed weight copies (and, in eval mode, the folded BN constants) up to date."""
        self.packs.refresh(train, self.wver, self.side_stream)
        if not train and self._folded_version != (self.wver, self.sver):
            self._fold_ops.run()
            self._folded_version = (self.wver, self.sver)

    # ------------------------------------------------------------------ compiled instances
    def net(self, shape, train):
        key = (tuple(shape), bool(train))
        if key not in self.nets:
            self.nets[key] = CompiledNet(self, tuple(shape), train, self.module.num_classes)
        return self.nets[key]

    # ------------------------------------------------------------------ one training step as ONE hipGraph
    def step_graph(self, net, kind, loss_scale, optimizer):
        """Capture pack -> forward (two streams) -> data-gradient packs -> loss -> backward (two streams) -> Adam of one compiled
        instance into a hipGraph (cached); replaying it is one launch instead of ~490.  Everything the step touches is static
        device memory; the learning rate / bias corrections live in the optimizer's device `hyper` vector (adam_tick)."""
        # the cache lives ON the compiled instance (which this engine owns) and holds the optimizer object itself: a rebuilt engine /
        # net / optimizer can never alias a stale executable through a recycled id()
        cache = net._step_graphs
        key = net.loss_key(kind, loss_scale)
        pack_fwd, pack_bwd, pack_fork = self.packs.programs()
        hit = cache.get(key)
        if hit is not None and hit[0] is optimizer and hit[2] == self.packs.generation:
            return hit[1]
        if hit is not None:
            lib.salt_graph_destroy(hit[1])
        optimizer._bind()
        optimizer._sync_hyper()
        loss_prog = net.loss_program(kind, loss_scale)
        st = self._graph_stream = self._graph_stream or torch.cuda.Stream(device=self.device)
        torch.cuda.synchronize()
        exec_ = ctypes.c_void_p()
        with torch.cuda.stream(st):
            _abi.check(lib.salt_graph_begin(ctypes.c_void_p(st.cuda_stream)), 'graph_begin')
            try:
                pack_fwd.run(stream=st)
                net.fwd.run(stream=st, side=self.side_stream)
                if len(pack_bwd):
                    # fork: the data-gradient packs run on the side stream under the loss kernel; backward's first operator joins
                    pack_fork.run(stream=st, side=self.side_stream, join=False)
                loss_prog.run(stream=st)
                net.bwd.run(stream=st, side=self.side_stream)
                optimizer.prog.run(stream=st)
            finally:
                rc = lib.salt_graph_end(ctypes.c_void_p(st.cuda_stream), ctypes.byref(exec_))
            _abi.check(rc, 'graph_end')
        torch.cuda.synchronize()
        cache[key] = (optimizer, exec_, self.packs.generation)
        return exec_

    def release_step_graphs(self):
        """Destroy the captured step executables of every compiled instance (called when the engine is dropped)."""
        for net in self.nets.values():
            for _, ex, *_gen in net._step_graphs.values():
                lib.salt_graph_destroy(ex)
            net._step_graphs = {}

    def run_step_graph(self, net, kind, loss_scale, optimizer):
        exec_ = self.step_graph(net, kind, loss_scale, optimizer)
        optimizer._sync_hyper()
        cur = torch.cuda.current_stream()
        st = self._graph_stream
        st.wait_stream(cur)                                  # the input / target copies of this step
        _abi.check(lib.salt_graph_launch(exec_, ctypes.c_void_p(st.cuda_stream)), 'graph_launch')
        cur.wait_stream(st)
        optimizer.steps += 1
        self.packs.note_packed(self.wver)                                # the graph packed the weights it started from ...
        self.touch(weights=True, stats=True)                             # ... and Adam / BatchNorm moved them

    def forward(self, x, train, bound=False, d=None, d_bound=False):
        """``bound``: the caller pointed the programs at ``x`` itself (CompiledNet.bind) - no copy into the static input buffer.
        ``d``: the depth input [B,1] of a depth-conditioned network (``d_bound``: likewise bound by the caller)."""
        _require_gpu(x.device)
        net = self.net(x.shape, train)
        if (net.d is None) != (d is None):
            raise SaltError('%s: depth input %s' % (type(self.module).__name__, 'missing' if d is None else 'given to a network without one'))
        if not bound:
            net.bind(x=None)
            net.x.copy_(x)
        if d is not None and not d_bound:
            if tuple(d.shape) != tuple(net.d.shape):
                raise SaltError('depth input must be [%d, 1]' % net.d.shape[0])
            net.bind(d=None)
            net.d.copy_(d)
        self.refresh(train)
        net.fwd.run(side=self.side_stream)
        if train:
            self.touch(weights=False, stats=True)            # BN running statistics moved
        return net
