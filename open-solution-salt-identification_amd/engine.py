"""Static-program engine: builds the forward and backward operator lists of a network ONCE per
(batch shape, mode) and runs each as a single call into libsaltnet_hip.so.

The reference executes its U-Nets through PyTorch autograd, one operator at a time from Python
(common_blocks/models.py:105-136).  Here the module tree (architectures.py) "emits" its operators into
a :class:`Graph`; every emitter also pushes a closure that later emits the matching backward operators,
so the backward program is derived mechanically in reverse order with static gradient-accumulation
flags.  Activations are NHWC buffers that live for the lifetime of the graph (288 GB of HBM makes
re-materialisation pointless); skip connections and the hypercolumn are channel SLICES of wider
buffers that their producers write in place, so ``torch.cat`` never copies anything.

PyTorch is used for device memory (tensors), streams and nothing else on this path.
"""
import contextlib
import ctypes
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Any

import numpy as np
import torch

from . import switches
from ._abi import OP_FUNCS, STRUCTS, SaltError, check, fill, lib

DT_CODE = {'f32': 0, 'bf16': 1}
TORCH_DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
VEC = {'f32': 4, 'bf16': 8}

# ---------------------------------------------------------------------- the builder's peephole protocol
# salt_bn_bwd_args.partials_ready, in saltnet.h's words:
PARTIALS_OWN = 0         # bn_bwd's own reduction pass; "partials_ready == 0 and fin_acc != NULL: the reduction pass accumulates into [8][2][C] fp64 shards"
PARTIALS_FILLED = 1      # "`partials` ([nparts][2][C], any nparts >= 1) was filled by the producer of da (salt_conv_args.bnb_*)"
PARTIALS_FINALIZED = 2   # "the producer also finalized (salt_conv_args.bnb_fin): coef / dgamma / dbeta are ready, only the apply pass runs"
PARTIALS_SHARDS = 3      # "the producer added the sums to fin_acc (salt_conv_args.bnb_acc without ticket): the apply pass finalizes them"

# Who supplies a layer's BatchNorm-backward sums (Graph._bnb_sums_source); the middle two are also the kinds of carrier a gradient writer offers
SUMS_OWN = 'own'         # the reduction pass of the layer's own salt_bn_bwd
SUMS_CONV = 'conv'       # the data-gradient launch that writes dL/da last (salt_conv_args.bnb_*)
SUMS_SEC = 'sec'         # the main branch's salt_bn_bwd, whose dres IS this layer's dL/da (salt_bn_bwd_args.sec_*)
SUMS_SCSE = 'scse'       # the scSE backward behind the layer (salt_scse_bwd_args.bnb_acc)


@dataclass
class GradWriter:
    """One writer of channels [c0, c0 + C) of a Buffer's gradient (Act.grad_state, backward-program order).  ``carrier``: its argument struct
    if it can also take the BatchNorm-backward sums of the slice's producer - a salt_conv_args (``kind`` SUMS_CONV) or a salt_bn_bwd_args
    (SUMS_SEC); set by Act.offer_carrier, claimed by Graph._bnb_sums_source."""
    c0: int
    C: int
    kind: Any = None
    carrier: Any = None


# Buffer.grad_bias: the scSE backward left the channel-SE term ``dgap`` [B][C] out of dL/dx; the bn_bwd of x's producer adds it (da_bias).  ``sums_from``:
# the salt_scse_bwd_args that also took that layer's BatchNorm-backward sums; ``fc_grads``: the deferred salt_scse_fc_grads struct, or None
GradBias = namedtuple('GradBias', 'c0 C dgap sums_from fc_grads', defaults=(None, None))
# Buffer.act_op: the salt_affine_act ``struct`` that stores channels [c0, c0 + C), and Buffer.reads right after it (Graph._take_act_op)
ActOp = namedtuple('ActOp', 'struct reads0 c0 C')
# Graph.depth_gate -> channel_gate: gate values ``s`` [B][C], dL/ds ``ds`` (None: through the fp64 arena), the backward channel_gate structs ``users`` that
# add to it, and the gate channels some channel_gate has ``covered``
DepthGate = namedtuple('DepthGate', 's B C ds users covered')


@dataclass
class Lazy:
    """Buffer.lazy (SALT_FWD_BN_FOLD candidate): raw convolution output ``y``, the layer's salt_bn_finalize_args ``F``, its affine_act ``sa``, byte
    offset ``off`` of its statistics shards, Buffer.reads right after ``sa``, the convolution structs that read y through their loader."""
    y: Any
    F: Any
    sa: Any
    off: int
    reads0: int
    users: list = field(default_factory=list)
    dropped: bool = False          # Graph._resolve_lazies removed ``sa``


def fwd_bn_fold():
    """SALT_FWD_BN_FOLD=1 (measurement / verification switch, DESIGN history round 3): the BatchNorm apply + ReLU of a conv -> BN -> ReLU output whose
    only reader is ONE 3x3 convolution runs in that convolution's loader (salt_conv_args.in_*; forward values bit-identical, tested).
    The weight-gradient kernels cannot re-derive the activation, so such a graph is FORWARD-ONLY: its backward closure raises instead
    of computing a wrong gradient."""
    return switches.get('SALT_FWD_BN_FOLD')


def _round_up(v, m):
    return (v + m - 1) // m * m


class Scratch:
    """Named shared workspace request; resolved to one allocation (max size) when the graph is finalized."""

    def __init__(self, name, nbytes):
        self.name, self.nbytes = name, int(nbytes)


# The address of a step input (``key`` = 'x' | 'd' | 'target' | 'loss') plus a byte offset.  A field given one is filled with the static
# buffer's address ``ptr`` (+ offset) and recorded in Program.slots, which CompiledNet.bind re-points at the caller's tensor.
StepInput = namedtuple('StepInput', 'key ptr offset', defaults=(0,))


def set_path(struct, path, value):
    """struct.<path[0]>. ... .<path[-1]> = value (``path`` names the nested argument structs on the way, e.g. (field, 'p') of a view)"""
    for a in path[:-1]:
        struct = getattr(struct, a)
    setattr(struct, path[-1], value)


class Program:
    """A flat list of (operator, argument struct) pairs executed by salt_program_run."""

    def __init__(self, name=''):
        self.name = name
        self.ops = []          # (opname, fn, struct)
        self.default_stream = 0
        self.join_next = False
        self.streams = []      # 0 main / 1 side, per op
        self.patches = []      # (struct, path, Scratch)
        self.slots = {}        # step-input key -> [(struct, path, byte offset)]: set_fields writes, CompiledNet.bind re-points them
        self._entries = None
        self.marks = {}
        self._pre_run = None           # callable(stream, begin) run before the entries are issued (Graph.finalize: shard hygiene)
        self._post_run = None          # callable(begin, end) after they were issued
        self._graph = None             # captured hipGraph executable: capture() writes, replay() / release_graph() read

    def add(self, opname, stream=None, **fields):
        fn, S = OP_FUNCS['salt_' + opname]
        s = S()
        if stream is None:                       # default tag: the enclosing Graph.side() block, or a pending join
            stream = self.default_stream
            if stream == 0 and self.join_next:
                stream, self.join_next = 2, False
        self.streams.append(stream)
        self.set_fields(s, **fields)
        self.ops.append((opname, fn, s))
        return s

    def set_fields(self, s, /, **fields):
        """Set fields of an argument struct of this program.  A Scratch value is patched in at finalize, a StepInput value is the static
        address now and a recorded slot; either may come as (view, value) for the view's pointer ``p``."""
        for k, v in fields.items():
            path = (k,)
            if isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], (Scratch, StepInput)):
                fill(s, **{k: v[0]})
                v, path = v[1], (k, 'p')
            if isinstance(v, Scratch):
                self.patches.append((s, path, v))
            elif isinstance(v, StepInput):
                self.slots.setdefault(v.key, []).append((s, path, v.offset))
                set_path(s, path, v.ptr + v.offset)
            else:
                fill(s, **{k: v})

    def mark(self, label):
        self.marks[label] = len(self.ops)

    def extend(self, other):
        self.ops.extend(other.ops)
        self.streams.extend(other.streams)
        self.patches.extend(other.patches)
        for key, slots in other.slots.items():
            self.slots.setdefault(key, []).extend(slots)
        self._entries = None

    def finalize(self):
        n = len(self.ops)
        Entry = STRUCTS['salt_program_entry']
        arr = (Entry * max(n, 1))()
        for i, (_, fn, s) in enumerate(self.ops):
            arr[i].fn = ctypes.cast(fn, ctypes.c_void_p).value
            arr[i].args = ctypes.addressof(s)
            arr[i].stream = self.streams[i]
        self._entries = arr
        return self

    def __len__(self):
        return len(self.ops)

    def run(self, stream=None, begin=0, end=None, side=None, join=True, marks=None):
        """Enqueue ops [begin, end).  With ``side`` (a torch.cuda.Stream) ops tagged stream=1 run on it concurrently; ``join=False``
        leaves the side stream un-joined at the end of the range (the caller orders its consumers after both streams).
        ``marks`` = (positions int array, n, main-event array, side-event array) prepared by parallel.DataParallel: the executor records
        the two events of a mark before it issues the entry at that position (salt_program_run_streams_marks)."""
        if self._entries is None:
            self.finalize()
        end = len(self.ops) if end is None else end
        if self._pre_run is not None:
            self._pre_run(stream, begin)
        st = _stream_ptr(stream)
        if side is None and 3 in self.streams[begin:end]:
            raise SaltError('program %s joins the side stream (data-gradient weight packs): run it with side=engine.side_stream' % self.name)
        if side is not None and marks is not None:
            rc = lib.salt_program_run_streams_marks(ctypes.cast(self._entries, ctypes.c_void_p), begin, end, st, ctypes.c_void_p(side.cuda_stream),
                                                    1 if join else 0, marks[0], marks[1], marks[2], marks[3])
        elif side is not None:
            rc = lib.salt_program_run_streams_ex(ctypes.cast(self._entries, ctypes.c_void_p), begin, end, st, ctypes.c_void_p(side.cuda_stream),
                                                 1 if join else 0)
        else:
            rc = lib.salt_program_run_range(ctypes.cast(self._entries, ctypes.c_void_p), begin, end, st)
        if rc != 0:
            msg = lib.salt_last_error().decode(errors='replace')
            m = None
            try:
                m = int(msg.split('program entry')[1].split()[0])
            except Exception:
                pass
            where = (' [%s]' % self.ops[m][0]) if m is not None and m < len(self.ops) else ''
            raise SaltError('program %s failed (%d)%s: %s' % (self.name, rc, where, msg))
        if self._post_run is not None:
            self._post_run(begin, end)

    def capture(self, stream):
        """Capture the whole program (single stream, tags ignored) into a hipGraph on ``stream`` (not the default stream)."""
        if self._entries is None:
            self.finalize()
        self.release_graph()
        h = ctypes.c_void_p()
        check(lib.salt_graph_capture(ctypes.cast(self._entries, ctypes.c_void_p), len(self.ops), ctypes.c_void_p(stream.cuda_stream),
                                     ctypes.byref(h)), 'graph_capture')
        self._graph = h
        return self

    def replay(self, stream=None):
        if self._graph is None:
            raise SaltError('program %s has no captured graph' % self.name)
        check(lib.salt_graph_launch(self._graph, _stream_ptr(stream)), 'graph_launch')

    def release_graph(self):
        if self._graph is not None:
            lib.salt_graph_destroy(self._graph)
            self._graph = None

    def run_timed(self, stream=None):
        """Run with a HIP event pair around every entry (on the launch stream); returns [(opname, struct, ms)]."""
        if self._entries is None:
            self.finalize()
        n = len(self.ops)
        ms = (ctypes.c_float * max(n, 1))()
        if self._pre_run is not None:
            self._pre_run(stream, 0)
        check(lib.salt_program_run_timed(ctypes.cast(self._entries, ctypes.c_void_p), 0, n, _stream_ptr(stream), ms), 'run_timed')
        if self._post_run is not None:
            self._post_run(0, n)
        return [(self.ops[i][0], self.ops[i][2], float(ms[i])) for i in range(n)]

    def run_debug(self, stream=None):
        """Run op by op with a device sync after each (pinpoints a faulting kernel)."""
        if self._pre_run is not None:
            self._pre_run(stream, 0)
        st = _stream_ptr(stream)
        for i, (name, fn, s) in enumerate(self.ops):
            check(fn(ctypes.byref(s), st), '%s[%d] %s' % (self.name, i, name))
            torch.cuda.synchronize()
        if self._post_run is not None:
            self._post_run(0, len(self.ops))


def _stream_ptr(stream):
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


class Buffer:
    """NHWC storage [B,H,W,Ct] (+ lazily allocated gradient storage of the same geometry).  ``planes`` > 0: PLANAR storage
    [C / planes][B,H,W,planes] for both - every channel slice of `planes` channels is a dense tensor of its own, and a launch that takes
    the whole buffer names the plane stride (salt_conv_args.x_plane / y_plane, salt_conv_wgrad_args.q_plane)."""

    def __init__(self, graph, B, H, W, C, name='', planes=0):
        self.g, self.B, self.H, self.W, self.C = graph, B, H, W, C
        self.Ct = _round_up(C, graph.ve)
        self.name = name
        self.planes = planes
        if planes and (C % planes or planes % graph.ve):
            raise SaltError('planar buffer %s: %d channels in planes of %d' % (name, C, planes))
        self.t = graph.alloc(self._shape(), graph.tdtype)
        self.grad_t = None
        self.grad_init = np.zeros(self.Ct, dtype=bool)
        self.grad_writers = []         # GradWriter per gradient writer in backward-program order (Act.grad_state; read by Graph._bnb_sums_source)
        self.reads = 0                 # views handed out (SALT_FWD_BN_FOLD: an activation nobody else reads need not be materialised)
        self.act_op = None             # ActOp: Graph._bn_train_fwd writes, Graph._take_act_op (scse / head) reads and clears
        self.bn_train_out = None       # (c0, C) of the train-mode BatchNorm output stored here: _bn_train_fwd writes, scse / _bn_train_bwd read
        self.grad_bias = None          # GradBias: the backward of Graph.scse writes, Graph._bnb_sums_source / _bn_train_bwd read and clear
        self.head_fused = None         # the logit-head nn.Conv2d that took the affine_act over: Graph.head writes, _bn_train_bwd reads
        self.lazy = None               # Lazy: Graph._bn_train_fwd writes, Graph.conv / _resolve_lazies read

    def _shape(self):
        return (self.C // self.planes, self.B, self.H, self.W, self.planes) if self.planes else (self.B, self.H, self.W, self.Ct)

    def plane_elems(self):
        return self.B * self.H * self.W * self.planes

    def grad(self):
        if self.grad_t is None:
            self.grad_t = self.g.alloc(self._shape(), self.g.tdtype)
        return self.grad_t


class Act:
    """A channel slice [c0, c0+C) of a Buffer."""

    def __init__(self, buf, c0=0, C=None):
        self.buf, self.c0 = buf, c0
        self.C = buf.C if C is None else C
        self.on_side = False           # produced on the side stream: conv / hyper_level / channel_gate write, consumers read (slice() does not inherit it)

    B = property(lambda s: s.buf.B)
    H = property(lambda s: s.buf.H)
    W = property(lambda s: s.buf.W)

    def slice(self, c0, C):
        return Act(self.buf, self.c0 + c0, C)

    def _view(self, t):
        v = STRUCTS['salt_view']()
        pc = self.buf.planes
        if pc:
            # one dense plane, or the whole buffer (cs < C: only a launch that also names the plane stride may take it)
            whole = self.c0 == 0 and self.C == self.buf.C
            if self.c0 % pc or not (self.C == pc or whole):
                raise SaltError('planar buffer %s: slice [%d, %d) is not one plane of %d channels' % (self.buf.name, self.c0, self.c0 + self.C, pc))
            v.p = t.data_ptr() + (self.c0 // pc) * self.buf.plane_elems() * t.element_size()
            v.B, v.H, v.W, v.C, v.cs = self.buf.B, self.buf.H, self.buf.W, self.C, pc
            return v
        v.p = t.data_ptr() + self.c0 * t.element_size()
        v.B, v.H, v.W, v.C, v.cs = self.buf.B, self.buf.H, self.buf.W, self.C, self.buf.Ct
        return v

    def plane_stride(self):
        """plane stride (elements) a launch over the WHOLE planar buffer passes as x_plane / y_plane / q_plane; 0 for ordinary buffers"""
        return self.buf.plane_elems() if (self.buf.planes and self.C != self.buf.planes) else 0

    def view(self):
        self.buf.reads += 1
        return self._view(self.buf.t)

    def gview(self):
        return self._view(self.buf.grad())

    def grad_state(self):
        """-> accumulate flag for the next writer of this slice's gradient; marks it initialised."""
        st = self.buf.grad_init[self.c0:self.c0 + self.C]
        self.buf.grad_writers.append(GradWriter(self.c0, self.C))
        if st.all():
            return 1
        if st.any():
            raise SaltError('gradient of %s partially initialised' % self.buf.name)
        self.buf.grad_init[self.c0:self.c0 + self.C] = True
        return 0

    def offer_carrier(self, kind, struct):
        """The LAST writer of this slice's gradient (it completes it) can also take the BatchNorm-backward sums of the slice's producer:
        ``struct`` is its salt_conv_args (SUMS_CONV) or salt_bn_bwd_args (SUMS_SEC).  (a planar dL/dx has one dense consumer per plane:
        nothing to ride along)"""
        if not self.plane_stride():
            self.buf.grad_writers[-1].kind, self.buf.grad_writers[-1].carrier = kind, struct

    def grad_ready(self):
        return bool(self.buf.grad_init[self.c0:self.c0 + self.C].all())

    def _nhwc(self, t):
        if self.buf.planes:
            t = t.permute(1, 2, 3, 0, 4).reshape(self.buf.B, self.buf.H, self.buf.W, self.buf.C)
        return t[..., self.c0:self.c0 + self.C]

    def tensor(self):
        """NHWC torch view [B,H,W,C] of the activation (tests / debugging; a copy for planar buffers)."""
        return self._nhwc(self.buf.t)

    def grad_tensor(self):
        return self._nhwc(self.buf.grad())


def null_view():
    return STRUCTS['salt_view']()


def shaped_view(ptr, B, H, W, C, cs=None):
    v = STRUCTS['salt_view']()
    v.p, v.B, v.H, v.W, v.C, v.cs = ptr, B, H, W, C, (C if cs is None else cs)
    return v


def conv_taps(KH, KW, pad_y, pad_x):
    """[(kh, kw, dy, dx)] for a cross-correlation with the given top/left padding."""
    return [(kh, kw, kh - pad_y, kw - pad_x) for kh in range(KH) for kw in range(KW)]


def stack_conv_parts(B, M, H, W, F):
    """BatchNorm partials a salt_stack_conv launch over a [B,M,H,W] stack with F filters writes; SaltError for a shape the kernel does
    not run (host-side rules of csrc/stacking.hip: 1 <= M <= 64, F in {16, 32, 64}) - nothing touches the GPU."""
    S = fill(STRUCTS['salt_stack_conv_args'](), B=B, M=M, H=H, W=W, F=F)
    n = lib.salt_stack_conv_stats_parts(ctypes.byref(S))
    if n < 1:
        raise SaltError(lib.salt_last_error().decode(errors='replace'))
    return n


class Graph:
    """Forward + backward programs of one network instance for fixed (B, H, W), dtype and BN mode."""

    def __init__(self, engine, train):
        self.engine = engine
        self.device = engine.device
        self.dtype = engine.dtype
        self.dt = DT_CODE[self.dtype]
        self.tdtype = TORCH_DT[self.dtype]
        self.ve = VEC[self.dtype]
        self.train = train
        self.fwd = Program('forward')
        self.bwd = Program('backward')
        self.tape = []
        self.keep = []
        self.scratch = {}
        self.bytes = 0
        self._touched = []
        self.grad_ready = []
        self._scratch_sfx = ''
        self._virtual_acts = []        # (buffer, reads) of activations never stored: _take_act_op writes, finalize checks
        self._bias_bufs = []           # buffers that got a GradBias: the backward of scse writes, build_backward checks they were consumed
        self._lazies = []              # buffers with a Lazy record: _bn_train_fwd writes, _resolve_lazies reads and clears
        self._n_bnb = 0                # data-gradient launches that carry BatchNorm-backward sums (names their 'bnb%d' partials): _bnb_sums_source
        self._uses_bwd_packs = False   # _bwd_pack_tag writes, build_backward reads (the first main-stream backward operator joins the packs)
        self.input_grads = []          # fp32 NCHW dL/d(input) buffers: from_nchw writes, the tests' harness reads
        self.dlogits = None            # fp32 NCHW dL/d(logits): head / _head_bn / pool_head / to_nchw write, CompiledNet and the backward emitters read
        self.n_folded = 0              # affine_acts dropped by _resolve_lazies (tests, tools/fwd_fold_probe.py)
        self._shard_state = None       # {'dirty', 'rezeroed'} of the backward statistics shards: finalize writes, its run hooks and the tests read
        self.step_inputs = {}          # 'x' | 'd' -> static input tensor of the instance: CompiledNet writes, _in and the depth networks' emit read
        # fp64 statistics shards of the train-mode BatchNorm layers (SALT_BN_FIN=2): slices of one arena per program, cleared by ONE
        # salt_zero at the head of the program
        self._fin_bytes = {'fwd': 0, 'bwd': 0}
        self._fin_patches = []                   # (struct, field, 'fwd' | 'bwd', byte offset)
        self._fin_zero = {}
        if train and self._fin_mode() == 2:
            self._fin_zero['fwd'] = self.fwd.add('zero', p=1, bytes=0)

    # ------------------------------------------------------------------ memory
    def alloc(self, shape, dtype, zero=True):
        t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
        self.keep.append(t)
        self.bytes += t.numel() * t.element_size()
        return t

    def new_act(self, B, H, W, C, name='', planes=0):
        return Act(Buffer(self, B, H, W, C, name, planes))

    # ------------------------------------------------------------------ forward branches on the side stream
    @contextlib.contextmanager
    def side(self):
        """``with g.side():`` - forward operators emitted inside run on the side stream, concurrently with the main-stream operators
        emitted after the block.  The caller must call ``g.join()`` before emitting the first consumer of their results.  Shared
        scratch workspaces get their own copies ('@side').  Backward operators of the same layers are unaffected."""
        self.fwd.default_stream, self._scratch_sfx = 1, '@side'
        try:
            yield
        finally:
            self.fwd.default_stream, self._scratch_sfx = 0, ''

    def join(self):
        """The next main-stream forward operator waits for everything the side stream has been given so far."""
        self.fwd.join_next = True

    def f32(self, n):
        return self.alloc((max(int(n), 1),), torch.float32)

    def _in(self, t):
        """Address of a network input: a step input of the instance as a recorded slot (CompiledNet.bind re-points it at the caller's
        batch), any other tensor - the tests' harness and the tools emit on tensors of their own - as its plain address."""
        for key, buf in self.step_inputs.items():
            if buf is t:
                return StepInput(key, t.data_ptr())
        return t.data_ptr()

    def finalize(self):
        for buf, reads in self._virtual_acts:
            if buf.reads != reads:
                raise SaltError('activation %s is applied on the fly by its only consumer (Graph._take_act_op) but another operator asked for its storage' % buf.name)
        sizes = {}
        for prog in (self.fwd, self.bwd):
            for _, _, sc in prog.patches:
                sizes[sc.name] = max(sizes.get(sc.name, 0), sc.nbytes)
        for name, nb in sizes.items():
            self.scratch[name] = self.alloc((_round_up(max(nb, 16), 16),), torch.uint8, zero=False)
        for prog in (self.fwd, self.bwd):
            for s, path, sc in prog.patches:
                set_path(s, path, self.scratch[sc.name].data_ptr())
            prog.finalize()
        # ONE arena for the fp64 statistics shards of both programs, cleared by ONE salt_zero at the head of the FORWARD program (a
        # training step runs forward -> loss -> backward exactly once each; the backward program's own clear - a 6 us launch at the
        # head of the critical queue - is dropped: its salt_zero entry stays in the program with 0 bytes, which launches nothing).
        split = 'fwd' not in self._fin_zero
        nbf, nbb = self._fin_bytes['fwd'], self._fin_bytes['bwd']
        if self._fin_zero:
            arena = self.alloc((max((nbf + nbb) // 8, 1),), torch.float64)
            base = {'fwd': arena.data_ptr(), 'bwd': arena.data_ptr() + nbf}
            for which, z in self._fin_zero.items():
                if split:
                    fill(z, p=base[which], bytes=self._fin_bytes[which])
                else:
                    fill(z, p=base[which], bytes=(nbf + nbb) if which == 'fwd' else 0)
            for st, field, w, off in self._fin_patches:
                setattr(st, field, base[w] + off)
            if not split and nbb and 'bwd' in self._fin_zero:
                # The backward shards are accumulate-only and only the FORWARD program clears them: a backward program that is run
                # again without a fresh forward pass (loss.backward(retain_graph=True) through autograd.py, a second loss's backward,
                # bwd.run_timed in the profiling tools) would add its BatchNorm-backward sums on top of the previous run's.
                # The programs keep a 'backward shards dirty' flag: forward clears it, backward sets it, and a backward run that finds
                # it set clears its own half first (one salt_zero launch, only ever on that off-path case).
                rz = Program('rezero_bwd_shards')
                rz.add('zero', p=base['bwd'], bytes=nbb)
                rz.finalize()
                state = self._shard_state = {'dirty': False, 'rezeroed': 0}

                def fwd_done(begin, end, state=state):
                    if begin == 0:
                        state['dirty'] = False

                def bwd_begin(stream, begin, state=state, rz=rz):
                    if begin == 0:
                        if state['dirty']:
                            rz.run(stream=stream)
                            state['rezeroed'] += 1
                        state['dirty'] = True
                self.fwd._post_run, self.bwd._pre_run = fwd_done, bwd_begin
        return self

    def _fin_slot(self, which, ndoubles, *targets):
        """Reserve ``ndoubles`` fp64 of the program's statistics arena; ``targets`` = (struct, field) pairs that receive its address."""
        off = self._fin_bytes[which]
        self._fin_bytes[which] = off + _round_up(ndoubles * 8, 64)
        for st, field in targets:
            self._fin_patches.append((st, field, which, off))
        return off

    def _gp(self, param):
        """Gradient pointer of a parameter; remembers that the current backward closure finalises it."""
        self._touched.append(param)
        return self.engine.grad_ptr(param)

    def build_backward(self):
        """Emit the backward program (reverse tape order).  Also records, per parameter, the program position
        after which its gradient is final (parallel.plan_buckets turns that into all-reduce buckets)."""
        self.grad_ready = []
        self._resolve_lazies()
        if self.train and self._fin_mode() == 2 and 'bwd' not in self._fin_zero:
            self._fin_zero['bwd'] = self.bwd.add('zero', p=1, bytes=0)
        for fn in reversed(self.tape):
            self._touched = []
            fn()
            for p in self._touched:
                off, n = self.engine.grad_range(p)
                self.grad_ready.append((off, n, len(self.bwd.ops)))
        self.tape = []
        for b in self._bias_bufs:        # every folded channel-SE term must have met its bn_bwd, or x.grad is incomplete
            if b.grad_bias is not None:
                raise SaltError('gradient bias of %s was never consumed (no BatchNorm backward read that slice)' % b.name)
        # The data-gradient weight packs of the step were enqueued on the side stream during forward (Engine.refresh): the FIRST
        # main-stream operator of the backward program joins the side stream - before any weight-gradient kernel is enqueued there,
        # so the join waits for the packs only.
        if self._uses_bwd_packs:
            for i, st in enumerate(self.bwd.streams):
                if st == 0:
                    self.bwd.streams[i] = 3
                    break
                if st == 1:
                    raise SaltError('backward program starts with a side-stream operator')

    def planar_ok(self, B, H, W, C, pc, conv):
        """Can a [B,H,W,C] buffer that feeds ONE replicate-padded 3x3 convolution (the hypercolumn -> final Conv2dBnRelu,
        architectures/unet.py:101-109) be stored as C / pc dense planes?  Yes iff the library runs the forward launch on conv_ls_kernel
        (x_plane) and, in train mode, the data gradient on conv_ws_kernel (y_plane) and accepts q_plane for the weight gradient."""
        if self.dtype != 'bf16' or switches.get('SALT_NO_PLANAR') or C % pc or pc % self.ve:
            return False
        if self.train and self._fin_mode() != 2:
            return False                               # the per-tile partials protocols run on conv_mfma_kernel only
        Cout, _, KH, KW = conv.weight.shape
        if (KH, KW) != (3, 3):
            return False
        d = 1 << 20                                     # stand-in pointer (the probes only plan, nothing is launched)
        td = [(kh - (KH - 1), kw) for kh in range(KH) for kw in range(KW)]
        xv, yv, plane = shaped_view(d, B, H, W, C, pc), shaped_view(d, B, H, W, Cout), B * H * W * pc
        S = self._conv_probe(xv, d, td, 1, 1, yv, H, W)               # (x_plane: _plane_args, xv has cs < C)
        if lib.salt_conv_kernel_id(ctypes.byref(S)) != 10:
            return False
        if not self.train:
            return True
        tg = [(-t[0] - (KH - 1), -t[1]) for t in td]
        S = self._conv_probe(yv, d, tg, 1, 0, xv, H + KH - 1, W + KW - 1, fold_top=KH - 1, fold_right=KW - 1)      # (y_plane likewise)
        if lib.salt_conv_kernel_id(ctypes.byref(S)) != 9:
            return False
        Wg = fill(STRUCTS['salt_conv_wgrad_args'](), dtype=self.dt, p=yv, q=xv, ntaps=9, tap_dy=[t[0] for t in td], tap_dx=[t[1] for t in td],
                  q_step=1, pad_mode=1, q_plane=plane)
        return lib.salt_conv_wgrad_nsplit(ctypes.byref(Wg)) >= 1

    def _resolve_lazies(self):
        """SALT_FWD_BN_FOLD: drop the affine_act of every conv -> BN -> ReLU output whose only forward reader is ONE convolution that
        applies the transform in its loader; every other candidate goes back to reading the materialised activation."""
        drop = []
        for buf in self._lazies:
            lz = buf.lazy
            if len(lz.users) == 1 and buf.reads == lz.reads0:
                lz.dropped = True
                drop.append(next(i for i, (_, _, st) in enumerate(self.fwd.ops) if st is lz.sa))
            else:
                for st in lz.users:
                    fill(st, x=Act(buf).view(), in_fin=None, in_relu=0)
                    self._fin_patches = [q for q in self._fin_patches if q[0] is not st or q[1] != 'in_fin_acc']
        for i in sorted(drop, reverse=True):
            if self.fwd.streams[i] != 0:
                raise SaltError('a dropped affine_act carried a stream join')
            del self.fwd.ops[i]
            del self.fwd.streams[i]
        self._lazies = []
        self.n_folded = len(drop)

    # ------------------------------------------------------------------ helpers
    def _es(self):
        return 4 if self.dtype == 'f32' else 2

    def _conv_args(self, x_view, wp, taps_dydx, in_step, pad_mode, y_view, OH, OW, **fields):
        """The fields of a salt_conv_args over the tap offsets ``taps_dydx`` = [(dy, dx)]: what _conv_launch emits and what every
        planning probe (_conv_probe) asks the library about."""
        kw = dict(dtype=self.dt, x=x_view, w=wp, ntaps=len(taps_dydx), tap_dy=[t[0] for t in taps_dydx], tap_dx=[t[1] for t in taps_dydx],
                  in_step=in_step, pad_mode=pad_mode, y=y_view, OH=OH, OW=OW, out_step=1)
        kw.update(fields)
        kw.update(self._plane_args(x_view, y_view))
        return kw

    def _conv_probe(self, *a, **fields):
        """A filled salt_conv_args that is only planned with (salt_conv_kernel_id / salt_conv_stats_parts), never launched."""
        return fill(STRUCTS['salt_conv_args'](), **self._conv_args(*a, **fields))

    def _conv_launch(self, prog, x_view, wp, taps_dydx, in_step, pad_mode, y_view, OH, OW, part0=0, stream=None, **fields):
        return prog.add('conv', stream=stream, **self._conv_args(x_view, wp, taps_dydx, in_step, pad_mode, y_view, OH, OW, stats_part0=part0, **fields))

    @staticmethod
    def _plane_args(x_view, y_view):
        """A view over a whole PLANAR buffer has cs < C (Act._view): the launch must name the plane stride (salt_conv_args.x_plane /
        y_plane; the library fails if its kernel for these arguments cannot address planes)."""
        kw = {}
        if not isinstance(y_view, tuple) and 0 < y_view.cs < y_view.C:
            kw['y_plane'] = y_view.B * y_view.H * y_view.W * y_view.cs
        if not isinstance(x_view, tuple) and 0 < x_view.cs < x_view.C:
            kw['x_plane'] = x_view.B * x_view.H * x_view.W * x_view.cs
        return kw

    def _conv_parts(self, x_view, taps_dydx, in_step, y_view, OH, OW, **fields):
        S = self._conv_probe(x_view, 1, taps_dydx, in_step, 0, y_view, OH, OW, **fields)
        n = lib.salt_conv_stats_parts(ctypes.byref(S))
        if n < 0:
            raise SaltError('conv plan failed: ' + lib.salt_last_error().decode())
        return n

    # ------------------------------------------------------------------ BatchNorm plumbing
    @staticmethod
    def _fin_mode():
        """SALT_BN_FIN: how the train-mode BatchNorm sums travel.  2 (default): fp64 shard atomics in the producing launch, finalized
        by the consumer (salt_affine_act / the apply pass of salt_bn_bwd); 1: the same shards, finalized in the producing launch by the
        workgroup that draws the last ticket; 0: per-tile partials + separate finalize launches."""
        return switches.get('SALT_BN_FIN')

    @classmethod
    def _fin_on(cls):
        return cls._fin_mode() != 0

    def _fin_buffers(self, ndoubles):
        acc = self.alloc((ndoubles,), torch.float64)
        ticket = self.alloc((16,), torch.int32)
        return acc.data_ptr(), ticket.data_ptr()

    def _bn_fin_fields(self, bn):
        """-> (the layer's work vectors, the fields of its salt_bn_finalize_args)"""
        w = self.engine.bn_work(bn)
        nbt = bn.num_batches_tracked.data_ptr() if bn.num_batches_tracked is not None else None
        return w, dict(C=bn.num_features, gamma=bn.weight.data_ptr(), beta=bn.bias.data_ptr(), running_mean=bn.running_mean.data_ptr(),
                       running_var=bn.running_var.data_ptr(), num_batches_tracked=nbt, momentum=bn.momentum, eps=bn.eps, mean=w['mean'].data_ptr(),
                       invstd=w['invstd'].data_ptr(), scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr())

    def _bn_train_fwd(self, y, bn, relu, res, out, nparts, stats, cnt, producer=None):
        """``producer``: the argument struct of the ONE convolution launch that writes y - it then finalizes the statistics itself
        (salt_conv_args.fin) and no bn_finalize operator is emitted."""
        w, fin = self._bn_fin_fields(bn)
        F = None
        if producer is not None:
            F = fill(STRUCTS['salt_bn_finalize_args'](), **fin)
            self.keep.append(F)
            if self._fin_mode() == 1:
                acc, ticket = self._fin_buffers(8 * (2 * bn.num_features + 1))
                self.fwd.set_fields(producer, fin=ctypes.addressof(F), fin_acc=acc, fin_ticket=ticket)
                F = None
        else:
            self.fwd.add('bn_finalize', stats=stats, stats_cnt=cnt, nparts=nparts, **fin)
        if res is not None and res.on_side:
            self.join()                          # the residual branch ran on the side stream
        out.buf.bn_train_out = (out.c0, out.C)      # dL/d(out) is consumed by this layer's bn_bwd only: it may take a per-image bias (scse)
        sa = self.fwd.add('affine_act', dtype=self.dt, y=y.view(), scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(),
                          res=res.view() if res is not None else null_view(), relu=int(relu), a=out.view())
        out.buf.act_op = ActOp(sa, out.buf.reads, out.c0, out.C)     # Graph.scse may take this operator over (the activation is then never stored)
        if F is not None:                        # the producer only adds to the shards; this operator finalizes them
            self.fwd.set_fields(sa, fin=ctypes.addressof(F))
            off = self._fin_slot('fwd', 8 * (2 * bn.num_features + 1), (producer, 'fin_acc'), (sa, 'fin_acc'))
            if (fwd_bn_fold() and res is None and relu and self.dtype == 'bf16' and out.c0 == 0 and out.C == out.buf.C
                    and self.fwd.streams[-1] == 0):
                # measurement switch: if the ONLY forward reader of `out` turns out to be one 3x3 convolution, that launch
                # applies this BatchNorm + ReLU in its loader (salt_conv_args.in_*) and this affine_act is dropped (build_backward)
                out.buf.lazy = Lazy(y=y, F=F, sa=sa, off=off, reads0=out.buf.reads)
                self._lazies.append(out.buf)
        return w

    def _bn_behind(self, launch, shards, nparts, y, bn, relu, res, out, sfx):
        """The train-mode BatchNorm behind the launch(es) that write ``y``.  ``launch(**stats)`` emits them and returns the last one's
        argument struct.  ``shards`` (it is ONE launch, of a kernel that can) and SALT_BN_FIN != 0: the launch adds y's statistics to the
        fp64 shards and _bn_train_fwd wires them to its struct; otherwise per-tile partials in the 'stats' / 'stats_cnt' workspaces + a
        bn_finalize operator.  ``sfx``: suffix of the workspace names (Graph.side: a side-stream launch must not share the main
        stream's).  -> (bn work vectors, producer | None)"""
        if shards and self._fin_on():
            prod = launch()
            return self._bn_train_fwd(y, bn, relu, res, out, nparts, None, None, producer=prod), prod
        stats, cnt = Scratch('stats' + sfx, 4 * lib.salt_bn_stats_floats(nparts, y.C)), Scratch('stats_cnt' + sfx, nparts * 4)
        launch(stats=stats, stats_cnt=cnt)
        return self._bn_train_fwd(y, bn, relu, res, out, nparts, stats, cnt), None

    def _conv_bn_train(self, x, y, launches, bn, relu, res, out, sfx, plan=None):
        """Convolution x -> y whose output feeds a train-mode BatchNorm: plan the statistics partials, launch, _bn_behind.
        ``launches`` = [(packed weights, [(dy, dx)], in_step, pad_mode, OH, OW, salt_conv_args fields)]: one entry, or the output-parity
        phases of an unfused transposed convolution (each planned against a dense stand-in of its own grid; they chain stats_part0).
        ``plan``: the fields of a single launch that its partial count depends on."""
        one = len(launches) == 1
        parts = [self._conv_parts(x.view(), td, in_step, y.view() if one else shaped_view(1, x.B, OH, OW, y.C), OH, OW, **(plan or {}))
                 for _, td, in_step, _, OH, OW, _ in launches]

        def launch(**stats):
            part0 = 0
            for (wp, td, in_step, pad_mode, OH, OW, fields), n in zip(launches, parts):
                prod = self._conv_launch(self.fwd, x.view(), wp, td, in_step, pad_mode, y.view(), OH, OW, part0=part0, **fields, **stats)
                part0 += n
            return prod
        return self._bn_behind(launch, one, sum(parts), y, bn, relu, res, out, sfx)

    def _bn_train_bwd(self, y, bn, relu, res, out, w):
        """emit backward of out = relu?(bn(y) (+res)); returns nothing, leaves grad in y.grad (and res.grad)."""
        if out.buf.head_fused is not None:
            # `out` was never stored: its only reader was the logit head (Graph.head took the affine_act over) - head gradients and this
            # BatchNorm's backward from (y, dlogits) alone
            if res is not None:
                raise SaltError('fused head behind a residual BatchNorm')
            return self._head_bn_bwd(y, bn, relu, out.buf.head_fused, w)
        nparts = lib.salt_bn_bwd_parts(ctypes.byref(fill(STRUCTS['salt_bn_bwd_args'](), y=y.view())))
        C = bn.num_features
        gw, gb = self._gp(bn.weight), self._gp(bn.bias)
        coef = self.f32(3 * C)
        acc_res, dres = (res.grad_state(), res.gview()) if res is not None else (0, null_view())
        assert y.grad_state() == 0, 'conv output gradient has a single producer'
        kind, producer, partials, ready, nparts = self._bnb_sums_source(y, bn, relu, res, out, w, nparts)
        # without a residual a = relu(y*scale + shift): the kernel recomputes the mask from y and never reads `a`
        s2 = self.bwd.add('bn_bwd', dtype=self.dt, da=out.gview(), a=out.view() if (relu and res is not None) else null_view(), y=y.view(), relu=int(relu),
                          mean=w['mean'].data_ptr(), invstd=w['invstd'].data_ptr(), gamma=bn.weight.data_ptr(), beta=bn.bias.data_ptr(),
                          partials=partials, nparts=nparts, dgamma=gw, dbeta=gb, accumulate_param_grads=0,
                          coef=coef.data_ptr(), dy=y.gview(), dres=dres, accumulate_dres=acc_res, partials_ready=ready)
        bias = out.buf.grad_bias
        if bias is not None:
            # the scSE backward left the channel-SE term out of dL/d(out); THIS bn_bwd - the slice's only consumer - adds it
            self.bwd.set_fields(s2, da_bias=bias.dgap.data_ptr())
            out.buf.grad_bias = None
        if res is not None and acc_res == 0 and ready == PARTIALS_SHARDS and self._fin_mode() == 2 and C % self.ve == 0 and 256 % (C // self.ve) == 0 \
                and res.buf.bn_train_out == (res.c0, res.C) and bias is None and switches.get('SALT_BNB_SEC'):
            res.offer_carrier(SUMS_SEC, s2)            # the residual's own BatchNorm (a projection shortcut) may ask this pass for its sums (never a planar one)
        self._bnb_wire(kind, producer, ready, s2, C, bias)

    def _bnb_sums_source(self, y, bn, relu, res, out, w, nparts):
        """Who supplies the BatchNorm-backward sums of the layer out = relu?(bn(y) (+res))?  -> (SUMS_* kind, the supplier's argument struct
        | None, the ``partials`` of the layer's bn_bwd, its ``partials_ready`` code, its ``nparts``).  A supplier other than the layer's own
        reduction pass is told here what to sum over (sec_* / bnb_* / bn_* fields); its shard slots are wired by _bnb_wire once the
        bn_bwd exists."""
        C = bn.num_features
        kind, producer, partials, ready = SUMS_OWN, None, Scratch('bn_bwd', nparts * 2 * C * 4), PARTIALS_OWN
        wr = out.buf.grad_writers
        # (round 6: only the LAST writer has to cover exactly this slice - earlier writers of the same buffer, e.g. the decoder's data
        #  gradient over the whole concat buffer an encoder output lives in, are complete before it runs)
        last = wr[-1] if (wr and (wr[-1].c0, wr[-1].C) == (out.c0, out.C)) else None
        if last is not None and last.kind == SUMS_SEC:
            if not relu and res is None and self._fin_mode() == 2:
                # round 6: dL/d(out) is the dres the main branch's bn_bwd wrote (this is a projection shortcut's BatchNorm): that apply
                # pass took this layer's sums as well (salt_bn_bwd_args.sec_*) - apply-only here
                kind, producer, partials, ready = SUMS_SEC, last.carrier, None, PARTIALS_SHARDS
                self.bwd.set_fields(producer, sec_y=y.view(), sec_mean=w['mean'].data_ptr(), sec_invstd=w['invstd'].data_ptr())
            # (else a shape the secondary sums do not cover: this layer keeps its reduction pass)
        elif last is not None and last.kind == SUMS_CONV and C % self.ve == 0:
            # the LAST writer of dL/d(out) is a plain data-gradient launch (it completes the gradient: earlier writers of the same
            # slice were accumulated): its epilogue also reduces this layer's BatchNorm-backward sums over its pixel tiles
            # (salt_conv_args.bnb_*), and bn_bwd skips its own pass over da and y.  With a residual the mask comes from `out`.
            kind, producer = SUMS_CONV, last.carrier
            nparts = lib.salt_conv_stats_parts(ctypes.byref(producer))
            if nparts < 1:
                raise SaltError('conv plan failed: ' + lib.salt_last_error().decode())
            self._n_bnb += 1
            if self._fin_mode() == 2:
                partials, ready = None, PARTIALS_SHARDS          # the launch adds the sums to fp64 shards; the apply pass of bn_bwd finalizes them
            elif self._fin_mode() == 1:
                partials, ready = None, PARTIALS_FINALIZED       # the launch also finalizes (salt_conv_args.bnb_fin): bn_bwd is the apply pass only
            else:
                partials, ready = Scratch('bnb%d' % self._n_bnb, nparts * 2 * C * 4), PARTIALS_FILLED
            self.bwd.set_fields(producer, bnb_y=y.view(), bnb_mean=w['mean'].data_ptr(), bnb_invstd=w['invstd'].data_ptr(), bnb_gamma=bn.weight.data_ptr(),
                                bnb_beta=bn.bias.data_ptr(), bnb_partials=partials, bnb_relu=int(relu),
                                bnb_a=out.view() if (relu and res is not None) else null_view())
        bias = out.buf.grad_bias
        if bias is not None:
            if (bias.c0, bias.C) != (out.c0, out.C):
                raise SaltError('gradient bias of %s covers channels [%d, %d), this BatchNorm backward reads [%d, %d)'
                                % (out.buf.name, bias.c0, bias.c0 + bias.C, out.c0, out.c0 + out.C))
            if ready != PARTIALS_OWN:
                raise SaltError('a per-image gradient bias needs the reduction pass of bn_bwd (the producer of dL/da is not a convolution)')
            if bias.sums_from is not None:
                # the scSE backward also took this layer's BatchNorm-backward sums (salt_scse_bwd_args.bnb_acc)
                kind, producer, partials, ready = SUMS_SCSE, bias.sums_from, None, PARTIALS_SHARDS
                self.bwd.set_fields(producer, bn_mean=w['mean'].data_ptr(), bn_invstd=w['invstd'].data_ptr())
        return kind, producer, partials, ready, nparts

    def _bnb_wire(self, kind, producer, ready, s2, C, bias):
        """Shard slots / tickets between the supplier of a layer's BatchNorm-backward sums (_bnb_sums_source) and its bn_bwd ``s2``."""
        if kind == SUMS_SEC:
            self._fin_slot('bwd', 8 * 2 * C, (producer, 'sec_acc'), (s2, 'fin_acc'))
        elif kind == SUMS_SCSE:
            peers = [(bias.fc_grads, 'bnb_acc')] if bias.fc_grads is not None else []       # scse_fc_grads reads the same 6 C + 1 wide rows
            self._fin_slot('bwd', 8 * 2 * C, (producer, 'bnb_acc'), (s2, 'fin_acc'), *peers)
        elif kind == SUMS_CONV and ready == PARTIALS_SHARDS:
            self._fin_slot('bwd', 8 * 2 * C, (producer, 'bnb_acc'), (s2, 'fin_acc'))
        elif kind == SUMS_CONV and ready == PARTIALS_FINALIZED:
            acc, ticket = self._fin_buffers(8 * 2 * C)
            self.bwd.set_fields(producer, bnb_fin=ctypes.addressof(s2), bnb_acc=acc, bnb_ticket=ticket)
        elif kind == SUMS_OWN and self._fin_mode() == 2:
            self._fin_slot('bwd', 8 * 2 * C, (s2, 'fin_acc'))       # reduction pass -> shards -> apply pass
        elif kind == SUMS_OWN and self._fin_mode() == 1:
            acc, ticket = self._fin_buffers(8 * 2 * C)       # the reduction pass of bn_bwd finalizes in-launch
            self.bwd.set_fields(s2, fin_acc=acc, fin_ticket=ticket)
        # (SUMS_CONV with PARTIALS_FILLED, SUMS_OWN under SALT_BN_FIN=0: per-tile partials in scratch, nothing to wire)

    # ------------------------------------------------------------------ dense convolution (+BN +ReLU +residual)
    def conv(self, x, conv, bn=None, relu=False, res=None, out=None, replicate=False, name='', raw_stats=None):
        """nn.Conv2d (k in {1,3} or (k,1)/(1,k); stride 1|2; zero pad or the reference's replicate top/right pad)
        optionally followed by BatchNorm2d, residual add and ReLU.  ``raw_stats`` (train, bn None): callable(stats, stats_cnt, nparts) -
        the launch also reports the per-tile statistics of its raw output (a dense layer's conv2 feeds the block's statistics table)."""
        eng = self.engine
        Cout, Cin, KH, KW = conv.weight.shape
        assert Cin == x.C, (name, Cin, x.C)
        stride = conv.stride[0]
        if replicate:
            assert stride == 1
            taps = [(kh, kw, kh - (KH - 1), kw) for kh in range(KH) for kw in range(KW)]
            pad_mode, OH, OW = 1, x.H, x.W
        else:
            py, px = conv.padding
            taps = conv_taps(KH, KW, py, px)
            pad_mode, OH, OW = 0, (x.H + 2 * py - KH) // stride + 1, (x.W + 2 * px - KW) // stride + 1
        tk = [(t[0], t[1]) for t in taps]
        td = [(t[2], t[3]) for t in taps]
        pk = eng.packs.dense(conv, tk, transposed=False)
        bias = conv.bias.data_ptr() if conv.bias is not None else None
        if out is None:
            out = self.new_act(x.B, OH, OW, Cout, name)
        assert (out.B, out.H, out.W, out.C) == (x.B, OH, OW, Cout), name
        y = w = None
        lz = x.buf.lazy if (self.train and x.c0 == 0 and x.C == x.buf.C and len(taps) == 9 and stride == 1) else None
        if bn is not None and self.train:
            y = self.new_act(x.B, OH, OW, Cout, name + '.y')
            xin, fold = x, {}
            if lz is not None and self._fin_on():
                # candidate for the loader fold: read the producer's raw output and transform it on the way into LDS
                S = self._conv_probe(lz.y.view(), 1, td, 1, pad_mode, y.view(), OH, OW, in_fin=ctypes.addressof(lz.F), in_fin_acc=8, in_relu=1)
                if lib.salt_conv_kernel_id(ctypes.byref(S)) in (1, 2, 3, 4):
                    xin, fold = lz.y, dict(in_fin=ctypes.addressof(lz.F), in_relu=1)
            if not fold:
                lz = None
            # (workspace names carry _scratch_sfx: a side-stream launch gets its own 'stats@side')
            w, prod = self._conv_bn_train(xin, y, [(pk.data_ptr(), td, stride, pad_mode, OH, OW, dict(bias=bias, **fold))], bn, relu, res, out,
                                          self._scratch_sfx)
            if fold:
                self._fin_patches.append((prod, 'in_fin_acc', 'fwd', lz.off))
                lz.users.append(prod)
        elif bn is not None:
            w = eng.bn_work(bn)
            act = dict(bias=bias, scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr())
            if res is None:
                self._conv_launch(self.fwd, x.view(), pk.data_ptr(), td, stride, pad_mode, out.view(), OH, OW, relu=int(relu), **act)
            elif Cout % self.ve == 0 and not switches.get('SALT_NO_RES_FOLD'):
                # eval-mode residual block: folded BN + identity add + ReLU all in the convolution's epilogue (salt_conv_args.res) - the
                # same values as the separate affine_act pass below, bit for bit, without its launch and its trip over `out`
                if res.on_side:
                    self.join()
                self._conv_launch(self.fwd, x.view(), pk.data_ptr(), td, stride, pad_mode, out.view(), OH, OW, relu=int(relu), res=res.view(), **act)
            else:
                self._conv_launch(self.fwd, x.view(), pk.data_ptr(), td, stride, pad_mode, out.view(), OH, OW, relu=0, **act)
                if res.on_side:
                    self.join()
                self.fwd.add('affine_act', dtype=self.dt, y=out.view(), scale=None, shift=None, res=res.view(), relu=int(relu), a=out.view())
        elif raw_stats is not None and self.train:
            assert res is None and not relu
            nparts = self._conv_parts(x.view(), td, stride, out.view(), OH, OW)
            st = dict(stats=Scratch('stats' + self._scratch_sfx, 4 * lib.salt_bn_stats_floats(nparts, Cout)), stats_cnt=Scratch('stats_cnt' + self._scratch_sfx, nparts * 4))
            self._conv_launch(self.fwd, x.view(), pk.data_ptr(), td, stride, pad_mode, out.view(), OH, OW, bias=bias, relu=0, **st)
            raw_stats(st['stats'], st['stats_cnt'], nparts)
        else:
            assert res is None
            self._conv_launch(self.fwd, x.view(), pk.data_ptr(), td, stride, pad_mode, out.view(), OH, OW, bias=bias, relu=int(relu))
        out.on_side = self.fwd.default_stream == 1
        if self.train:
            def backward():
                if bn is not None:
                    self._bn_train_bwd(y, bn, relu, res, out, w)
                    dy = y
                else:
                    if conv.bias is not None:
                        raise NotImplementedError('bias gradient of a dense conv without BatchNorm (not on the reference path)')
                    dy = out
                    if relu:
                        self.bwd.add('relu_bwd', dtype=self.dt, da=out.gview(), a=out.view(), dy=out.gview(), accumulate=0)
                # weight gradient: P = dY (a = cout), Q = X (b = cin)
                if lz is not None and lz.dropped:
                    # the activation was never materialised and the weight-gradient kernels (LDS-DMA loaders) cannot transform their
                    # operand: a graph built under SALT_FWD_BN_FOLD has no backward pass (fail loudly, never a wrong gradient)
                    raise SaltError('SALT_FWD_BN_FOLD graphs are forward-only (the folded activation of %s does not exist for the weight gradient)' % name)
                self._wgrad(dy.gview(), x.view(), td, tk, stride, pad_mode, conv.weight, KH, KW)
                # data gradient
                if x.buf.name != '__input__':
                    self._dgrad(conv, x, dy, taps, stride, replicate, KH, KW)
            self.tape.append(backward)
        return out

    # ------------------------------------------------------------------ factored hypercolumn (saltnet.h: salt_hyper_stencil)
    def hyper_factor_ok(self, B, H, W, C, Rs):
        """Can the levels up-sampled by ``Rs`` leave the hypercolumn (architectures/unet.py:101-109) and enter the final Conv2dBnRelu
        through the low-resolution tap GEMM + stencil instead?  (the stencil's shape rules, saltnet.h; consumer-side BatchNorm shards)"""
        if not Rs or C % 8 or (self.train and self._fin_mode() != 2) or (self.train and W > 256):
            return False
        if C % (16 if self.dtype == 'f32' else 32):
            return False                                # the transposed tap-GEMM pack places whole chunks
        return all(R >= 4 and R & (R - 1) == 0 and R <= 32 and H % R == 0 and W % R == 0 for R in Rs)

    def hyper_head_ok(self, C, hconv):
        """Can salt_hyper_stencil's epilogue apply the logit head ``hconv`` (eval; saltnet.h: 1..2 classes, 1 / 2 / 4 / 8 channel blocks)?"""
        if self.train:
            return False
        co, ci, kh, kw = hconv.weight.shape
        return (kh, kw) == (1, 1) and ci == C and 1 <= co <= 2 and C in ((64, 128, 256) if self.dtype == 'f32' else (64, 128, 256, 512))

    def head_bn_ok(self, C, hconv):
        """TRAIN mode: can the final block's BatchNorm apply + ReLU and the logit head ``hconv`` run as one pass over the raw convolution
        output (salt_head_bn / salt_head_bn_bwd; saltnet.h: <= 4 classes, C a power-of-two number of 16-byte pieces <= 64, consumer-side
        statistics shards)?  SALT_HEAD_BN=0 keeps the separate launches (A/B)."""
        if not self.train or self._fin_mode() != 2 or not switches.get('SALT_HEAD_BN'):
            return False
        co, ci, kh, kw = hconv.weight.shape
        cpv = C // self.ve
        return (kh, kw) == (1, 1) and ci == C and 1 <= co <= 4 and C % self.ve == 0 and 1 <= cpv <= 64 and cpv & (cpv - 1) == 0

    def _head_bn(self, y, bn, relu, hconv, logits, producer):
        """forward salt_head_bn behind ``producer`` (which adds y's statistics to the fp64 shards); the caller's backward closure starts
        with its counterpart _head_bn_bwd."""
        C = bn.num_features
        w, fin = self._bn_fin_fields(bn)
        F = fill(STRUCTS['salt_bn_finalize_args'](), **fin)
        self.keep.append(F)
        Cout = hconv.weight.shape[0]
        hb = self.fwd.add('head_bn', dtype=self.dt, y=y.view(), fin=ctypes.addressof(F), relu=int(relu), w=hconv.weight.data_ptr(),
                          bias=hconv.bias.data_ptr() if hconv.bias is not None else None, Cout=Cout, y_nchw=logits.data_ptr())
        self._fin_slot('fwd', 8 * (2 * C + 1), (producer, 'fin_acc'), (hb, 'fin_acc'))
        self.dlogits = self.alloc(tuple(logits.shape), torch.float32)

        return w

    def _head_bn_bwd(self, y, bn, relu, hconv, w):
        """backward of the fused BatchNorm apply + ReLU + logit head (Graph.head / _head_bn): head gradients and the BatchNorm backward
        from (y, dlogits) alone; leaves dL/dy in y.grad."""
        C, Cout = bn.num_features, hconv.weight.shape[0]
        S = fill(STRUCTS['salt_head_bn_bwd_args'](), y=y.view())
        nparts = lib.salt_head_bn_bwd_parts(ctypes.byref(S))
        assert y.grad_state() == 0, 'conv output gradient has a single producer'
        sb = self.bwd.add('head_bn_bwd', dtype=self.dt, y=y.view(), relu=int(relu), mean=w['mean'].data_ptr(), invstd=w['invstd'].data_ptr(),
                          gamma=bn.weight.data_ptr(), beta=bn.bias.data_ptr(), w=hconv.weight.data_ptr(), Cout=Cout, dy_nchw=self.dlogits.data_ptr(),
                          partials=Scratch('head', nparts * Cout * (C + 1) * 4), nparts=nparts, gw=self._gp(hconv.weight),
                          gb=self._gp(hconv.bias) if hconv.bias is not None else None, dgamma=self._gp(bn.weight), dbeta=self._gp(bn.bias),
                          coef=self.f32(3 * C).data_ptr(), dy=y.gview())
        self._fin_slot('bwd', 8 * 2 * C, (sb, 'fin_acc'))

    def hyper_level(self, x, conv, c0, name='hyper.z'):
        """z = [W[:, c0 : c0 + x.C, kh, kw]]_taps x  at x's (LOW) resolution: one 1x1 convolution x.C -> 9 Cout whose output channel
        t Cout + o is tap t of output channel o of the 3x3 convolution ``conv`` restricted to the input channels of this level.
        Backward (from dz, which conv_hyper's stencil adjoint writes): the 1x1 weight gradient scattered into conv.weight.grad and
        the 1x1 data gradient into dL/dx."""
        eng = self.engine
        Cout, _, KH, KW = conv.weight.shape
        taps = [(kh, kw) for kh in range(KH) for kw in range(KW)]
        pk = eng.packs.tapgemm(conv, c0, x.C, transposed=False)
        z = self.new_act(x.B, x.H, x.W, len(taps) * Cout, name)
        # cfg 11 | 1 << 16: ask for conv1x1_ls_kernel with 32-channel items wherever it applies - the heuristic sends these few-pixel
        # launches to conv_mfma_kernel's 128 x 32 tiles (a serial chain of K / 32 staged chunks per workgroup: 30 us for 0.15 GFLOP)
        # (with thousands of 64-channel items - the 256 x 256 inference shapes - 64-channel items halve the re-reads of x instead)
        items64 = (x.B * x.H * x.W // 256) * (len(taps) * Cout // 64)
        ask = 11 | ((1 << 16) if items64 < 2048 else 0)
        self._conv_launch(self.fwd, x.view(), pk.data_ptr(), [(0, 0)], 1, 0, z.view(), x.H, x.W, cfg=ask)
        z.on_side = self.fwd.default_stream == 1
        if self.train:
            D1 = conv.weight.shape[1]

            def backward():
                if not z.grad_ready():
                    raise SaltError('hyper_level: dL/dz was never written (conv_hyper must consume %s)' % name)
                self._wgrad(z.gview(), x.view(), [(0, 0)], None, 1, 0, conv.weight, KH, KW, b_slice=(c0, D1), tapgemm=(Cout, taps))
                pkt = eng.packs.tapgemm(conv, c0, x.C, transposed=True, bwd=True)
                acc = x.grad_state()
                self._conv_launch(self.bwd, z.gview(), pkt.data_ptr(), [(0, 0)], 1, 0, x.gview(), x.H, x.W, accumulate=acc, stream=self._bwd_pack_tag(), cfg=ask)
            self.tape.append(backward)
        return z

    def conv_hyper(self, x, zs, Rs, conv, bn, relu=True, out=None, name='final', head=None):
        """Conv2dBnRelu over the hypercolumn (architectures/unet.py:84-87,101-109; base.py:21-37) with the levels of ``zs`` factored out:
        y = conv3x3_replicate(x; W[:, :x.C]) + bias, then salt_hyper_stencil adds sum_k stencil_k(z_k) (and takes the BatchNorm
        statistics of the sum in training / applies the folded BatchNorm + ReLU in eval); x holds the full-resolution channels only.
        ``head`` = (nn.Conv2d(Cout, classes, 1), fp32 NCHW logits), eval only: the block's only consumer in the reference's ``final``
        Sequential (architectures/unet.py:84-87) is applied by the stencil's epilogue (salt_hyper_stencil_args.head_*; same values as
        salt_head1x1 on the stored activation, which is then never written) and None is returned."""
        eng = self.engine
        Cout, Cin, KH, KW = conv.weight.shape
        assert (KH, KW) == (3, 3) and bn is not None and x.C <= Cin and all(z.C == 9 * Cout for z in zs)
        taps = [(kh, kw, kh - (KH - 1), kw) for kh in range(KH) for kw in range(KW)]
        tk = [(t[0], t[1]) for t in taps]
        td = [(t[2], t[3]) for t in taps]
        d1 = (0, x.C)
        pk = eng.packs.dense(conv, tk, transposed=False, d1=d1)
        bias = conv.bias.data_ptr() if conv.bias is not None else None
        if head is not None and not (self.head_bn_ok(Cout, head[0]) if self.train else self.hyper_head_ok(Cout, head[0])):
            raise SaltError('conv_hyper: this head cannot be fused (ask hyper_head_ok / head_bn_ok first)')
        if out is None and head is None:
            out = self.new_act(x.B, x.H, x.W, Cout, name)
        ac = int(bool(getattr(getattr(self.engine, 'module', None), 'align_corners', False)))
        y = self.new_act(x.B, x.H, x.W, Cout, name + '.y')
        self._conv_launch(self.fwd, x.view(), pk.data_ptr(), td, 1, 1, y.view(), x.H, x.W, bias=bias)
        if any(z.on_side for z in zs):
            self.join()
        st = dict(dtype=self.dt, nlev=len(zs), z=[z.view() for z in zs], R=list(Rs), y_in=y.view(), backward=0, align_corners=ac)
        zs, Rs = list(zs), list(Rs)

        def backward_from_dy():
            """dL/dy -> the stencil adjoint into every dL/dz, the weight gradient and the data gradient of the full-resolution part"""
            for z in zs:
                assert z.grad_state() == 0
            self.bwd.add('hyper_stencil', dtype=self.dt, nlev=len(zs), z=[z.gview() for z in zs], R=Rs, y_in=null_view(), y=y.gview(),
                         backward=1, align_corners=ac)
            self._wgrad(y.gview(), x.view(), td, tk, 1, 1, conv.weight, KH, KW, b_slice=(0, Cin))
            self._dgrad(conv, x, y, taps, 1, True, KH, KW, d1=d1)
        if self.train and head is not None:
            # round 6: BatchNorm apply + ReLU + logit head in ONE pass over the raw sum (salt_head_bn): the block's activation and its
            # gradient are never stored.  Backward: salt_head_bn_bwd writes dL/dy directly (head gradients + BatchNorm-backward sums in
            # its first pass), then the stencil adjoint / weight gradient / data gradient as below.
            prod = self.fwd.add('hyper_stencil', y=y.view(), **st)
            w = self._head_bn(y, bn, relu, head[0], head[1], prod)
            self.tape.append(lambda: (self._head_bn_bwd(y, bn, relu, head[0], w), backward_from_dy()))
            return None
        if self.train:
            # (hyper_factor_ok: consumer-side shards only - the stencil has no per-tile partials protocol, so no workspace is ever named)
            w, _ = self._bn_behind(lambda: self.fwd.add('hyper_stencil', y=y.view(), **st), True, 0, y, bn, relu, None, out, '')
        elif head is not None:
            w = eng.bn_work(bn)
            hconv, logits = head
            yv = y.view()
            yv.p = None                                  # shape only: the activated block output is never stored
            self.fwd.add('hyper_stencil', y=yv, scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(), relu=int(relu),
                         head_w=hconv.weight.data_ptr(), head_b=hconv.bias.data_ptr() if hconv.bias is not None else None,
                         head_y_nchw=logits.data_ptr(), head_cout=hconv.weight.shape[0],
                         head_ws=self.alloc((x.B * (Cout // 64) * hconv.weight.shape[0] * x.H * x.W,), torch.float32).data_ptr() if Cout > 64 else None, **st)
            return None
        else:
            w = eng.bn_work(bn)
            self.fwd.add('hyper_stencil', y=out.view(), scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(), relu=int(relu), **st)
        out.on_side = False
        if self.train:
            self.tape.append(lambda: (self._bn_train_bwd(y, bn, relu, None, out, w), backward_from_dy()))
        return out

    def _wgrad(self, p_view, q_view, taps_dydx, taps_khkw, q_step, pad_mode, weight, KH, KW, b_slice=None, tapgemm=None):
        """dW = sum_p P[p,:]^T Q[p*q_step + tap, :] -> weight.grad (reference layout [Ca][Cb][KH][KW]).
        ``b_slice`` = (first, row stride): Q covers only channels [first, first + Cb) of the weight's second axis (salt_wgrad_reduce_args.ldb).
        ``tapgemm`` = (rows, [(kh, kw)]): a 1x1 launch whose P channels are t * rows + a (salt_wgrad_reduce_args.a_mod) - Graph.hyper_level."""
        gw = self._gp(weight)
        Ca, Cb = p_view.C, q_view.C
        extra = {}
        if b_slice is not None:
            gw += 4 * b_slice[0] * KH * KW
            extra['ldb'] = b_slice[1]
        if tapgemm is not None:
            assert len(taps_dydx) == 1 and Ca == tapgemm[0] * len(tapgemm[1])
            extra['a_mod'] = tapgemm[0]
            taps_khkw = list(tapgemm[1])
        for i in range(0, len(taps_dydx), 9 if len(taps_dydx) != 16 else 4):
            chunk = list(range(i, min(i + (9 if len(taps_dydx) != 16 else 4), len(taps_dydx))))
            qp = q_view.B * q_view.H * q_view.W * q_view.cs if 0 < q_view.cs < q_view.C else 0       # planar Q (Act._view of a whole planar buffer)
            wg = dict(dtype=self.dt, p=p_view, q=q_view, ntaps=len(chunk), tap_dy=[taps_dydx[j][0] for j in chunk],
                      tap_dx=[taps_dydx[j][1] for j in chunk], q_step=q_step, pad_mode=pad_mode, q_plane=qp)
            ns = lib.salt_conv_wgrad_nsplit(ctypes.byref(fill(STRUCTS['salt_conv_wgrad_args'](), **wg)))
            if ns < 0:
                raise SaltError('wgrad plan failed: ' + lib.salt_last_error().decode())
            nbytes = ns * len(chunk) * Ca * Cb * 4
            self.bwd.add('conv_wgrad', stream=1, partials=Scratch('wgrad', nbytes), nsplit=ns, **wg)
            rt = range(len(taps_khkw)) if tapgemm is not None else chunk
            rfields = dict(nsplit=ns, ntaps=len(chunk), Ca=Ca, Cb=Cb, KH=KH, KW=KW, tap_kh=[taps_khkw[j][0] for j in rt],
                           tap_kw=[taps_khkw[j][1] for j in rt], accumulate=0, **extra)
            self.bwd.add('wgrad_reduce', stream=1, partials=Scratch('wgrad', nbytes), grad=gw, **rfields)

    def _bwd_pack_tag(self):
        """Stream tag of a data-gradient convolution: the first one of the backward program joins the side stream, where the
        data-gradient weight packs of this step were enqueued during forward (Engine.refresh)."""
        self._uses_bwd_packs = True
        return None

    def _dgrad(self, conv, x, dy, taps, stride, replicate, KH, KW, d1=None):
        eng = self.engine
        tk = [(t[0], t[1]) for t in taps]
        pk = eng.packs.dense(conv, tk, transposed=True, bwd=True, d1=d1)       # n = cin, c = cout
        if replicate:
            # gradient w.r.t. the replicate-padded input on the extended domain, then fold the pad back
            top, right = KH - 1, KW - 1
            Hp, Wp = x.H + top, x.W + right
            td = [(-(t[2]) - top, -(t[3])) for t in taps]
            acc = x.grad_state()
            fused = x.C % self.ve == 0
            if fused and (top >= 8 or right >= 8):
                # a long line kernel ((9, 1) / (1, 9): the composed route of Graph.gcn_pair): the fused fold needs tiles larger than the pad,
                # which the plan of a small map does not give - ask it, and take the strip fold where it refuses
                S = self._conv_probe(dy._view(dy.buf.grad()), 1, td, 1, 0, x._view(x.buf.grad()), Hp, Wp, fold_top=top, fold_right=right)
                fused = lib.salt_conv_stats_parts(ctypes.byref(S)) >= 0
                if not fused and 'fused fold needs tiles larger than the pad' not in lib.salt_last_error().decode(errors='replace'):
                    raise SaltError('conv plan failed: ' + lib.salt_last_error().decode(errors='replace'))       # any other refusal is not the strip's to hide
            if fused:
                # fused fold: the launch tiles the extended grid so that every pad-ring pixel shares a tile with the edge pixel it folds
                # onto; the epilogue sums them from the staged tile - no strip, no second pass, and (a plain store of the complete
                # gradient) the launch can carry the BatchNorm-backward sums of x's producer
                s = self._conv_launch(self.bwd, dy.gview(), pk.data_ptr(), td, 1, 0, x.gview(), Hp, Wp, accumulate=acc,
                                      fold_top=top, fold_right=right, stream=self._bwd_pack_tag())
                x.offer_carrier(SUMS_CONV, s)
                return
            # strip fold: interior pixels go straight into x.grad, only the pad ring takes the detour through scratch
            scs = _round_up(x.C, self.ve)
            ring = lib.salt_fold_strip_pixels(x.H, x.W, top, 0, 0, right)
            strip = Scratch('dgrad_ring', x.B * ring * scs * self._es())
            self._conv_launch(self.bwd, dy.gview(), pk.data_ptr(), td, 1, 0, x.gview(), Hp, Wp, accumulate=acc,
                              strip=strip, strip_cs=scs, fold_top=top, fold_right=right, stream=self._bwd_pack_tag())
            self.bwd.add('pad_fold_strip', dtype=self.dt, strip=strip, strip_cs=scs, top=top, bottom=0, left=0, right=right, x=x.gview())
            return
        acc = x.grad_state()
        if stride == 1:
            td = [(-t[2], -t[3]) for t in taps]
            s = self._conv_launch(self.bwd, dy.gview(), pk.data_ptr(), td, 1, 0, x.gview(), x.H, x.W, accumulate=acc, stream=self._bwd_pack_tag())
            x.offer_carrier(SUMS_CONV, s)              # a plain full-grid launch: can carry the BatchNorm-backward sums of x's producer
            return
        # stride 2: the data gradient is a transposed convolution - four output-parity phases
        phases = []
        for ay in range(2):
            for ax in range(2):
                sel = [i for i, t in enumerate(taps) if (t[2] - ay) % 2 == 0 and (t[3] - ax) % 2 == 0]
                phases.append((ay, ax, sel))
        fused = self._phase_fused([[(((ay - taps[i][2]) // 2, (ax - taps[i][3]) // 2), tk[i]) for i in sel] for ay, ax, sel in phases], x.H, x.W)
        if fused is not None:
            # ONE launch for all four phases (each its own packed weight block; taps a phase lacks are zero weights)
            td_u, phase_taps = fused
            pk_t, elems = eng.packs.phases(conv, phase_taps, transposed=True, bwd=True)
            s = self._conv_launch(self.bwd, dy.gview(), pk_t.data_ptr(), td_u, 1, 0, x.gview(), x.H // 2, x.W // 2, out_step=2, accumulate=acc,
                                  nphase=4, w_phase_elems=elems, stream=self._bwd_pack_tag())
            x.offer_carrier(SUMS_CONV, s)              # all four parities of an even grid: every pixel once - can carry the BatchNorm-backward sums (round 6)
            return
        if any(not sel for _, _, sel in phases) and not acc:
            self.fill(x, 0.0, grad=True)
            acc = 1
        for ay, ax, sel in phases:
            oh, ow = (x.H - ay + 1) // 2, (x.W - ax + 1) // 2
            if not sel or oh <= 0 or ow <= 0:
                continue
            pk_s = eng.packs.dense(conv, [tk[i] for i in sel], transposed=True, bwd=True)
            td = [((ay - taps[i][2]) // 2, (ax - taps[i][3]) // 2) for i in sel]
            self._conv_launch(self.bwd, dy.gview(), pk_s.data_ptr(), td, 1, 0, x.gview(), oh, ow, out_step=2, out_oy=ay, out_ox=ax, accumulate=acc,
                              stream=self._bwd_pack_tag())

    def _phase_fused(self, per_phase, H, W):
        """per_phase: for each of the 4 output-parity phases a list of ((dy, dx), (kh, kw)).  -> (unified tap offsets, per-phase
        (kh, kw) | None lists) when the phases can share one launch (even grid, <= 9 distinct offsets, at least two non-empty
        phases), else None."""
        if H % 2 or W % 2:
            return None
        offs = sorted({o for ph in per_phase for o, _ in ph})
        if not offs or len(offs) > 9 or sum(1 for ph in per_phase if ph) < 2:
            return None
        # every phase runs ALL unified offsets (missing ones against zero weights): worth one launch instead of four only while the
        # padded work stays below ~2x (k3: 16 taps for 9 real ones; k4: 36 for 16 - not fused)
        if 4 * len(offs) > 1.8 * sum(len(ph) for ph in per_phase):
            return None
        if len(offs) not in (4, 9):               # the kernels unroll 4- and 9-tap loops; pad other counts with a repeated zero tap
            offs = offs + [offs[0]] * ((4 if len(offs) < 4 else 9) - len(offs))
        phase_taps = []
        for ph in per_phase:
            d = dict(ph)
            used = set()
            row = []
            for o in offs:
                if o in d and o not in used:
                    row.append(d[o]); used.add(o)
                else:
                    row.append(None)
            phase_taps.append(row)
        return offs, phase_taps

    def fill(self, act, value, grad=False):
        assert value == 0.0
        t = act.buf.grad() if grad else act.buf.t
        if act.c0 == 0 and act.C == act.buf.C:
            (self.bwd if grad else self.fwd).add('zero', p=t.data_ptr(), bytes=t.numel() * t.element_size())
        else:   # channel slice: y = a - a via affine (scale 0) keeps it one pass
            z = self.f32(2 * act.C)
            v = act.gview() if grad else act.view()
            (self.bwd if grad else self.fwd).add('affine_act', dtype=self.dt, y=v, scale=z.data_ptr(), shift=z.data_ptr() + 4 * act.C,
                                                 res=null_view(), relu=0, a=v)

    # ------------------------------------------------------------------ transposed convolution (k3 op1 / k4, stride 2, pad 1)
    def conv_transpose(self, x, deconv, bn=None, relu=False, out=None, name=''):
        eng = self.engine
        Cin, Cout, KH, KW = deconv.weight.shape
        assert Cin == x.C and deconv.stride[0] == 2 and deconv.padding[0] == 1 and KH == KW and KH in (3, 4)
        p = 1
        OH, OW = 2 * x.H, 2 * x.W
        bias = deconv.bias.data_ptr() if deconv.bias is not None else None
        if out is None:
            out = self.new_act(x.B, OH, OW, Cout, name)
        train_bn = bn is not None and self.train
        tgt = self.new_act(x.B, OH, OW, Cout, name + '.y') if train_bn else out
        w = eng.bn_work(bn) if bn is not None else None
        phases = []
        for fy in range(2):
            for fx in range(2):
                sel = [(u, v, (fy + p - u) // 2, (fx + p - v) // 2) for u in range(KH) for v in range(KW)
                       if (fy + p - u) % 2 == 0 and (fx + p - v) % 2 == 0]
                phases.append((fy, fx, sel))
        fused = self._phase_fused([[((s_[2], s_[3]), (s_[0], s_[1])) for s_ in sel] for _, _, sel in phases], OH, OW)
        if fused is not None:
            # ONE launch for the four output-parity phases of the transposed convolution
            td_u, phase_taps = fused
            pk_t, elems = eng.packs.phases(deconv, phase_taps, transposed=True)
            plan = dict(out_step=2, nphase=4, w_phase_elems=elems)
            launches = [(pk_t.data_ptr(), td_u, 1, 0, x.H, x.W, dict(bias=bias, **plan))]
        else:
            plan = None
            launches = [(eng.packs.dense(deconv, [(s[0], s[1]) for s in sel], transposed=True).data_ptr(), [(s[2], s[3]) for s in sel], 1, 0, x.H, x.W,
                         dict(out_step=2, out_oy=fy, out_ox=fx, bias=bias)) for fy, fx, sel in phases]       # n = cout (D1), c = cin (D0)
        if train_bn:
            # The workspace names carry NO _scratch_sfx here, unlike conv / _stem_s2d: a transposed convolution emitted inside Graph.side()
            # shares 'stats' / 'stats_cnt' with the main stream.  Known asymmetry, kept as it is (it decides which workspace a launch uses).
            self._conv_bn_train(x, tgt, launches, bn, relu, None, out, '', plan=plan)
        else:
            act = dict(scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr()) if bn is not None else {}
            for wp, td, in_step, pad_mode, oh, ow, fields in launches:
                self._conv_launch(self.fwd, x.view(), wp, td, in_step, pad_mode, tgt.view(), oh, ow, relu=int(relu), **act, **fields)
        if self.train:
            def backward():
                if bn is None:
                    raise NotImplementedError('ConvTranspose2d without BatchNorm in training')
                self._bn_train_bwd(tgt, bn, relu, None, out, w)
                taps_all = [(u, v, u - p, v - p) for u in range(KH) for v in range(KW)]
                # weight gradient: P = X (a = cin), Q = dY (b = cout), dY sampled at 2i - p + u
                self._wgrad(x.view(), tgt.gview(), [(t[2], t[3]) for t in taps_all], [(t[0], t[1]) for t in taps_all], 2, 0,
                            deconv.weight, KH, KW)
                # data gradient: stride-2 convolution of dY with W[cin][cout] (n = cin, c = cout)
                pk = eng.packs.dense(deconv, [(t[0], t[1]) for t in taps_all], transposed=False, bwd=True)
                acc = x.grad_state()
                self._conv_launch(self.bwd, tgt.gview(), pk.data_ptr(), [(t[2], t[3]) for t in taps_all], 2, 0, x.gview(), x.H, x.W, accumulate=acc,
                                  stream=self._bwd_pack_tag())
            self.tape.append(backward)
        return out

    # ------------------------------------------------------------------ first layer (fp32 NCHW input image)
    def conv_first(self, x_nchw, conv, bn, relu=True, name=''):
        eng = self.engine
        B, Cin, H, W = x_nchw.shape
        Cout, _, K, _ = conv.weight.shape
        stride, pad = conv.stride[0], conv.padding[0]
        if stride == 2 and K % 2 == 1 and pad == K // 2 and H % 2 == 0 and W % 2 == 0 and conv.bias is None and bn is not None:
            return self._stem_s2d(x_nchw, conv, bn, relu, name)
        OH = (H + 2 * pad - K) // stride + 1
        OW = (W + 2 * pad - K) // stride + 1
        out = self.new_act(B, OH, OW, Cout, name)
        bias = conv.bias.data_ptr() if conv.bias is not None else None
        common = dict(dtype=self.dt, x=self._in(x_nchw), B=B, Cin=Cin, H=H, W=W, w=conv.weight.data_ptr(), K=K, stride=stride, pad=pad, bias=bias)
        if self.train:
            y = self.new_act(B, OH, OW, Cout, name + '.y')
            S = fill(STRUCTS['salt_conv_first_args'](), B=B, Cin=Cin, H=H, W=W, K=K, stride=stride, pad=pad)
            nparts = lib.salt_conv_first_stats_parts(ctypes.byref(S))
            # (the direct kernel knows the per-tile partials protocol only)
            w, _ = self._bn_behind(lambda **st: self.fwd.add('conv_first', y=y.view(), relu=0, **st, **common), False, nparts, y, bn, relu, None, out,
                                   self._scratch_sfx)

            def backward():
                self._bn_train_bwd(y, bn, relu, None, out, w)
                S2 = fill(STRUCTS['salt_conv_first_wgrad_args'](), B=B, Cin=Cin, H=H, W=W, K=K, stride=stride, pad=pad)
                np_ = lib.salt_conv_first_wgrad_parts(ctypes.byref(S2))
                self.bwd.add('conv_first_wgrad', stream=1, dtype=self.dt, x=self._in(x_nchw), B=B, Cin=Cin, H=H, W=W, K=K, stride=stride, pad=pad,
                             dy=y.gview(), partials=Scratch('wgrad', np_ * Cout * Cin * K * K * 4), nparts=np_,
                             grad=self._gp(conv.weight), accumulate=0)
            self.tape.append(backward)
        else:
            w = eng.bn_work(bn)
            self.fwd.add('conv_first', y=out.view(), scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(), relu=int(relu), **common)
        return out

    def _stem_s2d(self, x_nchw, conv, bn, relu, name):
        """ResNet stem (KxK stride 2 over <= 4 channels) on the matrix cores: 2x2 space-to-depth turns it into a
        ((K+1)/2)^2-tap stride-1 convolution over 16 channels, which the dense MFMA kernels run ~15x faster than the
        vector-ALU direct kernel; weights / weight-gradients are folded between the two forms by tiny kernels."""
        eng = self.engine
        B, Cin, H, W = x_nchw.shape
        Cout, _, K, _ = conv.weight.shape
        TT, half = (K + 1) // 2, (K + 1) // 4
        z = self.new_act(B, H // 2, W // 2, 16, name + '.s2d')
        self.fwd.add('s2d', dtype=self.dt, x=self._in(x_nchw), B=B, Cin=Cin, H=H, W=W, z=z.view())
        wp = eng.packs.stem(conv)
        taps = [(dh - half, dw - half) for dh in range(TT) for dw in range(TT)]
        OH, OW = H // 2, W // 2
        out = self.new_act(B, OH, OW, Cout, name)
        if self.train:
            y = self.new_act(B, OH, OW, Cout, name + '.y')
            w, _ = self._conv_bn_train(z, y, [(wp.data_ptr(), taps, 1, 0, OH, OW, {})], bn, relu, None, out, self._scratch_sfx)

            def backward():
                self._bn_train_bwd(y, bn, relu, None, out, w)
                g16 = self.f32(Cout * 16 * TT * TT)
                # dW'[t][n][c'] : P = dY (a = cout), Q = z (b = 16 s2d channels); reduce into [Cout][16][T][T], then unfold
                gw_tmp = g16.data_ptr()
                per = 8 if len(taps) > 9 else 9
                for i in range(0, len(taps), per):
                    chunk = list(range(i, min(i + per, len(taps))))
                    wg = dict(dtype=self.dt, ntaps=len(chunk), tap_dy=[taps[j][0] for j in chunk], tap_dx=[taps[j][1] for j in chunk], q_step=1, pad_mode=0)
                    ns = lib.salt_conv_wgrad_nsplit(ctypes.byref(fill(STRUCTS['salt_conv_wgrad_args'](), p=y.gview(), q=z.view(), **wg)))
                    nbytes = ns * len(chunk) * Cout * 16 * 4
                    # the stem is the last layer of backward: its weight gradient runs on the MAIN stream (own workspace), which is
                    # idle by then, instead of queueing behind the side stream's remaining weight gradients
                    self.bwd.add('conv_wgrad', stream=0, p=y.gview(), q=z.view(), partials=Scratch('wgrad@main', nbytes), nsplit=ns, **wg)
                    self.bwd.add('wgrad_reduce', stream=0, partials=Scratch('wgrad@main', nbytes), nsplit=ns, ntaps=len(chunk), Ca=Cout, Cb=16, KH=TT, KW=TT,
                                 tap_kh=[j // TT for j in chunk], tap_kw=[j % TT for j in chunk], grad=gw_tmp, accumulate=0)
                self.bwd.add('stem_grad_unfold', stream=0, g16=gw_tmp, Cout=Cout, Cin=Cin, K=K, grad=self._gp(conv.weight), accumulate=0)
            self.tape.append(backward)
        else:
            w = eng.bn_work(bn)
            self._conv_launch(self.fwd, z.view(), wp.data_ptr(), taps, 1, 0, out.view(), OH, OW,
                              scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(), relu=int(relu))
        return out

    # ------------------------------------------------------------------ second-level network (fp32 NCHW stack of probability maps)
    def stack_conv(self, x_nchw, conv, bn, relu=True, head=None, gate=None, logits=None, name='stack'):
        """Conv2dBnRelu(M, F, (3,3)) of the reference's StackingFCN (architectures/misc.py:13,28; base.py:21-37) straight from the fp32
        NCHW batch ``x_nchw`` [B,M,H,W] (salt_stack_conv, csrc/stacking.hip).
        eval: ONE launch that also applies the channel ``gate`` (a Graph.depth_gate record, or None) and the 1x1 ``head`` and writes the
        fp32 NCHW ``logits``; returns None.
        train: the raw output y, its per-tile BatchNorm partials and the NHWC copy xs of the input; returns relu(bn(y)) for
        Graph.channel_gate / Graph.head.  Backward: BatchNorm backward, then the weight gradient with P = dL/dy, Q = xs through the
        dense kernels (the padded input channels are dropped by salt_stack_grad_unfold); the input gets no gradient."""
        eng = self.engine
        B, M, H, W = x_nchw.shape
        F = conv.weight.shape[0]
        if tuple(conv.weight.shape) != (F, M, 3, 3) or bn is None:
            raise SaltError('stack_conv: weight %s does not fit the %d-map stack (a 3x3 Conv2dBnRelu is expected)' % (tuple(conv.weight.shape), M))
        nparts = stack_conv_parts(B, M, H, W, F)
        bias = conv.bias.data_ptr() if conv.bias is not None else None
        common = dict(dtype=self.dt, x=self._in(x_nchw), B=B, M=M, H=H, W=W, w=conv.weight.data_ptr(), bias=bias, F=F)
        if not self.train:
            if head is None or logits is None:
                raise SaltError('stack_conv: the eval form is the whole network - it needs the head and the logits buffer')
            K = head.weight.shape[0]
            if tuple(head.weight.shape) != (K, F, 1, 1) or tuple(logits.shape) != (B, K, H, W) or not 1 <= K <= 4:
                raise SaltError('stack_conv: head %s / logits %s do not fit (1x1, F = %d, at most 4 classes)' % (tuple(head.weight.shape), tuple(logits.shape), F))
            if gate is not None and (gate.C != F or gate.B != B):
                raise SaltError('stack_conv: a [%d, %d] gate on %d images x %d filters' % (gate.B, gate.C, B, F))
            w = eng.bn_work(bn)
            self.fwd.add('stack_conv', scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(), relu=int(relu),
                         gate=gate.s.data_ptr() if gate is not None else None, gate_cs=gate.C if gate is not None else 0,
                         head_w=head.weight.data_ptr(), head_b=head.bias.data_ptr() if head.bias is not None else None, K=K,
                         logits_nchw=logits.data_ptr(), **common)
            return None
        Mpad = _round_up(M, 16)
        y = self.new_act(B, H, W, F, name + '.y')
        xs = self.new_act(B, H, W, Mpad, name + '.xs')
        out = self.new_act(B, H, W, F, name)
        # (the kernel knows the per-tile partials protocol only, like conv_first)
        w, _ = self._bn_behind(lambda **st: self.fwd.add('stack_conv', y=y.view(), xs=xs.view(), **st, **common), False, nparts, y, bn, relu, None, out,
                               self._scratch_sfx)
        td = [(kh - 2, kw) for kh in range(3) for kw in range(3)]

        def backward():
            self._bn_train_bwd(y, bn, relu, None, out, w)
            gw = self._gp(conv.weight)
            gtmp = gw if Mpad == M else self.f32(F * Mpad * 9).data_ptr()
            wg = dict(dtype=self.dt, p=y.gview(), q=xs.view(), ntaps=9, tap_dy=[t[0] for t in td], tap_dx=[t[1] for t in td], q_step=1, pad_mode=1)
            ns = lib.salt_conv_wgrad_nsplit(ctypes.byref(fill(STRUCTS['salt_conv_wgrad_args'](), **wg)))
            if ns < 1:
                raise SaltError('stack_conv: weight-gradient plan failed: ' + lib.salt_last_error().decode())
            nbytes = ns * 9 * F * Mpad * 4
            # the last layer of backward: on the main stream with its own workspace, like the stem's (Graph._stem_s2d)
            self.bwd.add('conv_wgrad', stream=0, partials=Scratch('wgrad@main', nbytes), nsplit=ns, **wg)
            self.bwd.add('wgrad_reduce', stream=0, partials=Scratch('wgrad@main', nbytes), nsplit=ns, ntaps=9, Ca=F, Cb=Mpad, KH=3, KW=3,
                         tap_kh=[t // 3 for t in range(9)], tap_kw=[t % 3 for t in range(9)], grad=gtmp, accumulate=0)
            if Mpad != M:
                self.bwd.add('stack_grad_unfold', stream=0, gpad=gtmp, F=F, M=M, Mpad=Mpad, grad=gw, accumulate=0)
        self.tape.append(backward)
        return out

    # ------------------------------------------------------------------ grouped 3x3 convolution (csrc/conv_group.hip)
    def gconv(self, x, conv, bn, relu=True, out=None, name=''):
        """nn.Conv2d(C, C, 3, stride 1|2, padding 1, groups 32, bias=False) + BatchNorm2d (+ReLU): conv2 of SEResNeXtBottleneck
        (salt_gconv, from the fp32 master weight - nothing to pack or refresh).
        eval: ONE launch with the folded scale / shift.  train: the raw output with its statistics - the fp64 shards under consumer
        finalize (SALT_BN_FIN=2), per-tile partials + bn_finalize otherwise - and the usual affine_act behind it.
        Backward: BatchNorm backward, the weight gradient on the weight-gradient stream, the data gradient into x's gradient.  The data
        gradient offers no BatchNorm-backward carrier: the bn_bwd of the layer in front keeps its own reduction pass."""
        eng = self.engine
        C = x.C
        stride, groups = conv.stride[0], conv.groups
        if tuple(conv.weight.shape) != (C, C // max(groups, 1), 3, 3) or tuple(conv.padding) != (1, 1) or conv.stride[0] != conv.stride[1] \
                or conv.bias is not None or bn is None or bn.num_features != C:
            raise SaltError('gconv %s: weight %s, padding %s, stride %s on %d channels (a bias-free 3x3, padding 1, with BatchNorm is expected)'
                            % (name, tuple(conv.weight.shape), tuple(conv.padding), tuple(conv.stride), C))
        S = fill(STRUCTS['salt_gconv_args'](), dtype=self.dt, x=shaped_view(1, x.B, x.H, x.W, C), groups=groups, stride=stride)
        nparts = lib.salt_gconv_stats_parts(ctypes.byref(S))
        if nparts < 1:
            raise SaltError('gconv %s: %s' % (name, lib.salt_last_error().decode(errors='replace')))
        OH, OW = (x.H - 1) // stride + 1, (x.W - 1) // stride + 1
        if out is None:
            out = self.new_act(x.B, OH, OW, C, name)
        if (out.B, out.H, out.W, out.C) != (x.B, OH, OW, C):
            raise SaltError('gconv %s: output %s does not fit %s' % (name, (out.B, out.H, out.W, out.C), (x.B, OH, OW, C)))
        common = dict(dtype=self.dt, w=conv.weight.data_ptr(), groups=groups, stride=stride)
        if x.on_side and self.fwd.default_stream == 0:
            self.join()
        if not self.train:
            w = eng.bn_work(bn)
            self.fwd.add('gconv', x=x.view(), y=out.view(), scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(), relu=int(relu), **common)
            out.on_side = self.fwd.default_stream == 1
            return out
        y = self.new_act(x.B, OH, OW, C, name + '.y')
        w, _ = self._bn_behind(lambda **st: self.fwd.add('gconv', x=x.view(), y=y.view(), **st, **common), self._fin_mode() == 2, nparts, y, bn, relu,
                               None, out, self._scratch_sfx)
        out.on_side = self.fwd.default_stream == 1

        def backward():
            self._bn_train_bwd(y, bn, relu, None, out, w)
            wg = dict(dtype=self.dt, x=x.view(), dy=y.gview(), groups=groups, stride=stride)
            ns = lib.salt_gconv_wgrad_parts(ctypes.byref(fill(STRUCTS['salt_gconv_wgrad_args'](), **wg)))
            if ns < 1:
                raise SaltError('gconv %s: weight-gradient plan failed: %s' % (name, lib.salt_last_error().decode(errors='replace')))
            self.bwd.add('gconv_wgrad', stream=1, partials=Scratch('gconv_wgrad', ns * conv.weight.numel() * 4), nsplit=ns,
                         grad=self._gp(conv.weight), accumulate=0, **wg)
            acc = x.grad_state()
            self.bwd.add('gconv_dgrad', dy=y.gview(), dx=x.gview(), accumulate=acc, **common)
        self.tape.append(backward)
        return out

    # ------------------------------------------------------------------ DenseNet: pre-activated 1x1 convolution on a shared statistics table
    def dense_table(self, block, eps=1e-5):
        """The statistics table of a dense block (train mode): batch mean / invstd / unbiased variance of every channel of the
        concatenation buffer ``block``, filled once when the channels are produced (dense_table_fill) and read by every later layer's
        norm1 and by the transition's norm (saltnet.h: salt_dense_bn_prep)."""
        t = {k: self.f32(block.C) for k in ('mean', 'invstd', 'unb', 'rm', 'scale', 'shift', 'zeros', 'ones')}
        t['ones'].fill_(1.0)
        t['block'], t['eps'] = block, eps
        return t

    def dense_table_fill(self, table, c0, C, stats, cnt, nparts):
        """per-tile partials of channels [c0, c0 + C) of the block -> the table's rows: salt_bn_finalize with gamma 1, beta 0 and
        momentum 1 (running_var <- the unbiased variance itself)"""
        o = 4 * c0
        p = lambda k: table[k].data_ptr() + o
        self.fwd.add('bn_finalize', stats=stats, stats_cnt=cnt, nparts=nparts, C=C, gamma=p('ones'), beta=p('zeros'), running_mean=p('rm'),
                     running_var=p('unb'), num_batches_tracked=None, momentum=1.0, eps=table['eps'], mean=p('mean'), invstd=p('invstd'),
                     scale=p('scale'), shift=p('shift'))

    def dense_moments(self, x, table, c0):
        """train: the statistics of the STORED channels ``x`` = [c0, c0 + x.C) of the block (stem output / pooled transition output)"""
        S = fill(STRUCTS['salt_dense_moments_args'](), dtype=self.dt, x=shaped_view(1, x.B, x.H, x.W, x.C))
        nparts = lib.salt_dense_moments_parts(ctypes.byref(S))
        if nparts < 1:
            raise SaltError('dense_moments: %s' % lib.salt_last_error().decode(errors='replace'))
        stats = Scratch('stats' + self._scratch_sfx, 4 * lib.salt_bn_stats_floats(nparts, x.C))
        cnt = Scratch('stats_cnt' + self._scratch_sfx, nparts * 4)
        if x.on_side and self.fwd.default_stream == 0:
            self.join()
        self.fwd.add('dense_moments', dtype=self.dt, x=x.view(), stats=stats, stats_cnt=cnt)
        self.dense_table_fill(table, c0, x.C, stats, cnt, nparts)

    def dense_conv(self, x, bn_in, conv, bn_out=None, relu=None, out=None, table=None, name=''):
        """conv(relu(bn_in(x))) with a bias-free 1x1 ``conv``, optionally followed by bn_out (+ReLU): conv1 of a DenseNet layer (bn_out =
        norm2) or a transition (bn_out None).  ``x`` is a channel prefix of the block's concatenation buffer; relu(bn_in(x)) is never
        stored (salt_dense_conv, csrc/dense.hip, reads the fp32 master weight: nothing to pack or refresh).
        eval: ONE launch, bn_in folded into the loader transform, bn_out into the epilogue.
        train: ``table`` (dense_table) holds the batch statistics of x's channels; salt_dense_bn_prep derives this layer's in_scale /
        in_shift and updates ITS running statistics; the launch stores the raw output with per-tile statistics partials and the usual
        bn_finalize + affine_act follow (_bn_behind).  Backward: bn_out's backward, the weight gradient on the weight-gradient
        stream, and the data gradient with bn_in's backward inside (dgamma / dbeta of bn_in included) into x's gradient."""
        eng = self.engine
        Cout, Cin = conv.weight.shape[0], conv.weight.shape[1]
        relu = (bn_out is not None) if relu is None else relu
        if tuple(conv.weight.shape[2:]) != (1, 1) or conv.bias is not None or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (0, 0) \
                or Cin != x.C or bn_in.num_features != Cin or (bn_out is not None and bn_out.num_features != Cout):
            raise SaltError('dense_conv %s: weight %s on %d channels (a bias-free unit-step 1x1 behind a BatchNorm of its input is expected)'
                            % (name, tuple(conv.weight.shape), x.C))
        S = fill(STRUCTS['salt_dense_conv_args'](), dtype=self.dt, x=shaped_view(1, x.B, x.H, x.W, Cin), y=shaped_view(1, x.B, x.H, x.W, Cout))
        nparts = lib.salt_dense_conv_stats_parts(ctypes.byref(S))
        if nparts < 1:
            raise SaltError('dense_conv %s: %s' % (name, lib.salt_last_error().decode(errors='replace')))
        if out is None:
            out = self.new_act(x.B, x.H, x.W, Cout, name)
        if (out.B, out.H, out.W, out.C) != (x.B, x.H, x.W, Cout):
            raise SaltError('dense_conv %s: output %s does not fit %s' % (name, (out.B, out.H, out.W, out.C), (x.B, x.H, x.W, Cout)))
        w1 = eng.bn_work(bn_in)
        tr = dict(in_scale=w1['scale'].data_ptr(), in_shift=w1['shift'].data_ptr())
        # the kernels read these vectors 16 bytes at a time.  Engine._flatten starts every live parameter on a multiple of 4 floats of the
        # flat buffer and the work vectors are allocations of their own, so this holds by construction; a parameter that is not in the
        # flat buffer (a dead or frozen one) need not be - refuse it here, not at run time
        for what, t in (('conv.weight', conv.weight), ('bn_in.weight', bn_in.weight), ('bn_in.bias', bn_in.bias)):
            if t.data_ptr() % 16:
                raise SaltError('dense_conv %s: %s is not 16-byte aligned' % (name, what))
        common = dict(dtype=self.dt, w=conv.weight.data_ptr(), **tr)
        if x.on_side and self.fwd.default_stream == 0:
            self.join()
        if not self.train:
            ep = {}
            if bn_out is not None:
                w2 = eng.bn_work(bn_out)
                ep = dict(scale=w2['scale'].data_ptr(), shift=w2['shift'].data_ptr())
            self.fwd.add('dense_conv', x=x.view(), y=out.view(), relu=int(relu), **ep, **common)
            out.on_side = self.fwd.default_stream == 1
            return out
        if table is None or x.buf is not table['block'].buf or x.c0 != table['block'].c0 or x.C > table['block'].C:
            raise SaltError('dense_conv %s: train mode needs the statistics table of the block x is a prefix of' % name)
        if bn_in.eps != table['eps']:
            raise SaltError('dense_conv %s: BatchNorm eps %g, the block statistics table was built with %g' % (name, bn_in.eps, table['eps']))
        if bn_in.momentum is None:
            raise SaltError('dense_conv %s: momentum=None (cumulative averaging) is not built' % name)
        if bn_out is None and relu:
            raise SaltError('dense_conv %s: a ReLU without a BatchNorm behind the convolution is not on the reference path' % name)
        nbt = bn_in.num_batches_tracked.data_ptr() if bn_in.num_batches_tracked is not None else None
        self.fwd.add('dense_bn_prep', C=Cin, mean=table['mean'].data_ptr(), invstd=table['invstd'].data_ptr(), unbiased_var=table['unb'].data_ptr(),
                     gamma=bn_in.weight.data_ptr(), beta=bn_in.bias.data_ptr(), running_mean=bn_in.running_mean.data_ptr(),
                     running_var=bn_in.running_var.data_ptr(), num_batches_tracked=nbt, momentum=bn_in.momentum, **tr)
        w2 = None
        if bn_out is not None:
            y = self.new_act(x.B, x.H, x.W, Cout, name + '.y')
            # (the kernel knows the per-tile partials protocol only)
            w2, _ = self._bn_behind(lambda **st: self.fwd.add('dense_conv', x=x.view(), y=y.view(), **st, **common), False, nparts, y, bn_out, relu,
                                    None, out, self._scratch_sfx)
        else:
            y = out
            self.fwd.add('dense_conv', x=x.view(), y=out.view(), relu=0, **common)
        out.on_side = self.fwd.default_stream == 1

        def backward():
            if bn_out is not None:
                self._bn_train_bwd(y, bn_out, relu, None, out, w2)
            wg = dict(dtype=self.dt, x=x.view(), dy=y.gview(), **tr)
            ns = lib.salt_dense_conv_wgrad_parts(ctypes.byref(fill(STRUCTS['salt_dense_conv_wgrad_args'](), **wg)))
            if ns < 1:
                raise SaltError('dense_conv %s: weight-gradient plan failed: %s' % (name, lib.salt_last_error().decode(errors='replace')))
            self.bwd.add('dense_conv_wgrad', stream=1, partials=Scratch('dense_wgrad', ns * Cout * Cin * 4), nsplit=ns, grad=self._gp(conv.weight),
                         accumulate=0, **wg)
            acc = x.grad_state()
            # g is recomputed by the apply pass, not stashed: the only workspaces are the per-tile sums, shared by every layer
            self.bwd.add('dense_conv_dgrad', dy=y.gview(), x=x.view(), mean=table['mean'].data_ptr(), invstd=table['invstd'].data_ptr(),
                         gamma=bn_in.weight.data_ptr(), partials=Scratch('dense_dgrad', nparts * 2 * Cin * 4), nparts=nparts,
                         sums=Scratch('dense_sums', 2 * Cin * 4), dgamma=self._gp(bn_in.weight), dbeta=self._gp(bn_in.bias), accumulate_param_grads=0,
                         dx=x.gview(), accumulate=acc, **common)
        self.tape.append(backward)
        return out

    # ------------------------------------------------------------------ PSPNet: pyramid pooling at low resolution (csrc/psp.hip)
    def _conv1x1_slice(self, x, conv, c0, name=''):
        """y = W[:, c0 : c0 + x.C] x for the 1x1 convolution ``conv`` (no bias: the merge adds it once) - one block of input channels of
        a weight whose other blocks meet other tensors.  Backward: that block of conv.weight.grad and the data gradient into dL/dx."""
        Cout, D1, KH, KW = conv.weight.shape
        d1, one = (c0, x.C), [(0, 0)]
        y = self.new_act(x.B, x.H, x.W, Cout, name)
        self._conv_launch(self.fwd, x.view(), self.engine.packs.dense(conv, one, transposed=False, d1=d1).data_ptr(), one, 1, 0, y.view(), x.H, x.W)
        if self.train:
            def backward():
                if not y.grad_ready():
                    raise SaltError('%s: dL/dy was never written (psp_merge must consume it)' % name)
                self._wgrad(y.gview(), x.view(), one, one, 1, 0, conv.weight, KH, KW, b_slice=(c0, D1))
                self._dgrad(conv, x, y, [(0, 0, 0, 0)], 1, False, KH, KW, d1=d1)
            self.tape.append(backward)
        return y

    def psp(self, x, module, name='psp'):
        """PSPModule (architectures/pspnet.py:9-28) without its 5 C-wide concatenation: a 1x1 convolution commutes with the bilinear
        resize, so every pyramid stage meets its block of ``bottleneck.weight`` at s x s bins and the merge adds the resized results to
        the block that x meets at h x w (saltnet.h: salt_psp_pool / salt_psp_merge).  Forward: pool, the stage convolutions, one slice
        convolution per stage and one for x, merge.  Backward, in reverse: salt_psp_merge_bwd (dL/df, every dL/dq, the bottleneck's bias
        gradient), the slice convolutions (their blocks of bottleneck.weight.grad; dL/dx from the x block), the stage convolutions, and
        salt_psp_pool_bwd, which adds to dL/dx."""
        sizes = [int(st[0].output_size[0] if isinstance(st[0].output_size, (tuple, list)) else st[0].output_size) for st in module.stages]
        bott, n, C = module.bottleneck, len(module.stages), x.C
        Cout = bott.weight.shape[0]
        if tuple(bott.weight.shape) != (Cout, (n + 1) * C, 1, 1) or any(tuple(st[1].weight.shape) != (C, C, 1, 1) or st[1].bias is not None for st in module.stages):
            raise SaltError('psp %s: bottleneck %s over %d stages of %d channels (bias-free 1x1 stage convolutions are expected)'
                            % (name, tuple(bott.weight.shape), n, C))
        if not 1 <= n <= 4 or any(not 1 <= s <= 6 for s in sizes) or x.H > 32 or x.W > 32 or C % 8 or Cout % 8:
            raise SaltError('psp %s: sizes %s on a %dx%d map, %d -> %d channels (salt_psp_pool: up to 4 sizes in 1..6, at most 32x32 pixels, '
                            'channels in multiples of 8)' % (name, sizes, x.H, x.W, C, Cout))
        if x.on_side and self.fwd.default_stream == 0:
            self.join()
        ac = int(bool(getattr(getattr(self.engine, 'module', None), 'align_corners', False)))
        # A 1 x 1 stage is stored as ONE image of B pixels, [1,1,B,C] - the same memory as [B,1,1,C]: salt_conv's tile arithmetic divides by
        # the pixels of a tile's image through a 32-bit reciprocal that does not exist for 1, and sends every image of a batch of 1 x 1 maps
        # to image 0.  The convolutions here are 1x1, so which pixels form an image is theirs to ignore; the psp operators get the per-image view.
        dims = lambda s: (1, 1, x.B) if s == 1 else (x.B, s, s)

        def per_image(v, s):
            v.B, v.H, v.W = x.B, s, s
            return v
        ps = [self.new_act(*dims(s), C, '%s.pool%d' % (name, s)) for s in sizes]
        self.fwd.add('psp_pool', dtype=self.dt, x=x.view(), nsizes=n, sizes=sizes, p=[per_image(p.view(), s) for p, s in zip(ps, sizes)])
        if self.train:
            def pool_backward():
                acc = x.grad_state()
                self.bwd.add('psp_pool_bwd', dtype=self.dt, nsizes=n, sizes=sizes, dp=[per_image(p.gview(), s) for p, s in zip(ps, sizes)], dx=x.gview(),
                             accumulate=acc)
            self.tape.append(pool_backward)
        ts = [self.conv(p, st[1], name='%s.stage%d' % (name, s)) for p, st, s in zip(ps, module.stages, sizes)]
        qs = [self._conv1x1_slice(t, bott, k * C, name='%s.q%d' % (name, s)) for k, (t, s) in enumerate(zip(ts, sizes))]
        f = self._conv1x1_slice(x, bott, n * C, name=name + '.f')
        out = self.new_act(x.B, x.H, x.W, Cout, name)
        bias = bott.bias.data_ptr() if bott.bias is not None else None
        self.fwd.add('psp_merge', dtype=self.dt, f=f.view(), bias=bias, nsizes=n, sizes=sizes, q=[per_image(q.view(), s) for q, s in zip(qs, sizes)],
                     align_corners=ac, y=out.view())
        if self.train:
            def merge_backward():
                for t in [f] + qs:
                    assert t.grad_state() == 0, 'a slice convolution output has a single consumer'
                self.bwd.add('psp_merge_bwd', dtype=self.dt, dy=out.gview(), y=out.view(), nsizes=n, sizes=sizes, align_corners=ac, df=f.gview(),
                             dq=[per_image(q.gview(), s) for q, s in zip(qs, sizes)], partials=Scratch('psp_dbias', x.B * Cout * 4), nparts=x.B,
                             dbias=self._gp(bott.bias) if bott.bias is not None else None, accumulate_dbias=0)
            self.tape.append(merge_backward)
        return out

    def conv_bn_prelu(self, x, conv, bn, prelu, out=None, name=''):
        """nn.Conv2d(3x3, padding 1, bias) -> BatchNorm2d -> nn.PReLU() with one slope (PSPUpsample.conv, architectures/pspnet.py:31-38).
        eval: the convolution with the folded BatchNorm in its epilogue, then the plain PReLU in place (salt_bn_prelu without scale /
        shift).  train: the raw output with per-tile statistics partials, salt_bn_finalize, and BatchNorm apply + PReLU in one pass
        (the normalised value is never stored).  Backward: salt_bn_prelu_bwd turns dL/da into dL/du in place and reduces dL/dalpha,
        then the usual BatchNorm backward (no ReLU), weight gradient and data gradient.  The convolution's bias is treated as Graph.conv
        treats it in front of a train-mode BatchNorm."""
        eng = self.engine
        Cout, Cin, KH, KW = conv.weight.shape
        if Cin != x.C or tuple(conv.stride) != (1, 1) or bn is None or bn.num_features != Cout or prelu.weight.numel() != 1 or Cout % 8:
            raise SaltError('conv_bn_prelu %s: weight %s on %d channels, PReLU with %d slopes (a unit-step convolution to a multiple of 8 channels, '
                            'a BatchNorm and ONE slope are expected)' % (name, tuple(conv.weight.shape), x.C, prelu.weight.numel()))
        py, px = conv.padding
        taps = conv_taps(KH, KW, py, px)
        tk, td = [(t[0], t[1]) for t in taps], [(t[2], t[3]) for t in taps]
        OH, OW = x.H + 2 * py - KH + 1, x.W + 2 * px - KW + 1
        pk = eng.packs.dense(conv, tk, transposed=False)
        bias = conv.bias.data_ptr() if conv.bias is not None else None
        alpha = prelu.weight.data_ptr()
        if out is None:
            out = self.new_act(x.B, OH, OW, Cout, name)
        if (out.B, out.H, out.W, out.C) != (x.B, OH, OW, Cout):
            raise SaltError('conv_bn_prelu %s: output %s does not fit %s' % (name, (out.B, out.H, out.W, out.C), (x.B, OH, OW, Cout)))
        if x.on_side and self.fwd.default_stream == 0:
            self.join()
        if not self.train:
            w = eng.bn_work(bn)
            self._conv_launch(self.fwd, x.view(), pk.data_ptr(), td, 1, 0, out.view(), OH, OW, bias=bias, scale=w['scale'].data_ptr(),
                              shift=w['shift'].data_ptr(), relu=0)
            self.fwd.add('bn_prelu', dtype=self.dt, y=out.view(), scale=None, shift=None, alpha=alpha, a=out.view())
            return out
        y = self.new_act(x.B, OH, OW, Cout, name + '.y')
        nparts = self._conv_parts(x.view(), td, 1, y.view(), OH, OW)
        stats = Scratch('stats' + self._scratch_sfx, 4 * lib.salt_bn_stats_floats(nparts, Cout))
        cnt = Scratch('stats_cnt' + self._scratch_sfx, nparts * 4)
        self._conv_launch(self.fwd, x.view(), pk.data_ptr(), td, 1, 0, y.view(), OH, OW, bias=bias, stats=stats, stats_cnt=cnt)
        w, fin = self._bn_fin_fields(bn)
        self.fwd.add('bn_finalize', stats=stats, stats_cnt=cnt, nparts=nparts, **fin)
        affine = dict(scale=w['scale'].data_ptr(), shift=w['shift'].data_ptr(), alpha=alpha)
        self.fwd.add('bn_prelu', dtype=self.dt, y=y.view(), a=out.view(), **affine)

        def backward():
            if not out.grad_ready():
                raise SaltError('conv_bn_prelu %s: dL/d(out) was never written' % name)
            S = fill(STRUCTS['salt_bn_prelu_bwd_args'](), dtype=self.dt, y=y.view())
            np_ = lib.salt_bn_prelu_bwd_parts(ctypes.byref(S))
            if np_ < 1:
                raise SaltError('conv_bn_prelu %s: %s' % (name, lib.salt_last_error().decode(errors='replace')))
            self.bwd.add('bn_prelu_bwd', dtype=self.dt, da=out.gview(), y=y.view(), du=out.gview(), partials=Scratch('prelu', np_ * 4), nparts=np_,
                         dalpha=self._gp(prelu.weight), accumulate_dalpha=0, **affine)
            # this operator completed dL/du in place: it is the slice's last gradient writer and carries nobody's sums, so the
            # BatchNorm backward below keeps its own reduction pass (a data-gradient launch in front of it summed dL/da, not dL/du)
            out.buf.grad_writers.append(GradWriter(out.c0, out.C))
            self._bn_train_bwd(y, bn, False, None, out, w)
            self._wgrad(y.gview(), x.view(), td, tk, 1, 0, conv.weight, KH, KW)
            self._dgrad(conv, x, y, taps, 1, False, KH, KW)
        self.tape.append(backward)
        return out

    # ------------------------------------------------------------------ GlobalConvolutionalNetwork entry: the paired line convolution (csrc/gcn.hip)
    @staticmethod
    def gcn_pair_composed(x, K):
        """The ONE shape rule of Graph.gcn_pair: True where the pair measured slower than two Graph.conv launches by more than the
        run-to-run spread of the same table (profiles/lkm_bench.json); those shapes take the composed route.  As measured
        that is EVERY shape of the table: a GCN block with the pair ran 5 .. 51 % slower forward + backward than the composed one at all
        nine shapes ([32,64,64,64] .. [32,2048,8,8] and [2,64,32,32] .. [2,512,4,4], 16 K to 8 M elements of x, spread under 2 %), and
        nothing in between or beyond was measured faster.  So the rule is True for every shape today: the pair runs only where a caller
        asks for it (``force``), until one of the causes listed in DESIGN 21 is removed and the table says otherwise.  tests/test_lkm_cpu.py
        holds this function to the table in both directions."""
        return True

    def gcn_pair(self, x, conv_v, bn_v, conv_h, bn_h, relu, name='gcn', force=False):
        """conv1[0] (K x 1) and conv2[0] (1 x K) of a GlobalConvolutionalNetwork (architectures/base.py:152-178), each a Conv2dBnRelu with
        the reference's one-sided replicate pad, on the SAME input x -> (a_v, a_h) (saltnet.h: salt_gcn_pair / salt_gcn_pair_dgrad).
        eval: ONE launch with both folded epilogues.  train: ONE launch with the raw outputs and their per-tile statistics partials, then
        per branch bn_finalize + affine_act (the per-tile protocol in every SALT_BN_FIN mode).  Backward: the two BatchNorm backwards, the
        two weight gradients on the existing path (P = dL/dy, Q = x, K taps each) and ONE data-gradient launch that stores dL/dx once.
        The convolution biases are treated as Graph.conv treats them in front of a train-mode BatchNorm.
        Where gcn_pair_composed says so the two convolutions run as two Graph.conv launches instead; ``force`` takes the pair regardless (tests,
        tools/lkm_bench.py)."""
        eng = self.engine
        Cout, Cin, K, one = conv_v.weight.shape
        if (one != 1 or tuple(conv_h.weight.shape) != (Cout, Cin, 1, K) or Cin != x.C or bn_v is None or bn_h is None
                or bn_v.num_features != Cout or bn_h.num_features != Cout or tuple(conv_v.stride) != (1, 1) or tuple(conv_h.stride) != (1, 1)):
            raise SaltError('gcn_pair %s: weights %s / %s on %d channels (a K x 1 and a 1 x K unit-step convolution of the same widths, each with a '
                            'BatchNorm, are expected)' % (name, tuple(conv_v.weight.shape), tuple(conv_h.weight.shape), x.C))
        if not force and self.gcn_pair_composed(x, K):
            return (self.conv(x, conv_v, bn_v, relu=relu, replicate=True, name=name + '.v'),
                    self.conv(x, conv_h, bn_h, relu=relu, replicate=True, name=name + '.h'))
        av, ah = self.new_act(x.B, x.H, x.W, Cout, name + '.v'), self.new_act(x.B, x.H, x.W, Cout, name + '.h')
        probe = fill(STRUCTS['salt_gcn_pair_args'](), dtype=self.dt, x=x._view(x.buf.t), K=K, yv=av._view(av.buf.t), yh=ah._view(ah.buf.t))
        nparts = lib.salt_gcn_pair_stats_parts(ctypes.byref(probe))
        if nparts < 1:
            raise SaltError('gcn_pair %s: %s' % (name, lib.salt_last_error().decode(errors='replace')))
        if x.on_side and self.fwd.default_stream == 0:
            self.join()
        bias = lambda c: c.bias.data_ptr() if c.bias is not None else None
        common = dict(dtype=self.dt, wv=conv_v.weight.data_ptr(), wh=conv_h.weight.data_ptr(), K=K)
        if not self.train:
            wv, wh = eng.bn_work(bn_v), eng.bn_work(bn_h)
            self.fwd.add('gcn_pair', x=x.view(), yv=av.view(), yh=ah.view(), bias_v=bias(conv_v), scale_v=wv['scale'].data_ptr(),
                         shift_v=wv['shift'].data_ptr(), relu_v=int(relu), bias_h=bias(conv_h), scale_h=wh['scale'].data_ptr(),
                         shift_h=wh['shift'].data_ptr(), relu_h=int(relu), **common)
            av.on_side = ah.on_side = self.fwd.default_stream == 1
            return av, ah
        yv, yh = self.new_act(x.B, x.H, x.W, Cout, name + '.v.y'), self.new_act(x.B, x.H, x.W, Cout, name + '.h.y')
        prod = []

        def launch_v(stats, stats_cnt):
            prod.append(self.fwd.add('gcn_pair', x=x.view(), yv=yv.view(), yh=yh.view(), bias_v=bias(conv_v), bias_h=bias(conv_h), stats_v=stats,
                                     stats_cnt_v=stats_cnt, **common))
            return prod[0]

        def launch_h(stats, stats_cnt):                  # the same launch: it fills the second branch's workspaces too
            self.fwd.set_fields(prod[0], stats_h=stats, stats_cnt_h=stats_cnt)
            return prod[0]
        w_v, _ = self._bn_behind(launch_v, False, nparts, yv, bn_v, relu, None, av, self._scratch_sfx + '.gcn_v')
        w_h, _ = self._bn_behind(launch_h, False, nparts, yh, bn_h, relu, None, ah, self._scratch_sfx + '.gcn_h')
        av.on_side = ah.on_side = self.fwd.default_stream == 1

        def backward():
            self._bn_train_bwd(yv, bn_v, relu, None, av, w_v)
            self._bn_train_bwd(yh, bn_h, relu, None, ah, w_h)
            self._wgrad(yv.gview(), x.view(), [(k - (K - 1), 0) for k in range(K)], [(k, 0) for k in range(K)], 1, 1, conv_v.weight, K, 1)
            self._wgrad(yh.gview(), x.view(), [(0, k) for k in range(K)], [(0, k) for k in range(K)], 1, 1, conv_h.weight, 1, K)
            if x.buf.name != '__input__':
                acc = x.grad_state()
                self.bwd.add('gcn_pair_dgrad', dyv=yv.gview(), dyh=yh.gview(), dx=x.gview(), accumulate=acc, **common)
        self.tape.append(backward)
        return av, ah

    # ------------------------------------------------------------------ logit head: 1x1 conv to <= 4 channels, fp32 NCHW out
    def head(self, x, conv, logits_nchw):
        Cout = conv.weight.shape[0]
        # round 6: x = relu(bn(y)) stored by the last forward operator and read by nobody else (the `final` Sequential of every U-Net here:
        # unet_models.py:131-138, architectures/unet.py:84-87) - BatchNorm apply + ReLU + head in one pass over y (salt_head_bn), the
        # activation and its gradient are never stored; the producer layer's _bn_train_bwd emits salt_head_bn_bwd instead of salt_bn_bwd
        taken = self._take_act_op(x) if self.head_bn_ok(x.C, conv) else None
        if taken is not None:
            sa, Fbn = taken
            hb = self.fwd.add('head_bn', dtype=self.dt, y=sa.y, fin=ctypes.addressof(Fbn), relu=int(sa.relu), w=conv.weight.data_ptr(),
                              bias=conv.bias.data_ptr() if conv.bias is not None else None, Cout=Cout, y_nchw=logits_nchw.data_ptr())
            self._retarget_fin_acc(sa, hb, 'fin_acc')
            self.dlogits = self.alloc(tuple(logits_nchw.shape), torch.float32)
            x.buf.head_fused = conv
            self.tape.append(lambda: None)               # the head's backward is part of the producer layer's closure (Graph._bn_train_bwd)
            return
        self.fwd.add('head1x1', dtype=self.dt, x=x.view(), w=conv.weight.data_ptr(), bias=conv.bias.data_ptr() if conv.bias is not None else None,
                     Cout=Cout, y_nchw=logits_nchw.data_ptr(), y=null_view())
        if self.train:
            self.dlogits = self.alloc(tuple(logits_nchw.shape), torch.float32)

            def backward():
                nparts = lib.salt_head1x1_bwd_parts(ctypes.byref(fill(STRUCTS['salt_head1x1_bwd_args'](), x=x.view())))
                acc = x.grad_state()
                self.bwd.add('head1x1_bwd', dtype=self.dt, x=x.view(), w=conv.weight.data_ptr(), Cout=Cout, dy_nchw=self.dlogits.data_ptr(),
                             dx=x.gview(), accumulate=acc, partials=Scratch('head', nparts * Cout * (x.C + 1) * 4), nparts=nparts,
                             gw=self._gp(conv.weight), gb=self._gp(conv.bias) if conv.bias is not None else None)
            self.tape.append(backward)

    # ------------------------------------------------------------------ classifier head: AvgPool2d(8) + 1x1 conv to <= 8 logits, fp32 NCHW out
    def pool_head(self, x, conv, logits_nchw, k=8):
        """nn.Sequential(nn.AvgPool2d(k), nn.Conv2d(C, K, 1)) (architectures/misc.py:70-71) in one launch; training keeps the pooled
        fp32 vector so that the backward launch never reads ``x`` again."""
        if k != 8:
            raise SaltError('pool_head: only the 8x8 window of the reference (nn.AvgPool2d(8)) is built, got %r' % (k,))
        K = conv.weight.shape[0]
        if tuple(conv.weight.shape[1:]) != (x.C, 1, 1) or tuple(logits_nchw.shape) != (x.B, K, x.H // k, x.W // k):
            raise SaltError('pool_head: weight %s / logits %s do not fit the %dx%dx%d map' % (tuple(conv.weight.shape), tuple(logits_nchw.shape), x.H, x.W, x.C))
        pooled = self.alloc((x.B, x.H // k, x.W // k, x.C), torch.float32) if self.train else None
        self.fwd.add('pool_head', dtype=self.dt, x=x.view(), w=conv.weight.data_ptr(), bias=conv.bias.data_ptr() if conv.bias is not None else None,
                     K=K, logits_nchw=logits_nchw.data_ptr(), pooled=pooled.data_ptr() if pooled is not None else None)
        if self.train:
            self.dlogits = self.alloc(tuple(logits_nchw.shape), torch.float32)

            def backward():
                acc = x.grad_state()
                self.bwd.add('pool_head_bwd', dtype=self.dt, dx=x.gview(), w=conv.weight.data_ptr(), K=K, dlogits_nchw=self.dlogits.data_ptr(),
                             pooled=pooled.data_ptr(), accumulate=acc, gw=self._gp(conv.weight), gb=self._gp(conv.bias) if conv.bias is not None else None)
            self.tape.append(backward)

    # ------------------------------------------------------------------ layout boundary (fp32 NCHW <-> NHWC activations)
    def from_nchw(self, x_nchw, name='input'):
        B, C, H, W = x_nchw.shape
        a = self.new_act(B, H, W, C, name)
        self.fwd.add('layout', dtype=self.dt, nchw=self._in(x_nchw), nhwc=a.view(), to_nhwc=1)
        if self.train:
            dx = self.alloc((B, C, H, W), torch.float32)
            self.input_grads.append(dx)

            def backward():
                if a.grad_ready():
                    self.bwd.add('layout', dtype=self.dt, nchw=dx.data_ptr(), nhwc=a.gview(), to_nhwc=0)
            self.tape.append(backward)
        return a

    def to_nchw(self, a, out_nchw):
        self.fwd.add('layout', dtype=self.dt, nchw=out_nchw.data_ptr(), nhwc=a.view(), to_nhwc=0)
        if self.train:
            self.dlogits = self.alloc(tuple(out_nchw.shape), torch.float32)

            def backward():
                assert a.grad_state() == 0
                self.bwd.add('layout', dtype=self.dt, nchw=self.dlogits.data_ptr(), nhwc=a.gview(), to_nhwc=1)
            self.tape.append(backward)

    # ------------------------------------------------------------------ pooling / resize
    def _maxpool(self, op, x, out):
        self.fwd.add(op, dtype=self.dt, x=x.view(), y=out.view())
        if self.train:
            def backward():
                acc = x.grad_state()
                self.bwd.add(op + '_bwd', dtype=self.dt, x=x.view(), dy=out.gview(), dx=x.gview(), accumulate=acc)
            self.tape.append(backward)
        return out

    def maxpool2(self, x, out=None, name=''):
        return self._maxpool('maxpool2', x, self.new_act(x.B, x.H // 2, x.W // 2, x.C, name) if out is None else out)

    def maxpool3s2(self, x, out=None, name=''):
        """nn.MaxPool2d(3, 2, 1) - the ResNet stem pool of ResNetEncoders(pool0=True) (architectures/encoders.py:23-27)."""
        return self._maxpool('maxpool3s2', x, self.new_act(x.B, (x.H + 1) // 2, (x.W + 1) // 2, x.C, name) if out is None else out)

    def avgpool2(self, x, out=None, name=''):
        if out is None:
            out = self.new_act(x.B, x.H // 2, x.W // 2, x.C, name)
        self.fwd.add('avgpool2', dtype=self.dt, x=x.view(), y=out.view(), backward=0, accumulate=0)
        if self.train:
            def backward():
                acc = x.grad_state()
                self.bwd.add('avgpool2', dtype=self.dt, x=x.gview(), y=out.gview(), backward=1, accumulate=acc)
            self.tape.append(backward)
        return out

    def upsample(self, x, R, out=None, name=''):
        if out is None:
            out = self.new_act(x.B, x.H * R, x.W * R, x.C, name)
        ac = int(bool(getattr(getattr(self.engine, 'module', None), 'align_corners', False)))      # HipNetwork.set_align_corners
        self.fwd.add('bilinear', dtype=self.dt, x=x.view(), y=out.view(), R=R, backward=0, accumulate=0, align_corners=ac)
        if self.train:
            def backward():
                acc = x.grad_state()
                tmp = Scratch('bilinear', x.B * out.H * x.W * _round_up(x.C, self.ve) * self._es()) if R >= 4 else None
                self.bwd.add('bilinear', dtype=self.dt, x=x.gview(), y=out.gview(), R=R, backward=1, accumulate=acc, tmp=tmp, align_corners=ac)
            self.tape.append(backward)
        return out

    def add(self, a, b, out=None, name=''):
        """out = a + b; ``b`` None: out = a (Graph.copy)"""
        if out is None:
            out = self.new_act(a.B, a.H, a.W, a.C, name)
        self.fwd.add('add', dtype=self.dt, a=a.view(), b=b.view() if b is not None else null_view(), y=out.view(), accumulate=0)
        if self.train:
            def backward():
                for t in (a, b) if b is not None else (a,):
                    acc = t.grad_state()
                    self.bwd.add('add', dtype=self.dt, a=out.gview(), b=null_view(), y=t.gview(), accumulate=acc)
            self.tape.append(backward)
        return out

    def copy(self, a, out):
        return self.add(a, None, out)

    def _take_act_op(self, x):
        """x = relu?(bn(y)) written by the LAST forward operator (a consumer-side-finalize salt_affine_act without residual, main stream)
        and read by nobody yet: remove that operator from the program and hand back (its argument struct, the layer's
        salt_bn_finalize_args) - the caller's kernels apply the transform to y themselves.  Graph.finalize fails loudly if anybody asks
        for a storage view of the activation afterwards."""
        rec = x.buf.act_op
        if rec is None or not self.fwd.ops or self.fwd.ops[-1][0] != 'affine_act':
            return None
        sa, reads0, c0, C = rec
        if (self.fwd.ops[-1][2] is not sa or (c0, C) != (x.c0, x.C) or x.c0 != 0 or x.C != x.buf.C or x.buf.reads != reads0 or not sa.fin or sa.res.p
                or self.fwd.streams[-1] != 0 or x.buf.planes):
            return None
        self.fwd.ops.pop(); self.fwd.streams.pop()
        self.fwd._entries = None
        x.buf.act_op = None
        self._virtual_acts.append((x.buf, x.buf.reads))
        return sa, STRUCTS['salt_bn_finalize_args'].from_address(sa.fin)

    def _retarget_fin_acc(self, sa, st, field):
        """The statistics shards the taken-over affine_act ``sa`` would have finalized go to ``st.field`` instead."""
        self._fin_patches = [(st, field, q[2], q[3]) if (q[0] is sa and q[1] == 'fin_acc') else q for q in self._fin_patches]

    # ------------------------------------------------------------------ scSE
    def scse(self, x, cse, sse, out=None, name=''):
        """relu(x*cSE(x) + x*sSE(x)); cse.fc = Sequential(Linear, ReLU, Linear, Sigmoid), sse.fc = Conv2d(C,1,1)."""
        eng = self.engine
        if out is None:
            out = self.new_act(x.B, x.H, x.W, x.C, name)
        l1, l2, cs = cse.fc[0], cse.fc[2], sse.fc
        R, C, B = l1.weight.shape[0], x.C, x.B
        shards = self.train and self._fin_mode() == 2 and switches.get('SALT_SE_SHARDS')   # per-image sums through the zeroed fp64 arena (see _fin_slot)
        # round 6: x = relu(bn(conv)) whose ONLY reader is this operator (base.DecoderBlock: conv2 -> scSE, architectures/base.py:60-85) -
        # the affine_act that would store it is taken back out of the program and the scSE kernels apply BatchNorm + ReLU to the raw
        # convolution output on the way in (salt_scse_args.in_fin); backward reads the raw output through the same transform
        taken = self._take_act_op(x) if (shards and switches.get('SALT_SE_IN_BN')) else None
        if taken is not None:
            sa, Fbn = taken
            xv_ = sa.y                                   # the raw convolution output; never x.view(): the activation has no storage reader
            in_kw = dict(in_fin=ctypes.addressof(Fbn), in_relu=int(sa.relu))
            in_bwd = dict(in_scale=Fbn.scale, in_shift=Fbn.shift, in_relu=int(sa.relu))
        else:
            xv_, in_kw, in_bwd = None, {}, {}
        xview = (lambda: xv_) if taken is not None else x.view
        nparts = lib.salt_scse_parts(ctypes.byref(fill(STRUCTS['salt_scse_args'](), x=xview())))
        gap, hid, gc, gs = self.f32(B * C), self.f32(B * R), self.f32(B * C), self.f32(B * x.H * x.W)
        sf = self.fwd.add('scse', dtype=self.dt, x=xview(), w1=l1.weight.data_ptr(), b1=l1.bias.data_ptr(), w2=l2.weight.data_ptr(),
                          b2=l2.bias.data_ptr(), R=R, ws=cs.weight.data_ptr(), bs=cs.bias.data_ptr(), gap_partials=Scratch('se', B * nparts * (2 * C + 1) * 4),
                          nparts=nparts, gap=gap.data_ptr(), hidden=hid.data_ptr(), gate_c=gc.data_ptr(), gate_s=gs.data_ptr(), y=out.view(), **in_kw)
        if taken is not None:
            self._retarget_fin_acc(sa, sf, 'in_fin_acc')
        if shards:
            self._fin_slot('fwd', B * C, (sf, 'gap_acc'))
        if self.train:
            def backward():
                acc = x.grad_state()
                dgap = self.f32(B * C)
                gp = self._gp
                # round 6: the FC parameter gradients (one workgroup over the whole batch: 18 - 24 us) are nobody's input before the optimizer -
                # they run as their own operator on the weight-gradient queue; the critical queue keeps the per-image dgap kernel
                defer = shards and switches.get('SALT_SE_FC_SIDE')
                kw = dict(dtype=self.dt, x=xview(), y=out.view(), dy=out.gview(), w1=l1.weight.data_ptr(), w2=l2.weight.data_ptr(),
                          R=R, ws=cs.weight.data_ptr(), gap=gap.data_ptr(), hidden=hid.data_ptr(), gate_c=gc.data_ptr(), gate_s=gs.data_ptr(),
                          partials=Scratch('se', B * nparts * (2 * C + 1) * 4), nparts=nparts, g_w1=gp(l1.weight), g_b1=gp(l1.bias),
                          g_w2=gp(l2.weight), g_b2=gp(l2.bias), g_ws=gp(cs.weight), g_bs=gp(cs.bias), dgap=dgap.data_ptr(),
                          dx=x.gview(), accumulate=acc, defer_param_grads=int(defer), **in_bwd)
                sb = self.bwd.add('scse_bwd', **kw)
                sg = self.bwd.add('scse_fc_grads', stream=1, **kw) if defer else None
                # round 6: with the input transform the kernel holds everything the producer layer's BatchNorm backward sums over - it takes
                # them too and that layer's bn_bwd loses its reduction pass (saltnet.h salt_scse_bwd_args.bnb_acc; SALT_SE_BNB=0: off)
                carry = (taken is not None and shards and x.buf.bn_train_out == (x.c0, x.C) and acc == 0
                         and x.B * x.H * x.W < (1 << 31) and switches.get('SALT_SE_BNB'))
                if shards:
                    self._fin_slot('bwd', B * ((6 if carry else 2) * C + 1), (sb, 'acc'), *([(sg, 'acc')] if sg is not None else []))
                # x = relu(bn(conv)): its only gradient consumer is that layer's bn_bwd, which can add the channel-SE term dgap[b][c]
                # wherever it reads dL/dx - the broadcast-add pass over dx (read + write of the whole tensor) disappears
                if (x.buf.bn_train_out == (x.c0, x.C) and acc == 0 and x.B * x.H * x.W < (1 << 31)):
                    if x.buf.grad_bias is not None:
                        raise SaltError('two pending gradient biases on %s' % x.buf.name)
                    self.bwd.set_fields(sb, skip_bcast=1)
                    x.buf.grad_bias = GradBias(x.c0, x.C, dgap, *((sb, sg) if carry else ()))
                    self._bias_bufs.append(x.buf)
            self.tape.append(backward)
        return out

    # ------------------------------------------------------------------ SE-ResNet bottleneck tail (csrc/se_res.hip)
    @staticmethod
    def se_res_ok(C, R):
        """The shapes salt_se_res runs (saltnet.h): C a multiple of 64 up to 2048, R = C / 16."""
        return C % 64 == 0 and C <= 2048 and R * 16 == C

    def se_res(self, x, bn, se, res, out=None, name=''):
        """relu(x * gate(x) + res) with gate = sigmoid(fc2(relu(fc1(mean_hw x)))) (SEModule + the residual tail of SEResNetBottleneck).
        ``x`` is what ``Graph.conv(a, conv3, bn, relu=False)`` returned.  Training with consumer-side BatchNorm shards: this operator is
        the only reader of that activation, so the affine_act that would store it is taken back out of the program (_take_act_op) and
        the kernels apply ``bn``'s scale / shift to the raw convolution output themselves (salt_se_res_args.in_fin); otherwise (eval:
        BatchNorm folded into the convolution; the partials protocols) x is read as stored.  Backward: dL/dres with the accumulate
        convention of Graph.conv(.., res=), dL/dx into x's gradient - the closure of the convolution in front runs bn's backward on it."""
        fc1, fc2 = se.fc1, se.fc2
        B, C, R = x.B, x.C, fc1.weight.shape[0]
        if bn.num_features != C or tuple(fc1.weight.shape) != (R, C, 1, 1) or tuple(fc2.weight.shape) != (C, R, 1, 1) or not self.se_res_ok(C, R):
            raise SaltError('se_res %s: %d channels with fc1 %s / fc2 %s (C a multiple of 64 up to 2048 and C / 16 hidden units are supported)'
                            % (name, C, tuple(fc1.weight.shape), tuple(fc2.weight.shape)))
        if (res.B, res.H, res.W, res.C) != (x.B, x.H, x.W, C):
            raise SaltError('se_res %s: shortcut %s does not fit %s' % (name, (res.B, res.H, res.W, res.C), (x.B, x.H, x.W, C)))
        if out is None:
            out = self.new_act(x.B, x.H, x.W, C, name)
        shards = bool(self.train and self._fin_mode() == 2 and switches.get('SALT_SE_SHARDS'))   # per-image sums through the zeroed fp64 arena
        taken = self._take_act_op(x) if (self.train and switches.get('SALT_SE_RES_IN_BN')) else None
        if taken is not None:
            sa, Fbn = taken
            xv_ = sa.y                                   # the raw convolution output; never x.view(): the activation has no storage
            in_kw, in_bwd = dict(in_fin=ctypes.addressof(Fbn)), dict(in_scale=Fbn.scale, in_shift=Fbn.shift)
        else:
            xv_, in_kw, in_bwd = None, {}, {}
        xview = (lambda: xv_) if taken is not None else x.view
        nparts = lib.salt_se_res_parts(ctypes.byref(fill(STRUCTS['salt_se_res_args'](), dtype=self.dt, x=xview())))
        if nparts < 1:
            raise SaltError('se_res plan failed: ' + lib.salt_last_error().decode(errors='replace'))
        gap, hid, gate = self.f32(B * C), self.f32(B * R), self.f32(B * C)
        # (one workspace name for both programs: the operator is the main branch's and is never emitted inside Graph.side())
        ws = Scratch('se_res', B * nparts * C * 4)
        if res.on_side:
            self.join()                                  # the projection shortcut ran on the side stream
        sf = self.fwd.add('se_res', dtype=self.dt, x=xview(), res=res.view(), w1=fc1.weight.data_ptr(), b1=fc1.bias.data_ptr(), w2=fc2.weight.data_ptr(),
                          b2=fc2.bias.data_ptr(), R=R, gap_partials=None if shards else ws, nparts=nparts, gap=gap.data_ptr(), hidden=hid.data_ptr(),
                          gate=gate.data_ptr(), y=out.view(), **in_kw)
        if taken is not None:
            self._retarget_fin_acc(sa, sf, 'in_fin_acc')
        if shards:
            self._fin_slot('fwd', B * C, (sf, 'gap_acc'))
        out.on_side = self.fwd.default_stream == 1
        if self.train:
            def backward():
                acc_res = res.grad_state()
                assert x.grad_state() == 0, 'the BatchNorm output in front of se_res has a single consumer'
                gp = self._gp
                du, dh, dgap = self.f32(B * C), self.f32(B * R), self.f32(B * C)
                kw = dict(dtype=self.dt, x=xview(), y=out.view(), dy=out.gview(), w1=fc1.weight.data_ptr(), w2=fc2.weight.data_ptr(), R=R,
                          gap=gap.data_ptr(), hidden=hid.data_ptr(), gate=gate.data_ptr(), partials=None if shards else ws,
                          nparts=nparts, du=du.data_ptr(), dh=dh.data_ptr(), dgap=dgap.data_ptr(), dx=x.gview(), dres=res.gview(),
                          accumulate_dres=acc_res, g_w1=gp(fc1.weight), g_b1=gp(fc1.bias), g_w2=gp(fc2.weight), g_b2=gp(fc2.bias),
                          defer_param_grads=1, **in_bwd)
                sb = self.bwd.add('se_res_bwd', **kw)
                # the four parameter gradients are nobody's input before the optimizer: their launch goes to the weight-gradient queue
                self.bwd.add('se_res_fc_grads', stream=1, **kw)
                if shards:
                    self._fin_slot('bwd', B * C, (sb, 'acc'))
            self.tape.append(backward)
        return out

    # ------------------------------------------------------------------ depth-conditioned channel gate (csrc/depth.hip)
    def _gate_shards(self):
        """dL/ds travels like the cSE pooled sums (Graph.scse): fp64 atomics into the zeroed arena, or fixed-order partials."""
        return bool(self.train and self._fin_mode() == 2 and switches.get('SALT_SE_SHARDS'))

    def depth_gate(self, d, fc):
        """s[B, C] = sigmoid(fc(d)) for ``fc = nn.Linear(1, C)`` and the static depth buffer ``d`` [B,1] (architectures/base.py:120-131).
        Returns the gate record that ``channel_gate`` consumes; backward (emitted LAST: every channel_gate backward has then delivered
        its columns of dL/ds) writes fc.weight.grad and fc.bias.grad.  ``d`` gets no gradient."""
        B, C = int(d.shape[0]), fc.weight.shape[0]
        s = self.f32(B * C)
        self.fwd.add('depth_gate', d=self._in(d), w=fc.weight.data_ptr(), bias=fc.bias.data_ptr(), B=B, C=C, s=s.data_ptr(), backward=0)
        gate = DepthGate(s, B, C, self.f32(B * C) if (self.train and not self._gate_shards()) else None, [], np.zeros(C, dtype=bool))
        if self.train:
            def backward():
                if not gate.covered.all():
                    raise SaltError('depth_gate: %d of %d gate channels never met a channel_gate' % (int((~gate.covered).sum()), C))
                sb = self.bwd.add('depth_gate', d=self._in(d), B=B, C=C, s=s.data_ptr(), backward=1,
                                  ds=gate.ds.data_ptr() if gate.ds is not None else None, gw=self._gp(fc.weight), gb=self._gp(fc.bias),
                                  accumulate=0)
                if gate.ds is None:
                    self._fin_slot('bwd', B * C, (sb, 'ds_acc'), *[(u, 'ds_acc') for u in gate.users])
            self.tape.append(backward)
        return gate

    def channel_gate(self, x, gate, c0, out=None, name='gate'):
        """out = x * s[:, c0 : c0 + x.C] per image and channel.  ``out`` = x's own slice: in place (x has no other forward reader and the backward
        of its producer does not need the ungated values); otherwise a gated copy.  Backward: dL/dx (+)= dL/dout * s and the columns
        [c0, c0 + x.C) of dL/ds."""
        inplace = out is not None and out.buf is x.buf and (out.c0, out.C) == (x.c0, x.C)
        if out is None:
            out = self.new_act(x.B, x.H, x.W, x.C, name)
        if gate.covered[c0:c0 + x.C].any() or c0 + x.C > gate.C or x.B != gate.B:
            raise SaltError('channel_gate: channels [%d, %d) of a %d-channel gate' % (c0, c0 + x.C, gate.C))
        gate.covered[c0:c0 + x.C] = True
        S = fill(STRUCTS['salt_channel_gate_args'](), dtype=self.dt, x=x.view())
        nparts = lib.salt_channel_gate_parts(ctypes.byref(S))
        if nparts < 1:
            raise SaltError('channel_gate: %d channels are not supported' % x.C)
        self.fwd.add('channel_gate', dtype=self.dt, x=x.view(), y=out.view(), s=gate.s.data_ptr(), sC=gate.C, c0=c0, backward=0)
        out.on_side = self.fwd.default_stream == 1
        if self.train:
            def backward():
                if not out.grad_ready():
                    raise SaltError('channel_gate: dL/d(%s) was never written' % name)
                acc = 0 if inplace else x.grad_state()
                kw = dict(dtype=self.dt, x=out.view() if inplace else x.view(), y=out.gview(), dx=out.gview() if inplace else x.gview(),
                          s=gate.s.data_ptr(), sC=gate.C, c0=c0, backward=1, accumulate=acc, inplace=int(inplace), nparts=nparts)
                if gate.ds is not None:
                    kw.update(ds=gate.ds.data_ptr(), partials=Scratch('gate', x.B * nparts * x.C * 4))
                gate.users.append(self.bwd.add('channel_gate', **kw))
            self.tape.append(backward)
        return out
