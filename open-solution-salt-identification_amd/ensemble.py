"""Ensembling between models on the device: what turns trained networks into a result.

  fold mean                main.py:892-912 (save_predictions: np.mean over the folds' test predictions, binarize, encode),
                           notebooks/prediction_average.ipynb (the same across experiments, float64 accumulator)
                                                                             -> salt_ensemble (mean / mask)
  first-level stacks       utils.py:560-581 (group_predictions_by_id, join_id_predictions: channel 1 of every model,
                           np.stack(axis=-1)), the input of StackingFCN / StackingPreprocessor
                                                                             -> salt_ensemble (stack)
  submission               utils.py:68-75, 99-111 (create_submission, run_length_encoding)
                                                                             -> salt_rle_encode (+ the csv module)
  fold split               utils.py:371-389 (KFoldBySortedValue), numpy only

The kernels need the HIP library; there is no CPU path.  The fold splitter and the submission writer are host code.
"""
import csv
import ctypes

import numpy as np
import torch

from ._abi import CONSTS, OP_FUNCS, SaltError, check, fill
from .inference import crop_window, predict_tta_tiles

MAX_MEMBERS = CONSTS['SALT_MAX_MEMBERS']
ENSEMBLE_MODES = {'resize_and_pad': 0, 'resize': 1, 'stacking': 1}        # crop window | resize_image
ACCUMULATORS = {'f32': 0, 'f64': 1}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _members(probs, what):
    """list of K fp32 device tensors [B,C,H,W] of one shape, or one [K,B,C,H,W] tensor -> list of contiguous tensors"""
    if torch.is_tensor(probs):
        if probs.dim() != 5:
            raise SaltError('%s: a tensor of members must be [K,B,C,H,W]' % what)
        probs = list(probs.contiguous().unbind(0))
    probs = list(probs)
    if not 1 <= len(probs) <= MAX_MEMBERS:
        raise SaltError('%s: 1 <= K <= %d members (got %d)' % (what, MAX_MEMBERS, len(probs)))
    out = []
    for p in probs:
        if not torch.is_tensor(p) or not p.is_cuda:
            raise SaltError('%s: members must live on the GPU (there is no CPU path)' % what)
        if p.dim() != 4 or p.dtype != torch.float32 or p.shape != probs[0].shape or p.device != probs[0].device:
            raise SaltError('%s: members must be fp32 [B,C,H,W] tensors of one shape on one device' % what)
        out.append(p.contiguous())
    return out


def _ensemble(what, probs, loader_mode, target_size, acc, mean=False, mask=False, threshold=0.5, cls=1, stack=None, strides=None, m0=0):
    members = _members(probs, what)
    if loader_mode not in ENSEMBLE_MODES:
        raise SaltError('%s: loader_mode %r (%s)' % (what, loader_mode, ' | '.join(ENSEMBLE_MODES)))
    mode = ENSEMBLE_MODES[loader_mode]
    if acc is None:
        acc = 'f64' if mode else 'f32'
    if acc not in ACCUMULATORS:
        raise SaltError("%s: acc %r ('f32' | 'f64' | None)" % (what, acc))
    if mode and acc == 'f32':
        raise SaltError("%s: the resized maps of the reference are float64: loader_mode %r needs acc='f64'" % (what, loader_mode))
    B, C, H, W = members[0].shape
    h, w = int(target_size[0]), int(target_size[1])
    if h < 1 or w < 1 or h > H or w > W:
        raise SaltError('%s: target size %dx%d for %dx%d maps' % (what, h, w, H, W))
    if not 0 <= int(cls) < C:
        raise SaltError('%s: cls %d of %d channels' % (what, cls, C))
    top, left = (0, 0) if mode else crop_window(H, W, (h, w))
    dev = members[0].device
    table = (ctypes.c_void_p * len(members))(*[m.data_ptr() for m in members])
    out_mean = torch.empty((B, C, h, w), dtype=torch.float32, device=dev) if mean else None
    out_mask = torch.empty((B, h, w), dtype=torch.uint8, device=dev) if mask else None
    fn, S = OP_FUNCS['salt_ensemble']
    s = fill(S(), members=ctypes.cast(table, ctypes.c_void_p).value, K=len(members), B=B, C=C, H=H, W=W, mode=mode, top=top, left=left,
             h=h, w=w, acc=ACCUMULATORS[acc], mean=out_mean.data_ptr() if mean else None, cls=int(cls), threshold=float(threshold),
             mask=out_mask.data_ptr() if mask else None, stack=stack.data_ptr() if stack is not None else None, m0=int(m0),
             **(strides or {}))
    check(fn(ctypes.byref(s), _stream()), what)
    return out_mean, out_mask


def fold_mean(probs, loader_mode='resize_and_pad', target_size=(101, 101), acc=None):
    """np.mean(np.array(maps), axis=0) of K probability maps on the crop window ('resize_and_pad') or behind resize_image ('resize' /
    'stacking'): fp32 [B,C,h,w].  ``acc``: 'f32' (main.py's mean of float32 maps: sequential fp32 adds, one division), 'f64' (the
    notebook's accumulator; the only one behind the float64 resize) or None = 'f32' for the crop, 'f64' for the resized modes."""
    return _ensemble('fold_mean', probs, loader_mode, target_size, acc, mean=True)[0]


def fold_masks(probs, loader_mode='resize_and_pad', target_size=(101, 101), acc=None, threshold=0.5, cls=1):
    """binarize(fold mean): uint8 [B,h,w] of ``mean[:, cls] > threshold``; the mean itself is never stored.  The fp32 mean is compared
    with float32(threshold) as numpy compares it, the float64 mean with the threshold itself."""
    return _ensemble('fold_masks', probs, loader_mode, target_size, acc, mask=True, threshold=threshold, cls=cls)[1]


def first_level_stack(probs, loader_mode='resize_and_pad', target_size=(101, 101), cls=1, layout='mhw', out=None, m0=0):
    """Every member's own class map, not averaged (utils.py:568, 580): fp32 [B,M,h,w] (``layout='mhw'``, the planes
    StackingPreprocessor(layout='mhw') reads) or [B,h,w,M] ('hwm' = np.stack(maps, axis=-1)).  ``out`` / ``m0``: fill maps
    [m0, m0 + K) of a wider contiguous stack (M experiments, each itself a fold mean) and leave its other maps alone."""
    members = _members(probs, 'first_level_stack')
    if layout not in ('mhw', 'hwm'):
        raise SaltError("first_level_stack: layout %r ('mhw' | 'hwm')" % (layout,))
    B, K = members[0].shape[0], len(members)
    h, w = int(target_size[0]), int(target_size[1])
    m0 = int(m0)
    if out is None:
        if m0 != 0:
            raise SaltError('first_level_stack: m0 belongs to out=')
        out = torch.empty((B, K, h, w) if layout == 'mhw' else (B, h, w, K), dtype=torch.float32, device=members[0].device)
    if not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.dim() != 4 or not out.is_contiguous():
        raise SaltError('first_level_stack: out must be a contiguous fp32 device tensor')
    M = out.shape[1] if layout == 'mhw' else out.shape[3]
    if tuple(out.shape) != ((B, M, h, w) if layout == 'mhw' else (B, h, w, M)) or m0 < 0 or m0 + K > M:
        raise SaltError('first_level_stack: maps [%d, %d) do not fit a stack of shape %s (%s)' % (m0, m0 + K, tuple(out.shape), layout))
    strides = dict(sb=M * h * w, sr=w, sc=1, sm=h * w) if layout == 'mhw' else dict(sb=h * w * M, sr=w * M, sc=M, sm=1)
    mode = ENSEMBLE_MODES.get(loader_mode, 0)
    _ensemble('first_level_stack', members, loader_mode, target_size, 'f64' if mode else 'f32', cls=cls, stack=out, strides=strides, m0=m0)
    return out


# ----------------------------------------------------------------------------- submission
def _rle_device(masks):
    """(counts [B] int64, runs [total, 2] int64) of uint8 device masks [B,h,w].  total, counts and the runs share one device buffer; the
    head (total, counts) is copied first because it holds the length of the second copy, runs[:total]."""
    if not torch.is_tensor(masks) or not masks.is_cuda:
        raise SaltError('rle_encode: masks must live on the GPU (inference.run_length_encoding is the host encoder)')
    if masks.dim() == 2:
        masks = masks[None]
    if masks.dim() != 3 or masks.shape[0] < 1:
        raise SaltError('rle_encode: masks must be [B,h,w]')
    masks = masks.contiguous().to(torch.uint8)
    B, h, w = masks.shape
    if not 1 <= h * w <= 65536:
        raise SaltError('rle_encode: 1 <= h w <= 65536 (got %dx%d)' % (h, w))
    cap = B * ((h * w + 1) // 2)                          # the worst case: a checkerboard in column-major order
    # one int32 buffer: [total (int64, two words) | counts [B] (+ pad to an even word) | runs [cap, 2]]
    words_counts = B + (B & 1)
    buf = torch.empty((2 + words_counts + 2 * cap,), dtype=torch.int32, device=masks.device)
    base = buf.data_ptr()
    fn, S = OP_FUNCS['salt_rle_encode']
    s = fill(S(), mask=masks.data_ptr(), B=B, h=h, w=w, counts=base + 8, runs=base + 8 + 4 * words_counts, cap_pairs=cap, total=base)
    check(fn(ctypes.byref(s), _stream()), 'rle_encode')
    head = buf[:2 + words_counts].cpu()                   # total and counts ...
    total = int(head[:2].view(torch.int64)[0])
    counts = head[2:2 + B].numpy().astype(np.int64)
    runs = buf[2 + words_counts:2 + words_counts + 2 * total].cpu().numpy().astype(np.int64).reshape(-1, 2)      # ... then only the runs
    return counts, runs


def rle_encode(masks):
    """utils.run_length_encoding of a batch of device masks [B,h,w]: a list of B flat lists [start, length, start, length, ...], each
    equal to inference.run_length_encoding of that mask.  Only the packed runs cross to the host, not the masks."""
    counts, runs = _rle_device(masks)
    flat, offs = runs.reshape(-1).tolist(), np.concatenate([[0], np.cumsum(counts)]) * 2
    return [flat[offs[b]:offs[b + 1]] for b in range(len(counts))]


def create_submission(ids, masks):
    """utils.create_submission (utils.py:68-75) without pandas: rows (id, 'start length start length ...'); an empty mask gives ''.
    ``masks``: device masks [B,h,w] (encoded by salt_rle_encode) or a list of run lists from rle_encode."""
    rles = rle_encode(masks) if torch.is_tensor(masks) else [list(r) for r in masks]
    ids = list(ids)
    if len(ids) != len(rles):
        raise SaltError('create_submission: %d ids for %d masks' % (len(ids), len(rles)))
    return [(str(i), ' '.join(str(v) for v in r)) for i, r in zip(ids, rles)]


def write_submission(path, ids, masks):
    """submission.csv as main.py:909-911 writes it (header id,rle_mask, no index) through the csv module; returns the rows"""
    rows = create_submission(ids, masks)
    with open(path, 'w', newline='', encoding='utf-8') as f:
        wr = csv.writer(f, lineterminator='\n')
        wr.writerow(['id', 'rle_mask'])
        wr.writerows(rows)
    return rows


# ----------------------------------------------------------------------------- fold split
class KFoldBySortedValue:
    """utils.py:371-389 without sklearn: the samples are ordered by value (a STABLE sort: ties keep their index order) and fold s tests
    every n_splits-th of them from s; both index arrays come in ascending index order, as BaseCrossValidator.split gives them
    (it turns the fold's indices into a mask).  ``shuffle`` / ``random_state`` are kept and, as in the reference, not used."""

    def __init__(self, n_splits=3, shuffle=False, random_state=None):
        self.n_splits, self.shuffle, self.random_state = int(n_splits), shuffle, random_state

    def get_n_splits(self, X=None, y=None, groups=None):
        return self.n_splits

    def split(self, values, y=None, groups=None):
        values = np.asarray(values).reshape(-1)
        order = np.argsort(values, kind='stable')
        index = np.arange(values.shape[0])
        for s in range(self.n_splits):
            test = order[s::self.n_splits]
            held = np.zeros(values.shape[0], dtype=bool)
            held[test] = True
            yield index[~held], index[held]


# ----------------------------------------------------------------------------- K networks, one result
class FoldEnsemble:
    """K eval-mode HipNetworks (the folds of one experiment, or different architectures) behind one preprocessor: every member runs
    through predict_tta_tiles, then ONE salt_ensemble launch gives the fold mean, its masks or the first-level stack.  In the resized
    modes the ensemble sees every member's un-resized TTA aggregate and evaluates the float64 interpolant itself, so the result is
    the reference's resize-each-then-mean."""

    def __init__(self, nets, preprocessor, flip_ud=False, flip_lr=True, rotation=False, method='mean', loader_mode='resize_and_pad',
                 pad_method='edge', target_size=(101, 101), activation='sigmoid'):
        """``activation``: the members' model_params['activation'], 'sigmoid' (default) or 'softmax'; passed to predict_tta_tiles"""
        nets = list(nets)
        if not 1 <= len(nets) <= MAX_MEMBERS:
            raise SaltError('FoldEnsemble: 1 <= K <= %d networks (got %d)' % (MAX_MEMBERS, len(nets)))
        for n in nets:
            if getattr(n, 'uses_depth', False):
                raise SaltError('FoldEnsemble: %s is depth-conditioned and predict_tta_tiles has no depth input' % type(n).__name__)
            if n.training:
                raise SaltError('FoldEnsemble: call net.eval() on every member first')
        if loader_mode not in ('resize_and_pad', 'resize'):
            raise SaltError("FoldEnsemble: loader_mode %r ('resize_and_pad' | 'resize')" % (loader_mode,))
        self.nets, self.preprocessor = nets, preprocessor
        self.tta = dict(flip_ud=flip_ud, flip_lr=flip_lr, rotation=rotation, method=method, loader_mode=loader_mode, pad_method=pad_method,
                        activation=activation)
        self.loader_mode, self.target_size = loader_mode, (int(target_size[0]), int(target_size[1]))

    def members(self, images):
        """every member's TTA aggregate at the network's own size, [B,C,H,W] each"""
        return [predict_tta_tiles(n, self.preprocessor, images, resize_back=False, **self.tta) for n in self.nets]

    def predict(self, images, acc=None):
        return fold_mean(self.members(images), self.loader_mode, self.target_size, acc)

    def predict_masks(self, images, threshold=0.5, cls=1, acc=None):
        return fold_masks(self.members(images), self.loader_mode, self.target_size, acc, threshold, cls)

    def predict_stack(self, images, layout='mhw', cls=1, out=None, m0=0):
        return first_level_stack(self.members(images), self.loader_mode, self.target_size, cls, layout, out, m0)
