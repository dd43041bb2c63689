"""On-device input pipeline (SURVEY.md §8 "next" row f-1).

The reference prepares every tile on the CPU with PIL / imgaug / torchvision and copies fp32 tensors to the GPU
(loaders.py:603-612, augmentation.py:79-96,247-284, utils.py:494-500, loaders.py:763-769).  Here the raw 101x101 gray tiles
(uint8, 10 KB each) are copied once and one kernel produces the network's input batch and the one-hot target:

    train      resize 101 -> 102 (cubic: imgaug 0.2.5's iaa.Scale default; or bilinear) + edge-pad 13 on every side -> 128   (neptune.yaml:22-26)
    inference  edge-pad to the next multiple of 64 with the reference's split: top 13 / bottom 14, left 14 / right 13
    both       Grayscale(3) + ToTensor + Normalize(ImageNet) + AddDepthChannels; mask -> {background, salt} one-hot

The reference's other loader modes (pipelines.py:12-14) and its other pad (neptune.yaml:24) are here too:

    DevicePreprocessor(..., loader_mode='resize')     scale to `resize` (128) without a pad, in both branches (augmentation.py:71-90)
    DevicePreprocessor(..., pad_method='reflect')     reflect-101 instead of the edge pad, in both branches and with augment=
    StackingPreprocessor(size=(128, 128))             loader_mode 'stacking' (loaders.py:564-579): first-level maps -> X, masks -> target

Training augmentation (the reference's affine_seq / intensity_seq, main.py:130-133, augmentation.py:34-65) runs on the device too,
fused into the same pass (csrc/augment.hip, `salt_augment_preprocess`).  It is off by default; a main.py-style caller turns it on for
the training batches only:

    pre_train = DevicePreprocessor(True, 3, augment=True, seed=1234 + rank)     # data-parallel ranks need distinct seeds
    pre_valid = DevicePreprocessor(False, 3)                                   # inference / validation batches are never augmented
    X, target = pre_train(images_u8, masks_u8)                                 # [B,101,101] uint8 on the GPU

``augment=AugmentConfig(...)`` changes probabilities / ranges or switches single ops off; every call draws fresh parameters from
(seed, call counter, image index), and ``record_params=True`` keeps the drawn record for ``last_params()``.
"""
import ctypes
import dataclasses

import numpy as np
import torch

from ._abi import OP_FUNCS, SaltError, check, fill

MEAN = (0.485, 0.456, 0.406)          # ImageNet statistics (neptune.yaml / loaders.py dataset_params)
STD = (0.229, 0.224, 0.225)


LOADER_MODES = ('resize_and_pad', 'resize')        # pipelines.py:12-14; 'stacking' is StackingPreprocessor's
PAD_METHODS = ('edge', 'reflect')                  # salt_preprocess_args.pad_mode 0 / 1


def pad_split(size, divisor=64):
    """(before, after) edge padding of one dimension for InferencePad (augmentation.py:262-277 + utils.py:308-313).
    Vertical: before = top = int(pad / 2).  Horizontal: the sequence is (top, right, bottom, left) with right = int(pad / 2),
    so the *left* side gets the larger half."""
    pad = 0 if size % divisor == 0 else divisor - size % divisor
    return int(pad / 2), pad - int(pad / 2)


AUG_OPS = ('fliplr', 'sharpen', 'emboss', 'affine', 'piecewise', 'perspective', 'invert', 'contrast', 'add', 'add_elementwise',
           'multiply', 'multiply_elementwise')          # the SALT_AUG_* enable bits, in bit order
N_PARAMS = 64                                          # SALT_AUG_PARAMS
STAGE_ORDERS = ('ABC', 'ACB', 'BAC', 'BCA', 'CAB', 'CBA')
INTENSITY_OPS = ('noop', 'add', 'add_elementwise', 'multiply', 'multiply_elementwise')


@dataclasses.dataclass
class AugmentConfig:
    """The reference's augmentation sequences (augmentation.py:34-65) as numbers; defaults are the reference's.  ``enable``: the ops that
    may be drawn (SomeOf draws among the enabled children of stage A only; OneOf among the enabled intensity ops)."""
    enable: tuple = AUG_OPS
    p_fliplr: float = 0.5
    sharpen_alpha: float = 0.5
    sharpen_lightness: float = 1.0
    emboss_alpha: float = 0.5
    emboss_strength: float = 1.0
    rotate: tuple = (-10.0, 10.0)
    shift: tuple = (-0.05, 0.05)
    p_piecewise: float = 0.3
    piecewise_scale: tuple = (0.04, 0.08)
    p_perspective: float = 0.3
    perspective_scale: tuple = (0.05, 0.1)
    p_invert: float = 0.3
    p_contrast: float = 0.3
    contrast: tuple = (0.5, 1.5)
    p_intensity_noop: float = 0.5
    add: tuple = (-10, 10)
    multiply: tuple = (0.95, 1.05)

    @classmethod
    def none(cls, **kw):
        """every op switched off (the identity): ``AugmentConfig.none(enable=('fliplr',))`` enables one"""
        kw.setdefault('enable', ())
        return cls(**kw)

    def enable_mask(self):
        bad = [o for o in self.enable if o not in AUG_OPS]
        if bad:
            raise SaltError('AugmentConfig: unknown ops %s (known: %s)' % (bad, ', '.join(AUG_OPS)))
        return sum(1 << AUG_OPS.index(o) for o in set(self.enable))

    def fill(self, cfg):
        """set a ctypes salt_augment_config"""
        fill(cfg, enable=self.enable_mask(), p_fliplr=self.p_fliplr, sharpen_alpha=self.sharpen_alpha, sharpen_lightness=self.sharpen_lightness,
             emboss_alpha=self.emboss_alpha, emboss_strength=self.emboss_strength, rotate_min=self.rotate[0], rotate_max=self.rotate[1],
             shift_min=self.shift[0], shift_max=self.shift[1], p_piecewise=self.p_piecewise, piecewise_scale_min=self.piecewise_scale[0],
             piecewise_scale_max=self.piecewise_scale[1], p_perspective=self.p_perspective, perspective_scale_min=self.perspective_scale[0],
             perspective_scale_max=self.perspective_scale[1], p_invert=self.p_invert, p_contrast=self.p_contrast,
             contrast_min=self.contrast[0], contrast_max=self.contrast[1], p_intensity_noop=self.p_intensity_noop,
             add_min=int(self.add[0]), add_max=int(self.add[1]), mul_min=self.multiply[0], mul_max=self.multiply[1])


def decode_params(params):
    """[B, 64] params record (saltnet.h SALT_AUG_PARAMS layout) -> dict of numpy arrays, one entry per image"""
    p = np.asarray(params.detach().cpu() if torch.is_tensor(params) else params, dtype=np.float32).reshape(-1, N_PARAMS)
    return {'order': p[:, 0].astype(np.int64), 'n': p[:, 1].astype(np.int64), 'chosen': p[:, 2:6] != 0, 'flip': p[:, 6] != 0,
            'angle': p[:, 7], 'shift': p[:, 8], 'piecewise': p[:, 9] != 0, 'piecewise_scale': p[:, 10],
            'piecewise_jitter': p[:, 11:43].reshape(-1, 4, 4, 2), 'perspective': p[:, 43] != 0, 'perspective_scale': p[:, 44],
            'perspective_corners': p[:, 45:53].reshape(-1, 4, 2), 'invert': p[:, 53] != 0, 'contrast': p[:, 54] != 0,
            'contrast_alpha': p[:, 55], 'intensity_op': p[:, 56].astype(np.int64), 'value': p[:, 57]}


class DevicePreprocessor:
    """Callable: (images [B,h,w] uint8|float, masks [B,h,w] or None) on the GPU -> (X [B,C,H,W], target [B,2,H,W] | None)."""

    def __init__(self, train, channels=3, resize=102, pad=13, divisor=64, mean=MEAN, std=STD, interpolation='cubic', augment=False, seed=1234,
                 record_params=False, loader_mode='resize_and_pad', pad_method='edge'):
        """``loader_mode``: 'resize_and_pad' (default: the geometry above) or 'resize' (pipelines.py:12-14, augmentation.py:71-90
        resize_seq / resize_to_fit_net): the tile is scaled to ``resize`` x ``resize`` (128 in the reference's config) and NOT padded, in the
        train and the inference branch, image and mask alike - the same resize kernel with top = left = 0.
        ``pad_method``: 'edge' (default) or 'reflect' (neptune.yaml:24; PadFixed's cv2.BORDER_REFLECT_101 in training, imgaug's
        np.pad(mode='reflect') at inference - one index map), applied where the edge pad is, in both branches and with ``augment``; it
        needs a pad of at most n - 1 pixels on every side.

        ``interpolation`` of the train-branch resize: 'cubic' (default) is what the reference executes - augmentation.py:79-85 calls
        ``iaa.Scale({...})`` without an interpolation argument and imgaug 0.2.5 (environment.yml:15) defaults to 'cubic' =
        cv2.INTER_CUBIC, applied to the uint8 tile AND the uint8 {0,1} mask.  uint8 tiles take cv2's own evaluation of that filter
        (11-bit fixed-point coefficients, integer sums, saturating shift: opencv_python 3.4.0.12, environment.yml:16); float tiles -
        and 'cubic_float' for uint8 ones - the float form of the same filter (differs by 1 LSB on a few percent of the pixels);
        'bilinear' is rounds 1-2 of this build.

        ``augment``: False (default: the tiles as they are), True (the reference's affine_seq + intensity_seq) or an AugmentConfig;
        training batches of uint8 tiles up to 128x128 with the 'cubic' resize only.  ``seed``: the draws of image b of the k-th call are a
        pure function of (seed, k, b) - give every data-parallel rank its own seed.  ``record_params``: keep the drawn parameters of the
        last call for ``last_params()``."""
        if interpolation not in ('cubic', 'cubic_float', 'bilinear'):
            raise SaltError('DevicePreprocessor: interpolation %r (cubic | cubic_float | bilinear)' % (interpolation,))
        if loader_mode not in LOADER_MODES:
            raise SaltError('DevicePreprocessor: loader_mode %r (%s; the stacking loader is StackingPreprocessor)' % (loader_mode, ' | '.join(LOADER_MODES)))
        if pad_method not in PAD_METHODS:
            raise SaltError('DevicePreprocessor: pad_method %r (%s)' % (pad_method, ' | '.join(PAD_METHODS)))
        self.loader_mode, self.pad_method = loader_mode, pad_method
        self.interpolation = interpolation
        self.train, self.channels, self.resize, self.pad, self.divisor = bool(train), int(channels), resize, pad, divisor
        self.mean, self.std = tuple(mean), tuple(std)
        if augment is True:
            augment = AugmentConfig()
        elif augment is False or augment is None:
            augment = None
        elif not isinstance(augment, AugmentConfig):
            raise SaltError('DevicePreprocessor: augment must be True, False or an AugmentConfig')
        if augment is not None and not self.train:
            raise SaltError('DevicePreprocessor: augmentation is for training batches (the reference never augments inference batches)')
        if augment is not None and interpolation != 'cubic':
            raise SaltError("DevicePreprocessor: augmentation runs with the 'cubic' resize of uint8 tiles")
        if augment is not None:
            augment.enable_mask()
        self.augment, self.seed, self.record_params = augment, int(seed), bool(record_params)
        self.counter = 0                       # calls so far: the `counter` of the next augmented call
        self._params = None

    def geometry(self, h, w):
        """(resize_h, resize_w, top, left, H, W)"""
        if self.loader_mode == 'resize':
            r = self.resize
            rh, rw = (0, 0) if (h, w) == (r, r) else (r, r)
            return rh, rw, 0, 0, r, r
        if self.train:
            r = self.resize
            return r, r, self.pad, self.pad, r + 2 * self.pad, r + 2 * self.pad
        top, bottom = pad_split(h, self.divisor)
        right, left = pad_split(w, self.divisor)          # horizontal: int(pad/2) goes to the right
        return 0, 0, top, left, h + top + bottom, w + left + right

    def __call__(self, images, masks=None, params=None, debug=False):
        """``params`` ([B, 64] fp32 on the GPU, augmentation only): replay that record instead of drawing.  ``debug``: also return a dict
        with the geometric-stage tiles 'geo_img' / 'geo_mask' [B,h,w] and the padded intensity-stage tile 'gray' [B,H,W] (uint8)."""
        if not images.is_cuda or (masks is not None and not masks.is_cuda) or (params is not None and not params.is_cuda):
            raise SaltError('DevicePreprocessor: tensors must live on the GPU (there is no CPU path)')
        if images.dtype not in (torch.uint8, torch.float32):
            raise SaltError('DevicePreprocessor: images must be uint8 or float32 in [0, 1]')
        if self.augment is not None:
            return self._augment(images, masks, params, debug)
        if params is not None or debug:
            raise SaltError('DevicePreprocessor: params / debug need augment')
        images = images.contiguous()
        B, h, w = images.shape
        rh, rw, top, left, H, W = self.geometry(h, w)
        self._check_pad(h, w, rh, rw, top, left, H, W)
        x = torch.empty((B, self.channels, H, W), dtype=torch.float32, device=images.device)
        target, mptr = None, None
        if masks is not None:
            masks = masks.contiguous().to(torch.uint8)
            target = torch.empty((B, 2, H, W), dtype=torch.float32, device=images.device)
            mptr = masks.data_ptr()
        fn, S = OP_FUNCS['salt_preprocess']
        s = S()
        fill(s, img=images.data_ptr(), img_is_u8=int(images.dtype == torch.uint8), mask=mptr, B=B, h=h, w=w, resize_h=rh, resize_w=rw,
             top=top, left=left, H=H, W=W, channels=self.channels, mean=list(self.mean), std=list(self.std), x=x.data_ptr(),
             target=target.data_ptr() if target is not None else None,
             interpolation=0 if self.interpolation == 'bilinear' else (2 if self.interpolation == 'cubic' and images.dtype == torch.uint8 else 1),
             pad_mode=PAD_METHODS.index(self.pad_method))
        check(fn(ctypes.byref(s), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'preprocess')
        return x, target

    def _check_pad(self, h, w, rh, rw, top, left, H, W):
        """reflect-101 reflects once: every side's pad is at most n - 1 pixels of the (resized) tile"""
        if self.pad_method != 'reflect':
            return
        nh, nw = rh or h, rw or w
        if max(top, H - top - nh) > nh - 1 or max(left, W - left - nw) > nw - 1:
            raise SaltError("DevicePreprocessor: pad_method='reflect' needs a pad of at most n - 1 pixels on every side "
                            '(tile %dx%d, pads %d/%d and %d/%d)' % (nh, nw, top, H - top - nh, left, W - left - nw))

    def _augment(self, images, masks, params, debug):
        if images.dtype != torch.uint8:
            raise SaltError('DevicePreprocessor: augmentation takes uint8 tiles (the reference augments uint8 arrays)')
        images = images.contiguous()
        B, h, w = images.shape
        if h > 128 or w > 128:
            raise SaltError('DevicePreprocessor: augmentation takes tiles up to 128x128 (got %dx%d)' % (h, w))
        rh, rw, top, left, H, W = self.geometry(h, w)
        self._check_pad(h, w, rh, rw, top, left, H, W)
        dev = images.device
        x = torch.empty((B, self.channels, H, W), dtype=torch.float32, device=dev)
        target, mptr = None, None
        if masks is not None:
            masks = masks.contiguous().to(torch.uint8)
            if tuple(masks.shape) != (B, h, w):
                raise SaltError('DevicePreprocessor: masks must be [B,h,w] like the images')
            target = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
            mptr = masks.data_ptr()
        if params is not None:
            params = params.contiguous()
            if params.dtype != torch.float32 or tuple(params.shape) != (B, N_PARAMS):
                raise SaltError('DevicePreprocessor: params must be fp32 [B, %d]' % N_PARAMS)
            rec = params
        else:
            rec = torch.empty((B, N_PARAMS), dtype=torch.float32, device=dev) if self.record_params else None
        dbg = {}
        if debug:
            dbg = {'geo_img': torch.empty((B, h, w), dtype=torch.uint8, device=dev), 'geo_mask': torch.empty((B, h, w), dtype=torch.uint8, device=dev),
                   'gray': torch.empty((B, H, W), dtype=torch.uint8, device=dev)}
        fn, S = OP_FUNCS['salt_augment_preprocess']
        s = S()
        self.augment.fill(s.cfg)
        fill(s, img=images.data_ptr(), mask=mptr, B=B, h=h, w=w, resize_h=rh, resize_w=rw, top=top, left=left, H=H, W=W,
             channels=self.channels, mean=list(self.mean), std=list(self.std), x=x.data_ptr(),
             target=target.data_ptr() if target is not None else None, seed=self.seed & (2 ** 64 - 1), counter=self.counter,
             params=rec.data_ptr() if rec is not None else None, params_given=int(params is not None),
             geo_img=dbg['geo_img'].data_ptr() if debug else None, geo_mask=dbg['geo_mask'].data_ptr() if debug else None,
             gray=dbg['gray'].data_ptr() if debug else None, pad_mode=PAD_METHODS.index(self.pad_method))
        check(fn(ctypes.byref(s), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'augment_preprocess')
        self.counter += 1
        self._params = rec
        return (x, target, dbg) if debug else (x, target)

    def last_params(self, raw=False):
        """the parameters of the last augmented call: decoded (dict of per-image numpy arrays) or ``raw`` ([B, 64] fp32 on the GPU);
        needs record_params=True (or a replayed record)"""
        if self._params is None:
            raise SaltError('DevicePreprocessor: no params recorded (construct with augment and record_params=True)')
        return self._params if raw else decode_params(self._params)


def pil_resize_table(n_in, n_out):
    """PIL's BILINEAR resample coefficients of one axis (Resample.c precompute_coeffs) in float64, as salt_mask_resize takes them:
    (start [n_out] int32, length [n_out] int32, weights [n_out, taps] float64).  scale = n_in / n_out, support = max(scale, 1),
    centre = (x + 0.5) scale, window [max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n_in)), triangle weights
    of (tap - centre + 0.5) * (1 / support), normalised to sum 1."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 1.0 * fs, 1.0 / fs
    taps = int(np.ceil(support)) * 2 + 1
    start, length = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    weights = np.zeros((n_out, taps), np.float64)
    for x in range(n_out):
        centre = (x + 0.5) * scale
        lo, hi = max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n_in)
        ww = 0.0
        for t in range(hi - lo):
            weights[x, t] = max(1.0 - abs((t + lo - centre + 0.5) * ss), 0.0)
            ww += weights[x, t]
        if ww != 0.0:
            weights[x, :hi - lo] *= 1.0 / ww
        start[x], length[x] = lo, hi - lo
    return start, length, weights


class StackingPreprocessor:
    """The second-level loader (loaders.py:564-579, ImageSegmentationLoaderStacking) on the device.  Callable:
    (stacks [B,h,w,M] or [B,M,h,w] fp32, masks [B,h,w] uint8 | None) on the GPU -> (X [B,M,H,W], target [B,2,H,W] | None).

    X is ResizeArray + to_tensor_stacking (skimage's order-1 'constant' resize of every first-level map, float64, one rounding to
    fp32: ``salt_stack_resize``); the target is the PIL BILINEAR resize of (mask == k), k in (0, 1), the two classes resized
    independently (``salt_mask_resize``).  ``layout``: 'hwm' ([B,h,w,M], what np.stack(maps, axis=-1) per tile gives, utils.py:580),
    'mhw' ([B,M,h,w] planes) or None = by shape (the last axis is M when it is the only one that differs from a square tile; ambiguous
    shapes must say).  A depth-conditioned network takes D / 1000 beside X as before."""

    def __init__(self, size=(128, 128), layout=None):
        if layout not in (None, 'hwm', 'mhw'):
            raise SaltError("StackingPreprocessor: layout %r ('hwm' | 'mhw' | None)" % (layout,))
        self.size, self.layout = (int(size[0]), int(size[1])), layout
        self._tables = {}

    def _layout(self, shape):
        if self.layout is not None:
            return self.layout
        _, a, b, c = shape
        if a == b and b != c:
            return 'hwm'
        if b == c and a != b:
            return 'mhw'
        raise SaltError('StackingPreprocessor: cannot tell [B,h,w,M] from [B,M,h,w] for shape %s: pass layout=' % (tuple(shape),))

    def tables(self, h, w, device):
        """the per-axis PIL tables of (h, w) -> size on ``device``, built once"""
        key = (h, w, str(device))
        if key not in self._tables:
            dev = []
            for start, length, weights in (pil_resize_table(h, self.size[0]), pil_resize_table(w, self.size[1])):
                dev.append((torch.from_numpy(start).to(device), torch.from_numpy(length).to(device), torch.from_numpy(weights).to(device)))
            self._tables[key] = dev
        return self._tables[key]

    def __call__(self, stacks, masks=None):
        if not torch.is_tensor(stacks) or not stacks.is_cuda or (masks is not None and (not torch.is_tensor(masks) or not masks.is_cuda)):
            raise SaltError('StackingPreprocessor: tensors must live on the GPU (there is no CPU path)')
        if stacks.dim() != 4 or stacks.dtype != torch.float32:
            raise SaltError('StackingPreprocessor: stacks must be fp32 [B,h,w,M] or [B,M,h,w]')
        stacks = stacks.contiguous()
        B = stacks.shape[0]
        if self._layout(stacks.shape) == 'hwm':
            h, w, M = stacks.shape[1:]
            strides = dict(sb=h * w * M, sr=w * M, sc=M, sm=1)
        else:
            M, h, w = stacks.shape[1:]
            strides = dict(sb=M * h * w, sr=w, sc=1, sm=h * w)
        if not 1 <= M <= 64:
            raise SaltError('StackingPreprocessor: 1 <= M <= 64 first-level maps (got %d)' % M)
        H, W = self.size
        dev = stacks.device
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        x = torch.empty((B, M, H, W), dtype=torch.float32, device=dev)
        fn, S = OP_FUNCS['salt_stack_resize']
        check(fn(ctypes.byref(fill(S(), x=stacks.data_ptr(), B=B, h=h, w=w, M=M, H=H, W=W, y=x.data_ptr(), **strides)), stream), 'stack_resize')
        if masks is None:
            return x, None
        if tuple(masks.shape) != (B, h, w):
            raise SaltError('StackingPreprocessor: masks must be [B,h,w] like the maps')
        masks = masks.contiguous().to(torch.uint8)
        (rs, rl, rw), (cs, cl, cw) = self.tables(h, w, dev)
        target = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
        fn, S = OP_FUNCS['salt_mask_resize']
        check(fn(ctypes.byref(fill(S(), mask=masks.data_ptr(), B=B, h=h, w=w, H=H, W=W, row_start=rs.data_ptr(), row_len=rl.data_ptr(),
                                   row_w=rw.data_ptr(), row_taps=rw.shape[1], col_start=cs.data_ptr(), col_len=cl.data_ptr(),
                                   col_w=cw.data_ptr(), col_taps=cw.shape[1], target=target.data_ptr())), stream), 'mask_resize')
        return x, target


def emptiness_target(is_not_empty):
    """loaders.py:778-783 (preprocess_emptiness_target) for a batch: per tile the float target [2,1,1] of the emptiness classifier,
    [1, 0] for an empty mask and [0, 1] otherwise.  ``is_not_empty``: [B] of {0, 1} (array or tensor) -> [B,2,1,1] float32."""
    x = torch.as_tensor(np.asarray(is_not_empty.cpu() if torch.is_tensor(is_not_empty) else is_not_empty)).reshape(-1).to(torch.float32)
    return torch.stack([(x == 0).to(torch.float32), x], 1).reshape(-1, 2, 1, 1)
