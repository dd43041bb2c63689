"""Drop-in for the reference's ``common_blocks/models.py`` on the U-Net hot path.

Same names and call contract as the reference (models.py:15-208,289-340):
  ARCHITECTURES registry, SegmentationModel(architecture_config, training_config, callbacks_config) with
  fit / _fit_loop / transform / _transform / set_model / set_loss / load (+ persist, fit_transform from the
  un-vendored steppy-toolkit ``Model`` base, restated from its call sites), weight_regularization,
  lovasz_loss, mixed_dice_bce_loss.

What is different underneath: ``self.model`` is a HipNetwork (compiled static HIP programs, NHWC, flat
parameter buffers), the optimizer is one fused Adam kernel, ``_fit_loop`` runs forward -> loss -> backward
-> (bucketed RCCL all-reduce overlapped with backward) -> Adam without touching torch autograd, and
``nn.DataParallel`` (models.py:81-85) is replaced by one process per GPU (parallel.py).
"""

import functools

import numpy as np
import torch

from . import architectures as A
from . import parallel
from . import switches
from ._abi import SaltError
from .losses import LOVASZ_DEFAULTS, dice_ce_params, lovasz_params, lovasz_loss, lovasz_softmax_loss, mixed_dice_bce_loss, mixed_dice_cross_entropy_loss
from .optim import FusedAdam, weight_regularization

ARCHITECTURES = {
    'UNetResNet': {'model': A.UNetResNet,
                   'model_config': {'encoder_depth': 34, 'use_hypercolumn': True, 'dropout_2d': 0.0, 'pretrained': False, 'pool0': False},
                   'init_weights': False},
    # models.py:46-50: the depth-conditioned network of main.py's USE_DEPTH switch (SegmentationModelWithDepth)
    'UNetResNetWithDepth': {'model': A.UNetResNetWithDepth,
                            'model_config': {'encoder_depth': 34, 'use_hypercolumn': True, 'dropout_2d': 0.0, 'pretrained': False},
                            'init_weights': False},
    # models.py:20-24 with `pretrained` off, like the other entries here: SE-ResNet50 encoders (csrc/se_res.hip)
    'UNetSeResNet': {'model': A.UNetSeResNet,
                     'model_config': {'encoder_depth': 50, 'use_hypercolumn': True, 'dropout_2d': 0.0, 'pretrained': False, 'pool0': False},
                     'init_weights': False},
    # models.py:25-29 with `pretrained` off: SE-ResNeXt50 (32x4d) encoders (csrc/conv_group.hip + csrc/se_res.hip)
    'UNetSeResNetXt': {'model': A.UNetSeResNetXt,
                       'model_config': {'encoder_depth': 50, 'use_hypercolumn': True, 'dropout_2d': 0.0, 'pretrained': False, 'pool0': False},
                       'init_weights': False},
    # models.py:30-34 with `pretrained` off: DenseNet-121 encoders (csrc/dense.hip)
    'UNetDenseNet': {'model': A.UNetDenseNet,
                     'model_config': {'encoder_depth': 121, 'use_hypercolumn': True, 'dropout_2d': 0.0, 'pretrained': False, 'pool0': False},
                     'init_weights': False},
    # models.py:41-45 with `pretrained` off: pyramid pooling on the /16 map (csrc/psp.hip); dropout_2d is the class default and an identity
    'PSPNet': {'model': A.PSPNet,
               'model_config': {'encoder_depth': 34, 'pretrained': False, 'use_hypercolumn': True, 'pool0': False},
               'init_weights': False},
    # models.py:35-40 with `pretrained` off: global convolutional networks on the /2 .. /16 maps (csrc/gcn.hip)
    'LargeKernelMatters': {'model': A.LargeKernelMatters,
                           'model_config': {'encoder_depth': 34, 'pretrained': False, 'kernel_size': 9, 'internal_channels': 21,
                                            'dropout_2d': 0.0, 'use_relu': True, 'pool0': False},
                           'init_weights': False},
    # unet_models.py zoo (named by BASELINE.json's north_star; not wired into the reference's registry)
    'TernausUNetResNet': {'model': A.TernausUNetResNet,
                          'model_config': {'encoder_depth': 34, 'num_filters': 32, 'dropout_2d': 0.0, 'pretrained': False, 'is_deconv': True},
                          'init_weights': False},
    'UNetResNet152': {'model': A.UNetResNet,
                      'model_config': {'encoder_depth': 152, 'use_hypercolumn': True, 'dropout_2d': 0.0, 'pretrained': False, 'pool0': False},
                      'init_weights': False},
    'SaltUNet': {'model': A.SaltUNet, 'model_config': {'dropout_2d': 0.0, 'pretrained': False, 'is_deconv': True}, 'init_weights': False},
    'SaltLinkNet': {'model': A.SaltLinkNet, 'model_config': {'dropout_2d': 0.0, 'pretrained': False, 'is_deconv': True}, 'init_weights': False},
    # models.py:59-63: the per-tile "any salt at all" classifier of empty_vs_non_empty.py
    'EmptinessClassifier': {'model': A.EmptinessClassifier,
                            'model_config': {'encoder_depth': 18, 'pretrained': False},
                            'init_weights': False},
    # models.py:51-58: the second-level networks of main.py's SECOND_LEVEL switch (loader_mode 'stacking').  'init_weights' is recorded as
    # the reference has it and has no effect: its set_model replaces the initialiser with a no-op too (models.py:184)
    'StackingFCN': {'model': A.StackingFCN,
                    'model_config': {'input_model_nr': 32, 'filter_nr': 32, 'dropout_2d': 0.0},
                    'init_weights': True},
    'StackingFCNWithDepth': {'model': A.StackingFCNWithDepth,
                             'model_config': {'input_model_nr': 32, 'filter_nr': 32, 'dropout_2d': 0.0},
                             'init_weights': True},
    'VanillaUNet': {'model': A.VanillaUNet, 'model_config': {'in_channels': 1, 'base_filters': 16, 'levels': 4}, 'init_weights': False},
}


def sigmoid(x):                      # utils.py:173-174
    return 1. / (1 + np.exp(-x))


def softmax(X, axis=0):
    y = np.exp(X - np.max(X, axis=axis, keepdims=True))
    return y / np.sum(y, axis=axis, keepdims=True)


def get_list_of_image_predictions(batch_predictions):      # utils.py:316-320
    return [img for batch in batch_predictions for img in list(batch)]


from .callbacks import Callback, CallbackList, callbacks_network, score_validation, score_validation_emptiness  # noqa: E402,F401  (callbacks.py surface)


class Model:
    """steppy-toolkit 0.1.5 ``toolkit.pytorch_transformers.models.Model`` restated from its call sites
    (models.py:6,67-70; callbacks.py:42-48; utils.py:444-467): holds the three configs, fit_transform, persist."""

    def __init__(self, architecture_config, training_config, callbacks_config):
        self.architecture_config = architecture_config
        self.training_config = training_config
        self.callbacks_config = callbacks_config
        self.model = None
        self.optimizer = None
        self.loss_function = None
        self.loss_params = None               # weights of 'dice_ce' / options of the Lovasz losses (model_params['loss_params']): set_loss writes, _fused_step reads
        self.callbacks = None
        self.validation_loss = {}
        self.validation_masks = None          # (loader_mode, original-size masks) set by ValidationMonitor.set_params, or None

    @property
    def output_names(self):
        return [name for (name, _, _) in self.loss_function]

    def fit_transform(self, *args, **kwargs):
        return self.fit(*args, **kwargs).transform(*args, **kwargs)

    def score_validation(self, validation_datagen):
        """{'sum', 'iou', 'iout'} of one pass over the validation generator (callbacks.py:503-568), threshold sweep on the GPU; a
        classifier network (``is_classifier``) is scored as {'sum', 'auc'} (callbacks.py:662-674)."""
        if getattr(self.model, 'is_classifier', False):
            return score_validation_emptiness(self, validation_datagen)
        if self.validation_masks is not None:                 # loader modes 'resize' / 'stacking' with meta_valid masks
            return score_validation(self, validation_datagen, loader_mode=self.validation_masks[0], y_true=self.validation_masks[1])
        return score_validation(self, validation_datagen)

    def persist(self, filepath):
        """Reference checkpoints are written through nn.DataParallel, so every key carries a 'module.' prefix
        (models.py:199-204, callbacks.py:776-792); keep that format.  One process per GPU: only rank 0 writes (the replicas are
        identical up to their per-rank BatchNorm running statistics, and DataParallel keeps device 0's as well)."""
        dp = getattr(self, 'dp', None)
        if dp is not None and dp.rank != 0:
            return
        self.model.eval()
        sd = {'module.' + k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        torch.save(sd, filepath)
        self.model.train()


class SegmentationModel(Model):
    takes_depth = False          # batches are (X, *targets); SegmentationModelWithDepth: (X, D, *targets)

    def __init__(self, architecture_config, training_config, callbacks_config):
        super().__init__(architecture_config, training_config, callbacks_config)
        self.activation_func = self.architecture_config['model_params']['activation']
        self.set_model()
        self.set_loss()
        self.weight_regularization = weight_regularization
        self.optimizer = FusedAdam(self.weight_regularization(self.model, **architecture_config['regularizer_params']),
                                   model=self.model, **architecture_config['optimizer_params'])
        self.callbacks = callbacks_network(self.callbacks_config)
        self.dp = parallel.DataParallel.from_env()
        # opt-in: one-GPU training replays the whole step as a hipGraph (training_config['step_graph'] / SALT_STEP_GRAPH=1);
        # the eager two-stream step is faster
        sg = switches.get('SALT_STEP_GRAPH')
        self.step_graph = bool((training_config or {}).get('step_graph', False)) if sg is None else sg

    # ------------------------------------------------------------------ reference surface
    def set_model(self):
        mp = self.architecture_config['model_params']
        config = ARCHITECTURES[mp['architecture']]
        model_config = dict(config['model_config'])
        # the second-level networks: how many first-level maps are stacked is the user's data, not the registry's (the reference makes
        # its users edit the registry entry)
        model_config.update({k: mp[k] for k in ('input_model_nr', 'filter_nr') if k in mp and k in model_config})
        self.model = config['model'](num_classes=mp['out_channels'], **model_config)
        if getattr(self.model, 'uses_depth', False) and not self.takes_depth:
            raise SaltError('%s is depth-conditioned: train it with SegmentationModelWithDepth on (X, D, target) batches' % mp['architecture'])
        if 'compute_dtype' in mp:
            self.model.set_compute_dtype(mp['compute_dtype'])
        if 'align_corners' in mp:            # True: bilinear up-sampling as torch 0.3.1 (the reference's pinned version) evaluated it
            self.model.set_align_corners(mp['align_corners'])
        self._initialize_model_weights = lambda: None

    def set_loss(self):
        mp = self.architecture_config['model_params']
        self.loss_params = None
        if self.activation_func == 'softmax':
            if getattr(self.model, 'is_classifier', False):
                raise SaltError('%s is a classifier: its emptiness path (pooled head, ROC-AUC validation) is sigmoid-only' % mp['architecture'])
            choices = {'lovasz_softmax': lovasz_softmax_loss, 'dice_ce': mixed_dice_cross_entropy_loss}
            if 'loss' not in mp:
                # the reference defines no softmax loss either (models.py:174-176); nothing is chosen on the user's behalf
                raise NotImplementedError("No softmax loss defined: name one in model_params['loss'] (%s)" % ' | '.join(choices))
            name = mp['loss']
            if name not in choices:
                raise SaltError("activation 'softmax' trains with loss %s, got %r" % (' | '.join(choices), name))
            if not 2 <= mp['out_channels'] <= 4:
                raise SaltError('the softmax losses take 2 .. 4 output channels, got %d' % mp['out_channels'])
            loss_function = choices[name]
            if name == 'dice_ce' and mp.get('loss_params'):
                # optional weights of Dice + cross entropy: dice_weight / cross_entropy_weight / smooth.  The fused step reads them
                # from here (they are part of the loss program's cache key); the same values reach the autograd-bridge path
                dice_ce_params(mp['loss_params'])
                self.loss_params = dict(mp['loss_params'])
                loss_function = functools.partial(mixed_dice_cross_entropy_loss, **self.loss_params)
                loss_function.native_kind = 'dice_ce'
        elif self.activation_func == 'sigmoid':
            name = self.architecture_config['model_params'].get('loss', 'lovasz')
            loss_function = {'lovasz': lovasz_loss, 'bce_dice': mixed_dice_bce_loss}[name]
        else:
            raise Exception('Only softmax and sigmoid activations are allowed')
        if name in LOVASZ_DEFAULTS and mp.get('loss_params'):
            # the options of the Lovasz losses: per_image / ignore (/ only_present), read by the fused step like the weights above
            lovasz_params(name, mp['loss_params'])
            self.loss_params = dict(mp['loss_params'])
            loss_function = functools.partial(loss_function, **self.loss_params)
            loss_function.native_kind = name
        self.loss_function = [('mask', loss_function, 1.0)]

    def fit(self, datagen, validation_datagen=None, meta_valid=None):
        self._initialize_model_weights()
        self._to_device()
        self.model.train()
        self.dp.broadcast_parameters(self.model)
        self.callbacks.set_params(self, validation_datagen=validation_datagen, meta_valid=meta_valid)
        self.callbacks.on_train_begin()
        batch_gen, steps = datagen
        for epoch_id in range(self.training_config['epochs']):
            self.callbacks.on_epoch_begin()
            for batch_id, data in enumerate(batch_gen):
                self.callbacks.on_batch_begin()
                metrics = self._fit_loop(data)
                self.callbacks.on_batch_end(metrics=metrics)
                if batch_id == steps:
                    break
            self.callbacks.on_epoch_end()
            if self.dp.any_rank(self.callbacks.training_break()):       # every rank leaves the loop in the same epoch
                break
        self.callbacks.on_train_end()
        return self

    def _to_device(self):
        if not torch.cuda.is_available():
            raise SaltError('SegmentationModel needs a GPU: the hot path is hand-written HIP with no CPU fallback')
        dev = torch.device('cuda', torch.cuda.current_device())
        if next(self.model.parameters()).device != dev:
            self.model.to(dev)
        return dev

    def _fit_loop(self, data):
        dev = self._to_device()
        X = data[0].to(dev, non_blocking=True)
        targets = [t.to(dev, non_blocking=True) for t in data[1:]]
        self.optimizer.zero_grad()
        if len(self.loss_function) != 1:
            raise NotImplementedError('multi-output losses are off the reference default path')
        (name, loss_function, weight), target = self.loss_function[0], targets[0]
        kind = getattr(loss_function, 'native_kind', None)
        if kind is not None:
            batch_loss = self._fused_step(X, target, kind, weight)     # (optimizer.step() follows below)
        else:                                   # any torch-differentiable loss: through the autograd bridge
            outputs_batch = self.model(X)
            batch_loss = loss_function(outputs_batch, target) * weight
            batch_loss.backward()
            self.dp.allreduce_gradients(self.model.engine(), self.optimizer)   # SUM over ranks; Adam's grad_scale carries 1/world
        if getattr(self, '_graph_stepped', False):
            self._graph_stepped = False                  # Adam ran inside the captured step
        else:
            self.optimizer.step()
        return {'sum': batch_loss}

    def _fused_step(self, X, target, kind, weight, D=None):
        """``D``: the depth input [B,1] of a depth-conditioned network (SegmentationModelWithDepth), fp32 on X's device."""
        eng = self.model.engine(X.device)
        eng.loss_params = self.loss_params
        if kind in LOVASZ_DEFAULTS and self.dp._active() and not dict(self.loss_params or {}).get('per_image', True):
            # every rank would sort its own shard; the reference computes the batch-flat loss on the gathered batch
            raise SaltError("loss %r with per_image=False is one sort over the whole batch: it does not train data-parallel" % kind)
        # 'first step of a shape ran eagerly' is remembered ON the engine (a rebuilt engine starts empty - no recycled id() can skip it)
        if self.step_graph and not self.dp._active() and (tuple(X.shape), kind) in eng.eager_done:
            # the whole step (pack, forward, loss, backward, Adam; both streams) replayed as ONE hipGraph launch (the first step of
            # a shape runs eagerly: lazy one-time work - kernel attributes, workspace allocation - must not fall into the capture)
            net = eng.net(tuple(X.shape), True)
            net.x.copy_(X)
            if (net.d is None) != (D is None):
                raise SaltError('depth input %s' % ('missing' if D is None else 'given to a network without one'))
            if D is not None:
                net.d.copy_(D)
            net.target.copy_(target[:, :net.logits.shape[1]])
            self.optimizer.grad_scale = 1.0
            eng.run_step_graph(net, kind, weight, self.optimizer)
            self._graph_stepped = True
            return net.loss[0].clone()
        # round 6: no torch copy / fill / clone kernel inside the step.  A resident fp32 batch / target is READ IN PLACE (the programs'
        # pointer fields are re-pointed for the duration of the enqueue calls, CompiledNet.bind), the loss scalar is written straight
        # into a fresh 0-dim tensor that is returned as is (read lazily by whoever wants the number: callbacks.TrainingMonitor).
        net = eng.net(tuple(X.shape), True)
        K = net.logits.shape[1]
        loss_prog = net.loss_program(kind, weight)
        bx = net.bindable(X, net.x)
        bt = net.bindable(target, net.target)
        bd = D is not None and net.d is not None and net.bindable(D, net.d)
        loss_t = torch.empty((1,), dtype=torch.float32, device=X.device)
        try:
            net.bind(x=X if bx else None, target=target if bt else None, loss=loss_t, **({'d': D} if bd else {}))
            eng.forward(X if bx else X.contiguous().float(), True, bound=bx, d=D, d_bound=bd)
            if not bt:
                net.target.copy_(target[:, :K])
            loss_prog.run()
            self.dp.backward(eng, net, self.optimizer)
        finally:
            net.bind()                           # back to the static buffers (tools / tests that run the programs on their own)
        eng.eager_done.add((tuple(X.shape), kind))
        return loss_t[0]

    def transform(self, datagen, validation_datagen=None, *args, **kwargs):
        outputs = self._transform(datagen, validation_datagen)
        for name, prediction in outputs.items():
            if self.activation_func == 'softmax':
                outputs[name] = [softmax(single_prediction, axis=0) for single_prediction in prediction]
            elif self.activation_func == 'sigmoid':
                outputs[name] = [sigmoid(np.squeeze(mask)) for mask in prediction]
            else:
                raise Exception('Only softmax and sigmoid activations are allowed')
        return outputs

    def _transform(self, datagen, validation_datagen=None, **kwargs):
        dev = self._to_device()
        self.model.eval()
        batch_gen, steps = datagen
        outputs = {}
        with torch.no_grad():
            for batch_id, data in enumerate(batch_gen):
                X = data[0] if isinstance(data, (list, tuple)) else data
                outputs_batch = self.model(X.to(dev))
                outputs.setdefault(self.output_names[0], []).append(outputs_batch.cpu().numpy())
                if batch_id == steps:
                    break
        self.model.train()
        return {'{}_prediction'.format(name): get_list_of_image_predictions(outs) for name, outs in outputs.items()}

    def load(self, filepath):
        """Reference checkpoints ('module.'-prefixed keys, models.py:196-208).  Which bilinear semantics the loaded weights get is the
        network's ``align_corners`` (architecture_config['model_params']['align_corners'], default False = torch >= 0.4, the oracle's):
        a checkpoint trained in the reference's own environment (torch 0.3.1) expects True - nothing in the file says which, so the
        caller states it."""
        self.model.eval()
        sd = torch.load(filepath, map_location='cpu')
        sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
        self.model.load_state_dict(sd)
        if torch.cuda.is_available():
            self._to_device()
        return self


class SegmentationModelWithDepth(SegmentationModel):
    """models.py:211-286: the trainer of main.py's USE_DEPTH switch.  Batches are ``(X, D, *targets)`` with D [B,1] the tiles' depths
    (loaders.py:310-311: z / 1000); the network is called as ``model(X, D)``.  Native losses run through the fused step, any other
    loss through the autograd bridge; everything else (load, persist, data-parallel buckets, FusedAdam) is SegmentationModel's - the two
    gate parameters are ordinary live parameters of the flat buffers."""

    takes_depth = True

    def set_model(self):
        super().set_model()
        if not getattr(self.model, 'uses_depth', False):
            raise SaltError('SegmentationModelWithDepth needs a depth-conditioned architecture (UNetResNetWithDepth, StackingFCNWithDepth), got %s'
                            % self.architecture_config['model_params']['architecture'])

    def _depth(self, D, X):
        D = D.to(X.device, non_blocking=True)
        if tuple(D.shape) != (X.shape[0], 1):
            raise SaltError('depth batch must be [%d, 1], got %s' % (X.shape[0], tuple(D.shape)))
        return D if D.dtype == torch.float32 else D.float()

    def _fit_loop(self, data):
        dev = self._to_device()
        X = data[0].to(dev, non_blocking=True)
        D = self._depth(data[1], X)
        targets = [t.to(dev, non_blocking=True) for t in data[2:]]
        self.optimizer.zero_grad()
        if len(self.loss_function) != 1:
            raise NotImplementedError('multi-output losses are off the reference default path')
        (name, loss_function, weight), target = self.loss_function[0], targets[0]
        kind = getattr(loss_function, 'native_kind', None)
        if kind is not None:
            batch_loss = self._fused_step(X, target, kind, weight, D=D)
        else:
            outputs_batch = self.model(X, D)
            batch_loss = loss_function(outputs_batch, target) * weight
            batch_loss.backward()
            self.dp.allreduce_gradients(self.model.engine(), self.optimizer)
        if getattr(self, '_graph_stepped', False):
            self._graph_stepped = False
        else:
            self.optimizer.step()
        return {'sum': batch_loss}

    def _transform(self, datagen, validation_datagen=None, **kwargs):
        dev = self._to_device()
        self.model.eval()
        batch_gen, steps = datagen
        outputs = {}
        with torch.no_grad():
            for batch_id, data in enumerate(batch_gen):
                X = data[0].to(dev)
                outputs_batch = self.model(X, self._depth(data[1], X))
                outputs.setdefault(self.output_names[0], []).append(outputs_batch.cpu().numpy())
                if batch_id == steps:
                    break
        self.model.train()
        return {'{}_prediction'.format(name): get_list_of_image_predictions(outs) for name, outs in outputs.items()}
