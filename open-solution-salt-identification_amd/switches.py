"""The SALT_* environment switches of the package: one table, one accessor.

Every switch the Python side reads is listed here with its default, its parser and what it selects; ``get`` is the only place of the
package that reads a SALT_* variable.  Nothing is cached: the tests set a switch (``monkeypatch.setenv``) and then build a fresh model
in the same process.  The engine reads switches while it BUILDS (Engine / Graph / CompiledNet / SegmentationModel / DataParallel
construction), never on the per-step path - with one exception, SALT_FORCE_DP_PATH, which bench.py toggles between steps of a live
model.  The library's own switches (``getenv`` in csrc/*.hip) are listed with these in DESIGN.md's switch table; a CPU test keeps the
three in step."""
import os


def _nonempty(raw):             # "set to anything" switches (SALT_NO_*=1)
    return bool(raw)


def _not0(raw):                 # default-on switches: '0' turns the path off
    return raw != '0'


def _on(raw):                   # default-off switches: anything but '' / '0' turns the path on
    return raw not in ('', '0')


SWITCHES = {
    # name: (default, parser, meaning)
    'SALT_LIB': ('', str, 'path of a libsaltnet_hip.so build variant to load instead of the package\'s own (tools/build_variant.sh)'),
    'SALT_DTYPE': ('f32', str, 'compute dtype of a network that does not name one (f32 | bf16)'),
    'SALT_STEP_GRAPH': (None, lambda raw: bool(int(raw)), '1 / 0: replay the one-GPU training step as a hipGraph; unset: training_config[\'step_graph\']'),
    'SALT_BN_FIN': (2, int, 'how train-mode BatchNorm sums travel: 2 fp64 shard atomics finalized by the consumer, 1 finalized in the producing launch, 0 per-tile partials (fixed summation order)'),
    'SALT_SE_SHARDS': (True, _not0, '0: scSE per-image sums through per-part partials (fixed summation order) instead of the fp64 shards'),
    'SALT_FWD_BN_FOLD': (False, _on, '1: BatchNorm apply + ReLU folded into the consuming convolution\'s loader; such a graph is forward-only'),
    'SALT_NO_PLANAR': (False, _nonempty, 'hypercolumn stored as channel-interleaved rows instead of dense planes'),
    'SALT_NO_SHORTCUT_FIRST': (False, _nonempty, 'projection shortcut emitted after the main branch, as the reference orders it'),
    'SALT_NO_RES_FOLD': (False, _nonempty, 'residual add + ReLU as separate launches instead of the BatchNorm apply\'s epilogue'),
    'SALT_BNB_SEC': (True, _not0, '0: a projection shortcut\'s BatchNorm backward keeps its own reduction pass'),
    'SALT_HEAD_BN': (True, _not0, '0: final BatchNorm apply and 1x1 logit head as separate launches'),
    'SALT_HYPER_FACTOR': (4, int, 'hypercolumn levels up-sampled by at least this factor enter the final convolution factored (0: none)'),
    'SALT_SE_IN_BN': (True, _not0, '0: scSE reads a materialised activation instead of applying BatchNorm + ReLU itself'),
    'SALT_SE_FC_SIDE': (True, _not0, '0: scSE backward\'s FC weight gradients on the main stream'),
    'SALT_SE_BNB': (True, _not0, '0: scSE backward does not carry the BatchNorm-backward sums of its input\'s producer'),
    'SALT_SE_RES_IN_BN': (True, _not0, '0: the SE-ResNet block tail reads the materialised BatchNorm output instead of applying scale / shift itself (measured 0.2 ms per step slower, DESIGN 16; tools/seresnet_bench.py)'),
    'SALT_RCCL_MAX_NCHANNELS': (0, int, '> 0: export NCCL_MAX_NCHANNELS=<n> before the process group is created'),
    'SALT_NO_PIN': (False, _nonempty, 'leave the process\'s CPU affinity alone'),
    'SALT_FORCE_DP_PATH': (False, _nonempty, 'one rank runs the bucketed all-reduce backward (bench.py, tools/dp_overhead.py)'),
}


def get(name):
    """Value of switch ``name``: parsed from the environment as it is NOW, or the table's default.  An unknown name raises."""
    try:
        default, parse, _ = SWITCHES[name]
    except KeyError:
        raise KeyError('%s is not a switch of this package (switches.SWITCHES)' % name) from None
    raw = os.environ.get(name)
    return default if raw is None else parse(raw)
