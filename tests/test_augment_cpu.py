"""CPU tests of the training augmentation's host side and of its numpy restatement (tests/aug_reference.py)."""
import dataclasses

import numpy as np
import pytest

import aug_reference as R


def test_sharpen_and_emboss_matrices_on_a_hand_computed_tile():
    assert np.array_equal(R.sharpen_matrix(), np.array([[-.5, -.5, -.5], [-.5, 5, -.5], [-.5, -.5, -.5]], np.float32))
    assert np.array_equal(R.emboss_matrix(), np.array([[-1, -.5, 0], [-.5, 1, .5], [0, .5, 1]], np.float32))
    a = np.zeros((5, 5), np.uint8)
    a[2, 2] = 100
    a[1, 3] = 40
    s = R.conv3x3(a, R.sharpen_matrix())
    # centre: 5 * 100 - 0.5 * 40 = 480 -> 255; (1, 3): 5 * 40 - 0.5 * 100 = 150; (2, 3): -0.5 * (100 + 40) < 0 -> 0
    assert s[2, 2] == 255 and s[1, 3] == 150 and s[2, 3] == 0 and s[0, 0] == 0
    e = R.conv3x3(a, R.emboss_matrix())
    # (1, 1): the bottom-right neighbour (2, 2) weighs 1 -> 100; (3, 3): top-left weighs -1 -> 0; (2, 2): 100 + 0.5 * 0 ... - 0.5 * 40 (top-right is 0 weight)
    assert e[1, 1] == 100 and e[3, 3] == 0 and e[2, 2] == 100
    # (2, 4): left neighbour (2, 3) is 0, top-left (1, 3) = 40 weighs -1 -> 0; (0, 2): bottom-right (1, 3) weighs 1 -> 40
    assert e[2, 4] == 0 and e[0, 2] == 40
    # reflect-101 border: tap (-1, -1) is (1, 1), so at (0, 0) the -1 top-left and +1 bottom-right weights cancel (a replicated
    # border would read 0 top-left and give 10)
    b = np.zeros((5, 5), np.uint8)
    b[1, 1] = 10
    assert R.conv3x3(b, R.emboss_matrix())[0, 0] == 0
    # binary masks: Sharpen leaves them unchanged after binarising
    m = (np.random.RandomState(0).rand(20, 20) < 0.4).astype(np.uint8)
    assert np.array_equal(R.conv3x3(m, R.sharpen_matrix(), True), m)


def test_flip_and_rounding():
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(R.fliplr(a), a[:, ::-1])
    assert list(R.to_u8(np.array([-3, 0.49, 0.5, 1.5, 254.5, 300], np.float32))) == [0, 0, 1, 2, 255, 255]


def test_rng_known_answers():
    # splitmix64 from state 0: the published first outputs 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4
    assert R.mix64(0) == 0xE220A8397B1DCDAF
    assert R.mix64(R.GOLD) == 0x6E789E6AA1B965F4
    k = R.key(1234, 0, 0)
    assert k == R.mix64(R.mix64(R.mix64(1234) ^ 0) ^ 0)
    b = [R.bits(k, s) for s in range(4)]
    assert np.array_equal(R.bits_np(k, np.arange(4)), np.array(b, np.uint64))
    u = R.uniform_np(np.array(b, np.uint64))
    assert np.array_equal(u, np.array([(x >> 40) / 2.0 ** 24 for x in b], np.float32))
    assert list(R.int_np(np.array(b, np.uint64), -10, 10)) == [-10 + (((x >> 32) * 21) >> 32) for x in b]
    # integer and uniform draws cover their ranges evenly
    many = R.bits_np(k, np.arange(1024, 1024 + 200000))
    iv = R.int_np(many, -10, 10)
    assert iv.min() == -10 and iv.max() == 10
    cnt = np.bincount(iv + 10)
    assert np.all(np.abs(cnt - 200000 / 21) < 5 * np.sqrt(200000 / 21))
    uv = R.uniform_np(many)
    assert 0 <= uv.min() and uv.max() < 1 and abs(uv.mean() - 0.5) < 0.003


def test_augment_config_defaults_are_the_reference_numbers():
    import salt_amd
    from salt_amd.input_pipeline import AugmentConfig, AUG_OPS
    c = AugmentConfig()
    assert c.enable == AUG_OPS and c.enable_mask() == (1 << 12) - 1
    assert (c.p_fliplr, c.sharpen_alpha, c.sharpen_lightness, c.emboss_alpha, c.emboss_strength) == (0.5, 0.5, 1.0, 0.5, 1.0)
    assert c.rotate == (-10.0, 10.0) and c.shift == (-0.05, 0.05)
    assert (c.p_piecewise, c.piecewise_scale, c.p_perspective, c.perspective_scale) == (0.3, (0.04, 0.08), 0.3, (0.05, 0.1))
    assert (c.p_invert, c.p_contrast, c.contrast, c.p_intensity_noop) == (0.3, 0.3, (0.5, 1.5), 0.5)
    assert c.add == (-10, 10) and c.multiply == (0.95, 1.05)
    assert AugmentConfig.none().enable_mask() == 0
    assert AugmentConfig.none(enable=('fliplr', 'invert')).enable_mask() == 1 | 64
    # the bit order is the header's
    abi = salt_amd._abi
    for i, op in enumerate(AUG_OPS):
        assert abi.CONSTS['SALT_AUG_' + op.upper()] == 1 << i
    assert abi.CONSTS['SALT_AUG_PARAMS'] == R.N_PARAMS == salt_amd.input_pipeline.N_PARAMS
    assert dataclasses.is_dataclass(c)


def test_params_decoder_mirrors_the_layout():
    from salt_amd.input_pipeline import decode_params
    p = np.zeros((2, 64), np.float32)
    p[1, [0, 1, 3, 6, 7, 8, 9, 10, 43, 44, 53, 54, 55, 56, 57]] = [4, 2, 1, 1, 3.5, -0.02, 1, 0.05, 1, 0.07, 1, 1, 1.2, 3, 1.01]
    p[1, 11:43] = np.arange(32) / 100
    p[1, 45:53] = np.arange(8) / 10
    d, r = decode_params(p), R.decode(p[1])
    assert d['order'][1] == r['order'] == 4 and d['n'][1] == 2 and list(d['chosen'][1]) == [False, True, False, False]
    assert d['flip'][1] and d['angle'][1] == np.float32(3.5) and d['shift'][1] == np.float32(-0.02)
    assert d['piecewise'][1] and np.array_equal(d['piecewise_jitter'][1], r['piecewise_jitter'])
    assert d['piecewise_jitter'][1][0, 1, 0] == np.float32(0.02)          # control point (0, 1), dy
    assert d['perspective'][1] and np.array_equal(d['perspective_corners'][1], r['perspective_corners'])
    assert d['invert'][1] and d['contrast'][1] and d['contrast_alpha'][1] == np.float32(1.2)
    assert d['intensity_op'][1] == 3 and d['value'][1] == np.float32(1.01)
    assert d['order'][0] == 0 and not d['flip'][0]


def test_augment_arguments_are_validated_without_a_device():
    import salt_amd
    from salt_amd.input_pipeline import AugmentConfig, DevicePreprocessor
    with pytest.raises(salt_amd.SaltError):
        DevicePreprocessor(False, 3, augment=True)                          # the reference never augments inference batches
    with pytest.raises(salt_amd.SaltError):
        DevicePreprocessor(True, 3, augment=True, interpolation='bilinear')
    with pytest.raises(salt_amd.SaltError):
        DevicePreprocessor(True, 3, augment=AugmentConfig(enable=('fliplr', 'swirl')))
    with pytest.raises(salt_amd.SaltError):
        DevicePreprocessor(True, 3, augment='yes')
    pre = DevicePreprocessor(True, 3, augment=True, seed=7)
    assert pre.counter == 0 and pre.seed == 7
    with pytest.raises(salt_amd.SaltError):
        pre.last_params()


def test_augment_entry_point_rejects_bad_arguments_without_a_launch():
    import ctypes
    import salt_amd
    abi = salt_amd._abi
    fn, S = abi.OP_FUNCS['salt_augment_preprocess']
    s = S()
    abi.fill(s, img=1, x=1, B=1, h=129, w=101, H=256, W=256, channels=1, std=[1, 1, 1])
    assert fn(ctypes.byref(s), None) == abi.CONSTS['SALT_E_BADARG']      # over-size tile
    assert b'128' in abi.lib.salt_last_error()
    abi.fill(s, h=101, params_given=1)
    assert fn(ctypes.byref(s), None) == abi.CONSTS['SALT_E_BADARG']      # replay without a record
