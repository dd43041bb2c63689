#!/usr/bin/env python
"""Generate the F23 fixture (ensembling between models) by EXECUTING THE REFERENCE'S OWN CODE.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_ensemble.py
Same conventions as the other generators: the reference's sources through ref_import.py / make_golden.extract_functions, only .npz
data is written.  common_blocks/utils.py cannot be imported as a module (collections.Iterable, cv2, imgaug, steppy ...), so the pieces
are pulled out of the file with ``ast`` and executed unmodified against numpy, pandas and sklearn's own BaseCrossValidator, all three
present where this runs: nothing had to be restated.

  F23_ensemble
    maps [6,2,2,16,16] f32      six small probability maps (sigmoid of closed-form inputs)
    mean_f32 / mean_f64         main.py:893 `np.mean(np.array(out_of_fold_test_predictions), axis=0)` on the float32 maps, and on the
                                same maps widened to float64 (the accumulator of notebooks/prediction_average.ipynb)
    mean_k<K>_f32               the same line on the first K of them, K in (2, 3)
    stack_hwm [2,16,16,6]       utils.py:568 + 580: image[1, :, :] of every model, np.stack(axis=-1), per tile
    kfold_values [23]           values with ties; kfold_<n>_train_<s> / kfold_<n>_test_<s>: KFoldBySortedValue(n).split(values), n in
                                (3, 5, 30): 30 splits of 23 samples leave the last folds empty
    masks_1x1 [5,1,1], masks_3x7 [5,3,7], masks_101 [3,101,101]   uint8 masks; rle_flat / rle_offsets: run_length_encoding of every
                                mask in that order; sub_ids / sub_rle: the rows of create_submission over all of them
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import closed_form as CF          # noqa: E402
import ref_import as R            # noqa: E402
from make_golden import extract_functions, save          # noqa: E402


def main():
    assert R.reference_available(), 'reference not mounted'
    import pandas as pd
    from sklearn.model_selection import BaseCrossValidator
    ns = {'np': np, 'pd': pd, 'BaseCrossValidator': BaseCrossValidator}
    extract_functions('common_blocks/utils.py', {'run_length_encoding', 'run_length_decoding', 'create_submission', 'KFoldBySortedValue'}, ns)

    out = {}
    maps = [torch.sigmoid(2.0 * CF.input_for('f23_%d' % k, (2, 2, 16, 16))).numpy().astype(np.float32) for k in range(6)]
    out['maps'] = np.stack(maps)
    out['mean_f32'] = np.mean(np.array(maps), axis=0)                                            # main.py:893
    assert out['mean_f32'].dtype == np.float32
    out['mean_f64'] = np.mean(np.array([m.astype(np.float64) for m in maps]), axis=0)
    for K in (2, 3):
        out['mean_k%d_f32' % K] = np.mean(np.array(maps[:K]), axis=0)
    # utils.py:568, 580 per tile: channel 1 of every experiment, stacked last
    out['stack_hwm'] = np.stack([np.stack([m[b][1, :, :] for m in maps], axis=-1) for b in range(2)])

    r = np.random.RandomState(23)
    values = np.round(r.uniform(0, 1, 23), 1)                                                    # one decimal: many ties
    out['kfold_values'] = values
    for n in (3, 5, 30):
        for s, (tr, te) in enumerate(ns['KFoldBySortedValue'](n_splits=n).split(values)):
            out['kfold_%d_train_%d' % (n, s)] = np.asarray(tr, np.int64)
            out['kfold_%d_test_%d' % (n, s)] = np.asarray(te, np.int64)

    m1 = np.array([0, 1, 1, 0, 1], np.uint8).reshape(5, 1, 1)
    m37 = (r.rand(5, 3, 7) > np.array([1.0, 0.0, 0.5, 0.8, 0.2])[:, None, None]).astype(np.uint8)   # empty, full, three densities
    yy, xx = np.mgrid[0:101, 0:101]
    m101 = np.stack([(((yy - 40) / 30.0) ** 2 + ((xx - 60) / 45.0) ** 2 <= 1).astype(np.uint8), (r.rand(101, 101) > 0.5).astype(np.uint8),
                     np.zeros((101, 101), np.uint8)])
    m101[2][:, 50:52] = 1                                                                        # two adjacent columns: one run
    out['masks_1x1'], out['masks_3x7'], out['masks_101'] = m1, m37, m101
    flat, offs, every = [], [0], list(m1) + list(m37) + list(m101)
    for mk in every:
        rle = ns['run_length_encoding'](mk)
        if rle:
            assert np.array_equal(ns['run_length_decoding'](' '.join(str(v) for v in rle), mk.shape), mk)
        flat += [int(v) for v in rle]
        offs.append(len(flat))
    out['rle_flat'], out['rle_offsets'] = np.array(flat, np.int64), np.array(offs, np.int64)
    ids = ['tile%02d' % i for i in range(len(every))]
    sub = ns['create_submission'](pd.DataFrame({'id': ids}), every)
    assert list(sub.columns) == ['id', 'rle_mask']
    out['sub_ids'], out['sub_rle'] = np.array(sub['id'].tolist()), np.array(sub['rle_mask'].tolist())
    save('F23_ensemble', **out)


if __name__ == '__main__':
    main()
