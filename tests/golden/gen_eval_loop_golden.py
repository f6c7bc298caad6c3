"""Golden output of the REFERENCE's own detection/tools/eval_utils.py:eval_one_epoch over the stub loader and model of
tests/test_shim.py: the returned recall dictionary and every record of the result.pkl it writes.

    python tests/golden/gen_eval_loop_golden.py      (build container only; needs the reference tree test_shim.py loads by path)

tests/test_shim.py::test_reference_eval_loop_equals_restated_loop checks the restated loop (tests/eval_loop.py) against this
file, and against the live reference where the tree exists.
"""
import logging
import os
import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    from tests import test_shim as ts
    assert ts.has_ref, 'the reference tree is not present'
    ref_eval = ts._reference_eval_utils()
    ds = ts._StubDataset()
    loader = torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=ds.collate_batch)
    with tempfile.TemporaryDirectory() as d:
        ret = ref_eval.eval_one_epoch(ts._stub_cfg(), ts._StubModel(), loader, 'x', logging.getLogger('gen-eval'), result_dir=Path(d), save_tb=True)
        recs = pickle.load(open(os.path.join(d, 'result.pkl'), 'rb'))
    out = {'ret_keys': np.array(list(ret)), 'ret_vals': np.array([float(v) for v in ret.values()], np.float64), 'n_records': np.int64(len(recs))}
    for i, r in enumerate(recs):
        out['rec%d_keys' % i] = np.array(list(r))
        for k, v in r.items():
            out['rec%d_%s' % (i, k)] = np.asarray(v)
    path = os.path.join(HERE, 'eval_loop_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, ret)


if __name__ == '__main__':
    main()
