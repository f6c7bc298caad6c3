"""Child of tests/test_gpu_sparse_conv.py::test_knobs_do_not_change_results (not collected by pytest): runs the coverage cases that
row KNOB_ENVS[argv[1]] of the knob table can change, in a process started with those DZ_TUNE_* values (the library reads them once),
and prints one JSON line per case: label, math mode, reported instance, worst normalised error, write-contract result.  A case that
fails its bound or its contract ends the child with exit status 1 after its line; nothing more is launched."""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import torch
    from tests import test_gpu_sparse_conv as T
    env = T.KNOB_ENVS[int(sys.argv[1])]
    for k, v in env.items():
        assert os.environ.get(k) == v, 'start this script with %s=%s' % (k, v)
    dev = torch.device('cuda', 0)
    for case in T.knob_cases(env):
        line = dict(label=case.label, mode=case.mode, name=None, worst=None, contract='ok')
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                line['name'], line['worst'] = T.run_case(case, dev)
        except AssertionError as exc:
            line['contract'] = 'FAILED: %s' % (exc,)
            print(json.dumps(line), flush=True)
            return 1
        print(json.dumps(line), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
