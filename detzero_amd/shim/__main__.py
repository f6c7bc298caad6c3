"""``python -m detzero_amd.shim``                      prints the two directories to put on PYTHONPATH;
``python -m detzero_amd.shim <script.py> [args ...]``  runs one of the reference's tools (detection/tools/test.py,
refining/tools/test.py, tracking/tools/run_track.py with any --split, tracking/tools/eval_track.py) unchanged, from the current
directory, with the shim packages installed."""
import os
import runpy
import sys

from . import FALLBACK_DIR, SHIM_DIR, install

if len(sys.argv) > 1:
    install()
    script = sys.argv[1]
    sys.argv = sys.argv[1:]
    sys.path.insert(0, os.path.dirname(os.path.abspath(script)))       # as `python script.py` does
    runpy.run_path(script, run_name='__main__')
else:
    print(SHIM_DIR + ':' + FALLBACK_DIR)
