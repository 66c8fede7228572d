"""Run a script against a timing-variant build of liblbwn.so (same-box A/B runs only; the product
always loads the in-tree lb-wavenet_amd/lbwn/liblbwn.so).

    python tools/with_lib.py <variant liblbwn.so> <script.py> [args...]

The variant is loaded first, so every later lbwn._lib.load() in the process returns it."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lb-wavenet_amd'))
sys.path.insert(0, ROOT)

if __name__ == '__main__':
    lib, script = sys.argv[1], sys.argv[2]
    import ctypes
    from lbwn import _lib
    # a variant built from an older revision lacks the entry points added since: they leave the
    # table of this process (a script that calls one fails there), the rest binds as in the product
    probe = ctypes.CDLL(os.path.abspath(lib))
    missing = [n for n in _lib._SIGS if not hasattr(probe, n)]
    for n in missing:
        del _lib._SIGS[n]
    if missing:
        print('with_lib: %s lacks %s' % (lib, ', '.join(missing)), file=sys.stderr)
    _lib.load(os.path.abspath(lib))
    sys.argv = [script] + sys.argv[3:]
    runpy.run_path(script, run_name='__main__')
