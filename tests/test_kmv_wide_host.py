"""The wide matrix-free kernel product (mxf_kmv_wide, mxf_kmv_wide_bwd) is declared, exported and bound with matching argument counts, and
its two limits agree between the header and the binding.  No GPU."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_limits_are_declared_exported_and_bound():
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, narrow in (('mxf_kmv_wide', 'mxf_kmv'), ('mxf_kmv_wide_bwd', 'mxf_kmv_bwd')):
        assert 'int ' + name + '(' in header and name in _lib.ALL_SYMBOLS and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[narrow], 'the argument list of ' + narrow
    assert '#define MXF_KMV_WIDE_MIN_Q %d' % _lib.KMV_WIDE_MIN_Q in header and _lib.KMV_WIDE_MIN_Q == _lib.KMV_MAX_Q + 1
    assert '#define MXF_KMV_WIDE_MAX_Q %d' % _lib.KMV_WIDE_MAX_Q in header and _lib.KMV_WIDE_MAX_Q == 16384
