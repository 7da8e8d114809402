"""ctypes binding of libapstyle.so (C ABI declared in include/animateportrait_style.h): the element-wise and statistics
kernels of the static cartoon generator.  Separate from _capi.py / libapamd.so, the boundary a model integrator binds.
Loaded on first use; as there, a missing library or a failed call raises -- there is no silent fallback."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('APSTYLE_LIB') or os.path.join(_HERE, 'libapstyle.so')

ABI_VERSION = 1      # APS_ABI_VERSION of include/animateportrait_style.h this binding was written against
MAX_PLANES, MAX_SIDE = 65535, 4096
ACT_NONE, ACT_RELU = 0, 1
JOIN, POOL2, UP2ADD, SUM3, STAT = 0, 1, 2, 3, 4
STAT_RELU = 1

_i32, _ptr, _f32 = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float
# name -> (restype, argtypes); every symbol include/animateportrait_style.h declares
SIGNATURES = {
    'aps_abi_version': (_i32, []),
    'aps_last_error': (ctypes.c_char_p, []),
    'aps_lin_coeffs_ok': (_i32, [_ptr] * 7 + [_i32] * 5),
    'aps_lin_coeffs': (ctypes.c_int, [_ptr] + [_i32] * 4 + [_ptr] * 3 + [_i32, _f32] + [_ptr] * 4),
    'aps_affine_apply_ok': (_i32, [_ptr] * 6 + [_i32] * 5),
    'aps_affine_apply': (ctypes.c_int, [_ptr] * 3 + [_i32, _ptr] + [_i32] * 4 + [_ptr] * 4),
    'aps_plane_combine_ok': (_i32, [_i32] + [_ptr] * 4 + [_i32] * 7 + [_ptr] * 3),
    'aps_plane_combine': (ctypes.c_int, [_i32] + [_ptr] * 4 + [_i32] * 7 + [_ptr] * 4),
    # cartoon training: luminance in front of the identity loss (added without an ABI change)
    'aps_luma_ok': (_i32, [_ptr] * 2 + [_i32] * 3),
    'aps_luma_fwd': (ctypes.c_int, [_ptr] + [_i32] * 3 + [_ptr] * 2),
    'aps_luma_bwd': (ctypes.c_int, [_ptr] + [_i32] * 3 + [_ptr] * 2),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load libapstyle.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError('animateportrait_amd: %s not found. Build it with `make -C animateportrait_amd/csrc`. '
                                       'The cartoon generator has no path without it.' % LIB_PATH)
                l = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    if not hasattr(l, name):
                        raise RuntimeError('animateportrait_amd: %s is stale: it lacks %s. Rebuild it '
                                           '(make -C animateportrait_amd/csrc)' % (LIB_PATH, name))
                    fn = getattr(l, name)
                    fn.restype = res
                    fn.argtypes = args
                if l.aps_abi_version() != ABI_VERSION:
                    raise RuntimeError('animateportrait_amd: %s speaks style ABI %d, this binding %d: rebuild the library '
                                       '(make -C animateportrait_amd/csrc)' % (LIB_PATH, l.aps_abi_version(), ABI_VERSION))
                _lib = l
    return _lib


def last_error():
    msg = lib().aps_last_error()
    return msg.decode() if msg else '?'


def check(rc, what=''):
    if rc < 0:
        raise RuntimeError('libapstyle %s failed (%d): %s' % (what, rc, last_error()))
    return rc
