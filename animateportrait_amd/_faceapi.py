"""ctypes binding of libapface.so (C ABI declared in include/animateportrait_face.h): the MTCNN face detector and the photo
alignment.  Separate from _capi.py / libapamd.so, the boundary a model integrator binds.  Loaded on first use; a missing
library or a failed call raises -- there is no silent fallback."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('APFACE_LIB') or os.path.join(_HERE, 'libapface.so')

ABI_VERSION = 1      # APF_ABI_VERSION of include/animateportrait_face.h this binding was written against
MAX_SIDE, MIN_LEVEL = 8192, 12
CAP_LEVEL, CAP_MERGED, CAP_RNET, CAP_ONET, CAP_SORT = 4096, 4096, 2048, 512, 4096
OVF_LEVEL, OVF_MERGED, OVF_STAGE = 1, 2, 4
PNET_PARAMS, RNET_PARAMS, ONET_PARAMS = 6632, 100178, 389040
NMS_UNION, NMS_MIN = 0, 1
NET_R, NET_O = 0, 1
FAN_POINTS, FAN_MAX_RES, FAN_MAX_B = 68, 1024, 16
FAN_RGB, FAN_BGR = 0, 1
ERR_INVALID, ERR_UNSUPPORTED = -1, -2

_i32, _i64, _ptr, _f32, _f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
# name -> (restype, argtypes); every symbol include/animateportrait_face.h declares
SIGNATURES = {
    'apf_abi_version': (_i32, []),
    'apf_last_error': (ctypes.c_char_p, []),
    'apf_resize_level_ok': (_i32, [_ptr] + [_i32] * 4 + [_ptr]),
    'apf_resize_level': (ctypes.c_int, [_ptr] + [_i32] * 4 + [_ptr] * 2),
    'apf_pnet_ok': (_i32, [_ptr, _i32, _i32, _ptr, _ptr]),
    'apf_pnet': (ctypes.c_int, [_ptr, _i32, _i32, _ptr, _f32] + [_ptr] * 7),
    'apf_stage1_level_ok': (_i32, [_ptr, _ptr, _i32, _f64, _ptr, _ptr, _ptr]),
    'apf_stage1_level': (ctypes.c_int, [_ptr] * 4 + [_i32, _f64, _f64] + [_ptr] * 6),
    'apf_box_stage_ws_bytes': (_i64, [_i32]),
    'apf_box_stage_ok': (_i32, [_ptr, _i32, _ptr, _i32, _i32, _i32, _ptr, _ptr, _ptr, _i32, _ptr]),
    'apf_box_stage': (ctypes.c_int, [_ptr, _i32, _ptr, _i32, _ptr, _ptr, _ptr, _f64, _f64, _i32, _i32, _ptr, _ptr, _ptr, _i32]
                      + [_ptr] * 6),
    'apf_cutouts_ok': (_i32, [_ptr, _i32, _i32, _ptr, _ptr, _i32, _i32, _ptr]),
    'apf_cutouts': (ctypes.c_int, [_ptr, _i32, _i32, _ptr, _ptr, _i32, _i32, _ptr, _ptr]),
    'apf_net_ws_bytes': (_i64, [_i32, _i32]),
    'apf_net_ok': (_i32, [_i32, _ptr, _ptr, _i32] + [_ptr] * 5),
    'apf_net': (ctypes.c_int, [_i32, _ptr, _ptr, _i32] + [_ptr] * 6),
    'apf_crop_resize_cubic_ok': (_i32, [_ptr] + [_i32] * 6 + [_ptr]),
    'apf_crop_resize_cubic': (ctypes.c_int, [_ptr] + [_i32] * 7 + [_ptr] * 2),
    'apf_fan_crop_ok': (_i32, [_ptr, _i32, _i32] + [_f64] * 4 + [_i32] * 3 + [_ptr]),
    'apf_fan_crop': (ctypes.c_int, [_ptr, _i32, _i32] + [_f64] * 4 + [_i32] * 3 + [_ptr] * 2),
    'apf_fan_decode_ok': (_i32, [_ptr, _ptr, _i32, _i32, _ptr, _ptr]),
    'apf_fan_decode': (ctypes.c_int, [_ptr, _ptr, _i32, _i32, _ptr, _i32, _ptr, _ptr]),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load libapface.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError('animateportrait_amd: %s not found. Build it with `make -C animateportrait_amd/csrc`. '
                                       'The face detector has no path without it.' % LIB_PATH)
                l = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    if not hasattr(l, name):
                        raise RuntimeError('animateportrait_amd: %s is stale: it lacks %s. Rebuild it '
                                           '(make -C animateportrait_amd/csrc)' % (LIB_PATH, name))
                    fn = getattr(l, name)
                    fn.restype = res
                    fn.argtypes = args
                if l.apf_abi_version() != ABI_VERSION:
                    raise RuntimeError('animateportrait_amd: %s speaks face ABI %d, this binding %d: rebuild the library '
                                       '(make -C animateportrait_amd/csrc)' % (LIB_PATH, l.apf_abi_version(), ABI_VERSION))
                _lib = l
    return _lib


def last_error():
    msg = lib().apf_last_error()
    return msg.decode() if msg else '?'


def check(rc, what=''):
    if rc < 0:
        raise RuntimeError('libapface %s failed (%d): %s' % (what, rc, last_error()))
    return rc
