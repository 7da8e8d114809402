"""ctypes binding of libapdata.so (C ABI declared in include/animateportrait_data.h): batch preparation for the data
layer.  Separate from _capi.py / libapamd.so, the boundary a model integrator binds.  Loaded on first use; as there, a
missing library or a failed call raises -- there is no silent fallback."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('APDATA_LIB') or os.path.join(_HERE, 'libapdata.so')

ABI_VERSION = 1      # APD_ABI_VERSION of include/animateportrait_data.h this binding was written against
MAX_TAPS, MAX_SOURCE, MAX_LOAD, MAX_IMAGES = 64, 8192, 4096, 65535


class ApdImagePrep(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('N', 'Hs', 'Ws', 'C', 'load_w', 'load_h', 'crop', 'to_gray', 'kh', 'kv',
                                              'max_x', 'max_y')]


# name -> (restype, argtypes); every symbol include/animateportrait_data.h declares
SIGNATURES = {
    'apd_abi_version': (ctypes.c_int32, []),
    'apd_last_error': (ctypes.c_char_p, []),
    'apd_image_prep_ok': (ctypes.c_int32, [ctypes.POINTER(ApdImagePrep)]),
    'apd_image_prep_u8': (ctypes.c_int, [ctypes.POINTER(ApdImagePrep)] + [ctypes.c_void_p] * 9),
}

# Added after the first release of data ABI 1 without changing any call above, so the version number stays: a library
# that predates them is recognised by the missing symbol.
_i32, _ptr = ctypes.c_int32, ctypes.c_void_p
SIGNATURES.update({
    'apd_landmark_map_ok': (ctypes.c_int32, [_ptr] * 4 + [_i32] * 8),
    'apd_landmark_map': (ctypes.c_int, [_ptr] * 3 + [_i32] * 8 + [ctypes.c_float, ctypes.c_float, _ptr, _ptr]),
    'apd_landmark_marks_ok': (ctypes.c_int32, [_ptr] * 4 + [_i32] * 6),
    'apd_landmark_marks': (ctypes.c_int, [_ptr] * 3 + [_i32] * 6 + [_ptr, _ptr]),
    'apd_frames_to_u8_ok': (ctypes.c_int32, [_ptr] * 2 + [_i32] * 4),
    'apd_frames_to_u8': (ctypes.c_int, [_ptr] + [_i32] * 4 + [_ptr, _ptr]),
})
MAX_SEGMENTS, MAX_RADIUS, MAX_THICKNESS, MAX_MAP, MAX_POINTS = 128, 31, 16, 1024, 1024

# the device PNG encoder (csrc/data/png_encode.hip), added the same way
_i64 = ctypes.c_int64
SIGNATURES.update({
    'apd_png_bound': (_i64, [_i32] * 3),
    'apd_png_workspace_bytes': (_i64, [_i32] * 4),
    'apd_png_encode_ok': (ctypes.c_int32, [_ptr] * 4 + [_i32] * 5 + [_i64] * 2),
    'apd_png_encode': (ctypes.c_int, [_ptr] + [_i32] * 5 + [_ptr, _i64, _ptr, _ptr, _i64, _ptr]),
})
MAX_PNG_SIDE = 2048

# the device JPEG encoder (csrc/data/jpeg_encode.hip), added the same way
SIGNATURES.update({
    'apd_jpeg_bound': (_i64, [_i32] * 3),
    'apd_jpeg_workspace_bytes': (_i64, [_i32] * 4),
    'apd_jpeg_encode_ok': (ctypes.c_int32, [_ptr] * 4 + [_i32] * 6 + [_i64] * 2),
    'apd_jpeg_encode': (ctypes.c_int, [_ptr] + [_i32] * 6 + [_ptr, _i64, _ptr, _ptr, _i64, _ptr]),
})
MAX_JPEG_SIDE = 2048

# the coloured landmark rasteriser (csrc/data/landmark_vis.hip), added the same way
_u32 = ctypes.c_uint32
SIGNATURES.update({
    'apd_landmark_vis_ok': (ctypes.c_int32, [_ptr] * 5 + [_i32] * 8 + [_u32, _u32, _ptr]),
    'apd_landmark_vis': (ctypes.c_int, [_ptr] * 5 + [_i32] * 8 + [_u32, _u32, _ptr, _ptr]),
})

_lib = None
_lock = threading.Lock()


def lib():
    """Load libapdata.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError('animateportrait_amd: %s not found. Build it with `make -C animateportrait_amd/csrc`. '
                                       'There is no CPU fallback inside --data_prep device.' % LIB_PATH)
                l = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    if not hasattr(l, name):
                        raise RuntimeError('animateportrait_amd: %s is stale: it lacks %s. Rebuild it '
                                           '(make -C animateportrait_amd/csrc)' % (LIB_PATH, name))
                    fn = getattr(l, name)
                    fn.restype = res
                    fn.argtypes = args
                if l.apd_abi_version() != ABI_VERSION:
                    raise RuntimeError('animateportrait_amd: %s speaks data ABI %d, this binding %d: rebuild the library '
                                       '(make -C animateportrait_amd/csrc)' % (LIB_PATH, l.apd_abi_version(), ABI_VERSION))
                _lib = l
    return _lib


def last_error():
    msg = lib().apd_last_error()
    return msg.decode() if msg else '?'


def check(rc, what=''):
    if rc < 0:
        raise RuntimeError('libapdata %s failed (%d): %s' % (what, rc, last_error()))
    return rc
