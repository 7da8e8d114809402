"""ctypes binding of libapseq.so (C ABI declared in include/animateportrait_seq.h): the batched LSTM forward of Module1's
landmark networks, the clip-level post-processing of their landmark sequence, the clip's f0 track (f0.py), the two ends of
its speaker embedding (speaker.py), its audio front end (audio_device.py) and the pose network's self-attention encoder
(encoder_hip.py).  Separate from _capi.py / libapamd.so, the boundary a model integrator binds.
Loaded on first use; as there, a missing library or a failed call raises -- there is no silent fallback."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('APSEQ_LIB') or os.path.join(_HERE, 'libapseq.so')

ABI_VERSION = 1      # APQ_ABI_VERSION of include/animateportrait_seq.h this binding was written against
LSTM_H = 256
MAX_B, MAX_T, MAX_I = 1048576, 65536, 512
ALIGN_WIDE, ALIGN_ELEM = 16, 4
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3

LM_C, SG_MIN_W, SG_MAX_W, SEG_MAX_T, MAX_STAMPS = 204, 5, 31, 512, 4096
SEG_CLOSE, SEG_LIP, SEG_NOSE = 1, 2, 4
IMG_TRANSFORM, IMG_EYES = 1, 2
REG_CENTER, REG_NO_X_ROT, REG_REGISTER, REG_MAX_ROUNDS = 1, 2, 4, 50
F0_HOP, F0_CANDS, F0_STATES, F0_MIN_LAG, F0_MAX_LAG, F0_UNVOICED = 256, 19, 20, 2, 320, 255
MEL_MIN_FFT, MEL_MAX_FFT, MEL_MAX_MELS, ALIGN_F64, SPK_E, SPK_MAX_B = 16, 1024, 128, 8, 256, 4096
RS_MAX_RATE, RS_MAX_TAPS, RS_MAX_C, RS_MAX_L = 1024, 16384, 2, 0x3fffffff
LOUD_MAX_N, LOUD_MAX_BLOCKS, FF_MAX_M, FF_MAX_L, FF_TILE = 8388607, 256, 8, 0x3fffffc0, 1024
ENC_D, ENC_HEADS, ENC_ROWS, ENC_MAX_T, ENC_FF_CHUNK, ENC_MAX_FF = 64, 2, 16, 512, 256, 8192

_i32, _i64, _ptr, _f32, _f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
# name -> (restype, argtypes); every symbol include/animateportrait_seq.h declares
SIGNATURES = {
    'apq_abi_version': (_i32, []),
    'apq_last_error': (ctypes.c_char_p, []),
    'apq_lstm_layer_fwd_ok': (_i32, [_ptr] * 6 + [_i32] * 5),
    'apq_lstm_layer_fwd': (ctypes.c_int, [_ptr] * 6 + [_i32] * 5 + [_ptr]),
    # the training pair of that layer (lstm_hip.lstm_train_batched)
    'apq_lstm_layer_fwd_train_ok': (_i32, [_ptr] * 8 + [_i32] * 4),
    'apq_lstm_layer_fwd_train': (ctypes.c_int, [_ptr] * 8 + [_i32] * 4 + [_ptr]),
    'apq_lstm_layer_bwd_ok': (_i32, [_ptr] * 5 + [_i32] * 4),
    'apq_lstm_layer_bwd': (ctypes.c_int, [_ptr] * 5 + [_i32] * 4 + [_ptr]),
    # clip-level landmark post-processing (landmark_post.py); each launching call = its _ok twin + the stream
    'apq_savgol_ok': (_i32, [_ptr] * 4 + [_i32] * 7),
    'apq_savgol': (ctypes.c_int, [_ptr] * 4 + [_i32] * 7 + [_ptr]),
    'apq_calib_baseline_ok': (_i32, [_ptr] * 2 + [_i32] * 2 + [_f32] * 2),
    'apq_calib_baseline': (ctypes.c_int, [_ptr] * 2 + [_i32] * 2 + [_f32] * 2 + [_ptr]),
    'apq_segment_assemble_ok': (_i32, [_ptr] * 4 + [_i32, _f64, _f32, _i32]),
    'apq_segment_assemble': (ctypes.c_int, [_ptr] * 4 + [_i32, _f64, _f32, _i32, _ptr]),
    'apq_image_landmarks_ok': (_i32, [_ptr] * 3 + [_i32] * 2 + [_f64] * 3 + [_i32]),
    'apq_image_landmarks': (ctypes.c_int, [_ptr] * 3 + [_i32] * 2 + [_f64] * 3 + [_i32, _ptr]),
    # rigid registration of landmark frames (landmark_post.rigid_register)
    'apq_rigid_register_ok': (_i32, [_ptr] * 4 + [_i32] * 2),
    'apq_rigid_register': (ctypes.c_int, [_ptr] * 4 + [_i32] * 2 + [_ptr]),
    # the clip's f0 track (f0.py)
    'apq_f0_candidates_ok': (_i32, [_ptr] + [_i32] * 4 + [_ptr] * 5),
    'apq_f0_candidates': (ctypes.c_int, [_ptr] + [_i32] * 4 + [_ptr] * 5 + [_ptr]),
    'apq_f0_track_ok': (_i32, [_ptr] * 5 + [_i32, _i32, _f64] + [_ptr] * 3),
    'apq_f0_track': (ctypes.c_int, [_ptr] * 5 + [_i32, _i32, _f64] + [_ptr] * 3 + [_ptr]),
    # the clip's speaker embedding (speaker.py)
    'apq_mel_frames_ok': (_i32, [_ptr] * 4 + [_i32] * 5),
    'apq_mel_frames': (ctypes.c_int, [_ptr] * 4 + [_i32] * 5 + [_ptr]),
    'apq_speaker_head_ok': (_i32, [_ptr] * 5 + [_i32]),
    'apq_speaker_head': (ctypes.c_int, [_ptr] * 5 + [_i32] + [_ptr]),
    # the clip's audio front end (audio_device.py)
    'apq_resample_poly_ok': (_i32, [_ptr] * 3 + [_i32] * 5),
    'apq_resample_poly': (ctypes.c_int, [_ptr] * 3 + [_i32] * 5 + [_ptr]),
    'apq_loudness_workspace_bytes': (_i64, [_i32]),
    'apq_loudness_sumsq_ok': (_i32, [_ptr] * 3 + [_i32]),
    'apq_loudness_sumsq': (ctypes.c_int, [_ptr] * 3 + [_i32] + [_ptr]),
    'apq_loudness_apply_ok': (_i32, [_ptr] * 2 + [_i32, _f64, _i32]),
    'apq_loudness_apply': (ctypes.c_int, [_ptr] * 2 + [_i32, _f64, _i32] + [_ptr]),
    'apq_filtfilt_workspace_bytes': (_i64, [_i32, _i32]),
    'apq_filtfilt_ok': (_i32, [_ptr] * 6 + [_i32] * 2),
    'apq_filtfilt': (ctypes.c_int, [_ptr] * 6 + [_i32] * 2 + [_ptr]),
    'apq_logmel_frames_ok': (_i32, [_ptr] * 4 + [_i32] * 4),
    'apq_logmel_frames': (ctypes.c_int, [_ptr] * 4 + [_i32] * 4 + [_ptr]),
    # the pose network's self-attention encoder (encoder_hip.py)
    'apq_enc_qkv_ok': (_i32, [_ptr] * 3 + [_f32] + [_ptr] * 9 + [_i32] * 3),
    'apq_enc_qkv': (ctypes.c_int, [_ptr] * 3 + [_f32] + [_ptr] * 9 + [_i32] * 3 + [_ptr]),
    'apq_enc_attn_ff_ok': (_i32, [_ptr] * 8 + [_f32] + [_ptr] * 6 + [_f32, _ptr] + [_i32] * 5),
    'apq_enc_attn_ff': (ctypes.c_int, [_ptr] * 8 + [_f32] + [_ptr] * 6 + [_f32, _ptr] + [_i32] * 5 + [_ptr]),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load libapseq.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError('animateportrait_amd: %s not found. Build it with `make -C animateportrait_amd/csrc`. '
                                       'The batched LSTM has no path without it.' % LIB_PATH)
                l = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    if not hasattr(l, name):
                        raise RuntimeError('animateportrait_amd: %s is stale: it lacks %s. Rebuild it '
                                           '(make -C animateportrait_amd/csrc)' % (LIB_PATH, name))
                    fn = getattr(l, name)
                    fn.restype = res
                    fn.argtypes = args
                if l.apq_abi_version() != ABI_VERSION:
                    raise RuntimeError('animateportrait_amd: %s speaks seq ABI %d, this binding %d: rebuild the library '
                                       '(make -C animateportrait_amd/csrc)' % (LIB_PATH, l.apq_abi_version(), ABI_VERSION))
                _lib = l
    return _lib


def last_error():
    msg = lib().apq_last_error()
    return msg.decode() if msg else '?'


def check(rc, what=''):
    if rc < 0:
        raise RuntimeError('libapseq %s failed (%d): %s' % (what, rc, last_error()))
    return rc
