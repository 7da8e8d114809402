"""The device JPEG encoder and the AVI writer without a device: the names the data ABI gained, what apd_jpeg_encode_ok
refuses, apd_jpeg_bound, the encoder's own text (csrc/data/jpeg_core.h) compiled for the host under
-fsanitize=address,undefined by tools/jpeg_host_check.py and judged by tests/jpeg_fixture.check_file, util/avi.AviWriter
read back by an independent RIFF reader, and the entry point's flags."""
import ctypes
import importlib.util
import io
import os
import struct
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_fixture as jf         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ('apd_jpeg_bound', 'apd_jpeg_workspace_bytes', 'apd_jpeg_encode_ok', 'apd_jpeg_encode')
IMAGES = jf.images()
CASES = jf.golden_cases()


def _tool():
    spec = importlib.util.spec_from_file_location('jpeg_host_check', os.path.join(ROOT, 'tools', 'jpeg_host_check.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def host_files(tmp_path_factory):
    """every golden case through the sanitised host program, once: (name, quality) -> (file bytes, bound)"""
    tool = _tool()
    work = str(tmp_path_factory.mktemp('jpeg_host'))
    exe = tool.build(work)
    return dict(zip(CASES, tool.encode(exe, work, [(IMAGES[n], q) for n, q in CASES])))


def test_new_names_are_declared_and_exported():
    from animateportrait_amd import _dataapi as D
    header = open(os.path.join(ROOT, 'include', 'animateportrait_data.h')).read()
    assert all(n in D.SIGNATURES and n + '(' in header for n in NEW_NAMES)
    assert '#define APD_ABI_VERSION 1' in header and D.ABI_VERSION == 1
    assert '#define APD_MAX_JPEG_SIDE %d ' % D.MAX_JPEG_SIDE in header and D.MAX_JPEG_SIDE == 2048
    lib = D.lib()
    assert all(hasattr(lib, n) for n in NEW_NAMES) and lib.apd_abi_version() == 1
    source = open(os.path.join(ROOT, 'animateportrait_amd', 'csrc', 'data', 'jpeg_encode.hip')).read()
    assert 'apd::to_byte(' in source and 'unsigned to_byte(float x)' not in source          # the one shared definition


def test_bound_and_workspace():
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    for h, w in ((1, 1), (37, 53), (256, 256), (8, 2048), (2048, 8), (2048, 2048)):
        for ch in (1, 3):
            b = lib.apd_jpeg_bound(h, w, ch)
            blocks = ((h + 7) // 8) * ((w + 7) // 8) * ch
            assert b > 0 and b % 4 == 0 and b >= 416 * blocks + 538, (h, w, ch, b)
            assert lib.apd_jpeg_workspace_bytes(3, h, w, ch) == 3 * lib.apd_jpeg_workspace_bytes(1, h, w, ch) > 0
    for args in ((0, 5, 3), (5, 0, 3), (2049, 5, 3), (5, 2049, 1), (5, 5, 2), (5, 5, 4)):
        assert lib.apd_jpeg_bound(*args) < 0 and 'jpeg_bound' in D.last_error(), args
        assert lib.apd_jpeg_workspace_bytes(1, *args) < 0
    assert lib.apd_jpeg_workspace_bytes(0, 5, 5, 3) < 0 and 'N = 0' in D.last_error()


def test_ok_refuses_without_a_device():
    """the pointers are never dereferenced by apd_jpeg_encode_ok: any non-null aligned value stands in"""
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    x = ctypes.c_void_p(4096)

    def ok(src=x, dst=x, sizes=x, ws=x, n=2, c=1, h=37, w=53, ch=3, q=90, slot=None, wsb=None):
        slot = lib.apd_jpeg_bound(h, w, ch) if slot is None else slot
        wsb = lib.apd_jpeg_workspace_bytes(n, h, w, ch) if wsb is None else wsb
        return lib.apd_jpeg_encode_ok(src, dst, sizes, ws, n, c, h, w, ch, q, slot, wsb)
    assert ok() == 1 and ok(c=3) == 1 and ok(ch=1) == 1 and ok(h=2048, w=2048, n=1) == 1 and ok(h=1, w=1) == 1
    assert ok(q=1) == 1 and ok(q=100) == 1
    bound = lib.apd_jpeg_bound(37, 53, 3)
    assert ok(slot=bound + 4) == 1
    for bad, word in ((dict(c=2), 'C = 2'), (dict(c=3, ch=1), 'needs C = 1'), (dict(q=0), 'quality = 0'), (dict(q=101), 'quality = 101'),
                      (dict(slot=bound - 4), 'below apd_jpeg_bound'), (dict(slot=bound + 2), 'multiple of 4'),
                      (dict(wsb=lib.apd_jpeg_workspace_bytes(2, 37, 53, 3) - 1), 'workspace'),
                      (dict(src=None), 'null'), (dict(dst=None), 'null'), (dict(sizes=None), 'null'), (dict(ws=None), 'null'),
                      (dict(n=0, slot=bound, wsb=1 << 20), 'N = 0'),
                      (dict(ch=2, slot=bound, wsb=1 << 20), 'channels = 2'), (dict(h=2049, slot=1 << 24, wsb=1 << 30), '2049'),
                      (dict(w=0, slot=bound, wsb=1 << 20), 'sides'), (dict(n=2, slot=1 << 30, wsb=1 << 30), '2^31'),
                      (dict(dst=ctypes.c_void_p(4097)), 'aligned'), (dict(sizes=ctypes.c_void_p(4098)), 'aligned')):
        assert ok(**bad) == 0, bad
        assert 'jpeg_encode' in D.last_error() and word in D.last_error(), (bad, D.last_error())
    # the launching call refuses the same way, before it asks the runtime anything: nothing is launched
    assert lib.apd_jpeg_encode(x, 2, 2, 37, 53, 3, 90, x, bound, x, x, 1 << 20, None) < 0 and 'C = 2' in D.last_error()
    assert lib.apd_jpeg_encode(x, 2, 1, 37, 53, 3, 0, x, bound, x, x, 1 << 20, None) < 0 and 'quality = 0' in D.last_error()


def test_walker_refuses_damage(host_files):
    """the yardstick itself: a wrong RSTm number, an unstuffed FF, a missing EOI and a wrong height are caught"""
    data, _ = host_files[('tall80x24', 90)]
    assert len(jf.walk(data, 80, 24, 1)) == 10
    first = data.index(b'\xff\xd0')
    for broken in (data[:first + 1] + b'\xd1' + data[first + 2:], data[:first + 2] + b'\xff\x01' + data[first + 2:], data[:-2], data + b'\0'):
        with pytest.raises(AssertionError):
            jf.walk(broken, 80, 24, 1)
    with pytest.raises(AssertionError):
        jf.walk(data, 81, 24, 1)


@pytest.mark.parametrize('name,quality', CASES)
def test_host_program_files(host_files, name, quality):
    from animateportrait_amd import _dataapi as D
    data, bound = host_files[(name, quality)]
    im = IMAGES[name]
    h, w, ch = im.shape
    figures = jf.measure(data, im, quality)
    print('%s q%d: %d bytes, bound %d; PSNR %.3f dB, max error %d; PIL\'s file %.3f dB, %d' % ((name, quality, len(data), bound) + figures))
    jf.check_file(data, im, quality)
    assert len(data) <= bound == D.lib().apd_jpeg_bound(h, w, ch)              # the host program and the library state one bound
    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_host.npz'))
    assert golden[jf.key(name, quality)].tobytes() == data


def test_golden_set_is_small_and_stuffing_runs(host_files):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg_host.npz')) < 256 * 1024
    for name in ('noise37x53_grey', 'noise37x53_rgb'):
        data, _ = host_files[(name, 100)]
        scan = data[data.index(b'\xff\xda'):]
        assert scan.count(b'\xff\x00') >= 1, name
    marks = [m for m in range(8) if bytes([0xFF, 0xD0 + m]) in host_files[('tall80x24', 90)][0]]
    assert marks == list(range(8))                                             # ten segments: the cycle wraps


# ---- util/avi.py

def _write_wav(path, samples, rate=16000, channels=1, width=2):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(samples.tobytes())


@pytest.fixture(scope='module')
def three_frames(host_files):
    """three different 37 x 53 grey files: the golden noise at qualities 90, 50 and 100"""
    return [host_files[('noise37x53_grey', q)][0] for q in (90, 50, 100)]


def test_avi_with_audio(three_frames, tmp_path):
    from animateportrait_amd.util import avi
    samples = (np.random.RandomState(4).randint(-3000, 3000, 1000)).astype('<i2')        # 1000 sample frames: 3 x 256 + 232 left over
    _write_wav(tmp_path / 'a.wav', samples)
    assert avi.fps_fraction(62.5) == (125, 2) and avi.fps_fraction(25) == (25, 1) and avi.fps_fraction(29.97) == (2997, 100)
    slot = max(len(f) for f in three_frames) + 5
    buf = np.full((3, slot), 0xA5, np.uint8)
    for i, f in enumerate(three_frames):
        buf[i, :len(f)] = np.frombuffer(f, np.uint8)
    path = tmp_path / 'clip.avi'
    w = avi.AviWriter(str(path), 53, 37, 125, 2, audio=str(tmp_path / 'a.wav'))
    w.add_frames(buf[:2], np.array([len(f) for f in three_frames[:2]], np.int32))
    w.add_frames(buf[2:], [len(three_frames[2])])
    w.close()
    blob = open(path, 'rb').read()
    got = jf.read_avi(blob)                                           # RIFF size, list structure, every idx1 entry
    avih = got['avih']
    assert avih[0] == 16000 and avih[4] == 3 and avih[6] == 2 and (avih[8], avih[9]) == (53, 37) and avih[3] & 0x10
    (vh, vf), (ah, af) = got['streams']
    assert vh[0] == b'vids' and vh[1] == b'MJPG' and (vh[7], vh[6]) == (125, 2) and vh[9] == 3
    assert vh[10] == max(len(f) for f in three_frames)
    size, bw, bh, planes, bits, comp, image = struct.unpack('<IiiHH4sI', vf[:24])
    assert (size, bw, bh, planes, bits, comp, image) == (40, 53, 37, 1, 24, b'MJPG', 53 * 37 * 3) and len(vf) == 40
    assert ah[0] == b'auds' and (ah[7], ah[6]) == (16000, 1) and ah[9] == 1000 and ah[12] == 2
    assert struct.unpack('<HHIIHHH', af) == (1, 1, 16000, 32000, 2, 16, 0)
    kinds = [cc for cc, _ in got['movi']]
    assert kinds == [b'00dc', b'01wb', b'00dc', b'01wb', b'00dc', b'01wb', b'01wb']
    video = [p for cc, p in got['movi'] if cc == b'00dc']
    assert video == three_frames                                      # byte for byte
    for f in video:
        image, _ = jf.decode_pil(f)
        assert image.shape == (37, 53, 1)
    sound = [p for cc, p in got['movi'] if cc == b'01wb']
    assert b''.join(sound) == samples.tobytes()
    for k in range(3):
        assert len(sound[k]) == 2 * ((k + 1) * 16000 * 2 // 125 - k * 16000 * 2 // 125) == 512
    assert len(sound[3]) == 2 * (1000 - 768)
    assert any(len(p) & 1 for _, p in got['movi'])                    # an odd chunk is there, so the padding was exercised
    assert struct.unpack('<I', blob[4:8])[0] == len(blob) - 8


def test_avi_audio_rates_and_formats(three_frames, tmp_path):
    """a rate the frame rate does not divide, stereo 8-bit: the chunk sizes follow the formula and nothing is lost"""
    from animateportrait_amd.util import avi
    samples = np.random.RandomState(5).randint(0, 256, (1500, 2)).astype(np.uint8)
    _write_wav(tmp_path / 'b.wav', samples, rate=11025, channels=2, width=1)
    path = tmp_path / 'b.avi'
    with avi.AviWriter(str(path), 53, 37, 30000, 1001, audio=str(tmp_path / 'b.wav')) as w:
        for f in three_frames:
            w.add_frame(f)
    got = jf.read_avi(open(path, 'rb').read())
    sound = [p for cc, p in got['movi'] if cc == b'01wb']
    assert b''.join(sound) == samples.tobytes()
    for k in range(3):
        assert len(sound[k]) == 2 * ((k + 1) * 11025 * 1001 // 30000 - k * 11025 * 1001 // 30000)
    assert struct.unpack('<HHIIHHH', got['streams'][1][1]) == (1, 2, 11025, 22050, 2, 8, 0)


def test_avi_without_audio_has_one_stream(three_frames, tmp_path):
    from animateportrait_amd.util import avi
    path = tmp_path / 'mute.avi'
    with avi.AviWriter(str(path), 53, 37, 125, 2) as w:
        for f in three_frames:
            w.add_frame(f)
    got = jf.read_avi(open(path, 'rb').read())
    assert len(got['streams']) == 1 and got['avih'][6] == 1 and got['avih'][4] == 3
    assert [cc for cc, _ in got['movi']] == [b'00dc'] * 3 and [p for _, p in got['movi']] == three_frames


def test_avi_refusals(three_frames, tmp_path):
    from animateportrait_amd.util import avi
    # an IEEE-float wav: the stdlib refuses format tag 3, the message names it
    data = np.zeros(100, '<f4').tobytes()
    fmt = struct.pack('<HHIIHH', 3, 1, 16000, 64000, 4, 32)
    body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + b'data' + struct.pack('<I', len(data)) + data
    (tmp_path / 'f.wav').write_bytes(b'RIFF' + struct.pack('<I', len(body)) + body)
    with pytest.raises(ValueError, match='IEEE float'):
        avi.AviWriter(str(tmp_path / 'f.avi'), 53, 37, 125, 2, audio=str(tmp_path / 'f.wav'))
    _write_wav(tmp_path / 'c.wav', np.zeros(300, np.uint8), width=3)
    with pytest.raises(ValueError, match='24-bit'):
        avi.AviWriter(str(tmp_path / 'c.avi'), 53, 37, 125, 2, audio=str(tmp_path / 'c.wav'))
    # a file that would pass the limit: the limit is lowered, not 2 GB written
    assert avi.AviWriter.MAX_BYTES == 2 ** 31 - 2 ** 20
    w = avi.AviWriter(str(tmp_path / 'big.avi'), 53, 37, 125, 2)
    w.MAX_BYTES = w.at + 2 * len(three_frames[0])
    w.add_frame(three_frames[0])
    with pytest.raises(ValueError, match='OpenDML'):
        w.add_frame(three_frames[0])
    w.close()
    assert jf.read_avi(open(tmp_path / 'big.avi', 'rb').read())['avih'][4] == 1          # what was written is a whole file


def test_flags():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    a = ap.parse_args(['--photo', 'p.png', '--out', 'o'])
    assert (a.video, a.video_quality, a.video_channels, a.frames) == ('ffmpeg', 90, None, 'png')
    a = ap.parse_args(['--photo', 'p.png', '--out', 'o', '--video', 'avi', '--frames', 'none', '--video_quality', '75', '--video_channels', '3'])
    assert (a.video, a.video_quality, a.video_channels, a.frames) == ('avi', 75, 3, 'none')
    for bad in (['--video', 'mp4'], ['--video_channels', '2'], ['--frames', 'jpeg']):
        with pytest.raises(SystemExit):
            ap.parse_args(['--photo', 'p.png', '--out', 'o'] + bad)
    # --frames none without --video avi is an argument error, raised before anything is built
    with pytest.raises(SystemExit):
        end2end.main(['--photo', 'p.png', '--out', 'o', '--landmarks_npy', 'x.npy', '--frames', 'none'])
    with pytest.raises(SystemExit):
        end2end.main(['--photo', 'p.png', '--out', 'o', '--landmarks_npy', 'x.npy', '--video', 'avi', '--video_quality', '0'])
