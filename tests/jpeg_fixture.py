"""What the JPEG-encoder tests (test_jpeg_encode_cpu.py, test_jpeg_encode_gpu.py) and tools/jpeg_host_check.py share: the u8
images the cases are made of, a marker walker in pure Python that checks the layout include/animateportrait_data.h states,
``check_file`` -- the walker, PIL as the decoder, and PIL's own encoder at the same tables as the yardstick of the error --
and an independent RIFF reader for the AVI files of util/avi.py."""
import io
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_fixture as pf          # noqa: E402

# check_file's margins: the worst shortfall against PIL's encoder that tools/jpeg_host_check.py --measure found over every
# image below at qualities 50, 90 and 100 (the table is in DESIGN.md section 4c-4), plus 0.1 dB and plus 1 grey level
WORST_PSNR_SHORTFALL_DB = 1.461    # one8x8 at quality 100: 7 of its 64 pixels are off by one grey level, 5 in PIL's file
WORST_MAX_ERROR_EXCESS = 1          # noise37x53_rgb at quality 100: 4 against 3
PSNR_MARGIN_DB = WORST_PSNR_SHORTFALL_DB + 0.1
MAX_ERROR_MARGIN = WORST_MAX_ERROR_EXCESS + 1
MSE_FLOOR = 1e-4                  # PSNR of an exact decode: 88.1 dB instead of infinity

to_frames = pf.to_frames


def images():
    """name -> (H, W, channels) uint8"""
    rng = np.random.RandomState(11)
    cases = {}
    cases['lines256_rgb'] = pf.line_drawing()
    cases['lines256_grey'] = pf.line_drawing()[:, :, :1].copy()
    cases['noise37x53_grey'] = rng.randint(0, 256, (37, 53, 1)).astype(np.uint8)         # 5 x 7 blocks, ragged on both sides
    cases['noise37x53_rgb'] = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    cases['one8x8'] = rng.randint(0, 256, (8, 8, 1)).astype(np.uint8)
    cases['one1x1'] = np.array([[[201]]], np.uint8)
    yy, xx = np.mgrid[0:80, 0:24]
    tall = (128 + 90 * np.sin(yy / 5.0) * np.cos(xx / 3.0) + rng.randint(-20, 21, (80, 24))).clip(0, 255)
    cases['tall80x24'] = tall.astype(np.uint8)[:, :, None]                                # 10 MCU rows: RSTm wraps past 7
    cases['wide8x2048_rgb'] = rng.randint(0, 256, (8, 2048, 3)).astype(np.uint8)          # 256 MCUs, 768 blocks in one segment
    cases['flat64_white'] = np.full((64, 64, 1), 255, np.uint8)
    cases['flat64_black'] = np.zeros((64, 64, 1), np.uint8)
    return cases


# (image, quality) of every file of tests/golden/jpeg_host.npz; the key is '<image>_q<quality>'
def golden_cases():
    cases = [(name, 90) for name in sorted(images())]
    cases += [('noise37x53_grey', q) for q in (1, 50, 100)] + [('noise37x53_rgb', q) for q in (1, 50, 100)]
    return cases


def key(name, quality):
    return '%s_q%d' % (name, quality)


SOI, EOI, APP0, DQT, SOF0, DHT, DRI, SOS = 0xD8, 0xD9, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA


def walk(data, height, width, channels):
    """The markers of one file.  Asserts the order SOI APP0 DQT SOF0 DHT DRI SOS scan EOI, the SOF0 fields, the four Huffman
    tables, the DRI value, the RSTm count and cycle, that no unstuffed 0xFF lies in the scan, and EOI as the last two bytes.
    Returns the list of entropy-coded segments (bytes, still stuffed)."""
    data = bytes(data)
    assert data[:2] == b'\xff\xd8', 'SOI'
    at, order, seen = 2, [SOI], {}
    while True:
        assert at + 4 <= len(data) and data[at] == 0xFF, 'marker expected at %d' % at
        m = data[at + 1]
        n, = struct.unpack('>H', data[at + 2:at + 4])
        assert at + 2 + n <= len(data), 'segment %02X runs past the end' % m
        order.append(m)
        seen[m] = data[at + 4:at + 2 + n]
        at += 2 + n
        if m == SOS:
            break
    assert order == [SOI, APP0, DQT, SOF0, DHT, DRI, SOS], ['%02X' % m for m in order]
    assert seen[APP0][:5] == b'JFIF\0'
    assert len(seen[DQT]) == 65 * (2 if channels == 3 else 1)
    sof = seen[SOF0]
    assert struct.unpack('>BHHB', sof[:6]) == (8, height, width, channels), sof[:6]
    for c in range(channels):
        assert tuple(sof[6 + 3 * c:9 + 3 * c]) == (c + 1, 0x11, 1 if c else 0), 'component %d of SOF0' % c
    dht, p, classes = seen[DHT], 0, []
    while p < len(dht):
        classes.append(dht[p])
        p += 17 + sum(dht[p + 1:p + 17])
    assert p == len(dht) and sorted(classes) == [0x00, 0x01, 0x10, 0x11], classes
    mcus = (width + 7) // 8
    assert struct.unpack('>H', seen[DRI]) == (mcus,)
    sos = seen[SOS]
    assert sos[0] == channels and tuple(sos[-3:]) == (0, 63, 0)
    for c in range(channels):
        assert tuple(sos[1 + 2 * c:3 + 2 * c]) == (c + 1, 0x11 if c else 0x00)
    assert data[-2:] == b'\xff\xd9', 'EOI is not the last two bytes'
    scan = data[at:-2]
    segments, start, k, expect = [], 0, 0, 0
    while k < len(scan):
        if scan[k] != 0xFF:
            k += 1
            continue
        assert k + 1 < len(scan), 'the scan ends in a lone FF'
        nxt = scan[k + 1]
        if nxt == 0x00:
            k += 2
            continue
        assert nxt == 0xD0 + expect, 'FF %02X in the scan at %d, expected RST%d' % (nxt, k, expect)
        segments.append(scan[start:k])
        expect = (expect + 1) & 7
        k += 2
        start = k
    segments.append(scan[start:])
    rows = (height + 7) // 8
    assert len(segments) == rows, '%d segments for %d MCU rows' % (len(segments), rows)
    assert all(len(s) > 0 for s in segments)
    return segments


def decode_pil(data):
    """(image (H, W, channels) uint8, quantization dict) of one file through Pillow, fully loaded"""
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(data)))
    im.load()
    assert im.format == 'JPEG' and im.mode in ('L', 'RGB'), (im.format, im.mode)
    a = np.asarray(im)
    return (a if a.ndim == 3 else a[:, :, None]), {k: list(v) for k, v in im.quantization.items()}


def pil_file(want, quality):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(want if want.shape[2] == 3 else want[:, :, 0]).save(f, format='JPEG', quality=quality, subsampling=0)
    return f.getvalue()


def error(got, want):
    """(PSNR in dB with the MSE floored, max absolute error)"""
    d = got.astype(np.float64) - want.astype(np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(float((d * d).mean()), MSE_FLOOR)), int(np.abs(d).max())


def measure(data, want, quality):
    """(our PSNR, our max error, PIL's PSNR, PIL's max error) against `want`, both files decoded by PIL; the layout, the mode, the
    size and the tables are asserted on the way"""
    h, w, ch = want.shape
    walk(data, h, w, ch)
    got, tables = decode_pil(data)
    assert got.shape == want.shape, (got.shape, want.shape)
    ref, ref_tables = decode_pil(pil_file(want, quality))
    assert tables == ref_tables, 'quantisation tables differ from PIL\'s at quality %d' % quality
    return error(got, want) + error(ref, want)


def check_file(data, want, quality):
    psnr, worst, ref_psnr, ref_worst = measure(data, want, quality)
    assert psnr >= ref_psnr - PSNR_MARGIN_DB, 'PSNR %.3f dB, PIL\'s file %.3f dB' % (psnr, ref_psnr)
    assert worst <= ref_worst + MAX_ERROR_MARGIN, 'max error %d, PIL\'s file %d' % (worst, ref_worst)
    return psnr, worst, ref_psnr, ref_worst


# ---- an independent reader of what util/avi.py writes

def riff_chunks(blob, start, end):
    """[(fourcc, payload offset, size)] of the chunks in blob[start:end]; every chunk is padded to even length"""
    out, at = [], start
    while at < end:
        assert at + 8 <= end, 'truncated chunk header at %d' % at
        cc, n = struct.unpack('<4sI', blob[at:at + 8])
        assert at + 8 + n <= end, 'chunk %r runs past its parent' % cc
        out.append((cc, at + 8, n))
        at += 8 + n + (n & 1)
    assert at == end, 'chunks end at %d, parent at %d' % (at, end)
    return out


def read_avi(blob):
    """dict: avih (tuple), streams [(strh tuple, strf bytes)], movi [(fourcc, payload)], idx [(fourcc, flags, offset, size)],
    movi_at (offset of the 'movi' fourcc).  Asserts the RIFF size, the list structure and every idx1 entry."""
    blob = bytes(blob)
    riff, size, form = struct.unpack('<4sI4s', blob[:12])
    assert riff == b'RIFF' and form == b'AVI ' and size == len(blob) - 8, (riff, form, size, len(blob))
    top = riff_chunks(blob, 12, len(blob))
    assert [c[0] for c in top] == [b'LIST', b'LIST', b'idx1'], [c[0] for c in top]
    assert blob[top[0][1]:top[0][1] + 4] == b'hdrl' and blob[top[1][1]:top[1][1] + 4] == b'movi'
    hdrl = riff_chunks(blob, top[0][1] + 4, top[0][1] + top[0][2])
    assert hdrl[0][0] == b'avih' and hdrl[0][2] == 56
    out = {'avih': struct.unpack('<14I', blob[hdrl[0][1]:hdrl[0][1] + 56]), 'streams': []}
    for cc, at, n in hdrl[1:]:
        assert cc == b'LIST' and blob[at:at + 4] == b'strl'
        strl = riff_chunks(blob, at + 4, at + n)
        assert [c[0] for c in strl] == [b'strh', b'strf'] and strl[0][2] == 56
        strh = struct.unpack('<4s4sIHHIIIIIIII4h', blob[strl[0][1]:strl[0][1] + 56])
        out['streams'].append((strh, blob[strl[1][1]:strl[1][1] + strl[1][2]]))
    movi_at = top[1][1]
    out['movi_at'] = movi_at
    out['movi'] = [(cc, blob[at:at + n]) for cc, at, n in riff_chunks(blob, movi_at + 4, movi_at + top[1][2])]
    positions = [(cc, at - 8 - movi_at, n) for cc, at, n in riff_chunks(blob, movi_at + 4, movi_at + top[1][2])]
    assert top[2][2] % 16 == 0
    out['idx'] = [struct.unpack('<4sIII', blob[top[2][1] + 16 * i:top[2][1] + 16 * i + 16]) for i in range(top[2][2] // 16)]
    assert len(out['idx']) == len(positions)
    for (cc, flags, offset, n), (want_cc, want_offset, want_n) in zip(out['idx'], positions):
        assert (cc, offset, n) == (want_cc, want_offset, want_n), (cc, offset, n, want_cc, want_offset, want_n)
        assert blob[movi_at + offset:movi_at + offset + 4] == cc                    # the entry points at a chunk of its fourcc
        assert struct.unpack('<I', blob[movi_at + offset + 4:movi_at + offset + 8]) == (n,)
        assert (flags & 0x10) == 0x10 if cc == b'00dc' else True                    # AVIIF_KEYFRAME on every video entry
    return out
