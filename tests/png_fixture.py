"""What the PNG-encoder tests (test_png_encode_cpu.py, test_png_encode_gpu.py) and tools/png_host_check.py share: an
independent decoder -- chunks parsed here, every CRC checked with zlib.crc32, the IDAT data through zlib.decompress (which
verifies the Adler-32), the row filters undone in numpy -- a second decoder (PIL), and the u8 images the cases are made of."""
import io
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def decode(data):
    """bytes of one file -> (H, W, channels) uint8.  Raises AssertionError on anything a strict reader would refuse."""
    data = bytes(data)
    assert data[:8] == SIGNATURE, 'signature'
    at, chunks = 8, []
    while at < len(data):
        assert at + 12 <= len(data), 'truncated chunk header at %d' % at
        n, kind = struct.unpack('>I4s', data[at:at + 8])
        assert at + 12 + n <= len(data), 'chunk %r runs past the end' % kind
        body = data[at + 8:at + 8 + n]
        crc, = struct.unpack('>I', data[at + 8 + n:at + 12 + n])
        assert zlib.crc32(kind + body) & 0xffffffff == crc, 'CRC of chunk %d (%r, %d bytes)' % (len(chunks), kind, n)
        chunks.append((kind, body))
        at += 12 + n
        if kind == b'IEND':
            break
    assert at == len(data), '%d bytes after IEND' % (len(data) - at)
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b'IHDR' and kinds[-1] == b'IEND' and chunks[-1][1] == b'', kinds[:2] + kinds[-2:]
    assert len(kinds) >= 3 and all(k == b'IDAT' for k in kinds[1:-1]), sorted(set(kinds))
    assert len(chunks[0][1]) == 13
    w, h, depth, ctype, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert depth == 8 and ctype in (0, 2) and comp == 0 and filt == 0 and lace == 0, (depth, ctype, comp, filt, lace)
    ch = 3 if ctype == 2 else 1
    raw = zlib.decompress(b''.join(b for k, b in chunks[1:-1]))          # one complete zlib stream: header, blocks, Adler-32
    assert len(raw) == h * (w * ch + 1), (len(raw), h, w, ch)
    rows = np.frombuffer(raw, np.uint8).reshape(h, w * ch + 1)
    out = np.zeros((h, w, ch), np.uint8)
    for y in range(h):
        f, line = int(rows[y, 0]), rows[y, 1:].reshape(w, ch)
        if f == 0:
            out[y] = line
        elif f == 1:
            out[y] = (np.cumsum(line.astype(np.uint64), axis=0) & 255).astype(np.uint8)
        elif f == 2:
            out[y] = line + (out[y - 1] if y else 0)                      # uint8 wraps
        else:
            raise AssertionError('row %d: filter %d is not one the encoder writes' % (y, f))
    return out


def decode_pil(data):
    """the same file through Pillow: (H, W, channels) uint8; the mode must be RGB or L"""
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(data)))
    im.load()
    assert im.mode in ('RGB', 'L'), im.mode
    a = np.asarray(im)
    return a if a.ndim == 3 else a[:, :, None]


def check_both(data, want):
    """both decoders give `want` (H, W, channels) exactly"""
    for name, fn in (('own', decode), ('PIL', decode_pil)):
        got = fn(data)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got, want), '%s decoder: %d bytes differ' % (name, int((got != want).sum()))


def line_drawing(size=256, seed=5):
    """60 random segments of width 2 on white"""
    from PIL import Image, ImageDraw
    rng = np.random.RandomState(seed)
    im = Image.new('RGB', (size, size), (255, 255, 255))
    draw = ImageDraw.Draw(im)
    for _ in range(60):
        x0, y0, x1, y1 = (int(v) for v in rng.randint(0, size, 4))
        draw.line((x0, y0, x1, y1), fill=(0, 0, 0), width=2)
    return np.asarray(im).copy()


def run_row(lengths=(2, 3, 258, 259, 260, 516)):
    """one grey row: white runs of exactly these lengths, a black pixel before, between and after them"""
    row = [0]
    for n in lengths:
        row += [255] * n + [0]
    return np.array(row, np.uint8)


def images():
    """name -> (H, W, channels) uint8: the smallest images that reach each rule of the stream"""
    rng = np.random.RandomState(9)
    cases = {}
    cases['one_pixel_rgb'] = np.array([[[7, 200, 144]]], np.uint8)
    cases['one_pixel_grey'] = np.array([[[143]]], np.uint8)
    cases['noise37x53_rgb'] = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)          # row bytes 160: H is no multiple of the band
    cases['noise37x53_grey'] = rng.randint(0, 256, (37, 53, 1)).astype(np.uint8)
    cases['white_row87'] = np.full((2, 87, 3), 255, np.uint8)                              # 261 bytes: a 258 run + 3
    # rows under Up: above a black row the pattern itself is the filtered row (runs of exactly 2 .. 516 bytes), above itself
    # it filters to zeros; as the first row it goes through Sub
    pattern = run_row()
    cases['runs_grey'] = np.stack([pattern, np.zeros_like(pattern), pattern, pattern])[:, :, None]
    edge = np.array([0, 142, 143, 144, 145, 255, 143, 144, 144, 143, 1, 254], np.uint8)       # 8-bit codes end at literal 143
    cases['literal144'] = np.stack([np.zeros_like(edge), edge, np.zeros_like(edge), edge[::-1]])[:, :, None]
    same = rng.randint(0, 256, (1, 40, 3)).astype(np.uint8)
    cases['up_all_zero'] = np.repeat(same, 21, axis=0)                                       # every Up-filtered row is zeros
    cases['noise256_rgb'] = rng.randint(0, 256, (256, 256, 3)).astype(np.uint8)              # the expansion case
    cases['lines256_rgb'] = line_drawing()
    cases['white256_rgb'] = np.full((256, 256, 3), 255, np.uint8)
    tall = rng.randint(0, 256, (2048, 3, 3)).astype(np.uint8)
    tall[100:1900] = 255
    cases['tall2048x3'] = tall
    wide = rng.randint(0, 256, (3, 2048, 3)).astype(np.uint8)                                # row bytes 6145: bands of 2 rows
    wide[:, 300:1500] = 255
    cases['wide3x2048'] = wide
    cases['wide3x2048_grey'] = wide[:, :, :1].copy()
    return cases


def bound_limit(h, w, ch):
    """the ceiling the issue sets for apd_png_bound"""
    return 9 * h * (w * ch + 1) / 8 + 64 * h + 256


def to_frames(image):
    """(H, W, channels) uint8 -> (1, channels, H, W) float32 whose tensor2im bytes are the image: the middle of each byte's
    interval, (v + 0.5) / 255 * 2 - 1"""
    a = (image.astype(np.float64) + 0.5) / 255.0 * 2.0 - 1.0
    return np.ascontiguousarray(a.transpose(2, 0, 1)[None]).astype(np.float32)
