"""AVI 1.0 writer for a clip of JPEG frames with PCM sound: the host half of ``end2end.py --video avi``.  The frames are the
complete baseline JPEG files apd_jpeg_encode makes on the device (data/visuals.encode_jpeg_batch); this module only shuffles
bytes.

    RIFF 'AVI '
      LIST 'hdrl'   avih, LIST 'strl' (strh vids / MJPG, strf BITMAPINFOHEADER) [, LIST 'strl' (strh auds, strf WAVEFORMATEX)]
      LIST 'movi'   00dc (one JPEG file), 01wb (the sound of that frame's time), 00dc, 01wb, ...
      idx1          one AVIOLDINDEX entry per chunk, offsets from the 'movi' fourcc

One RIFF, no OpenDML: a file that would pass 2^31 - 2^20 bytes is refused.  Nothing is resampled or re-encoded."""
import fractions
import struct
import wave

AVIF_HASINDEX, AVIF_ISINTERLEAVED, AVIIF_KEYFRAME = 0x10, 0x100, 0x10


def fps_fraction(fps):
    """62.5 -> (125, 2): dwRate / dwScale of the video stream"""
    f = fractions.Fraction(fps).limit_denominator(1001)
    if f <= 0:
        raise ValueError('avi: fps = %r' % (fps,))
    return f.numerator, f.denominator


def read_wav(path):
    """(channels, sample width in bytes, rate, sample bytes) of a PCM wav through the stdlib; anything but 8- or 16-bit PCM with
    1 or 2 channels is refused by name"""
    try:
        with wave.open(path, 'rb') as w:
            channels, width, rate = w.getnchannels(), w.getsampwidth(), w.getframerate()
            if w.getcomptype() != 'NONE':
                raise ValueError('avi: %s is %s-compressed; served: 8- and 16-bit PCM' % (path, w.getcomptype()))
            data = w.readframes(w.getnframes())
    except wave.Error as e:
        with open(path, 'rb') as f:
            head = f.read(4096)
        at = head.find(b'fmt ')
        tag = struct.unpack('<H', head[at + 8:at + 10])[0] if at >= 0 and at + 10 <= len(head) else None
        names = {3: 'IEEE float', 6: 'A-law', 7: 'mu-law', 0xFFFE: 'WAVE_FORMAT_EXTENSIBLE'}
        raise ValueError('avi: %s is not a PCM wav the stdlib reads (%s; format tag %s%s); served: 8- and 16-bit PCM'
                         % (path, e, tag, ', ' + names[tag] if tag in names else ''))
    if width not in (1, 2) or channels not in (1, 2):
        raise ValueError('avi: %s holds %d-bit PCM with %d channels; served: 8- and 16-bit PCM, 1 or 2 channels'
                         % (path, 8 * width, channels))
    return channels, width, rate, data[:len(data) - len(data) % (channels * width)]


class AviWriter:
    """``AviWriter(path, width, height, fps_num, fps_den, audio=None)``; ``add_frames(buf, sizes)`` appends frames
    ``buf[i][:sizes[i]]`` (each followed by its share of the sound), ``close()`` writes the index and patches the counts.
    ``audio``: path of a PCM wav (read_wav).  Audio chunk k holds the sample frames from floor(k rate fps_den / fps_num) to
    floor((k + 1) rate fps_den / fps_num); what is left after the last video frame goes into one last chunk."""

    MAX_BYTES = 2 ** 31 - 2 ** 20

    def __init__(self, path, width, height, fps_num, fps_den, audio=None):
        if not (0 < width < 65536 and 0 < height < 65536 and fps_num > 0 and fps_den > 0):
            raise ValueError('avi: %r x %r at %r / %r fps' % (width, height, fps_num, fps_den))
        self.path, self.width, self.height, self.fps_num, self.fps_den = path, int(width), int(height), int(fps_num), int(fps_den)
        self.audio = read_wav(audio) if audio is not None else None
        self.frames = self.audio_at = 0                # video frames written, sample frames written
        self.index, self.largest = [], [0, 0]          # (fourcc, flags, offset, size); the largest chunk per stream
        self.f = open(path, 'wb')
        self.f.write(self._headers(0, 0))
        self.movi_at = self.f.tell() - 4               # the 'movi' fourcc
        self.at = self.f.tell()
        self.closed = False

    def _headers(self, riff_size, movi_size):
        usec = (1000000 * self.fps_den + self.fps_num // 2) // self.fps_num
        per_frame = self.largest[0] + self.largest[1]
        streams = 2 if self.audio else 1
        avih = struct.pack('<14I', usec, per_frame * self.fps_num // self.fps_den, 0, AVIF_HASINDEX | AVIF_ISINTERLEAVED, self.frames, 0,
                           streams, per_frame, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIII4h', b'vids', b'MJPG', 0, 0, 0, 0, self.fps_den, self.fps_num, 0, self.frames, self.largest[0],
                           0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.width, self.height, 1, 24, b'MJPG', self.width * self.height * 3, 0, 0, 0, 0)
        strls = [self._list(b'strl', self._chunk(b'strh', strh) + self._chunk(b'strf', strf))]
        if self.audio:
            channels, width, rate, _ = self.audio
            align = channels * width
            strh = struct.pack('<4s4sIHHIIIIIIII4h', b'auds', b'\0\0\0\0', 0, 0, 0, 0, 1, rate, 0, self.audio_at, self.largest[1], 0xFFFFFFFF,
                               align, 0, 0, 0, 0)
            strf = struct.pack('<HHIIHHH', 1, channels, rate, rate * align, align, 8 * width, 0)
            strls.append(self._list(b'strl', self._chunk(b'strh', strh) + self._chunk(b'strf', strf)))
        hdrl = self._list(b'hdrl', self._chunk(b'avih', avih) + b''.join(strls))
        return b'RIFF' + struct.pack('<I', riff_size) + b'AVI ' + hdrl + b'LIST' + struct.pack('<I', movi_size) + b'movi'

    @staticmethod
    def _chunk(cc, body):
        return cc + struct.pack('<I', len(body)) + body + (b'\0' if len(body) & 1 else b'')

    @staticmethod
    def _list(kind, body):
        return b'LIST' + struct.pack('<I', 4 + len(body)) + kind + body

    def _put(self, stream, cc, flags, body):
        need = self.at + 8 + len(body) + 1 + 16 * (len(self.index) + 1) + 8
        if need > self.MAX_BYTES:
            raise ValueError('avi: %s would pass %d bytes (one RIFF, no OpenDML): write a shorter clip or a lower --video_quality'
                             % (self.path, self.MAX_BYTES))
        self.index.append((cc, flags, self.at - self.movi_at, len(body)))
        self.largest[stream] = max(self.largest[stream], len(body))
        self.f.write(cc + struct.pack('<I', len(body)))
        self.f.write(body)
        if len(body) & 1:
            self.f.write(b'\0')
        self.at += 8 + len(body) + (len(body) & 1)

    def _sound(self, upto):
        """the sample frames [audio_at, upto) as one 01wb chunk; nothing when the wav has run out"""
        channels, width, _, data = self.audio
        align = channels * width
        upto = min(upto, len(data) // align)
        if upto > self.audio_at:
            self._put(1, b'01wb', 0, data[self.audio_at * align:upto * align])
            self.audio_at = upto

    def add_frame(self, data):
        if self.closed:
            raise ValueError('avi: %s is closed' % self.path)
        self._put(0, b'00dc', AVIIF_KEYFRAME, bytes(data))
        self.frames += 1
        if self.audio:
            self._sound(self.frames * self.audio[2] * self.fps_den // self.fps_num)

    def add_frames(self, buf, sizes):
        """buf: (N, slot) uint8 -- a numpy array or a host tensor; sizes: N ints"""
        buf = buf.numpy() if hasattr(buf, 'numpy') else buf
        sizes = sizes.tolist() if hasattr(sizes, 'tolist') else list(sizes)
        for i, size in enumerate(sizes):
            self.add_frame(buf[i, :int(size)].tobytes())

    def close(self):
        if self.closed:
            return
        self.closed = True
        if self.audio:
            self._sound(len(self.audio[3]))
        movi_end = self.at
        self.f.write(self._chunk(b'idx1', b''.join(struct.pack('<4sIII', *e) for e in self.index)))
        end = self.f.tell()
        self.f.seek(0)
        self.f.write(self._headers(end - 8, movi_end - self.movi_at))
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
