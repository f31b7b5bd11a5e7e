"""PNG files of 8-bit pictures: RGB [H, W, 3] and grey [H, W], non-interlaced.  Host only: numpy, zlib and struct.

The writer stores every row with filter type 0 (none) in one zlib stream; the reader undoes all five filter types and
verifies every chunk's CRC, so it reads what other encoders write for these two colour types as well.
"""
import struct
import zlib

import numpy as np

_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_CHANNELS = {0: 1, 2: 3}                 # colour type -> samples per pixel


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, rgb, level=6):
    """Write a uint8 array [H, W, 3] (RGB) or [H, W] (grey) as a PNG file."""
    a = np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: expected a uint8 array [H, W, 3] or [H, W], got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + w * (3 if a.ndim == 3 else 1)), dtype=np.uint8)         # column 0: the filter type
    rows[:, 1:] = a.reshape(h, -1)
    header = struct.pack('>IIBBBBB', w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    with open(path, 'wb') as f:
        f.write(_SIGNATURE + _chunk(b'IHDR', header) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level))
                + _chunk(b'IEND', b''))


def _unfilter(rows, bpp):
    """Undo the per-row filters in place; rows is [H, 1 + stride] with the filter type in column 0."""
    h, stride = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((h + 1, stride + bpp), dtype=np.uint8)                   # a zero row above and bpp zero bytes left
    for y in range(h):
        kind, line, above = int(rows[y, 0]), rows[y, 1:], out[y]
        cur = out[y + 1]
        if kind == 0:
            cur[bpp:] = line
        elif kind == 2:
            cur[bpp:] = line + above[bpp:]
        elif kind in (1, 3, 4):
            for x in range(stride):
                left, up, corner = int(cur[x]), int(above[x + bpp]), int(above[x])
                if kind == 1:
                    pred = left
                elif kind == 3:
                    pred = (left + up) >> 1
                else:
                    p = left + up - corner
                    pa, pb, pc = abs(p - left), abs(p - up), abs(p - corner)
                    pred = left if pa <= pb and pa <= pc else (up if pb <= pc else corner)
                cur[x + bpp] = (int(line[x]) + pred) & 0xff
        else:
            raise ValueError("read_png: filter type %d" % kind)
    return out[1:, bpp:]


def read_png(path):
    """The picture of an 8-bit RGB or grey non-interlaced PNG file as uint8 [H, W, 3] or [H, W]."""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:8] != _SIGNATURE:
        raise ValueError("read_png: %s is not a PNG file" % (path,))
    at, header, packed = 8, None, []
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError("read_png: truncated chunk")
        (length,), kind = struct.unpack('>I', data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + length]
        if len(body) != length or at + 12 + length > len(data):
            raise ValueError("read_png: truncated chunk %r" % kind)
        (crc,) = struct.unpack('>I', data[at + 8 + length:at + 12 + length])
        if crc != zlib.crc32(kind + body) & 0xffffffff:
            raise ValueError("read_png: CRC mismatch in chunk %r" % kind)
        at += 12 + length
        if kind == b'IHDR':
            header = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            packed.append(body)
        elif kind == b'IEND':
            break
    if header is None or not packed:
        raise ValueError("read_png: no IHDR or no IDAT chunk")
    w, h, depth, colour, compression, filtering, interlace = header
    if depth != 8 or colour not in _CHANNELS or compression or filtering or interlace:
        raise ValueError("read_png: only 8-bit RGB or grey, non-interlaced (depth %d, colour type %d, interlace %d)"
                         % (depth, colour, interlace))
    bpp = _CHANNELS[colour]
    raw = np.frombuffer(zlib.decompress(b''.join(packed)), dtype=np.uint8)
    if raw.size != h * (1 + w * bpp):
        raise ValueError("read_png: %d bytes of picture data for %d x %d" % (raw.size, w, h))
    pixels = _unfilter(raw.reshape(h, 1 + w * bpp), bpp)
    return np.ascontiguousarray(pixels.reshape(h, w, 3) if bpp == 3 else pixels.reshape(h, w))
