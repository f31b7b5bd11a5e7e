"""Triangle meshes as files a viewer or a printer reads: binary STL and binary little-endian PLY.  Host only, numpy only.

STL holds float32 triangles with a normal each and no shared vertices; PLY holds the float64 positions and the int32
face rows as they are, so a PLY round trip is exact and an STL round trip is exact up to float32.  The readers exist for
the round-trip tests and for users; they read what the writers write (plus any binary STL).  A centreline is a PLY of
vertices alone with a radius each (write_points_ply / read_points_ply).
"""
import struct

import numpy as np

_STL_RECORD = np.dtype([('normal', '<f4', (3,)), ('points', '<f4', (3, 3)), ('attribute', '<u2')])
_PLY_FACE = np.dtype([('count', 'u1'), ('index', '<i4', (3,))])


def _arrays(vertices, faces, what):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("%s: vertices must have shape [V, 3], got %s" % (what, v.shape))
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in 'iu':
        raise ValueError("%s: faces must be an integer array [F, 3], got %s %s" % (what, f.dtype, f.shape))
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("%s: a face names a vertex outside 0 .. %d" % (what, len(v) - 1))
    return v, f.astype(np.int32)


def write_stl(path, vertices, faces, header=b''):
    """Binary STL: 80 header bytes, the triangle count, then per triangle the unit normal of its winding (right-hand
    rule; zero for a degenerate triangle), its three points as float32 and a zero attribute."""
    v, f = _arrays(vertices, faces, "write_stl")
    if len(f) >= 1 << 32:
        raise ValueError("write_stl: %d triangles do not fit the format's 32-bit count" % len(f))
    header = bytes(header)[:80]
    if header[:5].lower() == b'solid':
        raise ValueError("write_stl: a binary file's header must not start with 'solid' (readers take it for ASCII)")
    records = np.zeros(len(f), dtype=_STL_RECORD)
    points = v[f]                                                           # [F, 3, 3]
    normal = np.cross(points[:, 1] - points[:, 0], points[:, 2] - points[:, 0])
    length = np.sqrt((normal ** 2).sum(axis=1, keepdims=True))
    records['normal'] = np.divide(normal, length, out=np.zeros_like(normal), where=length > 0)
    records['points'] = points
    with open(str(path), 'wb') as out:
        out.write(header.ljust(80, b'\0'))
        out.write(struct.pack('<I', len(f)))
        out.write(records.tobytes())


def read_stl(path):
    """-> (points float32 [F, 3, 3], normals float32 [F, 3]) of a binary STL file."""
    with open(str(path), 'rb') as src:
        raw = src.read()
    if len(raw) < 84:
        raise ValueError("%s: too short for a binary STL file" % path)
    count = struct.unpack('<I', raw[80:84])[0]
    if len(raw) != 84 + count * _STL_RECORD.itemsize:
        raise ValueError("%s: %d bytes do not hold the %d triangles the header promises (an ASCII STL?)"
                         % (path, len(raw), count))
    records = np.frombuffer(raw, dtype=_STL_RECORD, count=count, offset=84)
    return records['points'].copy(), records['normal'].copy()


def write_ply(path, vertices, faces, comment=None):
    """Binary little-endian PLY: `double` x, y, z per vertex, a list of three `int` vertex indices per face."""
    v, f = _arrays(vertices, faces, "write_ply")
    lines = ['ply', 'format binary_little_endian 1.0']
    if comment:
        lines += ['comment %s' % line for line in str(comment).splitlines()]
    lines += ['element vertex %d' % len(v), 'property double x', 'property double y', 'property double z',
              'element face %d' % len(f), 'property list uchar int vertex_indices', 'end_header']
    records = np.zeros(len(f), dtype=_PLY_FACE)
    records['count'] = 3
    records['index'] = f
    with open(str(path), 'wb') as out:
        out.write(('\n'.join(lines) + '\n').encode('ascii'))
        out.write(v.astype('<f8').tobytes())
        out.write(records.tobytes())


def read_ply(path):
    """-> (vertices float64 [V, 3], faces int32 [F, 3]) of a binary little-endian PLY file with the elements and
    properties write_ply writes (triangles only)."""
    with open(str(path), 'rb') as src:
        raw = src.read()
    end = raw.find(b'end_header\n')
    if not raw.startswith(b'ply\n') or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    header = [line.split() for line in raw[:end].decode('ascii').splitlines() if not line.startswith('comment')]
    wanted = [['ply'], ['format', 'binary_little_endian', '1.0'], ['element', 'vertex'], ['property', 'double', 'x'],
              ['property', 'double', 'y'], ['property', 'double', 'z'], ['element', 'face'],
              ['property', 'list', 'uchar', 'int', 'vertex_indices']]
    if len(header) != len(wanted) or any(line[:len(w)] != w for line, w in zip(header, wanted)):
        raise ValueError("%s: only binary little-endian PLY files of double vertices and int triangle lists are read" % path)
    nv, nf = int(header[2][2]), int(header[6][2])
    body = end + len(b'end_header\n')
    if len(raw) != body + nv * 24 + nf * _PLY_FACE.itemsize:
        raise ValueError("%s: %d bytes do not hold %d vertices and %d triangles" % (path, len(raw), nv, nf))
    vertices = np.frombuffer(raw, dtype='<f8', count=3 * nv, offset=body).reshape(nv, 3).astype(np.float64)
    records = np.frombuffer(raw, dtype=_PLY_FACE, count=nf, offset=body + nv * 24)
    if nf and not (records['count'] == 3).all():
        raise ValueError("%s: a face that is not a triangle" % path)
    return vertices, records['index'].astype(np.int32)


_POINT_HEADER = ['property double x', 'property double y', 'property double z', 'property double radius', 'end_header']


def write_points_ply(path, points, radius, comment=None):
    """Binary little-endian PLY of vertices alone, `double` x, y, z and radius each: a centreline with the radius of the
    structure at every point."""
    p = np.asarray(points, dtype=np.float64)
    r = np.asarray(radius, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or r.shape != (len(p),):
        raise ValueError("write_points_ply: points [V, 3] and radius [V], got %s and %s" % (p.shape, r.shape))
    lines = ['ply', 'format binary_little_endian 1.0']
    if comment:
        lines += ['comment %s' % line for line in str(comment).splitlines()]
    lines += ['element vertex %d' % len(p)] + _POINT_HEADER
    with open(str(path), 'wb') as out:
        out.write(('\n'.join(lines) + '\n').encode('ascii'))
        out.write(np.column_stack((p, r)).astype('<f8').tobytes())


def read_points_ply(path):
    """-> (points float64 [V, 3], radius float64 [V]) of a file write_points_ply wrote."""
    with open(str(path), 'rb') as src:
        raw = src.read()
    end = raw.find(b'end_header\n')
    if not raw.startswith(b'ply\n') or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    header = [line for line in raw[:end + len(b'end_header')].decode('ascii').splitlines() if not line.startswith('comment')]
    if (len(header) != 3 + len(_POINT_HEADER) or header[:2] != ['ply', 'format binary_little_endian 1.0']
            or header[2].split()[:2] != ['element', 'vertex'] or header[3:] != _POINT_HEADER):
        raise ValueError("%s: only binary little-endian PLY files of double x, y, z, radius vertices are read" % path)
    nv = int(header[2].split()[2])
    body = end + len(b'end_header\n')
    if len(raw) != body + nv * 32:
        raise ValueError("%s: %d bytes do not hold %d vertices" % (path, len(raw), nv))
    table = np.frombuffer(raw, dtype='<f8', count=4 * nv, offset=body).reshape(nv, 4).astype(np.float64)
    return np.ascontiguousarray(table[:, :3]), np.ascontiguousarray(table[:, 3])


WRITERS = {'stl': write_stl, 'ply': write_ply}
