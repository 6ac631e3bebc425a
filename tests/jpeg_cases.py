"""Baseline JPEG scan, restated in NumPy from the rules of include/dynaboa_hip.h (dyb_jpeg_encode_many), and the cases of
tests/test_jpeg_kernels.py written once for both backends of tests/backends.py.

The restatement is the yardstick of the device encoder and is itself pinned to libjpeg: tests/test_jpeg_host.py compares `scan`
with the scan bytes inside the file PIL writes for the same picture, quality and subsampling.  The tables below are this file's own
copies (ITU T.81 Annex K), typed apart from dynaboa_amd/jpeg.py on purpose."""
from __future__ import annotations

import ctypes
import io

import numpy as np

Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
     0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
     0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
     0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
     0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
     0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
     0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
     0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
     0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
     0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def _huff(bits, vals):
    """{symbol: (code, length)}: Annex C - codes of one length count upwards, doubling at each longer length"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


HUFF_DC = tuple(_huff(DC_BITS[t], DC_VALS[t]) for t in range(2))
HUFF_AC = tuple(_huff(AC_BITS[t], AC_VALS[t]) for t in range(2))


def quant(quality):
    """the two tables in natural order, scaled as libjpeg's jpeg_set_quality does"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (Q_LUMA, Q_CHROMA))


def _D(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(v, n, first):
    """one pass over the last axis of v [..., 8] (int64)"""
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., i] for i in range(8))
    t0, t1, t2, t3 = v0 + v7, v1 + v6, v2 + v5, v3 + v4
    t7, t6, t5, t4 = v0 - v7, v1 - v6, v2 - v5, v3 - v4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _D(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _D(t10 - t11, 2)
    z = (t12 + t13) * 4433
    o[2] = _D(z + t13 * 6270, n)
    o[6] = _D(z - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _D(t4 + z1 + z3, n), _D(t5 + z2 + z4, n), _D(t6 + z2 + z3, n), _D(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(blocks, q):
    """blocks [n][8][8] level-shifted samples, q [64] natural order -> [n][64] quantised, zig-zag order"""
    b = blocks.astype(np.int64)
    b = _dct_pass(b, 11, True)                                   # rows
    b = _dct_pass(b.transpose(0, 2, 1), 15, False).transpose(0, 2, 1)   # columns
    c = b.reshape(-1, 64)
    d = 8 * q.astype(np.int64)
    out = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    return out[:, ZIGZAG]


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def _extend(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _blocks(p):
    """[8 a][8 b] -> [a][b][8][8]"""
    a, b = p.shape[0] // 8, p.shape[1] // 8
    return p.reshape(a, 8, b, 8).transpose(0, 2, 1, 3)


def coefficients(rgb, quality, subsampling):
    """-> list of (component, [64] zig-zag coefficients or None for a dummy block) in coding order"""
    H, W = rgb.shape[:2]
    ql, qc = quant(quality)
    y, cb, cr = ycc(rgb)
    out = []
    if subsampling == 444:
        bh, bw = -(-H // 8), -(-W // 8)
        planes = [fdct_quant(_blocks(_extend(p, 8 * bh, 8 * bw) - 128).reshape(-1, 8, 8), q).reshape(bh, bw, 64)
                  for p, q in ((y, ql), (cb, qc), (cr, qc))]
        for r in range(bh):
            for c in range(bw):
                for comp in range(3):
                    out.append((comp, planes[comp][r, c]))
        return out
    assert subsampling == 420
    mh, mw = -(-H // 16), -(-W // 16)
    bh, bw = -(-H // 8), -(-W // 8)
    yq = fdct_quant(_blocks(_extend(y, 8 * bh, 8 * bw) - 128).reshape(-1, 8, 8), ql).reshape(bh, bw, 64)
    chroma = []
    for p in (cb, cr):
        p = _extend(p, H + (H & 1), 16 * mw)
        a, b, c, d = p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]
        bias = np.where(np.arange(a.shape[1]) % 2 == 0, 1, 2)[None, :]
        ds = (a + b + c + d + bias) >> 2
        ds = _extend(ds, 8 * mh, 8 * mw)
        chroma.append(fdct_quant(_blocks(ds - 128).reshape(-1, 8, 8), qc).reshape(mh, mw, 64))
    for r in range(mh):
        for c in range(mw):
            for k in range(4):
                br, bc = 2 * r + (k >> 1), 2 * c + (k & 1)
                out.append((0, yq[br, bc] if br < bh and bc < bw else None))
            out.append((1, chroma[0][r, c]))
            out.append((2, chroma[1][r, c]))
    return out


class Stats:
    """what the case set exercised (asserted by the coverage test)"""

    def __init__(self):
        self.dc_cat, self.ac_size = set(), set()
        self.zrl = self.eob = self.no_eob = self.stuffed = self.ends_stuffed = 0


def scan(rgb, quality, subsampling, stats: Stats | None = None) -> bytes:
    """the entropy-coded scan of the picture: stuffed, padded with 1-bits, no markers"""
    acc, nbits, raw = 0, 0, bytearray()

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code
        nbits += length
        while nbits >= 8:
            nbits -= 8
            raw.append((acc >> nbits) & 0xFF)
        acc &= (1 << nbits) - 1

    def value(v, size):
        if size:
            put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)

    pred = [0, 0, 0]
    last_dc = 0
    for comp, zz in coefficients(rgb, quality, subsampling):
        t = 0 if comp == 0 else 1
        dc = last_dc if zz is None else int(zz[0])           # a dummy repeats the block coded just before it (always a Y of its MCU)
        last_dc = dc
        diff = dc - pred[comp]
        pred[comp] = dc
        cat = abs(diff).bit_length()
        put(*HUFF_DC[t][cat])
        value(diff, cat)
        if stats:
            stats.dc_cat.add(cat)
        run = 0
        if zz is not None:
            for k in range(1, 64):
                v = int(zz[k])
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    put(*HUFF_AC[t][0xF0])
                    run -= 16
                    if stats:
                        stats.zrl += 1
                size = abs(v).bit_length()
                put(*HUFF_AC[t][(run << 4) | size])
                value(v, size)
                run = 0
                if stats:
                    stats.ac_size.add(size)
        else:
            run = 63
        if run:
            put(*HUFF_AC[t][0x00])
        if stats:
            stats.eob += 1 if run else 0
            stats.no_eob += 0 if run else 1
    if nbits:
        put((1 << (8 - nbits)) - 1, 8 - nbits)
    out = bytearray()
    for b in raw:
        out.append(b)
        if b == 0xFF:
            out.append(0)
    if stats:
        stats.stuffed += sum(1 for b in raw if b == 0xFF)
        stats.ends_stuffed += 1 if raw and raw[-1] == 0xFF else 0
    return bytes(out)


# ---- pictures ---------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (33, 17), (24, 40), (40, 56), (31, 8)]        # (H, W)
CONTENTS = ["noise", "gradient", "zeros", "full", "pixel_checker", "block_checker"]
QUALITIES = [10, 50, 90, 100]
SUBSAMPLINGS = [444, 420]


def picture(content, H, W, seed=0):
    yy, xx = np.mgrid[0:H, 0:W]
    if content == "noise":
        return np.random.default_rng(1000 * H + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if content == "gradient":
        return np.stack([(255 * xx) // max(W - 1, 1), (255 * yy) // max(H - 1, 1), (255 * (xx + yy)) // max(H + W - 2, 1)],
                        axis=-1).astype(np.uint8)
    if content == "zeros":
        return np.zeros((H, W, 3), np.uint8)
    if content == "full":
        return np.full((H, W, 3), 255, np.uint8)
    if content == "pixel_checker":
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    if content == "block_checker":
        return np.repeat(((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    raise ValueError(content)


def pil_scan(rgb, quality, subsampling):
    """the scan inside the file PIL (libjpeg) writes: the bytes after the SOS segment up to EOI"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=0 if subsampling == 444 else 2)
    data = buf.getvalue()
    i = 2
    while data[i + 1] != 0xDA:
        i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    assert data[-2:] == b"\xff\xd9"
    return data[i:-2], data


# ---- the C ABI on either backend --------------------------------------------------------------------------------------------------
class Desc(ctypes.Structure):
    _fields_ = [("rgb", ctypes.c_void_p), ("out", ctypes.c_void_p), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("capacity", ctypes.c_longlong)]


GUARD = 0xA5
TAIL = 64                                             # guard bytes behind every capacity


def _u8(be, a):
    if be.name == "emu":
        return be.dev(a, dtype=np.uint8)
    t = be.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(be.device)
    be._keep.append(t)
    return t


def _i64(be, n):
    if be.name == "emu":
        return np.full(n, -7, np.int64)
    return be.torch.full((n,), -7, dtype=be.torch.int64, device=be.device)


def encode(be, pictures, quality, subsampling, capacities=None, ws_short=0):
    """one dyb_jpeg_encode_many call -> (rc, lengths [N], outs: list of uint8 arrays of capacity + TAIL bytes, guard filled)"""
    N = len(pictures)
    caps = capacities or [p.shape[0] * p.shape[1] * 3 // 2 + 4096 for p in pictures]
    rgb = [_u8(be, p) for p in pictures]
    outs = [_u8(be, np.full(c + TAIL, GUARD, np.uint8)) for c in caps]
    table = (Desc * N)(*[Desc(be.ptr(r), be.ptr(o), p.shape[0], p.shape[1], c) for r, o, p, c in zip(rgb, outs, pictures, caps)])
    need = be.lib.dyb_jpeg_workspace_bytes(ctypes.cast(table, ctypes.c_void_p), N, subsampling)
    assert need > 0
    ws = _u8(be, np.zeros(need, np.uint8))
    lengths = _i64(be, N)
    rc = be.lib.dyb_jpeg_encode_many(ctypes.cast(table, ctypes.c_void_p), N, quality, subsampling, be.ptr(lengths), be.ptr(ws),
                                     need - ws_short, be.stream)
    be.sync()
    return rc, be.host(lengths), [be.host(o) for o in outs]


def check_one(be, rgb, quality, subsampling, want=None):
    want = scan(rgb, quality, subsampling) if want is None else want
    # (noise at quality 100 needs more than the wrapper's default capacity; the capacity cases cover too little room)
    rc, lengths, outs = encode(be, [rgb], quality, subsampling, [max(rgb.shape[0] * rgb.shape[1] * 3 // 2 + 4096, len(want))])
    assert rc == 0, rc
    assert int(lengths[0]) == len(want), (int(lengths[0]), len(want))
    got = outs[0]
    assert bytes(got[:len(want)]) == want
    cap = len(got) - TAIL
    assert (got[cap:] == GUARD).all()


# ---- cases ------------------------------------------------------------------------------------------------------------------------
_WANT = {}


def want(content, H, W, quality, subsampling):
    """the restatement's scan, computed once per picture and shared by the emulator and the device tests"""
    key = (content, H, W, quality, subsampling)
    if key not in _WANT:
        _WANT[key] = scan(picture(content, H, W), quality, subsampling)
    return _WANT[key]


def case_equal(be, content, subsampling, quality):
    """every size of the issue's list, one picture per call"""
    for H, W in SIZES:
        check_one(be, picture(content, H, W), quality, subsampling, want(content, H, W, quality, subsampling))


def coverage():
    st = Stats()
    for H, W in SIZES:
        for content in CONTENTS:
            for q in QUALITIES:
                for s in SUBSAMPLINGS:
                    scan(picture(content, H, W), q, s, st)
    return st


# The emit and stuff kernels work in tiles of 256 stream words = 1024 bytes, the bits kernel in tiles of 1024 blocks, and the scan
# kernel (one code path for both prefixes) walks a picture's tiles 256 at a time.
LARGE = [("noise", 72, 200, 100, 444),       # about 55 KB: more than 4 byte tiles
         ("noise", 264, 200, 50, 420),
         ("gradient", 296, 304, 90, 444),    # 4218 blocks: more than 4 block tiles
         ("noise", 512, 512, 100, 444)]      # 12288 blocks in 12 block tiles and more than 1 MB of scan: more than 4 x 256 byte tiles, so
                                             # the scan kernel's carry between its steps is exercised (through the stuffing prefix)


def case_large(be, i):
    content, H, W, q, s = LARGE[i]
    w = want(content, H, W, q, s)
    if i == 0:
        assert len(w) >= 4 * 1024
    if i == 3:
        assert len(w) > 4 * 256 * 1024
    check_one(be, picture(content, H, W), q, s, w)


RAGGED = [("noise", 17, 33), ("gradient", 40, 56), ("zeros", 1, 1), ("block_checker", 24, 40), ("pixel_checker", 31, 8),
          ("noise", 72, 200), ("full", 9, 7)]


def case_ragged(be, subsampling):
    """seven pictures in one call = each alone; again in reversed order; two calls give equal bytes"""
    q = 90
    pics = [picture(c, H, W) for c, H, W in RAGGED]
    wants = [want(c, H, W, q, subsampling) for c, H, W in RAGGED]
    caps = [max(p.shape[0] * p.shape[1] * 3 // 2 + 4096, len(w)) for p, w in zip(pics, wants)]
    runs = []
    for order in (list(range(7)), list(range(6, -1, -1)), list(range(7))):
        rc, lengths, outs = encode(be, [pics[i] for i in order], q, subsampling, [caps[i] for i in order])
        assert rc == 0
        for slot, i in enumerate(order):
            assert int(lengths[slot]) == len(wants[i]), (i, int(lengths[slot]), len(wants[i]))
            assert bytes(outs[slot][:len(wants[i])]) == wants[i], i
            assert (outs[slot][caps[i]:] == GUARD).all()
        runs.append((lengths.copy(), [o.copy() for o in outs]))
    assert (runs[0][0] == runs[2][0]).all()
    for a, b in zip(runs[0][1], runs[2][1]):
        assert (a == b).all()


def case_capacity(be, subsampling):
    q = 100
    names = [("gradient", 17, 33), ("noise", 40, 56), ("block_checker", 24, 40)]
    pics = [picture(*n) for n in names]
    wants = [want(c, H, W, q, subsampling) for c, H, W in names]
    need = len(wants[1])
    assert need > 40 * 56 * 3 // 2 if subsampling == 444 else True
    for cap, written in ((need - 1, False), (need, True), (0, False), (1021, False)):
        caps = [len(wants[0]) + 5, cap, len(wants[2])]
        rc, lengths, outs = encode(be, pics, q, subsampling, caps)
        assert rc == 0
        assert [int(v) for v in lengths] == [len(w) for w in wants]              # the needed size, whatever the room
        for i in range(3):
            assert (outs[i][caps[i]:] == GUARD).all(), (cap, i)                  # nothing at or beyond out + capacity
        assert bytes(outs[0][:len(wants[0])]) == wants[0] and bytes(outs[2][:len(wants[2])]) == wants[2]
        assert (outs[0][len(wants[0]):] == GUARD).all()                          # nor beyond the scan's own end
        if written:
            assert bytes(outs[1][:need]) == wants[1]


def case_arguments(be):
    """every error code, with outputs and guards untouched"""
    ARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    p = picture("gradient", 17, 33)
    cap = 4096
    rgb = _u8(be, p)

    def call(H=17, W=33, N=1, quality=90, sub=444, rgb_ptr=True, out_ptr=True, lengths_ptr=True, table=True, short=0, capacity=cap):
        out = _u8(be, np.full(cap + TAIL, GUARD, np.uint8))
        lengths = _i64(be, max(N, 1))
        tab = (Desc * max(N, 1))(*[Desc(be.ptr(rgb) if rgb_ptr else None, be.ptr(out) if out_ptr else None, H, W, capacity)
                                   for _ in range(max(N, 1))])
        good = (Desc * 1)(Desc(be.ptr(rgb), be.ptr(out), 17, 33, cap))
        need = be.lib.dyb_jpeg_workspace_bytes(ctypes.cast(good, ctypes.c_void_p), 1, 444)
        ws = _u8(be, np.full(need, GUARD, np.uint8))
        rc = be.lib.dyb_jpeg_encode_many(ctypes.cast(tab, ctypes.c_void_p) if table else None, N, quality, sub,
                                         be.ptr(lengths) if lengths_ptr else None, be.ptr(ws), need - short, be.stream)
        be.sync()
        untouched = bool((be.host(out) == GUARD).all() and (be.host(lengths) == -7).all() and (be.host(ws) == GUARD).all())
        return rc, untouched

    assert call()[0] == 0
    for kw, code in ((dict(table=False), ARG), (dict(rgb_ptr=False), ARG), (dict(out_ptr=False), ARG), (dict(lengths_ptr=False), ARG),
                     (dict(H=0), ARG), (dict(W=-3), ARG), (dict(N=0), ARG), (dict(quality=0), ARG), (dict(quality=101), ARG),
                     (dict(capacity=-1), ARG), (dict(N=65), UNSUPPORTED), (dict(H=8193), UNSUPPORTED), (dict(W=8193), UNSUPPORTED),
                     (dict(sub=422), UNSUPPORTED), (dict(sub=0), UNSUPPORTED), (dict(short=1), WORKSPACE)):
        rc, untouched = call(**kw)
        assert rc == code, (kw, rc)
        assert untouched, kw
    zero = (Desc * 1)(Desc(None, None, 0, 5, 10))
    assert be.lib.dyb_jpeg_workspace_bytes(ctypes.cast(zero, ctypes.c_void_p), 1, 444) == 0
    assert be.lib.dyb_jpeg_workspace_bytes(None, 1, 444) == 0
