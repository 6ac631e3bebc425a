"""Pictures as JPEG and Motion-JPEG: the device encoder of csrc/jpeg.hip behind ``JpegEncoder``, the file header it needs
(``jpeg_header``), an AVI writer (``MjpegWriter``) and the sink the drivers write their overlays through (``OverlaySink``).

The device returns the entropy-coded scan of each picture - libjpeg's integer arithmetic, the fixed ITU T.81 Annex K tables; the host
puts SOI .. SOS in front of it and EOI behind.  Baseline only: no optimised tables, no restart markers, no 4:2:2, no decoder."""
from __future__ import annotations

import ctypes
import os
import struct
from fractions import Fraction
from typing import Dict, List, Optional, Sequence

import numpy as np

MAX_PICTURES = 64
MAX_DIM = 8192

# ITU T.81 Annex K.1 / K.2, natural order
_Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
           103, 99]
_Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] \
    + [99] * 32
_ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
           57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# Annex K.3: (BITS, HUFFVAL) of the DC and AC tables, luminance and chrominance.  The AC symbols are (run << 4 | size), listed by
# code length; both tables hold the same 162 symbols: 0x00, 0xF0 and every run 0 .. 15 with size 1 .. 10.
_DC = (([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
       ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))))
_AC = (([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
        [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
         0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
         0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
         0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
         0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
         0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
         0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
         0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
       ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
        [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
         0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
         0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
         0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
         0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
         0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
         0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
         0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]))


def _subsampling(s) -> int:
    v = int(str(s).replace(":", ""))
    if v not in (444, 420):
        raise ValueError(f"subsampling must be 444 or 420, not {s!r}")
    return v


def _quality(q) -> int:
    q = int(q)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be 1 .. 100, not {q}")
    return q


def quant_tables(quality: int):
    """-> (luminance, chrominance): uint8 [64] in natural (row-major) order, Annex K scaled as libjpeg's jpeg_set_quality does."""
    q = _quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255).astype(np.uint8) for base in (_Q_LUMA, _Q_CHROMA))


def huffman_tables() -> Dict[str, tuple]:
    """{'dc_luma', 'ac_luma', 'dc_chroma', 'ac_chroma'}: (BITS uint8 [16]: codes per length 1 .. 16, HUFFVAL uint8: the symbols)."""
    pack = lambda t: (np.asarray(t[0], np.uint8), np.asarray(t[1], np.uint8))
    return dict(dc_luma=pack(_DC[0]), ac_luma=pack(_AC[0]), dc_chroma=pack(_DC[1]), ac_chroma=pack(_AC[1]))


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_header(W: int, H: int, quality: int, subsampling=444) -> bytes:
    """Everything of a baseline JFIF file in front of the scan: SOI, APP0 (JFIF 1.01, aspect 1:1, no thumbnail), two DQT, SOF0, the
    four DHT and SOS.  A file is ``jpeg_header(...) + scan + EOI``."""
    W, H, sub = int(W), int(H), _subsampling(subsampling)
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError(f"picture size {(W, H)} outside 1 .. 65535")
    ql, qc = quant_tables(quality)
    zz = np.asarray(_ZIGZAG)
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for i, q in enumerate((ql, qc)):
        out.append(_segment(0xDB, bytes([i]) + q[zz].tobytes()))
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x11 if sub == 444 else 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    h = huffman_tables()
    for tc_th, key in ((0x00, "dc_luma"), (0x10, "ac_luma"), (0x01, "dc_chroma"), (0x11, "ac_chroma")):
        out.append(_segment(0xC4, bytes([tc_th]) + h[key][0].tobytes() + h[key][1].tobytes()))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


EOI = b"\xff\xd9"


def jpeg_size(data: bytes):
    """(W, H) from the first frame header (SOF0 .. SOF2) of a JPEG file."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file")
    i = 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if m in (0xC0, 0xC1, 0xC2):
            h, w = struct.unpack(">HH", data[i + 5:i + 9])
            return w, h
        if m == 0xDA:
            break
        i += 2 + n
    raise ValueError("no frame header in the JPEG file")


class JpegDesc(ctypes.Structure):
    """dyb_jpeg_desc (include/dynaboa_hip.h): one picture of a call."""
    _fields_ = [("rgb", ctypes.c_void_p), ("out", ctypes.c_void_p), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("capacity", ctypes.c_longlong)]


class JpegEncoder:
    """``encode(pictures)``: uint8 RGB (H, W, 3) tensors on the device, of any sizes -> one whole JFIF file (bytes) each; 64 pictures per
    device call.  The workspace, the arena the scans land in and the pinned staging buffer are kept between calls and grown when a
    call needs more.  A call waits once, for the scans' lengths, and copies only the used bytes to the host.  A picture whose scan
    did not fit its default room of H W 3 / 2 + 4096 bytes (noise at quality 100 needs more than its raw size) is encoded again, alone,
    with exactly the room its length asks for."""

    def __init__(self, device, quality: int = 90, subsampling="444"):
        import torch
        self.device = torch.device(device)
        self.quality = _quality(quality)
        self.subsampling = _subsampling(subsampling)
        self._ws = self._arena = self._pinned = None
        self._lengths = torch.empty(MAX_PICTURES, dtype=torch.int64, device=self.device)
        self._lengths_host = torch.empty(MAX_PICTURES, dtype=torch.int64).pin_memory() if self.device.type == "cuda" else None
        self.bytes_to_host = 0                         # of the last encode(): the used scan bytes + the lengths
        self.retries = 0                               # pictures encoded again for want of room, over the encoder's life

    def _grow(self, name: str, nbytes: int, pinned: bool = False):
        import torch
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cpu" if pinned else self.device)
            if pinned and self.device.type == "cuda":
                buf = buf.pin_memory()
            setattr(self, name, buf)
        return buf

    def _launch(self, pics, caps):
        """dyb_jpeg_encode_many alone: the launches are issued, nothing is waited for -> (arena, offsets)"""
        from . import _lib
        from ._abi import check
        from .hmr import stream_of
        N = len(pics)
        offs, at = [], 0
        for c in caps:
            offs.append(at)
            at += (c + 15) & ~15
        arena = self._grow("_arena", at)
        desc = (JpegDesc * N)()
        for i, (p, c) in enumerate(zip(pics, caps)):
            desc[i] = JpegDesc(p.data_ptr(), arena.data_ptr() + offs[i], int(p.shape[0]), int(p.shape[1]), c)
        lib = _lib.load()
        table = ctypes.cast(desc, ctypes.c_void_p)
        need = int(lib.dyb_jpeg_workspace_bytes(table, N, self.subsampling))
        if need == 0:
            raise ValueError("dyb_jpeg_workspace_bytes refuses the pictures' sizes")
        ws = self._grow("_ws", need)
        check(lib.dyb_jpeg_encode_many(table, N, self.quality, self.subsampling, self._lengths.data_ptr(), ws.data_ptr(), ws.numel(),
                                       stream_of(arena)), "dyb_jpeg_encode_many")
        return arena, offs

    def _call(self, pics, caps):
        """one device call -> (lengths list, arena, offsets): the scans lie at arena[offsets[i] : offsets[i] + min(length, cap)]"""
        import torch
        N = len(pics)
        arena, offs = self._launch(pics, caps)
        if self._lengths_host is not None:
            self._lengths_host[:N].copy_(self._lengths[:N], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()               # the one wait of the call
            lengths = self._lengths_host[:N].tolist()
        else:
            lengths = self._lengths[:N].tolist()
        return lengths, arena, offs

    def _scans(self, pics) -> List[bytes]:
        import torch
        caps = [int(p.shape[0]) * int(p.shape[1]) * 3 // 2 + 4096 for p in pics]
        lengths, arena, offs = self._call(pics, caps)
        fit = [i for i in range(len(pics)) if lengths[i] <= caps[i]]
        total = sum(lengths[i] for i in fit)
        stage = self._grow("_pinned", total, pinned=True)
        at, where = 0, {}
        for i in fit:                                                          # only the used bytes cross to the host
            stage[at:at + lengths[i]].copy_(arena[offs[i]:offs[i] + lengths[i]], non_blocking=True)
            where[i] = at
            at += lengths[i]
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        host = stage.numpy()
        out: List[Optional[bytes]] = [host[where[i]:where[i] + lengths[i]].tobytes() if i in where else None for i in range(len(pics))]
        self.bytes_to_host += total + 8 * len(pics)
        for i in range(len(pics)):
            if out[i] is None:                                                 # too little room: again, alone, with what it needs
                self.retries += 1
                n = int(lengths[i])
                again, arena, offs = self._call([pics[i]], [n])
                if again[0] != n:
                    raise RuntimeError(f"JPEG scan of {again[0]} bytes where {n} were announced")
                out[i] = arena[offs[0]:offs[0] + n].cpu().numpy().tobytes()
                self.bytes_to_host += n + 8
        return out

    def encode(self, pictures: Sequence) -> List[bytes]:
        import torch
        pics = []
        for p in pictures:
            p = torch.as_tensor(p)
            if p.dtype != torch.uint8 or p.dim() != 3 or p.shape[2] != 3:
                raise ValueError("a picture must be uint8 RGB (H, W, 3)")
            if not (1 <= p.shape[0] <= MAX_DIM and 1 <= p.shape[1] <= MAX_DIM):
                raise ValueError(f"picture size {tuple(p.shape[:2])} outside 1 .. {MAX_DIM}")
            pics.append(p.detach().to(self.device).contiguous())
        self.bytes_to_host = 0
        files: List[bytes] = []
        for lo in range(0, len(pics), MAX_PICTURES):
            part = pics[lo:lo + MAX_PICTURES]
            for p, scan in zip(part, self._scans(part)):
                files.append(jpeg_header(int(p.shape[1]), int(p.shape[0]), self.quality, self.subsampling) + scan + EOI)
        return files

    def save(self, pictures: Sequence, paths: Sequence[str]) -> List[str]:
        if len(pictures) != len(paths):
            raise ValueError("one path per picture")
        for data, path in zip(self.encode(pictures), paths):
            with open(path, "wb") as fh:
                fh.write(data)
        return list(paths)


# ---- Motion-JPEG in AVI 1.0 -------------------------------------------------------------------------------------------------------
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
AVI_LIMIT = 1 << 30


class MjpegWriter:
    """RIFF 'AVI ' (AVI 1.0): LIST hdrl (avih; LIST strl (strh 'vids' / 'MJPG', strf BITMAPINFOHEADER 24 bit 'MJPG')), LIST movi with one
    '00dc' chunk per frame (padded to even length) and idx1, every entry a key frame.  ``add(jpeg_bytes)`` takes a whole JFIF file
    (with its DHT: a decoder needs no default tables) of exactly ``width`` x ``height``; sizes and frame counts are patched by
    ``close()``.  Before a file would pass ``limit`` bytes (1 GiB) it is closed and the writer goes on in ``<stem>_part2.avi``,
    ``_part3`` ...; ``paths`` lists the files written.  fps is kept as the fraction rate / scale."""

    _MOVI_AT = 12 + 8 + 4 + 8 + 56 + 8 + 4 + 8 + 56 + 8 + 40         # where the LIST 'movi' chunk begins

    def __init__(self, path, width: int, height: int, fps=30, limit: int = AVI_LIMIT):
        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1:
            raise ValueError("a video needs a positive size")
        fr = Fraction(str(fps)).limit_denominator(100000)
        if fr <= 0:
            raise ValueError("fps must be positive")
        self.rate, self.scale = fr.numerator, fr.denominator
        self.limit = int(limit)
        self._first = str(path)
        self.paths: List[str] = []
        self.frames = 0                                 # over all parts
        self._fh = None
        self._open(self._first)

    def _open(self, path: str):
        self._fh = open(path, "wb")
        self.paths.append(path)
        self._index: List[tuple] = []
        self._largest = 0
        self._fh.write(self._headers(0, 0, 0))
        self._fh.write(b"LIST" + struct.pack("<I", 4) + b"movi")
        self._pos = self._MOVI_AT + 12

    def _headers(self, nframes: int, largest: int, riff_size: int) -> bytes:
        usec = (1000000 * self.scale + self.rate // 2) // self.rate
        per_sec = (largest * self.rate + self.scale - 1) // self.scale
        avih = struct.pack("<14I", usec, min(per_sec, 0xFFFFFFFF), 0, AVIF_HASINDEX, nframes, 0, 1, largest, self.width, self.height,
                           0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, self.scale, self.rate, 0, nframes, largest, 0xFFFFFFFF, 0,
                                         0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        out = b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
        assert len(out) == self._MOVI_AT
        return out

    def add(self, jpeg_bytes: bytes) -> None:
        if self._fh is None:
            raise ValueError("the writer is closed")
        size = jpeg_size(jpeg_bytes)
        if size != (self.width, self.height):
            raise ValueError(f"a frame of {size[0]} x {size[1]} in a video of {self.width} x {self.height}")
        n = len(jpeg_bytes)
        chunk = 8 + n + (n & 1)
        # what the file would be with this frame in it: the chunks so far, this one, the index
        if self._index and self._pos + chunk + 8 + 16 * (len(self._index) + 1) > self.limit:
            self._finish()
            stem, ext = os.path.splitext(self._first)
            self._open(f"{stem}_part{len(self.paths) + 1}{ext}")
        self._fh.write(b"00dc" + struct.pack("<I", n) + jpeg_bytes + (b"\x00" if n & 1 else b""))
        self._index.append((self._pos - (self._MOVI_AT + 8), n))      # from the 'movi' fourcc, as AVI 1.0 counts
        self._pos += chunk
        self._largest = max(self._largest, n)
        self.frames += 1

    def _finish(self):
        fh, n = self._fh, len(self._index)
        fh.write(b"idx1" + struct.pack("<I", 16 * n))
        fh.write(b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, off, size) for off, size in self._index))
        end = self._pos + 8 + 16 * n
        fh.seek(0)
        fh.write(self._headers(n, self._largest, end - 8))
        fh.write(b"LIST" + struct.pack("<I", self._pos - self._MOVI_AT - 8) + b"movi")
        fh.close()
        self._fh = None

    def close(self) -> None:
        if self._fh is not None:
            self._finish()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ---- what the drivers write their pictures through --------------------------------------------------------------------------------
def add_arguments(parser) -> None:
    """--overlay_format / --jpeg_quality / --jpeg_subsampling / --overlay_video / --video_fps: every default is the PNG behaviour."""
    parser.add_argument('--overlay_format', type=str, default='png', choices=['png', 'jpg'],
                        help='the pictures --save_res 1 / --scene_overlays 1 / the online driver write: png (PIL on the host) or jpg '
                             '(encoded on the device, same names with the extension .jpg)')
    parser.add_argument('--jpeg_quality', type=int, default=90, help='1 .. 100, libjpeg\'s scale')
    parser.add_argument('--jpeg_subsampling', type=str, default='444', choices=['444', '420'],
                        help='444 by default: wireframe edges are one pixel wide and coloured')
    parser.add_argument('--overlay_video', type=int, default=0, choices=[0, 1],
                        help='1: also write the pictures of each sequence as a Motion-JPEG .avi (implies the device JPEG encode for '
                             'the video, whatever --overlay_format says for the per-picture files)')
    parser.add_argument('--video_fps', type=float, default=30.0)


def wants_sink(options) -> bool:
    return getattr(options, "overlay_format", "png") == "jpg" or bool(int(getattr(options, "overlay_video", 0) or 0))


class OverlaySink:
    """Writes the finished pictures of a driver.  ``write(pictures, paths, videos)``: all pictures go through ONE
    ``JpegEncoder.encode`` call; with ``fmt == 'jpg'`` picture i is written at paths[i] with the extension .jpg, else as PNG at
    paths[i] as before (None: no picture file); with ``video`` it is appended to the Motion-JPEG file videos[i] (None: no video for
    it).  Every video path has a writer of its own - another sequence is another path - that stays open between calls until
    ``close()``, so frames of several sequences may arrive interleaved.  When the pictures of one path change size (3DPW mixes
    1920 x 1080 and 1080 x 1920) its writer is closed and the path goes on in ``<stem>_2.avi``, ``_3`` ...  ``close()`` ends every
    video and forgets the counts: a path asked for after it starts over and replaces the file of that name."""

    def __init__(self, device, fmt: str = "png", quality: int = 90, subsampling="444", video: bool = False, fps=30.0):
        if fmt not in ("png", "jpg"):
            raise ValueError("overlay_format must be png or jpg")
        self.fmt, self.video, self.fps = fmt, bool(video), fps
        self.encoder = JpegEncoder(device, quality, subsampling)
        self._writers: Dict[str, MjpegWriter] = {}
        self._serial: Dict[str, int] = {}
        self.video_paths: List[str] = []

    @classmethod
    def from_options(cls, options, device):
        return cls(device, getattr(options, "overlay_format", "png"), int(getattr(options, "jpeg_quality", 90)),
                   getattr(options, "jpeg_subsampling", "444"), bool(int(getattr(options, "overlay_video", 0) or 0)),
                   float(getattr(options, "video_fps", 30.0)))

    def picture_path(self, path: str) -> str:
        return os.path.splitext(path)[0] + ".jpg" if self.fmt == "jpg" else path

    def _writer(self, key: str, W: int, H: int) -> MjpegWriter:
        w = self._writers.get(key)
        if w is not None and (w.width, w.height) != (W, H):
            w.close()
            w = None
        if w is None:
            n = self._serial[key] = self._serial.get(key, 0) + 1
            stem, ext = os.path.splitext(key)
            path = key if n == 1 else f"{stem}_{n}{ext}"
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            w = self._writers[key] = MjpegWriter(path, W, H, self.fps)
            self.video_paths.append(path)
        return w

    def write(self, pictures, paths, videos=None) -> List[str]:
        files = self.encoder.encode(pictures) if pictures else []
        written = []
        for i, (pic, data) in enumerate(zip(pictures, files)):
            if paths[i] is not None:                                   # (None: a picture for the video alone)
                out = self.picture_path(paths[i])
                if self.fmt == "jpg":
                    with open(out, "wb") as fh:
                        fh.write(data)
                else:
                    from PIL import Image
                    Image.fromarray(pic.cpu().numpy()).save(out)
                written.append(out)
            if self.video and videos is not None and videos[i] is not None:
                self._writer(videos[i], int(pic.shape[1]), int(pic.shape[0])).add(data)
        return written

    def close(self) -> None:
        for w in self._writers.values():
            w.close()
        self._writers.clear()
        self._serial.clear()


def sink_for(options, device) -> Optional[OverlaySink]:
    """A new sink for these flags on this device, owned by the caller (who closes it: an adaptor, a replica group, a driver's pass);
    None when the flags ask for PNG files and no video - nothing changes then."""
    return OverlaySink.from_options(options, device) if wants_sink(options) else None
