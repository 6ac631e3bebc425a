"""The host side of the JPEG path, no GPU: the NumPy restatement of tests/jpeg_cases.py against the scans PIL (libjpeg) writes - the
outside yardstick the device tests lean on -, dynaboa_amd.jpeg's header and tables against PIL's own file, the Motion-JPEG writer by
the structure of its files (a RIFF walker written here from the AVI 1.0 layout) and by decoding its frames, and the new flags."""
import io
import os
import struct

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as J
from dynaboa_amd import jpeg as JP

# the sizes of the device cases and the ones the restatement was first pinned on
PIN_SIZES = sorted(set(J.SIZES + [(16, 24), (48, 64), (72, 200)]))


@pytest.mark.parametrize("content", J.CONTENTS)
def test_restatement_equals_libjpeg(content):
    for H, W in PIN_SIZES:
        rgb = J.picture(content, H, W)
        for q in J.QUALITIES:
            for s in J.SUBSAMPLINGS:
                assert J.scan(rgb, q, s) == J.pil_scan(rgb, q, s)[0], (content, H, W, q, s)


def _segments(data):
    """[(marker, payload)] up to and including SOS, and the offset of the scan"""
    assert data[:2] == b"\xff\xd8"
    i, out = 2, []
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return out, i


def _tables(segs):
    dqt, dht = {}, {}
    for m, p in segs:
        j = 0
        while m == 0xDB and j < len(p):
            assert p[j] >> 4 == 0                                    # 8-bit entries
            dqt[p[j] & 15] = bytes(p[j + 1:j + 65])
            j += 65
        while m == 0xC4 and j < len(p):
            n = sum(p[j + 1:j + 17])
            dht[p[j]] = (bytes(p[j + 1:j + 17]), bytes(p[j + 17:j + 17 + n]))
            j += 17 + n
    return dqt, dht


@pytest.mark.parametrize("quality", J.QUALITIES)
@pytest.mark.parametrize("subsampling", J.SUBSAMPLINGS)
def test_header_tables_equal_pils(quality, subsampling):
    rgb = J.picture("gradient", 17, 33)
    _, theirs = J.pil_scan(rgb, quality, subsampling)
    ours = JP.jpeg_header(33, 17, quality, subsampling)
    a, end = _segments(ours)
    assert end == len(ours)
    b, _ = _segments(theirs)
    assert _tables(a) == _tables(b)
    assert [m for m, _ in a] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    sof = lambda segs: [p for m, p in segs if m == 0xC0][0]
    sos = lambda segs: [p for m, p in segs if m == 0xDA][0]
    assert sof(a) == sof(b) and sos(a) == sos(b)
    app0 = a[0][1]
    assert app0[:5] == b"JFIF\x00" and app0[5:7] == b"\x01\x01" and app0[7] == 0 and app0[8:12] == b"\x00\x01\x00\x01"
    assert app0[12:] == b"\x00\x00"                                  # no thumbnail
    # the exposed constants are what the segments hold
    ql, qc = JP.quant_tables(quality)
    zz = np.asarray(JP._ZIGZAG)
    assert _tables(a)[0] == {0: ql[zz].tobytes(), 1: qc[zz].tobytes()}
    h = JP.huffman_tables()
    assert _tables(a)[1] == {0x00: tuple(x.tobytes() for x in h["dc_luma"]), 0x10: tuple(x.tobytes() for x in h["ac_luma"]),
                             0x01: tuple(x.tobytes() for x in h["dc_chroma"]), 0x11: tuple(x.tobytes() for x in h["ac_chroma"])}


@pytest.mark.parametrize("subsampling", J.SUBSAMPLINGS)
def test_file_decodes_like_pils(subsampling):
    for content, H, W, q in (("noise", 17, 33, 90), ("gradient", 40, 56, 50), ("block_checker", 24, 40, 100), ("zeros", 1, 1, 10)):
        rgb = J.picture(content, H, W)
        data = JP.jpeg_header(W, H, q, subsampling) + J.scan(rgb, q, subsampling) + JP.EOI
        im = Image.open(io.BytesIO(data))
        assert im.size == (W, H) and im.mode == "RGB" and im.format == "JPEG"
        theirs = Image.open(io.BytesIO(J.pil_scan(rgb, q, subsampling)[1]))
        assert np.array_equal(np.asarray(im), np.asarray(theirs))
        assert JP.jpeg_size(data) == (W, H)


def test_argument_checks():
    with pytest.raises(ValueError):
        JP.jpeg_header(8, 8, 0)
    with pytest.raises(ValueError):
        JP.jpeg_header(8, 8, 90, 422)
    with pytest.raises(ValueError):
        JP.quant_tables(101)
    with pytest.raises(ValueError):
        JP.jpeg_size(b"RIFF....")


# ---- AVI ---------------------------------------------------------------------------------------------------------------------------
def _frame(W, H, seed, q=90):
    rgb = J.picture("noise", H, W, seed=seed)
    return JP.jpeg_header(W, H, q, 444) + J.scan(rgb, q, 444) + JP.EOI


def walk(data, lo, hi, depth=0):
    """RIFF chunks of data[lo:hi] -> [(fourcc, payload offset, size, children or None)]; every size must fit and chunks are word aligned"""
    out = []
    while lo < hi:
        assert lo + 8 <= hi
        cc, n = data[lo:lo + 4], struct.unpack("<I", data[lo + 4:lo + 8])[0]
        assert lo + 8 + n <= hi, (cc, n)
        kids = None
        if cc in (b"RIFF", b"LIST"):
            kids = (data[lo + 8:lo + 12], walk(data, lo + 12, lo + 8 + n, depth + 1))
        out.append((cc, lo + 8, n, kids))
        lo += 8 + n + (n & 1)
    assert lo == hi                                                  # a list's size counts its children's padding
    return out


def check_avi(path, frames, width, height, rate, scale):
    data = open(path, "rb").read()
    top = walk(data, 0, len(data))
    assert len(top) == 1 and top[0][0] == b"RIFF" and top[0][2] == len(data) - 8 and top[0][3][0] == b"AVI "
    kids = top[0][3][1]
    assert [c[0] for c in kids] == [b"LIST", b"LIST", b"idx1"]
    hdrl, movi, idx1 = kids
    assert hdrl[3][0] == b"hdrl" and movi[3][0] == b"movi"
    avih, strl = hdrl[3][1]
    assert avih[0] == b"avih" and avih[2] == 56 and strl[3][0] == b"strl"
    a = struct.unpack("<14I", data[avih[1]:avih[1] + 56])
    assert a[0] == round(1e6 * scale / rate) and a[3] & 0x10 and a[4] == len(frames) and a[6] == 1 and a[8:10] == (width, height)
    strh, strf = strl[3][1]
    assert strh[0] == b"strh" and strh[2] == 56 and strf[0] == b"strf" and strf[2] == 40
    assert data[strh[1]:strh[1] + 8] == b"vidsMJPG"
    h = struct.unpack("<IHHIIIIIIII4H", data[strh[1] + 8:strh[1] + 56])
    assert (h[4], h[5]) == (scale, rate) and h[7] == len(frames) and h[11:] == (0, 0, width, height)
    f = struct.unpack("<IiiHH4sIiiII", data[strf[1]:strf[1] + 40])
    assert f[:6] == (40, width, height, 1, 24, b"MJPG")
    chunks = movi[3][1]
    assert [c[0] for c in chunks] == [b"00dc"] * len(frames)
    for c in chunks:
        assert c[1] % 2 == 0                                         # every chunk starts on an even offset: the padding is there
    assert idx1[2] == 16 * len(frames)
    movi_fourcc = movi[1]                                            # the offset of 'movi' itself: what AVI 1.0 index entries count from
    for k, want in enumerate(frames):
        cc, flags, off, size = struct.unpack("<4sIII", data[idx1[1] + 16 * k:idx1[1] + 16 * k + 16])
        assert cc == b"00dc" and flags & 0x10
        at = movi_fourcc + off
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == size == len(want)
        assert data[at + 8:at + 8 + size] == want
        im = Image.open(io.BytesIO(data[at + 8:at + 8 + size]))
        assert im.size == (width, height)
        im.load()
    return len(data)


def test_mjpeg_writer_structure(tmp_path):
    frames = [_frame(33, 17, s) for s in range(5)]
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)          # padded and unpadded chunks
    path = str(tmp_path / "a.avi")
    with JP.MjpegWriter(path, 33, 17, 29.97) as w:
        for f in frames:
            w.add(f)
        with pytest.raises(ValueError):
            w.add(_frame(17, 33, 0))                                 # another size
    assert w.paths == [path] and w.frames == 5
    check_avi(path, frames, 33, 17, 2997, 100)
    w.close()                                                        # a second close changes nothing
    check_avi(path, frames, 33, 17, 2997, 100)
    with pytest.raises(ValueError):
        w.add(frames[0])
    empty = str(tmp_path / "empty.avi")
    JP.MjpegWriter(empty, 8, 8, 30).close()
    check_avi(empty, [], 8, 8, 30, 1)


def test_mjpeg_writer_rolls_over(tmp_path):
    frames = [_frame(40, 24, s) for s in range(9)]
    limit = 4 * max(len(f) for f in frames)
    path = str(tmp_path / "b.avi")
    w = JP.MjpegWriter(path, 40, 24, 25, limit=limit)
    for f in frames:
        w.add(f)
    w.close()
    assert len(w.paths) >= 3 and w.paths[0] == path
    assert w.paths[1:] == [str(tmp_path / f"b_part{k}.avi") for k in range(2, len(w.paths) + 1)]
    at = 0
    for p in w.paths:
        n = struct.unpack("<I", open(p, "rb").read()[48:52])[0]       # avih.dwTotalFrames
        assert n >= 1
        assert check_avi(p, frames[at:at + n], 40, 24, 25, 1) <= limit
        at += n
    assert at == len(frames)


def test_overlay_sink_names():
    s = JP.OverlaySink.__new__(JP.OverlaySink)
    s.fmt = "jpg"
    assert s.picture_path("/x/image/Pred_3.png") == "/x/image/Pred_3.jpg"
    s.fmt = "png"
    assert s.picture_path("/x/image/Pred_3.png") == "/x/image/Pred_3.png"


def test_flags_default_to_todays_behaviour():
    from dynaboa_amd import benchmark as DB, internet as IN, online as ON
    for parser in (DB.parser, IN.parser, ON.parser):
        o = parser.parse_args([])
        assert (o.overlay_format, o.jpeg_quality, o.jpeg_subsampling, o.overlay_video, o.video_fps) == ("png", 90, "444", 0, 30.0)
        assert not JP.wants_sink(o) and JP.sink_for(o, "cpu") is None
        o = parser.parse_args(["--overlay_format", "jpg", "--jpeg_quality", "75", "--jpeg_subsampling", "420", "--overlay_video", "1",
                               "--video_fps", "25"])
        assert (o.overlay_format, o.jpeg_quality, o.jpeg_subsampling, o.overlay_video, o.video_fps) == ("jpg", 75, "420", 1, 25.0)
        assert JP.wants_sink(o)
        with pytest.raises(SystemExit):
            parser.parse_args(["--overlay_format", "gif"])
    assert JP.wants_sink(DB.parser.parse_args(["--overlay_video", "1"]))      # the video alone implies the encoder
