"""Videos for the GOP cut (pcamv_gpu_annexb_gops, k_video_cut) and jobs for the chunked copy (k_stream_copy): what
tests/test_video_host.py holds the host function to, what tests/test_video_cpu.py runs through the control code under the sanitizers,
and what tests/test_gpu_video.py hands to the device afterwards.  What can go wrong depends on byte positions, on counts of 64 units
and on chunk boundaries, not on picture size, so the units here are a few bytes long.

rule(video) is the definition of include/pcamv_gpu.h restated naively: every 00 00 01, the unit behind it up to the next one or the end
without its trailing zeros, and for every unit of type 5 a look back for the nearest unit of type 1 .. 5."""
import struct

import numpy as np

CHUNK = 2048                    # PCAMV_STREAM_CHUNK
SC3, SC4 = b"\x00\x00\x01", b"\x00\x00\x00\x01"
IDR, P, P_NOREF, SPS, PPS, AUD, SEI = 0x65, 0x41, 0x61, 0x67, 0x68, 0x09, 0x06
ALPHABET = (0x00, 0x01, 0x03, IDR, P, P_NOREF, SPS, PPS, AUD, SEI, 0x9A, 0xE7)      # 00, 01, 03, the seven header bytes, two payload bytes
COPY_LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 4099)


def unit(header, payload=b"\x9a\xe7", sc=SC4):
    return sc + bytes([header]) + payload


def rule(video):
    """(GOPs as (off, len, first_unit, n_units), preamble) by the definition, naively"""
    v = bytes(video)
    pre = [i for i in range(len(v) - 2) if v[i] == 0 and v[i + 1] == 0 and v[i + 2] == 1]
    units = []
    for k, i in enumerate(pre):
        b, e = i + 3, pre[k + 1] if k + 1 < len(pre) else len(v)
        while e > b and v[e - 1] == 0:
            e -= 1
        units.append((b, e - b, v[b] & 31 if e > b else None))
    vcl = lambda t: t is not None and 1 <= t <= 5      # noqa: E731
    starts = []
    for u, (_, _, t) in enumerate(units):
        if t != 5:
            continue
        before = [j for j in range(u) if vcl(units[j][2])]
        if before and units[before[-1]][2] == 5:
            continue
        f = before[-1] + 1 if before else 0
        starts.append((units[f - 1][0] + units[f - 1][1] if f else 0, f))
    ends = starts[1:] + [(len(v), len(units))]
    gops = [(a, ea - a, f, ef - f) for (a, f), (ea, ef) in zip(starts, ends)]
    return gops, starts[0][0] if starts else len(v)


def _opener_at(index):
    """P units, then an IDR unit as unit number `index`, then two P units"""
    return b"".join(unit(P, bytes([0x80 | (k & 0x7F)])) for k in range(index)) + unit(IDR) + unit(P) + unit(P)


def _straddle(k):
    """a GOP whose IDR unit's long start code has its byte k, or the byte k behind its first, at the first byte of the second chunk"""
    front = unit(IDR) + unit(P, b"\xaa" * 40)
    fill = CHUNK - k - len(front) - 4
    return front + unit(P, b"\x9b" * fill)[:4 + fill] + unit(IDR, b"\x11\x22") + unit(P)


def listed_videos():
    """the named cases, as (name, bytes)"""
    head = unit(AUD, b"\x10") + unit(SPS, b"\x42\x00\x1e") + unit(PPS, b"\xce\x38\x80") + unit(SEI, b"\x05\x01\x80")
    gop = lambda n, first=unit(IDR): first + b"".join(unit(P, bytes([0x88 + k])) for k in range(n))      # noqa: E731
    out = [(f"opener at unit {i}", _opener_at(i)) for i in (0, 63, 64, 65, 127, 128)]
    # (k = 0 .. 3 with the video at a multiple of 4; the chunks are cut at addresses, so a video 1 .. 3 bytes off has them at k + 1 .. k + 3)
    out += [(f"start code byte {k} on a chunk boundary", _straddle(k)) for k in range(7)]
    out += [("short start codes", unit(IDR, sc=SC3) + unit(P, sc=SC3) + unit(IDR, sc=SC3) + unit(P, sc=SC3)),
            ("long and short start codes mixed", unit(IDR) + unit(P, sc=SC3) + unit(SPS, sc=SC3) + unit(IDR) + unit(P, sc=SC3)),
            ("runs of zeros between units", unit(IDR) + b"\x00" * 7 + unit(P) + b"\x00" * 300 + unit(IDR, sc=SC3) + b"\x00" * 5 + unit(P) + b"\x00" * 3),
            ("delimiter, sets and SEI in front of every IDR unit", head + gop(3) + head + gop(2) + head + gop(1)),
            ("nothing in front of the IDR units", gop(2) + gop(2) + gop(0) + gop(1)),
            ("sets in front of the first IDR unit alone", head + gop(2) + gop(3) + unit(AUD, b"\x10") + gop(1)),
            ("two IDR units in a row", unit(IDR) + unit(IDR, b"\x33") + unit(P) + unit(IDR) + unit(IDR) + unit(P)),
            ("three IDR units in a row", unit(IDR) + unit(IDR) + unit(IDR) + unit(P) + unit(P) + unit(IDR) + unit(IDR) + unit(IDR)),
            ("IDR units with sets between them", unit(IDR) + unit(SPS) + unit(IDR) + unit(P) + unit(IDR)),
            ("P units before the first IDR unit", unit(P) + unit(P_NOREF) + head + gop(2) + gop(1)),
            ("bytes before the first start code", b"\x17\x00\x42" + gop(1) + gop(1)),
            ("no IDR unit at all", unit(SPS) + unit(P) + unit(P) + unit(SEI)),
            ("no unit at all", b"\x65\x41\x00\x00\x02\x65"),
            ("empty video", b""),
            ("a video of zeros", b"\x00" * 700),
            ("ends inside a start code", gop(1) + gop(1) + b"\x00\x00"),
            ("ends behind a start code", gop(1) + SC4),
            ("ends in an IDR header byte", gop(1) + SC3 + bytes([IDR])),
            ("empty units", SC3 + SC3 + unit(IDR) + SC4 + SC3 + unit(P) + SC3 + unit(IDR)),
            ("data partitions between P and IDR", unit(IDR) + unit(P) + unit(0x42) + unit(0x43) + unit(0x44) + unit(IDR) + unit(0x62) + unit(IDR) + unit(P)),
            ("type 5 under other nal_ref_idc", unit(0x25) + unit(P) + unit(0x45) + unit(0x05) + unit(P) + unit(0x65)),
            ("types above 5 are not slices", unit(IDR) + unit(0x0C) + unit(0x14) + unit(IDR) + unit(P) + unit(0x1F) + unit(IDR)),
            ("seventy GOPs", b"".join(gop(1 + k % 3) for k in range(70))),
            ("two hundred GOPs of one unit", unit(IDR) + b"".join(unit(P) + unit(IDR) for _ in range(199)))]
    return out


CAP_CASES = (0, 1, 2, 69)       # gops[cap] below and at the count of "seventy GOPs" less one


def random_videos(count=400, seed=77):
    """strings over ALPHABET, zeros and ones favoured so that start codes are frequent, from 0 to some 600 bytes"""
    rng = np.random.default_rng(seed)
    w = np.array([8, 5, 1, 3, 3, 1, 1, 1, 1, 1, 2, 2], float)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 40)) if k % 4 == 0 else int(rng.integers(40, 600))
        out.append(bytes(rng.choice(ALPHABET, size=n, p=w / w.sum()).astype(np.uint8)))
    return out


def big_video():
    """a video of more than 64 chunks -- several blocks of the two-level prefix over a long stream's chunks and a last block that is not
    full: 700 GOPs of an IDR unit and one to three P units of 150 .. 250 bytes, sets in front of every tenth, some 430 KB"""
    rng = np.random.default_rng(12)
    head = unit(SPS, b"\x42\x00\x1e") + unit(PPS, b"\xce\x38\x80")
    out = []
    for g in range(700):
        body = b"".join(unit(P, b"\x9a" + bytes(rng.integers(1, 256, int(rng.integers(150, 250))).astype(np.uint8)), sc=(SC3, SC4)[(g + k) & 1]) for k in range(1 + g % 3))
        out.append((head if g % 10 == 0 else b"") + unit(IDR, bytes(rng.integers(1, 256, 200).astype(np.uint8))) + body)
    return b"".join(out)


def all_videos():
    return [v for _, v in listed_videos()] + random_videos()


def single_idr_streams():
    """streams that begin with a start code, hold exactly one IDR picture (of one or two slices), at least one P unit behind it, and end
    in a non-zero byte: joined, they are the GOPs.  (Without the P unit the property does not hold: by the rule an IDR picture directly
    behind another stays in its GOP, so a stream of an IDR picture alone takes up a following stream that begins with its IDR unit.)"""
    head = unit(SPS, b"\x42\x00\x1e") + unit(PPS, b"\xce\x38\x80")
    rng = np.random.default_rng(5)
    out = []
    for k in range(40):
        body = b"".join(unit(P, bytes(rng.integers(1, 256, int(rng.integers(1, 50))).astype(np.uint8)), sc=(SC3, SC4)[int(rng.integers(0, 2))])
                        for _ in range(int(rng.integers(1, 5))))
        idr = unit(IDR, bytes(rng.integers(1, 256, int(rng.integers(1, 90))).astype(np.uint8)))
        out.append((head if k % 3 else b"") + (unit(AUD, b"\x10") if k % 2 else b"") + idr + (unit(IDR, b"\x44") if k % 5 == 0 else b"") + body)
    return out


def copy_jobs():
    """(source alignment, destination alignment, length) for all 16 pairs mod 4 and every listed length, and a few pairs mod 16"""
    jobs = [(sa, da, n) for sa in range(4) for da in range(4) for n in COPY_LENGTHS]
    jobs += [(sa, da, n) for sa, da in ((0, 0), (16, 0), (0, 12), (5, 13), (15, 15), (8, 4)) for n in (17, 1023, 1025, 4099)]
    return jobs


def write_cases(path):
    """the case file of tests/fuzz/check_video.cpp: int32 n_videos, per video int32 cap (-1: all GOPs), int32 len, bytes; int32 n_jobs, per
    job int32 source alignment, destination alignment, length.  Returns (videos, jobs) written"""
    videos = [(-1, v) for v in all_videos()]
    seventy = dict(listed_videos())["seventy GOPs"]
    videos += [(cap, seventy) for cap in CAP_CASES] + [(-1, big_video())]
    jobs = copy_jobs()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(videos)))
        for cap, v in videos:
            f.write(struct.pack("<ii", cap, len(v)) + v)
        f.write(struct.pack("<i", len(jobs)))
        for j in jobs:
            f.write(struct.pack("<iii", *j))
    return len(videos), len(jobs)
