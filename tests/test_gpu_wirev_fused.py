"""GPU: a write held in a list of device buffers as one wire stream in device
memory, made in one pass (include/hadoofus_wirev_fused.h) --
frame_fused_gather_kernel copies the fragments' bytes, computes the chunk CRCs
from the registers it copies and writes every byte of the stream; a 4 KiB
round, a 512-B chunk or a 16-B lane piece whose bytes lie in more than one
fragment is assembled piece by piece.

The expected stream everywhere is built on the host from the CPU oracle:
oracle.compose_packets(concatenation, ...) gives the header buffers and the
records; packet after packet, hdr[hdr_off : hdr_off + hdr_len] is followed by
data[data_off : data_off + data_len].  Fragments and destination are carved
from one device allocation between 0xA5 guards, at chosen byte residues mod
16; after every call the whole allocation is downloaded and compared with the
image expected, so the fragments and the guards are untouched and `wire`
equals the expected stream.  Where a test claims a path of the kernel, it
first asks hdfs_wirev_fused_layout whether its shape takes it.  Everything is
bit-exact."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from packet_stream import payload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = 512
EINVAL = -1
GUARD = 0xA5
GAP = 96  # guard bytes before, between and after the ranges (at least)


@pytest.fixture(scope="module")
def wvf(engine):
    from hadoofus_amd import wirev_fused
    wirev_fused.load()
    return wirev_fused


def expect(oracle, data, off=0, seq=0, proto=2, ctype=2, finish=False):
    """-> (stream bytes (numpy), records with hdr_off counting in the stream)."""
    hdr, pkts = oracle.compose_packets(data, off, seq, proto, ctype, finish)
    hdr = np.frombuffer(hdr, dtype=np.uint8)
    parts, recs, at = [], [], 0
    for p in pkts:
        parts.append(hdr[p["hdr_off"]:p["hdr_off"] + p["hdr_len"]])
        parts.append(data[p["data_off"]:p["data_off"] + p["data_len"]])
        recs.append(dict(p, hdr_off=at))
        at += p["hdr_len"] + p["data_len"]
    stream = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    assert len(stream) == at == len(hdr) + len(data)
    return stream, recs


def cut(data, lens):
    assert sum(lens) == len(data)
    ends = np.cumsum(lens)
    return [data[e - n:e] for n, e in zip(lens, ends)]


def room(lens, wire_len):
    """Bytes of an arena for fragments of these lengths and a stream."""
    return sum(lens) + (GAP + 32) * (len(lens) + 2) + wire_len


class Arena:
    """One device allocation: guards, then every non-empty fragment at its
    residue mod 16 with guards between, then the destination at residue
    dst_mis mod 16, guards."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.buf = engine.DeviceBuffer(nbytes)
        assert self.buf.ptr % 16 == 0

    def place(self, pieces, wire_len, mis=(0,), dst_mis=0, order=None):
        """pieces: the fragments' bytes.  Fragment i lies at residue
        mis[i % len(mis)]; order: the fragments from the lowest address up
        (default: as given).  -> ([(ptr or None, nbytes)], wire ptr)."""
        at = 0
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        self.where = [None] * len(pieces)
        for i in (order if order is not None else range(len(pieces))):
            if not len(pieces[i]):
                continue
            at = (at + GAP + 15) // 16 * 16 + mis[i % len(mis)]
            self.where[i] = at
            self.image[at:at + len(pieces[i])] = pieces[i]
            at += len(pieces[i])
        self.dst = (at + GAP + 15) // 16 * 16 + dst_mis
        assert self.dst + wire_len + GAP <= self.buf.nbytes
        self.buf.upload(self.image)
        iov = [(self.buf.ptr + w, len(p)) if w is not None else (None, 0) for w, p in zip(self.where, pieces)]
        return iov, self.buf.ptr + self.dst

    def check(self, stream):
        """The whole allocation: the stream where it belongs, nothing else changed."""
        want = self.image.copy()
        want[self.dst:self.dst + len(stream)] = stream
        got = self.buf.download()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (fragments {self.where[:8]}, dst "
                                 f"{self.dst}, stream {len(stream)}): got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def run(wvf, arena, pieces, want, mis=(0,), dst_mis=0, off=0, seq=0, proto=2, ctype=2, finish=False, order=None):
    stream, recs = want
    iov, dp = arena.place(pieces, len(stream), mis, dst_mis, order)
    got_len, got = wvf.compose_wirev_fused(iov, dp, len(stream), off, seq, proto, ctype, finish)
    assert got_len == len(stream) and got == recs
    arena.check(stream)
    return dp


# ---- the write of tests/test_gpu_wirev.py: 287, 64 KiB, 64 KiB, 413, 0 ------------------------
N2 = 2 * 65536 + 700
_two = {}


def two(oracle):
    if not _two:
        _two["d"] = payload(91, 0, N2)
        _two["want"] = expect(oracle, _two["d"], 4321, 3, 2, 2, True)
        assert [p["data_len"] for p in _two["want"][1]] == [287, 65536, 65536, 700 - 287, 0]
    return _two["d"], _two["want"]


# ---- 1 ------------------------------------------------------------------------------------------
def test_one_fragment_is_the_fused_single_write_call(engine, wvf, oracle):
    """No seam anywhere; the stream is hdfs_wire_fused_compose_packets' and
    hdfs_wirev_compose_packets', both downloaded (and the oracle's)."""
    from hadoofus_amd import wire_fused, wirev
    d, want = two(oracle)
    info = wvf.layout([N2], 4321, 2, 2, True)
    assert (info["rounds"], info["seamed_rounds"], info["seamed_ragged"], info["max_frags_per_round"]) == (32, 0, 0, 1)
    a = Arena(engine, room([N2], len(want[0])))
    wl = len(want[0])
    for mis, dst_mis in ((0, 0), (3, 6), (1, 15)):
        dp = run(wvf, a, [d], want, (mis,), dst_mis, 4321, 3, 2, 2, True)
        ours = a.buf.download(wl, a.dst)
        a.buf.upload(np.full(wl, GUARD, np.uint8), a.dst)
        assert wire_fused.compose_wire(a.buf.ptr + a.where[0], N2, dp, wl, 4321, 3, 2, 2, True) == (wl, want[1])
        assert np.array_equal(a.buf.download(wl, a.dst), ours)
        a.buf.upload(np.full(wl, GUARD, np.uint8), a.dst)
        assert wirev.compose_wire([(a.buf.ptr + a.where[0], N2)], dp, wl, 4321, 3, 2, 2, True) == (wl, want[1])
        assert np.array_equal(a.buf.download(wl, a.dst), ours)


# ---- 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 4321])
def test_every_split_of_a_small_write(engine, wvf, oracle, off):
    """1 100 bytes in two fragments, split at every byte: chunks of 512, 512
    and 76 bytes at offset 0, of 287, 512 and 301 at 4321.  The seam crosses
    every byte of a lane piece, of a full chunk and of both ragged chunks."""
    n = 1100
    d = payload(92, 0, n)
    want = expect(oracle, d, off, 5, 2, 2, True)
    head = (512 - off % 512) % 512
    nfull = (n - head) // 512 * 512
    a = Arena(engine, room([n, 0], len(want[0])))
    seen = set()
    for s in range(n + 1):
        info = wvf.layout([s, n - s], off, 2, 2, True)
        in_round = head < s < head + nfull
        in_ragged = 0 < s < head or head + nfull < s < n
        assert (info["seamed_rounds"], info["seamed_ragged"]) == (int(in_round), int(in_ragged)), s
        seen.add((in_round, in_ragged))
        run(wvf, a, cut(d, [s, n - s]), want, (1 + s % 3, (5 * s) % 16), (7 * s) % 16, off, 5, 2, 2, True)
    assert seen == {(False, False), (True, False), (False, True)}


# ---- 3 ------------------------------------------------------------------------------------------
def test_splits_at_the_corners_of_a_large_write(engine, wvf, oracle):
    """Around the short first packet's end, a chunk's, a round's, a packet's,
    a packet's last round's and the write's last chunk."""
    d, want = two(oracle)
    a = Arena(engine, room([N2, 0], len(want[0])))
    last_chunk = 287 + 2 * 65536  # the 413 bytes behind the full packets
    corners = [287, 287 + 512, 287 + 4096, 287 + 65536, 287 + 65536 + 4096 * 15, last_chunk]
    k = 0
    for c in corners:
        for delta in (0, 1, 15, 16, 17):
            for s in {c - delta, c + delta}:
                if 0 <= s <= N2:
                    run(wvf, a, cut(d, [s, N2 - s]), want, (1 + k % 3, (5 * k) % 16), (7 * k) % 16, 4321, 3, 2, 2, True)
                    k += 1
    assert wvf.layout([287 + 4096 + 1, N2 - 287 - 4097], 4321, 2, 2, True)["seamed_rounds"] == 1
    assert wvf.layout([last_chunk + 1, N2 - last_chunk - 1], 4321, 2, 2, True)["seamed_ragged"] == 1


# ---- 4 ------------------------------------------------------------------------------------------
def test_two_seams_in_one_lane_piece_and_one_byte_pieces_at_round_ends(engine, wvf, oracle):
    """Three fragments, the middle one of 1 to 33 bytes, laid across a
    lane-piece boundary (1040), a chunk boundary (1536), a round boundary
    (4096) and a packet boundary (65536): ending at it, ending one byte past
    it, straddling it, starting at it and lying three bytes behind it (both
    seams inside one 16-B lane piece when it is short).  With one byte it is
    a round's last byte and a round's first byte."""
    n = 65536 + 4096 + 600
    d = payload(93, 0, n)
    want = expect(oracle, d, 0, 1, 2, 2, False)
    assert [p["data_len"] for p in want[1]] == [65536, 4096 + 600]
    a = Arena(engine, room([n, 0, 0], len(want[0])))
    info = wvf.layout([4095, 1, n - 4096], 0, 2, 2, False)
    assert info["seamed_rounds"] == 1 and info["max_frags_per_round"] == 2
    info = wvf.layout([1043, 5, n - 1048], 0, 2, 2, False)
    assert info["seamed_rounds"] == 1 and info["max_frags_per_round"] == 3
    k = 0
    for b in (1040, 1536, 4096, 65536):
        for mid in range(1, 34):
            for start in sorted({b - mid, b - mid + 1, b - mid // 2, b, b + 3}):
                lens = [start, mid, n - start - mid]
                run(wvf, a, cut(d, lens), want, (5, k % 16, 10), (3 * k) % 16, 0, 1, 2, 2, False)
                k += 1


# ---- 5 ------------------------------------------------------------------------------------------
def test_one_byte_fragments(engine, wvf, oracle):
    """1 300 fragments of one byte: every chunk is seamed, a round has 512
    fragments under it and the lookup's upper-bound probe answers."""
    n = 1300
    d = payload(94, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    info = wvf.layout([1] * n, 4321, 2, 2, True)
    assert (info["nfrags"], info["rounds"], info["seamed_rounds"], info["seamed_ragged"],
            info["max_frags_per_round"]) == (n, 1, 1, 2, 512)
    a = Arena(engine, room([1] * n, len(want[0])))
    run(wvf, a, cut(d, [1] * n), want, (0, 3, 2, 1, 7), 9, 4321, 0, 2, 2, True)
    want = expect(oracle, d, 0, 0, 2, 2, False)
    run(wvf, a, cut(d, [1] * n), want, (15, 4, 9), 2, 0, 0, 2, 2, False)


# ---- 6 ------------------------------------------------------------------------------------------
def test_zero_length_fragments(engine, wvf, oracle):
    """NULL bases of no bytes first, in the middle, in runs and last; and nothing else."""
    n = 70000
    d = payload(95, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    lens = [0, 0, 30000, 0, 0, 0, 40000 - 77, 0, 77, 0]
    a = Arena(engine, room(lens, len(want[0])))
    iov, _ = a.place(cut(d, lens), len(want[0]), (3, 1), 5)
    assert [p for p, _ in iov] == [None, None, iov[2][0], None, None, None, iov[6][0], None, iov[8][0], None]
    assert wvf.layout(lens, 4321, 2, 2, True)["nfrags"] == 3
    run(wvf, a, cut(d, lens), want, (3, 1), 5, 4321, 0, 2, 2, True)
    empty = np.zeros(0, np.uint8)
    fin = expect(oracle, empty, 1024, 4, 2, 2, True)
    assert len(fin[1]) == 1 and len(fin[0]) == 31
    run(wvf, a, [empty, empty, empty], fin, (0,), 9, 1024, 4, 2, 2, True)
    iov, dp = a.place([empty, empty], 0, (0,), 3)
    assert wvf.compose_wirev_fused(iov, dp, 64, 1024, 4, 2, 2, False) == (0, [])
    assert wvf.compose_wirev_fused([], dp, 64, 1024, 4, 2, 2, False) == (0, [])
    a.check(empty)


# ---- 7 ------------------------------------------------------------------------------------------
def test_every_source_residue(engine, wvf, oracle):
    """Seven fragments whose bases take every residue mod 16 over 16 runs (fast
    rounds, seamed rounds and both ragged chunks read from every residue), and
    one placement against every residue of the stream."""
    lens = [100, 633, 4096 + 5, 1, 5000, 3411, 100]
    n = sum(lens)
    d = payload(96, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    info = wvf.layout(lens, 4321, 2, 2, True)
    assert (info["rounds"], info["seamed_rounds"], info["seamed_ragged"]) == (4, 3, 2)
    a = Arena(engine, room(lens, len(want[0])))
    for r in range(16):
        run(wvf, a, cut(d, lens), want, tuple((r + 5 * i) % 16 for i in range(7)), (3 * r) % 16, 4321, 0, 2, 2, True)
    for dst_mis in range(16):
        run(wvf, a, cut(d, lens), want, (3, 8, 13, 2, 7, 12, 1), dst_mis, 4321, 0, 2, 2, True)


# ---- 8 ------------------------------------------------------------------------------------------
def test_repeated_overlapping_and_descending_fragments(engine, wvf, oracle):
    """The same buffer given twice, two fragments that share bytes, and
    fragments in descending and in shuffled address order."""
    x, y = payload(97, 0, 70001), payload(98, 0, 333)
    a = Arena(engine, room([70001, 333], 2 * 70001 + 333 + 4000))
    for frags in ([(0, 0, 70001), (1, 0, 333), (0, 0, 70001)],           # x, y, x
                  [(0, 0, 50000), (0, 20000, 50001), (1, 0, 333)]):      # x[:50000], x[20000:], y
        d = np.concatenate([(x, y)[w][s:s + n] for w, s, n in frags])
        want = expect(oracle, d, 4321, 0, 2, 2, True)
        iov, dp = a.place([x, y], len(want[0]), (5, 2), 13)
        iov = [(iov[w][0] + s, n) for w, s, n in frags]
        assert wvf.compose_wirev_fused(iov, dp, len(want[0]), 4321, 0, 2, 2, True) == (len(want[0]), want[1])
        a.check(want[0])
    n = 2 * 65536 + 100
    d = payload(99, 0, n)
    want = expect(oracle, d, 0, 0, 2, 2, True)
    lens = [50000, 70001, 9, 3, n - 120013]
    b = Arena(engine, room(lens, len(want[0])))
    run(wvf, b, cut(d, lens), want, (7, 0, 2), 11, 0, 0, 2, 2, True, order=[4, 3, 2, 1, 0])
    run(wvf, b, cut(d, lens), want, (7, 0, 2), 11, 0, 0, 2, 2, True, order=[2, 0, 4, 1, 3])


# ---- 9 ------------------------------------------------------------------------------------------
EIGHTEEN = 17 * 65536 + 45
_eighteen = {}


@pytest.mark.parametrize("ctype", [2, 1, 0], ids=["crc32c", "crc32", "null"])
@pytest.mark.parametrize("proto", [2, 1])
def test_protocols_and_checksum_types(engine, wvf, oracle, proto, ctype):
    """18 packets in five odd fragments; the packets start at all 16 residues."""
    if "d" not in _eighteen:
        _eighteen["d"] = payload(100, 0, EIGHTEEN)
    d = _eighteen["d"]
    lens = [300, 5 * 65536 + 7, 5001, 3]
    lens.append(EIGHTEEN - sum(lens))
    want = expect(oracle, d, 0, 100, proto, ctype, False)
    assert len(want[1]) == 18 and {p["hdr_off"] % 16 for p in want[1]} == set(range(16))
    assert wvf.layout(lens, 0, proto, ctype, False)["seamed_rounds"] == 3
    run(wvf, Arena(engine, room(lens, len(want[0]))), cut(d, lens), want, (1, 6, 3, 11, 14), 0, 0, 100, proto, ctype,
        False)


# ---- 10 -----------------------------------------------------------------------------------------
NINE = (9 << 20) + 321
MANY = 2305 * 4097  # 2 305 fragments of 4 097 bytes: 9 MiB + 6 401 bytes
_nine = {}


@pytest.mark.parametrize("shape", ["five", "many"])
def test_few_workgroups_walk_many_packets(engine, wvf, oracle, shape):
    """About 9 MiB (145 packets) on the product's grid and on 1, 3 and 7
    workgroups: a workgroup walks many packets and a wave's hint moves across
    many fragments.  In five odd fragments (9 MiB + 321 bytes) nearly every
    round is fast; in 2 305 fragments of 4 097 bytes (2 305 x 4 097 bytes, the
    nearest such write) nearly every round is seamed."""
    if "d" not in _nine:
        _nine["d"] = payload(101, 0, MANY)
    if shape == "five":
        n = NINE
        lens = [(3 << 20) + 11, (1 << 20) + 7, 2000001, 5]
        lens.append(n - sum(lens))
    else:
        n = MANY
        lens = [4097] * 2305
    d = _nine["d"][:n]
    info = wvf.layout(lens, 4321, 2, 2, True)
    if shape == "five":
        assert info["seamed_rounds"] == 3 and info["rounds"] > 2300 and info["seamed_ragged"] == 0
    else:
        assert info["seamed_rounds"] > 2200 and info["rounds"] - info["seamed_rounds"] > 0
        assert info["max_frags_per_round"] == 2
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    assert len(want[1]) > 140
    a = Arena(engine, room(lens, len(want[0])))
    pieces = cut(d, lens)
    mis = (3, 1, 7, 5, 9)
    run(wvf, a, pieces, want, mis, 6, 4321, 0, 2, 2, True)
    for g in (1, 3, 7):
        iov, dp = a.place(pieces, len(want[0]), mis, 6)
        assert wvf.fused_time(iov, dp, len(want[0]), 4321, 2, 2, True, wvf.time_groups(g), 1) > 0
        a.check(want[0])


# ---- 11 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("finish", [False, True])
def test_short_writes(engine, wvf, oracle, finish):
    """0, 1, 511, 512 and 513 bytes, whole and split, at an aligned and an
    unaligned block offset: packets of nothing but a ragged chunk, one full
    chunk and a byte, and rounds without a full chunk next to the write's end."""
    a = Arena(engine, 8192)
    for n in (0, 1, 511, 512, 513):
        d = payload(102 + n, 0, n)
        splits = [[n]] if n < 2 else [[n], [1, n - 1], [n // 2, 0, n - n // 2], [n - 1, 1]]
        for off in (0, 4321):
            want = expect(oracle, d, off, 9, 2, 2, finish)
            for k, lens in enumerate(splits):
                run(wvf, a, cut(d, lens), want, (k, 5 + k, 11), 3 * k + n % 5, off, 9, 2, 2, finish)


# ---- 12 -----------------------------------------------------------------------------------------
def test_round_trip_through_the_read_side(engine, wvf, oracle):
    lens = [65536 + 1234, 999, 4 * 65536 - 999]
    n = sum(lens)
    d = payload(110, 0, n)
    want = expect(oracle, d, 0, 0, 2, 2, True)
    a = Arena(engine, room(lens, len(want[0])))
    dp = run(wvf, a, cut(d, lens), want, (5, 2, 3), 11, 0, 0, 2, 2, True)
    wl = len(want[0])
    ref = oracle.verify_packets(want[0].tobytes())
    got = engine.verify_packets(None, dptr=dp, nbytes=wl)
    assert got == ref and got[0] == 0 and got[2] == wl and len(got[1]) == len(want[1])
    for v, p in zip(got[1], want[1]):
        assert (v["stream_off"], v["offset_in_block"], v["seqno"], v["data_len"], v["crc_len"], v["last"]) == \
            (p["hdr_off"], p["offset_in_block"], p["seqno"], p["data_len"], p["crc_len"], p["last"])
    # the seam at byte 65536 + 1234 of the write: byte 1233 of packet 1, in its chunk 2; the byte ahead of it flipped
    p1 = want[1][1]
    assert p1["data_off"] == 65536
    at = a.dst + p1["hdr_off"] + p1["hdr_len"] + 1233
    a.buf.upload(np.array([want[0][at - a.dst] ^ 0x20], dtype=np.uint8), at)
    rc, got, _ = engine.verify_packets(None, dptr=dp, nbytes=wl)
    assert rc == engine.ERR_BAD_CHECKSUM
    assert [(i, p["first_bad"], p["bad_chunks"]) for i, p in enumerate(got) if p["error"]] == [(1, 2, 1)]


# ---- 13 -----------------------------------------------------------------------------------------
def test_rejections_write_nothing(engine, wvf, oracle):
    from hadoofus_amd.abi import IoVec, OutPacket
    lens = [40000, 0, 60000]
    n = sum(lens)
    d = payload(111, 0, n)
    stream, recs = expect(oracle, d, 0, 0, 2, 2, True)
    wl, npk = len(stream), len(recs)
    a = Arena(engine, room(lens, wl))
    iov, dp = a.place(cut(d, lens), wl, (1, 0, 6), 3)
    (f0, _), _, (f2, _) = iov
    lib = wvf.load()
    arr = (OutPacket * npk)()
    before = bytes(arr)
    cnt, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    host = np.zeros(wl + 64, dtype=np.uint8)
    end = a.buf.ptr + a.buf.nbytes

    def call(p0=f0, p2=f2, wire=dp, cap=wl, maxp=npk):
        vec = (IoVec * 3)(IoVec(p0, 40000), IoVec(None, 0), IoVec(p2, 60000))
        return lib.hdfs_wirev_fused_compose_packets(vec, 3, 0, 0, 2, 2, 1, wire, cap, arr, maxp, ctypes.byref(cnt),
                                                    ctypes.byref(used), None)
    cases = {
        "wire_cap one short": (dict(cap=wl - 1), b""),
        "max_pkts one short": (dict(maxp=npk - 1), b""),
        "a null base with a length": (dict(p2=None), b"fragment 2"),
        "host fragments": (dict(p0=host.ctypes.data, p2=host.ctypes.data), b"fragment 0"),
        "mixed: a host fragment behind a device one": (dict(p2=host.ctypes.data), b"fragment 2"),
        "mixed: a host fragment ahead of a device one": (dict(p0=host.ctypes.data), b"fragment 0"),
        "a fragment past its allocation": (dict(p2=end - 60000 + 1), b"fragment 2"),
        "wire over fragment 2's end": (dict(wire=f2 + 60000 - 1), b"fragment 2"),
        "wire inside fragment 0": (dict(wire=f0 + 10), b"fragment 0"),
        "fragment 2 over the wire's start": (dict(p2=dp - 60000 + 1), b"fragment 2"),
        "wire past its allocation": (dict(wire=end - wl + 1), b"wire"),
        "host wire": (dict(wire=host.ctypes.data), b"wire"),
    }
    for name, (kw, text) in cases.items():
        assert call(**kw) == EINVAL, name
        err = lib.hdfs_wirev_fused_last_error()
        assert err and text in err, (name, err)
        assert (cnt.value, used.value) == (npk, wl), name
        assert bytes(arr) == before and not host.any(), name
    # workgroups out of range, or a flag bit that means nothing
    ms = ctypes.c_double(0)
    vec = (IoVec * 3)(IoVec(f0, 40000), IoVec(None, 0), IoVec(f2, 60000))
    for flags in (wvf.time_groups(wvf.MAX_GROUPS + 1), wvf.time_groups(1 << 23), 1, wvf.time_groups(2) | 4):
        assert lib.hdfs_wirev_fused_time(vec, 3, 0, 2, 2, 1, dp, wl, flags, 1, ctypes.byref(ms)) == EINVAL, flags
        assert b"workgroups" in lib.hdfs_wirev_fused_last_error()
    a.check(np.zeros(0, np.uint8))
    assert call() == 0  # and the same arguments, unspoilt, work
    a.check(stream)


# ---- 14 -----------------------------------------------------------------------------------------
def _filled_on(engine, wvf, oracle, seed, stream):
    """Fragments filled by a kernel on `stream` (None: the NULL stream) and the
    call right behind it, no synchronisation between the two."""
    lens = [2 << 20, 8, (3 << 20) + 64, 1 << 20]
    n = sum(lens)
    d = payload(seed, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, False)
    a = Arena(engine, room(lens, len(want[0])))
    iov, dp = a.place(cut(np.zeros(n, np.uint8), lens), len(want[0]), (8,), 13)
    at = 0
    for p, ln in iov:
        assert p % 8 == 0 and ln % 8 == 0
        engine.fill_splitmix64(p, ln // 8, seed, at // 8, stream)
        at += ln
    got_len, got = wvf.compose_wirev_fused(iov, dp, len(want[0]), 4321, 0, 2, 2, False, stream=stream)
    assert got_len == len(want[0]) and got == want[1]
    for w, piece in zip(a.where, cut(d, lens)):
        a.image[w:w + len(piece)] = piece
    a.check(want[0])


def test_fragments_filled_on_the_null_stream_just_before(engine, wvf, oracle):
    """The library's stream waits for the NULL stream."""
    _filled_on(engine, wvf, oracle, 112, None)


def test_on_a_stream_of_the_callers(engine, wvf, oracle):
    st = engine.stream_create()
    try:
        _filled_on(engine, wvf, oracle, 113, st)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, wvf, oracle):
    jobs = []
    for seed, lens, off, proto in [(114, [100000, 7, 300000 - 7], 0, 2), (115, [123, 250000], 4321, 1)]:
        n = sum(lens)
        d = payload(seed, 0, n)
        want = expect(oracle, d, off, 0, proto, 2, True)
        a = Arena(engine, room(lens, len(want[0])))
        iov, dp = a.place(cut(d, lens), len(want[0]), (seed % 4, 9), seed % 16)
        jobs.append((a, iov, dp, off, proto, want))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, iov, dp, off, proto, want = jobs[i]
            start.wait()
            for _ in range(4):
                assert wvf.compose_wirev_fused(iov, dp, len(want[0]), off, 0, proto, 2, True) == \
                    (len(want[0]), want[1])
        except BaseException as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for a, *_, want in jobs:
        a.check(want[0])


# ---- 15 -----------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "wirev_fused_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wirev_fused_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wirev_fused", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
