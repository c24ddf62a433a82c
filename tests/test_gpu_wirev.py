"""GPU: a write held in a list of device buffers as one wire stream in device
memory (include/hadoofus_wirev.h) -- the chunk CRCs as the gather-write
library computes them (one compute plan over the runs, gather_chunks_kernel
over the rest), then frame_gather_kernel, which writes every byte of the
stream from a table of the fragments.

The expected stream everywhere is built on the host from the CPU oracle:
oracle.compose_packets(concatenation, ...) gives the header buffers and the
records; packet after packet, hdr[hdr_off : hdr_off + hdr_len] is followed by
data[data_off : data_off + data_len].  Fragments and destination are carved
from one device allocation between 0xA5 guards, at chosen byte residues mod
16; after every call the whole allocation is downloaded and compared with the
image expected, so the fragments and the guards are untouched and `wire`
equals the expected stream.  Everything is bit-exact."""
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
def wv(engine):
    from hadoofus_amd import wirev
    wirev.load()
    return wirev


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


def run(wv, arena, pieces, want, mis=(0,), dst_mis=0, off=0, seq=0, proto=2, ctype=2, finish=False, order=None):
    stream, recs = want
    iov, dp = arena.place(pieces, len(stream), mis, dst_mis, order)
    got_len, got = wv.compose_wire(iov, dp, len(stream), off, seq, proto, ctype, finish)
    assert got_len == len(stream) and got == recs
    arena.check(stream)
    return dp


# ---- the write of tests/test_gpu_wire.py: 287, 64 KiB, 64 KiB, 413, 0 ------------------------
N2 = 2 * 65536 + 700
_two = {}


def two(oracle):
    if not _two:
        _two["d"] = payload(71, 0, N2)
        _two["want"] = expect(oracle, _two["d"], 4321, 3, 2, 2, True)
        assert [p["data_len"] for p in _two["want"][1]] == [287, 65536, 65536, 700 - 287, 0]
    return _two["d"], _two["want"]


def test_one_fragment_is_the_single_write_call(engine, wv, oracle):
    """Same stream and records as hdfs_wire_compose_packets (and the oracle's)."""
    from hadoofus_amd import wire
    d, want = two(oracle)
    a = Arena(engine, room([N2], len(want[0])))
    for mis, dst_mis in ((0, 0), (3, 6), (1, 15)):
        dp = run(wv, a, [d], want, (mis,), dst_mis, 4321, 3, 2, 2, True)
        ours = a.buf.download(len(want[0]), a.dst)
        a.buf.upload(np.full(len(want[0]), GUARD, np.uint8), a.dst)
        assert wire.compose_wire(a.buf.ptr + a.where[0], N2, dp, len(want[0]), 4321, 3, 2, 2, True) == \
            (len(want[0]), want[1])
        assert np.array_equal(a.buf.download(len(want[0]), a.dst), ours)


def test_two_fragments_split_at_every_corner(engine, wv, oracle):
    """n0 = 287: splits at the write's ends, around the short first packet,
    around a chunk boundary, around a packet boundary."""
    d, want = two(oracle)
    a = Arena(engine, room([N2, 0], len(want[0])))
    splits = [0, 1, 286, 287, 288, 287 + 511, 287 + 513, 287 + 65535, 287 + 65536, 287 + 65537, N2 - 1, N2]
    for k, s in enumerate(splits):
        run(wv, a, cut(d, [s, N2 - s]), want, (1 + k % 3, (5 * k) % 16), (7 * k) % 16, 4321, 3, 2, 2, True)


# ---- piece phases -------------------------------------------------------------------------------
def test_piece_phases(engine, wv, oracle):
    """Three fragments in one packet.  The middle one starts at each of 16
    consecutive stream positions (so at every residue of the destination's
    16-B grid) with source residues 0-3, and is 1 to 4 096 bytes long: pieces
    inside one 16-B block, pieces that end or start inside a block another
    piece shares, pieces with and without an interior."""
    n = 4096 + 16 + 300
    d = payload(72, 0, n)
    want = expect(oracle, d, 0, 1, 2, 2, False)
    assert len(want[1]) == 1
    a = Arena(engine, room([n, 0, 0], len(want[0])))
    for start in range(100, 116):
        for src in range(4):
            for mid in (1, 15, 16, 17, 31, 32, 33, 4096):
                lens = [start, mid, n - start - mid]
                run(wv, a, cut(d, lens), want, (5, src, 10), 2, 0, 1, 2, 2, False)


def test_one_byte_fragments(engine, wv, oracle):
    n = 700
    d = payload(73, 0, n)
    a = Arena(engine, room([1] * n, n + 200))
    for off, finish in ((0, True), (4321, False)):
        want = expect(oracle, d, off, 0, 2, 2, finish)
        run(wv, a, cut(d, [1] * n), want, (0, 3, 2, 1, 7), 9, off, 0, 2, 2, finish)


def test_zero_length_fragments(engine, wv, oracle):
    """NULL bases of no bytes first, in the middle and last; and nothing else."""
    n = 70000
    d = payload(74, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    lens = [0, 0, 30000, 0, 0, 0, 40000, 0]
    a = Arena(engine, room(lens, len(want[0])))
    iov, _ = a.place(cut(d, lens), len(want[0]), (3, 1), 5)
    assert [p for p, _ in iov] == [None, None, iov[2][0], None, None, None, iov[6][0], None]
    run(wv, a, cut(d, lens), want, (3, 1), 5, 4321, 0, 2, 2, True)
    empty = np.zeros(0, np.uint8)
    fin = expect(oracle, empty, 1024, 4, 2, 2, True)
    assert len(fin[1]) == 1 and len(fin[0]) == 31
    run(wv, a, [empty, empty, empty], fin, (0,), 9, 1024, 4, 2, 2, True)
    iov, dp = a.place([empty, empty], 0, (0,), 3)
    assert wv.compose_wire(iov, dp, 64, 1024, 4, 2, 2, False) == (0, [])
    assert wv.compose_wire([], dp, 64, 1024, 4, 2, 2, False) == (0, [])
    a.check(empty)


# ---- the search -------------------------------------------------------------------------------------
def test_many_fragments_and_a_long_tail(engine, wv, oracle):
    """300 fragments of 431 B and one of three packets: the table is longer
    than a workgroup, every entry is some packet's first or inner piece, and
    the last packets all find the last entry."""
    lens = [431] * 300 + [3 * 65536]
    n = sum(lens)
    d = payload(75, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    info = wv.layout(lens, 4321, 2, 2, True)
    assert info["nfrags"] == 301 and info["max_frags_per_packet"] > 150 and info["npkts"] == len(want[1]) == 7
    a = Arena(engine, room(lens, len(want[0])))
    run(wv, a, cut(d, lens), want, (0, 1, 2, 3, 5, 11), 7, 4321, 0, 2, 2, True)


# ---- layout corners -----------------------------------------------------------------------------------
def test_layout_corners(engine, wv, oracle):
    n = 4 * 65536 + 100
    d = payload(76, 0, n)
    want = expect(oracle, d, 0, 0, 2, 2, True)
    a = Arena(engine, room([n] + [0] * 4, len(want[0])))
    # fragment boundaries on packet boundaries
    run(wv, a, cut(d, [65536, 2 * 65536, 65536 + 100]), want, (3, 9, 14), 1, 0, 0, 2, 2, True)
    # one fragment spanning three packets between two short ones
    run(wv, a, cut(d, [1000, 3 * 65536 + 50, 65536 - 950]), want, (1, 2, 3), 4, 0, 0, 2, 2, True)
    # descending address order, and a shuffled one
    lens = [50000, 70001, 65536, 9, n - 185546]
    run(wv, a, cut(d, lens), want, (7, 0, 2), 11, 0, 0, 2, 2, True, order=[4, 3, 2, 1, 0])
    run(wv, a, cut(d, lens), want, (7, 0, 2), 11, 0, 0, 2, 2, True, order=[2, 0, 4, 1, 3])


def test_repeated_and_overlapping_fragments(engine, wv, oracle):
    """The same buffer given twice, and two fragments that share bytes."""
    x, y = payload(77, 0, 70001), payload(78, 0, 333)
    a = Arena(engine, room([70001, 333], 2 * 70001 + 333 + 4000))
    for frags in ([(0, 0, 70001), (1, 0, 333), (0, 0, 70001)],           # x, y, x
                  [(0, 0, 50000), (0, 20000, 50001), (1, 0, 333)]):      # x[:50000], x[20000:], y
        d = np.concatenate([(x, y)[w][s:s + n] for w, s, n in frags])
        want = expect(oracle, d, 4321, 0, 2, 2, True)
        iov, dp = a.place([x, y], len(want[0]), (5, 2), 13)
        iov = [(iov[w][0] + s, n) for w, s, n in frags]
        assert wv.compose_wire(iov, dp, len(want[0]), 4321, 0, 2, 2, True) == (len(want[0]), want[1])
        a.check(want[0])


@pytest.mark.parametrize("ctype", [2, 1, 0], ids=["crc32c", "crc32", "null"])
@pytest.mark.parametrize("proto", [2, 1])
def test_protocols_and_checksum_types(engine, wv, oracle, proto, ctype):
    lens = [300, 65536 + 7, 5000, 3, 2 * 65536 + 45]
    n = sum(lens)
    d = payload(79, 0, n)
    for off, finish in ((0, False), (4321, True)):
        want = expect(oracle, d, off, 100, proto, ctype, finish)
        run(wv, Arena(engine, room(lens, len(want[0]))), cut(d, lens), want, (1, 6, 3), 0, off, 100, proto, ctype,
            finish)


# ---- both CRC paths and hundreds of workgroups -----------------------------------------------------------
def test_nine_mib_in_five_odd_fragments(engine, wv, oracle):
    n = (9 << 20) + 321
    lens = [(3 << 20) + 11, (1 << 20) + 7, 2000001, 5]
    lens.append(n - sum(lens))
    info = wv.layout(lens, 4321, 2, 2, True)
    assert info["nsegments"] > 0 and info["ngathered"] > 0 and info["max_pieces"] >= 2
    d = payload(80, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    assert len(want[1]) > 140
    run(wv, Arena(engine, room(lens, len(want[0]))), cut(d, lens), want, (3, 1, 7, 5, 9), 6, 4321, 0, 2, 2, True)


# ---- round trip without host bytes ----------------------------------------------------------------
def test_round_trip_through_the_read_side(engine, wv, oracle):
    lens = [65536 + 1234, 999, 4 * 65536 - 999]
    n = sum(lens)
    d = payload(81, 0, n)
    want = expect(oracle, d, 0, 0, 2, 2, True)
    a = Arena(engine, room(lens, len(want[0])))
    dp = run(wv, a, cut(d, lens), want, (5, 2, 3), 11, 0, 0, 2, 2, True)
    wl = len(want[0])
    ref = oracle.verify_packets(want[0].tobytes())
    got = engine.verify_packets(None, dptr=dp, nbytes=wl)
    assert got == ref and got[0] == 0 and got[2] == wl and len(got[1]) == len(want[1])
    for v, p in zip(got[1], want[1]):
        assert (v["stream_off"], v["offset_in_block"], v["seqno"], v["data_len"], v["crc_len"], v["last"]) == \
            (p["hdr_off"], p["offset_in_block"], p["seqno"], p["data_len"], p["crc_len"], p["last"])
    # one byte of packet 3's chunk 10 flipped on the device
    p3 = want[1][3]
    at = a.dst + p3["hdr_off"] + p3["hdr_len"] + 10 * CS + 100
    a.buf.upload(np.array([want[0][at - a.dst] ^ 0x20], dtype=np.uint8), at)
    rc, got, _ = engine.verify_packets(None, dptr=dp, nbytes=wl)
    assert rc == engine.ERR_BAD_CHECKSUM
    assert [(i, p["first_bad"], p["bad_chunks"]) for i, p in enumerate(got) if p["error"]] == [(3, 10, 1)]


# ---- ordering ------------------------------------------------------------------------------------
def _filled_on(engine, wv, oracle, seed, stream):
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
    got_len, got = wv.compose_wire(iov, dp, len(want[0]), 4321, 0, 2, 2, False, stream=stream)
    assert got_len == len(want[0]) and got == want[1]
    for w, piece in zip(a.where, cut(d, lens)):
        a.image[w:w + len(piece)] = piece
    a.check(want[0])


def test_fragments_filled_on_the_null_stream_just_before(engine, wv, oracle):
    """The library's stream waits for the NULL stream."""
    _filled_on(engine, wv, oracle, 82, None)


def test_on_a_stream_of_the_callers(engine, wv, oracle):
    st = engine.stream_create()
    try:
        _filled_on(engine, wv, oracle, 83, st)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


# ---- rejections: nothing is written ------------------------------------------------------------------
def test_rejections_write_nothing(engine, wv, oracle):
    from hadoofus_amd.abi import IoVec, OutPacket
    lens = [40000, 0, 60000]
    n = sum(lens)
    d = payload(84, 0, n)
    stream, recs = expect(oracle, d, 0, 0, 2, 2, True)
    wl, npk = len(stream), len(recs)
    a = Arena(engine, room(lens, wl))
    iov, dp = a.place(cut(d, lens), wl, (1, 0, 6), 3)
    (f0, _), _, (f2, _) = iov
    lib = wv.load()
    arr = (OutPacket * npk)()
    before = bytes(arr)
    cnt, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    host = np.zeros(wl + 64, dtype=np.uint8)
    end = a.buf.ptr + a.buf.nbytes

    def call(p0=f0, p2=f2, wire=dp, cap=wl, maxp=npk):
        vec = (IoVec * 3)(IoVec(p0, 40000), IoVec(None, 0), IoVec(p2, 60000))
        return lib.hdfs_wirev_compose_packets(vec, 3, 0, 0, 2, 2, 1, wire, cap, arr, maxp, ctypes.byref(cnt),
                                              ctypes.byref(used), None)
    cases = {
        "wire_cap one short": (dict(cap=wl - 1), b""),
        "max_pkts one short": (dict(maxp=npk - 1), b""),
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
        err = lib.hdfs_wirev_last_error()
        assert err and text in err, (name, err)
        assert (cnt.value, used.value) == (npk, wl), name
        assert bytes(arr) == before and not host.any(), name
    a.check(np.zeros(0, np.uint8))
    assert call() == 0  # and the same arguments, unspoilt, work
    a.check(stream)


# ---- threads --------------------------------------------------------------------------------------------
def test_two_threads_at_once(engine, wv, oracle):
    jobs = []
    for seed, lens, off, proto in [(85, [100000, 7, 300000 - 7], 0, 2), (86, [123, 250000], 4321, 1)]:
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
                assert wv.compose_wire(iov, dp, len(want[0]), off, 0, proto, 2, True) == (len(want[0]), want[1])
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


# ---- the measurement entry writes the same stream under every flag ----------------------------------------
def test_frame_time_flags_write_the_same_stream(engine, wv, oracle):
    lens = [65536 + 999, 13, 2 * 65536 - 13]
    d = payload(87, 0, sum(lens))
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    a = Arena(engine, room(lens, len(want[0])))
    for flags in (0, wv.TIME_SC1, wv.time_slices(1), wv.time_slices(3) | wv.TIME_SC1, wv.time_slices(16)):
        iov, dp = a.place(cut(d, lens), len(want[0]), (3, 1, 2), 9)
        assert wv.frame_time(iov, dp, len(want[0]), 4321, 2, 2, True, flags, 1) > 0
        a.check(want[0])


# ---- the C consumer -----------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "wirev_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wirev_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wirev", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
