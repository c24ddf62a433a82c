"""GPU: a write's packets as one wire stream in device memory, made in one pass
(include/hadoofus_wire_fused.h) -- frame_fused_kernel copies the data, computes
the chunk CRCs from the registers it copies and writes every byte of the stream.

The expected stream everywhere is built on the host from the CPU oracle:
oracle.compose_packets(data, ...) gives the header buffers and the records;
packet after packet, hdr[hdr_off : hdr_off + hdr_len] is followed by
data[data_off : data_off + data_len].  Source and destination are carved from
one device allocation between 0xA5 guards, at chosen byte residues mod 16;
after every call the whole allocation is downloaded and compared with the
image expected, so the source and the guards are untouched and `wire` equals
the expected stream.  Everything is bit-exact."""
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
GAP = 96  # guard bytes before, between and after the two ranges (at least)


@pytest.fixture(scope="module")
def wf(engine):
    from hadoofus_amd import wire_fused
    wire_fused.load()
    return wire_fused


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


class Arena:
    """One device allocation: guards, the source at residue src_mis mod 16,
    guards, the destination at residue dst_mis mod 16, guards."""

    def __init__(self, engine, max_src, max_wire):
        self.engine = engine
        self.buf = engine.DeviceBuffer(GAP + 16 + max_src + GAP + 16 + max_wire + GAP + 16)
        assert self.buf.ptr % 16 == 0

    def place(self, data, wire_len, src_mis=0, dst_mis=0):
        self.src = (GAP + 15) // 16 * 16 + src_mis
        self.dst = (self.src + len(data) + GAP + 15) // 16 * 16 + dst_mis
        assert self.dst + wire_len + GAP <= self.buf.nbytes
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        self.image[self.src:self.src + len(data)] = data
        self.buf.upload(self.image)
        self.n, self.wire_len = len(data), wire_len
        return self.buf.ptr + self.src, self.buf.ptr + self.dst

    def check(self, stream):
        """The whole allocation: the stream where it belongs, nothing else changed."""
        want = self.image.copy()
        want[self.dst:self.dst + len(stream)] = stream
        got = self.buf.download()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (src {self.src}, dst {self.dst}, "
                                 f"stream {len(stream)}): got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def run(wf, arena, data, want, src_mis=0, dst_mis=0, off=0, seq=0, proto=2, ctype=2, finish=False):
    stream, recs = want
    sp, dp = arena.place(data, len(stream), src_mis, dst_mis)
    got_len, got = wf.compose_wire(sp, len(data), dp, len(stream), off, seq, proto, ctype, finish)
    assert got_len == len(stream) and got == recs
    arena.check(stream)
    return dp


# ---- every phase -----------------------------------------------------------------------
def test_every_source_and_destination_phase(engine, wf, oracle):
    """A 287-byte first packet, two full packets and a tail; every destination
    residue mod 16 against source residues 0, 1, 2, 3 and 7.  For one of them
    the stream is also the two-pass library's, downloaded."""
    n = 2 * 65536 + 700
    d = payload(51, 0, n)
    want = expect(oracle, d, 4321, 3, 2, 2, True)
    assert [p["data_len"] for p in want[1]] == [287, 65536, 65536, 700 - 287, 0]
    a = Arena(engine, n, len(want[0]))
    for dst_mis in range(16):
        for src_mis in (0, 1, 2, 3, 7):
            run(wf, a, d, want, src_mis, dst_mis, 4321, 3, 2, 2, True)
    from hadoofus_amd import wire
    two = engine.DeviceBuffer(len(want[0]) + 16)
    sp = a.buf.ptr + a.src
    assert wire.compose_wire(sp, n, two.ptr + 5, len(want[0]), 4321, 3, 2, 2, True) == (len(want[0]), want[1])
    fused = a.buf.download()[a.dst:a.dst + len(want[0])]
    assert np.array_equal(two.download()[5:5 + len(want[0])], fused)


# ---- every packet-start residue in one call ----------------------------------------------
EIGHTEEN = 17 * 65536 + 45
_eighteen = {}


def eighteen():
    if "d" not in _eighteen:
        _eighteen["d"] = payload(52, 0, EIGHTEEN)
    return _eighteen["d"]


@pytest.mark.parametrize("ctype", [2, 1, 0], ids=["crc32c", "crc32", "null"])
@pytest.mark.parametrize("proto", [2, 1])
def test_every_packet_start_residue(engine, wf, oracle, proto, ctype):
    """18 packets; a full packet's stride is 15 (v2) or 9 (v1) mod 16 with
    checksums, 15 or 9 without: the packets start at all 16 residues."""
    d = eighteen()
    want = expect(oracle, d, 0, 100, proto, ctype, False)
    assert len(want[1]) == 18 and {p["hdr_off"] % 16 for p in want[1]} == set(range(16))
    run(wf, Arena(engine, EIGHTEEN, len(want[0])), d, want, 1, 0, 0, 100, proto, ctype, False)


# ---- small writes: only ragged chunks, or one full chunk and a byte ---------------------------
def test_small_writes(engine, wf, oracle):
    d = payload(53, 0, 513)
    a = Arena(engine, 513, 513 + 2 * 31 + 8 + 64)
    k = 0
    for n in (1, 15, 16, 17, 287, 511, 512, 513):
        for off in (0, 4321):
            for finish in (False, True):
                k += 1
                for proto, ctype in ((2, 2), (1, 1)):
                    want = expect(oracle, d[:n], off, 9, proto, ctype, finish)
                    run(wf, a, d[:n], want, k % 5, (7 * k) % 16, off, 9, proto, ctype, finish)


def test_empty_write(engine, wf, oracle):
    a = Arena(engine, 0, 64)
    empty = np.zeros(0, np.uint8)
    for dst_mis in (0, 1, 9, 15):
        for proto in (1, 2):
            want = expect(oracle, empty, 1024, 4, proto, 2, True)
            assert len(want[1]) == 1 and want[1][0]["last"] == 1 and len(want[0]) == (25 if proto == 1 else 31)
            run(wf, a, empty, want, 0, dst_mis, 1024, 4, proto, 2, True)
    # without finish: no packet, nothing written
    _, dp = a.place(empty, 0, 0, 3)
    assert wf.compose_wire(None, 0, dp, 64, 1024, 4, 2, 2, False) == (0, [])
    a.check(empty)


# ---- ragged rounds: a last packet of few chunks, a last round of few, a partial last chunk ---------
RAGGED = [(c, t) for c in (1, 7, 8, 9, 127) for t in (0, 1, 15, 16, 17, 511)]


def test_ragged_rounds(engine, wf, oracle):
    """One full packet, then a last packet of c full chunks and a partial last
    chunk of t bytes (t = 0: none).  Five of the thirty also at block offset
    4321, where a 287-byte packet comes first and the grid moves."""
    top = 65536 + 127 * CS + 511
    d = payload(62, 0, top)
    a = Arena(engine, top, top + 3 * 31 + 4 * 260 + 64)
    for k, (c, t) in enumerate(RAGGED):
        n = 65536 + c * CS + t
        for off in ((0, 4321) if k % 6 == 2 else (0,)):
            want = expect(oracle, d[:n], off, 0, 2, 2, False)
            if off == 0:
                assert want[1][-1]["data_len"] == c * CS + t and want[1][-1]["crc_len"] == 4 * (c + (t > 0))
            run(wf, a, d[:n], want, (k + 1) % 4, (5 * k + 3) % 16, off, 0, 2, 2, False)


# ---- the walk: every workgroup takes many packets and an uneven share --------------------------
@pytest.mark.parametrize("groups", [1, 3, 7])
def test_few_workgroups_walk_many_packets(engine, wf, oracle, groups):
    d = eighteen()
    want = expect(oracle, d, 0, 0, 2, 2, True)
    assert len(want[1]) == 19
    a = Arena(engine, EIGHTEEN, len(want[0]))
    sp, dp = a.place(d, len(want[0]), 3, 9)
    assert wf.fused_time(sp, EIGHTEEN, dp, len(want[0]), 0, 2, 2, True, wf.time_groups(groups), 1) > 0
    a.check(want[0])


def test_nine_mib_at_an_odd_address(engine, wf, oracle):
    """The product's grid: more packets than one per workgroup would need."""
    n = (9 << 20) + 321
    d = payload(54, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    assert len(want[1]) > 140
    run(wf, Arena(engine, n, len(want[0])), d, want, 3, 6, 4321, 0, 2, 2, True)


def test_groups_out_of_range_is_einval(engine, wf, oracle):
    n = 3 * 65536 + 999
    d = payload(61, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, True)
    a = Arena(engine, n, len(want[0]))
    sp, dp = a.place(d, len(want[0]), 3, 9)
    lib, ms = wf.load(), ctypes.c_double(0)
    for flags in (wf.time_groups(wf.MAX_GROUPS + 1), wf.time_groups(1 << 20), 1, wf.time_groups(2) | 4):
        assert lib.hdfs_wire_fused_time(sp, n, 4321, 2, 2, 1, dp, len(want[0]), flags, 1, ctypes.byref(ms)) == EINVAL
        assert lib.hdfs_wire_fused_last_error()
    a.check(np.zeros(0, np.uint8))
    assert wf.fused_time(sp, n, dp, len(want[0]), 4321, 2, 2, True, wf.time_groups(wf.MAX_GROUPS), 1) > 0
    a.check(want[0])


# ---- round trip without host bytes ----------------------------------------------------------------
def test_round_trip_through_the_read_side(engine, wf, oracle):
    """The main library's verify kernels check the CRCs this library computed:
    neither this library's arithmetic nor the oracle's decides."""
    n = 5 * 65536 + 1234
    d = payload(55, 0, n)
    want = expect(oracle, d, 0, 0, 2, 2, True)
    a = Arena(engine, n, len(want[0]))
    dp = run(wf, a, d, want, 5, 11, 0, 0, 2, 2, True)
    wl = len(want[0])
    ref = oracle.verify_packets(want[0].tobytes())
    got = engine.verify_packets(None, dptr=dp, nbytes=wl)
    assert got == ref and got[0] == 0 and got[2] == wl and len(got[1]) == len(want[1])
    for v, p in zip(got[1], want[1]):
        assert (v["stream_off"], v["offset_in_block"], v["seqno"], v["data_len"], v["crc_len"], v["last"]) == \
            (p["hdr_off"], p["offset_in_block"], p["seqno"], p["data_len"], p["crc_len"], p["last"])
    out = engine.DeviceBuffer(n)
    rc, pk, used, delivered = engine.read_packets(dp, wl, out.ptr, n, read_len=engine.READ_ALL)
    assert (rc, used, delivered) == (0, wl, n) and np.array_equal(out.download(), d)
    # one byte of packet 3's chunk 10 flipped on the device
    p3 = want[1][3]
    at = a.dst + p3["hdr_off"] + p3["hdr_len"] + 10 * CS + 100
    a.buf.upload(np.array([want[0][at - a.dst] ^ 0x20], dtype=np.uint8), at)
    rc, got, _ = engine.verify_packets(None, dptr=dp, nbytes=wl)
    assert rc == engine.ERR_BAD_CHECKSUM
    assert [(i, p["first_bad"], p["bad_chunks"]) for i, p in enumerate(got) if p["error"]] == [(3, 10, 1)]


# ---- ordering ------------------------------------------------------------------------------------
def test_source_filled_on_the_null_stream_just_before(engine, wf, oracle):
    """No synchronisation between the fill (NULL stream) and the call: the
    library's stream waits for the NULL stream."""
    n = 6 << 20
    d = payload(56, 0, n)
    want = expect(oracle, d, 4321, 0, 2, 2, False)
    a = Arena(engine, n, len(want[0]))
    sp, dp = a.place(np.zeros(n, np.uint8), len(want[0]), 8, 13)
    assert sp % 8 == 0
    engine.fill_splitmix64(sp, n // 8, 56, 0, None)
    got_len, got = wf.compose_wire(sp, n, dp, len(want[0]), 4321, 0, 2, 2, False)
    assert got_len == len(want[0]) and got == want[1]
    a.image[a.src:a.src + n] = d
    a.check(want[0])


def test_on_a_stream_of_the_callers(engine, wf, oracle):
    n = 3 * 65536 + 77
    d = payload(57, 0, n)
    want = expect(oracle, d, 512, 0, 1, 1, True)
    a = Arena(engine, n, len(want[0]))
    sp, dp = a.place(d, len(want[0]), 2, 5)
    st = engine.stream_create()
    try:
        assert wf.compose_wire(sp, n, dp, len(want[0]), 512, 0, 1, 1, True, stream=st) == (len(want[0]), want[1])
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0
    a.check(want[0])


# ---- rejections: nothing is written ------------------------------------------------------------------
def test_rejections_write_nothing(engine, wf, oracle):
    from hadoofus_amd.abi import OutPacket
    n = 100000
    d = payload(58, 0, n)
    stream, recs = expect(oracle, d, 0, 0, 2, 2, True)
    wl, npk = len(stream), len(recs)
    a = Arena(engine, n, wl)
    sp, dp = a.place(d, wl, 1, 3)
    lib = wf.load()
    arr = (OutPacket * npk)()
    before = bytes(arr)
    cnt, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    host = np.zeros(wl + 64, dtype=np.uint8)
    end = a.buf.ptr + a.buf.nbytes

    def call(data=sp, nbytes=n, wire=dp, cap=wl, maxp=npk, proto=2, ctype=2):
        return lib.hdfs_wire_fused_compose_packets(data, nbytes, 0, 0, proto, ctype, 1, wire, cap, arr, maxp,
                                                   ctypes.byref(cnt), ctypes.byref(used), None)
    cases = {
        "host source": dict(data=host.ctypes.data),
        "host wire": dict(wire=host.ctypes.data),
        "source past its allocation": dict(data=end - n + 1, wire=a.buf.ptr),
        "wire past its allocation": dict(wire=end - wl + 1),
        "wire inside the source": dict(wire=sp + 10),
        "wire_cap one short": dict(cap=wl - 1),
        "max_pkts one short": dict(maxp=npk - 1),
        "null data with bytes": dict(data=None),
    }
    for name, kw in cases.items():
        assert call(**kw) == EINVAL, name
        assert (cnt.value, used.value) == (npk, wl) and lib.hdfs_wire_fused_last_error(), name
        assert bytes(arr) == before and not host.any(), name
    # a bad proto or ctype: refused before the sizes are known
    for kw in (dict(proto=3), dict(ctype=7)):
        assert call(**kw) == EINVAL and (cnt.value, used.value) == (0, 0), kw
        assert bytes(arr) == before
    a.check(np.zeros(0, np.uint8))
    assert call() == 0  # and the same arguments, unspoilt, work
    a.check(stream)


# ---- threads --------------------------------------------------------------------------------------------
def test_two_threads_at_once(engine, wf, oracle):
    jobs = []
    for seed, n, off, proto in [(59, 400000, 0, 2), (60, 250123, 4321, 1)]:
        d = payload(seed, 0, n)
        want = expect(oracle, d, off, 0, proto, 2, True)
        a = Arena(engine, n, len(want[0]))
        sp, dp = a.place(d, len(want[0]), seed % 4, seed % 16)
        jobs.append((a, sp, dp, n, off, proto, want))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, sp, dp, n, off, proto, want = jobs[i]
            start.wait()
            for _ in range(4):
                assert wf.compose_wire(sp, n, dp, len(want[0]), off, 0, proto, 2, True) == (len(want[0]), want[1])
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


# ---- the C consumer -----------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "wire_fused_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wire_fused_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wire_fused", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
