"""GPU: a batch of positional reads in one call (include/hadoofus_pread_batch.h)
-- pread_probe_kernel frames packet 0 and the tail of every stream and works
out each read's window, unframe_window_batch_kernel walks the packets the
reads take, verifies every one of them whole and stores only the window's
bytes; everything else goes to hdfs_crc32c_read_packets, with its window,
inside the call.

The expected result of every entry is the CPU oracle's read_packets of its
stream and window, and also the main library's windowed read of the same
device bytes into a buffer of its own (pread_helpers.reference).  All streams
and all destinations of a batch are carved from one device allocation between
0xA5 guards, at chosen byte residues mod 16; after every call the whole
allocation is downloaded and compared with the image expected (a destination's
bytes between `delivered` and min(dst_cap, read_len) are unspecified and not
compared; its room past the read must stay untouched).  Everything is
bit-exact."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from packet_stream import header_v2
from pread_helpers import AGAIN, Arena, compare, fields, flip, read_of, reference, run, stream_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def pb(engine):
    from hadoofus_read import pread_batch
    pread_batch.load()
    return pread_batch


@pytest.fixture(scope="module")
def scratch(engine):
    """The destination of the main library's reference reads."""
    return engine.DeviceBuffer(10 << 20)


# ---- 1. regular windows ---------------------------------------------------------------------------------
SHAPES = [[65536] * 3 + [12345], [4096] * 20, [512], [65536, 700], [8192] * 5 + [100]]
OFFSETS = (0, 1 << 20)
C_BEGINS = (0, 1, 15, 16, 17, 511, 512, 4095, 4096)


def regular_streams(oracle, proto, ctype):
    """-> [(stream, dlens, offset0)]: the five shapes at both block offsets; the
    last shape carries syncBlock on every packet (v2)."""
    out = []
    for o, off0 in enumerate(OFFSETS):
        for k, dl in enumerate(SHAPES):
            kw = dict(sync_every=1) if proto == 2 and k == 4 else {}
            out.append((stream_of(oracle, proto, ctype, dl, 10 + k + 7 * o, offset0=off0, **kw), dl, off0))
    return out


def window_ends(dlens, cb):
    """The read's ends of every class, as payload positions behind cb: one byte
    in, at a 16-B boundary, mid-piece, at a round boundary, at a packet
    boundary, inside the ragged chunk, at the payload's end."""
    dlen0, payload = dlens[0], sum(dlens)
    ends = {cb + 1, (cb + 16) // 16 * 16, (cb + 16) // 16 * 16 + 7, (cb + 4096) // 4096 * 4096, dlen0,
            len([d for d in dlens if d == dlen0]) * dlen0, payload}
    if dlens[-1] % 512:
        ends.add(payload - dlens[-1] % 512 + 1)
        ends.add(payload - 1)
    return sorted(e for e in ends if cb < e <= payload)


def regular_reads(streams):
    reads = []
    for s, (_, dl, off0) in enumerate(streams):
        for cb in sorted(set(C_BEGINS + (dl[0] - 1,))):
            if cb >= dl[0]:
                continue
            reads += [read_of(s, off0 + cb, e - cb) for e in window_ends(dl, cb)]
        if off0:  # the read starts 5 bytes before packet 0: c_begin 0
            reads += [read_of(s, off0 - 5, e) for e in window_ends(dl, 0)]
    return reads


@pytest.mark.parametrize("ctype", [2, 1])
@pytest.mark.parametrize("proto", [1, 2])
def test_regular_windows_take_the_kernel_path(engine, pb, oracle, scratch, proto, ctype):
    """Five stream shapes at block offsets 0 and 1 MiB, every c_begin of the
    list (and a read that starts 5 bytes before packet 0) crossed with read
    ends of every class, read_len 1 and the whole remaining payload among
    them: one batch, with records and without."""
    streams = regular_streams(oracle, proto, ctype)
    reads = regular_reads(streams)
    assert 500 < len(reads) <= pb.MAX_ENTRIES and min(r["n"] for r in reads) == 1
    raw = [s for s, _, _ in streams]
    K = [pb.PATH_KERNEL] * len(reads)
    got, want, a = run(pb, engine, oracle, scratch, raw, reads, proto, ctype, paths=K)
    assert all(g["rc"] == 0 and g["delivered"] == r["n"] for g, r in zip(got, reads))
    assert max(len(g["records"]) for g in got) == 20 and min(len(g["records"]) for g in got) == 1
    run(pb, engine, oracle, scratch, raw, reads, proto, ctype, paths=K, records=False, want=want)


def test_a_read_before_block_offset_zero_is_the_main_librarys_einval(engine, pb, oracle, scratch):
    """client_offset 5 bytes before a packet 0 at block offset 0 is negative: no
    client read (hdfs_crc32c_read_packets: EINVAL).  That entry's rc is the main
    call's and the text names it; its neighbours are served."""
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 5)]
    reads = [read_of(0, 0, 100), read_of(0, -5, 100), read_of(0, 7, 100)]
    a = Arena(engine, streams, reads)
    with pytest.raises(engine.CRC32CError) as e:
        engine.read_packets(a.stream_ptr(reads[1]), len(streams[0]), scratch.ptr, 100, max_pkts=8, client_offset=-5,
                            read_len=100)
    assert e.value.code == EINVAL
    got = pb.read(a.batch(pb), max_pkts=8)
    assert [g["rc"] for g in got] == [0, EINVAL, 0] and got[1]["path"] == pb.PATH_FALLBACK
    assert (got[1]["consumed"], got[1]["delivered"], got[1]["records"]) == (0, 0, [])
    assert b"entry 1" in pb.load().hdfs_pread_batch_last_error()
    assert [g["path"] for g in got[::2]] == [pb.PATH_KERNEL] * 2
    want = [oracle.read_packets(streams[0], r["off"], r["n"])[3] for r in reads[::2]]
    a.check([want[0], None, want[1]])


# ---- 2. the read ends early ---------------------------------------------------------------------------------
def test_the_read_ends_early(engine, pb, oracle, scratch):
    """A 64 KiB window at the head of a 2 MiB stream takes one packet (c_begin 0)
    or two; a CRC byte and a data byte flipped in the packet behind the window
    are never looked at."""
    s = stream_of(oracle, 2, 2, [65536] * 32, 30, offset0=1 << 20)
    recs = oracle.verify_packets(s, 2, 512, 2)[1]
    for p in (1, 2):  # the packet after the one-packet window, and after the two-packet one
        s = flip(s, recs[p]["stream_off"] + recs[p]["header_len"] + 4 * (3 + p) + 1)
        s = flip(s, recs[p]["stream_off"] + recs[p]["header_len"] + recs[p]["crc_len"] + 20000 + p)
    assert oracle.verify_packets(s, 2, 512, 2)[0] == engine.ERR_BAD_CHECKSUM
    reads = [read_of(0, 1 << 20, 65536), read_of(0, (1 << 20) + 100, 65536 - 100)]
    got, _, _ = run(pb, engine, oracle, scratch, [s], reads, paths=[pb.PATH_KERNEL] * 2)
    assert [(g["rc"], len(g["records"]), g["consumed"]) for g in got] == [(0, 1, recs[1]["stream_off"])] * 2
    s2 = stream_of(oracle, 2, 2, [65536] * 32, 31)
    recs = oracle.verify_packets(s2, 2, 512, 2)[1]
    s2 = flip(flip(s2, recs[2]["stream_off"] + recs[2]["header_len"] + 9), recs[2]["stream_off"] + 40000)
    got, _, _ = run(pb, engine, oracle, scratch, [s2], [read_of(0, 100, 65536)], paths=[pb.PATH_KERNEL])
    assert (got[0]["rc"], len(got[0]["records"]), got[0]["consumed"]) == (0, 2, recs[2]["stream_off"])


# ---- 3. corruption inside taken packets, outside the delivered bytes ---------------------------------------------
@pytest.mark.parametrize("what", ["skipped head", "behind the read's end", "behind the end, ragged chunk",
                                  "header of a body packet"])
@pytest.mark.parametrize("proto", [1, 2])
def test_corruption_outside_the_delivered_bytes(engine, pb, oracle, scratch, proto, what):
    """The window [3000, 3000 + 2 * 65536) of [65536] * 3 + [12345] takes packets
    0..2 and delivers neither the first 3000 bytes of packet 0 nor packet 2
    from byte 3000 on; a second read ends inside the ragged chunk of packet 3.
    One entry of five is corrupt; the others stay on the kernel path."""
    streams = [stream_of(oracle, proto, 2, [65536] * 3 + [12345], 40 + k, offset0=512) for k in range(5)]
    recs = oracle.verify_packets(streams[2], proto, 512, 2)[1]
    data = lambda i: recs[i]["stream_off"] + recs[i]["header_len"] + recs[i]["crc_len"]  # noqa: E731
    reads = [read_of(k, 512 + 3000, 2 * 65536) for k in range(5)]
    if what == "behind the end, ragged chunk":
        reads[2] = read_of(2, 512 + 3000, 3 * 65536 + 24 * 512 + 10 - 3000)
    where = {"skipped head": data(0) + 2 * 512 + 77, "behind the read's end": data(2) + 100 * 512 + 5,
             "behind the end, ragged chunk": data(3) + 24 * 512 + 40,
             "header of a body packet": recs[1]["stream_off"] + (12 + 7 if proto == 1 else 6 + 10)}[what]
    streams[2] = flip(streams[2], where)
    paths = [pb.PATH_KERNEL] * 5
    paths[2] = pb.PATH_FALLBACK
    got, _, _ = run(pb, engine, oracle, scratch, streams, reads, proto, 2, paths=paths)
    bad = got[2]
    chunk = {"skipped head": (0, 2), "behind the read's end": (2, 100), "behind the end, ragged chunk": (3, 24)}
    if what in chunk:
        pkt, first = chunk[what]
        assert bad["rc"] == engine.ERR_BAD_CHECKSUM and len(bad["records"]) == pkt + 1
        assert [(r["first_bad"], r["bad_chunks"]) for r in bad["records"] if r["error"]] == [(first, 1)]
        assert bad["delivered"] == (0 if pkt == 0 else pkt * 65536 - 3000)
    else:  # the seqno is another one: the main library takes the packet as it is
        assert bad["rc"] == 0 and bad["records"][1]["seqno"] != 1 and bad["delivered"] == 2 * 65536


@pytest.mark.parametrize("which", ["packet K - 1", "the shorter packet"])
@pytest.mark.parametrize("to", ["block offset 0", "50 bytes below the read's start", "512 bytes early", "512 bytes late"])
@pytest.mark.parametrize("proto", [1, 2])
def test_an_offset_off_the_sequence_on_a_tail_packet(engine, pb, oracle, scratch, proto, which, to):
    """The probe frames packet K - 1 and the shorter packet itself and predicts
    neither, so the header comparison takes their offsetInBlock as it is.  The
    main library gives every packet the c_begin of its own offsetInBlock: a
    CRC-clean stream whose tail packet names another offset ends in
    UNEXPECTED_READ_OFFSET, skips bytes of that packet, or delivers the same
    bytes -- the oracle's result each time, on the fallback path whenever the
    read takes that packet, on the kernel path when it ends ahead of it."""
    dl, off0, cb = [8192] * 3 + [700], 1 << 20, 300
    k = 2 if which == "packet K - 1" else 3
    at = off0 + sum(dl[:k])
    skew = {"block offset 0": -at, "50 bytes below the read's start": off0 + cb - 50 - at, "512 bytes early": -512,
            "512 bytes late": 512}[to]
    streams = [stream_of(oracle, proto, 2, dl, 45 + j, offset0=off0, offset_skew={k: skew} if j == 1 else None)
               for j in range(3)]
    whole = sum(dl) - cb
    reads = [read_of(0, off0 + cb, whole), read_of(1, off0 + cb, whole), read_of(1, off0 + cb, sum(dl[:k]) - cb + 10),
             read_of(1, off0 + cb, sum(dl[:k]) - cb), read_of(2, off0 + cb, whole)]
    K, F = pb.PATH_KERNEL, pb.PATH_FALLBACK
    got, want, _ = run(pb, engine, oracle, scratch, streams, reads, proto, 2, paths=[K, F, F, K, K])
    assert got[1]["records"][k]["offset_in_block"] == at + skew
    if to == "block offset 0":
        assert got[1]["rc"] == got[2]["rc"] == engine.ERR_UNEXPECTED_READ_OFFSET
        assert got[1]["delivered"] == got[2]["delivered"] == sum(dl[:k]) - cb
    elif to == "50 bytes below the read's start":
        # 50 bytes of that packet are skipped: the short read completes, the whole one runs out of stream
        assert got[2]["rc"] == 0 and got[2]["delivered"] == reads[2]["n"]
        assert got[1]["rc"] == engine.ERR_BAD_LASTPACKET and got[1]["delivered"] == whole - 50
    else:
        assert got[1]["rc"] == 0 and got[1]["delivered"] == whole
    assert got[3]["rc"] == 0 and got[3]["delivered"] == reads[3]["n"]


# ---- 4. irregular entries among regular ones ---------------------------------------------------------------------
def test_irregular_entries_among_regular_ones(engine, pb, oracle, scratch):
    reg = lambda k: stream_of(oracle, 2, 2, [65536] * 2 + [3000], 50 + k, offset0=4096)  # noqa: E731
    pay = 2 * 65536 + 3000
    streams = [reg(0),
               reg(1),                                                              # c_begin >= dlen0
               reg(2),                                                              # longer than the stream, empty last
               stream_of(oracle, 2, 2, [65536] * 2 + [3000], 53, offset0=4096, last_empty=False),  # ... last flag
               stream_of(oracle, 2, 2, [65536] * 3, 54, offset0=4096, last_flag=99, last_empty=False)[:-1000],  # cut
               stream_of(oracle, 2, 2, [4096] * 6, 55, offset0=4096,                # a non-canonical v2 header
                         header=lambda k, off, seq, last, dl: header_v2(off, seq, last, dl) + b"\x30\x01"),
               stream_of(oracle, 2, 2, [4096] * 6, 56, offset0=4096, last_flag=2),  # a last flag on a body packet
               reg(7)]
    reads = [read_of(0, 4096 + 10, 70000),
             read_of(1, 4096 + 65536, 100),
             read_of(2, 4096 + 10, pay),
             read_of(3, 4096 + 10, pay),
             read_of(4, 4096 + 10, 3 * 65536 - 10),
             read_of(5, 4096 + 10, 9000),
             read_of(6, 4096 + 10, 5 * 4096),
             read_of(7, 4096 + 65535, 3002)]
    K, F = pb.PATH_KERNEL, pb.PATH_FALLBACK
    got, _, _ = run(pb, engine, oracle, scratch, streams, reads, paths=[K, F, F, F, F, F, F, K])
    assert [g["rc"] for g in got] == [0, engine.ERR_UNEXPECTED_READ_OFFSET, engine.ERR_BAD_LASTPACKET,
                                      engine.ERR_BAD_LASTPACKET, 0, 0, engine.ERR_BAD_LASTPACKET, 0]
    assert got[4]["delivered"] == 2 * 65536 - 10 and len(got[4]["records"]) == 2  # the walk ends at the cut packet
    assert got[6]["delivered"] == 3 * 4096 - 10 and got[7]["delivered"] == 3002


def test_a_destination_one_byte_short_is_again_and_resumes(engine, pb, oracle, scratch):
    """dst_cap = read_len - 1: AGAIN with the resume point, on the fallback path;
    a second call with stream + consumed, client_offset + delivered and
    read_len - delivered completes the read."""
    streams = [stream_of(oracle, 2, 2, [8192] * 4 + [999], 60 + k, offset0=1024) for k in range(3)]
    n = 3 * 8192 + 500
    reads = [read_of(0, 1024 + 300, n), read_of(1, 1024 + 300, n, cap=n - 1), read_of(2, 1024 + 300, n)]
    K = pb.PATH_KERNEL
    got, want, a = run(pb, engine, oracle, scratch, streams, reads, paths=[K, pb.PATH_FALLBACK, K])
    g = got[1]
    assert (g["rc"], g["delivered"]) == (AGAIN, n - 1) and 0 < g["consumed"] < len(streams[1])
    whole = oracle.read_packets(streams[1], 1024 + 300, n)[3]
    assert want[1][3] == whole[:n - 1]
    rest = streams[1][g["consumed"]:]
    got2, want2, _ = run(pb, engine, oracle, scratch, [rest], [read_of(0, 1024 + 300 + n - 1, 1)], paths=[K])
    assert got2[0]["rc"] == 0 and want[1][3] + want2[0][3] == whole


def test_max_pkts_one_short_cuts_the_run(engine, pb, oracle, scratch):
    streams = [stream_of(oracle, 2, 2, [65536] * 4, 70 + k) for k in range(3)]
    reads = [read_of(0, 100, 3 * 65536 - 100), read_of(1, 100, 3 * 65536), read_of(2, 100, 65536)]
    K = pb.PATH_KERNEL
    got, _, _ = run(pb, engine, oracle, scratch, streams, reads, max_pkts=3, paths=[K, pb.PATH_FALLBACK, K])
    assert [(g["rc"], len(g["records"]), g["delivered"]) for g in got] == \
        [(0, 3, 3 * 65536 - 100), (0, 3, 3 * 65536 - 100), (0, 2, 65536)]


def test_chunk_size_4096_is_the_main_librarys(engine, pb, oracle, scratch):
    streams = [stream_of(oracle, 2, 2, dl, 80 + k, cs=4096) for k, dl in enumerate([[65536] * 2 + [5000], [8192]])]
    reads = [read_of(0, 100, 70000), read_of(1, 4097, 4000)]
    run(pb, engine, oracle, scratch, streams, reads, cs=4096, paths=[pb.PATH_FALLBACK] * 2)


# ---- 5. many packets per workgroup ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case1(engine, pb, oracle, scratch):
    """Case 1's batch (v2, CRC32C) placed once, with its references."""
    streams = regular_streams(oracle, 2, 2)
    reads = regular_reads(streams)
    raw = [s for s, _, _ in streams]
    a = Arena(engine, raw, reads)
    want = [reference(engine, oracle, scratch, a, raw, r, 2, 2, 512, 64) for r in reads]
    return raw, reads, a, want


@pytest.mark.parametrize("groups", [1, 3, 1024])
def test_few_workgroups_walk_many_packets(engine, pb, oracle, scratch, case1, groups):
    raw, reads, a, want = case1
    a.buf.upload(a.image)  # the destinations as they were
    run(pb, engine, oracle, scratch, raw, reads, groups=groups, paths=[pb.PATH_KERNEL] * len(reads), want=want, arena=a)


def test_groups_out_of_range_is_einval_and_writes_nothing(engine, pb, oracle):
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 91)]
    a = Arena(engine, streams, [read_of(0, 10, 5000)])
    lib, ms = pb.load(), ctypes.c_double(0)
    for flags in (pb.time_groups(pb.MAX_GROUPS + 1), pb.time_groups(1 << 20), 1, pb.time_groups(2) | 4):
        arr = pb.entries(a.batch(pb))
        assert lib.hdfs_pread_batch_time(arr, 1, 2, 512, 2, flags, 1, ctypes.byref(ms)) == EINVAL
        assert b"workgroups" in lib.hdfs_pread_batch_last_error()
        assert (arr[0].rc, arr[0].npkts, arr[0].consumed, arr[0].delivered) == (0, 0, 0, 0)
    a.check([])


# ---- 6. ordering ----------------------------------------------------------------------------------------------------
def test_streams_copied_on_the_null_stream_just_before(engine, pb, oracle):
    """No synchronisation between the device-to-device copies that put the
    streams in place (NULL stream) and the call: the library's stream waits for
    the NULL stream."""
    streams = [stream_of(oracle, 2, 2, [65536] * 30 + [777], 100 + k, offset0=512) for k in range(2)]
    reads = [read_of(k, 512 + 300, 29 * 65536 + 1000) for k in range(2)]
    pay = [oracle.read_packets(s, r["off"], r["n"])[3] for s, r in zip(streams, reads)]
    stage = engine.DeviceBuffer(sum(len(s) for s in streams))
    stage.upload(np.frombuffer(b"".join(streams), dtype=np.uint8))
    a = Arena(engine, [bytes(len(s)) for s in streams], reads)  # zeros where the streams go
    engine.device_sync()
    lib, at = engine.load(), 0
    for k, s in enumerate(streams):
        assert lib.hdfs_crc32c_memcpy(a.buf.ptr + a.src[k], stage.ptr + at, len(s), 2) == 0
        at += len(s)
    got = pb.read(a.batch(pb), max_pkts=40)
    assert [(g["rc"], g["delivered"], g["path"]) for g in got] == [(0, len(p), pb.PATH_KERNEL) for p in pay]
    for k, s in enumerate(streams):
        a.image[a.src[k]:a.src[k] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    a.check(pay)


def test_on_a_stream_of_the_callers(engine, pb, oracle, scratch, case1):
    raw, reads, a, want = case1
    a.buf.upload(a.image)
    st = engine.stream_create()
    try:
        run(pb, engine, oracle, scratch, raw, reads, stream=st, paths=[pb.PATH_KERNEL] * len(reads), want=want, arena=a)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, pb, oracle):
    jobs = []
    for seed, dl, proto in [(110, [65536] * 5 + [900], 2), (111, [8192] * 30, 1)]:
        streams = [stream_of(oracle, proto, 2, dl, seed + 10 * k, offset0=1024) for k in range(3)]
        streams[1] = flip(streams[1], len(streams[1]) // 2)  # one entry of each batch falls back
        reads = [read_of(k, 1024 + 77 + k, sum(dl) - 1000) for k in range(3)]
        want = [oracle.read_packets(s, r["off"], r["n"], proto, 512, 2) for s, r in zip(streams, reads)]
        jobs.append((Arena(engine, streams, reads), proto, want))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, proto, want = jobs[i]
            start.wait()
            for _ in range(4):
                got = pb.read(a.batch(pb), proto, max_pkts=40)
                compare(got, want, [pb.PATH_KERNEL, pb.PATH_FALLBACK, pb.PATH_KERNEL])
        except BaseException as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for a, _, want in jobs:
        a.check([w[3] for w in want])


# ---- 7. refusals that need the device ----------------------------------------------------------------------------------
def test_refusals_leave_the_arena_untouched_and_name_the_entry(engine, pb, oracle):
    from hadoofus_amd.abi import Packet
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 120 + k) for k in range(4)]
    reads = [read_of(k, 100, 8000) for k in range(4)]
    pay = [oracle.read_packets(s, 100, 8000)[3] for s in streams]
    a = Arena(engine, streams, reads)
    lib, p, end = pb.load(), a.buf.ptr, a.buf.ptr + a.buf.nbytes
    host = np.zeros(1 << 16, dtype=np.uint8)
    pk = (Packet * 32)()
    before = bytes(pk)
    cap = reads[0]["cap"]

    def call(n=4, **kw):
        """kw: {field}{entry}=value, e.g. dst2=..., stream0=..., rl1=..."""
        b = a.batch(pb)
        for key, v in kw.items():
            b[int(key[-1])][{"stream": "stream_ptr", "dst": "dst_ptr", "rl": "read_len"}[key[:-1]]] = v
        arr = pb.entries(b)
        for e in arr:
            e.rc, e.npkts, e.consumed, e.delivered = 7, 7, 7, 7
        rc = lib.hdfs_pread_batch_read(arr, n, 2, 512, 2, pk, 8, None)
        assert [(e.rc, e.npkts, e.consumed, e.delivered) for e in arr][:n] == [(0, 0, 0, 0)] * n or rc == 0
        return rc, lib.hdfs_pread_batch_last_error().decode()
    # (kw, text, exact): exact texts are asserted whole, the others as a part.  Of the overlap cases "inside stream 1"
    # provokes exactly one overlapping pair.  The other two provoke two each, of which one is named: a range of this
    # size laid over the last byte of dst 0 reaches over the guard bytes into dst 1 as well, and one laid back from
    # the first byte of stream 1 reaches into stream 0 as well.
    cases = {
        "a host stream in entry 3": (dict(stream3=host.ctypes.data), "entry 3", False),
        "a host destination in entry 2": (dict(dst2=host.ctypes.data), "entry 2", False),
        "stream 0 past its allocation": (dict(stream0=end - a.lens[0] + 1), "entry 0", False),
        "destination 3 past its allocation": (dict(dst3=end - cap + 1), "entry 3", False),
        "destination 2 overlaps destination 0": (dict(dst2=p + a.dst[0] + cap - 1), "entry 2", False),
        "destination 3 inside stream 1": (dict(dst3=p + a.src[1] + 10), "entry 3: dst overlaps the stream of entry 1", True),
        "destination 1 overlaps its own stream": (dict(dst1=p + a.src[1] - cap + 1), "entry 1", False),
        "read_len 0 in entry 2": (dict(rl2=0), "entry 2", False),
        "READ_ALL in entry 1": (dict(rl1=-1), "hdfs_read_batch_read_blocks", False),
    }
    for name, (kw, text, exact) in cases.items():
        rc, err = call(**kw)
        assert rc == EINVAL and (err == text if exact else text in err), (name, err)
        assert bytes(pk) == before and not host.any(), name
    a.check([])
    rc, err = call()  # and the same arguments, unspoilt, work
    assert rc == 0
    a.check(pay)


# ---- 8. agreement with the read batch -----------------------------------------------------------------------------------
def test_a_whole_payload_window_agrees_with_the_read_batch(engine, pb, oracle, scratch):
    from hadoofus_read import read_batch as rb
    dls = [[65536] * 3 + [12345], [4096] * 20, [65536, 700]]
    streams = [stream_of(oracle, 2, 2, dl, 130 + k, offset0=1 << 20) for k, dl in enumerate(dls)]
    reads = [read_of(k, 1 << 20, sum(dl)) for k, dl in enumerate(dls)]
    got, want, a = run(pb, engine, oracle, scratch, streams, reads, paths=[pb.PATH_KERNEL] * 3)
    whole = engine.DeviceBuffer(sum(r["n"] + 64 for r in reads))
    at = [sum(r["n"] + 64 for r in reads[:k]) + (1, 0, 5)[k] for k in range(3)]
    blocks = rb.read_blocks([rb.entry(a.stream_ptr(r), len(streams[k]), whole.ptr + at[k], r["n"])
                             for k, r in enumerate(reads)], max_pkts=40)
    img = whole.download()
    for k, (g, b, r) in enumerate(zip(got, blocks, reads)):
        assert b["rc"] == 0 and b["path"] == rb.PATH_KERNEL and b["delivered"] == g["delivered"] == r["n"]
        assert img[at[k]:at[k] + r["n"]].tobytes() == want[k][3]
        assert b["consumed"] - g["consumed"] == 31 and len(b["records"]) == len(g["records"]) + 1  # the empty last one
        assert fields(b["records"][:-1]) == fields(g["records"])


# ---- 9. one large entry -------------------------------------------------------------------------------------------------
def test_one_large_entry(engine, pb, oracle, scratch):
    """8 MiB + 777 B of 64 KiB packets; the window starts at c_begin 300 and ends
    1000 B before the payload's end, inside the last packet's full chunks."""
    n = (8 << 20) + 777
    s = stream_of(oracle, 2, 2, [65536] * 128 + [777], 140, offset0=1 << 30)
    reads = [read_of(0, (1 << 30) + 300, n - 300 - 1000)]
    got, _, _ = run(pb, engine, oracle, scratch, [s], reads, max_pkts=160, paths=[pb.PATH_KERNEL])
    assert got[0]["rc"] == 0 and len(got[0]["records"]) == 128 and got[0]["delivered"] == n - 1300


# ---- 10. the C consumer -------------------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "pread_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "pread_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_pread_batch", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
