"""GPU: a batch of scatter reads in one call (include/hadoofus_preadv_batch.h) --
preadv_probe_kernel frames packet 0 and the tail of every stream and works out
each read's window, unframe_scatter_batch_kernel walks the packets the reads
take, verifies every one of them whole and lays only the window's bytes over
the read's device fragments; everything else goes to hdfs_crc32c_read_packets,
with its window and fragment list, inside the call.

The expected result of every entry is the CPU oracle's read_packets of its
stream and window with the fragments' total as its room, its bytes laid over
the fragments in order, and also the main library's read of the same device
bytes into a scatter list of the same lengths (preadv_helpers.reference).  All
streams and all fragments of a batch are carved from one device allocation
between 0xA5 guards, the fragments in shuffled address order at residues 0, 1,
5 and 15 mod 16; after every call the whole allocation is downloaded and
compared with the image expected (fragment bytes between `delivered` and
min(cap, read_len) are unspecified and not compared; everything past that must
stay untouched).  The path is asserted for every entry.  Everything is
bit-exact."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from preadv_helpers import (AGAIN, Arena, cap_of, compare, cycle, fields, flip, read_of, reference, run, split,
                            stream_of)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
OFF0 = 1 << 20
# the smallest streams at which each branch runs: a full round and a two-chunk round a packet, a packet with a
# ragged chunk of 276 B, the empty last one; all 16 waves; a single 512 B packet
SHAPES = [[5120, 5120, 1300], [65536, 65536, 700], [512]]
C_BEGINS = (0, 100, 511)


@pytest.fixture(scope="module")
def pv(engine):
    from hadoofus_read import preadv_batch
    preadv_batch.load()
    return preadv_batch


@pytest.fixture(scope="module")
def scratch(engine):
    """Where the main library's reference reads scatter to."""
    return engine.DeviceBuffer(4 << 20)


def window_ends(dl, cb):
    """Payload positions: a packet's end, inside a round, inside the ragged
    chunk (where the shape has them)."""
    payload = sum(dl)
    ends = {dl[0], payload, 4096 + 1000, cb + 1}
    if dl[-1] % 512:
        ends.add(payload - 17)
    return sorted(e for e in ends if cb < e <= payload)


def fragment_lists(dl, cb, n, heavy):
    """The fragment lists of a read of n bytes whose first byte is payload
    position cb.  heavy: the lists of thousands of fragments too."""
    rounds = [p * dl[0] + r - cb for p in range(len(dl)) for r in range(0, dl[0] + 1, 4096)]  # round boundaries
    ragged = sum(dl) - dl[-1] % 512 + 100 - cb if dl[-1] % 512 else 0
    lists = [[n], [1, n - 1], [n - 1, 1], split(n, [16, 64, 1024, 4096 + 160]), split(n, rounds),
             split(n, [4096 - cb - 6 + i for i in range(38)]), split(n, [ragged]),
             [None, 0] + split(n, [n // 3]) [:1] + [0, None] + split(n, [n // 3])[1:] + [None, 0],
             [n, 50, 7], split(n, [n - 10]) [:-1] + [10 if n > 10 else n, 33], [n + 5]]
    if heavy:
        lists.append(cycle(n))
    out = []
    for fl in lists:
        fl = [f for f in fl if f is None or f >= 0]
        if sum(f or 0 for f in fl) >= n and fl not in out:
            out.append(fl)
    return out


def regular_reads(shapes=SHAPES):
    reads = []
    for s, dl in enumerate(shapes):
        for cb in C_BEGINS:
            if cb >= dl[0]:
                continue
            for e in window_ends(dl, cb):
                heavy = cb == 100 and e == sum(dl) and dl[0] <= 5120
                reads += [read_of(s, OFF0 + cb, e - cb, fl) for fl in fragment_lists(dl, cb, e - cb, heavy)]
    return reads


def streams_of(oracle, proto, ctype, seed=10):
    return [stream_of(oracle, proto, ctype, dl, seed + k, offset0=OFF0) for k, dl in enumerate(SHAPES)]


# ---- 1. regular reads over every kind of fragment list ------------------------------------------------------
@pytest.mark.parametrize("ctype", [2, 1])
@pytest.mark.parametrize("proto", [1, 2])
def test_regular_reads_take_the_kernel_path(engine, pv, oracle, scratch, proto, ctype):
    """Three stream shapes, c_begin 0, 100 and 511, window ends on a packet's
    end, inside a round and inside the ragged chunk, each read over: one
    fragment, [1, rest], [rest, 1], cuts at multiples of 16, cuts on the round
    boundaries, 37 one-byte fragments from 6 bytes before a round boundary, a
    boundary inside the ragged chunk, empty fragments with and without a base
    at the front, middle and end, room behind the read (a boundary exactly at
    read_len, untouched trailing fragments), and 3-5-7-11-13-byte fragments over
    the whole read.  One batch, with records and without."""
    streams = streams_of(oracle, proto, ctype)
    reads = regular_reads()
    assert 100 < len(reads) <= pv.MAX_ENTRIES and min(r["n"] for r in reads) == 1
    assert max(len(r["frags"]) for r in reads) > 1000 and any(cap_of(r) > r["n"] for r in reads)
    K = [pv.PATH_KERNEL] * len(reads)
    got, want, a = run(pv, engine, oracle, scratch, streams, reads, K, proto, ctype)
    assert all(g["rc"] == 0 and g["delivered"] == r["n"] for g, r in zip(got, reads))
    run(pv, engine, oracle, scratch, streams, reads, K, proto, ctype, records=False, want=want, arena=a)


def test_one_fragment_agrees_with_the_pread_batch(engine, pv, oracle, scratch):
    from hadoofus_read import pread_batch as pb
    streams = streams_of(oracle, 2, 2, 20)
    reads = [read_of(s, OFF0 + cb, sum(dl) - cb - 3) for s, dl in enumerate(SHAPES) for cb in C_BEGINS if cb < dl[0] - 3]
    got, want, a = run(pv, engine, oracle, scratch, streams, reads, [pv.PATH_KERNEL] * len(reads))
    dst = engine.DeviceBuffer(sum(r["n"] + 16 for r in reads))
    at = [sum(q["n"] + 16 for q in reads[:k]) + k % 3 for k in range(len(reads))]
    flat = pb.read([pb.entry(a.stream_ptr(r), a.lens[r["s"]], dst.ptr + at[k], r["n"], r["off"], r["n"])
                    for k, r in enumerate(reads)], max_pkts=64)
    img = dst.download()
    for k, (g, f, r) in enumerate(zip(got, flat, reads)):
        assert (f["rc"], f["path"], f["consumed"], f["delivered"]) == (0, pb.PATH_KERNEL, g["consumed"], g["delivered"])
        assert fields(f["records"]) == fields(g["records"]) and img[at[k]:at[k] + r["n"]].tobytes() == want[k][3]


# ---- 2. corruption ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["inside a seamed round", "skipped head", "behind the read's end"])
def test_a_flipped_crc_is_the_fallbacks(engine, pv, oracle, scratch, what):
    """[5120, 5120, 1300], the read [700, 700 + 6000): packet 0 from byte 700
    on and 1 580 bytes of packet 1, over 100-byte fragments (every round is
    seamed).  One CRC byte of entry 1 of 3 is flipped: of the chunk that holds
    destination bytes inside a seamed round, of chunk 0 (the skipped head), of
    packet 1's chunk 9 (behind the read's end)."""
    streams = [stream_of(oracle, 2, 2, SHAPES[0], 30 + k, offset0=OFF0) for k in range(3)]
    recs = oracle.verify_packets(streams[1], 2, 512, 2)[1]
    crc = lambda p, c: recs[p]["stream_off"] + recs[p]["header_len"] + 4 * c + 1  # noqa: E731
    streams[1] = flip(streams[1], {"inside a seamed round": crc(0, 5), "skipped head": crc(0, 0),
                                   "behind the read's end": crc(1, 9)}[what])
    reads = [read_of(k, OFF0 + 700, 6000, [100] * 60) for k in range(3)]
    K, F = pv.PATH_KERNEL, pv.PATH_FALLBACK
    got, _, _ = run(pv, engine, oracle, scratch, streams, reads, [K, F, K])
    assert got[1]["rc"] == engine.ERR_BAD_CHECKSUM
    assert got[1]["delivered"] == (5120 - 700 if what == "behind the read's end" else 0)


# ---- 3. the cursor across entries of very different fragment counts -------------------------------------------------
@pytest.fixture(scope="module")
def cursor_case(engine, pv, oracle, scratch):
    """About 500 fragments, then 1, then 40, twice over, placed once with the
    references."""
    streams = [stream_of(oracle, 2, 2, [5120] * 5 + [1300], 40 + k, offset0=OFF0) for k in range(6)]
    n = 5 * 5120 + 1300 - 100 - 9
    lists = [split(n, range(53, n, 53)), [n], split(n, range(659, n, 659))] * 2
    assert len(lists[0]) > 490 and len(lists[2]) == 41
    reads = [read_of(k, OFF0 + 100, n, fl) for k, fl in enumerate(lists)]
    a = Arena(engine, streams, reads)
    want = [reference(engine, oracle, scratch, a, streams, r, 2, 2, 512, 64) for r in reads]
    return streams, reads, a, want


@pytest.mark.parametrize("groups", [1, 3, 1024])
def test_the_fragment_hint_is_reset_between_entries(engine, pv, oracle, scratch, cursor_case, groups):
    """With 1 and 3 workgroups every wave walks from an entry of about 500
    fragments into one of 1 and on into one of 40; a hint kept across them
    would read past a slice."""
    streams, reads, a, want = cursor_case
    a.buf.upload(a.image)
    run(pv, engine, oracle, scratch, streams, reads, [pv.PATH_KERNEL] * len(reads), groups=groups, want=want, arena=a)


# ---- 4. irregular entries among regular ones ------------------------------------------------------------------------
def test_irregular_entries_among_regular_ones(engine, pv, oracle, scratch):
    reg = lambda k: stream_of(oracle, 2, 2, [5120, 5120, 1300], 50 + k, offset0=OFF0)  # noqa: E731
    pay = 2 * 5120 + 1300
    streams = [reg(0),
               reg(1),                                                                    # c_begin >= dlen0
               reg(2),                                                                    # longer than the stream
               stream_of(oracle, 2, 2, [5120] * 3, 53, offset0=OFF0, last_flag=99, last_empty=False)[:-1000],  # cut
               stream_of(oracle, 2, 2, [4096] * 6, 54, offset0=OFF0, last_flag=2),        # a last flag on a body packet
               reg(5), reg(6)]
    fl = lambda n: split(n, range(97, n, 97))  # noqa: E731
    reads = [read_of(0, OFF0 + 10, 7000, fl(7000)),
             read_of(1, OFF0 + 5120, 100, [40, 60]),
             read_of(2, OFF0 + 10, pay, fl(pay)),
             read_of(3, OFF0 + 10, 3 * 5120 - 10, fl(3 * 5120 - 10)),
             read_of(4, OFF0 + 10, 5 * 4096, fl(5 * 4096)),
             read_of(5, -5, 100, [50, 50]),                                               # a negative client_offset
             read_of(6, OFF0 + 5119, 1302, [1, 1300, 1])]
    K, F = pv.PATH_KERNEL, pv.PATH_FALLBACK
    a = Arena(engine, streams, reads)
    want = [None if k == 5 else reference(engine, oracle, scratch, a, streams, r, 2, 2, 512, 64)
            for k, r in enumerate(reads)]
    got = pv.read(a.batch(pv), max_pkts=64)
    assert got[5]["rc"] == EINVAL and (got[5]["consumed"], got[5]["delivered"], got[5]["records"]) == (0, 0, [])
    assert b"entry 5" in pv.load().hdfs_preadv_batch_last_error()
    keep = [k for k in range(len(reads)) if k != 5]
    compare([got[k] for k in keep], [want[k] for k in keep], [K, F, F, F, F, K])
    assert got[5]["path"] == F
    assert [got[k]["rc"] for k in keep] == [0, engine.ERR_UNEXPECTED_READ_OFFSET, engine.ERR_BAD_LASTPACKET, 0,
                                            engine.ERR_BAD_LASTPACKET, 0]
    a.check([None if w is None else w[3] for w in want])


def test_max_pkts_and_chunk_size_4096(engine, pv, oracle, scratch):
    streams = [stream_of(oracle, 2, 2, [5120] * 4, 60 + k, offset0=OFF0) for k in range(3)]
    reads = [read_of(0, OFF0 + 100, 3 * 5120 - 100, [5000, 5000, 5260]), read_of(1, OFF0 + 100, 3 * 5120, [15360]),
             read_of(2, OFF0 + 100, 5120, [5120])]
    K = pv.PATH_KERNEL
    got, _, _ = run(pv, engine, oracle, scratch, streams, reads, [K, pv.PATH_FALLBACK, K], max_pkts=3)
    assert [(g["rc"], len(g["records"]), g["delivered"]) for g in got] == \
        [(0, 3, 3 * 5120 - 100), (0, 3, 3 * 5120 - 100), (0, 2, 5120)]
    streams = [stream_of(oracle, 2, 2, [8192, 5000], 63, cs=4096)]
    run(pv, engine, oracle, scratch, streams, [read_of(0, 100, 9000, [10, 8000, 990])], [pv.PATH_FALLBACK], cs=4096)


def test_fragments_one_byte_short_are_again_and_resume(engine, pv, oracle, scratch):
    """cap = read_len - 1: AGAIN with the resume point, on the fallback path; a
    second call with stream + consumed, client_offset + delivered, read_len -
    delivered and a further fragment completes the read."""
    streams = [stream_of(oracle, 2, 2, [5120] * 4 + [999], 70 + k, offset0=1024) for k in range(3)]
    n = 3 * 5120 + 500
    fl = split(n, [1, 4000, 4001, 9000])
    short = fl[:-1] + [fl[-1] - 1]
    reads = [read_of(0, 1024 + 300, n, fl), read_of(1, 1024 + 300, n, short), read_of(2, 1024 + 300, n, fl)]
    K = pv.PATH_KERNEL
    got, want, a = run(pv, engine, oracle, scratch, streams, reads, [K, pv.PATH_FALLBACK, K])
    g = got[1]
    assert (g["rc"], g["delivered"]) == (AGAIN, n - 1) and 0 < g["consumed"] < len(streams[1])
    whole = oracle.read_packets(streams[1], 1024 + 300, n)[3]
    assert want[1][3] == whole[:n - 1]
    rest = streams[1][g["consumed"]:]
    got2, want2, _ = run(pv, engine, oracle, scratch, [rest], [read_of(0, 1024 + 300 + n - 1, 1, [None, 1])], [K])
    assert got2[0]["rc"] == 0 and want[1][3] + want2[0][3] == whole


def test_entries_without_a_stream_or_without_room_name_no_range(engine, pv, oracle, scratch):
    s = stream_of(oracle, 2, 2, [5120, 1300], 75, offset0=OFF0)
    a = Arena(engine, [s], [read_of(0, OFF0 + 10, 600, [100] * 6)] * 3)
    b = a.batch(pv)
    b[0] = pv.entry(None, 0, [(0x1000, 600)], OFF0 + 10, 600)          # len == 0: its fragments are not looked at
    b[1] = pv.entry(b[1]["stream_ptr"], len(s), [(None, 0), (0x1000, 0)], OFF0 + 10, 600)  # cap == 0
    got = pv.read(b, max_pkts=8)
    assert [g["path"] for g in got] == [pv.PATH_FALLBACK, pv.PATH_FALLBACK, pv.PATH_KERNEL]
    for g, e in zip(got[:2], b[:2]):  # what the main call answers, whatever it is
        rc, recs, used, n = engine.read_packets(e["stream_ptr"], e["nbytes"], None, 0, max_pkts=8,
                                                client_offset=OFF0 + 10, read_len=600, iov=e["frags"])
        assert (g["rc"], fields(g["records"]), g["consumed"], g["delivered"]) == (rc, fields(recs), used, n) and n == 0
    assert (got[2]["rc"], got[2]["delivered"]) == (0, 600)
    a.check([None, None, oracle.read_packets(s, OFF0 + 10, 600)[3]])


# ---- 5. ordering ----------------------------------------------------------------------------------------------------
def test_streams_copied_on_the_null_stream_just_before(engine, pv, oracle):
    """No synchronisation between the device-to-device copies that put the
    streams in place (NULL stream) and the call: the library's stream waits for
    the NULL stream."""
    streams = [stream_of(oracle, 2, 2, [65536] * 6 + [777], 80 + k, offset0=512) for k in range(2)]
    n = 5 * 65536 + 1000
    reads = [read_of(k, 512 + 300, n, split(n, range(1000, n, 1000))) for k in range(2)]
    pay = [oracle.read_packets(s, r["off"], r["n"])[3] for s, r in zip(streams, reads)]
    stage = engine.DeviceBuffer(sum(len(s) for s in streams))
    stage.upload(np.frombuffer(b"".join(streams), dtype=np.uint8))
    a = Arena(engine, [bytes(len(s)) for s in streams], reads)  # zeros where the streams go
    engine.device_sync()
    lib, at = engine.load(), 0
    for k, s in enumerate(streams):
        assert lib.hdfs_crc32c_memcpy(a.buf.ptr + a.src[k], stage.ptr + at, len(s), 2) == 0
        at += len(s)
    got = pv.read(a.batch(pv), max_pkts=40)
    assert [(g["rc"], g["delivered"], g["path"]) for g in got] == [(0, len(p), pv.PATH_KERNEL) for p in pay]
    for k, s in enumerate(streams):
        a.image[a.src[k]:a.src[k] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    a.check(pay)


def test_on_a_stream_of_the_callers(engine, pv, oracle, scratch, cursor_case):
    streams, reads, a, want = cursor_case
    a.buf.upload(a.image)
    st = engine.stream_create()
    try:
        run(pv, engine, oracle, scratch, streams, reads, [pv.PATH_KERNEL] * len(reads), stream=st, want=want, arena=a)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, pv, oracle):
    jobs = []
    for seed, dl, proto in [(90, [5120] * 5 + [900], 2), (91, [8192] * 6, 1)]:
        streams = [stream_of(oracle, proto, 2, dl, seed + 10 * k, offset0=1024) for k in range(3)]
        streams[1] = flip(streams[1], len(streams[1]) // 2)  # one entry of each batch falls back
        n = sum(dl) - 1000
        reads = [read_of(k, 1024 + 77 + k, n, split(n, range(300 + k, n, 300 + k))) for k in range(3)]
        want = [oracle.read_packets(s, r["off"], r["n"], proto, 512, 2) for s, r in zip(streams, reads)]
        jobs.append((Arena(engine, streams, reads, seed=seed), proto, want))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, proto, want = jobs[i]
            start.wait()
            for _ in range(4):
                got = pv.read(a.batch(pv), proto, max_pkts=40)
                compare(got, want, [pv.PATH_KERNEL, pv.PATH_FALLBACK, pv.PATH_KERNEL])
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


# ---- 6. refusals that need the device ----------------------------------------------------------------------------------
def test_refusals_leave_the_arena_untouched_and_name_the_entry_and_fragment(engine, pv, oracle):
    from hadoofus_amd.abi import Packet
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 100 + k) for k in range(4)]
    reads = [read_of(k, 100, 8000, [3000, 0, 5000, None, 24]) for k in range(4)]
    pay = [oracle.read_packets(s, 100, 8000)[3] for s in streams]
    a = Arena(engine, streams, reads)
    lib, p, end = pv.load(), a.buf.ptr, a.buf.ptr + a.buf.nbytes
    host = np.zeros(1 << 16, dtype=np.uint8)
    pk = (Packet * 32)()
    before = bytes(pk)

    def call(n=4, stream=None, frag=None):
        """stream=(entry, ptr); frag=(entry, index, ptr, length or None for its own)."""
        b = a.batch(pv)
        if stream:
            b[stream[0]]["stream_ptr"] = stream[1]
        if frag:
            k, i, ptr, ln = frag
            b[k]["frags"][i] = (ptr, b[k]["frags"][i][1] if ln is None else ln)
        arr, _keep = pv.entries(b)
        for e in arr:
            e.rc, e.npkts, e.consumed, e.delivered = 7, 7, 7, 7
        rc = lib.hdfs_preadv_batch_read(arr, n, 2, 512, 2, pk, 8, None)
        assert [(e.rc, e.npkts, e.consumed, e.delivered) for e in arr][:n] == [(0, 0, 0, 0)] * n or rc == 0
        return rc, lib.hdfs_preadv_batch_last_error().decode()
    f = lambda k, i: p + a.frag[k][i]  # noqa: E731
    # A str is asserted whole, a list as parts.  Of the overlap cases two provoke exactly one overlapping pair: the
    # 24-byte fragment laid over the last byte of fragment 0 of its own entry ends 23 bytes behind it, inside the 40
    # guard bytes there, and the fragment inside stream 1 ends inside it.  The other two provoke two pairs each, of
    # which one is named: 3 000 bytes laid over the last byte of entry 0's fragment 2 reach over the guard bytes into
    # entry 2's own fragment 2, the next range of the shuffled arena, and 5 000 bytes laid over the last byte of
    # stream 1 reach into stream 2.
    cases = {
        "a host stream in entry 3": (dict(stream=(3, host.ctypes.data)), ["entry 3"]),
        "a host fragment in entry 2": (dict(frag=(2, 2, host.ctypes.data, None)), ["entry 2", "fragment 2"]),
        "stream 0 past its allocation": (dict(stream=(0, end - a.lens[0] + 1)), ["entry 0"]),
        "a fragment past its allocation": (dict(frag=(3, 4, end - 23, None)), ["entry 3", "fragment 4"]),
        "a fragment over another entry's": (dict(frag=(2, 0, f(0, 2) + 4999, None)), ["entry 2", "fragment 0",
                                                                                  "fragment 2 of entry 0"]),
        "a fragment over one of its own": (dict(frag=(1, 4, f(1, 0) + 2999, None)),
                                           "entry 1: fragment 4 overlaps fragment 0 of entry 1"),
        "a fragment inside stream 1": (dict(frag=(3, 0, p + a.src[1] + 10, None)),
                                       "entry 3: fragment 0 overlaps the stream of entry 1"),
        "a fragment over its own stream": (dict(frag=(1, 2, p + a.src[1] + a.lens[1] - 1, None)), ["entry 1", "fragment 2",
                                                                                      "stream of entry 1"]),
        "a NULL base with a length": (dict(frag=(2, 3, None, 9)), ["entry 2", "fragment 3", "null base"]),
    }
    for name, (kw, texts) in cases.items():
        rc, err = call(**kw)
        assert rc == EINVAL and (err == texts if isinstance(texts, str) else all(t in err for t in texts)), (name, err)
        assert bytes(pk) == before and not host.any(), name
    a.check([])
    rc, err = call()  # and the same arguments, unspoilt, work
    assert rc == 0
    a.check(pay)


def test_groups_out_of_range_is_einval_and_writes_nothing(engine, pv, oracle):
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 110)]
    a = Arena(engine, streams, [read_of(0, 10, 5000, [2500, 2500])])
    lib, ms = pv.load(), ctypes.c_double(0)
    for flags in (pv.time_groups(pv.MAX_GROUPS + 1), pv.time_groups(1 << 20), 1, pv.time_groups(2) | 4):
        arr, _keep = pv.entries(a.batch(pv))
        assert lib.hdfs_preadv_batch_time(arr, 1, 2, 512, 2, flags, 1, ctypes.byref(ms)) == EINVAL
        assert b"workgroups" in lib.hdfs_preadv_batch_last_error()
        assert (arr[0].rc, arr[0].npkts, arr[0].consumed, arr[0].delivered) == (0, 0, 0, 0)
    a.check([])


# ---- 7. the C consumer --------------------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "preadv_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "preadv_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_preadv_batch", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
