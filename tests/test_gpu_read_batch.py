"""GPU: a batch of block reads in one call (include/hadoofus_read_batch.h) --
probe_kernel frames packet 0 and the tail of every stream,
unframe_fused_batch_kernel walks the packets of the regular entries, copies
the data, computes the chunk CRCs from the registers it copies and compares
them and every header with the stream's; everything else goes to
hdfs_crc32c_read_packets inside the call.

The expected result of every entry is the CPU oracle's verify_packets of its
stream plus the concatenated payloads before the first error, and also the
main library's read_packets of the same device bytes into a buffer of its own.
All streams and all destinations of a batch are carved from one device
allocation between 0xA5 guards, at chosen byte residues mod 16; after every
call the whole allocation is downloaded and compared with the image expected
(a destination's bytes past `delivered` are unspecified and not compared), so
the streams and the guards are untouched.  Everything is bit-exact."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from packet_stream import build_stream, header_v2, payload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
GUARD = 0xA5
GAP = 96  # guard bytes before, between and after the ranges (at least)
SLACK = 16  # room of a destination beyond its payload
FIELDS = ("stream_off", "offset_in_block", "seqno", "data_len", "crc_len", "header_len", "error", "first_bad",
          "bad_chunks", "last", "sync")
SRES, DRES = (0, 1, 3, 7), (0, 5, 15)


@pytest.fixture(scope="module")
def rb(engine):
    from hadoofus_read import read_batch
    read_batch.load()
    return read_batch


@pytest.fixture(scope="module")
def scratch(engine):
    """The destination of the main library's reference reads."""
    return engine.DeviceBuffer(12 << 20)


def _payloads(s, pkts):
    out = bytearray()
    for p in pkts:
        if p["error"]:
            break
        a = p["stream_off"] + p["header_len"] + p["crc_len"]
        out += s[a:a + p["data_len"]]
    return bytes(out)


def fields(recs):
    return [tuple(r[f] for f in FIELDS) for r in recs]


def stream_of(oracle, proto, ctype, dlens, seed, cs=512, **kw):
    return build_stream(oracle.crc32c, proto, cs, ctype, dlens, seed=seed, **kw)[0]


class Arena:
    """One device allocation: guards, then every stream and every destination,
    each at its own residue mod 16 with guards between."""

    def __init__(self, engine, streams, caps):
        self.buf = engine.DeviceBuffer(sum(n + GAP + 32 for n in [len(s) for s in streams] + list(caps)) + GAP + 32)
        assert self.buf.ptr % 16 == 0
        at, self.src, self.dst, self.caps = GAP, [], [], list(caps)
        for k, s in enumerate(streams):
            at = (at + 15) // 16 * 16 + SRES[k % len(SRES)]
            self.src.append(at)
            at += len(s) + GAP
        for k, n in enumerate(caps):
            at = (at + 15) // 16 * 16 + DRES[k % len(DRES)]
            self.dst.append(at)
            at += n + GAP
        assert at <= self.buf.nbytes
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        for s, o in zip(streams, self.src):
            self.image[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.buf.upload(self.image)
        self.lens = [len(s) for s in streams]

    def batch(self, rb, caps=None):
        p = self.buf.ptr
        caps = caps or self.caps
        return [rb.entry(p + self.src[k], self.lens[k], p + self.dst[k], caps[k]) for k in range(len(self.src))]

    def check(self, payloads):
        """The whole allocation: payload k at destination k (its room behind the
        payload is unspecified), nothing else changed.  payloads: None = untouched."""
        want, got = self.image.copy(), self.buf.download()
        for o, cap, pl in zip(self.dst, self.caps, payloads or []):
            if pl is None:
                continue
            want[o:o + len(pl)] = np.frombuffer(pl, dtype=np.uint8)
            got[o + len(pl):o + cap] = GUARD
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (streams {self.src[:8]}, destinations "
                                 f"{self.dst[:8]}): got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def reference(engine, oracle, scratch, arena, k, s, proto, ctype, cs, max_pkts, cap):
    """Entry k's expected (rc, records, consumed, payload): the oracle's, which
    the main library's read of the same device bytes must give too."""
    rc, recs, used = oracle.verify_packets(s, proto, cs, ctype, max_pkts)
    pl = _payloads(s, recs)
    erc, erecs, eused, egot = engine.read_packets(arena.buf.ptr + arena.src[k], len(s), scratch.ptr, cap, proto, cs,
                                                  ctype, max_pkts)
    assert (erc, fields(erecs), eused, egot) == (rc, fields(recs), used, len(pl)), k
    assert scratch.download(egot).tobytes() == pl, k
    return rc, recs, used, pl


def run(rb, engine, oracle, scratch, streams, proto=2, ctype=2, cs=512, max_pkts=None, groups=None, stream=None,
        paths=None, records=True):
    """Places the streams, reads the batch (groups: through the timing entry with
    that many workgroups, so without records) and checks every entry against
    its reference, and the whole arena.  -> the results."""
    full = [oracle.verify_packets(s, proto, cs, ctype)[1] for s in streams]
    # READ_ALL wants room for the framed payload, the packets with bad CRCs included
    caps = [sum(p["data_len"] for p in r if p["error"] in (0, engine.ERR_BAD_CHECKSUM)) + SLACK for r in full]
    a = Arena(engine, streams, caps)
    mp = max(len(r) for r in full) + 2 if max_pkts is None else max_pkts
    want = [reference(engine, oracle, scratch, a, k, s, proto, ctype, cs, mp, caps[k]) for k, s in enumerate(streams)]
    if groups is None:
        got = rb.read_blocks(a.batch(rb), proto, cs, ctype, mp if records else None, stream)
    else:
        ms, got = rb.time(a.batch(rb), proto, cs, ctype, rb.time_groups(groups), 1)
        assert ms > 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["rc"], g["consumed"], g["delivered"]) == (w[0], w[2], len(w[3])), (k, g, w[:3])
        if g["records"] is not None:
            assert fields(g["records"]) == fields(w[1]), k
        if paths is not None and paths[k] is not None:
            assert g["path"] == paths[k], (k, g["path"])
    a.check([w[3] for w in want])
    return got


# ---- 1. regular batches -------------------------------------------------------------------------------
SHAPES = [[65536] * 3 + [12345], [4096] * 20, [512], [65536] * 2, [65536, 700], []]


def regular_streams(oracle, proto, ctype):
    out = []
    for k, dl in enumerate(SHAPES):
        out.append(stream_of(oracle, proto, ctype, dl, 10 + k, last_empty=dl != [65536] * 2))
    if proto == 2:
        out.append(stream_of(oracle, proto, ctype, [8192] * 5 + [100], 20, sync_every=1))
        out.append(stream_of(oracle, proto, ctype, [8192] * 5 + [100], 21,  # and on the empty last packet too, unset there
                             header=lambda k, off, seq, last, dl: header_v2(off, seq, last, dl, dl != 0)))
    else:
        out.append(stream_of(oracle, proto, ctype, [8192] * 5 + [100], 20, last_empty=False))
    return out


@pytest.mark.parametrize("ctype", [2, 1])
@pytest.mark.parametrize("proto", [1, 2])
def test_regular_batch_takes_the_kernel_path(engine, rb, oracle, scratch, proto, ctype):
    """Six shapes at stream residues 0, 1, 3, 7 and destination residues 0, 5,
    15, plus syncBlock on every data packet and on every packet, the empty last one
    included (v2), or the last flag on the final data packet without a trailing
    one (v1): every entry with a data packet is served by the kernel."""
    streams = regular_streams(oracle, proto, ctype)
    paths = [rb.PATH_KERNEL if dl else None for dl in SHAPES] + [rb.PATH_KERNEL] * (len(streams) - len(SHAPES))
    got = run(rb, engine, oracle, scratch, streams, proto, ctype, paths=paths)
    assert [len(g["records"]) for g in got[:6]] == [5, 21, 2, 2, 3, 1]
    # and the same batch without records
    run(rb, engine, oracle, scratch, streams, proto, ctype, paths=paths, records=False)


# ---- 2. packet tails of every kind -----------------------------------------------------------------------
@pytest.mark.parametrize("proto", [1, 2])
def test_every_tail_of_the_last_packet(engine, rb, oracle, scratch, proto):
    """A full packet, then a last packet of 1, 7, 8, 9 and 127 full chunks, each
    with a partial chunk of 0, 1, 15, 16, 17 and 511 bytes: the write side's
    ragged matrix, one batch of thirty entries."""
    tails = [512 * f + p for f in (1, 7, 8, 9, 127) for p in (0, 1, 15, 16, 17, 511)]
    streams = [stream_of(oracle, proto, 2, [65536, t], 30 + k) for k, t in enumerate(tails)]
    run(rb, engine, oracle, scratch, streams, proto, 2, paths=[rb.PATH_KERNEL] * len(tails))


# ---- 3. corruption in one entry of five ---------------------------------------------------------------------
def _flip(s, at, mask=0x04):
    b = bytearray(s)
    b[at] ^= mask
    return bytes(b)


@pytest.mark.parametrize("what", ["full chunk", "ragged chunk", "crc byte", "seqno of a middle header",
                                  "plen of a middle packet"])
@pytest.mark.parametrize("proto", [1, 2])
def test_one_corrupt_entry_of_five_falls_back_alone(engine, rb, oracle, scratch, proto, what):
    streams = [stream_of(oracle, proto, 2, [65536] * 3 + [12345], 40 + k) for k in range(5)]
    recs = oracle.verify_packets(streams[2], proto, 512, 2)[1]
    at = lambda i: recs[i]["stream_off"]  # noqa: E731
    data = lambda i: at(i) + recs[i]["header_len"] + recs[i]["crc_len"]  # noqa: E731
    where = {"full chunk": data(1) + 5 * 512 + 77, "ragged chunk": data(3) + 24 * 512 + 30,
             "crc byte": at(2) + recs[2]["header_len"] + 4 * 9 + 2,
             "seqno of a middle header": at(1) + (12 + 7 if proto == 1 else 6 + 10),
             "plen of a middle packet": at(1) + 3}[what]
    streams[2] = _flip(streams[2], where)
    paths = [rb.PATH_KERNEL] * 5
    paths[2] = rb.PATH_FALLBACK
    got = run(rb, engine, oracle, scratch, streams, proto, 2, paths=paths)
    bad = got[2]
    if what == "full chunk":
        assert bad["rc"] == engine.ERR_BAD_CHECKSUM and bad["delivered"] == 65536
        assert [(r["first_bad"], r["bad_chunks"]) for r in bad["records"] if r["error"]] == [(5, 1)]
    elif what == "ragged chunk":
        assert bad["rc"] == engine.ERR_BAD_CHECKSUM and bad["delivered"] == 3 * 65536
        assert [(r["first_bad"], r["bad_chunks"]) for r in bad["records"] if r["error"]] == [(24, 1)]
    elif what == "crc byte":
        assert bad["rc"] == engine.ERR_BAD_CHECKSUM and bad["delivered"] == 2 * 65536
        assert [(r["first_bad"], r["bad_chunks"]) for r in bad["records"] if r["error"]] == [(9, 1)]
    elif what == "seqno of a middle header":
        assert bad["rc"] == 0 and bad["records"][1]["seqno"] != 1 and bad["delivered"] == 3 * 65536 + 12345
    else:
        assert bad["rc"] == engine.ERR_CRC_LEN and len(bad["records"]) == 2 and bad["delivered"] == 65536


# ---- 4. irregular entries among regular ones -----------------------------------------------------------------
def test_irregular_entries_among_regular_ones(engine, rb, oracle, scratch):
    reg = lambda k: stream_of(oracle, 2, 2, [65536] * 2 + [3000], 50 + k)  # noqa: E731
    streams = [reg(0),
               stream_of(oracle, 2, 2, [65536, 4096, 65536], 51),              # a size break
               reg(2),
               stream_of(oracle, 2, 2, [4096] * 6, 53, sync_at=(2,)),         # syncBlock on one packet
               stream_of(oracle, 2, 2, [40000] * 5, 54),                      # partial chunks in every packet
               stream_of(oracle, 2, 2, [65536] * 3, 55, last_empty=False)[:-1000],  # cut inside a packet
               stream_of(oracle, 2, 2, [65536] * 3 + [5000], 56)[:-40],       # cut inside the empty packet's header
               reg(7)]
    K, F = rb.PATH_KERNEL, rb.PATH_FALLBACK
    got = run(rb, engine, oracle, scratch, streams, paths=[K, F, K, F, F, None, None, K])
    assert got[5]["consumed"] == 2 * (65536 + 512 + 31) and len(got[5]["records"]) == 2


def test_chunk_size_4096_is_the_main_librarys(engine, rb, oracle, scratch):
    streams = [stream_of(oracle, 2, 2, dl, 60 + k, cs=4096) for k, dl in enumerate([[65536] * 2 + [5000], [8192]])]
    run(rb, engine, oracle, scratch, streams, cs=4096, paths=[rb.PATH_FALLBACK] * 2)


# ---- 5. limits --------------------------------------------------------------------------------------------
def test_a_destination_one_byte_short(engine, rb, oracle, scratch):
    """That entry's rc is the main call's EINVAL for it and nothing is written
    past the cap; the others are served."""
    streams = [stream_of(oracle, 2, 2, [65536, 65536, 999], 70 + k) for k in range(3)]
    pay = [_payloads(s, oracle.verify_packets(s)[1]) for s in streams]
    caps = [len(p) + SLACK for p in pay]
    caps[1] = len(pay[1]) - 1
    a = Arena(engine, streams, caps)
    with pytest.raises(engine.CRC32CError) as e:  # what hdfs_crc32c_read_packets returns for it
        engine.read_packets(a.buf.ptr + a.src[1], len(streams[1]), scratch.ptr, caps[1], max_pkts=8)
    assert e.value.code == EINVAL
    got = rb.read_blocks(a.batch(rb), max_pkts=8)
    assert [g["rc"] for g in got] == [0, EINVAL, 0] and got[1]["path"] == rb.PATH_FALLBACK
    assert (got[1]["consumed"], got[1]["delivered"], got[1]["records"]) == (0, 0, [])
    assert b"entry 1" in rb.load().hdfs_read_batch_last_error()
    assert [g["path"] for g in got[::2]] == [rb.PATH_KERNEL] * 2 and [len(g["records"]) for g in got[::2]] == [4, 4]
    a.check([pay[0], b"", pay[2]])  # entry 1's room is unspecified, the guards behind it are not


def test_max_pkts_one_short_cuts_the_run(engine, rb, oracle, scratch):
    streams = [stream_of(oracle, 2, 2, [65536] * 3, 80), stream_of(oracle, 2, 2, [65536] * 4, 81),
               stream_of(oracle, 2, 2, [4096] * 2, 82)]
    got = run(rb, engine, oracle, scratch, streams, max_pkts=4, paths=[rb.PATH_KERNEL, rb.PATH_FALLBACK, rb.PATH_KERNEL])
    assert [len(g["records"]) for g in got] == [4, 4, 3]


# ---- 6. many packets per workgroup ------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3, 7])
def test_few_workgroups_walk_many_packets(engine, rb, oracle, scratch, groups):
    streams = regular_streams(oracle, 2, 2)[:6] + [stream_of(oracle, 2, 2, [65536] * 40, 90)]
    run(rb, engine, oracle, scratch, streams, groups=groups, paths=[rb.PATH_KERNEL] * 5 + [None, rb.PATH_KERNEL])


def test_groups_out_of_range_is_einval_and_writes_nothing(engine, rb, oracle):
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 91)]
    a = Arena(engine, streams, [3 * 4096 + SLACK])
    lib, ms = rb.load(), ctypes.c_double(0)
    for flags in (rb.time_groups(rb.MAX_GROUPS + 1), rb.time_groups(1 << 20), 1, rb.time_groups(2) | 4):
        assert lib.hdfs_read_batch_time(rb.entries(a.batch(rb)), 1, 2, 512, 2, flags, 1, ctypes.byref(ms)) == EINVAL
        assert b"workgroups" in lib.hdfs_read_batch_last_error()
    a.check([])
    ms, got = rb.time(a.batch(rb), flags=rb.time_groups(rb.MAX_GROUPS), iters=1)
    assert ms > 0 and got[0]["path"] == rb.PATH_KERNEL
    a.check([_payloads(streams[0], oracle.verify_packets(streams[0])[1])])


# ---- 7. round trip from the write side ----------------------------------------------------------------------------
def test_round_trip_from_the_fused_batch_write_library(engine, rb):
    """Four writes composed by hadoofus_amd.wire_fused_batch, one of them 9 MiB
    + 321 B at an odd address, read back by one call and compared byte for byte
    with the source: neither this library's CRC code nor the oracle decides."""
    from hadoofus_amd import wire_fused_batch as fb
    lens = [65536, (9 << 20) + 321, 3 * 65536 + 17, 512]
    data = [payload(95 + k, 0, n) for k, n in enumerate(lens)]
    writes = [fb.write(nbytes=n, offset_in_block=0, seqno=3 * k, finish=True) for k, n in enumerate(lens)]
    outs, _ = fb.layout(writes)
    wl = [o["wire_len"] for o in outs]
    src = Arena(engine, [d.tobytes() for d in data], wl)  # the writes' sources, then their wire streams
    p = src.buf.ptr
    assert lens[1] > 9 << 20 and (p + src.src[1]) % 2 == 1 and (p + src.dst[1]) % 2 == 1
    fb.compose([fb.write(p + src.src[k], lens[k], p + src.dst[k], wl[k], 0, 3 * k, True) for k in range(4)])
    back = engine.DeviceBuffer(sum(lens) + 4 * 64)
    at = [sum(lens[:k]) + 64 * k + (1, 0, 5, 15)[k] for k in range(4)]
    got = rb.read_blocks([rb.entry(p + src.dst[k], wl[k], back.ptr + at[k], lens[k]) for k in range(4)], max_pkts=160)
    assert [(g["rc"], g["consumed"], g["delivered"], g["path"]) for g in got] == \
        [(0, wl[k], lens[k], rb.PATH_KERNEL) for k in range(4)]
    assert [len(g["records"]) for g in got] == [o["npkts"] for o in outs]
    img = back.download()
    for k in range(4):
        assert np.array_equal(img[at[k]:at[k] + lens[k]], data[k]), k


# ---- 8. other behaviour ---------------------------------------------------------------------------------------------
def test_streams_copied_on_the_null_stream_just_before(engine, rb, oracle):
    """No synchronisation between the device-to-device copies that put the
    streams in place (NULL stream) and the call: the library's stream waits for
    the NULL stream."""
    streams = [stream_of(oracle, 2, 2, [65536] * 30 + [777], 100 + k) for k in range(2)]
    pay = [_payloads(s, oracle.verify_packets(s)[1]) for s in streams]
    stage = engine.DeviceBuffer(sum(len(s) for s in streams))
    stage.upload(np.frombuffer(b"".join(streams), dtype=np.uint8))
    a = Arena(engine, [bytes(len(s)) for s in streams], [len(p) + SLACK for p in pay])  # zeros where the streams go
    engine.device_sync()
    lib, at = engine.load(), 0
    for k, s in enumerate(streams):
        assert lib.hdfs_crc32c_memcpy(a.buf.ptr + a.src[k], stage.ptr + at, len(s), 2) == 0
        at += len(s)
    got = rb.read_blocks(a.batch(rb), max_pkts=40)
    assert [(g["rc"], g["delivered"], g["path"]) for g in got] == [(0, len(p), rb.PATH_KERNEL) for p in pay]
    for k, s in enumerate(streams):
        a.image[a.src[k]:a.src[k] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    a.check(pay)


def test_on_a_stream_of_the_callers(engine, rb, oracle, scratch):
    st = engine.stream_create()
    try:
        run(rb, engine, oracle, scratch, regular_streams(oracle, 1, 2), 1, 2, stream=st)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, rb, oracle):
    jobs = []
    for seed, dl, proto in [(110, [65536] * 5 + [900], 2), (111, [8192] * 30, 1)]:
        streams = [stream_of(oracle, proto, 2, dl, seed + 10 * k) for k in range(3)]
        streams[1] = _flip(streams[1], len(streams[1]) // 2)  # one entry of each batch falls back
        want = [oracle.verify_packets(s, proto, 512, 2) for s in streams]
        pay = [_payloads(s, w[1]) for s, w in zip(streams, want)]
        a = Arena(engine, streams, [sum(dl) + SLACK] * 3)
        jobs.append((a, proto, want, pay))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, proto, want, pay = jobs[i]
            start.wait()
            for _ in range(4):
                got = rb.read_blocks(a.batch(rb), proto, max_pkts=40)
                assert [(g["rc"], fields(g["records"]), g["consumed"], g["delivered"]) for g in got] == \
                    [(w[0], fields(w[1]), w[2], len(p)) for w, p in zip(want, pay)]
        except BaseException as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for a, _, _, pay in jobs:
        a.check(pay)


def test_refusals_leave_the_arena_untouched_and_name_the_entry(engine, rb, oracle):
    from hadoofus_amd.abi import Packet
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 120 + k) for k in range(4)]
    pay = [_payloads(s, oracle.verify_packets(s)[1]) for s in streams]
    a = Arena(engine, streams, [len(p) + SLACK for p in pay])
    lib, p, end = rb.load(), a.buf.ptr, a.buf.ptr + a.buf.nbytes
    host = np.zeros(1 << 16, dtype=np.uint8)
    pk = (Packet * 32)()
    before = bytes(pk)

    def call(n=4, proto=2, cs=512, ctype=2, **kw):
        """kw: {field}{entry}=value, e.g. dst2=..., stream0=..., len3=..."""
        b = a.batch(rb)
        for key, v in kw.items():
            b[int(key[-1])][{"stream": "stream_ptr", "len": "nbytes", "dst": "dst_ptr", "cap": "dst_cap"}[key[:-1]]] = v
        arr = rb.entries(b) if n <= 4 else (rb.Entry * n)()
        rc = lib.hdfs_read_batch_read_blocks(arr, n, proto, cs, ctype, pk, 8, None)
        return rc, lib.hdfs_read_batch_last_error().decode()
    # (kw, text, exact): exact texts are asserted whole, the others as a part.  Of the overlap cases "inside stream 1"
    # provokes exactly one overlapping pair.  The other two provoke two each, of which one is named: a range of this
    # size laid over the last byte of dst 0 reaches over the guard bytes into dst 1 as well, and one laid back from
    # the first byte of stream 1 reaches into stream 0 as well.
    cases = {
        "a host stream in entry 3": (dict(stream3=host.ctypes.data), "entry 3", False),
        "a host destination in entry 2": (dict(dst2=host.ctypes.data), "entry 2", False),
        "stream 0 past its allocation": (dict(stream0=end - a.lens[0] + 1), "entry 0", False),
        "destination 3 past its allocation": (dict(dst3=end - a.caps[3] + 1), "entry 3", False),
        "destination 2 overlaps destination 0": (dict(dst2=p + a.dst[0] + a.caps[0] - 1), "entry 2", False),
        "destination 3 inside stream 1": (dict(dst3=p + a.src[1] + 10), "entry 3: dst overlaps the stream of entry 1", True),
        "destination 1 overlaps its own stream": (dict(dst1=p + a.src[1] - a.caps[1] + 1), "entry 1", False),
        "chunk_size 0": (dict(cs=0), "chunk_size", False),
        "CSUM_NULL": (dict(ctype=0), "CRC32", False),
        "proto 3": (dict(proto=3), "proto", False),
        "no entries": (dict(n=0), "no entries", False),
        "too many entries": (dict(n=rb.MAX_ENTRIES + 1), "1024", False),
    }
    for name, (kw, text, exact) in cases.items():
        rc, err = call(**kw)
        assert rc == EINVAL and (err == text if exact else text in err), (name, err)
        assert bytes(pk) == before and not host.any(), name
    a.check([])
    rc, err = call()  # and the same arguments, unspoilt, work
    assert rc == 0
    a.check(pay)


def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "read_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "read_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_read_batch", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr


# ---- a batch at the limit ---------------------------------------------------------------------------------------------
def test_a_batch_at_the_limit_is_swept_and_refused_by_name(engine, rb, oracle):
    """1 024 entries of one 512-byte packet and the empty last packet in one
    arena, the destinations in falling address order, so the overlap sweep
    has to sort; then one destination at a time is moved onto another range."""
    n, cap = rb.MAX_ENTRIES, 512 + SLACK
    kinds = [stream_of(oracle, 2, 2, [512], 300 + k) for k in range(8)]  # entry k reads kinds[k % 8]
    pays = [_payloads(s, oracle.verify_packets(s)[1]) for s in kinds]
    slen = len(kinds[0])
    assert n == 1024 and all(len(s) == slen for s in kinds) and all(len(p) == 512 for p in pays)
    spitch, dpitch = (slen + 16 + 15) // 16 * 16, cap + 16  # 16 guard bytes at least behind every range
    src = [GAP + k * spitch for k in range(n)]
    d0 = GAP + n * spitch + GAP
    dst = [d0 + (n - 1 - k) * dpitch for k in range(n)]  # entry 0's is the highest
    buf = engine.DeviceBuffer(d0 + n * dpitch + GAP)
    image = np.full(buf.nbytes, GUARD, dtype=np.uint8)
    for k in range(n):
        image[src[k]:src[k] + slen] = np.frombuffer(kinds[k % 8], dtype=np.uint8)
    buf.upload(image)
    p = buf.ptr

    def batch(**moved):
        return [rb.entry(p + src[k], slen, p + moved.get(f"dst{k}", dst[k]), cap) for k in range(n)]
    got = rb.read_blocks(batch(), 2, 512, 2, None, None)
    assert [(g["rc"], g["consumed"], g["delivered"]) for g in got] == [(0, slen, 512)] * n
    after = buf.download()
    for k in range(n):
        assert after[dst[k]:dst[k] + 512].tobytes() == pays[k % 8], k
        after[dst[k] + 512:dst[k] + cap] = GUARD  # a destination's room behind its payload is unspecified
        image[dst[k]:dst[k] + 512] = np.frombuffer(pays[k % 8], dtype=np.uint8)
    assert np.array_equal(after, image)
    # Where the moved destination overlaps nothing else.  8 bytes into entry 0's destination, the highest range of
    # the arena: it ends 8 bytes into the 16 guard bytes behind that, ahead of the arena's last GAP bytes.  8 bytes
    # into a stream: cap + 8 <= slen, so it ends inside that stream.  Its own place stays empty.
    assert cap + 8 <= slen and dst[0] + 8 + cap <= buf.nbytes
    lib = rb.load()
    held = buf.download()
    for moved, text in ((dict(dst1023=dst[0] + 8), "entry 1023: dst overlaps the dst of entry 0"),
                        (dict(dst5=src[900] + 8), "entry 5: dst overlaps the stream of entry 900"),
                        (dict(dst7=src[7] + 8), "entry 7: dst overlaps the stream of entry 7")):
        rc = lib.hdfs_read_batch_read_blocks(rb.entries(batch(**moved)), n, 2, 512, 2, None, 0, None)
        assert rc == EINVAL and lib.hdfs_read_batch_last_error().decode() == text, text
        assert np.array_equal(buf.download(), held), text
