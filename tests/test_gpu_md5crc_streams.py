"""GPU: MD5CRC block digests and the file checksum taken from packet streams in
device memory (include/hadoofus_md5crc_streams.h) -- probe_streams_kernel
frames packet 0 and the tail of every stream, check_headers_kernel compares
every header with the predicted one, digest_streams_kernel runs one MD5 chain
per lane over the packets' CRC regions where they lie; everything else is
framed by hdfs_crc32c_parse_packets inside the call, gathered and digested by
the same kernel.

The expected result of every entry is the CPU oracle's framing walk of the host
copy of its stream and hashlib.md5 over the CRC bytes cut from that copy with
the walk's records.  For whole-block CRC32C streams the digests are also
compared with hdfs_md5crc_block_digests over a compute plan of the payload, so
the check does not rest on one definition alone.  All streams of a batch are
carved from one device allocation between 0xA5 guards, at chosen byte residues
mod 16; after every call the whole allocation is downloaded and compared: the
call writes nothing there.  Everything is bit-exact."""
import ctypes
import hashlib
import os
import subprocess
import threading

import numpy as np
import pytest

from packet_stream import build_stream, header_v2_padded, payload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
GUARD = 0xA5
GAP = 96  # guard bytes before, between and after the streams (at least)
RES = (0, 1, 2, 3, 15)  # address residues mod 16
MD5_EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")
# the selftest's matrix: body packets of one, ten and 128 CRCs; counts that give every total of 1, 13 .. 17 and
# 16 k + {0, 13, 14, 15} with the tails' 0 .. 3 CRCs
BODIES = ((512, (1, 2, 13, 14, 15, 16, 17, 29, 30, 31, 32, 33, 48)), (5120, (1, 2, 3, 8, 16)), (65536, (1, 2, 3)))
RAGGED = (0, 1, 511, 513, 1300)


@pytest.fixture(scope="module")
def ms(engine):
    from hadoofus_read import md5crc_streams
    md5crc_streams.load()
    return md5crc_streams


def stream_of(oracle, proto, ctype, dlens, seed, cs=512, **kw):
    return build_stream(oracle.crc32c, proto, cs, ctype, dlens, seed=seed, **kw)[0]


def expect(oracle, s, proto=2, ctype=2, cs=512):
    """What the call must say of the stream s: the oracle's framing walk, and
    hashlib.md5 over the CRC bytes its records name."""
    rc, recs, used = oracle.verify_packets(s, proto, cs, ctype, verify=False)
    clean = [r for r in recs if not r["error"]]
    crcs = b"".join(s[r["stream_off"] + r["header_len"]:r["stream_off"] + r["header_len"] + r["crc_len"]]
                    for r in clean)
    assert len(crcs) == sum(r["crc_len"] for r in clean)
    return dict(rc=rc, consumed=used, npkts=len(recs), payload=sum(r["data_len"] for r in clean),
                nchunks=0 if rc else len(crcs) // 4, offset_in_block=recs[0]["offset_in_block"] if recs else 0,
                md5=bytes(16) if rc else hashlib.md5(crcs).digest())


class Arena:
    """One device allocation: guards, then every stream at its own residue mod
    16 with guards between.  lens: an entry's length when it is not its stream's
    (a cut packet at the end)."""

    def __init__(self, engine, streams, res=RES):
        self.buf = engine.DeviceBuffer(sum(len(s) + GAP + 32 for s in streams) + GAP + 32)
        assert self.buf.ptr % 16 == 0
        at, self.src = GAP, []
        for k, s in enumerate(streams):
            at = (at + 15) // 16 * 16 + res[k % len(res)]
            self.src.append(at)
            at += len(s) + GAP
        assert at <= self.buf.nbytes
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        for s, o in zip(streams, self.src):
            self.image[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.buf.upload(self.image)
        self.lens = [len(s) for s in streams]

    def batch(self, ms, lens=None):
        return [ms.entry(self.buf.ptr + o if n else None, n) for o, n in zip(self.src, lens or self.lens)]

    def check(self):
        got = self.buf.download()
        if not np.array_equal(got, self.image):
            bad = np.flatnonzero(got != self.image)
            raise AssertionError(f"{bad.size} bytes of the caller's allocation changed, first at {bad[0]}")


def compare(got, want, paths=None):
    keys = ("rc", "consumed", "npkts", "payload", "nchunks", "offset_in_block", "md5")
    for k, (g, w) in enumerate(zip(got, want)):
        assert {f: g[f] for f in keys} == {f: w[f] for f in keys}, (k, g, w)
        if paths is not None and paths[k] is not None:
            assert g["path"] == paths[k], (k, g["path"])
    assert len(got) == len(want)


def run(ms, engine, oracle, streams, proto=2, ctype=2, cs=512, stream=None, paths=None, res=RES):
    a = Arena(engine, streams, res)
    want = [expect(oracle, s, proto, ctype, cs) for s in streams]
    got = ms.block_digests(a.batch(ms), proto, cs, ctype, stream)
    compare(got, want, paths)
    a.check()
    return got, want, a


def plan_digests(engine, payloads, flags=None):
    """hdfs_md5crc_block_digests over a compute plan of the payloads: the chain
    a caller without this library runs.  -> (digests, segments, what they point to)."""
    flags = engine.SEG_BE if flags is None else flags
    keep, segs = [], []
    for p in payloads:
        d = engine.DeviceBuffer(max(16, len(p)))
        d.upload(np.frombuffer(p, dtype=np.uint8))
        c = engine.DeviceBuffer(max(4, (len(p) + 511) // 512 * 4))
        keep += [d, c]
        segs.append(engine.Segment(data=d.ptr, len=len(p), chunk_size=512, flags=flags, crc_init=0, crcs=c.ptr,
                                   bitmap=None))
    engine.Plan(engine.MODE_COMPUTE, segs).execute(None)
    return engine.block_md5crcs(segs), segs, keep


def payload_of(oracle, s, proto=2, ctype=2):
    recs = oracle.verify_packets(s, proto, 512, ctype, verify=False)[1]
    return b"".join(s[r["stream_off"] + r["header_len"] + r["crc_len"]:][:r["data_len"]] for r in recs)


# ---- 1. the shape matrix ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matrix(oracle):
    """{(proto, ctype): [(name, stream, kernel path expected)]}, built once and shared."""
    out = {}
    for proto in (1, 2):
        for ctype in (1, 2):
            rows, seed = [], 1000 * proto + 100 * ctype
            for body, counts in BODIES:
                for K in counts:
                    for ragged in RAGGED:
                        for empty_last in (True, False):
                            dl = [body] * K + ([ragged] if ragged else [])
                            kw = dict(sync_every=1) if (proto == 2 and K % 3 == 2) else {}
                            rows.append((f"{dl[:1]}*{K}+[{ragged}]{'+empty' if empty_last else ''}",
                                         stream_of(oracle, proto, ctype, dl, seed, last_empty=empty_last, **kw),
                                         ragged < body))
                            seed += 1
            out[proto, ctype] = rows
    return out


@pytest.mark.parametrize("ctype", [2, 1])
@pytest.mark.parametrize("proto", [1, 2])
def test_shape_matrix(engine, ms, oracle, matrix, proto, ctype):
    """Body packets of 512, 5 120 and 65 536 bytes; no tail, a shorter packet of
    1, 511, 513 and 1 300 bytes, the empty last packet present and absent, and
    every stream once more with a cut packet at its end (the same bytes, seven
    fewer: streams may overlap); v2 with and without syncBlock; the streams at
    address residues 0, 1, 2, 3 and 15 mod 16.  One call.  A packet behind the
    run that is not shorter than the run's is the main library's to frame: those
    entries, and only those, take the fallback."""
    rows = matrix[proto, ctype]
    streams = [s for _, s, _ in rows]
    a = Arena(engine, streams)
    assert {(a.buf.ptr + o) % 16 for o in a.src} == set(RES)
    lens = a.lens + [n - 7 for n in a.lens]
    batch = a.batch(ms) + a.batch(ms, [n - 7 for n in a.lens])
    assert len(batch) <= ms.MAX_ENTRIES and len(batch) > 400
    want = [expect(oracle, s[:n], proto, ctype) for s, n in zip(streams + streams, lens)]
    got = ms.block_digests(batch, proto, 512, ctype)
    compare(got, want)
    a.check()
    assert all(w["rc"] == 0 for w in want)
    totals = {w["nchunks"] for w in want}
    assert {1, 13, 14, 15, 16, 17, 29, 30, 31, 32} <= totals, sorted(totals)
    whole = got[:len(rows)]
    assert [g["path"] for g in whole] == [ms.PATH_KERNEL if reg else ms.PATH_FALLBACK for _, _, reg in rows]
    assert {g["path"] for g in got[len(rows):]} == {ms.PATH_KERNEL, ms.PATH_FALLBACK}
    assert all(g["consumed"] < n for g, n in zip(got[len(rows):], a.lens))  # the cut packet is not consumed
    if ctype == 2:  # whole blocks from offset 0: the chain a caller runs today gives the same digests
        pick = list(range(0, len(rows), 17))
        want_plan = plan_digests(engine, [payload_of(oracle, streams[k], proto, ctype) for k in pick])[0]
        assert [whole[k]["md5"] for k in pick] == want_plan


# ---- 2. two waves of divergent lengths ------------------------------------------------------------------------
def test_65_entries_of_divergent_lengths(engine, ms, oracle):
    """65 entries are two workgroups of the digest; the trip counts of the lanes
    of one wave differ widely, and one entry has no bytes at all."""
    rng = np.random.default_rng(65)
    streams = []
    for k in range(65):
        body = (512, 5120, 65536, 4096)[k % 4]
        K = int(rng.integers(1, (40, 12, 3, 20)[k % 4] + 1))
        tail = int(rng.integers(0, min(body, 3000)))
        streams.append(stream_of(oracle, 2, 2, [body] * K + ([tail] if tail else []), 2000 + k, last_empty=k % 5 != 0))
    streams[40] = b""
    got, want, _ = run(ms, engine, oracle, streams, paths=[ms.PATH_KERNEL] * 40 + [None] + [ms.PATH_KERNEL] * 24)
    assert (got[40]["rc"], got[40]["nchunks"], got[40]["npkts"], got[40]["md5"]) == (0, 0, 0, MD5_EMPTY)
    assert len({w["nchunks"] for w in want}) > 40


def test_streams_without_a_complete_packet(engine, ms, oracle):
    s = stream_of(oracle, 2, 2, [4096] * 2, 2100)
    streams = [s[:20], s[:5], stream_of(oracle, 2, 2, [], 2101), s]
    got, _, _ = run(ms, engine, oracle, streams)
    assert [(g["rc"], g["nchunks"], g["md5"]) for g in got[:3]] == [(0, 0, MD5_EMPTY)] * 3
    assert [g["npkts"] for g in got] == [0, 0, 1, 3]


# ---- 3. round trips from the write side and after the read side ----------------------------------------------------
@pytest.fixture(scope="module")
def written(engine, ms):
    """Three blocks composed by hadoofus_amd.wire_fused_batch from data in device
    memory, the wire streams at odd addresses of one allocation:
    (that allocation, the streams' batch, lens, wire lens, data)."""
    from hadoofus_amd import wire_fused_batch as fb
    lens = [5 * 65536 + 7 * 512, 5 * 65536 + 7 * 512, 65536 + 2 * 512 + 321]
    data = [payload(300 + k, 0, n) for k, n in enumerate(lens)]
    writes = [fb.write(nbytes=n, offset_in_block=0, seqno=0, finish=True) for n in lens]
    outs, _ = fb.layout(writes)
    wl = [o["wire_len"] for o in outs]
    src = engine.DeviceBuffer(sum(lens))
    src.upload(np.concatenate(data))
    wire = engine.DeviceBuffer(sum(wl) + 4 * 64)
    wire.fill(GUARD)
    at = [sum(wl[:k]) + 64 * k + (1, 3, 15)[k] for k in range(3)]
    fb.compose([fb.write(src.ptr + sum(lens[:k]), lens[k], wire.ptr + at[k], wl[k], 0, 0, True) for k in range(3)])
    engine.device_sync()
    return (wire, src), [ms.entry(wire.ptr + at[k], wl[k]) for k in range(3)], lens, wl, data


def test_round_trip_from_the_fused_batch_write_library(engine, ms, written):
    """The file checksum from the wire streams hdfs_wire_fused_batch_compose wrote
    equals hdfs_md5crc_file_checksum_dev's over a compute plan of the same data:
    neither the oracle nor this library's framing decides."""
    (wire, _src), batch, lens, wl, data = written
    before = wire.download()
    fc, got = ms.file_checksum(batch)
    assert [(g["rc"], g["consumed"], g["payload"], g["nchunks"], g["offset_in_block"], g["path"]) for g in got] == \
        [(0, wl[k], lens[k], (lens[k] + 511) // 512, 0, ms.PATH_KERNEL) for k in range(3)]
    digests, segs, _keep = plan_digests(engine, [d.tobytes() for d in data])
    assert [g["md5"] for g in got] == digests
    ref = engine.file_checksum(segs)
    assert (fc["md5"], fc["crc_per_block"], fc["bytes_per_crc"], fc["ctype"]) == \
        (ref.md5, ref.crc_per_block, ref.bytes_per_crc, ref.ctype)
    assert fc["crc_per_block"] == got[0]["nchunks"] == 5 * 128 + 7
    one, _ = ms.file_checksum(batch[:1])
    assert one["crc_per_block"] == 0 and one["md5"] == hashlib.md5(digests[0]).digest()
    assert np.array_equal(wire.download(), before)


def test_after_a_read_batch_on_the_same_stream(engine, ms, written):
    """hdfs_read_batch_read_blocks verifies the streams on a stream of the
    caller's, then this call digests them on the same stream: nothing between."""
    from hadoofus_read import read_batch as rb
    _bufs, batch, lens, wl, data = written
    back = engine.DeviceBuffer(sum(lens) + 3 * 64)
    at = [sum(lens[:k]) + 64 * k + (1, 0, 5)[k] for k in range(3)]
    st = engine.stream_create()
    try:
        read = rb.read_blocks([rb.entry(batch[k]["stream_ptr"], wl[k], back.ptr + at[k], lens[k]) for k in range(3)],
                              stream=st)
        got = ms.block_digests(batch, stream=st)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0
    assert [(r["rc"], r["delivered"]) for r in read] == [(0, n) for n in lens]
    want = plan_digests(engine, [d.tobytes() for d in data])[0]
    assert [g["md5"] for g in got] == want and [g["payload"] for g in got] == lens


# ---- 4. irregular entries among regular ones ---------------------------------------------------------------------
def _flip(s, at, mask=0x04):
    b = bytearray(s)
    b[at] ^= mask
    return bytes(b)


def test_chunk_size_4096_is_the_main_librarys(engine, ms, oracle):
    streams = [stream_of(oracle, 2, 2, dl, 400 + k, cs=4096) for k, dl in enumerate([[65536] * 2 + [5000], [8192], []])]
    got, _, _ = run(ms, engine, oracle, streams, cs=4096, paths=[ms.PATH_FALLBACK] * 3)
    assert [g["nchunks"] for g in got] == [34, 2, 0]


@pytest.mark.parametrize("proto", [1, 2])
def test_irregular_entries_among_regular_ones(engine, ms, oracle, proto):
    reg = lambda k: stream_of(oracle, proto, 2, [8192] * 6 + [3000], 410 + k)  # noqa: E731
    recs = oracle.verify_packets(reg(3), proto, 512, 2, verify=False)[1]
    seq_at = recs[2]["stream_off"] + (12 + 7 if proto == 1 else 6 + 10)      # a body packet's seqno
    dlen_at = recs[3]["stream_off"] + (24 if proto == 1 else 6 + 21)          # a body packet's dataLen, low byte
    streams = [reg(0),
               stream_of(oracle, proto, 2, [8192, 4096, 8192], 411),          # a size break
               reg(2),
               _flip(reg(3), seq_at),                                         # flagged by the header check
               _flip(reg(3), dlen_at),                                        # framing raises an error there
               stream_of(oracle, proto, 2, [40000] * 3, 415),                 # partial chunks in every packet
               reg(6)]
    K, F = ms.PATH_KERNEL, ms.PATH_FALLBACK
    paths = [K, F, K, F, F, F, K]
    if proto == 2:  # a valid header that is not the canonical encoding, and syncBlock on one packet only
        streams.append(stream_of(oracle, 2, 2, [8192] * 6 + [3000], 417,
                                 header=lambda k, off, seq, last, dl: header_v2_padded(40, off, seq, last, dl)))
        streams.append(stream_of(oracle, 2, 2, [4096] * 6, 418, sync_at=(2,)))
        paths += [F, F]
    got, want, _ = run(ms, engine, oracle, streams, proto, paths=paths)
    assert want[3]["rc"] == 0 and got[3]["md5"] == expect(oracle, reg(3), proto)["md5"]  # the unflipped stream's
    assert got[4]["rc"] == want[4]["rc"] != 0 and got[4]["md5"] == bytes(16) and got[4]["nchunks"] == 0
    assert got[4]["npkts"] == 4 and got[4]["consumed"] == recs[3]["stream_off"] and got[4]["payload"] == 3 * 8192


def test_the_call_returns_the_first_entry_error(engine, ms, oracle):
    reg = stream_of(oracle, 2, 2, [8192] * 6, 420)
    recs = oracle.verify_packets(reg, 2, 512, 2, verify=False)[1]
    bad = _flip(reg, recs[3]["stream_off"] + 6 + 21)
    a = Arena(engine, [reg, bad, reg])
    arr = ms.entries(a.batch(ms))
    rc = ms.load().hdfs_md5crc_streams_block_digests(arr, 3, 2, 512, 2, None)
    assert rc == arr[1].rc == expect(oracle, bad)["rc"] > 0 and arr[0].rc == arr[2].rc == 0
    assert bytes(arr[0].md5) == bytes(arr[2].md5) == expect(oracle, reg)["md5"]


def test_identical_and_overlapping_streams(engine, ms, oracle):
    s = stream_of(oracle, 2, 2, [5120] * 9 + [700], 430)
    a = Arena(engine, [s], res=(3,))
    p, n = a.buf.ptr + a.src[0], len(s)
    first = oracle.verify_packets(s, 2, 512, 2, verify=False)[1][1]["stream_off"]
    got = ms.block_digests([ms.entry(p, n), ms.entry(p, n), ms.entry(p + first, n - first)])
    w = expect(oracle, s)
    compare(got[:2], [w, w], [ms.PATH_KERNEL] * 2)
    compare(got[2:], [expect(oracle, s[first:])], [ms.PATH_KERNEL])
    assert got[2]["offset_in_block"] == 5120 and got[2]["nchunks"] == w["nchunks"] - 10
    a.check()


# ---- 5. ordering ----------------------------------------------------------------------------------------------
def test_streams_copied_on_the_null_stream_just_before(engine, ms, oracle):
    """No synchronisation between the device-to-device copies that put the
    streams in place (NULL stream) and the call: the library's stream waits for
    the NULL stream."""
    streams = [stream_of(oracle, 2, 2, [65536] * 30 + [777], 440 + k) for k in range(2)]
    stage = engine.DeviceBuffer(sum(len(s) for s in streams))
    stage.upload(np.frombuffer(b"".join(streams), dtype=np.uint8))
    a = Arena(engine, [bytes(len(s)) for s in streams])  # zeros where the streams go
    engine.device_sync()
    lib, at = engine.load(), 0
    for k, s in enumerate(streams):
        assert lib.hdfs_crc32c_memcpy(a.buf.ptr + a.src[k], stage.ptr + at, len(s), 2) == 0
        at += len(s)
    got = ms.block_digests(a.batch(ms))
    compare(got, [expect(oracle, s) for s in streams], [ms.PATH_KERNEL] * 2)


def test_on_a_stream_of_the_callers(engine, ms, oracle):
    st = engine.stream_create()
    try:
        streams = [stream_of(oracle, 1, 2, dl, 450 + k, last_empty=False)
                   for k, dl in enumerate([[65536] * 3 + [12345], [4096] * 20, [512], [8192, 4096, 8192]])]
        run(ms, engine, oracle, streams, 1, stream=st, paths=[ms.PATH_KERNEL] * 3 + [ms.PATH_FALLBACK])
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, ms, oracle):
    jobs = []
    for seed, dl, proto in [(460, [65536] * 5 + [900], 2), (461, [5120] * 30, 1)]:
        streams = [stream_of(oracle, proto, 2, dl, seed + 10 * k) for k in range(3)]
        recs = oracle.verify_packets(streams[1], proto, 512, 2, verify=False)[1]
        streams[1] = _flip(streams[1], recs[2]["stream_off"] + (12 + 7 if proto == 1 else 6 + 10))  # one falls back
        jobs.append((Arena(engine, streams), proto, [expect(oracle, s, proto) for s in streams]))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, proto, want = jobs[i]
            start.wait()
            for _ in range(4):
                compare(ms.block_digests(a.batch(ms), proto), want, [ms.PATH_KERNEL, ms.PATH_FALLBACK, ms.PATH_KERNEL])
        except BaseException as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for a, _, _ in jobs:
        a.check()


def test_the_timing_entry(engine, ms, oracle):
    streams = [stream_of(oracle, 2, 2, [65536] * 4 + [100], 470), stream_of(oracle, 2, 2, [40000] * 2, 471)]
    a = Arena(engine, streams)
    t, got = ms.time(a.batch(ms), iters=3)
    assert t > 0
    compare(got, [expect(oracle, s) for s in streams], [ms.PATH_KERNEL, ms.PATH_FALLBACK])
    a.check()


# ---- 6. refusals ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_arena_untouched_and_name_the_entry(engine, ms, oracle):
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 480 + k) for k in range(4)]
    a = Arena(engine, streams)
    lib, end = ms.load(), a.buf.ptr + a.buf.nbytes
    host = np.zeros(1 << 16, dtype=np.uint8)

    def call(n=4, proto=2, cs=512, ctype=2, **kw):
        """kw: {field}{entry}=value, e.g. stream0=..., len3=..."""
        b = a.batch(ms)
        for key, v in kw.items():
            b[int(key[-1])][{"stream": "stream_ptr", "len": "nbytes"}[key[:-1]]] = v
        arr = ms.entries(b) if n <= 4 else (ms.Entry * n)()
        for e in arr:
            e.npkts = e.nchunks = e.consumed = 9
        rc = lib.hdfs_md5crc_streams_block_digests(arr, n, proto, cs, ctype, None)
        return rc, lib.hdfs_md5crc_streams_last_error().decode(), arr
    cases = {
        "a host stream in entry 3": (dict(stream3=host.ctypes.data), "entry 3"),
        "stream 0 past its allocation": (dict(stream0=end - a.lens[0] + 1), "entry 0"),
        "stream 2 longer than its allocation": (dict(len2=a.buf.nbytes), "entry 2"),
        "a null stream with bytes": (dict(stream1=None), "entry 1"),
        "chunk_size 0": (dict(cs=0), "entry 0: chunk_size"),
        "CSUM_NULL": (dict(ctype=0), "entry 0"),
        "ctype 3": (dict(ctype=3), "entry 0"),
        "proto 3": (dict(proto=3), "entry 0: proto"),
        "no entries": (dict(n=0), "no entries"),
        "too many entries": (dict(n=ms.MAX_ENTRIES + 1), "entry 1024"),
    }
    for name, (kw, text) in cases.items():
        rc, err, arr = call(**kw)
        assert rc == EINVAL and text in err, (name, err)
        if kw.get("n", 4) == 4:
            assert [(e.rc, e.npkts, e.nchunks, e.consumed, bytes(e.md5)) for e in arr] == [(0, 0, 0, 0, bytes(16))] * 4
        assert not host.any(), name
    a.check()
    rc, err, arr = call()  # and the same arguments, unspoilt, work
    assert rc == 0 and [e.nchunks for e in arr] == [24] * 4
    a.check()


def test_file_checksum_refusals(engine, ms, oracle):
    """EINVAL with the entries' out fields still filled: an entry with a packet
    error, and a stream that does not start at its block's start."""
    good = stream_of(oracle, 2, 2, [8192] * 4, 490)
    recs = oracle.verify_packets(good, 2, 512, 2, verify=False)[1]
    inside = stream_of(oracle, 2, 2, [8192] * 4, 491, offset0=8192)
    bad = _flip(good, recs[2]["stream_off"] + 6 + 21)
    lib = ms.load()
    for k, (streams, text) in enumerate((([good, inside, good], "entry 1"), ([good, good, bad], "entry 2"))):
        a = Arena(engine, streams)
        arr, fc = ms.entries(a.batch(ms)), ms.FileChecksum()
        rc = lib.hdfs_md5crc_streams_file_checksum(arr, 3, 2, 512, 2, None, ctypes.byref(fc))
        err = lib.hdfs_md5crc_streams_last_error().decode()
        assert rc == EINVAL and text in err, err
        want = [expect(oracle, s) for s in streams]
        assert [(e.rc, e.nchunks, e.offset_in_block, bytes(e.md5)) for e in arr] == \
            [(w["rc"], w["nchunks"], w["offset_in_block"], w["md5"]) for w in want]
        assert bytes(fc.md5) == bytes(16)
        with pytest.raises(ms.abi.CRC32CError):
            ms.file_checksum(a.batch(ms))
    a = Arena(engine, [good, good])
    arr = ms.entries(a.batch(ms))
    assert lib.hdfs_md5crc_streams_file_checksum(arr, 2, 2, 512, 2, None, None) == EINVAL
    fc, got = ms.file_checksum(a.batch(ms), ctype=1)  # the ctype is the caller's word: the CRCs are not verified
    assert fc["ctype"] == 1 and fc["crc_per_block"] == 64 and fc["md5"] == hashlib.md5(got[0]["md5"] * 2).digest()


# ---- 7. the C caller ----------------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "md5crc_streams_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "md5crc_streams_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_md5crc_streams", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    crcs = [bytes.fromhex(l.split()[1]) for l in lines if l.startswith("crcs ")]
    blocks = [bytes.fromhex(l.split()[1]) for l in lines if l.startswith("block ")]
    assert len(crcs) == 3 and blocks == [hashlib.md5(c).digest() for c in crcs]
    cpb, md5 = [l for l in lines if l.startswith("file ")][0][5:].split(":")
    assert int(cpb) == len(crcs[0]) // 4 and bytes.fromhex(md5.strip()) == hashlib.md5(b"".join(blocks)).digest()
