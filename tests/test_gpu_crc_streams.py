"""GPU: composite CRCs of blocks and files taken from packet streams in device
memory (include/hadoofus_crc_streams.h) -- probe_streams_kernel frames packet
0 and the tail of every stream, fold_packets_kernel compares every header with
the predicted one and folds the CRC region behind it into the packet's CRC,
reduce_entries_kernel reduces every entry's packets with one wave; everything
else is framed by hdfs_crc32c_parse_packets inside the call and folded and
reduced by the same two kernels.

The expected result of every entry is the CPU oracle's framing walk of the host
copy of its stream and the oracle's CRC32C (zlib.crc32 for CRC32) of the payload
bytes cut from that copy with the walk's records; never a value of the library
under test.  Streams written on the device are compared with
hdfs_crc32c_composite_crcs over a compute plan and with hdfs_crc32c_stream_ex.
All streams of a batch are carved from one device allocation between 0xA5
guards, at chosen byte residues mod 16; after every call the whole allocation
is downloaded and compared: the call writes nothing there.  Everything is
bit-exact."""
import ctypes
import os
import subprocess
import threading
import zlib

import numpy as np
import pytest

from packet_stream import build_stream, header_v2_padded, payload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
GUARD = 0xA5
GAP = 96  # guard bytes before, between and after the streams (at least)
RES = (0, 1, 2, 3, 15)  # address residues mod 16
# the selftest's matrix: every packet count is a run boundary of the reduce (64 lanes) for every body size, but 129
# packets of 65 536 bytes (84 MB a protocol and checksum type for nothing the 128 MiB block below does not reach)
BODIES = ((512, (1, 2, 63, 64, 65, 129)), (5120, (1, 2, 63, 64, 65, 129)), (65536, (1, 2, 63, 64, 65)))
RAGGED = (0, 1, 511, 513, 1300)


@pytest.fixture(scope="module")
def cs(engine):
    from hadoofus_read import crc_streams
    crc_streams.load()
    return crc_streams


def stream_of(oracle, proto, ctype, dlens, seed, chunk=512, **kw):
    return build_stream(oracle.crc32c, proto, chunk, ctype, dlens, seed=seed, **kw)[0]


def crc_of(oracle, ctype, data):
    return zlib.crc32(data) if ctype == 1 else oracle.crc32c(0, data)


def expect(oracle, s, proto=2, ctype=2, chunk=512):
    """What the call must say of the stream s: the oracle's framing walk, and
    the CRC of the payload bytes its records name."""
    rc, recs, used = oracle.verify_packets(s, proto, chunk, ctype, verify=False)
    clean = [r for r in recs if not r["error"]]
    data = b"".join(s[r["stream_off"] + r["header_len"] + r["crc_len"]:][:r["data_len"]] for r in clean)
    assert len(data) == sum(r["data_len"] for r in clean)
    return dict(rc=rc, consumed=used, npkts=len(recs), payload=len(data),
                nchunks=0 if rc else sum(r["crc_len"] for r in clean) // 4,
                offset_in_block=recs[0]["offset_in_block"] if recs else 0,
                crc=0 if rc else crc_of(oracle, ctype, data))


class Arena:
    """One device allocation: guards, then every stream at its own residue mod
    16 with guards between."""

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

    def batch(self, cs, lens=None):
        return [cs.entry(self.buf.ptr + o if n else None, n) for o, n in zip(self.src, lens or self.lens)]

    def check(self):
        got = self.buf.download()
        if not np.array_equal(got, self.image):
            bad = np.flatnonzero(got != self.image)
            raise AssertionError(f"{bad.size} bytes of the caller's allocation changed, first at {bad[0]}")


def compare(got, want, paths=None):
    keys = ("rc", "consumed", "npkts", "payload", "nchunks", "offset_in_block", "crc")
    for k, (g, w) in enumerate(zip(got, want)):
        assert {f: g[f] for f in keys} == {f: w[f] for f in keys}, (k, g, w)
        if paths is not None and paths[k] is not None:
            assert g["path"] == paths[k], (k, g["path"])
    assert len(got) == len(want)


def run(cs, engine, oracle, streams, proto=2, ctype=2, chunk=512, stream=None, paths=None, res=RES):
    a = Arena(engine, streams, res)
    want = [expect(oracle, s, proto, ctype, chunk) for s in streams]
    got = cs.block_crcs(a.batch(cs), proto, chunk, ctype, stream)
    compare(got, want, paths)
    a.check()
    return got, want, a


def plan_crcs(engine, payloads):
    """hdfs_crc32c_composite_crcs over a compute plan of the payloads: what a
    caller without this library runs."""
    keep, segs = [], []
    for p in payloads:
        d = engine.DeviceBuffer(max(16, len(p)))
        d.upload(np.frombuffer(p, dtype=np.uint8))
        c = engine.DeviceBuffer(max(4, (len(p) + 511) // 512 * 4))
        keep += [d, c]
        segs.append(engine.Segment(data=d.ptr, len=len(p), chunk_size=512, flags=engine.SEG_BE, crc_init=0, crcs=c.ptr,
                                   bitmap=None))
    engine.Plan(engine.MODE_COMPUTE, segs).execute(None)
    return engine.composite_crcs(segs)


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
                            kw = dict(sync_every=1) if (proto == 2 and (K + ragged) % 3 == 2) else {}
                            s = stream_of(oracle, proto, ctype, dl, seed, last_empty=empty_last, **kw)
                            rows.append((f"{dl[:1]}*{K}+[{ragged}]{'+empty' if empty_last else ''}", s, ragged < body))
                            seed += 1
            out[proto, ctype] = rows
    return out


@pytest.mark.parametrize("ctype", [2, 1])
@pytest.mark.parametrize("proto", [1, 2])
def test_shape_matrix(engine, cs, oracle, matrix, proto, ctype):
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
    batch = a.batch(cs) + a.batch(cs, [n - 7 for n in a.lens])
    assert 200 < len(batch) <= cs.MAX_ENTRIES
    want = [expect(oracle, s[:n], proto, ctype) for s, n in zip(streams + streams, lens)]
    got = cs.block_crcs(batch, proto, 512, ctype)
    compare(got, want)
    a.check()
    assert all(w["rc"] == 0 for w in want)
    whole = got[:len(rows)]
    assert [g["path"] for g in whole] == [cs.PATH_KERNEL if reg else cs.PATH_FALLBACK for _, _, reg in rows]
    assert {g["path"] for g in got[len(rows):]} == {cs.PATH_KERNEL, cs.PATH_FALLBACK}
    assert all(g["consumed"] < n for g, n in zip(got[len(rows):], a.lens))  # the cut packet is not consumed
    if ctype == 2:  # the chain a caller runs today gives the same CRCs
        pick = list(range(0, len(rows), 17))
        payloads = [b"".join(oracle_payload(oracle, streams[k], proto, ctype)) for k in pick]
        assert [whole[k]["crc"] for k in pick] == plan_crcs(engine, payloads)


def oracle_payload(oracle, s, proto=2, ctype=2):
    recs = oracle.verify_packets(s, proto, 512, ctype, verify=False)[1]
    return [s[r["stream_off"] + r["header_len"] + r["crc_len"]:][:r["data_len"]] for r in recs]


# ---- 2. the reduce's run boundaries, divergent lengths, nothing to fold ------------------------------------------
def test_run_boundaries_of_the_reduce(engine, cs, oracle):
    """Entries of 1, 2, 63, 64, 65 and 129 packets of 512 bytes, with and without
    the empty last packet and a shorter one: one packet a lane, some lanes
    without any, the first lanes with one more."""
    streams = []
    for k, n in enumerate((1, 2, 63, 64, 65, 129)):
        streams.append(stream_of(oracle, 2, 2, [512] * n, 1500 + k, last_empty=False))
        streams.append(stream_of(oracle, 2, 2, [512] * (n - 1) + [77], 1520 + k))
        streams.append(stream_of(oracle, 1, 2, [512] * n, 1540 + k))
    v2 = [s for k, s in enumerate(streams) if k % 3 != 2]
    # a lone packet of 77 bytes is no run of whole chunks: the main library's
    got, want, _ = run(cs, engine, oracle, v2, paths=[cs.PATH_KERNEL, cs.PATH_FALLBACK] + [cs.PATH_KERNEL] * 10)
    assert sorted({w["npkts"] for w in want}) == [1, 2, 3, 63, 64, 65, 66, 129, 130]
    run(cs, engine, oracle, streams[2::3], proto=1, paths=[cs.PATH_KERNEL] * 6)


def test_65_entries_of_divergent_lengths(engine, cs, oracle):
    """65 entries: the fold's waves find their packets' entries across a prefix
    of widely differing counts, and one entry has no bytes at all."""
    rng = np.random.default_rng(65)
    streams = []
    for k in range(65):
        body = (512, 5120, 65536, 4096)[k % 4]
        K = int(rng.integers(1, (40, 12, 3, 20)[k % 4] + 1))
        tail = int(rng.integers(0, min(body, 3000)))
        streams.append(stream_of(oracle, 2, 2, [body] * K + ([tail] if tail else []), 2000 + k, last_empty=k % 5 != 0))
    streams[40] = b""
    got, want, _ = run(cs, engine, oracle, streams, paths=[cs.PATH_KERNEL] * 40 + [None] + [cs.PATH_KERNEL] * 24)
    assert (got[40]["rc"], got[40]["nchunks"], got[40]["npkts"], got[40]["crc"]) == (0, 0, 0, 0)
    assert len({w["nchunks"] for w in want}) > 40


def test_streams_without_a_complete_packet(engine, cs, oracle):
    s = stream_of(oracle, 2, 2, [4096] * 2, 2100)
    streams = [s[:20], s[:5], stream_of(oracle, 2, 2, [], 2101), s]
    got, _, _ = run(cs, engine, oracle, streams)
    assert [(g["rc"], g["nchunks"], g["crc"]) for g in got[:3]] == [(0, 0, 0)] * 3
    assert [g["npkts"] for g in got] == [0, 0, 1, 3]


# ---- 3. irregular entries among regular ones ---------------------------------------------------------------------
def _flip(s, at, mask=0x04):
    b = bytearray(s)
    b[at] ^= mask
    return bytes(b)


@pytest.mark.parametrize("ctype", [2, 1])
def test_chunk_size_4096_is_the_main_librarys(engine, cs, oracle, ctype):
    """Another chunk size: the same two kernels with that size's multipliers,
    over the packets the main library framed; ragged last chunks in packets that
    are not the stream's last."""
    dls = [[65536] * 2 + [5000], [8192], [], [40000] * 3 + [4097], [300000, 4096 * 70 + 1, 5]]
    streams = [stream_of(oracle, 2, ctype, dl, 400 + k, chunk=4096) for k, dl in enumerate(dls)]
    got, _, _ = run(cs, engine, oracle, streams, ctype=ctype, chunk=4096, paths=[cs.PATH_FALLBACK] * 5)
    assert [g["nchunks"] for g in got] == [34, 2, 0, 32, 74 + 71 + 1]


@pytest.mark.parametrize("proto", [1, 2])
def test_irregular_entries_among_regular_ones(engine, cs, oracle, proto):
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
    K, F = cs.PATH_KERNEL, cs.PATH_FALLBACK
    paths = [K, F, K, F, F, F, K]
    if proto == 2:  # a valid header that is not the canonical encoding, and syncBlock on one packet only
        streams.append(stream_of(oracle, 2, 2, [8192] * 6 + [3000], 417,
                                 header=lambda k, off, seq, last, dl: header_v2_padded(40, off, seq, last, dl)))
        streams.append(stream_of(oracle, 2, 2, [4096] * 6, 418, sync_at=(2,)))
        paths += [F, F]
    got, want, _ = run(cs, engine, oracle, streams, proto, paths=paths)
    assert want[3]["rc"] == 0 and got[3]["crc"] == expect(oracle, reg(3), proto)["crc"]  # the unflipped stream's
    assert got[4]["rc"] == want[4]["rc"] != 0 and got[4]["crc"] == 0 and got[4]["nchunks"] == 0
    assert got[4]["npkts"] == 4 and got[4]["consumed"] == recs[3]["stream_off"] and got[4]["payload"] == 3 * 8192


def test_the_call_returns_the_first_entry_error(engine, cs, oracle):
    reg = stream_of(oracle, 2, 2, [8192] * 6, 420)
    recs = oracle.verify_packets(reg, 2, 512, 2, verify=False)[1]
    bad = _flip(reg, recs[3]["stream_off"] + 6 + 21)
    a = Arena(engine, [reg, bad, reg])
    arr = cs.entries(a.batch(cs))
    rc = cs.load().hdfs_crc_streams_block_crcs(arr, 3, 2, 512, 2, None)
    assert rc == arr[1].rc == expect(oracle, bad)["rc"] > 0 and arr[0].rc == arr[2].rc == 0
    assert arr[0].crc == arr[2].crc == expect(oracle, reg)["crc"] and arr[1].crc == 0


def test_nothing_is_verified_and_nothing_read_but_the_crcs(engine, cs, oracle):
    """One CRC word altered, in a body packet and in a ragged tail packet, and
    all the data bytes altered: the value is the combine of the words as they
    stand over their chunks' lengths, folded here with the oracle's combine."""
    dl = [5120] * 9 + [700]
    s = bytearray(stream_of(oracle, 2, 2, dl, 425))
    recs = oracle.verify_packets(bytes(s), 2, 512, 2, verify=False)[1]
    for r in recs:  # the data says nothing any more
        d0 = r["stream_off"] + r["header_len"] + r["crc_len"]
        s[d0:d0 + r["data_len"]] = bytes(b ^ 0xFF for b in s[d0:d0 + r["data_len"]])
    s[recs[4]["stream_off"] + recs[4]["header_len"] + 4 * 3 + 1] ^= 0x40   # packet 4, chunk 3
    s[recs[9]["stream_off"] + recs[9]["header_len"] + 4 + 2] ^= 0x01       # the tail packet's ragged chunk
    s = bytes(s)
    want = 0
    for r in recs:
        c0 = r["stream_off"] + r["header_len"]
        for i in range(r["crc_len"] // 4):
            want = oracle.combine(want, int.from_bytes(s[c0 + 4 * i:c0 + 4 * i + 4], "big"),
                                  min(512, r["data_len"] - 512 * i))
    clean = stream_of(oracle, 2, 2, dl, 425)
    a = Arena(engine, [s, clean], res=(1, 3))
    got = cs.block_crcs(a.batch(cs))
    assert [g["path"] for g in got] == [cs.PATH_KERNEL] * 2 and got[0]["rc"] == 0
    assert got[0]["crc"] == want != got[1]["crc"] == expect(oracle, clean)["crc"]
    a.check()


def test_identical_and_overlapping_streams(engine, cs, oracle):
    s = stream_of(oracle, 2, 2, [5120] * 9 + [700], 430)
    a = Arena(engine, [s], res=(3,))
    p, n = a.buf.ptr + a.src[0], len(s)
    first = oracle.verify_packets(s, 2, 512, 2, verify=False)[1][1]["stream_off"]
    got = cs.block_crcs([cs.entry(p, n), cs.entry(p, n), cs.entry(p + first, n - first)])
    w = expect(oracle, s)
    compare(got[:2], [w, w], [cs.PATH_KERNEL] * 2)
    compare(got[2:], [expect(oracle, s[first:])], [cs.PATH_KERNEL])
    assert got[2]["offset_in_block"] == 5120 and got[2]["nchunks"] == w["nchunks"] - 10
    a.check()


# ---- 4. round trips from the write side and after the read side ----------------------------------------------------
@pytest.fixture(scope="module")
def written(engine, cs):
    """Three blocks composed by hadoofus_amd.wire_fused_batch from data in device
    memory, the wire streams at odd addresses of one allocation:
    (the allocations, the streams' batch, lens, wire lens, data)."""
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
    return (wire, src), [cs.entry(wire.ptr + at[k], wl[k]) for k in range(3)], lens, wl, data


def test_round_trip_from_the_fused_batch_write_library(engine, cs, written):
    """The block CRCs from the wire streams hdfs_wire_fused_batch_compose wrote
    equal hdfs_crc32c_composite_crcs over a compute plan of the same data and
    hdfs_crc32c_stream_ex of it: neither the oracle nor this library's framing
    decides.  The file checksum is the CRC of the three payloads in a row."""
    (wire, _src), batch, lens, wl, data = written
    before = wire.download()
    fc, got = cs.file_checksum(batch)
    assert [(g["rc"], g["consumed"], g["payload"], g["nchunks"], g["offset_in_block"], g["path"]) for g in got] == \
        [(0, wl[k], lens[k], (lens[k] + 511) // 512, 0, cs.PATH_KERNEL) for k in range(3)]
    assert [g["crc"] for g in got] == plan_crcs(engine, [d.tobytes() for d in data]) == \
        [engine.stream_ex(2, 0, d) for d in data]
    whole = engine.stream_ex(2, 0, np.concatenate(data))
    assert (fc["crc"], fc["bytes"], fc["length"], fc["bytes_per_crc"], fc["ctype"]) == \
        (whole, whole.to_bytes(4, "big"), sum(lens), 512, 2)
    assert np.array_equal(wire.download(), before)


def test_after_a_read_batch_on_the_same_stream(engine, cs, written):
    """hdfs_read_batch_read_blocks verifies the streams on a stream of the
    caller's, then this call folds them on the same stream: nothing between."""
    from hadoofus_read import read_batch as rb
    _bufs, batch, lens, wl, data = written
    back = engine.DeviceBuffer(sum(lens) + 3 * 64)
    at = [sum(lens[:k]) + 64 * k + (1, 0, 5)[k] for k in range(3)]
    st = engine.stream_create()
    try:
        read = rb.read_blocks([rb.entry(batch[k]["stream_ptr"], wl[k], back.ptr + at[k], lens[k]) for k in range(3)],
                              stream=st)
        got = cs.block_crcs(batch, stream=st)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0
    assert [(r["rc"], r["delivered"]) for r in read] == [(0, n) for n in lens]
    assert [g["crc"] for g in got] == plan_crcs(engine, [d.tobytes() for d in data]) == \
        [engine.stream_ex(2, 0, d) for d in data]
    assert [g["payload"] for g in got] == lens


def test_one_block_of_128_mib_and_513_bytes(engine, cs):
    """Filled and composed on the device: the shift exponents of a whole block
    (2 049 packets, 32 or 33 a lane of the reduce, up to 2^27 bytes behind a
    run) cannot be reached any smaller.  Expected is hdfs_crc32c_stream_ex of
    the payload in device memory."""
    from hadoofus_amd import wire_fused_batch as fb
    n = (128 << 20) + 513
    outs, _ = fb.layout([fb.write(nbytes=n, offset_in_block=0, seqno=0, finish=True)])
    wl = outs[0]["wire_len"]
    src = engine.DeviceBuffer((n + 7) // 8 * 8)
    engine.fill_splitmix64(src.ptr, (n + 7) // 8, seed=128)
    wire = engine.DeviceBuffer(wl + 64)
    fb.compose([fb.write(src.ptr, n, wire.ptr + 3, wl, 0, 0, True)])
    engine.device_sync()
    want = ctypes.c_uint32(0)
    assert engine.load().hdfs_crc32c_stream_ex(2, 0, src.ptr, n, ctypes.byref(want)) == 0
    got = cs.block_crcs([cs.entry(wire.ptr + 3, wl)])[0]
    assert (got["rc"], got["consumed"], got["payload"], got["nchunks"], got["path"]) == \
        (0, wl, n, (n + 511) // 512, cs.PATH_KERNEL)
    assert got["npkts"] >= 2049 and got["crc"] == want.value


# ---- 5. the file checksum ------------------------------------------------------------------------------------------
def test_file_checksum_of_four_unequal_blocks(engine, cs, oracle):
    for ctype in (2, 1):
        dls = [[65536] * 3 + [100], [512], [5120] * 20, [8192, 4096, 8192, 1]]  # the last one falls back
        streams = [stream_of(oracle, 2, ctype, dl, 495 + k) for k, dl in enumerate(dls)]
        a = Arena(engine, streams)
        fc, got = cs.file_checksum(a.batch(cs), ctype=ctype)
        compare(got, [expect(oracle, s, 2, ctype) for s in streams], [0, 0, 0, 1])
        data = b"".join(b"".join(oracle_payload(oracle, s, 2, ctype)) for s in streams)
        want = crc_of(oracle, ctype, data)
        assert (fc["crc"], fc["bytes"], fc["length"], fc["bytes_per_crc"], fc["ctype"]) == \
            (want, want.to_bytes(4, "big"), len(data), 512, ctype)
        assert cs.combine([g["crc"] for g in got], [g["payload"] for g in got], ctype) == want
        a.check()


def test_file_checksum_refusals(engine, cs, oracle):
    """EINVAL with the entries' out fields still filled: an entry with a packet
    error, and a stream that does not start at its block's start."""
    good = stream_of(oracle, 2, 2, [8192] * 4, 490)
    recs = oracle.verify_packets(good, 2, 512, 2, verify=False)[1]
    inside = stream_of(oracle, 2, 2, [8192] * 4, 491, offset0=8192)
    bad = _flip(good, recs[2]["stream_off"] + 6 + 21)
    lib = cs.load()
    for k, (streams, text) in enumerate((([good, inside, good], "entry 1"), ([good, good, bad], "entry 2"))):
        a = Arena(engine, streams)
        arr, fc = cs.entries(a.batch(cs)), cs.FileChecksum()
        rc = lib.hdfs_crc_streams_file_checksum(arr, 3, 2, 512, 2, None, ctypes.byref(fc))
        err = lib.hdfs_crc_streams_last_error().decode()
        assert rc == EINVAL and text in err, err
        want = [expect(oracle, s) for s in streams]
        assert [(e.rc, e.nchunks, e.offset_in_block, e.crc) for e in arr] == \
            [(w["rc"], w["nchunks"], w["offset_in_block"], w["crc"]) for w in want]
        assert (fc.crc, bytes(fc.bytes), fc.length) == (0, bytes(4), 0)
        with pytest.raises(cs.abi.CRC32CError):
            cs.file_checksum(a.batch(cs))
    a = Arena(engine, [good, good])
    arr = cs.entries(a.batch(cs))
    assert lib.hdfs_crc_streams_file_checksum(arr, 2, 2, 512, 2, None, None) == EINVAL
    assert [e.crc for e in arr] == [expect(oracle, good)["crc"]] * 2  # the out fields are filled all the same


# ---- 6. ordering ----------------------------------------------------------------------------------------------
def test_streams_copied_on_the_null_stream_just_before(engine, cs, oracle):
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
    got = cs.block_crcs(a.batch(cs))
    compare(got, [expect(oracle, s) for s in streams], [cs.PATH_KERNEL] * 2)


def test_on_a_stream_of_the_callers(engine, cs, oracle):
    st = engine.stream_create()
    try:
        streams = [stream_of(oracle, 1, 2, dl, 450 + k, last_empty=False)
                   for k, dl in enumerate([[65536] * 3 + [12345], [4096] * 20, [512], [8192, 4096, 8192]])]
        run(cs, engine, oracle, streams, 1, stream=st, paths=[cs.PATH_KERNEL] * 3 + [cs.PATH_FALLBACK])
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, cs, oracle):
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
                compare(cs.block_crcs(a.batch(cs), proto), want, [cs.PATH_KERNEL, cs.PATH_FALLBACK, cs.PATH_KERNEL])
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


def test_the_timing_entry(engine, cs, oracle):
    streams = [stream_of(oracle, 2, 2, [65536] * 4 + [100], 470), stream_of(oracle, 2, 2, [40000] * 2, 471)]
    a = Arena(engine, streams)
    t, got = cs.time(a.batch(cs), iters=3)
    assert t > 0
    compare(got, [expect(oracle, s) for s in streams], [cs.PATH_KERNEL, cs.PATH_FALLBACK])
    a.check()


# ---- 7. refusals ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_arena_untouched_and_name_the_entry(engine, cs, oracle):
    streams = [stream_of(oracle, 2, 2, [4096] * 3, 480 + k) for k in range(4)]
    a = Arena(engine, streams)
    lib, end = cs.load(), a.buf.ptr + a.buf.nbytes
    host = np.zeros(1 << 16, dtype=np.uint8)

    def call(n=4, proto=2, chunk=512, ctype=2, **kw):
        """kw: {field}{entry}=value, e.g. stream0=..., len3=..."""
        b = a.batch(cs)
        for key, v in kw.items():
            b[int(key[-1])][{"stream": "stream_ptr", "len": "nbytes"}[key[:-1]]] = v
        arr = cs.entries(b) if n <= 4 else (cs.Entry * n)()
        for e in arr:
            e.npkts = e.nchunks = e.consumed = e.crc = 9
        rc = lib.hdfs_crc_streams_block_crcs(arr, n, proto, chunk, ctype, None)
        return rc, lib.hdfs_crc_streams_last_error().decode(), arr
    cases = {
        "a host stream in entry 3": (dict(stream3=host.ctypes.data), "entry 3"),
        "stream 0 past its allocation": (dict(stream0=end - a.lens[0] + 1), "entry 0"),
        "stream 2 longer than its allocation": (dict(len2=a.buf.nbytes), "entry 2"),
        "a null stream with bytes": (dict(stream1=None), "entry 1"),
        "chunk_size 0": (dict(chunk=0), "entry 0: chunk_size"),
        "CSUM_NULL": (dict(ctype=0), "entry 0"),
        "ctype 3": (dict(ctype=3), "entry 0"),
        "proto 3": (dict(proto=3), "entry 0: proto"),
        "no entries": (dict(n=0), "no entries"),
        "too many entries": (dict(n=cs.MAX_ENTRIES + 1), "entry 1024"),
    }
    for name, (kw, text) in cases.items():
        rc, err, arr = call(**kw)
        assert rc == EINVAL and text in err, (name, err)
        if kw.get("n", 4) == 4:
            assert [(e.rc, e.npkts, e.nchunks, e.consumed, e.crc) for e in arr] == [(0, 0, 0, 0, 0)] * 4
        assert not host.any(), name
    a.check()
    rc, err, arr = call()  # and the same arguments, unspoilt, work
    assert rc == 0 and [e.nchunks for e in arr] == [24] * 4
    a.check()


# ---- 8. the C caller ----------------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "crc_streams_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "crc_streams_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_crc_streams", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    blocks = [(int(l.split()[1], 16), int(l.split()[2])) for l in lines if l.startswith("block ")]
    crc, length = [l for l in lines if l.startswith("file ")][0].split()[1:]
    assert len(blocks) == 3 and int(length) == sum(n for _, n in blocks)
    from hadoofus_read import crc_streams
    assert crc_streams.combine([c for c, _ in blocks], [n for _, n in blocks]) == int(crc, 16)
