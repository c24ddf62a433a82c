"""GPU: the wire streams of a batch of writes in one call
(include/hadoofus_wire_batch.h) -- one compute plan of the main library over
every write's chunk grid, one table upload, then frame_batch_kernel, where each
workgroup finds its packet's write by binary search and frames the packet with
the single-write kernel's code.

The expected stream of every write is built on the host from the CPU oracle:
oracle.compose_packets(data, ...) of that write alone gives the header buffers
and the records; packet after packet, hdr[hdr_off : hdr_off + hdr_len] is
followed by data[data_off : data_off + data_len].  All sources and all
destinations of a batch are carved from one device allocation between 0xA5
guards, at chosen byte residues mod 16; after every call the whole allocation
is downloaded and compared with the image expected, so the sources and the
guards are untouched and every wire equals its expected stream.  Everything
is bit-exact."""
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
EMPTY = np.zeros(0, np.uint8)


@pytest.fixture(scope="module")
def wb(engine):
    from hadoofus_amd import wire_batch
    wire_batch.load()
    return wire_batch


@pytest.fixture(scope="module")
def wr(engine):
    from hadoofus_amd import wire
    wire.load()
    return wire


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


def room(sources, dests):
    """Bytes of an arena that holds these many source and destination bytes."""
    return sum(n + GAP + 32 for n in list(sources) + list(dests)) + GAP + 32


class Arena:
    """One device allocation: guards, then every source and every destination,
    each at its own residue mod 16 with guards between."""

    def __init__(self, engine, nbytes):
        self.buf = engine.DeviceBuffer(nbytes)
        assert self.buf.ptr % 16 == 0

    def place(self, sources, dests):
        """sources: [(data, residue)], dests: [(bytes, residue)] -> (source
        pointers, destination pointers)."""
        at, self.src, self.dst = GAP, [], []
        for n, mis, into in [(len(d), m, self.src) for d, m in sources] + [(n, m, self.dst) for n, m in dests]:
            at = (at + 15) // 16 * 16 + mis
            into.append(at)
            at += n + GAP
        assert at <= self.buf.nbytes, (at, self.buf.nbytes)
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        for (d, _), o in zip(sources, self.src):
            self.image[o:o + len(d)] = d
        self.buf.upload(self.image)
        p = self.buf.ptr
        return [p + o for o in self.src], [p + o for o in self.dst]

    def check(self, streams):
        """The whole allocation: stream k at destination k, nothing else changed."""
        want = self.image.copy()
        for o, s in zip(self.dst, streams):
            want[o:o + len(s)] = s
        got = self.buf.download()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (sources {self.src[:8]}, destinations "
                                 f"{self.dst[:8]}): got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def batch(wb, oracle, arena, specs, proto=2, ctype=2, stream=None, want=None):
    """specs: [dict(data, off, seq, finish, src_mis, dst_mis)].  Places them,
    composes the batch and checks lengths, records and the whole arena.
    -> (expected [(stream, records)], destination pointers)."""
    if want is None:
        want = [expect(oracle, s["data"], s.get("off", 0), s.get("seq", 0), proto, ctype, s.get("finish", False))
                for s in specs]
    sp, dp = arena.place([(s["data"], s.get("src_mis", 0)) for s in specs],
                         [(len(x[0]), s.get("dst_mis", 0)) for s, x in zip(specs, want)])
    writes = [wb.write(sp[k], len(s["data"]), dp[k], len(want[k][0]), s.get("off", 0), s.get("seq", 0),
                       s.get("finish", False)) for k, s in enumerate(specs)]
    got = wb.compose_wire_batch(writes, proto, ctype, stream)
    assert [g[0] for g in got] == [len(x[0]) for x in want]
    assert [g[1] for g in got] == [x[1] for x in want]
    arena.check([x[0] for x in want])
    return want, dp


# ---- 1. a batch of one is the single call ---------------------------------------------------
def test_batch_of_one_equals_the_single_call(engine, wb, wr, oracle):
    big = 2 * 65536 + 700
    d = payload(71, 0, big)
    a = Arena(engine, room([big], [big + 4096] * 2))
    k = 0
    for n, finish in ((0, True), (1, False), (513, True), (65537, False), (big, True)):
        for off in (0, 4321):
            k += 1
            stream, recs = expect(oracle, d[:n], off, 40 + k, 2, 2, finish)
            sp, dp = a.place([(d[:n], k % 4)], [(len(stream), (5 * k) % 16), (len(stream), (7 * k + 1) % 16)])
            got = wb.compose_wire_batch([wb.write(sp[0], n, dp[0], len(stream), off, 40 + k, finish)])
            single = wr.compose_wire(sp[0], n, dp[1], len(stream), off, 40 + k, 2, 2, finish)
            assert got == [single] and single == (len(stream), recs), (n, off)
            a.check([stream, stream])


# ---- 2. a mixed batch, zero-packet entries first, in the middle and last -----------------------
def test_mixed_batch_of_nine_at_every_destination_residue(engine, wb, oracle):
    big = 2 * 65536 + 700
    d = payload(72, 0, big + 65537 + 65536 + 512 + 511 + 1)
    cut, at = [], 0
    for n in (0, 0, 1, 511, 512, 65536, 65537, big, 0):
        cut.append(d[at:at + n])
        at += n
    specs = [dict(data=c, seq=1000 * k + 3, off=4321 if k == 7 else 0, finish=k in (1, 7))
             for k, c in enumerate(cut)]
    want = [expect(oracle, s["data"], s["off"], s["seq"], 2, 2, s["finish"]) for s in specs]
    assert [len(x[1]) for x in want] == [0, 1, 1, 1, 1, 1, 2, 5, 0]
    assert [p["data_len"] for p in want[7][1]] == [287, 65536, 65536, 700 - 287, 0]
    a = Arena(engine, room([len(c) for c in cut], [len(x[0]) for x in want]))
    for r in range(16):
        for k, s in enumerate(specs):
            s["dst_mis"] = (r + 3 * k) % 16
            s["src_mis"] = (0, 1, 2, 3, 7)[(k + r) % 5]
        assert {(r + 3 * 7) % 16 for r in range(16)} == set(range(16))
        batch(wb, oracle, a, specs, want=want)


# ---- 3. the lookup at every index -----------------------------------------------------------------
def test_lookup_at_every_index_of_three_hundred_writes(engine, wb, oracle):
    """300 writes of 100 B, one packet each, an empty no-finish write after
    every seventh: the search runs over 300 table entries (past 256) and every
    global packet index selects another write."""
    d = payload(73, 0, 300 * 100)
    specs = []
    for k in range(300):
        specs.append(dict(data=d[100 * k:100 * k + 100], seq=7 * k, off=512 * (k % 3), src_mis=k % 5,
                          dst_mis=(11 * k) % 16))
        if k % 7 == 6:
            specs.append(dict(data=EMPTY, seq=5))
    assert len(specs) == 342
    a = Arena(engine, room([100] * 342, [139] * 342))
    want, _ = batch(wb, oracle, a, specs)
    assert sum(len(x[1]) for x in want) == 300 and len({x[0].tobytes() for x in want}) == 301


# ---- 4. protocols and checksum types -----------------------------------------------------------------
@pytest.mark.parametrize("ctype", [2, 1, 0], ids=["crc32c", "crc32", "null"])
@pytest.mark.parametrize("proto", [2, 1])
def test_protocols_and_checksum_types(engine, wb, oracle, proto, ctype):
    d = payload(74, 0, 65536 + 3000)
    specs = [dict(data=d[:65536 + 3000], off=4321, seq=1, finish=True, src_mis=1, dst_mis=9),
             dict(data=EMPTY, seq=2, finish=True, dst_mis=2),
             dict(data=d[100:613], seq=3, src_mis=3, dst_mis=15),
             dict(data=d[7:70007], off=1024, seq=4, finish=True, src_mis=2, dst_mis=4)]
    a = Arena(engine, room([len(s["data"]) for s in specs], [len(s["data"]) + 2048 for s in specs]))
    want, _ = batch(wb, oracle, a, specs, proto, ctype)
    assert len(want[1][0]) == (25 if proto == 1 else 31)


# ---- 5. two writes of one source -----------------------------------------------------------------------
def test_two_writes_share_one_source(engine, wb, oracle):
    n = 65536 + 777
    d = payload(75, 0, n)
    stream, recs = expect(oracle, d, 0, 9, 2, 2, True)
    a = Arena(engine, room([n], [len(stream)] * 2))
    sp, dp = a.place([(d, 3)], [(len(stream), 6), (len(stream), 13)])
    got = wb.compose_wire_batch([wb.write(sp[0], n, dp[k], len(stream), 0, 9, True) for k in range(2)])
    assert got == [(len(stream), recs)] * 2
    a.check([stream, stream])  # both equal, the source and the guards untouched


# ---- 6. larger writes: the plan's tiled path, hundreds of packets per write --------------------------------
def test_three_writes_of_nine_mib_at_odd_addresses(engine, wb, oracle):
    n = (9 << 20) + 321
    d = payload(76, 0, n)
    specs = [dict(data=d, off=off, seq=seq, finish=True, src_mis=sm, dst_mis=dm)
             for off, seq, sm, dm in ((4321, 0, 3, 6), (0, 500, 1, 11), (512 * 5 + 1, 900, 7, 1))]
    a = Arena(engine, room([n] * 3, [n + 80000] * 3))
    want, _ = batch(wb, oracle, a, specs)
    assert all(len(x[1]) > 140 for x in want)


# ---- 7. round trip through the read side -----------------------------------------------------------------
def test_round_trip_through_verify_blocks(engine, wb, oracle):
    d = payload(77, 0, 4 * (3 * 65536 + 1234))
    n = 3 * 65536 + 1234
    specs = [dict(data=d[k * n:(k + 1) * n], seq=0, finish=True, src_mis=k + 1, dst_mis=(5 * k + 3) % 16)
             for k in range(4)]
    a = Arena(engine, room([n] * 4, [n + 4096] * 4))
    want, dp = batch(wb, oracle, a, specs)
    blocks = [(dp[k], len(want[k][0])) for k in range(4)]
    rc, got = engine.VerifyBlocksJob(blocks).wait()
    assert rc == 0 and got == [oracle.verify_packets(x[0].tobytes()) for x in want]
    assert all(g[0] == 0 and g[2] == len(x[0]) and len(g[1]) == len(x[1]) for g, x in zip(got, want))
    # one byte of packet 1's chunk 10 of write 2 flipped on the device, inside its stream
    p = want[2][1][1]
    at = p["hdr_off"] + p["hdr_len"] + 10 * CS + 100
    a.buf.upload(np.array([want[2][0][at] ^ 0x20], dtype=np.uint8), a.dst[2] + at)
    rc, got = engine.VerifyBlocksJob(blocks).wait()
    assert rc == engine.ERR_BAD_CHECKSUM and [g[0] for g in got] == [0, 0, engine.ERR_BAD_CHECKSUM, 0]
    bad = [(b, i, q["first_bad"], q["bad_chunks"]) for b, g in enumerate(got) for i, q in enumerate(g[1]) if q["error"]]
    assert bad == [(2, 1, 10, 1)]


# ---- 8. ordering ------------------------------------------------------------------------------------------
def test_sources_filled_on_the_null_stream_just_before(engine, wb, oracle):
    """No synchronisation between the fills (NULL stream) and the call: the
    library's stream waits for the NULL stream."""
    n = 3 << 20
    ds = [payload(78 + k, 0, n) for k in range(2)]
    want = [expect(oracle, ds[k], 4321 * k, k, 2, 2, False) for k in range(2)]
    a = Arena(engine, room([n] * 2, [len(x[0]) for x in want]))
    sp, dp = a.place([(np.zeros(n, np.uint8), 8), (np.zeros(n, np.uint8), 0)], [(len(want[0][0]), 13), (len(want[1][0]), 2)])
    assert all(p % 8 == 0 for p in sp)
    for k in range(2):
        engine.fill_splitmix64(sp[k], n // 8, 78 + k, 0, None)
    got = wb.compose_wire_batch([wb.write(sp[k], n, dp[k], len(want[k][0]), 4321 * k, k) for k in range(2)])
    assert got == [(len(x[0]), x[1]) for x in want]
    for k in range(2):
        a.image[a.src[k]:a.src[k] + n] = ds[k]
    a.check([x[0] for x in want])


def test_on_a_stream_of_the_callers(engine, wb, oracle):
    d = payload(80, 0, 3 * 65536 + 77)
    specs = [dict(data=d, off=512, seq=0, finish=True, src_mis=2, dst_mis=5),
             dict(data=d[:1000], off=0, seq=70, src_mis=1, dst_mis=12),
             dict(data=EMPTY, seq=0),
             dict(data=d[65536:], off=4321, seq=90, finish=True, src_mis=3, dst_mis=8)]
    a = Arena(engine, room([len(s["data"]) for s in specs], [len(s["data"]) + 4096 for s in specs]))
    want, _ = batch(wb, oracle, a, specs, 1, 1)  # the same batch on the library's stream ...
    st = engine.stream_create()
    try:
        batch(wb, oracle, a, specs, 1, 1, stream=st, want=want)  # ... and on the caller's
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


# ---- 9. rejections: nothing is written anywhere, the text names the entry -------------------------------------
def test_rejections_write_nothing_and_name_the_entry(engine, wb, oracle):
    from hadoofus_amd.abi import OutPacket
    lens = [100000, 0, 70000, 513]
    d = payload(81, 0, sum(lens))
    cut = [d[sum(lens[:k]):sum(lens[:k + 1])] for k in range(4)]
    fin = [True, True, False, True]
    want = [expect(oracle, cut[k], 0, k, 2, 2, fin[k]) for k in range(4)]
    wl = [len(x[0]) for x in want]
    npk = sum(len(x[1]) for x in want)
    a = Arena(engine, room(lens, wl))
    sp, dp = a.place([(cut[k], k + 1) for k in range(4)], [(wl[k], 3 * k + 2) for k in range(4)])
    lib = wb.load()
    arr = (OutPacket * npk)()
    before = bytes(arr)
    cnt = ctypes.c_size_t(0)
    host = np.zeros(max(wl) + 64, dtype=np.uint8)
    end = a.buf.ptr + a.buf.nbytes

    def call(maxp=npk, n=4, **kw):
        """kw: {field}{entry}=value, e.g. wire2=..., cap0=..., data3=..."""
        ws = [dict(dptr=sp[k], nbytes=lens[k], wire_ptr=dp[k], wire_cap=wl[k], offset_in_block=0, seqno=k,
                   finish=fin[k]) for k in range(4)]
        for key, v in kw.items():
            ws[int(key[-1])][{"wire": "wire_ptr", "cap": "wire_cap", "data": "dptr"}[key[:-1]]] = v
        e = wb.entries(ws * (n // 4) if n > 4 else ws)
        rc = lib.hdfs_wire_batch_compose(e, n, 2, 2, arr, maxp, ctypes.byref(cnt), None)
        return rc, e, lib.hdfs_wire_batch_last_error().decode()
    cases = {
        "wire 2 overlaps wire 0": (dict(wire2=dp[0] + wl[0] - 1), 2),
        "wire 3 inside wire 2": (dict(wire3=dp[2] + 100), 3),
        "wire 2 overlaps data 3": (dict(wire2=sp[3] - wl[2] + 1), 2),
        "wire 3 inside data 0": (dict(wire3=sp[0] + 10), 3),
        "data 3 over wire 0's start": (dict(data3=dp[0] - lens[3] + 1), 0),
        "wire 1 (header only) inside data 0": (dict(wire1=sp[0] + lens[0] - 5), 1),
        "short capacity in entry 2": (dict(cap2=wl[2] - 1), 2),
        "a host wire in entry 3": (dict(wire3=host.ctypes.data), 3),
        "a host source in entry 2": (dict(data2=host.ctypes.data), 2),
        "wire 0 past its allocation": (dict(wire0=end - wl[0] + 1), 0),
        "source 3 past its allocation": (dict(data3=end - lens[3] + 1), 3),
        "a NULL wire in entry 2 alone": (dict(wire2=None), 2),
    }
    for name, (kw, k) in cases.items():
        rc, e, err = call(**kw)
        assert rc == EINVAL and f"entry {k}" in err, (name, err)
        assert cnt.value == npk and [(x.wire_len, x.npkts) for x in e[:4]] == [(wl[j], len(want[j][1])) for j in range(4)], name
        assert [x.first_pkt for x in e[:4]] == [sum(len(y[1]) for y in want[:j]) for j in range(4)], name
        assert bytes(arr) == before and not host.any(), name
    rc, e, err = call(maxp=npk - 1)
    assert rc == EINVAL and "entry 3" in err and cnt.value == npk and bytes(arr) == before, err
    rc, e, err = call(maxp=len(want[0][1]))
    assert rc == EINVAL and "entry 1" in err and cnt.value == npk and bytes(arr) == before, err
    rc, e, err = call(n=wb.MAX_WRITES + 4)
    assert rc == EINVAL and str(wb.MAX_WRITES) in err and bytes(arr) == before, err
    a.check([])
    rc, e, err = call()  # and the same arguments, unspoilt, work
    assert rc == 0 and [arr[i].as_dict() for i in range(npk)] == [p for x in want for p in x[1]]
    a.check([x[0] for x in want])


# ---- 10. threads and C ---------------------------------------------------------------------------------------
def test_two_threads_at_once(engine, wb, oracle):
    jobs = []
    for seed, n, off, proto in [(82, 400000, 0, 2), (83, 250123, 4321, 1)]:
        d = payload(seed, 0, n)
        specs = [dict(data=d, off=off, seq=1, finish=True, src_mis=seed % 4, dst_mis=seed % 16),
                 dict(data=d[:n // 3], off=0, seq=2, src_mis=1, dst_mis=(seed + 5) % 16)]
        want = [expect(oracle, s["data"], s["off"], s["seq"], proto, 2, s.get("finish", False)) for s in specs]
        a = Arena(engine, room([len(s["data"]) for s in specs], [len(x[0]) for x in want]))
        sp, dp = a.place([(s["data"], s["src_mis"]) for s in specs],
                         [(len(x[0]), s["dst_mis"]) for s, x in zip(specs, want)])
        ws = [wb.write(sp[k], len(s["data"]), dp[k], len(want[k][0]), s["off"], s["seq"], s.get("finish", False))
              for k, s in enumerate(specs)]
        jobs.append((a, ws, proto, want))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, ws, proto, want = jobs[i]
            start.wait()
            for _ in range(4):
                assert wb.compose_wire_batch(ws, proto, 2) == [(len(x[0]), x[1]) for x in want]
        except BaseException as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for a, _, _, want in jobs:
        a.check([x[0] for x in want])


def test_frame_time_writes_the_same_streams(engine, wb, oracle):
    d = payload(84, 0, 3 * 65536 + 999)
    specs = [dict(data=d, off=4321, finish=True, src_mis=3, dst_mis=9), dict(data=d[:700], seq=8, dst_mis=1)]
    want = [expect(oracle, s["data"], s.get("off", 0), s.get("seq", 0), 2, 2, s.get("finish", False)) for s in specs]
    a = Arena(engine, room([len(s["data"]) for s in specs], [len(x[0]) for x in want]))
    sp, dp = a.place([(s["data"], s.get("src_mis", 0)) for s in specs],
                     [(len(x[0]), s["dst_mis"]) for s, x in zip(specs, want)])
    ws = [wb.write(sp[k], len(s["data"]), dp[k], len(want[k][0]), s.get("off", 0), s.get("seq", 0),
                   s.get("finish", False)) for k, s in enumerate(specs)]
    assert wb.frame_time(ws, iters=2) > 0
    a.check([x[0] for x in want])


def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "wire_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wire_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wire_batch", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
