"""GPU: the wire streams of a batch of writes in one call, one launch and one
pass over the data (include/hadoofus_wire_fused_batch.h) --
frame_fused_batch_kernel walks the packets of all writes, finds each packet's
write with write_of, copies the data, computes the chunk CRCs from the
registers it copies and writes every byte of every stream.

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
def fb(engine):
    from hadoofus_amd import wire_fused_batch
    wire_fused_batch.load()
    return wire_fused_batch


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


def expect_all(oracle, specs, proto=2, ctype=2):
    return [expect(oracle, s["data"], s.get("off", 0), s.get("seq", 0), proto, ctype, s.get("finish", False))
            for s in specs]


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

    def reset(self):
        self.buf.upload(self.image)

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


def placed(fb, arena, specs, want):
    """Places the specs' sources and their streams' destinations.  -> (write dicts, destination pointers)."""
    sp, dp = arena.place([(s["data"], s.get("src_mis", 0)) for s in specs],
                         [(len(x[0]), s.get("dst_mis", 0)) for s, x in zip(specs, want)])
    return [fb.write(sp[k], len(s["data"]), dp[k], len(want[k][0]), s.get("off", 0), s.get("seq", 0),
                     s.get("finish", False)) for k, s in enumerate(specs)], dp


def batch(fb, arena, specs, want, proto=2, ctype=2, stream=None, groups=None):
    """Places the specs, composes the batch (groups: through the timing entry
    with that many workgroups) and checks lengths, records and the whole arena.
    -> destination pointers."""
    writes, dp = placed(fb, arena, specs, want)
    if groups is None:
        got = fb.compose(writes, proto, ctype, stream)
        assert [g[0] for g in got] == [len(x[0]) for x in want]
        assert [g[1] for g in got] == [x[1] for x in want]
    else:
        assert fb.fused_batch_time(writes, proto, ctype, fb.time_groups(groups), 1) > 0
    arena.check([x[0] for x in want])
    return dp


# ---- 1. the mixed batch ------------------------------------------------------------------------
BIG = 2 * 65536 + 700      # at block offset 4321: packets of 287, 64 KiB, 64 KiB, 413 and 0 bytes
NINETEEN = 17 * 65536 + 45  # with finish: 19 packets, starting at all 16 residues
_mixed = {}


def mixed_specs():
    """Empty without finish; 1 byte; the 287 / 64 KiB / 64 KiB / 413 / 0 write at
    block offset 4321; empty with finish; a 19-packet write; 513 bytes at
    offset 511; empty without finish, last."""
    if "specs" not in _mixed:
        d = payload(91, 0, 1 + BIG + NINETEEN + 513)
        cut, at = [], 0
        for n in (0, 1, BIG, 0, NINETEEN, 513, 0):
            cut.append(d[at:at + n])
            at += n
        offs, fin = (0, 0, 4321, 1024, 0, 511, 0), (False, False, True, True, True, False, False)
        _mixed["specs"] = [dict(data=c, off=offs[k], seq=1000 * k + 3, finish=fin[k], src_mis=(0, 1, 3, 0, 7, 2, 0)[k],
                                dst_mis=(0, 5, 9, 14, 3, 11, 0)[k]) for k, c in enumerate(cut)]
    return _mixed["specs"]


def mixed_want(oracle, proto=2, ctype=2):
    if (proto, ctype) not in _mixed:
        _mixed[proto, ctype] = expect_all(oracle, mixed_specs(), proto, ctype)
    return _mixed[proto, ctype]


def mixed_arena(engine, oracle):
    specs, want = mixed_specs(), mixed_want(oracle, 2, 2)  # CRC32C v2 streams are the longest
    return Arena(engine, room([len(s["data"]) for s in specs], [len(x[0]) for x in want]))


def test_mixed_batch_on_the_product_grid(engine, fb, wf, oracle):
    specs, want = mixed_specs(), mixed_want(oracle)
    assert [len(x[1]) for x in want] == [0, 1, 5, 1, 19, 2, 0]
    assert [p["data_len"] for p in want[2][1]] == [287, 65536, 65536, 413, 0]
    assert [p["data_len"] for p in want[5][1]] == [1, 512]
    a = mixed_arena(engine, oracle)
    batch(fb, a, specs, want)
    # every write's stream against the single fused call's, downloaded
    image = a.buf.download()
    one = engine.DeviceBuffer(max(len(x[0]) for x in want) + 16)
    for k, (s, x) in enumerate(zip(specs, want)):
        n, wl = len(s["data"]), len(x[0])
        got = wf.compose_wire(a.buf.ptr + a.src[k], n, one.ptr + 5, wl, s["off"], s["seq"], 2, 2, s["finish"])
        assert got == (wl, x[1]), k
        assert np.array_equal(one.download()[5:5 + wl], image[a.dst[k]:a.dst[k] + wl]), k


@pytest.mark.parametrize("groups", [1, 3, 7])
def test_mixed_batch_with_few_workgroups(engine, fb, oracle, groups):
    """28 packets on 1, 3 and 7 workgroups: a workgroup's walk crosses write
    boundaries, in both halves of the unrolled loop."""
    batch(fb, mixed_arena(engine, oracle), mixed_specs(), mixed_want(oracle), groups=groups)


@pytest.mark.parametrize("ctype", [2, 1, 0], ids=["crc32c", "crc32", "null"])
@pytest.mark.parametrize("proto", [2, 1])
def test_protocols_and_checksum_types(engine, fb, oracle, proto, ctype):
    want = mixed_want(oracle, proto, ctype)
    assert len(want[3][0]) == (25 if proto == 1 else 31)
    a = mixed_arena(engine, oracle)
    batch(fb, a, mixed_specs(), want, proto, ctype)
    if (proto, ctype) != (2, 2):
        a.reset()
        batch(fb, a, mixed_specs(), want, proto, ctype, groups=3)


# ---- 2. many tiny writes: the lookup past its hop bound ------------------------------------------
_tiny = {}


def tiny(oracle):
    if not _tiny:
        rng = np.random.default_rng(92)
        lens = rng.integers(1, 701, 300)
        lens[rng.integers(0, 300, 25)] = 0  # some empty
        fin = rng.integers(0, 3, 300) == 0  # a third with finish
        d = payload(92, 0, int(lens.sum()))
        specs, at = [], 0
        for k in range(300):
            n = int(lens[k])
            specs.append(dict(data=d[at:at + n], off=int(rng.integers(0, 4)) * 511, seq=13 * k, finish=bool(fin[k]),
                              src_mis=k % 5, dst_mis=(11 * k) % 16))
            at += n
        _tiny["specs"], _tiny["want"] = specs, expect_all(oracle, specs)
    return _tiny["specs"], _tiny["want"]


@pytest.mark.parametrize("groups", [1, 3, 256])
def test_three_hundred_tiny_writes(engine, fb, oracle, groups):
    """300 writes of 0 to 700 bytes, some empty, some with finish: with 256
    workgroups consecutive packets of one workgroup lie some 170 entries
    apart, past the lookup's hops into its search; with 1 every step is the
    next entry or the same one."""
    specs, want = tiny(oracle)
    npk = sum(len(x[1]) for x in want)
    assert 300 < npk < 700 and sum(1 for x in want if not x[1]) > 5
    a = Arena(engine, room([len(s["data"]) for s in specs], [len(x[0]) for x in want]))
    batch(fb, a, specs, want, groups=groups)
    if groups == 256:  # and the call itself, records included
        a.reset()
        got = fb.compose(placed(fb, a, specs, want)[0])
        assert got == [(len(x[0]), x[1]) for x in want]
        a.check([x[0] for x in want])


# ---- 3. alignment -----------------------------------------------------------------------------------
def test_every_wire_residue_against_four_source_residues(engine, fb, oracle):
    d = payload(93, 0, 65536 + 700 + 513 + 1000)
    specs = [dict(data=d[:65536 + 700], off=4321, seq=5, finish=True), dict(data=d[65536 + 700:][:513], off=511, seq=6),
             dict(data=d[65536 + 1213:], seq=7, finish=True)]
    want = expect_all(oracle, specs)
    a = Arena(engine, room([len(s["data"]) for s in specs], [len(x[0]) for x in want]))
    for r in range(16):
        for sm in (0, 1, 3, 7):
            for k, s in enumerate(specs):
                s["dst_mis"] = (r + 5 * k) % 16
                s["src_mis"] = (sm + k) % 16 if k else sm
            batch(fb, a, specs, want)


# ---- 4. replicas: identical and overlapping data ranges --------------------------------------------------
def test_replicas_and_overlapping_sources(engine, fb, oracle):
    n = 65536 + 777
    d = payload(94, 0, n)
    ranges = [(0, n, 0, 9, True), (0, n, 4321, 400, False), (100, 66000, 512, 7, True), (65000, n, 0, 1, False)]
    want = [expect(oracle, d[lo:hi], off, seq, 2, 2, fin) for lo, hi, off, seq, fin in ranges]
    a = Arena(engine, room([n], [len(x[0]) for x in want]))
    sp, dp = a.place([(d, 3)], [(len(x[0]), (5 * k + 6) % 16) for k, x in enumerate(want)])
    writes = [fb.write(sp[0] + lo, hi - lo, dp[k], len(want[k][0]), off, seq, fin)
              for k, (lo, hi, off, seq, fin) in enumerate(ranges)]
    assert fb.compose(writes) == [(len(x[0]), x[1]) for x in want]
    a.check([x[0] for x in want])  # the one source and the guards untouched
    assert not np.array_equal(want[0][0][:31], want[1][0][:31])  # the replicas differ in their headers


# ---- 5. a batch of one write is the single fused call ---------------------------------------------------------
@pytest.mark.parametrize("n,off,finish", [(17 * 65536 + 45, 0, False), ((9 << 20) + 321, 4321, True)],
                         ids=["18 packets", "9 MiB + 321 B"])
def test_batch_of_one_equals_the_single_fused_call(engine, fb, wf, oracle, n, off, finish):
    d = payload(95, 0, n)
    stream, recs = expect(oracle, d, off, 100, 2, 2, finish)
    assert len(recs) == 18 or len(recs) > 140
    a = Arena(engine, room([n], [len(stream)] * 2))
    sp, dp = a.place([(d, 3)], [(len(stream), 6), (len(stream), 13)])
    got = fb.compose([fb.write(sp[0], n, dp[0], len(stream), off, 100, finish)])
    single = wf.compose_wire(sp[0], n, dp[1], len(stream), off, 100, 2, 2, finish)
    assert got == [single] and single == (len(stream), recs)
    a.check([stream, stream])


# ---- 6. round trip through the read side -----------------------------------------------------------------
def test_round_trip_through_the_read_side(engine, fb, oracle):
    """The main library's verify kernels check the CRCs this library computed:
    neither this library's arithmetic nor the oracle's decides."""
    n = 5 * 65536 + 1234
    d = payload(96, 0, n + 1000)
    specs = [dict(data=d[n:], seq=50, src_mis=1, dst_mis=2), dict(data=d[:n], seq=0, finish=True, src_mis=5, dst_mis=11)]
    want = expect_all(oracle, specs)
    a = Arena(engine, room([1000, n], [len(x[0]) for x in want]))
    dp = batch(fb, a, specs, want)
    wl = len(want[1][0])
    got = engine.verify_packets(None, dptr=dp[1], nbytes=wl)
    assert got[0] == 0 and got[2] == wl and len(got[1]) == len(want[1][1])
    for v, p in zip(got[1], want[1][1]):
        assert (v["stream_off"], v["offset_in_block"], v["seqno"], v["data_len"], v["crc_len"], v["last"]) == \
            (p["hdr_off"], p["offset_in_block"], p["seqno"], p["data_len"], p["crc_len"], p["last"])
    # one byte of packet 3's chunk 10 flipped on the device
    p3 = want[1][1][3]
    at = p3["hdr_off"] + p3["hdr_len"] + 10 * CS + 100
    a.buf.upload(np.array([want[1][0][at] ^ 0x20], dtype=np.uint8), a.dst[1] + at)
    rc, got, _ = engine.verify_packets(None, dptr=dp[1], nbytes=wl)
    assert rc == engine.ERR_BAD_CHECKSUM
    assert [(i, p["first_bad"], p["bad_chunks"]) for i, p in enumerate(got) if p["error"]] == [(3, 10, 1)]


# ---- 7. refusals: nothing is written anywhere, the text names the entry ------------------------------------
def test_refusals_write_nothing_and_name_the_entry(engine, fb, oracle):
    from hadoofus_amd.abi import OutPacket
    lens = [100000, 0, 70000, 513]
    d = payload(97, 0, sum(lens))
    cut = [d[sum(lens[:k]):sum(lens[:k + 1])] for k in range(4)]
    fin = [True, True, False, True]
    want = [expect(oracle, cut[k], 0, k, 2, 2, fin[k]) for k in range(4)]
    wl = [len(x[0]) for x in want]
    npk = sum(len(x[1]) for x in want)
    a = Arena(engine, room(lens, wl))
    sp, dp = a.place([(cut[k], k + 1) for k in range(4)], [(wl[k], 3 * k + 2) for k in range(4)])
    lib = fb.load()
    arr = (OutPacket * npk)()
    before = bytes(arr)
    cnt = ctypes.c_size_t(0)
    host = np.zeros(max(wl) + 64, dtype=np.uint8)
    end = a.buf.ptr + a.buf.nbytes

    def call(maxp=npk, **kw):
        """kw: {field}{entry}=value, e.g. wire2=..., cap0=..., data3=..."""
        ws = [dict(dptr=sp[k], nbytes=lens[k], wire_ptr=dp[k], wire_cap=wl[k], offset_in_block=0, seqno=k,
                   finish=fin[k]) for k in range(4)]
        for key, v in kw.items():
            ws[int(key[-1])][{"wire": "wire_ptr", "cap": "wire_cap", "data": "dptr"}[key[:-1]]] = v
        e = fb.entries(ws)
        rc = lib.hdfs_wire_fused_batch_compose(e, 4, 2, 2, arr, maxp, ctypes.byref(cnt), None)
        return rc, e, lib.hdfs_wire_fused_batch_last_error().decode()
    cases = {
        "a host wire in entry 3": (dict(wire3=host.ctypes.data), 3),
        "a host source in entry 2": (dict(data2=host.ctypes.data), 2),
        "wire 0 past its allocation": (dict(wire0=end - wl[0] + 1), 0),
        "source 3 past its allocation": (dict(data3=end - lens[3] + 1), 3),
        "wire 2 overlaps wire 0": (dict(wire2=dp[0] + wl[0] - 1), 2),
        "wire 3 inside wire 2": (dict(wire3=dp[2] + 100), 3),
        "wire 2 overlaps data 3": (dict(wire2=sp[3] - wl[2] + 1), 2),
        "wire 3 inside data 0": (dict(wire3=sp[0] + 10), 3),
        "wire 1 (header only) inside data 0": (dict(wire1=sp[0] + lens[0] - 5), 1),
        "wire_cap one byte short in entry 2": (dict(cap2=wl[2] - 1), 2),
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
    a.check([])
    rc, e, err = call()  # and the same arguments, unspoilt, work
    assert rc == 0 and [arr[i].as_dict() for i in range(npk)] == [p for x in want for p in x[1]]
    a.check([x[0] for x in want])


def test_groups_out_of_range_is_einval_and_writes_nothing(engine, fb, oracle):
    specs, want = mixed_specs()[1:3], mixed_want(oracle)[1:3]
    a = Arena(engine, room([len(s["data"]) for s in specs], [len(x[0]) for x in want]))
    writes, _ = placed(fb, a, specs, want)
    lib, ms = fb.load(), ctypes.c_double(0)
    for flags in (fb.time_groups(fb.MAX_GROUPS + 1), fb.time_groups(1 << 20), 1, fb.time_groups(2) | 4):
        assert lib.hdfs_wire_fused_batch_time(fb.entries(writes), 2, 2, 2, flags, 1, ctypes.byref(ms)) == EINVAL
        assert lib.hdfs_wire_fused_batch_last_error()
    a.check([])
    assert fb.fused_batch_time(writes, flags=fb.time_groups(fb.MAX_GROUPS), iters=1) > 0
    a.check([x[0] for x in want])


# ---- 8. streams and threads -----------------------------------------------------------------------------------
def test_sources_filled_on_the_null_stream_just_before(engine, fb, oracle):
    """No synchronisation between the fills (NULL stream) and the call: the
    library's stream waits for the NULL stream."""
    n = 3 << 20
    ds = [payload(98 + k, 0, n) for k in range(2)]
    want = [expect(oracle, ds[k], 4321 * k, k, 2, 2, False) for k in range(2)]
    a = Arena(engine, room([n] * 2, [len(x[0]) for x in want]))
    sp, dp = a.place([(np.zeros(n, np.uint8), 8), (np.zeros(n, np.uint8), 0)],
                     [(len(want[0][0]), 13), (len(want[1][0]), 2)])
    assert all(p % 8 == 0 for p in sp)
    for k in range(2):
        engine.fill_splitmix64(sp[k], n // 8, 98 + k, 0, None)
    got = fb.compose([fb.write(sp[k], n, dp[k], len(want[k][0]), 4321 * k, k) for k in range(2)])
    assert got == [(len(x[0]), x[1]) for x in want]
    for k in range(2):
        a.image[a.src[k]:a.src[k] + n] = ds[k]
    a.check([x[0] for x in want])


def test_on_a_stream_of_the_callers(engine, fb, oracle):
    want = mixed_want(oracle, 1, 1)
    a = mixed_arena(engine, oracle)
    st = engine.stream_create()
    try:
        batch(fb, a, mixed_specs(), want, 1, 1, stream=st)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, fb, oracle):
    jobs = []
    for seed, n, off, proto in [(101, 400000, 0, 2), (102, 250123, 4321, 1)]:
        d = payload(seed, 0, n)
        specs = [dict(data=d, off=off, seq=1, finish=True, src_mis=seed % 4, dst_mis=seed % 16),
                 dict(data=d[:n // 3], off=0, seq=2, src_mis=1, dst_mis=(seed + 5) % 16)]
        want = expect_all(oracle, specs, proto, 2)
        a = Arena(engine, room([len(s["data"]) for s in specs], [len(x[0]) for x in want]))
        jobs.append((a, placed(fb, a, specs, want)[0], proto, want))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, ws, proto, want = jobs[i]
            start.wait()
            for _ in range(4):
                assert fb.compose(ws, proto, 2) == [(len(x[0]), x[1]) for x in want]
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


# ---- 9. the C consumer -----------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "wire_fused_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wire_fused_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wire_fused_batch", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
