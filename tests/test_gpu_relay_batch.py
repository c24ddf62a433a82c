"""GPU: a batch of verified reads re-framed as writes in one call
(include/hadoofus_relay_batch.h) -- probe_relay_kernel frames packet 0 and the
tail of every input stream and sizes the write's stream,
relay_fused_batch_kernel walks the OUTPUT packets of the entries it takes,
loads each round's chunks from their places in the input, stores them as the
write's packets, computes the chunk CRCs once from those registers, compares
them and every input header with the input's and stores them as the output's;
everything else goes to hdfs_crc32c_read_packets and the fused framing kernel
inside the call.

The expected result of every entry is the CPU oracle's verify_packets of its
input plus, where that is clean, the oracle's compose_packets of the payload
(the way tests/test_gpu_wire_fused.py builds its expectation).  Every case is
also compared with hdfs_read_batch_read_blocks followed by
hdfs_wire_fused_batch_compose on the same device bytes.  All streams and all
wire ranges of a batch are carved from one device allocation between 0xA5
guards, at byte residues 0, 1, 5 and 15 mod 16 in shuffled order; after every
call the whole allocation is downloaded and compared with the image expected
(the wire range of an entry whose read found an error is unspecified and not
compared), so the inputs, the guards and a clean entry's room past wire_len are
untouched.  Everything is bit-exact."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from packet_stream import build_stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
GUARD = 0xA5
GAP = 96  # guard bytes before, between and after the ranges (at least)
SLACK = 24  # room of a wire range beyond its stream
RES = (0, 1, 5, 15)
OFFSETS, SEQNOS = (0, 3584, (1 << 31) + 512), (0, 12345)


@pytest.fixture(scope="module")
def rl(engine):
    from hadoofus_read import relay_batch
    relay_batch.load()
    return relay_batch


def stream_of(oracle, proto, ctype, dlens, seed, cs=512, **kw):
    return build_stream(oracle.crc32c, proto, cs, ctype, dlens, seed=seed, **kw)[0]


def _payloads(s, pkts):
    out = bytearray()
    for p in pkts:
        if p["error"]:
            break
        a = p["stream_off"] + p["header_len"] + p["crc_len"]
        out += s[a:a + p["data_len"]]
    return bytes(out)


_reads, _writes = {}, {}


def read_of(oracle, s, proto, ctype, cs=512):
    """The oracle's read of a stream, computed once: (rc, consumed, payload, packet 0's offsetInBlock)."""
    key = (s, proto, ctype, cs)
    if key not in _reads:
        rc, recs, used = oracle.verify_packets(s, proto, cs, ctype)
        _reads[key] = (rc, used, _payloads(s, recs), recs[0]["offset_in_block"] if recs else 0)
    return _reads[key]


def write_of(oracle, pay, off, seq, proto, ctype, finish):
    """The oracle's stream of a write of that payload, computed once: (bytes, packets)."""
    key = (pay, off, seq, proto, ctype, finish)
    if key not in _writes:
        data = np.frombuffer(pay, dtype=np.uint8)
        hdr, pkts = oracle.compose_packets(data, off, seq, proto, ctype, finish)
        hdr = np.frombuffer(hdr, dtype=np.uint8)
        parts = []
        for p in pkts:
            parts.append(hdr[p["hdr_off"]:p["hdr_off"] + p["hdr_len"]])
            parts.append(data[p["data_off"]:p["data_off"] + p["data_len"]])
        _writes[key] = (np.concatenate(parts).tobytes() if parts else b"", len(pkts))
    return _writes[key]


def job(s, off=0, seq=0, finish=False, cap=None):
    """One entry of a case: the input's bytes and the write's arguments (cap: None = the stream's size + SLACK)."""
    return dict(s=s, off=off, seq=seq, finish=finish, cap=cap)


class Arena:
    """One device allocation: guards, then every distinct input stream and every
    wire range in shuffled order, each at its own residue mod 16 with guards
    between.  Identical inputs share one place."""

    def __init__(self, engine, jobs, caps, seed=1):
        streams = list(dict.fromkeys(j["s"] for j in jobs))
        ranges = [("s", k, len(s)) for k, s in enumerate(streams)] + [("w", k, c) for k, c in enumerate(caps)]
        order = np.random.default_rng(seed).permutation(len(ranges))
        self.buf = engine.DeviceBuffer(sum(n + GAP + 32 for _, _, n in ranges) + GAP + 32)
        assert self.buf.ptr % 16 == 0
        at, place = GAP, {}
        for i, r in enumerate(order):
            kind, k, n = ranges[r]
            at = (at + 15) // 16 * 16 + RES[i % len(RES)]
            place[(kind, k)] = at
            at += n + GAP
        assert at <= self.buf.nbytes
        self.src = [place[("s", streams.index(j["s"]))] for j in jobs]
        self.dst = [place[("w", k)] for k in range(len(jobs))]
        self.caps, self.jobs = list(caps), jobs
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        for j, o in zip(jobs, self.src):
            self.image[o:o + len(j["s"])] = np.frombuffer(j["s"], dtype=np.uint8)
        self.buf.upload(self.image)

    def batch(self, rl):
        p = self.buf.ptr
        return [rl.entry(p + self.src[k], len(j["s"]), p + self.dst[k], self.caps[k], j["off"], j["seq"], j["finish"])
                for k, j in enumerate(self.jobs)]

    def check(self, wires):
        """The whole allocation.  wires[k]: the bytes expected at wire range k from
        its start (the rest of its room untouched), or None: the range is unspecified.
        -> the downloaded bytes."""
        want, got = self.image.copy(), self.buf.download()
        raw = got.copy()
        for o, cap, w in zip(self.dst, self.caps, wires):
            if w is None:
                got[o:o + cap] = GUARD
            else:
                want[o:o + len(w)] = np.frombuffer(w, dtype=np.uint8)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (streams {self.src[:8]}, wire ranges "
                                 f"{self.dst[:8]}): got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")
        return raw


def expectation(oracle, jobs, proto, ctype, cs=512):
    """Per entry: (rc, consumed, delivered, src_offset_in_block, wire bytes or None, npkts)."""
    out = []
    for j in jobs:
        rc, used, pay, off0 = read_of(oracle, j["s"], proto, ctype, cs)
        wire, npk = write_of(oracle, pay, j["off"], j["seq"], proto, ctype, j["finish"]) if rc == 0 else (None, 0)
        out.append((rc, used, len(pay), off0, wire, npk))
    return out


def two_calls(engine, a, jobs, want, got_img, proto, ctype, cs):
    """The parent's way on the same device bytes: hdfs_read_batch_read_blocks into a
    buffer, then hdfs_wire_fused_batch_compose of it; the relay's bytes must be the same."""
    from hadoofus_amd import wire_fused_batch as fb
    from hadoofus_read import read_batch as rb
    n, p = len(jobs), a.buf.ptr
    room = [len(j["s"]) for j in jobs]
    pay = engine.DeviceBuffer(sum(room) + 16 * n + 16)
    at = [sum(room[:k]) + 16 * k for k in range(n)]
    reads = rb.read_blocks([rb.entry(p + a.src[k], room[k], pay.ptr + at[k], room[k]) for k in range(n)], proto, cs,
                           ctype)
    assert [(r["rc"], r["consumed"], r["delivered"]) for r in reads] == [w[:3] for w in want]
    clean = [k for k in range(n) if want[k][0] == 0 and want[k][4]]  # the entries that have a stream
    if not clean:
        return
    sizes = [len(want[k][4]) for k in clean]
    out = engine.DeviceBuffer(sum(sizes) + 16 * len(clean) + 16)
    oat = [sum(sizes[:i]) + 16 * i + 3 for i in range(len(clean))]
    res = fb.compose([fb.write(pay.ptr + at[k], want[k][2], out.ptr + oat[i], sizes[i], jobs[k]["off"], jobs[k]["seq"],
                               jobs[k]["finish"]) for i, k in enumerate(clean)], proto, ctype)
    img = out.download()
    for i, k in enumerate(clean):
        assert res[i][0] == sizes[i], k
        assert np.array_equal(img[oat[i]:oat[i] + sizes[i]], got_img[a.dst[k]:a.dst[k] + sizes[i]]), k


def run(rl, engine, oracle, jobs, proto=2, ctype=2, cs=512, groups=None, stream=None, paths=None, second=True, seed=1):
    """Places the inputs and the wire ranges, relays the batch (groups: through
    the timing entry with that many workgroups), checks every entry against its
    expectation and the whole arena, then the two-call comparison.  -> the results."""
    want = expectation(oracle, jobs, proto, ctype, cs)
    caps = [(len(w[4]) if w[4] is not None else 64) + SLACK if j["cap"] is None else j["cap"] for j, w in zip(jobs, want)]
    a = Arena(engine, jobs, caps, seed)
    if groups is None:
        got = rl.relay(a.batch(rl), proto, cs, ctype, stream)
    else:
        ms, got = rl.time(a.batch(rl), proto, cs, ctype, rl.time_groups(groups), 1)
        assert ms > 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["rc"], g["consumed"], g["delivered"], g["src_offset_in_block"]) == w[:4], (k, g, w[:4])
        assert (g["wire_len"], g["npkts"]) == ((len(w[4]), w[5]) if w[0] == 0 else (0, 0)), (k, g)
        if paths is not None and paths[k] is not None:
            assert g["path"] == paths[k], (k, g["path"])
    img = a.check([w[4] for w in want])
    if second:
        two_calls(engine, a, jobs, want, img, proto, ctype, cs)
    return got


# ---- 1. the smallest shapes at which the kernel can go wrong ------------------------------------------------
def shapes(oracle, proto, ctype):
    s = lambda dl, seed, **kw: stream_of(oracle, proto, ctype, dl, seed, **kw)  # noqa: E731
    return [s([512], 10),                                        # one chunk, one round, one packet each side
            s([512] * 20, 11),                                   # eight input packets under one round, 20 headers
            s([5120] * 3 + [1300], 12),                          # a seam inside round 1; a ragged chunk of 276 B
            s([64512] * 3 + [700], 13),                          # stock HDFS: three output packets, ragged 188 B
            s([65536] * 2 + [700], 14, last_empty=False),        # no seam; no lastPacketInBlock packet behind
            s([4096] * 2, 15, last_empty=False)[:-1000]]         # the walk ends ahead of an incomplete packet


@pytest.mark.parametrize("ctype", [2, 1])
@pytest.mark.parametrize("proto", [1, 2])
def test_every_shape_takes_the_kernel_path(engine, rl, oracle, proto, ctype):
    """Six input shapes, each written at three block offsets on the chunk grid,
    two sequence numbers, with and without finish: 72 entries, one call, every
    one served by the kernel."""
    ss = shapes(oracle, proto, ctype)
    assert read_of(oracle, ss[5], proto, ctype)[1] < len(ss[5])  # consumed < len
    jobs = [job(s, off, seq, fin) for s in ss for off in OFFSETS for seq in SEQNOS for fin in (False, True)]
    run(rl, engine, oracle, jobs, proto, ctype, paths=[rl.PATH_KERNEL] * len(jobs))


def test_an_unaligned_write_takes_the_fallback(engine, rl, oracle):
    """offset_in_block = 4321: the write's first packet completes its chunk; the
    bytes are hdfs_wire_fused_compose_packets' of the payload."""
    from hadoofus_amd import wire_fused as wf
    ss = shapes(oracle, 2, 2)
    jobs = [job(ss[2], 4321, 5, True), job(ss[3], 0, 0, True), job(ss[3], 4321, 9, False)]
    K, F = rl.PATH_KERNEL, rl.PATH_FALLBACK
    want = expectation(oracle, jobs, 2, 2)
    a = Arena(engine, jobs, [len(w[4]) + SLACK for w in want])
    got = rl.relay(a.batch(rl))
    assert [g["path"] for g in got] == [F, K, F] and [g["wire_len"] for g in got] == [len(w[4]) for w in want]
    img = a.check([w[4] for w in want])
    for k in (0, 2):
        pay = np.frombuffer(read_of(oracle, jobs[k]["s"], 2, 2)[2], dtype=np.uint8)
        src, out = engine.DeviceBuffer(len(pay)), engine.DeviceBuffer(len(want[k][4]))
        src.upload(pay)
        wl, _ = wf.compose_wire(src.ptr, len(pay), out.ptr, out.nbytes, 4321, jobs[k]["seq"], 2, 2, jobs[k]["finish"])
        assert wl == got[k]["wire_len"] and np.array_equal(out.download(), img[a.dst[k]:a.dst[k] + wl]), k


def test_syncblock_headers_in_plain_headers_out(engine, rl, oracle):
    """A v2 input whose headers carry syncBlock (33 B) is written with the
    writer's 31-byte headers."""
    s = stream_of(oracle, 2, 2, [8192] * 5 + [100], 20, sync_every=1)
    got = run(rl, engine, oracle, [job(s, 512, 3, True), job(s, 0, 0, False)], paths=[rl.PATH_KERNEL] * 2)
    assert got[0]["npkts"] == 2 and got[0]["wire_len"] == 2 * 31 + 4 * 81 + 5 * 8192 + 100


# ---- 2. corruption in one entry of five ---------------------------------------------------------------------
def _flip(s, at, mask=0x04):
    b = bytearray(s)
    b[at] ^= mask
    return bytes(b)


@pytest.mark.parametrize("what", ["full chunk in a seamed round", "ragged chunk", "crc byte", "seqno of a middle header",
                                  "dlen of a middle header"])
@pytest.mark.parametrize("proto", [1, 2])
def test_one_corrupt_entry_of_five_falls_back_alone(engine, rl, oracle, proto, what):
    ss = [stream_of(oracle, proto, 2, [5120] * 3 + [1300], 40 + k) for k in range(5)]
    recs = oracle.verify_packets(ss[2], proto, 512, 2)[1]
    at = lambda i: recs[i]["stream_off"]  # noqa: E731
    data = lambda i: at(i) + recs[i]["header_len"] + recs[i]["crc_len"]  # noqa: E731
    where = {"full chunk in a seamed round": data(1) + 1 * 512 + 77,  # payload chunk 11: round 1 holds chunks 8..15
             "ragged chunk": data(3) + 2 * 512 + 30,
             "crc byte": at(2) + recs[2]["header_len"] + 4 * 9 + 2,
             "seqno of a middle header": at(1) + (12 + 7 if proto == 1 else 6 + 10),
             "dlen of a middle header": at(1) + (21 + 3 if proto == 1 else 6 + 21)}[what]
    ss[2] = _flip(ss[2], where)
    paths = [rl.PATH_KERNEL] * 5
    paths[2] = rl.PATH_FALLBACK
    got = run(rl, engine, oracle, [job(s, 512 * k, k, k % 2 == 0) for k, s in enumerate(ss)], proto, 2, paths=paths)
    bad = got[2]
    if what in ("full chunk in a seamed round", "ragged chunk", "crc byte"):
        assert bad["rc"] == engine.ERR_BAD_CHECKSUM and bad["wire_len"] == 0 and bad["npkts"] == 0
        assert bad["delivered"] == {"full chunk in a seamed round": 5120, "ragged chunk": 3 * 5120,
                                    "crc byte": 2 * 5120}[what]
    elif what == "seqno of a middle header":  # framing-clean: the read succeeds, and the write is made of its payload
        assert bad["rc"] == 0 and bad["delivered"] == 3 * 5120 + 1300 and bad["wire_len"] > bad["delivered"]
    else:
        assert bad["rc"] != 0 and bad["delivered"] == 5120 and bad["wire_len"] == 0


# ---- 3. irregular entries among regular ones -----------------------------------------------------------------
def test_irregular_entries_among_regular_ones(engine, rl, oracle):
    reg = lambda k: stream_of(oracle, 2, 2, [65536] * 2 + [3000], 50 + k)  # noqa: E731
    only_empty = stream_of(oracle, 2, 2, [], 51)
    jobs = [job(reg(0), 0, 0, True),
            job(only_empty, 512, 4, True),                                   # one header-only packet
            job(only_empty, 512, 4, False),                                  # nothing
            job(stream_of(oracle, 2, 2, [40000] * 5, 54), 0, 1, True),       # partial chunks in every packet
            job(stream_of(oracle, 2, 2, [65536, 4096, 65536], 55), 0, 2, False),  # a size break
            job(reg(5), 3584, 7, False)]
    K, F = rl.PATH_KERNEL, rl.PATH_FALLBACK
    got = run(rl, engine, oracle, jobs, paths=[K, F, F, F, F, K])
    assert [(g["wire_len"], g["npkts"]) for g in got[1:3]] == [(31, 1), (0, 0)]


def test_chunk_size_4096_is_the_main_librarys(engine, rl, oracle):
    jobs = [job(stream_of(oracle, 2, 2, dl, 60 + k, cs=4096), 0, k, True) for k, dl in enumerate([[65536] * 2 + [5000],
                                                                                                 [8192]])]
    # chunk_size is the read's; the write's chunk is 512 whatever the read's was
    run(rl, engine, oracle, jobs, cs=4096, paths=[rl.PATH_FALLBACK] * 2)


# ---- 4. limits --------------------------------------------------------------------------------------------
def test_a_wire_range_one_byte_short(engine, rl, oracle):
    """That entry's rc is EINVAL with the entry named, nothing is written outside
    its wire range and the others are served."""
    ss = [stream_of(oracle, 2, 2, [64512, 64512, 999], 70 + k) for k in range(3)]
    jobs = [job(s, 0, k, True) for k, s in enumerate(ss)]
    want = expectation(oracle, jobs, 2, 2)
    caps = [len(w[4]) + SLACK for w in want]
    caps[1] = len(want[1][4]) - 1
    a = Arena(engine, jobs, caps)
    got = rl.relay(a.batch(rl))
    assert [g["rc"] for g in got] == [0, EINVAL, 0] and got[1]["path"] == rl.PATH_FALLBACK
    assert (got[1]["wire_len"], got[1]["npkts"]) == (0, 0)
    assert (got[1]["consumed"], got[1]["delivered"]) == want[1][1:3]  # the read itself was clean
    assert b"entry 1" in rl.load().hdfs_relay_batch_last_error()
    assert [g["path"] for g in got[::2]] == [rl.PATH_KERNEL] * 2
    a.check([want[0][4], None, want[2][4]])  # entry 1's range is unspecified, everything around it is not


# ---- 5. many packets per workgroup ------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 3, 7])
def test_few_workgroups_walk_many_packets(engine, rl, oracle, groups):
    ss = shapes(oracle, 2, 2) + [stream_of(oracle, 2, 2, [64512] * 20 + [5], 90)]
    jobs = [job(s, OFFSETS[k % 3], k, k % 2 == 1) for k, s in enumerate(ss)]
    run(rl, engine, oracle, jobs, groups=groups, paths=[rl.PATH_KERNEL] * len(jobs), second=groups == 3)


def test_groups_out_of_range_is_einval_and_writes_nothing(engine, rl, oracle):
    jobs = [job(stream_of(oracle, 2, 2, [4096] * 3, 91), 0, 0, True)]
    want = expectation(oracle, jobs, 2, 2)
    a = Arena(engine, jobs, [len(want[0][4]) + SLACK])
    lib, ms = rl.load(), ctypes.c_double(0)
    for flags in (rl.time_groups(rl.MAX_GROUPS + 1), rl.time_groups(1 << 20), 1, rl.time_groups(2) | 4):
        assert lib.hdfs_relay_batch_time(rl.entries(a.batch(rl)), 1, 2, 512, 2, flags, 1, ctypes.byref(ms)) == EINVAL
        assert b"workgroups" in lib.hdfs_relay_batch_last_error()
    a.check([b""])
    ms, got = rl.time(a.batch(rl), flags=rl.time_groups(rl.MAX_GROUPS), iters=1)
    assert ms > 0 and got[0]["path"] == rl.PATH_KERNEL
    a.check([want[0][4]])


# ---- 6. other behaviour ---------------------------------------------------------------------------------------------
def test_streams_copied_on_the_null_stream_just_before(engine, rl, oracle):
    """No synchronisation between the device-to-device copies that put the
    inputs in place (NULL stream) and the call: the library's stream waits for
    the NULL stream."""
    ss = [stream_of(oracle, 2, 2, [64512] * 30 + [777], 100 + k) for k in range(2)]
    real = [job(s, 512, k, True) for k, s in enumerate(ss)]
    want = expectation(oracle, real, 2, 2)
    stage = engine.DeviceBuffer(sum(len(s) for s in ss))
    stage.upload(np.frombuffer(b"".join(ss), dtype=np.uint8))
    zeros = [job(bytes([k]) * len(s), 512, k, True) for k, s in enumerate(ss)]  # placeholders where the inputs go
    a = Arena(engine, zeros, [len(w[4]) + SLACK for w in want])
    engine.device_sync()
    lib, at = engine.load(), 0
    for k, s in enumerate(ss):
        assert lib.hdfs_crc32c_memcpy(a.buf.ptr + a.src[k], stage.ptr + at, len(s), 2) == 0
        at += len(s)
    got = rl.relay(a.batch(rl))
    assert [(g["rc"], g["wire_len"], g["path"]) for g in got] == [(0, len(w[4]), rl.PATH_KERNEL) for w in want]
    for k, s in enumerate(ss):
        a.image[a.src[k]:a.src[k] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    a.check([w[4] for w in want])


def test_on_a_stream_of_the_callers(engine, rl, oracle):
    st = engine.stream_create()
    try:
        ss = shapes(oracle, 1, 2)
        run(rl, engine, oracle, [job(s, 3584, 12345, True) for s in ss] + [job(ss[2], 4321, 1, True)], 1, 2, stream=st)
    finally:
        assert engine.load().hdfs_crc32c_stream_destroy(st) == 0


def test_two_threads_at_once(engine, rl, oracle):
    work = []
    for seed, dl, proto in [(110, [64512] * 5 + [900], 2), (111, [5120] * 30, 1)]:
        ss = [stream_of(oracle, proto, 2, dl, seed + 10 * k) for k in range(3)]
        ss[1] = _flip(ss[1], len(ss[1]) // 2)  # one entry of each batch falls back
        jobs = [job(s, 512, k, True) for k, s in enumerate(ss)]
        want = expectation(oracle, jobs, proto, 2)
        a = Arena(engine, jobs, [(len(w[4]) if w[4] is not None else 64) + SLACK for w in want], seed)
        work.append((a, proto, want))
    errors = []
    start = threading.Barrier(2)

    def go(i):
        try:
            a, proto, want = work[i]
            start.wait()
            for _ in range(4):
                got = rl.relay(a.batch(rl), proto)
                assert [(g["rc"], g["consumed"], g["delivered"], g["wire_len"]) for g in got] == \
                    [(w[0], w[1], w[2], len(w[4]) if w[0] == 0 else 0) for w in want]
        except BaseException as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for a, _, want in work:
        a.check([w[4] for w in want])


def test_refusals_leave_the_arena_untouched_and_name_the_entry(engine, rl, oracle):
    ss = [stream_of(oracle, 2, 2, [4096] * 3, 120 + k) for k in range(4)]
    jobs = [job(s, 512, k, True) for k, s in enumerate(ss)]
    want = expectation(oracle, jobs, 2, 2)
    a = Arena(engine, jobs, [len(w[4]) + SLACK for w in want])
    lib, p, end = rl.load(), a.buf.ptr, a.buf.ptr + a.buf.nbytes
    host = np.zeros(1 << 16, dtype=np.uint8)
    names = {"stream": "stream_ptr", "len": "nbytes", "wire": "wire_ptr", "cap": "wire_cap", "off": "offset_in_block",
             "seq": "seqno"}

    def call(n=4, proto=2, cs=512, ctype=2, **kw):
        """kw: {field}{entry}=value, e.g. wire2=..., stream0=..., len3=..."""
        b = a.batch(rl)
        for key, v in kw.items():
            b[int(key[-1])][names[key[:-1]]] = v
        arr = rl.entries(b) if n <= 4 else (rl.Entry * n)()
        rc = lib.hdfs_relay_batch_relay(arr, n, proto, cs, ctype, None)
        if rc == EINVAL:  # a refusal: every out field zero
            assert all((e.rc, e.consumed, e.delivered, e.wire_len, e.npkts) == (0, 0, 0, 0, 0) for e in arr[:min(n, 4)])
        return rc, lib.hdfs_relay_batch_last_error().decode()
    # (kw, text, exact): exact texts are asserted whole, the others as a part.  Of the overlap cases "inside stream 1"
    # provokes exactly one overlapping pair.  The other two provoke two each, of which one is named: a range of this
    # size laid over the last byte of wire 0 reaches over the guard bytes into stream 2, its neighbour in the shuffled arena, as well, and one laid back from
    # the first byte of stream 1 reaches into stream 0 as well.
    cases = {
        "a host stream in entry 3": (dict(stream3=host.ctypes.data), "entry 3", False),
        "a host wire range in entry 2": (dict(wire2=host.ctypes.data), "entry 2", False),
        "stream 0 past its allocation": (dict(stream0=end - len(ss[0]) + 1), "entry 0", False),
        "wire range 3 past its allocation": (dict(wire3=end - a.caps[3] + 1), "entry 3", False),
        "wire range 2 overlaps wire range 0": (dict(wire2=p + a.dst[0] + a.caps[0] - 1), "entry 2", False),
        "wire range 3 inside stream 1": (dict(wire3=p + a.src[1] + 10), "entry 3: wire overlaps the stream of entry 1", True),
        "wire range 1 overlaps its own stream": (dict(wire1=p + a.src[1] - a.caps[1] + 1), "entry 1", False),
        "a negative block offset in entry 2": (dict(off2=-512), "entry 2", False),
        "a negative seqno in entry 1": (dict(seq1=-1), "entry 1", False),
        "chunk_size 0": (dict(cs=0), "chunk_size", False),
        "CSUM_NULL": (dict(ctype=0), "CRC32", False),
        "proto 3": (dict(proto=3), "proto", False),
        "no entries": (dict(n=0), "no entries", False),
        "too many entries": (dict(n=rl.MAX_ENTRIES + 1), "1024", False),
    }
    for name, (kw, text, exact) in cases.items():
        rc, err = call(**kw)
        assert rc == EINVAL and (err == text if exact else text in err), (name, err)
        assert not host.any(), name
    a.check([b""] * 4)
    rc, err = call()  # and the same arguments, unspoilt, work
    assert rc == 0
    a.check([w[4] for w in want])
    # identical and overlapping input streams are allowed
    run(rl, engine, oracle, [job(ss[0], 0, 0, True), job(ss[0], 512, 9, False)], paths=[rl.PATH_KERNEL] * 2)


# ---- 7. round trip ---------------------------------------------------------------------------------------------------
def test_round_trip_and_one_large_entry(engine, rl, oracle):
    """One entry of 8 MiB + 777 B in stock 64 512-byte packets beside two small
    ones.  The relay's output, read back by hdfs_read_batch_read_blocks, is the
    input's payload; and the block CRC hdfs_crc_streams_block_crcs takes from
    the output stream is the one it takes from the input: neither this library's
    CRC code nor the oracle's framing decides."""
    from hadoofus_read import crc_streams as cs
    from hadoofus_read import read_batch as rb
    n = (8 << 20) + 777
    big = [64512] * (n // 64512) + [n % 64512]
    ss = [stream_of(oracle, 2, 2, big, 130), stream_of(oracle, 2, 2, [5120] * 7 + [1], 131),
          stream_of(oracle, 2, 2, [512], 132)]
    jobs = [job(s, 0, 3 * k, True) for k, s in enumerate(ss)]
    want = expectation(oracle, jobs, 2, 2)
    assert want[0][2] == n
    a = Arena(engine, jobs, [len(w[4]) + SLACK for w in want])
    got = rl.relay(a.batch(rl))
    assert [(g["rc"], g["delivered"], g["wire_len"], g["path"]) for g in got] == \
        [(0, w[2], len(w[4]), rl.PATH_KERNEL) for w in want]
    a.check([w[4] for w in want])
    p = a.buf.ptr
    back = engine.DeviceBuffer(sum(w[2] for w in want) + 3 * 64)
    at = [sum(w[2] for w in want[:k]) + 64 * k + (1, 0, 5)[k] for k in range(3)]
    reads = rb.read_blocks([rb.entry(p + a.dst[k], got[k]["wire_len"], back.ptr + at[k], want[k][2]) for k in range(3)])
    assert [(r["rc"], r["consumed"], r["delivered"]) for r in reads] == \
        [(0, got[k]["wire_len"], want[k][2]) for k in range(3)]
    assert reads[0]["path"] == rb.PATH_KERNEL  # (a single packet that is no whole number of chunks is the main library's)
    img = back.download()
    for k in range(3):
        assert img[at[k]:at[k] + want[k][2]].tobytes() == read_of(oracle, ss[k], 2, 2)[2], k
    crc_in = cs.block_crcs([cs.entry(p + a.src[k], len(ss[k])) for k in range(3)])
    crc_out = cs.block_crcs([cs.entry(p + a.dst[k], got[k]["wire_len"]) for k in range(3)])
    assert [(c["rc"], c["crc"], c["payload"]) for c in crc_in] == [(c["rc"], c["crc"], c["payload"]) for c in crc_out]
    assert all(c["rc"] == 0 for c in crc_in) and crc_in[0]["payload"] == n


def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "relay_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "relay_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_relay_batch", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr


# ---- a batch at the limit ---------------------------------------------------------------------------------------------
def test_a_batch_at_the_limit_is_swept_and_refused_by_name(engine, rl, oracle):
    """1 024 entries of one 512-byte packet and the empty last packet in one
    arena, the wire ranges in falling address order, so the overlap sweep has
    to sort; then one wire range at a time is moved onto another range."""
    n = rl.MAX_ENTRIES
    kinds = [stream_of(oracle, 2, 2, [512], 300 + k) for k in range(8)]  # entry k relays kinds[k % 8]
    wires = [write_of(oracle, read_of(oracle, s, 2, 2)[2], 0, 0, 2, 2, True)[0] for s in kinds]
    slen, wlen = len(kinds[0]), len(wires[0])
    assert n == 1024 and all(len(s) == slen for s in kinds) and all(len(w) == wlen for w in wires)
    cap = wlen + SLACK
    # behind every stream, room for a wire range laid 8 bytes into it, and 16 guard bytes at least behind every range
    spitch, dpitch = (max(slen, 8 + cap) + 16 + 15) // 16 * 16, cap + 16
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
        return [rl.entry(p + src[k], slen, p + moved.get(f"wire{k}", dst[k]), cap, 0, 0, True) for k in range(n)]
    got = rl.relay(batch(), 2, 512, 2)
    assert [(g["rc"], g["consumed"], g["delivered"], g["wire_len"]) for g in got] == [(0, slen, 512, wlen)] * n
    for k in range(n):
        image[dst[k]:dst[k] + wlen] = np.frombuffer(wires[k % 8], dtype=np.uint8)
    held = buf.download()
    assert np.array_equal(held, image)
    # Where the moved wire range overlaps nothing else.  8 bytes into entry 0's wire range, the highest range of the
    # arena: it ends 8 bytes into the 16 guard bytes behind that, ahead of the arena's last GAP bytes.  8 bytes into
    # a stream: it ends at most 8 + cap bytes behind the stream's start, and the next stream starts 16 bytes
    # further at least (spitch).  Its own place stays empty.
    assert 8 + cap + 16 <= spitch and dst[0] + 8 + cap <= buf.nbytes
    lib = rl.load()
    for moved, text in ((dict(wire1023=dst[0] + 8), "entry 1023: wire overlaps the wire of entry 0"),
                        (dict(wire5=src[900] + 8), "entry 5: wire overlaps the stream of entry 900"),
                        (dict(wire7=src[7] + 8), "entry 7: wire overlaps the stream of entry 7")):
        rc = lib.hdfs_relay_batch_relay(rl.entries(batch(**moved)), n, 2, 512, 2, None)
        assert rc == EINVAL and lib.hdfs_relay_batch_last_error().decode() == text, text
        assert np.array_equal(buf.download(), held), text
