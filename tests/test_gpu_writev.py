"""GPU: gather writes (include/hadoofus_writev.h) -- the packets of a write held
in a list of device buffers, composed where the fragments lie: in-place
segments of one compute plan plus gather_chunks_kernel for the chunks that
cross a fragment boundary.

The expected value everywhere is the CPU oracle on the fragments'
concatenation, oracle.compose_packets(b"".join(frags), ...): the reference's
loop carries `crc` across iovecs (src/datanode.c:2840-2855), so chaining over
fragments and the CRC of the concatenation are the same thing; one test also
compares a packet's CRC bytes with oracle.compose_crcs(iovecs), the direct
restatement of that loop.  Device fragments are carved from one allocation
with 0xA5 guard gaps between them, at chosen misalignments; after every call
the allocation is downloaded and compared with its upload, and the header
buffer's 64 guard bytes past hdr_used are checked.  Everything is bit-exact."""
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
GUARD, HGUARD = 0xA5, 0xEE


@pytest.fixture(scope="module")
def wv(engine):
    from hadoofus_amd import writev
    writev.load()
    return writev


class Arena:
    """Fragments of `data` (lengths lens) carved from one device allocation:
    fragment i starts `mis[i % len(mis)]` bytes past a 16-byte boundary, 64 to
    79 guard bytes of 0xA5 lie before, between and after them."""

    def __init__(self, engine, data, lens, mis=(0,)):
        assert sum(lens) == len(data)
        pos, at = 64, []
        for i, n in enumerate(lens):
            pos = (pos + 15) // 16 * 16 + mis[i % len(mis)]
            at.append(pos)
            pos += n + 64
        self.image = np.full(pos + 16, GUARD, dtype=np.uint8)
        src = 0
        for a, n in zip(at, lens):
            self.image[a:a + n] = data[src:src + n]
            src += n
        self.buf = engine.DeviceBuffer(self.image.nbytes)
        self.buf.upload(self.image)
        self.frags = [(self.buf.ptr + a, n) for a, n in zip(at, lens)]
        self.at = at

    def untouched(self):
        return np.array_equal(self.buf.download(), self.image)


def compose(wv, frags, off=0, seq=0, proto=2, ctype=2, finish=False):
    """hdfs_writev_compose_packets with a header buffer that has 64 guard
    bytes past hdr_used.  -> (header bytes, [packet dicts])."""
    from hadoofus_amd.abi import OutPacket
    lib = wv.load()
    vec, n, keep = wv.iovecs(frags)
    npk, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    args = (vec, n, off, seq, proto, ctype, int(finish))
    assert lib.hdfs_writev_compose_packets(*args, None, 0, None, 0, ctypes.byref(npk), ctypes.byref(used)) == 0
    want_n, want_used = npk.value, used.value
    hdr = np.full(want_used + 64, HGUARD, dtype=np.uint8)
    arr = (OutPacket * (want_n + 1))()
    rc = lib.hdfs_writev_compose_packets(*args, hdr.ctypes.data, want_used, arr, want_n, ctypes.byref(npk),
                                         ctypes.byref(used))
    assert rc == 0, lib.hdfs_writev_last_error()
    assert (npk.value, used.value) == (want_n, want_used)
    assert (hdr[want_used:] == HGUARD).all(), "header guard bytes written"
    return hdr[:want_used].tobytes(), [arr[i].as_dict() for i in range(want_n)]


def cuts(total, points):
    p = [0] + list(points) + [total]
    return [b - a for a, b in zip(p[:-1], p[1:])]


# ---- one fragment ------------------------------------------------------------------
def test_single_fragment_is_compose_packets(engine, wv, oracle):
    d = payload(31, 0, 300 * CS + 45)
    a = Arena(engine, d, [len(d)], mis=(3,))
    for off, proto, ctype, finish in [(0, 2, 2, True), (4321, 1, 1, False), (77, 2, 0, True)]:
        got = compose(wv, a.frags, off, 5, proto, ctype, finish)
        assert got == engine.compose_packets(None, off, 5, proto, ctype, finish, dptr=a.frags[0][0], nbytes=len(d))
        assert got == oracle.compose_packets(d, off, 5, proto, ctype, finish)
    assert a.untouched()


# ---- two fragments -------------------------------------------------------------------
TWO_LEN = 200 * 1024 + 123
TWO_DATA = payload(32, 0, TWO_LEN)
_two_want = {}


def _two_expected(oracle, off, proto, ctype, finish):
    key = (off, proto, ctype, finish)
    if key not in _two_want:
        _two_want[key] = oracle.compose_packets(TWO_DATA, off, 9, proto, ctype, finish)
    return _two_want[key]


@pytest.mark.parametrize("off", [0, 4321])
@pytest.mark.parametrize("split", [CS * 100, CS * 100 + 1, CS * 100 + 511, 1, 200, TWO_LEN - 1],
                         ids=["512k", "512k+1", "512k+511", "1", "200", "len-1"])
def test_two_fragments(engine, wv, oracle, split, off):
    """At block offset 4321 the short first chunk (287 bytes) crosses the
    split when the split is 1 or 200."""
    a = Arena(engine, TWO_DATA, [split, TWO_LEN - split], mis=(1, 2))
    info = wv.layout([split, TWO_LEN - split], off)
    assert info["seg_chunks"] + info["ngathered"] == info["nchunks"] and info["nsegments"] >= 1
    for ctype in (engine.CSUM_CRC32C, engine.CSUM_CRC32):
        for proto in (1, 2):
            for finish in (False, True):
                got = compose(wv, a.frags, off, 9, proto, ctype, finish)
                assert got == _two_expected(oracle, off, proto, ctype, finish), (ctype, proto, finish)
    assert a.untouched()


def test_packet_crcs_are_the_fragment_chained_loop(engine, wv, oracle):
    """The CRC bytes of the write's first packet against the reference's own
    loop over the iovecs (src/datanode.c:2836-2859)."""
    split = CS * 3 + 17
    a = Arena(engine, TWO_DATA, [split, TWO_LEN - split], mis=(3, 1))
    hdr, pkts = compose(wv, a.frags, 0, 0, 2, engine.CSUM_CRC32C, False)
    p = pkts[0]
    assert p["data_len"] == 65536 and p["crc_len"] == 128 * 4
    crcs = hdr[p["hdr_off"] + p["hdr_len"] - p["crc_len"]:p["hdr_off"] + p["hdr_len"]]
    assert crcs == oracle.compose_crcs([TWO_DATA[:split], TWO_DATA[split:65536]])
    assert a.untouched()


# ---- odd addresses ---------------------------------------------------------------------
def test_odd_addresses_engage_both_paths(engine, wv, oracle):
    total = 9 << 20
    lens = cuts(total, [1887437, 3774873 + 2, 5662311 + 3, 7549747])
    assert all(n % 4 for n in lens[:4]) and len(lens) == 5
    d = payload(33, 0, total)
    a = Arena(engine, d, lens, mis=(1, 2, 3, 1, 3))
    assert all(p % 16 in (1, 2, 3) for p, _ in a.frags)
    info = wv.layout(lens, 0)
    assert info["nsegments"] >= 5 and info["ngathered"] >= 4, info
    for off, ctype in [(0, engine.CSUM_CRC32C), (4321, engine.CSUM_CRC32)]:
        assert compose(wv, a.frags, off, 0, 2, ctype, True) == oracle.compose_packets(d, off, 0, 2, ctype, True)
    assert a.untouched()


# ---- tiny fragments ----------------------------------------------------------------------
def test_tiny_fragments_are_all_gathered(engine, wv, oracle):
    total = 64 * 1024 + 77
    rng = np.random.default_rng(34)
    lens, left = [], total
    while left:
        n = 0 if rng.integers(0, 6) == 0 else int(min(left, rng.integers(1, 101)))
        lens.append(n)
        left -= n
    assert 0 in lens
    d = payload(34, 0, total)
    a = Arena(engine, d, lens, mis=(0, 1, 2, 3, 5, 7, 11, 13))
    for off in (0, 4321):
        info = wv.layout(lens, off)
        assert info["seg_chunks"] == 0 and info["ngathered"] == info["nchunks"] and info["max_pieces"] > 5
        for ctype in (engine.CSUM_CRC32C, engine.CSUM_CRC32):
            assert compose(wv, a.frags, off, 1, 2, ctype, True) == oracle.compose_packets(d, off, 1, 2, ctype, True)
    assert a.untouched()


def test_seven_hundred_one_byte_fragments(engine, wv, oracle):
    d = payload(35, 0, 700)
    a = Arena(engine, d, [1] * 700, mis=(0, 1, 2, 3))
    assert wv.layout([1] * 700, 0)["max_pieces"] == 512
    for off in (0, 300):
        assert compose(wv, a.frags, off, 0, 2, 2, True) == oracle.compose_packets(d, off, 0, 2, 2, True)
    assert a.untouched()


# ---- the partial last chunk ------------------------------------------------------------------
def test_partial_last_chunk_crosses_a_boundary(engine, wv, oracle):
    d = payload(36, 0, 5300)
    a = Arena(engine, d, [5000, 300, 0], mis=(2, 3, 0))  # last chunk [4608, 5300) crosses byte 5000
    for off in (0, 4321):
        assert compose(wv, a.frags, off, 0, 2, 2, True) == oracle.compose_packets(d, off, 0, 2, 2, True)
    assert a.untouched()


def test_less_than_a_chunk_in_three_fragments(engine, wv, oracle):
    d = payload(37, 0, 401)
    a = Arena(engine, d, [100, 1, 300], mis=(1, 1, 2))
    for off in (0, 4321, 511):
        for ctype in (1, 2):
            assert compose(wv, a.frags, off, 0, 1, ctype, False) == oracle.compose_packets(d, off, 0, 1, ctype, False)
    assert a.untouched()


def test_empty_write_with_finish_is_the_last_packet_only(engine, wv, oracle):
    a = Arena(engine, payload(38, 0, 0), [0, 0])
    hdr, pkts = compose(wv, a.frags, 1024, 4, 2, 2, True)
    assert (hdr, pkts) == oracle.compose_packets(b"", 1024, 4, 2, 2, True)
    assert len(pkts) == 1 and pkts[0]["last"] == 1 and pkts[0]["data_len"] == 0
    assert a.untouched()


# ---- host fragments -------------------------------------------------------------------------
def test_host_fragments(engine, wv, oracle):
    total = (1 << 20) + 5
    d = payload(39, 0, total)
    pts = [1, 70000, 70001, 500000, 777777, total - 3]
    frags = [d[a:b].copy() for a, b in zip([0] + pts, pts + [total])]
    assert len(frags) == 7
    for off, ctype in [(0, 2), (4321, 1)]:
        assert compose(wv, frags, off, 2, 2, ctype, True) == oracle.compose_packets(d, off, 2, 2, ctype, True)


def test_host_fragments_across_a_window(engine, wv, oracle):
    total = 70 << 20
    d = payload(40, 0, total)
    frags = [d[:30000001], d[30000001:(64 << 20) + 12345], d[(64 << 20) + 12345:]]
    assert compose(wv, frags, 4321, 0, 2, 2, True) == oracle.compose_packets(d, 4321, 0, 2, 2, True)


def test_mixed_fragments_are_einval(engine, wv):
    d = payload(41, 0, 20000)
    a = Arena(engine, d, [10000, 10000])
    host = d[:5000].copy()
    with pytest.raises(engine.CRC32CError) as e:
        wv.compose_packets_iov([a.frags[0], a.frags[1], host])
    assert e.value.code == EINVAL and "fragment 2" in str(e.value) and "host" in str(e.value)
    with pytest.raises(engine.CRC32CError) as e:
        wv.compose_packets_iov([host, a.frags[0]])
    assert e.value.code == EINVAL and "fragment 1" in str(e.value)
    assert a.untouched()


# ---- nothing else is written --------------------------------------------------------------------
def test_undersized_outputs_write_nothing(engine, wv):
    from hadoofus_amd.abi import OutPacket
    d = payload(42, 0, 100000)
    a = Arena(engine, d, [33333, 66667], mis=(1, 3))
    lib = wv.load()
    vec, n, keep = wv.iovecs(a.frags)
    npk, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    assert lib.hdfs_writev_compose_packets(vec, n, 0, 0, 2, 2, 1, None, 0, None, 0, ctypes.byref(npk),
                                           ctypes.byref(used)) == 0
    need_n, need_b = npk.value, used.value
    hdr = np.full(need_b + 64, HGUARD, dtype=np.uint8)
    arr = (OutPacket * need_n)()
    before = bytes(arr)
    for cap, maxp in [(need_b - 1, need_n), (need_b, need_n - 1), (0, need_n)]:
        rc = lib.hdfs_writev_compose_packets(vec, n, 0, 0, 2, 2, 1, hdr.ctypes.data, cap, arr, maxp,
                                             ctypes.byref(npk), ctypes.byref(used))
        assert rc == EINVAL and (npk.value, used.value) == (need_n, need_b)
        assert (hdr == HGUARD).all() and bytes(arr) == before
    assert a.untouched()


# ---- round trip ----------------------------------------------------------------------------------
def test_round_trip_through_the_packet_verifier(engine, wv):
    """Header buffers interleaved with the data gathered from the fragments by
    data_off: the wire stream verifies clean; one flipped byte inside a
    gathered chunk is BAD_CHECKSUM at exactly that packet and chunk."""
    total = 300 * 1024 + 99
    split = 3 * 65536 + 10 * CS + 100  # inside packet 3, chunk 10: a gathered chunk
    d = payload(43, 0, total)
    a = Arena(engine, d, [split, total - split], mis=(3, 1))
    hdr, pkts = compose(wv, a.frags, 0, 0, 2, engine.CSUM_CRC32C, True)
    host_frags = [a.buf.download(n, p - a.buf.ptr) for p, n in a.frags]
    cat = np.concatenate(host_frags)
    wire = bytearray()
    for p in pkts:
        wire += hdr[p["hdr_off"]:p["hdr_off"] + p["hdr_len"]]
        wire += cat[p["data_off"]:p["data_off"] + p["data_len"]].tobytes()
    rc, got, used = engine.verify_packets(bytes(wire))
    assert rc == 0 and used == len(wire) and len(got) == len(pkts)
    assert all(p["error"] == 0 for p in got)
    p3 = got[3]
    assert p3["offset_in_block"] == 3 * 65536
    wire[p3["stream_off"] + p3["header_len"] + p3["crc_len"] + 10 * CS + 100] ^= 0x20  # the first byte of fragment 1
    rc, got, _ = engine.verify_packets(bytes(wire))
    assert rc == engine.ERR_BAD_CHECKSUM
    assert [(i, p["first_bad"], p["bad_chunks"]) for i, p in enumerate(got) if p["error"]] == [(3, 10, 1)]
    assert a.untouched()


# ---- threads -----------------------------------------------------------------------------------------
def test_two_threads_at_once(engine, wv, oracle):
    jobs = []
    for seed, lens, off in [(44, cuts(400000, [1, 70000, 70001, 333333]), 0), (45, cuts(250123, [999, 125000]), 4321)]:
        d = payload(seed, 0, sum(lens))
        jobs.append((Arena(engine, d, lens, mis=(1, 2, 3)), off, oracle.compose_packets(d, off, 0, 2, 2, True)))
    results, errors = [None, None], []
    start = threading.Barrier(2)

    def run(i):
        try:
            start.wait()
            for _ in range(4):
                results[i] = compose(wv, jobs[i][0].frags, jobs[i][1], 0, 2, 2, True)
                assert results[i] == jobs[i][2]
        except BaseException as e:  # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert results[0] == jobs[0][2] and results[1] == jobs[1][2]
    assert jobs[0][0].untouched() and jobs[1][0].untouched()


# ---- the C consumer ------------------------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    libdir = build.LIBDIR
    exe = tmp_path / "writev_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "writev_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_writev", "-lhadoofus_crc32c"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
