"""Non-canonical PacketHeaderProto encodings on every device framing path.

frame::decode_header (crc32c_frame.h) is compiled into the host walk, the
host walk over device memory (walk_device_stream: 64-byte header windows,
a D2H copy for a header longer than a window row), frame_build_kernel and
small_run_kernel (grid_frame: the LDS window when 6 + hlen <= kHdrWin, flat
loads otherwise) and spec_verify_kernel (its prologue refuses a run whose
packet 0 leaves the canonical byte layout; a later packet off the prediction
is framed with frame_step from the stream and either keeps the launch with a
record of its own or voids it).  Every other GPU test builds its streams with
packet_stream.header_v2, the canonical 25- or 27-byte encoding; here whole
streams carry the valid encodings of packet_stream.header_v2_variant /
header_v2_padded, at the sizes that select each path (cs = 512 throughout):

  small_run_kernel     <= kSmallRunMax (64) packets in <= kSmallRunBytes
  frame_build_kernel   more than 64 packets of one size
  speculative launch   stream > kSmallRunBytes (4 456 448 B), dataLen % 512 == 0
  window walk          packet sizes that leave the grid

Expected records come from the oracle (oracle_verify_packets /
oracle_read_packets: src/datanode.c:2345-2553) and are cross-checked against
the construction: the header fields each packet was given, its header length
and which chunks were corrupted.
"""
import ctypes

import numpy as np
import pytest

from packet_stream import CSUM_CRC32C, build_stream, header_v2, header_v2_padded, header_v2_variant

pytestmark = pytest.mark.gpu

CS, BAD, ERR_PROTO = 512, 29, 18
SMALL_RUN_BYTES = 64 * (65536 + 4096)  # kSmallRunBytes, crc32c_internal.h

# name -> (k, offset, seqno, last, dlen) -> PacketHeaderProto bytes; syncBlock decodes 0 in all but long_bool,
# whose bools (false lastPacketInBlock, true syncBlock) are 10-byte varints, a true one's bit in the last byte
VARIANTS = {
    "canonical": lambda k, o, s, l, d: header_v2(o, s, l, d),
    "reversed": lambda k, o, s, l, d: header_v2_variant(o, s, l, d, order=(4, 3, 2, 1, 5)),          # 25 B
    "unknown6": lambda k, o, s, l, d: header_v2_variant(o, s, l, d, unknown=((9, 6, 0, 1),)),       # 27 B
    "long_bool": lambda k, o, s, l, d: header_v2_variant(o, s, l, d, True, bool_bytes=10),
    "repeated": lambda k, o, s, l, d: header_v2_variant(o, s, l, d, repeat=1),
    "padded_tags": lambda k, o, s, l, d: header_v2_variant(o, s, l, d, tag_pad=2),
    "len64": lambda k, o, s, l, d: header_v2_padded(64, o, s, l, d),
    "len65": lambda k, o, s, l, d: header_v2_padded(65, o, s, l, d),
    "len4000": lambda k, o, s, l, d: header_v2_padded(4000, o, s, l, d),
}
V = list(VARIANTS)
SYNC = {v: int(v == "long_bool") for v in V}


def test_variant_lengths():
    """The encodings are what the shapes below rely on."""
    n = {v: 6 + len(VARIANTS[v](0, 65536, 1, False, 4096)) for v in V}
    assert n == {"canonical": 31, "reversed": 31, "unknown6": 33, "long_bool": 51, "repeated": 40,
                 "padded_tags": 39, "len64": 64, "len65": 65, "len4000": 4000}
    assert VARIANTS["reversed"](0, 65536, 1, False, 4096) != VARIANTS["canonical"](0, 65536, 1, False, 4096)
    assert len(VARIANTS["unknown6"](0, 0, 0, False, 4096)) == len(header_v2(0, 0, False, 4096, True))


class Run:
    """A built stream, the oracle's verdict on it and that verdict checked
    against the construction."""

    def __init__(self, oracle, header, dlens, corrupt, sync_of=None, stop_at=None):
        self.dl, self.hl = list(dlens), {}

        def hdr(k, o, s, l, d):
            h = header(k, o, s, l, d)
            self.hl[k] = 6 + len(h)
            return h

        self.s, self.bad = build_stream(oracle.crc32c, 2, CS, CSUM_CRC32C, self.dl, seed=len(self.dl), corrupt=corrupt,
                                        header=hdr)
        self.mp = len(self.dl) + 8
        self.want = oracle.verify_packets(self.s, max_pkts=self.mp)
        self.check(self.want, sync_of or (lambda k: 0), stop_at)

    def check(self, want, sync_of, stop_at):
        rc, pkts, used = want
        n = len(self.dl)
        assert len(pkts) == (n + 1 if stop_at is None else stop_at + 1)
        pos = off = 0
        for k, p in enumerate(pkts):
            dl = self.dl[k] if k < n else 0
            if k == stop_at:  # rejected header: the walk ends here, nothing of it consumed
                assert p == {"stream_off": pos, "offset_in_block": 0, "seqno": 0, "data_len": 0, "crc_len": 0,
                             "header_len": self.hl[k], "error": ERR_PROTO, "first_bad": -1, "bad_chunks": 0,
                             "last": 0, "sync": 0}
                assert used == pos
                break
            b = self.bad.get(k, [])
            assert p == {"stream_off": pos, "offset_in_block": off, "seqno": k, "data_len": dl,
                         "crc_len": 4 * ((dl + CS - 1) // CS), "header_len": self.hl[k], "error": BAD if b else 0,
                         "first_bad": b[0] if b else -1, "bad_chunks": len(b), "last": int(k == n),
                         "sync": sync_of(k)}, k
            pos += self.hl[k] + p["crc_len"] + dl
            off += dl
        else:
            assert used == len(self.s) == pos
        first = next((p["error"] for p in pkts if p["error"]), 0)
        assert rc == first

    def payload_before_error(self):
        out = bytearray()
        for p in self.want[1]:
            if p["error"]:
                break
            a = p["stream_off"] + p["header_len"] + p["crc_len"]
            out += self.s[a:a + p["data_len"]]
        return bytes(out)


_RUNS = {}


def _uniform(oracle, v, npk, dlen, corrupt):
    key = (v, npk, dlen, tuple(corrupt))
    if key not in _RUNS:
        _RUNS[key] = Run(oracle, VARIANTS[v], [dlen] * npk, corrupt, lambda k: SYNC[v])
    return _RUNS[key]


def _grid_run(oracle, v):
    """a. / e.: 200 packets x 4 096 B of one encoding + the empty last packet."""
    return _uniform(oracle, v, 200, 4096, [(120, 3), (170, 7)])


def _dev(engine, s, shift=0):
    buf = engine.DeviceBuffer(len(s) + shift + 64)
    buf.fill(0)
    buf.upload(np.frombuffer(s, np.uint8), offset=shift)
    engine.device_sync()
    return buf, buf.ptr + shift


def _framing_only(pkts):
    out = []
    for p in pkts:
        p = dict(p)
        if p["error"] == BAD:
            p.update(error=0, first_bad=-1, bad_chunks=0)
        out.append(p)
    return out


def _device_equals(engine, r, lib=None, parse=True):
    """verify_packets (and parse_packets) of the run in device memory at start
    shifts 0 and 1, and the host-stream verify, equal the oracle."""
    for shift in (0, 1):
        keep, p = _dev(engine, r.s, shift)
        assert engine.verify_packets(None, max_pkts=r.mp, dptr=p, nbytes=len(r.s), lib=lib) == r.want, shift
        if parse:
            rc, pkts, used = engine.parse_packets(None, max_pkts=r.mp, dptr=p, nbytes=len(r.s), lib=lib)
            want = _framing_only(r.want[1])
            assert pkts == want and used == r.want[2], shift
            assert rc == next((q["error"] for q in want if q["error"]), 0)
        keep.free()
    assert engine.verify_packets(r.s, max_pkts=r.mp, lib=lib) == r.want


def _reads_equal(engine, oracle, r):
    """read_packets of the run in device memory (start shifts 0 and 1): whole
    payloads and the client window [777, total - 1000), into a device buffer
    pre-filled with 0xA5 and into a host buffer -- records, consumed,
    delivered and the bytes equal the oracle's read (and the payload before
    the first error, from the construction); the 64-byte guard is intact."""
    total = sum(r.dl)
    whole = r.payload_before_error()
    co, rl = 777, total - 1000 - 777
    wwin = oracle.read_packets(r.s, co, rl, max_pkts=r.mp)
    assert wwin[3] == whole[co:co + rl] and wwin[1] == r.want[1][:len(wwin[1])]
    for shift in (0, 1):
        keep, p = _dev(engine, r.s, shift)
        for kw, want, data in ((dict(), r.want, whole), (dict(client_offset=co, read_len=rl), wwin[:3], wwin[3])):
            cap = total if not kw else rl
            dst = engine.DeviceBuffer(cap + 64)
            dst.fill(0xA5)
            engine.device_sync()
            rc, pkts, used, got = engine.read_packets(p, len(r.s), dst.ptr, cap, max_pkts=r.mp, **kw)
            assert (rc, pkts, used) == tuple(want), (shift, kw)
            assert got == len(data) and dst.download(got).tobytes() == data, (shift, kw)
            assert dst.download(64, offset=cap).tobytes() == b"\xa5" * 64
            dst.free()
            host = np.full(cap + 64, 0xA5, np.uint8)
            rc, pkts, used, got = engine.read_packets(p, len(r.s), None, 0, max_pkts=r.mp,
                                                      iov=[(host.ctypes.data, cap)], **kw)
            assert (rc, pkts, used) == tuple(want), (shift, kw, "host")
            assert got == len(data) and host[:got].tobytes() == data, (shift, kw, "host")
            assert host[cap:].tobytes() == b"\xa5" * 64
        keep.free()


# --- a. uniform runs on the device framing grid --------------------------------
@pytest.mark.parametrize("v", V)
def test_gpu_uniform_run_grid(engine, oracle, v):
    """201 packets > kSmallRunMax: frame_build_kernel frames every header --
    the general scan for every encoding but the canonical one, from the LDS
    window up to 6 + hlen = 64 and with flat loads for 65 and 4 000."""
    r = _grid_run(oracle, v)
    assert len(r.s) <= SMALL_RUN_BYTES
    assert r.want[0] == BAD and [k for k, p in enumerate(r.want[1]) if p["error"]] == [120, 170]
    _device_equals(engine, r)


# --- b. short runs: small_run_kernel and the hand-over to the grid -------------
@pytest.mark.parametrize("v", V)
def test_gpu_uniform_run_short(engine, oracle, v):
    """12 data packets (small_run_kernel), and 63 / 64 / 65 data packets + the
    empty one: 64 packets is the last run small_run_kernel takes."""
    for npk in (12, 63, 64, 65):
        r = _uniform(oracle, v, npk, 4096, [(3, 0), (npk - 1, 7)])
        assert len(r.s) <= SMALL_RUN_BYTES
        _device_equals(engine, r)


# --- c. speculation refused, kept with an exception record, or abandoned -------
@pytest.fixture(scope="module")
def diag(engine):
    from hadoofus_amd import abi, build
    lib = abi.bind_diag(abi.bind_product(ctypes.CDLL(build.DIAG_LIB)))
    assert lib.hdfs_crc32c_set_speculation(1) == 0
    return lib


def _spec_stats(lib):
    out = (ctypes.c_uint64 * 4)()
    assert lib.hdfs_crc32c_diag_spec_stats(out, 1) == 0
    return dict(zip(("launched", "eligible", "taken", "exc"), out))


def _spec_outcome(engine, diag, r):
    """The run verified from device memory by the diagnostic build: equal to
    the oracle; -> the speculative-launch counters of that one call."""
    keep, p = _dev(engine, r.s, 1)
    _spec_stats(diag)
    got = engine.verify_packets(None, max_pkts=r.mp, dptr=p, nbytes=len(r.s), lib=diag)
    st = _spec_stats(diag)
    keep.free()
    assert got == r.want
    return st


BLOCK = [65536] * 80
BLOCK_CORRUPT = [(10, 5), (60, 100)]  # before and after packet 40


@pytest.mark.parametrize("v", V)
def test_gpu_spec_refuses_noncanonical_packet0(engine, oracle, diag, v):
    """80 x 64 KiB (> kSmallRunBytes, whole chunks: the speculative launch is
    tried), every packet in one encoding: packet 0 off the canonical layout
    makes the run ineligible, and the regular path's records equal the
    oracle's.  The canonical control is taken."""
    r = _uniform(oracle, v, 80, 65536, BLOCK_CORRUPT)
    assert len(r.s) > SMALL_RUN_BYTES
    _device_equals(engine, r, parse=False)
    st = _spec_outcome(engine, diag, r)
    if v == "canonical":
        assert st["eligible"] >= 1 and st["taken"] >= 1 and st["exc"] == 0, st
    else:
        assert st["eligible"] == 0 and st["taken"] == 0, st


def _wrong_wire_type_25(o, s, l, d):
    """25 bytes like the canonical header, lastPacketInBlock sent as an empty
    length-delimited field: protobuf-c rejects the message."""
    h = header_v2(o, s, l, d)
    assert h[18] == 0x18
    return h[:18] + b"\x1a\x00" + h[20:]


ODD_AT_40 = {
    # (header of packet k, syncBlock packet k decodes to, packet whose header is rejected)
    "reversed_same_length": (lambda k, o, s, l, d: (VARIANTS["reversed"] if k == 40 else VARIANTS["canonical"])(
        k, o, s, l, d), lambda k: 0, None),
    "unknown6_in_sync_run": (lambda k, o, s, l, d: VARIANTS["unknown6"](k, o, s, l, d) if k == 40 else
                             header_v2(o, s, l, d, True), lambda k: int(k != 40), None),
    "wrong_wire_type": (lambda k, o, s, l, d: _wrong_wire_type_25(o, s, l, d) if k == 40 else
                        header_v2(o, s, l, d), lambda k: 0, 40),
}


@pytest.mark.parametrize("name", list(ODD_AT_40))
def test_gpu_spec_run_with_odd_packet_40(engine, oracle, diag, name):
    """A canonical run the speculative launch takes from packet 0, whose packet
    40 has the neighbours' length and other bytes: the same field values in
    reversed order; an unknown field 6 where the run carries syncBlock (sync
    decodes 0 there); a known field in the wrong wire type (error 18 at
    packet 40, the walk stops, consumed ends before it).  spec_verify_kernel
    frames a header off its prediction with frame_step -- the general scan,
    from the stream: a clean packet in the run's layout keeps the launch and
    gets the record of its own decode (the first two), anything else voids
    the launch and the run is framed the regular way (the third)."""
    header, sync_of, stop_at = ODD_AT_40[name]
    r = Run(oracle, header, BLOCK, BLOCK_CORRUPT, sync_of, stop_at)
    assert len({r.hl[k] for k in range(80)}) == 1
    if stop_at is not None:
        assert r.want[0] == BAD and r.want[1][10]["first_bad"] == 5 and r.want[1][40]["error"] == ERR_PROTO
        assert r.want[2] == r.want[1][40]["stream_off"] and len(r.want[1]) == 41
    _device_equals(engine, r, parse=False)
    st = _spec_outcome(engine, diag, r)
    if stop_at is None:
        assert st["eligible"] == 1 and st["taken"] == 1 and st["exc"] == 0, st
    else:
        assert st["eligible"] == 1 and st["exc"] == 1 and st["taken"] == 0, st
    # verify + copy-out of the same run with its one corruption behind packet 40: the speculative
    # launch copies packet 40's payload (or nothing from packet 40 on, after the rejected header)
    r2 = Run(oracle, header, BLOCK, BLOCK_CORRUPT[1:], sync_of, stop_at)
    assert len(r2.payload_before_error()) == (60 if stop_at is None else 40) * 65536
    _reads_equal(engine, oracle, r2)


# --- d. mixed encodings: the header-window walk --------------------------------
def test_gpu_mixed_encodings_window_walk(engine, oracle):
    """Packet k in variant k % 9: the wire sizes leave the grid after a packet
    or two, so the host walks the stream through header windows, copying the
    4 000-byte headers D2H.  A view cut inside a 4 000-byte header, and one
    cut at byte 64 of a 65-byte header, end before that packet."""
    r = Run(oracle, lambda k, o, s, l, d: VARIANTS[V[k % len(V)]](k, o, s, l, d), [4096] * 150,
            [(8, 1), (17, 0), (77, 7), (149, 3)], lambda k: SYNC[V[k % len(V)]])
    assert r.hl[8] == 4000 and r.hl[7] == 65
    _device_equals(engine, r)
    offs = [p["stream_off"] for p in r.want[1]]
    for k, inside in ((80, 2000), (80, 70), (79, 64), (79, 5)):
        assert r.hl[k] > inside
        cut = offs[k] + inside
        want = oracle.verify_packets(r.s[:cut], max_pkts=r.mp)
        assert len(want[1]) == k and want[2] == offs[k] and want[1] == r.want[1][:k]
        for shift in (0, 1):
            keep, p = _dev(engine, r.s, shift)
            assert engine.verify_packets(None, max_pkts=r.mp, dptr=p, nbytes=cut) == want, (k, inside, shift)
            keep.free()
        assert engine.verify_packets(r.s[:cut], max_pkts=r.mp) == want


# --- e. copy-out behind headers of other lengths -------------------------------
@pytest.mark.parametrize("v", ["len64", "len65", "len4000", "reversed"])
def test_gpu_copy_out_behind_noncanonical_headers(engine, oracle, v):
    """read_packets of a.'s stream (frame_build_kernel's records place the
    copies) and of a 12-packet run (small_run_kernel copies), the payloads
    starting at a header_len other than 31 or 33."""
    r = _grid_run(oracle, v)
    assert len(r.payload_before_error()) == 120 * 4096
    _reads_equal(engine, oracle, r)
    _reads_equal(engine, oracle, _uniform(oracle, v, 12, 4096, [(10, 2)]))


# --- f. jobs ---------------------------------------------------------------------
def test_gpu_jobs_with_noncanonical_blocks(engine, oracle):
    """Three blocks of 80 x 64 KiB in one verify_blocks_submit: canonical; the
    reversed encoding at packet 0; the reversed encoding at packet 40.  Each
    block's result is what verify_packets gives it alone and the oracle's
    records; the same as three verify_packets_submit jobs back to back."""
    def odd_at(j):
        return lambda k, o, s, l, d: (VARIANTS["reversed"] if k == j else VARIANTS["canonical"])(k, o, s, l, d)

    runs = [_uniform(oracle, "canonical", 80, 65536, BLOCK_CORRUPT),
            Run(oracle, odd_at(0), BLOCK, [(0, 1), (79, 127)]),
            Run(oracle, odd_at(40), BLOCK, [(39, 0), (41, 64)])]
    mp = runs[0].mp
    bufs = [_dev(engine, r.s, b) for b, r in enumerate(runs)]
    alone = [engine.verify_packets(None, max_pkts=mp, dptr=p, nbytes=len(r.s)) for (_, p), r in zip(bufs, runs)]
    assert alone == [r.want for r in runs]
    rc, got = engine.VerifyBlocksJob([(p, len(r.s)) for (_, p), r in zip(bufs, runs)], max_pkts=mp).wait()
    assert got == alone
    jobs = [engine.VerifyJob(p, len(r.s), max_pkts=mp) for (_, p), r in zip(bufs, runs)]
    assert [j.wait() for j in jobs] == alone
    for keep, _ in bufs:
        keep.free()
