"""GPU: the scratch of the four companion libraries across its floor and back
(hadoofus_amd/csrc/companion_support.h: grow-only buffers on a scratch bound
to the engine's device).

Each library keeps the device buffers of a call between calls, at least 64 KiB
of each, and replaces a buffer when a call needs more.  The other GPU tests of
a library use one size per test, so none of them walks small -> just over the
floor -> small again on the real runtime: a call served by the floor block, a
call that frees it and allocates a larger one, and a call served by what the
larger one left.  Here every library does, and every stream, header buffer,
record and digest is the CPU oracle's, bit for bit."""
import hashlib

import numpy as np
import pytest

import test_gpu_wire as tw
import test_gpu_wire_batch as tb
import test_gpu_writev as tv
from packet_stream import payload

pytestmark = pytest.mark.gpu

CS = 512
SMALL = 513
BIG = (8 << 20) + 513  # at block offset 1: 511 + 16384 * 512 + 2 bytes, 16386 CRCs = 65544 bytes, 8 past the floor
OFF = 1


@pytest.fixture(scope="module")
def data():
    return payload(91, 0, BIG)


def test_sizes_cross_the_floor(oracle, data):
    _, pk = oracle.compose_packets(data, OFF, 0, 2, 2, False)
    assert pk[0]["data_len"] == 511 and pk[-1]["data_len"] % CS == 2  # a short head chunk, a partial last one
    assert sum(p["crc_len"] for p in pk) == 65544 > 65536 > 4 * 3


def test_wire(engine, oracle, data):
    from hadoofus_amd import wire
    wire.load()
    big = tw.expect(oracle, data, OFF, 5, 2, 2, True)
    small = tw.expect(oracle, data[:SMALL], OFF, 5, 2, 2, True)
    a = tw.Arena(engine, BIG, len(big[0]))
    tw.run(wire, a, data[:SMALL], small, 1, 3, OFF, 5, 2, 2, True)
    tw.run(wire, a, data, big, 3, 6, OFF, 5, 2, 2, True)
    tw.run(wire, a, data[:SMALL], small, 2, 9, OFF, 5, 2, 2, True)


def test_wire_batch(engine, oracle, data):
    from hadoofus_amd import wire_batch
    wire_batch.load()
    one = [dict(data=data[7:7 + SMALL], off=OFF, seq=3, finish=True, src_mis=1, dst_mis=5)]
    three = [dict(data=data[:SMALL], off=OFF, seq=10, finish=False, src_mis=3, dst_mis=1),
             dict(data=data, off=OFF, seq=20, finish=True, src_mis=5, dst_mis=11),
             dict(data=data[100:100 + SMALL], off=OFF, seq=30, finish=True, src_mis=2, dst_mis=14)]
    a = tb.Arena(engine, tb.room([SMALL, BIG, SMALL], [SMALL + 256, BIG + (1 << 17), SMALL + 256]))
    tb.batch(wire_batch, oracle, a, one)
    tb.batch(wire_batch, oracle, a, three)
    tb.batch(wire_batch, oracle, a, one)


def test_writev(engine, oracle, data):
    from hadoofus_amd import writev
    writev.load()
    for n, points in ((SMALL, (5, 260)), (BIG, (70001, (4 << 20) + 333)), (SMALL, (1, 512))):
        d = data[:n]
        a = tv.Arena(engine, d, tv.cuts(n, points), mis=(1, 7, 13))
        assert len(a.frags) == 3
        assert tv.compose(writev, a.frags, OFF, 9, 2, 2, True) == oracle.compose_packets(d, OFF, 9, 2, 2, True), n
        assert a.untouched()


def test_md5crc(engine, oracle, data):
    """1, 2049 and 1 segments of one chunk each: 32 bytes of table and digest
    per segment, so 2049 of them need 65568 bytes."""
    nseg = 2049
    assert nseg * 32 > 65536 >= (nseg - 1) * 32
    host = data[:nseg * CS]
    dbuf = engine.DeviceBuffer(host.nbytes)
    dbuf.upload(host)
    crcs = engine.DeviceBuffer(nseg * 4)
    segs = [engine.Segment(data=dbuf.ptr + k * CS, len=CS, chunk_size=CS, flags=engine.SEG_BE, crc_init=0,
                           crcs=crcs.ptr + 4 * k, bitmap=None) for k in range(nseg)]
    plan = engine.Plan(engine.MODE_COMPUTE, segs)
    plan.execute(None)  # no synchronise: the digests are ordered behind it on the same stream
    want = [hashlib.md5(int(c).to_bytes(4, "big")).digest() for c in oracle.chunk_crcs(host, CS)]
    assert engine.block_md5crcs(segs[:1]) == want[:1]
    assert engine.block_md5crcs(segs) == want
    assert engine.block_md5crcs(segs[5:6]) == want[5:6]
