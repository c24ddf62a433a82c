"""GPU: the scratch of the companion libraries across its floor and back
(hadoofus_amd/csrc/companion_support.h: grow-only buffers, and a device table
with its pinned staging twin, on a scratch bound to the engine's device).

Each library keeps the device buffers of a call between calls, at least 64 KiB
of each (16 KiB of a table and its pinned twin), and replaces a buffer when a
call needs more.  The other GPU tests of a library use one size per test, so
none of them walks small -> just over the floor -> small again on the real
runtime: a call served by the floor block, a call that frees it and allocates
a larger one, and a call served by what the larger one left.  Here every
library that owns such a buffer does, and every stream, header buffer, record
and digest is the CPU oracle's, bit for bit."""
import hashlib

import numpy as np
import pytest

import test_gpu_wire as tw
import test_gpu_wire_batch as tb
import test_gpu_wire_fused_batch as tfb
import test_gpu_wirev as tg
import test_gpu_wirev_fused as tgf
import test_gpu_writev as tv
from packet_stream import payload

pytestmark = pytest.mark.gpu

CS = 512
SMALL = 513
BIG = (8 << 20) + 513  # at block offset 1: 511 + 16384 * 512 + 2 bytes, 16386 CRCs = 65544 bytes, 8 past the floor
OFF = 1
TABLE_FLOOR = 16384  # kTableFloor
# a fragment table: an entry per non-empty fragment and the sentinel, 16 bytes each (sizeof(Frag), which
# wirev_internal.h and wirev_fused_internal.h assert)
FRAG_ENTRY, FEW, MANY = 16, [5, 255, SMALL - 260], [5] * 1024
# a batch table: 80 bytes per write that has packets (sizeof(Write), which wire_batch_layout.h asserts) and 4
# of its first packet's index, then 4 more for the total
WRITE_ENTRY, WRITES = 80 + 4, 196


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


def _gather(t, lib, engine, oracle, data):
    """3 fragments, 1024 of 5 bytes, 3 again: 4, 1025 and 4 table entries."""
    assert (len(FEW) + 1) * FRAG_ENTRY < TABLE_FLOOR < (len(MANY) + 1) * FRAG_ENTRY == 16400
    want = {n: t.expect(oracle, data[:n], OFF, 9, 2, 2, True) for n in (sum(FEW), sum(MANY))}
    a = t.Arena(engine, max(t.room(lens, len(want[sum(lens)][0])) for lens in (FEW, MANY)))
    for lens in (FEW, MANY, FEW):
        n = sum(lens)
        t.run(lib, a, t.cut(data[:n], lens), want[n], mis=(1, 7, 13), dst_mis=5, off=OFF, seq=9, finish=True)


def test_wirev(engine, oracle, data):
    from hadoofus_amd import wirev
    wirev.load()
    assert wirev.layout(MANY, OFF, finish=True)["nfrags"] == len(MANY)
    _gather(tg, wirev, engine, oracle, data)


def test_wirev_fused(engine, oracle, data):
    from hadoofus_amd import wirev_fused
    wirev_fused.load()
    assert wirev_fused.layout(MANY, OFF, finish=True)["nfrags"] == len(MANY)
    _gather(tgf, wirev_fused, engine, oracle, data)


def test_wire_fused_batch(engine, oracle, data):
    """2 writes, 196 one-packet writes of 513 bytes, 2 again.  195 writes
    would fill the floor to the byte and not cross it."""
    from hadoofus_amd import wire_fused_batch
    wire_fused_batch.load()
    assert 2 * WRITE_ENTRY + 4 < (WRITES - 1) * WRITE_ENTRY + 4 == TABLE_FLOOR < WRITES * WRITE_ENTRY + 4 == 16468
    two = [dict(data=data[7:7 + SMALL], off=OFF, seq=3, finish=True, src_mis=1, dst_mis=5),
           dict(data=data[100:100 + SMALL], off=0, seq=30, finish=False, src_mis=2, dst_mis=14)]
    many = [dict(data=data[3 * k:3 * k + SMALL], off=0, seq=7 * k, finish=False, src_mis=k % 16, dst_mis=(5 * k) % 16)
            for k in range(WRITES)]
    want_two, want_many = tfb.expect_all(oracle, two), tfb.expect_all(oracle, many)
    assert all(len(x[1]) == 1 for x in want_many)  # one packet each: every write is a table entry
    writes = [wire_fused_batch.write(None, SMALL, None, None, 0, 7 * k, False) for k in range(WRITES)]
    assert wire_fused_batch.layout(writes)[1]["table_entries"] == WRITES
    a = tfb.Arena(engine, tfb.room([SMALL] * WRITES, [len(x[0]) for x in want_many]))
    tfb.batch(wire_fused_batch, a, two, want_two)
    tfb.batch(wire_fused_batch, a, many, want_many)
    tfb.batch(wire_fused_batch, a, two, want_two)


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
