"""GPU: MD5CRC block and file checksums from chunk CRCs in device memory
(include/hadoofus_md5crc.h; the default BlockChecksumType of
src/proto/hdfs.proto:483-495, carried by src/proto/datatransfer.proto:316-322).

The block checksum is MD5 over the block's chunk CRCs as wire bytes (each CRC
big-endian, chunk order); the file checksum is MD5 over the block digests.
Expected values are Python's hashlib.md5 over bytes built from that
definition -- from the CRC arrays downloaded from the device, and, for the
CRC32C / wire-order case, also from the CPU oracle's chunk CRCs of the host
bytes, so the check does not rest on the engine's own CRCs alone.  No
Hadoop-generated vector is available offline, so none is used.  Everything is
bit-exact."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CS = 512
MD5_EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")


def _wire(stored_u8, flags):
    """Bytes of a CRC array as stored on the device -> the bytes MD5CRC
    digests: wire order (big-endian CRCs)."""
    if flags & 1:  # SEG_BE: stored in wire order already
        return stored_u8.tobytes()
    return stored_u8.view("<u4").astype(">u4").tobytes()


def _segments(engine, dbuf, specs, flags, stream=None, execute=True):
    """One compute plan over (offset, len) specs of dbuf at 512 B per CRC.
    -> (segments, their CRC buffers, the plan)."""
    segs, keep = [], []
    for off, n in specs:
        out = engine.DeviceBuffer(max(4, (n + CS - 1) // CS * 4))
        keep.append(out)
        segs.append(engine.Segment(data=dbuf.ptr + off, len=n, chunk_size=CS, flags=flags, crc_init=0,
                                   crcs=out.ptr, bitmap=None))
    plan = engine.Plan(engine.MODE_COMPUTE, segs)
    if execute:
        plan.execute(stream)
    return segs, keep, plan


def _want(keep, specs, flags):
    """hashlib.md5 of each segment's downloaded CRCs in wire order."""
    out = []
    for buf, (_, n) in zip(keep, specs):
        nch = (n + CS - 1) // CS
        out.append(hashlib.md5(_wire(buf.download(nch * 4), flags)).digest())
    return out


# ---- padding boundaries -------------------------------------------------------
PAD_NCHUNKS = [0, 1, 13, 14, 15, 16, 17, 29, 30, 31, 32, 33, 47, 48, 100]


@pytest.mark.parametrize("flags", [0, 1, 4, 5])  # host / wire order x CRC32C / CRC32
def test_padding_boundaries(engine, oracle, flags):
    rng = np.random.default_rng(100 + flags)
    specs, off = [], 0
    for k, nch in enumerate(PAD_NCHUNKS):
        n = nch * CS - (int(rng.integers(1, CS)) if nch and k % 2 else 0)  # every other last chunk is partial
        specs.append((off, n))
        off += (n + 4095) // 4096 * 4096
    host = rng.integers(0, 256, max(off, 4096), dtype=np.uint8)
    dbuf = engine.DeviceBuffer(host.nbytes)
    dbuf.upload(host)
    segs, keep, _ = _segments(engine, dbuf, specs, flags)
    got = engine.block_md5crcs(segs)  # one call; no sync after the plan
    assert [(s[1] + CS - 1) // CS for s in specs] == PAD_NCHUNKS
    assert got == _want(keep, specs, flags)
    assert got[0] == MD5_EMPTY
    if flags == engine.SEG_BE:  # CRC32C in wire order: the CPU oracle's CRCs of the host bytes
        for (o, n), g in zip(specs, got):
            crcs = oracle.chunk_crcs(host[o:o + n], CS)
            assert g == hashlib.md5(crcs.astype(">u4").tobytes()).digest(), n


# ---- wave boundaries and divergence -------------------------------------------
@pytest.fixture(scope="module")
def lane_pool(engine):
    """130 segments of 0..200 chunks (fixed seed), one compute plan, and the
    expected digest of each -- computed once, shared, not modified."""
    rng = np.random.default_rng(2024)
    nchs = [int(x) for x in rng.integers(0, 201, 130)]
    nchs[0], nchs[64] = 200, 0  # the extremes sit in different waves
    specs, off = [], 0
    for nch in nchs:
        specs.append((off, nch * CS))
        off += nch * CS
    host = rng.integers(0, 256, off, dtype=np.uint8)
    dbuf = engine.DeviceBuffer(host.nbytes)
    dbuf.upload(host)
    segs, keep, _ = _segments(engine, dbuf, specs, engine.SEG_BE)
    engine.device_sync()
    want = _want(keep, specs, engine.SEG_BE)
    return segs, keep, want


@pytest.mark.parametrize("nseg", [1, 63, 64, 65, 130])
def test_wave_boundaries_and_divergence(engine, lane_pool, nseg):
    segs, _, want = lane_pool
    got = engine.block_md5crcs(segs[:nseg])
    assert len(got) == nseg
    bad = [i for i in range(nseg) if got[i] != want[i]]
    assert not bad, bad
    # the same segments in reverse order: each digest follows its own segment
    assert engine.block_md5crcs(segs[:nseg][::-1]) == want[:nseg][::-1]


# ---- alignment and bounds -------------------------------------------------------
@pytest.mark.parametrize("past", [4, 8, 12])
def test_misaligned_crcs_and_guards(engine, past):
    """crcs at 4, 8 and 12 bytes past a 16-byte boundary, guard words of a
    known pattern before and after each array inside the same allocation."""
    rng = np.random.default_rng(past)
    nchs = [1, 3, 15, 16, 17, 32, 35, 64, 100]  # whole-vector trips, word-by-word tails, both
    guard = np.uint32(0xDEADBEEF)
    words = np.full(4096, guard, dtype=np.uint32)
    places, at = [], 64
    for nch in nchs:
        at = (at + 3) // 4 * 4 + past // 4  # word index: 16-byte boundary + past
        words[at:at + nch] = rng.integers(0, 2**32, nch, dtype=np.uint32)
        places.append((at, nch))
        at += nch + 8  # at least 8 guard words between arrays
    mask = np.ones(words.size, dtype=bool)
    for a, nch in places:
        mask[a:a + nch] = False
    image = words.copy()
    dbuf = engine.DeviceBuffer(words.nbytes)
    dbuf.upload(words)
    assert dbuf.ptr % 16 == 0
    for flags in (0, engine.SEG_BE):
        segs = [engine.Segment(data=None, len=nch * CS, chunk_size=CS, flags=flags, crc_init=0,
                               crcs=dbuf.ptr + 4 * a, bitmap=None) for a, nch in places]
        assert all(s.crcs % 16 == past for s in segs)
        got = engine.block_md5crcs(segs)
        want = [hashlib.md5(_wire(words[a:a + nch].view(np.uint8), flags)).digest() for a, nch in places]
        assert got == want, flags
    back = dbuf.download(dtype=np.uint32)
    assert np.array_equal(back, image)
    assert np.all(back[mask] == guard)


# ---- output placement -----------------------------------------------------------
def test_output_in_host_and_device_memory(engine, lane_pool):
    segs, _, want = lane_pool
    n = 70
    host_out = engine.block_md5crcs(segs[:n])
    dout = engine.DeviceBuffer(16 * n + 16)
    dout.fill(0xAB)
    assert engine.block_md5crcs(segs[:n], out_dptr=dout.ptr) is None
    back = dout.download()
    assert back[:16 * n].tobytes() == b"".join(host_out) == b"".join(want[:n])
    assert np.all(back[16 * n:] == 0xAB)  # nothing past 16 * nseg bytes
    # a device destination that is only 4-byte aligned
    engine.block_md5crcs(segs[:n], out_dptr=dout.ptr + 4)
    assert dout.download()[4:4 + 16 * n].tobytes() == b"".join(want[:n])


# ---- ordering ---------------------------------------------------------------------
def test_ordered_after_plan_on_the_same_stream(engine):
    """fill, plan.execute and block_md5crcs on one non-blocking stream with no
    synchronisation between them."""
    nbytes = 64 << 20
    dbuf = engine.DeviceBuffer(nbytes)
    s = engine.stream_create()
    try:
        specs = [(0, nbytes // 2), (nbytes // 2, nbytes // 2 - 1000)]
        segs, keep, plan = _segments(engine, dbuf, specs, engine.SEG_BE, execute=False)
        for buf in keep:
            buf.fill(0)
        engine.device_sync()
        engine.fill_splitmix64(dbuf.ptr, nbytes // 8, 5, 0, stream=s)
        plan.execute(stream=s)
        got = engine.block_md5crcs(segs, stream=s)
        assert got == _want(keep, specs, engine.SEG_BE)
        zeros = hashlib.md5(bytes(4 * (nbytes // 2 // CS))).digest()
        assert got[0] != zeros  # not the CRC buffer's earlier content
    finally:
        engine.load().hdfs_crc32c_stream_destroy(s)


# ---- block shape ------------------------------------------------------------------
def test_two_128mib_blocks_and_file_checksum(engine):
    blk = 128 << 20
    dbuf = engine.DeviceBuffer(2 * blk)
    engine.fill_splitmix64(dbuf.ptr, 2 * blk // 8, 0, 0)
    specs = [(0, blk), (blk, blk)]
    segs, keep, _ = _segments(engine, dbuf, specs, engine.SEG_BE)
    got = engine.block_md5crcs(segs)
    want = [hashlib.md5(buf.download(blk // CS * 4).tobytes()).digest() for buf in keep]
    assert got == want and got[0] != got[1]
    fc = engine.file_checksum(segs)
    assert fc.crc_per_block == 262144 and fc.bytes_per_crc == CS and fc.ctype == engine.CSUM_CRC32C
    assert fc.md5 == hashlib.md5(want[0] + want[1]).digest()
    assert fc.algorithm == "MD5-of-262144MD5-of-512CRC32C"
    assert fc.to_bytes() == (512).to_bytes(4, "big") + (262144).to_bytes(8, "big") + fc.md5
    one = engine.file_checksum(segs[:1])
    assert one.crc_per_block == 0 and one.md5 == hashlib.md5(want[0]).digest()
    assert one.algorithm == "MD5-of-0MD5-of-512CRC32C"


# ---- rejections ---------------------------------------------------------------------
def test_rejections(engine):
    dbuf = engine.DeviceBuffer(8192)
    out = engine.DeviceBuffer(64)

    def seg(**kw):
        a = dict(data=dbuf.ptr, len=4096, chunk_size=CS, flags=0, crc_init=0, crcs=out.ptr, bitmap=None)
        a.update(kw)
        return engine.Segment(**a)

    assert len(engine.block_md5crcs([seg()])) == 1
    for bad in (seg(flags=engine.SEG_RAW), seg(flags=engine.SEG_RAW | engine.SEG_BE), seg(crc_init=5),
                seg(chunk_size=0), seg(crcs=None), seg(crcs=out.ptr + 2)):
        with pytest.raises(engine.CRC32CError) as e:
            engine.block_md5crcs([seg(), bad])
        assert e.value.code == -1  # EINVAL
    hostmem = np.zeros(8, dtype=np.uint32)
    with pytest.raises(engine.CRC32CError):
        engine.block_md5crcs([seg(crcs=hostmem.ctypes.data)])
    # CRC32 and CRC32C may mix in block digests, not in one file
    mixed = [seg(), seg(flags=engine.SEG_CRC32)]
    assert len(engine.block_md5crcs(mixed)) == 2
    with pytest.raises(engine.CRC32CError):
        engine.file_checksum(mixed)
    with pytest.raises(engine.CRC32CError):
        engine.file_checksum([seg(), seg(chunk_size=1024)])
    assert engine.block_md5crcs([]) == []
    # a zero-length segment needs no CRC array
    assert engine.block_md5crcs([seg(len=0, crcs=None)]) == [MD5_EMPTY]


# ---- the C caller -------------------------------------------------------------------
def test_c_consumer_runs(engine, tmp_path):
    from hadoofus_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "md5crc_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "consumer", "md5crc_consumer.c"), "-o", str(exe),
                           "-L", build.LIBDIR, "-Wl,-rpath," + build.LIBDIR, "-lhadoofus_md5crc",
                           "-lhadoofus_crc32c"])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout
    blocks = [bytes.fromhex(l.split()[1]) for l in p.stdout.splitlines() if l.startswith("block ")]
    assert len(blocks) == 3
    name, md5 = [l for l in p.stdout.splitlines() if l.startswith("file ")][0][5:].split(":")
    assert name == "MD5-of-2048MD5-of-512CRC32C"
    assert bytes.fromhex(md5) == hashlib.md5(b"".join(blocks)).digest()
