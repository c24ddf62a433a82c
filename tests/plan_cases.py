"""Helpers of tests/test_gpu_plan_lifecycle.py and tests/test_plan_expect_cpu.py:
the tables ("shapes") a batch plan is run on again and again, their layout in
three guarded device allocations, the chunks each pass corrupts, and what a
verify plan must report for them -- all derived here, never from the engine.

A case holds, per segment, the chunk geometry, the bytes (host bytes for the
small shapes, a splitmix64 formula for the two pool-sized ones), the expected
chunk CRCs and, per pass, a set of bad chunks {(segment, chunk): kind} with
kind "data" (one bit of the chunk's data flipped) or "crc" (one bit of its
expected CRC word flipped).  From the set alone come each segment's first bad
chunk, the mismatch count and the bitmap bytes.

classify() and launch_class() restate the engine's split of a table between
its tiled and generic kernels and the size rule of launch_all
(hadoofus_amd/csrc/crc32c_engine.cpp), so a test can say which launch class a
shape reaches on the device it runs on and compare that with Plan.stats()."""
import bisect

import numpy as np

GUARD = 0xA5
NONE = 0xFFFFFFFF      # first_bad of a segment without a bad chunk
TILE_CHUNKS = 8        # chunks per tile, one bitmap byte
ROUND_BYTES = 512      # bytes of each chunk per round
WAVES = 16             # waves per workgroup of the tiled kernels
POOL_MIN = 32          # rounds per wave from which the global pool is used
PHASE1 = (23, 25)      # the static phase's share of the tiles when the pool is on (crc32c_deal.h)
DATA_GAP = 64          # guard bytes around every segment's data (at least)
CRC_GAP_WORDS = 4      # guard words between CRC arrays
SHAPES = (1, 2, 3, 4, 5)
SMALL_SHAPES = (1, 2, 3)


def splitmix_words(seed, g):
    """splitmix64(seed, g) for an array of word indices (oracle.splitmix64_np's formula)."""
    g = np.asarray(g, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (g + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


class Seg:
    """One segment: chunk geometry, the engine's tile split, its place in the allocations."""

    def __init__(self, cs, length, residue=0):
        self.cs, self.len, self.residue = cs, length, residue
        self.nchunks = (length + cs - 1) // cs
        self.full = length // cs                      # whole chunks
        self.ragged = length - self.full * cs         # bytes of the partial last chunk (0: none)
        self.ntiles = (self.nchunks + TILE_CHUNKS - 1) // TILE_CHUNKS
        self.main_tiles = self.gen_tiles = 0
        self.data_at = self.crc_at = self.bm_at = None  # byte offsets in the three allocations
        self.g0 = 0                                   # device-filled cases: first splitmix64 word index

    @property
    def bm_bytes(self):
        return (self.nchunks + 7) // 8

    def chunk_len(self, c):
        return min(self.cs, self.len - c * self.cs)

    def last_main_tile(self):
        """Chunks of the segment's last tile on the tiled kernel."""
        if not self.main_tiles:
            return range(0)
        return range((self.main_tiles - 1) * TILE_CHUNKS, min(self.main_tiles * TILE_CHUNKS, self.nchunks))


def classify(segs):
    """The engine's classify(): which tiles of each segment the tiled kernel takes
    (chunk size a multiple of 512, whole chunks; any data alignment) and which
    the generic kernel.  -> (rounds, mtiles, gtiles, main_bytes, generic_bytes)."""
    rounds = mtiles = gtiles = main_bytes = gen_bytes = 0
    for s in segs:
        eligible = s.nchunks > 0 and s.cs % ROUND_BYTES == 0
        partial = s.len % s.cs != 0
        if eligible:
            s.main_tiles, s.gen_tiles = (s.ntiles - 1, 1) if partial else (s.ntiles, 0)
        else:
            s.main_tiles, s.gen_tiles = 0, s.ntiles
        s.mtile_start = mtiles
        mtiles += s.main_tiles
        rounds += s.main_tiles * (s.cs // ROUND_BYTES)
        gtiles += s.gen_tiles
        mb = min(s.len, s.main_tiles * TILE_CHUNKS * s.cs)
        main_bytes += mb
        gen_bytes += s.len - mb
    return rounds, mtiles, gtiles, main_bytes, gen_bytes


def uniform_tiles(segs):
    """The engine's uniform_tiles(): main tiles per segment when every segment
    but the last holds the same number and the last no more; else 0."""
    if not segs or not segs[0].main_tiles:
        return 0
    t = segs[0].main_tiles
    for i, s in enumerate(segs[1:], 1):
        if (s.main_tiles != t) if i + 1 < len(segs) else (s.main_tiles > t):
            return 0
    return t


def launch_class(segs, num_cu, compute=False):
    """launch_all's size rule for a table on a device of num_cu CUs (no mailbox
    open): the schedule of the tiled launch (None: no tiled launch), whether
    its global pool is on, the realigning kernel, compute mode's group gather."""
    rounds, mtiles, gtiles, main_bytes, gen_bytes = classify(segs)
    out = dict(rounds=rounds, mtiles=mtiles, gtiles=gtiles, main_bytes=main_bytes, generic_bytes=gen_bytes,
               nchunks=sum(s.nchunks for s in segs), order=None, pool=False, grid=0, una=False, gather=False,
               utiles=0)
    if not rounds:
        return out
    grid = min(max((rounds + 63) // 64, 1), num_cu)
    ut = uniform_tiles(segs)
    small = rounds < POOL_MIN * WAVES * grid or (not ut and mtiles < 2 * grid * len(segs))
    una = any(s.main_tiles and s.residue % 4 for s in segs)
    order = 2 if small else 3
    out.update(order=order, pool=rounds >= POOL_MIN * WAVES * grid, grid=grid, una=una, utiles=ut,
               gather=bool(compute and order == 3 and not una))
    return out


def pool_first_tile(mtiles):
    """First main tile of the pool's share when the pool is on (phase1)."""
    return mtiles * PHASE1[0] // PHASE1[1]


class Case:
    """A table, its layout, its bytes and its expected CRCs."""

    def __init__(self, name, segs, seed, device_fill=False, g0=0):
        self.name, self.segs, self.seed, self.device_fill = name, segs, seed, device_fill
        classify(segs)
        at = DATA_GAP
        for s in segs:
            if s.len:
                at = (at + DATA_GAP + 15) // 16 * 16 + s.residue
                s.data_at = at
                at += s.len
        self.data_size = at + DATA_GAP + 16
        at = 4 * CRC_GAP_WORDS
        for s in segs:
            if s.nchunks:
                s.crc_at = at
                at += 4 * (s.nchunks + CRC_GAP_WORDS)
        self.crc_size = at + 4 * CRC_GAP_WORDS
        at = 5
        for i, s in enumerate(segs):
            if s.nchunks:
                s.bm_at = at
                at += s.bm_bytes + 1 + i % 3     # one to three guard bytes between neighbours
        self.bm_size = at + 16
        for i, s in enumerate(segs):
            s.g0 = g0 + (i << 24)
        self.host = None      # per segment: the clean bytes (small shapes)
        self.crcs = None      # per segment: the expected chunk CRCs, uint32
        self.mtile_start = [s.mtile_start for s in segs]

    # ---- bytes ------------------------------------------------------------------------------------------
    def make_host(self, oracle):
        """Host bytes and oracle CRCs of every segment (small shapes)."""
        assert not self.device_fill
        self.host = [oracle.splitmix((s.len + 7) // 8, seed=self.seed, g0=s.g0).view(np.uint8)[:s.len].copy()
                     for s in self.segs]
        self.crcs = [oracle.chunk_crcs(h, s.cs) if s.len else np.zeros(0, np.uint32)
                     for h, s in zip(self.host, self.segs)]

    def make_crcs(self, oracle):
        """Device-filled cases: the oracle's CRCs of every segment, its bytes
        regenerated by formula one segment at a time (no host copy of the table)."""
        assert self.device_fill
        self.crcs = [oracle.chunk_crcs(oracle.splitmix(s.len // 8, seed=self.seed, g0=s.g0).view(np.uint8), s.cs)
                     for s in self.segs]

    def chunk_bytes(self, picks):
        """Device-filled cases: the bytes of chunks [(segment, chunk)], regenerated
        by formula (512-B chunks, 64 words each), one after another."""
        g = np.array([self.segs[s].g0 + c * 64 for s, c in picks], dtype=np.uint64)
        return splitmix_words(self.seed, g[:, None] + np.arange(64, dtype=np.uint64)[None, :]).reshape(-1).view(np.uint8)

    def samples(self, extra=240):
        """(segment, chunk) picks: the first and last chunk of every segment and
        `extra` more spread over the table."""
        picks = set()
        for i, s in enumerate(self.segs):
            picks |= {(i, 0), (i, s.nchunks - 1)}
        rng = np.random.default_rng(len(self.segs))
        for i in rng.integers(0, len(self.segs), extra):
            picks.add((int(i), int(rng.integers(0, self.segs[int(i)].nchunks))))
        return sorted(picks)

    # ---- flips ------------------------------------------------------------------------------------------
    def data_flip(self, s, c):
        """-> (byte offset in the segment, mask) of the bit a "data" corruption of chunk c flips."""
        seg = self.segs[s]
        return c * seg.cs + (c * 131 + s * 17 + 5) % seg.chunk_len(c), 1 << ((c + s) % 8)

    @staticmethod
    def crc_flip(s, c):
        return np.uint32(1 << ((c * 7 + s) % 32))

    def data_image(self, bad=None):
        """The data allocation (small shapes): guards, every segment's bytes, the "data" flips of bad."""
        img = np.full(self.data_size, GUARD, dtype=np.uint8)
        for s, h in zip(self.segs, self.host):
            if s.len:
                img[s.data_at:s.data_at + s.len] = h
        for (s, c), kind in (bad or {}).items():
            if kind == "data":
                off, mask = self.data_flip(s, c)
                img[self.segs[s].data_at + off] ^= mask
        return img

    def crc_image(self, bad=None):
        """The CRC allocation as uploaded for a verify pass (and as a compute
        pass must leave it, bad empty): guard words, big-endian CRC arrays,
        the "crc" flips of bad."""
        img = np.full(self.crc_size, GUARD, dtype=np.uint8)
        arrs = [c.copy() for c in self.crcs]
        for (s, c), kind in (bad or {}).items():
            if kind == "crc":
                arrs[s][c] ^= self.crc_flip(s, c)
        for s, a in zip(self.segs, arrs):
            if s.nchunks:
                img[s.crc_at:s.crc_at + 4 * s.nchunks] = a.astype(">u4").view(np.uint8)
        return img

    # ---- what a verify pass must report -------------------------------------------------------------------
    def first_bad(self, bad):
        fb = [NONE] * len(self.segs)
        for s, c in bad:
            fb[s] = min(fb[s], c)
        return fb

    @staticmethod
    def count(bad):
        return len(bad)

    def bitmap_image(self, bad):
        """The bitmap allocation after a verify pass: guards, ceil(nchunks / 8)
        bytes per segment with bit c % 8 of byte c // 8 set for a bad chunk c, good bytes 0."""
        img = np.full(self.bm_size, GUARD, dtype=np.uint8)
        for s in self.segs:
            if s.nchunks:
                img[s.bm_at:s.bm_at + s.bm_bytes] = 0
        for s, c in bad:
            img[self.segs[s].bm_at + c // 8] |= 1 << (c % 8)
        return img

    def bitmap_prefill(self, value):
        img = np.full(self.bm_size, GUARD, dtype=np.uint8)
        for s in self.segs:
            if s.nchunks:
                img[s.bm_at:s.bm_at + s.bm_bytes] = value
        return img

    def tile_chunk(self, tile, k):
        """Chunk k of global main tile `tile` -> (segment, chunk)."""
        s = bisect.bisect_right(self.mtile_start, tile) - 1
        assert tile < self.segs[s].mtile_start + self.segs[s].main_tiles
        return s, (tile - self.segs[s].mtile_start) * TILE_CHUNKS + k


def _kinds(chunks):
    """{(segment, chunk): kind}, the two kinds alternating in table order."""
    return {sc: ("data", "crc")[i % 2] for i, sc in enumerate(sorted(chunks))}


def small_sets(case, spare, healed):
    """Sets A and B of a small shape.  A: chunk 0, the last whole chunk, the
    ragged chunk and a chunk of the last main tile of every segment except
    `spare`, which stays clean so that B can make a clean segment bad (its last
    main tile is hit under B instead).  B: other chunks of every segment
    except `healed`, all after chunk 0."""
    a, b = set(), set()
    for i, s in enumerate(case.segs):
        n = s.nchunks
        if not n:
            continue
        lm = s.last_main_tile()
        mine = set()
        if i != spare:
            mine = {0, max(s.full - 1, 0)}
            if s.ragged:
                mine.add(n - 1)
            if lm:
                mine.add(lm[len(lm) // 2])
            a |= {(i, c) for c in mine}
        if i != healed:
            cand = [n // 3, n - 2, 1] + ([lm[-1], lm[0]] if lm else [])
            picks = [c for c in dict.fromkeys(cand) if 0 < c < n and c not in mine][:4]
            assert picks, (case.name, i)
            b |= {(i, c) for c in picks}
    return _kinds(a), _kinds(b)


def big_sets(case):
    """Sets A and B of a pool-sized shape, by position in the global tile
    order: chunks of the first and the last tile, of eight tiles in the pool's
    share (the last 8 %) and of six tiles in the static 92 % before it.  A also
    holds a chunk of every segment's last main tile, except in the segments
    only B makes bad, whose last main tile B hits instead."""
    t = case.segs[-1].mtile_start + case.segs[-1].main_tiles
    a = {case.tile_chunk(0, 0), case.tile_chunk(0, 5), case.tile_chunk(t - 1, 2), case.tile_chunk(t - 1, 7)}
    b = {case.tile_chunk(0, 3), case.tile_chunk(t - 1, 6)}
    for i in range(8):
        a.add(case.tile_chunk(t * (925 + 9 * i) // 1000, 1))
        b.add(case.tile_chunk(t * (929 + 9 * i) // 1000, 6))
    for fa, fb in zip((100, 250, 400, 550, 700, 850), (150, 300, 450, 600, 750, 880)):
        a.add(case.tile_chunk(t * fa // 1000, 1))
        b.add(case.tile_chunk(t * fb // 1000, 6))
    a, b = _kinds(a), _kinds(b)
    spare = {s for s, _ in b} - {s for s, _ in a}
    for i, s in enumerate(case.segs):
        if i in spare:
            b.setdefault((i, s.last_main_tile()[2]), "crc")
        else:
            a.setdefault((i, s.last_main_tile()[4]), "crc")
    return a, b


def check_sets(case, a, b, pool=False):
    """What the verify sequence needs of A and B (asserted for every shape by the CPU test)."""
    assert a and b and not set(a) & set(b)
    for bad in (a, b):
        assert {"data", "crc"} <= set(bad.values())
        for (s, c), kind in bad.items():
            assert 0 <= c < case.segs[s].nchunks
    fa, fb = case.first_bad(a), case.first_bad(b)
    assert sum(1 for x, y in zip(fa, fb) if x != NONE and y != NONE and y > x) >= 2, "B's first bad chunk later"
    assert any(x != NONE and y == NONE for x, y in zip(fa, fb)), "a segment bad under A, clean under B"
    assert any(x == NONE and y != NONE for x, y in zip(fa, fb)), "a segment newly bad under B"
    segs = case.segs
    # chunk 0, a last whole chunk, a ragged chunk, wherever the shape has them
    assert any(c == 0 for _, c in a)
    assert any(c == segs[s].full - 1 for s, c in a)
    if any(s.ragged for s in segs):
        assert any(segs[s].ragged and c == segs[s].nchunks - 1 for s, c in a)
    # every segment's last main tile under A or, for the segment A spares, under B
    ta, tb = ({(t, c // TILE_CHUNKS) for t, c in x} for x in (a, b))
    for i, s in enumerate(segs):
        if s.main_tiles:
            last = (i, s.main_tiles - 1)
            assert last in ta or (fa[i] == NONE and last in tb), i
    if pool:
        t = segs[-1].mtile_start + segs[-1].main_tiles
        p2 = pool_first_tile(t)
        for bad in (a, b):
            tiles = [segs[s].mtile_start + c // TILE_CHUNKS for s, c in bad]
            assert 0 in tiles and t - 1 in tiles
            assert sum(1 for x in tiles if x >= p2 + TILE_CHUNKS) >= 8
            assert sum(1 for x in tiles if TILE_CHUNKS <= x < p2 - TILE_CHUNKS) >= 4


def pool_rounds(num_cu):
    """Rounds from which shapes 4 and 5 are sized: 5/4 of the pool's threshold on a full grid."""
    return POOL_MIN * WAVES * num_cu * 5 // 4


def build(shape, num_cu, seed=1, g0=0):
    """-> Case of shape 1..5 (see tests/test_gpu_plan_lifecycle.py) with its bad sets a and b."""
    if shape == 1:     # generic kernel only
        segs = [Seg(100, 9999), Seg(512, 300), Seg(777, 777 * 9), Seg(4, 256), Seg(4096, 0)]
        case, sets = Case("generic", segs, seed, g0=g0), lambda c: small_sets(c, spare=3, healed=1)
    elif shape == 2:   # small tiled launch, whole tiles, aligned
        segs = [Seg(cs, cs * 8 * t) for cs, t in zip((512, 1024, 1536, 4096, 512, 2048), (1, 5, 13, 8, 16, 3))]
        case, sets = Case("small-tiled", segs, seed, g0=g0), lambda c: small_sets(c, spare=4, healed=0)
    elif shape == 3:   # small tiled launch, byte residues 0..3, tails on the generic kernel
        segs = [Seg(512, 512 * (8 * 13 + 3) + 100, 0), Seg(512, 512 * (8 * 8 + 5), 1),
                Seg(512, 512 * (8 * 2 + 7) + 511, 2), Seg(512, 512 * 8, 3)]
        case, sets = Case("small-unaligned", segs, seed, g0=g0), lambda c: small_sets(c, spare=1, healed=3)
    elif shape == 4:   # pool, uniform table: equal 16 MiB segments
        per = (16 << 20) // (ROUND_BYTES * TILE_CHUNKS)
        n = (pool_rounds(num_cu) + per - 1) // per
        case = Case("pool-uniform", [Seg(512, 16 << 20) for _ in range(n)], seed, device_fill=True, g0=g0)
        sets = big_sets
    elif shape == 5:   # pool, table of small segments: 13 and 11 tiles in turn
        segs, tiles = [], 0
        while tiles < pool_rounds(num_cu):
            t = 13 if len(segs) % 2 == 0 else 11
            segs.append(Seg(512, 512 * 8 * t))
            tiles += t
        case, sets = Case("pool-small-segments", segs, seed, device_fill=True, g0=g0), big_sets
    else:
        raise ValueError(shape)
    case.shape = shape
    case.a, case.b = sets(case)
    return case


def check_class(case, num_cu, compute=False):
    """The launch class the shape is built to reach, from the size rule alone."""
    k = launch_class(case.segs, num_cu, compute)
    if case.shape == 1:
        assert k["rounds"] == 0 and k["order"] is None and k["main_bytes"] == 0 and k["gtiles"] > 0
    elif case.shape == 2:
        assert [s.main_tiles for s in case.segs] == [1, 5, 13, 8, 16, 3]
        assert k["order"] == 2 and not k["pool"] and not k["una"] and k["generic_bytes"] == 0 and k["gtiles"] == 0
    elif case.shape == 3:
        assert [s.main_tiles for s in case.segs] == [13, 9, 2, 1] and [s.gen_tiles for s in case.segs] == [1, 0, 1, 0]
        assert k["order"] == 2 and not k["pool"] and k["una"] and k["generic_bytes"] > 0
        for s in case.segs:    # the last main tile and the generic tile: two bitmap bytes of one segment
            if s.gen_tiles:
                assert s.last_main_tile()[-1] // 8 + 1 == (s.nchunks - 1) // 8 == s.main_tiles
    elif case.shape == 4:
        assert k["rounds"] >= pool_rounds(num_cu) and k["grid"] == num_cu
        assert k["order"] == 3 and k["pool"] and k["utiles"] == 4096 and not k["una"] and k["generic_bytes"] == 0
        assert all(s.main_tiles % TILE_CHUNKS == 0 for s in case.segs)
        assert k["gather"] == bool(compute)
    elif case.shape == 5:
        assert k["rounds"] >= pool_rounds(num_cu) and k["grid"] == num_cu
        assert k["utiles"] == 0 and k["mtiles"] < 2 * k["grid"] * len(case.segs)
        assert k["order"] == 2 and k["pool"] and not k["una"] and k["generic_bytes"] == 0
    return k


class OnDevice:
    """A case in three device allocations: data, CRC arrays, bitmaps, each
    carved between 0xA5 guards; the CRC and bitmap allocations are downloaded
    and compared as a whole.  Every image goes through one block of pinned host
    memory the case owns, so the many transfers of a sequence leave the runtime
    no pageable buffer to pin."""

    def __init__(self, engine, case):
        self.e, self.case = engine, case
        self.data = engine.DeviceBuffer(case.data_size)
        self.crc = engine.DeviceBuffer(case.crc_size)
        self.bm = engine.DeviceBuffer(case.bm_size)
        self.applied = {}
        self.stage = engine.PinnedBuffer(max(case.crc_size, case.bm_size, 0 if case.device_fill else case.data_size))
        self.load(case)
        self.crc.fill(GUARD)
        self.bm.fill(GUARD)
        engine.device_sync()

    def free(self):
        for b in (self.data, self.crc, self.bm, self.stage):
            b.free()

    def _up(self, buf, img, offset=0):
        self.stage.array[:img.size] = img
        buf.upload(self.stage.array[:img.size], offset=offset)

    def _down(self, buf, nbytes=None, offset=0):
        nbytes = buf.nbytes if nbytes is None else nbytes
        buf.copy_to(self.stage.ptr, nbytes, offset)
        return self.stage.array[:nbytes].copy()

    def crc_bytes(self):
        """The whole CRC allocation (the caller has waited for what writes it)."""
        return self._down(self.crc)

    def bitmap_bytes(self):
        return self._down(self.bm)

    def load(self, case):
        """Put case's clean data in place (the same layout: another seed)."""
        assert case.data_size == self.case.data_size
        self.case, self.applied = case, {}
        if case.device_fill:
            self.data.fill(GUARD)
            for s in case.segs:
                self.e.fill_splitmix64(self.data.ptr + s.data_at, s.len // 8, case.seed, s.g0)
        else:
            self._up(self.data, case.data_image())
        self.e.device_sync()

    def segments(self, verify):
        e = self.e
        return [e.Segment(data=self.data.ptr + s.data_at if s.len else None, len=s.len, chunk_size=s.cs,
                          flags=e.SEG_BE, crc_init=0, crcs=self.crc.ptr + s.crc_at if s.nchunks else None,
                          bitmap=self.bm.ptr + s.bm_at if verify and s.nchunks else None)
                for s in self.case.segs]

    def plan(self, verify):
        return self.e.Plan(self.e.MODE_VERIFY if verify else self.e.MODE_COMPUTE, self.segments(verify))

    def _poke(self, s, c):
        off, mask = self.case.data_flip(s, c)
        at = self.case.segs[s].data_at + off
        b = self._down(self.data, 1, at)
        b[0] ^= mask
        self._up(self.data, b, at)

    def set_bad(self, bad):
        """Restore what is corrupted now, then corrupt `bad`."""
        for (s, c), kind in list(self.applied.items()) + list(bad.items()):
            if kind == "data":
                self._poke(s, c)
        self.applied = dict(bad)
        self._up(self.crc, self.case.crc_image(bad))
        self.e.device_sync()

    def prefill_bitmaps(self, value):
        self._up(self.bm, self.case.bitmap_prefill(value))
        self.e.device_sync()

    def prefill_crcs(self):
        self.crc.fill(GUARD)
        self.e.device_sync()

    @staticmethod
    def _same(got, want, what):
        if not np.array_equal(got, want):
            d = np.flatnonzero(got != want)
            return [f"{what}: {d.size} bytes differ, first at {d[0]}: got {got[d[0]]:#x}, want {want[d[0]]:#x}"]
        return []

    def verify_errors(self, plan, bad, stream=None):
        """What differs from the helper's expectation after a verify pass:
        results (read on `stream`, which waits for it) and the whole bitmap allocation."""
        fb, m = plan.results(stream)
        errs = []
        want = self.case.first_bad(bad)
        if fb != want:
            d = [(i, x, y) for i, (x, y) in enumerate(zip(fb, want)) if x != y]
            errs.append(f"first_bad: {len(d)} segments differ, (segment, got, want) {d[:4]}")
        if m != len(bad):
            errs.append(f"mismatches {m}, want {len(bad)}")
        return errs + self._same(self.bitmap_bytes(), self.case.bitmap_image(bad), "bitmaps")

    def compute_errors(self):
        """What differs after a compute pass (the caller has waited for it): the whole CRC allocation."""
        return self._same(self.crc_bytes(), self.case.crc_image(), "CRC arrays")
