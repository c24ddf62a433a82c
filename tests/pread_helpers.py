"""Scaffolding of tests/test_gpu_pread_batch.py: one device allocation that
holds every stream and every destination of a batch of positional reads
between guard bytes, the expected result of a read (the CPU oracle's
read_packets, which the main library's windowed read of the same device bytes
must give too), and the comparison of a call's results and of the whole
allocation with them."""
import numpy as np

from packet_stream import build_stream

GUARD = 0xA5
GAP = 96  # guard bytes before, between and after the ranges (at least)
SLACK = 24  # room of a destination beyond its read: never written
FIELDS = ("stream_off", "offset_in_block", "seqno", "data_len", "crc_len", "header_len", "error", "first_bad",
          "bad_chunks", "last", "sync")
SRES, DRES = (0, 1, 3, 7), (0, 5, 15)
AGAIN = 1000
MANY = 1024  # room for records no walk of these tests fills


def fields(recs):
    return [tuple(r[f] for f in FIELDS) for r in recs]


def stream_of(oracle, proto, ctype, dlens, seed, cs=512, **kw):
    return build_stream(oracle.crc32c, proto, cs, ctype, dlens, seed=seed, **kw)[0]


def read_of(s, off, n, cap=None):
    """A positional read: stream index, client_offset, read_len, dst_cap."""
    return dict(s=s, off=off, n=n, cap=n + SLACK if cap is None else cap)


def flip(s, at, mask=0x04):
    b = bytearray(s)
    b[at] ^= mask
    return bytes(b)


class Arena:
    """One device allocation: guards, then every stream and every read's
    destination, streams at residues 0, 1, 3, 7 mod 16 and destinations at 0,
    5, 15, with guards between."""

    def __init__(self, engine, streams, reads):
        caps = [r["cap"] for r in reads]
        self.buf = engine.DeviceBuffer(sum(n + GAP + 32 for n in [len(s) for s in streams] + caps) + GAP + 32)
        assert self.buf.ptr % 16 == 0
        at, self.src, self.dst, self.reads = GAP, [], [], [dict(r) for r in reads]
        for k, s in enumerate(streams):
            at = (at + 15) // 16 * 16 + SRES[k % len(SRES)]
            self.src.append(at)
            at += len(s) + GAP
        for k, n in enumerate(caps):
            at = (at + 15) // 16 * 16 + DRES[k % len(DRES)]
            self.dst.append(at)
            at += n + GAP
        assert at <= self.buf.nbytes
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        for s, o in zip(streams, self.src):
            self.image[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.buf.upload(self.image)
        self.lens = [len(s) for s in streams]

    def stream_ptr(self, r):
        return self.buf.ptr + self.src[r["s"]]

    def batch(self, pb):
        return [pb.entry(self.stream_ptr(r), self.lens[r["s"]], self.buf.ptr + self.dst[k], r["cap"], r["off"], r["n"])
                for k, r in enumerate(self.reads)]

    def check(self, delivered):
        """The whole allocation.  delivered[k]: the bytes read k delivered (None:
        its destination is untouched).  Behind them the destination is
        unspecified up to min(dst_cap, read_len) and untouched from there on;
        nothing else changed."""
        want, got = self.image.copy(), self.buf.download()
        for o, r, pl in zip(self.dst, self.reads, delivered or []):
            if pl is None:
                continue
            want[o:o + len(pl)] = np.frombuffer(pl, dtype=np.uint8)
            got[o + len(pl):o + max(len(pl), min(r["cap"], r["n"]))] = GUARD
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (streams {self.src[:8]}, destinations "
                                 f"{self.dst[:8]}): got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def reference(engine, oracle, scratch, arena, streams, r, proto, ctype, cs, max_pkts):
    """Read r's expected (rc, records, consumed, bytes): the oracle's, which the
    main library's windowed read of the same device bytes must give too."""
    s = streams[r["s"]]
    rc, recs, used, data = oracle.read_packets(s, r["off"], r["n"], proto, cs, ctype, max_pkts, r["cap"])
    erc, erecs, eused, egot = engine.read_packets(arena.stream_ptr(r), len(s), scratch.ptr, r["cap"], proto, cs, ctype,
                                                  max_pkts, r["off"], r["n"])
    assert (erc, fields(erecs), eused, egot) == (rc, fields(recs), used, len(data)), r
    assert scratch.download(egot).tobytes() == data, r
    return rc, recs, used, data


def compare(got, want, paths=None):
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["rc"], g["consumed"], g["delivered"]) == (w[0], w[2], len(w[3])), (k, g["rc"], g["consumed"],
                                                                                    g["delivered"], w[0], w[2])
        if g["records"] is not None:
            assert fields(g["records"]) == fields(w[1]), k
        if paths is not None and paths[k] is not None:
            assert g["path"] == paths[k], (k, g["path"])


def run(pb, engine, oracle, scratch, streams, reads, proto=2, ctype=2, cs=512, max_pkts=None, groups=None,
        stream=None, paths=None, records=True, want=None, arena=None):
    """Places the streams and destinations, serves the batch (groups: through
    the timing entry with that many workgroups, so without records) and checks
    every entry against its reference, and the whole arena.
    -> (results, references, arena)."""
    a = arena or Arena(engine, streams, reads)
    mp = MANY if max_pkts is None else max_pkts
    if want is None:
        want = [reference(engine, oracle, scratch, a, streams, r, proto, ctype, cs, mp) for r in reads]
    if groups is None:
        got = pb.read(a.batch(pb), proto, cs, ctype, (64 if max_pkts is None else mp) if records else None, stream)
    else:
        ms, got = pb.time(a.batch(pb), proto, cs, ctype, pb.time_groups(groups), 1)
        assert ms > 0
    compare(got, want, paths)
    a.check([w[3] for w in want])
    return got, want, a
