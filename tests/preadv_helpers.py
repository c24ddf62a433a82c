"""Scaffolding of tests/test_gpu_preadv_batch.py: one device allocation that
holds every stream and every destination fragment of a batch of scatter reads
between guard bytes, the expected result of a read (the CPU oracle's
read_packets, which the main library's read of the same device bytes into a
fragment list of the same lengths must give too), and the comparison of a
call's results and of the whole allocation with them.

A read is a dict: s (stream index), off (client_offset), n (read_len), frags
(the fragment lengths in order; 0 is an empty fragment with a base, None an
empty one without)."""
import random

import numpy as np

from pread_helpers import AGAIN, FIELDS, MANY, fields, flip, stream_of  # noqa: F401  (re-exported)

GUARD = 0xA5
GAP = 40  # guard bytes before, between and after the ranges (at least)
SRES, FRES = (0, 1, 3, 7), (0, 1, 5, 15)


def read_of(s, off, n, frags=None):
    return dict(s=s, off=off, n=n, frags=[n] if frags is None else list(frags))


def cap_of(r):
    return sum(f or 0 for f in r["frags"])


def split(n, cuts):
    """Fragment lengths of n bytes cut at the destination positions `cuts`
    (those outside (0, n) are dropped)."""
    at = sorted({c for c in cuts if 0 < c < n})
    return [b - a for a, b in zip([0] + at, at + [n])]


def cycle(n, lens=(3, 5, 7, 11, 13)):
    out, k = [], 0
    while n:
        out.append(min(n, lens[k % len(lens)]))
        n -= out[-1]
        k += 1
    return out


class Arena:
    """One device allocation: guards, then every stream (residues 0, 1, 3, 7
    mod 16), then every fragment of every read in shuffled address order
    (residues 0, 1, 5, 15), guards between all of them."""

    def __init__(self, engine, streams, reads, seed=1):
        self.reads = [dict(r) for r in reads]
        order = [(k, i) for k, r in enumerate(reads) for i, f in enumerate(r["frags"]) if f is not None]
        random.Random(seed).shuffle(order)
        total = sum(len(s) + GAP + 16 for s in streams) + sum((reads[k]["frags"][i] or 0) + GAP + 16 for k, i in order)
        self.buf = engine.DeviceBuffer(total + GAP + 32)
        assert self.buf.ptr % 16 == 0
        at, self.src = GAP, []
        for k, s in enumerate(streams):
            at = (at + 15) // 16 * 16 + SRES[k % len(SRES)]
            self.src.append(at)
            at += len(s) + GAP
        self.frag = [[None] * len(r["frags"]) for r in reads]  # offsets in the allocation
        for j, (k, i) in enumerate(order):
            at = (at + 15) // 16 * 16 + FRES[j % len(FRES)]
            self.frag[k][i] = at
            at += reads[k]["frags"][i] + GAP
        assert at <= self.buf.nbytes
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        for s, o in zip(streams, self.src):
            self.image[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.buf.upload(self.image)
        self.lens = [len(s) for s in streams]

    def stream_ptr(self, r):
        return self.buf.ptr + self.src[r["s"]]

    def iov(self, k):
        return [(None if o is None else self.buf.ptr + o, f or 0) for o, f in zip(self.frag[k], self.reads[k]["frags"])]

    def batch(self, pv):
        return [pv.entry(self.stream_ptr(r), self.lens[r["s"]], self.iov(k), r["off"], r["n"])
                for k, r in enumerate(self.reads)]

    def check(self, delivered):
        """The whole allocation.  delivered[k]: the bytes read k delivered, laid
        over its fragments in order (None: its fragments are untouched).
        Behind them the fragments are unspecified up to destination position
        min(cap, read_len) and untouched from there on; nothing else changed."""
        want, got = self.image.copy(), self.buf.download()
        for k, (r, pl) in enumerate(zip(self.reads, delivered or [])):
            if pl is None:
                continue
            data, y, loose = np.frombuffer(pl, dtype=np.uint8), 0, min(cap_of(r), r["n"])
            for o, f in zip(self.frag[k], r["frags"]):
                if not f:
                    continue
                take = max(0, min(f, len(pl) - y))
                want[o:o + take] = data[y:y + take]
                got[o + take:o + max(take, min(f, loose - y))] = GUARD
                y += f
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (streams {self.src[:8]}): "
                                 f"got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def reference(engine, oracle, scratch, arena, streams, r, proto, ctype, cs, max_pkts):
    """Read r's expected (rc, records, consumed, bytes): the oracle's, which the
    main library's read of the same device bytes into a scatter list of the
    same lengths (in the scratch buffer, 7 bytes apart) must give too."""
    s, cap = streams[r["s"]], cap_of(r)
    rc, recs, used, data = oracle.read_packets(s, r["off"], r["n"], proto, cs, ctype, max_pkts, cap)
    iov, at = [], 0
    for f in r["frags"]:
        iov.append((scratch.ptr + at if f else None, f or 0))
        at += (f or 0) + 7
    assert at <= scratch.nbytes
    erc, erecs, eused, egot = engine.read_packets(arena.stream_ptr(r), len(s), None, 0, proto, cs, ctype, max_pkts,
                                                  r["off"], r["n"], iov=iov)
    assert (erc, fields(erecs), eused, egot) == (rc, fields(recs), used, len(data)), r
    img = scratch.download(at)
    joined = b"".join(img[p - scratch.ptr:p - scratch.ptr + n].tobytes() for p, n in iov if n)
    assert joined[:egot] == data, r
    return rc, recs, used, data


def compare(got, want, paths):
    """Every entry's outputs, and every entry's path: none left out."""
    assert len(got) == len(want) == len(paths)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["rc"], g["consumed"], g["delivered"]) == (w[0], w[2], len(w[3])), (k, g["rc"], g["consumed"],
                                                                                    g["delivered"], w[0], w[2])
        if g["records"] is not None:
            assert fields(g["records"]) == fields(w[1]), k
        assert g["path"] == paths[k], (k, g["path"])


def run(pv, engine, oracle, scratch, streams, reads, paths, proto=2, ctype=2, cs=512, max_pkts=None, groups=None,
        stream=None, records=True, want=None, arena=None):
    """Places the streams and fragments, serves the batch (groups: through the
    timing entry with that many workgroups, so without records) and checks
    every entry against its reference and its path, and the whole arena.
    -> (results, references, arena)."""
    a = arena or Arena(engine, streams, reads)
    mp = MANY if max_pkts is None else max_pkts
    if want is None:
        want = [reference(engine, oracle, scratch, a, streams, r, proto, ctype, cs, mp) for r in reads]
    if groups is None:
        got = pv.read(a.batch(pv), proto, cs, ctype, (64 if max_pkts is None else mp) if records else None, stream)
    else:
        ms, got = pv.time(a.batch(pv), proto, cs, ctype, pv.time_groups(groups), 1)
        assert ms > 0
    compare(got, want, paths)
    a.check([w[3] for w in want])
    return got, want, a
