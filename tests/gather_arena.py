"""Helpers of the GPU tests of the fused gather libraries
(tests/test_gpu_wirev_fused.py keeps its own copies of `expect`, `cut` and a
one-write arena; tests/test_gpu_wirev_fused_batch.py uses these): the expected
stream of a write built from the CPU oracle, and one device allocation in
which any number of source buffers and destinations are carved between 0xA5
guards at chosen byte residues mod 16 and which is downloaded and compared as
a whole after every call."""
import numpy as np

GUARD = 0xA5
GAP = 96  # guard bytes before, between and after the ranges (at least)


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


def cut(data, lens):
    assert sum(lens) == len(data)
    ends = np.cumsum(lens) if len(lens) else []
    return [data[e - n:e] for n, e in zip(lens, ends)]


def room(nbytes, nranges):
    """Bytes of an arena for nranges ranges of nbytes bytes in all."""
    return nbytes + (GAP + 32) * (nranges + 2)


class Arena:
    """One device allocation.  begin(); put() every source buffer and wire()
    every destination, in the address order wanted; commit() uploads the image
    (guards everywhere else); after a call, check(streams) downloads all of it:
    destination i holds streams[i] and then guards, nothing else changed."""

    def __init__(self, engine, nbytes):
        self.buf = engine.DeviceBuffer(nbytes)
        assert self.buf.ptr % 16 == 0
        self.begin()

    def begin(self):
        self.image = np.full(self.buf.nbytes, GUARD, dtype=np.uint8)
        self.at, self.wires = 0, []

    def _carve(self, n, mis):
        at = (self.at + GAP + 15) // 16 * 16 + mis
        self.at = at + n
        assert self.at + GAP <= self.buf.nbytes, (self.at, self.buf.nbytes)
        return at

    def put(self, piece, mis=0):
        """-> the device pointer of a copy of piece at residue mis (None: no bytes)."""
        if not len(piece):
            return None
        at = self._carve(len(piece), mis)
        self.image[at:at + len(piece)] = piece
        return self.buf.ptr + at

    def wire(self, nbytes, mis=0):
        """-> the device pointer of nbytes of destination at residue mis."""
        at = self._carve(nbytes, mis)
        self.wires.append((at, nbytes))
        return self.buf.ptr + at

    def commit(self):
        self.buf.upload(self.image)

    def check(self, streams=()):
        want = self.image.copy()
        for (at, n), s in zip(self.wires, streams):
            assert len(s) <= n
            want[at:at + len(s)] = s
        got = self.buf.download()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (destinations {self.wires[:8]}): "
                                 f"got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")
