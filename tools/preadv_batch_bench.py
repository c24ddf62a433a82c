"""A batch of scatter reads in one call: hdfs_preadv_batch_read against the ways
of doing the job without it, for DESIGN.md section 22 and the comment of
include/hadoofus_preadv_batch.h.

For each shape (N reads of one window size, each into F device fragments of
equal length 16 bytes apart; v2, CRC32C; every read's packet stream composed on
the device beforehand by the fused batch write library at a block offset of
its own, with the empty last packet, at odd addresses; all buffers allocated
beforehand), in one process:
  A, batch: hdfs_preadv_batch_read, one call for all reads, records kept;
  B, loop:  hdfs_crc32c_read_packets with the read's window and the same
            fragment list, one call per read: the main library as it stands;
  C, pread: hdfs_pread_batch_read of the same reads into contiguous buffers: a
            floor that leaves the caller's scatter undone.
The host clock runs around each whole path (each ends synchronised).  A and B
give the same outputs, records and bytes, and A's bytes joined are C's
(asserted once per shape).  Medians of --reps with the three paths alternated
after one warm-up of each, with the min-max spread, per read.  `verdict` is
"faster" only where A's whole range lies below B's, "slower" where it lies
above, else "overlaps"; `vs_pread` the same against C.  Beside it the two
launches alone, from the timing entry (HIP events around back-to-back probe +
main launches), and how many entries took each path.
GPU box only.

    python tools/preadv_batch_bench.py [--reps 5] [--quick] [--out file.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hadoofus_amd as h  # noqa: E402
from hadoofus_amd import wire_fused_batch  # noqa: E402
from hadoofus_amd.abi import IoVec, Packet  # noqa: E402
from hadoofus_read import pread_batch, preadv_batch  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, 512, h.CSUM_CRC32C)
PACKET = 65536  # data bytes of the packets the fused batch write library composes
STRIDE = 31 + 4 * (PACKET // 512) + PACKET  # their wire bytes (v2)
GAP = 16  # bytes between two fragments of a read
# (name, reads, window bytes, composed stream's payload bytes, c_begin, packets of the composed stream skipped):
# the rows of tools/pread_batch_bench.py
ROWS = [("256 x 64 KiB of a 64.5 KiB stream", 256, 65536, 65536 + 512, 100, 0),
        ("1024 x 4 KiB of a 4.5 KiB stream", 1024, 4096, 4096 + 512, 100, 0),
        ("64 x 1 MiB of a 1 MiB + 512 B stream", 64, MIB, MIB + 512, 300, 0),
        ("16 x (128 MiB - 1000 B) of a 128 MiB stream", 16, 128 * MIB - 1000, 128 * MIB, 500, 0),
        ("256 x 64 KiB from packet 12 on of a 2 MiB stream", 256, 65536, 2 * MIB, 30000, 12)]
FRAGS = (1, 16, 1024)
# each with 1, 16 and 1 024 fragments a read, and one row of 4 KiB reads in 64-B fragments
SHAPES = [r + (f,) for r in ROWS for f in FRAGS] + [ROWS[1] + (64,)]


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _stats(xs, n):
    us = lambda x: round(x * 1e6 / n, 3)  # noqa: E731  (per read)
    return {"us": us(_median(xs)), "min_us": us(min(xs)), "max_us": us(max(xs))}


def _verdict(a, b):
    return "faster" if a["max_us"] < b["min_us"] else "slower" if a["min_us"] > b["max_us"] else "overlaps"


def _iovecs(base, window, nf):
    """nf fragments of window // nf bytes (the last takes the rest), GAP bytes apart, from base on.
    -> (IoVec array, bytes from base to the last fragment's end)."""
    flen = window // nf
    raw = np.zeros((nf, 2), dtype=np.uint64)
    raw[:, 0] = base + np.arange(nf, dtype=np.uint64) * np.uint64(flen + GAP)
    raw[:, 1] = flen
    raw[nf - 1, 1] = window - flen * (nf - 1)
    arr = (IoVec * nf)()
    ctypes.memmove(arr, raw.ctypes.data, raw.nbytes)
    return arr, (nf - 1) * (flen + GAP) + int(raw[nf - 1, 1])


def measure_shape(name, nb, window, payload, c_begin, skip, nf, src, wires, dsts, reps, iters):
    vlib, plib, lib = preadv_batch.load(), pread_batch.load(), h.load()
    block0 = [512 * (1000 + 77 * k) for k in range(nb)]  # each stream's first byte in its block: a chunk boundary
    writes = [wire_fused_batch.write(nbytes=payload, offset_in_block=block0[k], finish=True) for k in range(nb)]
    outs, _ = wire_fused_batch.layout(writes, ARGS[0], ARGS[2])
    wl, npk = [o["wire_len"] for o in outs], [o["npkts"] for o in outs]
    span = _iovecs(0, window, nf)[1]
    at_w, at_d, a, b = [], [], 5, 3
    for k in range(nb):
        at_w.append(a)
        at_d.append(b)
        a += (wl[k] + 64) // 16 * 16 + 1
        b += (span + 64) // 16 * 16 + 2
    assert a <= wires.nbytes and b <= dsts[0].nbytes
    wire_fused_batch.compose([wire_fused_batch.write(src.ptr + 1 + (k % 7), payload, wires.ptr + at_w[k], wl[k],
                                                     block0[k], 0, True) for k in range(nb)], ARGS[0], ARGS[2])
    for d in dsts[:2]:  # the same bytes between the fragments of A and of B
        h.fill_splitmix64(d.ptr, b // 8 + 1, 23, 0)
    h.device_sync()
    mp = max(npk)
    if skip:  # the entries' streams start at packet `skip` of the composed ones
        assert all(w == (payload // PACKET) * STRIDE + 31 for w in wl) and payload % PACKET == 0
        at_w = [a + skip * STRIDE for a in at_w]
        wl = [w - skip * STRIDE for w in wl]
        block0 = [b + skip * PACKET for b in block0]
        payload -= skip * PACKET
    iov_a = [_iovecs(dsts[0].ptr + at_d[k], window, nf)[0] for k in range(nb)]
    iov_b = [_iovecs(dsts[1].ptr + at_d[k], window, nf)[0] for k in range(nb)]
    ent = (preadv_batch.Entry * nb)()
    for k, e in enumerate(ent):
        e.stream, e.len, e.iov, e.iovcnt = wires.ptr + at_w[k], wl[k], iov_a[k], nf
        e.client_offset, e.read_len = block0[k] + c_begin, window
    flat = [(window + 64) // 16 * 16 * k + 2 for k in range(nb)]
    assert flat[-1] + window <= dsts[2].nbytes
    ent_c = pread_batch.entries([pread_batch.entry(wires.ptr + at_w[k], wl[k], dsts[2].ptr + flat[k], window,
                                                   block0[k] + c_begin, window) for k in range(nb)])
    pk_a, pk_b, pk_c = (Packet * (mp * nb))(), (Packet * (mp * nb))(), (Packet * (mp * nb))()
    cnt, used, got = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    out_b = [None] * nb
    rec_b = [ctypes.cast(ctypes.addressof(pk_b) + k * mp * ctypes.sizeof(Packet), ctypes.POINTER(Packet))
             for k in range(nb)]

    def path_a():
        t0 = time.perf_counter()
        rc = vlib.hdfs_preadv_batch_read(ent, nb, *ARGS, pk_a, mp, None)
        t = time.perf_counter() - t0
        assert rc == 0, (rc, vlib.hdfs_preadv_batch_last_error())
        return t

    def path_b():
        t0 = time.perf_counter()
        for k in range(nb):
            rc = lib.hdfs_crc32c_read_packets(wires.ptr + at_w[k], wl[k], *ARGS, block0[k] + c_begin, window,
                                              iov_b[k], nf, rec_b[k], mp, ctypes.byref(cnt), ctypes.byref(used),
                                              ctypes.byref(got))
            assert rc == 0, (k, rc)
            out_b[k] = (rc, cnt.value, used.value, got.value)
        return time.perf_counter() - t0

    def path_c():
        t0 = time.perf_counter()
        rc = plib.hdfs_pread_batch_read(ent_c, nb, *ARGS, pk_c, mp, None)
        t = time.perf_counter() - t0
        assert rc == 0, (rc, plib.hdfs_pread_batch_last_error())
        return t

    paths = (path_a, path_b, path_c)
    for p in paths:  # warm-up: code objects, scratch growth
        p()
    # A and B give the same outputs, records and bytes (the whole region, fragments and gaps); A's bytes joined are C's
    size = ctypes.sizeof(Packet)
    for k in range(nb):
        e = ent[k]
        assert (e.rc, e.npkts, e.consumed, e.delivered) == out_b[k], (k, out_b[k])
        assert e.delivered == window
        assert bytes(pk_a)[k * mp * size:(k * mp + e.npkts) * size] == bytes(pk_b)[k * mp * size:(k * mp + e.npkts) * size], k
    some, flen = sorted({0, nb // 2, nb - 1}), window // nf
    for k in range(nb) if nb * span <= 512 * MIB else some:  # (three reads of the largest shapes)
        img_a = dsts[0].download(span, at_d[k])
        assert np.array_equal(img_a, dsts[1].download(span, at_d[k])), k
        if k in some:
            joined = np.concatenate([img_a[i * (flen + GAP):i * (flen + GAP) +
                                           (flen if i < nf - 1 else window - flen * (nf - 1))] for i in range(nf)])
            assert np.array_equal(joined, dsts[2].download(window, flat[k])), k
    n_kernel = sum(1 for k in range(nb) if ent[k].path == preadv_batch.PATH_KERNEL)
    t = [[], [], []]
    for _ in range(reps):  # alternate the three paths
        for i, p in enumerate(paths):
            t[i].append(p())
    sa, sb, sc = (_stats(x, nb) for x in t)
    ms = []
    for _ in range(3):
        one = ctypes.c_double(0)
        rc = vlib.hdfs_preadv_batch_time(ent, nb, *ARGS, 0, iters, ctypes.byref(one))
        assert rc == 0, (rc, vlib.hdfs_preadv_batch_last_error())
        ms.append(one.value)
    return {"shape": name, "reads": nb, "window": window, "frags_per_read": nf, "frag_bytes": window // nf,
            "c_begin": c_begin, "skipped_packets": skip, "kernel_path": n_kernel, "fallback_path": nb - n_kernel,
            "batch": sa, "loop": sb, "pread_batch": sc, "verdict": _verdict(sa, sb), "vs_pread": _verdict(sa, sc),
            "launches_us_per_read": round(_median(ms) * 1e3 / nb, 3)}


def measure(reps=5, quick=False):
    h.load()
    arch, ncu = h.device_info()
    todo = [s for s in SHAPES if not quick or s[1] * s[3] <= 300 * MIB]
    most_w = max(s[1] * (s[2] + GAP * s[6]) for s in todo)
    most_p = max(s[1] * s[3] for s in todo)
    reads = max(s[1] for s in todo)
    src = h.DeviceBuffer(max(s[3] for s in todo) + 64)
    wires = h.DeviceBuffer(most_p + most_p // 100 + reads * 4096 + MIB)
    dsts = [h.DeviceBuffer(most_w + reads * 128 + MIB) for _ in range(3)]
    h.fill_splitmix64(src.ptr, src.nbytes // 8, 17, 0)
    h.device_sync()
    rows = []
    try:
        for name, nb, window, payload, c_begin, skip, nf in todo:
            rows.append(measure_shape(name, nb, window, payload, c_begin, skip, nf, src, wires, dsts, reps, 5))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    finally:
        for b in [src, wires] + dsts:
            b.free()
    return {"arch": arch, "num_cu": ncu, "reps": reps, "rows": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="only shapes of at most 300 MiB of streams in all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reps, a.quick)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
