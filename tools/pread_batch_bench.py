"""A batch of positional reads in one call: hdfs_pread_batch_read against the
ways of doing the job without it, for DESIGN.md section 21 and the comment of
include/hadoofus_pread_batch.h.

For each shape (N reads of one window size; v2, CRC32C; every read's packet
stream composed on the device beforehand by the fused batch write library at a
block offset of its own, with the empty last packet, at odd addresses; all
buffers allocated beforehand), in one process:
  A, batch:    hdfs_pread_batch_read, one call for all reads, records kept;
  B, loop:     hdfs_crc32c_read_packets with the read's window (device stream
               to device buffer), one call per read: the main library as it
               stands;
  C, read_all: hdfs_read_batch_read_blocks of the same streams, which delivers
               every stream's whole payload (the skipped head and whatever
               lies behind the read included) into buffers of that size: what
               a caller without this library could do in one call, then copy
               the window out (the copy is not timed).
The host clock runs around each whole path (each ends synchronised).  A and B
give the same outputs, records and bytes (asserted once per shape).  Medians of
--reps with the three paths alternated after one warm-up of each, with the
min-max spread, per read.  `verdict` is "faster" only where A's whole range
lies below B's, "slower" where it lies above, else "overlaps"; `vs_read_all`
the same against C.  Beside it the two launches alone, from the timing entry
(HIP events around back-to-back probe + main launches), and how many entries
took each path.
GPU box only.

    python tools/pread_batch_bench.py [--reps 5] [--quick] [--out file.json]
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
from hadoofus_read import pread_batch, read_batch  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, 512, h.CSUM_CRC32C)
PACKET = 65536  # data bytes of the packets the fused batch write library composes
STRIDE = 31 + 4 * (PACKET // 512) + PACKET  # their wire bytes (v2)
# (name, reads, window bytes, composed stream's payload bytes, c_begin, packets of the composed stream skipped).
# skip > 0: the entry's stream is taken from the middle of the composed one -- it starts at packet `skip`, so its
# first packet names a later offsetInBlock and seqno, and it goes on long behind the read.
SHAPES = [("256 x 64 KiB of a 64.5 KiB stream", 256, 65536, 65536 + 512, 100, 0),
          ("1024 x 4 KiB of a 4.5 KiB stream", 1024, 4096, 4096 + 512, 100, 0),
          ("64 x 1 MiB of a 1 MiB + 512 B stream", 64, MIB, MIB + 512, 300, 0),
          ("16 x (128 MiB - 1000 B) of a 128 MiB stream", 16, 128 * MIB - 1000, 128 * MIB, 500, 0),
          ("256 x 64 KiB from packet 12 on of a 2 MiB stream", 256, 65536, 2 * MIB, 30000, 12)]


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _stats(xs, n):
    us = lambda x: round(x * 1e6 / n, 3)  # noqa: E731  (per read)
    return {"us": us(_median(xs)), "min_us": us(min(xs)), "max_us": us(max(xs))}


def _verdict(a, b):
    return "faster" if a["max_us"] < b["min_us"] else "slower" if a["min_us"] > b["max_us"] else "overlaps"


def measure_shape(name, nb, window, payload, c_begin, skip, src, wires, dsts, whole, reps, iters):
    plib, rlib, lib = pread_batch.load(), read_batch.load(), h.load()
    block0 = [512 * (1000 + 77 * k) for k in range(nb)]  # each stream's first byte in its block: a chunk boundary
    writes = [wire_fused_batch.write(nbytes=payload, offset_in_block=block0[k], finish=True) for k in range(nb)]
    outs, _ = wire_fused_batch.layout(writes, ARGS[0], ARGS[2])
    wl, npk = [o["wire_len"] for o in outs], [o["npkts"] for o in outs]
    at_w, at_d, at_p, a, b, c = [], [], [], 5, 3, 7
    for k in range(nb):
        at_w.append(a)
        at_d.append(b)
        at_p.append(c)
        a += (wl[k] + 64) // 16 * 16 + 1
        b += (window + 64) // 16 * 16 + 2
        c += (payload + 64) // 16 * 16 + 2
    assert a <= wires.nbytes and b <= dsts[0].nbytes and c <= whole.nbytes
    wire_fused_batch.compose([wire_fused_batch.write(src.ptr + 1 + (k % 7), payload, wires.ptr + at_w[k], wl[k],
                                                     block0[k], 0, True) for k in range(nb)], ARGS[0], ARGS[2])
    mp = max(npk)
    if skip:  # the entries' streams start at packet `skip` of the composed ones
        assert all(w == (payload // PACKET) * STRIDE + 31 for w in wl) and payload % PACKET == 0
        at_w = [a + skip * STRIDE for a in at_w]
        wl = [w - skip * STRIDE for w in wl]
        block0 = [b + skip * PACKET for b in block0]
        payload -= skip * PACKET
    ent = pread_batch.entries([pread_batch.entry(wires.ptr + at_w[k], wl[k], dsts[0].ptr + at_d[k], window,
                                                 block0[k] + c_begin, window) for k in range(nb)])
    ent_c = read_batch.entries([read_batch.entry(wires.ptr + at_w[k], wl[k], whole.ptr + at_p[k], payload)
                                for k in range(nb)])
    pk_a, pk_b, pk_c = (Packet * (mp * nb))(), (Packet * (mp * nb))(), (Packet * (mp * nb))()
    cnt, used, got = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    out_b = [None] * nb
    rec_b = [ctypes.cast(ctypes.addressof(pk_b) + k * mp * ctypes.sizeof(Packet), ctypes.POINTER(Packet))
             for k in range(nb)]

    def path_a():
        t0 = time.perf_counter()
        rc = plib.hdfs_pread_batch_read(ent, nb, *ARGS, pk_a, mp, None)
        t = time.perf_counter() - t0
        assert rc == 0, (rc, plib.hdfs_pread_batch_last_error())
        return t

    def path_b():
        t0 = time.perf_counter()
        for k in range(nb):
            iov = IoVec(dsts[1].ptr + at_d[k], window)
            rc = lib.hdfs_crc32c_read_packets(wires.ptr + at_w[k], wl[k], *ARGS, block0[k] + c_begin, window,
                                              ctypes.byref(iov), 1, rec_b[k], mp, ctypes.byref(cnt), ctypes.byref(used),
                                              ctypes.byref(got))
            assert rc == 0, (k, rc)
            out_b[k] = (rc, cnt.value, used.value, got.value)
        return time.perf_counter() - t0

    def path_c():
        t0 = time.perf_counter()
        rc = rlib.hdfs_read_batch_read_blocks(ent_c, nb, *ARGS, pk_c, mp, None)
        t = time.perf_counter() - t0
        assert rc == 0, (rc, rlib.hdfs_read_batch_last_error())
        return t

    paths = (path_a, path_b, path_c)
    for p in paths:  # warm-up: code objects, scratch growth
        p()
    # A and B give the same outputs, records and bytes; C's payload holds the window at c_begin
    for k in range(nb):
        e = ent[k]
        assert (e.rc, e.npkts, e.consumed, e.delivered) == out_b[k], (k, out_b[k])
        assert e.delivered == window
        assert bytes(pk_a)[k * mp * ctypes.sizeof(Packet):(k * mp + e.npkts) * ctypes.sizeof(Packet)] == \
            bytes(pk_b)[k * mp * ctypes.sizeof(Packet):(k * mp + e.npkts) * ctypes.sizeof(Packet)], k
        got_a = dsts[0].download(window, at_d[k])
        assert np.array_equal(got_a, dsts[1].download(window, at_d[k])), k
        assert np.array_equal(got_a, whole.download(window, at_p[k] + c_begin)), k
    n_kernel = sum(1 for k in range(nb) if ent[k].path == pread_batch.PATH_KERNEL)
    taken = sum(ent[k].npkts for k in range(nb))
    in_streams = sum(npk) - skip * nb
    t = [[], [], []]
    for _ in range(reps):  # alternate the three paths
        for i, p in enumerate(paths):
            t[i].append(p())
    sa, sb, sc = (_stats(x, nb) for x in t)
    ms = _median([pread_batch.time([pread_batch.entry(wires.ptr + at_w[k], wl[k], dsts[0].ptr + at_d[k], window,
                                                      block0[k] + c_begin, window) for k in range(nb)],
                                   *ARGS, 0, iters)[0] for _ in range(3)])
    return {"shape": name, "reads": nb, "window": window, "stream_payload": payload, "c_begin": c_begin, "skipped_packets": skip,
            "packets_in_streams": in_streams, "packets_taken": taken, "kernel_path": n_kernel,
            "fallback_path": nb - n_kernel, "batch": sa, "loop": sb, "read_all_batch": sc, "verdict": _verdict(sa, sb),
            "vs_read_all": _verdict(sa, sc), "launches_us_per_read": round(ms * 1e3 / nb, 3)}


def measure(reps=5, quick=False):
    h.load()
    arch, ncu = h.device_info()
    todo = [s for s in SHAPES if not quick or s[1] * s[3] <= 300 * MIB]
    most_w = max(s[1] * s[2] for s in todo)
    most_p = max(s[1] * s[3] for s in todo)
    reads = max(s[1] for s in todo)
    src = h.DeviceBuffer(max(s[3] for s in todo) + 64)
    wires = h.DeviceBuffer(most_p + most_p // 100 + reads * 4096 + MIB)
    dsts = [h.DeviceBuffer(most_w + reads * 128 + MIB) for _ in range(2)]
    whole = h.DeviceBuffer(most_p + reads * 128 + MIB)
    h.fill_splitmix64(src.ptr, src.nbytes // 8, 17, 0)
    h.device_sync()
    rows = []
    try:
        for name, nb, window, payload, c_begin, skip in todo:
            rows.append(measure_shape(name, nb, window, payload, c_begin, skip, src, wires, dsts, whole, reps, 5))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    finally:
        for b in [src, wires, whole] + dsts:
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
