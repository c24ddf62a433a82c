"""The wire streams of a batch of writes in one pass and one launch:
hdfs_wire_fused_batch_compose against the two ways of doing the same job
without it, for DESIGN.md section 17 and the comment of
include/hadoofus_wire_fused_batch.h.

For each shape (writes x bytes per write at a block offset; CRC32C, v2,
finish; distinct sources at odd addresses, all buffers allocated beforehand),
in one process:
  A, fused batch:  hdfs_wire_fused_batch_compose, one call for all writes;
  B, fused loop:   hdfs_wire_fused_compose_packets, one call per write;
  C, batch:        hdfs_wire_batch_compose (two passes), one call for all.
The host clock runs around each whole path (each ends synchronised).  All three
give the same bytes (asserted: every stream of every path is downloaded once
per shape and compared).  Medians of --reps with the three paths alternated
after a warm-up of each (one ahead of the comparison, one behind it), with the
min-max spread, per write.  `verdict` is
"faster" only where A's whole range lies below both other ranges, "slower"
where it lies above one of them, else "overlaps".

Then the kernels alone through the three timing entries (HIP events around
back-to-back launches): the fused batch kernel on the product's grid, the
two-pass library's frame kernel (after its CRC array is filled; the CRC pass is
not in it), and the fused kernel of one write (times the number of writes:
what the loop's kernels add up to).  `layout_us` is
hdfs_wire_fused_batch_layout alone, the host's walk over every packet.

The last shape, 65 536 writes of one 512-B packet (no finish), is the lookup's
worst case: there the fused batch kernel alone is also compared with the same
32 MiB as ONE write through hdfs_wire_fused_time, which has no lookup.
GPU box only.

    python tools/wire_fused_batch_bench.py [--reps 5] [--quick] [--shapes small|large|all] [--out file.json]
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
from hadoofus_amd import wire_batch, wire_fused, wire_fused_batch  # noqa: E402
from hadoofus_amd.abi import OutPacket  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, h.CSUM_CRC32C)
LARGE = [(16, 128 * MIB, 0, True), (16, 128 * MIB, 4321, True), (64, 128 * MIB, 0, True), (64, 128 * MIB, 4321, True)]
SMALL = [(64, MIB, 0, True), (64, 8 * MIB, 0, True), (1024, 65536, 0, True), (65536, 512, 0, False)]


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _stats(xs, nwrites):
    us = lambda x: round(x * 1e6 / nwrites, 3)  # noqa: E731  (per write)
    return {"us": us(_median(xs)), "min_us": us(min(xs)), "max_us": us(max(xs))}


def measure_shape(src, dsts, nwrites, n, off, finish, reps, iters):
    flib, slib, blib = wire_fused_batch.load(), wire_fused.load(), wire_batch.load()
    wl, recs = wire_fused.packet_records(n, off, 0, *ARGS, finish)
    npk = len(recs)
    stride_s, stride_d = (n + 64) // 16 * 16 + 16, (wl + 64) // 16 * 16
    sp = [src.ptr + k * stride_s + 1 for k in range(nwrites)]
    writes = [[wire_fused_batch.write(sp[k], n, d.ptr + k * stride_d, wl, off, 0, finish) for k in range(nwrites)]
              for d in dsts]
    arr_a, arr_c = wire_fused_batch.entries(writes[0]), wire_batch.entries(writes[2])
    pk_all, pk_one = (OutPacket * (npk * nwrites))(), (OutPacket * npk)()
    cnt, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    tot = wire_fused_batch.Totals()

    def path_a():
        t0 = time.perf_counter()
        rc = flib.hdfs_wire_fused_batch_compose(arr_a, nwrites, *ARGS, pk_all, npk * nwrites, ctypes.byref(cnt), None)
        t = time.perf_counter() - t0
        assert rc == 0, flib.hdfs_wire_fused_batch_last_error()
        return t

    def path_b():
        t0 = time.perf_counter()
        for k in range(nwrites):
            rc = slib.hdfs_wire_fused_compose_packets(sp[k], n, off, 0, *ARGS, int(finish),
                                                      dsts[1].ptr + k * stride_d, wl, pk_one, npk, ctypes.byref(cnt),
                                                      ctypes.byref(used), None)
            assert rc == 0, slib.hdfs_wire_fused_last_error()
        return time.perf_counter() - t0

    def path_c():
        t0 = time.perf_counter()
        rc = blib.hdfs_wire_batch_compose(arr_c, nwrites, *ARGS, pk_all, npk * nwrites, ctypes.byref(cnt), None)
        t = time.perf_counter() - t0
        assert rc == 0, blib.hdfs_wire_batch_last_error()
        return t

    def layout_only():
        t0 = time.perf_counter()
        assert flib.hdfs_wire_fused_batch_layout(arr_a, nwrites, *ARGS, ctypes.byref(tot)) == 0
        return time.perf_counter() - t0

    paths = (path_a, path_b, path_c)
    for p in paths:  # warm-up: code objects, scratch growth
        p()
    per = max(1, (256 * MIB) // stride_d)  # streams per download
    for k0 in range(0, nwrites, per):
        k1 = min(nwrites, k0 + per)
        got = [d.download((k1 - k0) * stride_d, k0 * stride_d).reshape(k1 - k0, stride_d)[:, :wl] for d in dsts]
        assert np.array_equal(got[0], got[1]), f"fused batch and fused loop differ in writes {k0}..{k1}"
        assert np.array_equal(got[0], got[2]), f"fused batch and two-pass batch differ in writes {k0}..{k1}"
    for p in paths:  # and once more, behind the downloads
        p()
    t = [[], [], []]
    for _ in range(reps):  # alternate the three paths
        for i, p in enumerate(paths):
            t[i].append(p())
    a, b, c = (_stats(x, nwrites) for x in t)
    if a["max_us"] < min(b["min_us"], c["min_us"]):
        verdict = "faster"
    elif a["min_us"] > min(b["max_us"], c["max_us"]):
        verdict = "slower"
    else:
        verdict = "overlaps"
    lay = _median([layout_only() for _ in range(reps)])
    k_a = _median([wire_fused_batch.fused_batch_time(writes[0], *ARGS, 0, iters) for _ in range(3)])
    k_c = _median([wire_batch.frame_time(writes[2], *ARGS, iters) for _ in range(3)])
    k_b = _median([wire_fused.fused_time(sp[0], n, dsts[1].ptr, wl, off, *ARGS, finish, 0, iters) for _ in range(3)])
    row = {"writes": nwrites, "write_bytes": n, "offset_in_block": off, "finish": finish, "packets": npk * nwrites,
           "fused_batch": a, "fused_loop": b, "batch": c, "verdict": verdict,
           "layout_us": round(lay * 1e6 / nwrites, 3),
           "kernel_us": {"fused_batch": round(k_a * 1e3 / nwrites, 3), "batch_frame_only": round(k_c * 1e3 / nwrites, 3),
                         "fused_one_write": round(k_b * 1e3, 3)},
           "fused_batch_kernel_TBps": round(nwrites * (n + wl) / (k_a * 1e-3) / 1e12, 3)}
    if n * nwrites <= 64 * MIB and not finish and off == 0:
        # the same bytes as ONE write (contiguous source needed: the sources are stride_s apart, so its own copy)
        whole = n * nwrites
        wl1, _ = wire_fused.packet_records(whole, 0, 0, *ARGS, False)
        k_1 = _median([wire_fused.fused_time(src.ptr + 1, whole, dsts[1].ptr, wl1, 0, *ARGS, False, 0, iters)
                       for _ in range(3)])
        row["one_write_of_the_same_bytes_kernel_ms"] = round(k_1, 4)
        row["fused_batch_kernel_ms"] = round(k_a, 4)
    return row


def measure(reps=5, shapes="all", quick=False):
    h.load()
    arch, ncu = h.device_info()
    todo = {"small": SMALL, "large": LARGE, "all": LARGE + SMALL}[shapes]
    if quick:
        todo = [s for s in todo if s[0] * s[1] <= 64 * MIB]
    need_s = max(nw * ((n + 64) // 16 * 16 + 16) for nw, n, _, _ in todo) + 64
    need_d = max(nw * ((n + n // 100 + 4096) // 16 * 16) for nw, n, _, _ in todo) + MIB
    src = h.DeviceBuffer(need_s)
    dsts = [h.DeviceBuffer(need_d) for _ in range(3)]
    h.fill_splitmix64(src.ptr, src.nbytes // 8, 17, 0)
    h.device_sync()
    rows = []
    try:
        for nwrites, n, off, finish in todo:
            rows.append(measure_shape(src, dsts, nwrites, n, off, finish, reps, 10))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    finally:
        for b in [src] + dsts:
            b.free()
    return {"arch": arch, "num_cu": ncu, "reps": reps, "rows": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="only shapes of at most 64 MiB in all")
    ap.add_argument("--shapes", choices=["small", "large", "all"], default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reps, a.shapes, a.quick)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
