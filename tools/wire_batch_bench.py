"""The wire streams of a batch of writes: one hdfs_wire_batch_compose call
against a loop of hdfs_wire_compose_packets calls over the same writes, for
DESIGN.md section 14 and the comment of include/hadoofus_wire_batch.h.

For batches of 16 and 64 writes of 128 MiB (one pass with every write at block
offset 0, one with 4321; CRC32C, v2, finish; distinct sources at odd
addresses, all buffers allocated beforehand), in one process:
  A, batch:  hdfs_wire_batch_compose, one call for all writes;
  B, loop:   hdfs_wire_compose_packets, one call per write.
The host clock runs around each whole path (each ends synchronised).  Both
give the same bytes (asserted, every stream of both paths downloaded once per
batch).  Medians of --reps with the two paths alternated after a warm-up of
each, with the min-max spread.

`layout_ms` is hdfs_wire_batch_layout alone (the host's walk over every
packet of every write, no GPU): the part of path A that grows with the packet
count on the host.  Then the batch frame kernel alone
(hdfs_wire_batch_frame_time: HIP events around back-to-back launches, after the
CRC array is filled).  Traffic per launch: reads len + 4 B per chunk, writes
the streams.  GPU box only.

    python tools/wire_batch_bench.py [--reps 5] [--quick] [--out file.json]
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
from hadoofus_amd import wire, wire_batch  # noqa: E402
from hadoofus_amd.abi import OutPacket  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, h.CSUM_CRC32C)


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def measure_batch(src, dst_a, dst_b, nwrites, n, off, reps, iters):
    wlib, blib = wire.load(), wire_batch.load()
    info = wire.layout(n, off, *ARGS, True)
    wl, npk = info["wire_len"], info["npkts"]
    stride_s, stride_d = n + 4096, (wl + 4096) // 16 * 16
    writes_a = [wire_batch.write(src.ptr + k * stride_s + 1, n, dst_a.ptr + k * stride_d, wl, off, 0, True)
                for k in range(nwrites)]
    arr = wire_batch.entries(writes_a)
    pk_a, pk_b = (OutPacket * (npk * nwrites))(), (OutPacket * npk)()
    cnt, cnt_b, used = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
    tot = wire_batch.Totals()

    def path_a():
        t0 = time.perf_counter()
        rc = blib.hdfs_wire_batch_compose(arr, nwrites, *ARGS, pk_a, npk * nwrites, ctypes.byref(cnt), None)
        t = time.perf_counter() - t0
        assert rc == 0, blib.hdfs_wire_batch_last_error()
        return t

    def path_b():
        t0 = time.perf_counter()
        for k in range(nwrites):
            rc = wlib.hdfs_wire_compose_packets(src.ptr + k * stride_s + 1, n, off, 0, *ARGS, 1,
                                                dst_b.ptr + k * stride_d, wl, pk_b, npk, ctypes.byref(cnt_b),
                                                ctypes.byref(used), None)
            assert rc == 0, wlib.hdfs_wire_last_error()
        return time.perf_counter() - t0

    def layout_only():
        t0 = time.perf_counter()
        assert blib.hdfs_wire_batch_layout(arr, nwrites, *ARGS, ctypes.byref(tot)) == 0
        return time.perf_counter() - t0

    path_a()  # warm-up: code objects, scratch growth
    path_b()
    for k in range(nwrites):  # both paths' streams, one write at a time
        assert np.array_equal(dst_a.download(wl, k * stride_d), dst_b.download(wl, k * stride_d)), \
            f"the two paths differ in write {k}"
    assert cnt.value == npk * nwrites and bytes(pk_a)[-ctypes.sizeof(pk_b):] == bytes(pk_b)
    a, b = [], []
    for _ in range(reps):  # alternate the two paths
        a.append(path_a())
        b.append(path_b())
    lay = _median([layout_only() for _ in range(reps)])
    kern = _median([wire_batch.frame_time(writes_a, *ARGS, iters) for _ in range(3)])
    traffic = nwrites * (n + 4 * info["nchunks"] + wl)
    us = lambda x: round(x * 1e6 / nwrites, 2)  # noqa: E731  (per block)
    return {"writes": nwrites, "write_mib": n / MIB, "offset_in_block": off, "packets": npk * nwrites,
            "batch_ms": round(_median(a) * 1e3, 3), "loop_ms": round(_median(b) * 1e3, 3),
            "batch_us_per_block": us(_median(a)), "batch_min_us": us(min(a)), "batch_max_us": us(max(a)),
            "loop_us_per_block": us(_median(b)), "loop_min_us": us(min(b)), "loop_max_us": us(max(b)),
            "loop_over_batch": round(_median(b) / _median(a), 2),
            "layout_ms": round(lay * 1e3, 3), "layout_us_per_block": us(lay),
            "kernel_ms": round(kern, 4), "kernel_us_per_block": round(kern * 1e3 / nwrites, 2),
            "kernel_traffic_TBps": round(traffic / (kern * 1e-3) / 1e12, 2)}


def measure(reps=5, quick=False):
    h.load()
    arch, ncu = h.device_info()
    n = 128 * MIB
    counts = [16] if quick else [16, 64]
    most = max(counts)
    wl = wire.layout(n, 4321, *ARGS, True)["wire_len"]
    src = h.DeviceBuffer(most * (n + 4096))
    dst_a, dst_b = (h.DeviceBuffer(most * ((wl + 4096) // 16 * 16)) for _ in range(2))
    h.fill_splitmix64(src.ptr, src.nbytes // 8, 13, 0)
    h.device_sync()
    rows = []
    try:
        for nwrites in counts:
            for off in (0, 4321):
                rows.append(measure_batch(src, dst_a, dst_b, nwrites, n, off, reps, 10))
    finally:
        for b in (src, dst_a, dst_b):
            b.free()
    return {"arch": arch, "num_cu": ncu, "reps": reps, "rows": rows,
            "loop_faster_at": [(r["writes"], r["offset_in_block"]) for r in rows if r["loop_ms"] <= r["batch_ms"]]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batches of 16 only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reps, a.quick)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
