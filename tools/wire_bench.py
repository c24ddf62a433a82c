"""A write's packets as one wire stream in device memory:
hdfs_wire_compose_packets against what a caller can assemble from the main
library alone, for DESIGN.md section 13 and the comment of
include/hadoofus_wire.h.

For each write (128 MiB and 1 GiB, at block offsets 0 and 4321, CRC32C, v2,
finish), in one process:
  A, wire:    hdfs_wire_compose_packets (host clock around the call, which
              ends in a stream synchronise; buffers allocated beforehand);
  B, copies:  hdfs_crc32c_compose_packets on the device buffer, one
              host-to-device copy of the header buffers, then two
              hipMemcpyAsync device-to-device per packet (header buffer,
              data) into a pre-allocated stream, and a stream synchronise.
Both give the same bytes (asserted, whole stream downloaded once per write).
Medians of --reps with the two paths alternated.  Path B's copies are issued
from a Python loop; `loop_ms` is the same loop calling a function that does
nothing, so the interpreter's share can be subtracted.

Then the frame kernel alone (hdfs_wire_frame_time: HIP events around
back-to-back launches, after the CRC array is filled) for 1 MiB, 8 MiB,
128 MiB and 1 GiB at offset 4321: plain and write-through 16-B stores, 1, 2, 4
and 8 workgroups per packet.  Traffic per launch: reads len + 4 B per chunk, writes the stream.
GPU box only.

    python tools/wire_bench.py [--reps 5] [--quick] [--out file.json]
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
from hadoofus_amd import wire  # noqa: E402
from hadoofus_amd.abi import OutPacket  # noqa: E402

MIB = 1 << 20
H2D, D2D = 1, 3  # hipMemcpyHostToDevice, hipMemcpyDeviceToDevice
ARGS = (h.PROTO_V2, h.CSUM_CRC32C, 1)  # proto, ctype, finish


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def measure_write(hip, lib, wlib, src, dst_a, dst_b, hdr_dev, n, off, reps):
    npk, wl, used = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert wlib.hdfs_wire_compose_packets(None, n, off, 0, *ARGS, None, 0, None, 0, ctypes.byref(npk),
                                          ctypes.byref(wl), None) == 0
    cap_n, wire_len = npk.value, wl.value
    pk_a, pk_b = (OutPacket * cap_n)(), (OutPacket * cap_n)()
    hdr_cap = wire_len - n
    hdr = h.PinnedBuffer(hdr_cap)
    sp = src.ptr + 1  # an odd source address

    def path_a():
        t0 = time.perf_counter()
        rc = wlib.hdfs_wire_compose_packets(sp, n, off, 0, *ARGS, dst_a.ptr, wire_len, pk_a, cap_n, ctypes.byref(npk),
                                            ctypes.byref(wl), None)
        t = time.perf_counter() - t0
        assert rc == 0, wlib.hdfs_wire_last_error()
        return t

    def path_b():
        t0 = time.perf_counter()
        rc = lib.hdfs_crc32c_compose_packets(sp, n, off, 0, *ARGS, hdr.ptr, hdr_cap, pk_b, cap_n, ctypes.byref(npk),
                                             ctypes.byref(used))
        t1 = time.perf_counter()
        hip.hipMemcpyAsync(hdr_dev.ptr, hdr.ptr, used.value, H2D, None)
        at = dst_b.ptr
        for i in range(cap_n):
            p = pk_b[i]
            hip.hipMemcpyAsync(at, hdr_dev.ptr + p.hdr_off, p.hdr_len, D2D, None)
            at += p.hdr_len
            if p.data_len:
                hip.hipMemcpyAsync(at, sp + p.data_off, p.data_len, D2D, None)
                at += p.data_len
        t2 = time.perf_counter()
        hip.hipStreamSynchronize(None)
        t3 = time.perf_counter()
        assert rc == 0 and at - dst_b.ptr == wire_len
        return t3 - t0, t1 - t0, t2 - t1

    def empty_loop():
        t0 = time.perf_counter()
        for i in range(cap_n):
            p = pk_b[i]
            lib.hdfs_crc32c_abi_version()
            if p.data_len:
                lib.hdfs_crc32c_abi_version()
        return time.perf_counter() - t0

    path_a()  # warm-up: code objects, scratch growth
    path_b()
    assert np.array_equal(dst_a.download(wire_len), dst_b.download(wire_len)), "the two paths differ"
    a, b, bc, bi = [], [], [], []
    for _ in range(reps):  # alternate the two paths
        a.append(path_a())
        t, tc, ti = path_b()
        b.append(t)
        bc.append(tc)
        bi.append(ti)
    loop = _median([empty_loop() for _ in range(3)])
    hdr.free()
    ms = lambda x: round(x * 1e3, 3)  # noqa: E731
    return {"write_mib": n / MIB, "offset_in_block": off, "packets": cap_n, "wire_len": wire_len,
            "wire_ms": ms(_median(a)), "wire_min_ms": ms(min(a)), "wire_max_ms": ms(max(a)),
            "copies_ms": ms(_median(b)), "copies_min_ms": ms(min(b)), "copies_max_ms": ms(max(b)),
            "copies_compose_ms": ms(_median(bc)), "copies_issue_ms": ms(_median(bi)), "loop_ms": ms(loop),
            "wire_GiBps": round(n / _median(a) / (1 << 30), 1), "copies_GiBps": round(n / _median(b) / (1 << 30), 1)}


def measure_kernel(src, dst, n, off, iters):
    info = wire.layout(n, off, *ARGS)
    traffic = n + 4 * info["nchunks"] + info["wire_len"]
    rows = []
    for slices in (1, 2, 4, 8):
        for sc1 in (0, 1):
            flags = wire.time_slices(slices) | (wire.TIME_SC1 if sc1 else 0)
            t = _median([wire.frame_time(src.ptr + 1, n, dst.ptr, info["wire_len"], off, *ARGS, flags, iters)
                         for _ in range(3)])
            rows.append({"write_mib": n / MIB, "slices": slices, "sc1": sc1, "kernel_ms": round(t, 4),
                         "traffic_TBps": round(traffic / (t * 1e-3) / 1e12, 2)})
    t = _median([wire.frame_time(src.ptr + 1, n, dst.ptr, info["wire_len"], off, *ARGS, 0, iters) for _ in range(3)])
    rows.append({"write_mib": n / MIB, "slices": "product", "sc1": "product", "kernel_ms": round(t, 4),
                 "traffic_TBps": round(traffic / (t * 1e-3) / 1e12, 2)})
    return rows


def measure(reps=5, quick=False):
    lib, wlib = h.load(), wire.load()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.restype = ctypes.c_int
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    arch, ncu = h.device_info()
    big = (128 if quick else 1024) * MIB
    room = wire.layout(big, 4321, *ARGS)["wire_len"] + 64
    src = h.DeviceBuffer(big + 4096)
    dst_a, dst_b = h.DeviceBuffer(room), h.DeviceBuffer(room)
    hdr_dev = h.DeviceBuffer(room - big)
    h.fill_splitmix64(src.ptr, (big + 4096) // 8, 13, 0)
    h.device_sync()
    sizes = [128 * MIB] + ([] if quick else [1024 * MIB])
    rows, kernel = [], []
    try:
        for n in sizes:
            for off in (0, 4321):
                rows.append(measure_write(hip, lib, wlib, src, dst_a, dst_b, hdr_dev, n, off, reps))
        for n in [MIB, 8 * MIB] + sizes:  # the small ones: how many workgroups per packet a short write wants
            kernel += measure_kernel(src, dst_a, n, 4321, 10)
    finally:
        for b in (src, dst_a, dst_b, hdr_dev):
            b.free()
    return {"arch": arch, "num_cu": ncu, "reps": reps, "rows": rows, "kernel": kernel,
            "copies_faster_at": [(r["write_mib"], r["offset_in_block"]) for r in rows
                                 if r["copies_ms"] <= r["wire_ms"]]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="128 MiB writes only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reps, a.quick)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
