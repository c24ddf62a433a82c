"""A write held in device fragments as one wire stream in device memory:
hdfs_wirev_compose_packets against packing the fragments and
hdfs_wire_compose_packets, for DESIGN.md section 15 and the comment of
include/hadoofus_wirev.h.

For each shape (128 MiB in 1, 16, 128, 1 024, 16 383 and 33 555 fragments,
1 GiB in 64; block offsets 0 and 4321; CRC32C, v2, finish; every fragment at
an odd address), in one process:
  A, in place: hdfs_wirev_compose_packets on the fragments;
  B, packed:   one hipMemcpyAsync device-to-device per fragment into a
               contiguous buffer allocated beforehand, then
               hdfs_wire_compose_packets on it.
Host clock around each whole path, which ends in a stream synchronise; all
buffers and the iovec array exist beforehand.  Both give the same bytes
(asserted, both streams downloaded once per shape).  Medians of --reps with
the two paths alternated after one warm-up of each.  `issue_ms` is the part of
B spent issuing the copies; `loop_ms` is the same loop calling a function that
does nothing, the interpreter's share.

For the one-fragment shapes also hdfs_wire_compose_packets on the fragment
itself (`contiguous_ms`): what the fragment table, the gather layout and the
gathered first chunk cost a write that needs none of them.  And for every
shape the frame kernel alone (hdfs_wirev_frame_time: HIP events around
back-to-back launches).  Traffic per launch: reads len + 4 B per chunk,
writes the stream.  GPU box only.

    python tools/wirev_bench.py [--reps 5] [--quick] [--out file.json]
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
from hadoofus_amd import wire, wirev  # noqa: E402
from hadoofus_amd.abi import IoVec, OutPacket  # noqa: E402

MIB = 1 << 20
D2D = 3  # hipMemcpyDeviceToDevice
ARGS = (h.PROTO_V2, h.CSUM_CRC32C, 1)  # proto, ctype, finish
GAP = 3  # bytes between two fragments in the source buffer: neighbours are not contiguous, residues differ


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def shapes(quick):
    n = 128 * MIB
    out = [(n, [n]), (n, [n // 16] * 16), (n, [n // 128] * 128), (n, [n // 1024] * 1024)]
    for frag in (8193, 4000):
        k = n // frag
        out.append((n, [frag] * k + ([n - k * frag] if n - k * frag else [])))
    if not quick:
        out.append((1024 * MIB, [16 * MIB] * 64))
    return out


def measure_shape(hip, wlib, vlib, src, packed, dst_a, dst_b, n, lens, off, reps, iters):
    assert sum(lens) == n
    nf = len(lens)
    vec = (IoVec * nf)()
    at = src.ptr + 1
    for i, ln in enumerate(lens):
        vec[i].base, vec[i].len = at, ln
        at += ln + GAP + (ln + GAP) % 2  # an even step: the next one at an odd address too
    assert at <= src.ptr + src.nbytes
    ptrs = [(vec[i].base, vec[i].len) for i in range(nf)]
    info = wirev.layout(lens, off, *ARGS)
    wire_len, cap_n = info["wire_len"], info["npkts"]
    pk_a, pk_b = (OutPacket * cap_n)(), (OutPacket * cap_n)()
    npk, wl = ctypes.c_size_t(0), ctypes.c_uint64(0)
    pp = packed.ptr + 1

    def path_a():
        t0 = time.perf_counter()
        rc = vlib.hdfs_wirev_compose_packets(vec, nf, off, 0, *ARGS, dst_a.ptr, wire_len, pk_a, cap_n,
                                             ctypes.byref(npk), ctypes.byref(wl), None)
        t = time.perf_counter() - t0
        assert rc == 0, vlib.hdfs_wirev_last_error()
        return t

    def path_b():
        t0 = time.perf_counter()
        to = pp
        for p, ln in ptrs:
            hip.hipMemcpyAsync(to, p, ln, D2D, None)
            to += ln
        t1 = time.perf_counter()
        rc = wlib.hdfs_wire_compose_packets(pp, n, off, 0, *ARGS, dst_b.ptr, wire_len, pk_b, cap_n, ctypes.byref(npk),
                                            ctypes.byref(wl), None)
        t2 = time.perf_counter()
        assert rc == 0 and to - pp == n, wlib.hdfs_wire_last_error()
        return t2 - t0, t1 - t0

    def contiguous():
        t0 = time.perf_counter()
        rc = wlib.hdfs_wire_compose_packets(ptrs[0][0], n, off, 0, *ARGS, dst_b.ptr, wire_len, pk_b, cap_n,
                                            ctypes.byref(npk), ctypes.byref(wl), None)
        t = time.perf_counter() - t0
        assert rc == 0, wlib.hdfs_wire_last_error()
        return t

    def empty_loop():
        t0 = time.perf_counter()
        to = pp
        for p, ln in ptrs:
            wlib.hdfs_wire_abi_version()
            to += ln
        return time.perf_counter() - t0

    path_a()  # warm-up: code objects, scratch growth
    path_b()
    assert np.array_equal(dst_a.download(wire_len), dst_b.download(wire_len)), "the two paths differ"
    assert bytes(pk_a) == bytes(pk_b), "the two paths' records differ"
    a, b, bi, c = [], [], [], []
    for _ in range(reps):  # alternate the paths
        a.append(path_a())
        t, ti = path_b()
        b.append(t)
        bi.append(ti)
        if nf == 1:
            c.append(contiguous())
    loop = _median([empty_loop() for _ in range(3)])
    kt = _median([wirev.frame_time(ptrs, dst_a.ptr, wire_len, off, *ARGS, 0, iters) for _ in range(3)])
    traffic = n + 4 * info["nchunks"] + wire_len
    ms = lambda x: round(x * 1e3, 3)  # noqa: E731
    row = {"write_mib": n / MIB, "fragments": nf, "fragment_bytes": lens[0], "offset_in_block": off,
           "packets": cap_n, "nsegments": info["nsegments"], "ngathered": info["ngathered"],
           "max_frags_per_packet": info["max_frags_per_packet"],
           "in_place_ms": ms(_median(a)), "in_place_min_ms": ms(min(a)), "in_place_max_ms": ms(max(a)),
           "packed_ms": ms(_median(b)), "packed_min_ms": ms(min(b)), "packed_max_ms": ms(max(b)),
           "issue_ms": ms(_median(bi)), "loop_ms": ms(loop),
           "in_place_GiBps": round(n / _median(a) / (1 << 30), 1), "packed_GiBps": round(n / _median(b) / (1 << 30), 1),
           "kernel_ms": round(kt, 4), "traffic_TBps": round(traffic / (kt * 1e-3) / 1e12, 2)}
    if c:
        row.update(contiguous_ms=ms(_median(c)), contiguous_min_ms=ms(min(c)), contiguous_max_ms=ms(max(c)))
    return row


def measure(reps=5, quick=False):
    h.load()
    wlib, vlib = wire.load(), wirev.load()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    arch, ncu = h.device_info()
    todo = shapes(quick)
    big = max(n for n, _ in todo)
    most = max(len(lens) for _, lens in todo)
    room = wire.layout(big, 4321, *ARGS)["wire_len"] + 64
    src_bytes = (big + most * (GAP + 1) + 4096 + 7) // 8 * 8
    src, packed = h.DeviceBuffer(src_bytes), h.DeviceBuffer(big + 4096)
    dst_a, dst_b = h.DeviceBuffer(room), h.DeviceBuffer(room)
    h.fill_splitmix64(src.ptr, src_bytes // 8, 14, 0)
    h.device_sync()
    rows = []
    try:
        for n, lens in todo:
            for off in (0, 4321):
                rows.append(measure_shape(hip, wlib, vlib, src, packed, dst_a, dst_b, n, lens, off, reps, 10))
    finally:
        for b in (src, packed, dst_a, dst_b):
            b.free()
    return {"arch": arch, "num_cu": ncu, "reps": reps, "rows": rows,
            "packed_faster_at": [(r["write_mib"], r["fragments"], r["offset_in_block"]) for r in rows
                                 if r["packed_ms"] <= r["in_place_ms"]]}


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
