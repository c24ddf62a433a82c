"""Gather writes: hdfs_writev_compose_packets on a write held in F device
fragments against the packed alternative built from what the main library
already offers, for DESIGN.md section 12 and the comment of
include/hadoofus_writev.h.

For each shape, in one process:
  in place: hdfs_writev_compose_packets over the fragments (host clock around
            the call, which ends in a stream synchronise; output buffers
            allocated before the clock starts);
  packed:   one hipMemcpyAsync device-to-device per fragment into a contiguous
            device buffer of the write's size (allocated before the clock
            starts), then hdfs_crc32c_compose_packets on it.
Both give the same header bytes and packet records (asserted).  The copies of
the packed path are issued from a Python loop; `loop_ms` is the same loop
calling a function that does nothing, so the interpreter's share can be
subtracted.  Shapes: 128 MiB in 1, 16 and 1 024 equal odd-sized fragments,
128 MiB of 4 000-byte fragments (every chunk gathered), 1 GiB in 64 fragments,
and a sweep of fragment sizes over 128 MiB that locates the fragment size
below which packing is the faster path.  Fragments start at odd addresses.
GPU box only.

    python tools/writev_bench.py [--reps 5] [--quick] [--out file.json]
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
from hadoofus_amd import writev  # noqa: E402
from hadoofus_amd.abi import OutPacket  # noqa: E402

MIB = 1 << 20
D2D = 3  # hipMemcpyDeviceToDevice


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def equal_odd(total, nfrag):
    """nfrag fragments of one odd size, the last one taking the rest."""
    if nfrag == 1:
        return [total]
    n = (total // nfrag) | 1
    lens = [n] * (nfrag - 1)
    return lens + [total - sum(lens)]


def of_size(total, size):
    lens = [size] * (total // size)
    return lens + ([total - sum(lens)] if total % size else [])


def measure_shape(hip, lib, wlib, arena, packed, total, lens, reps):
    """arena: device buffer of the fragments, one after the other from byte 1
    (odd-sized fragments then start at odd and even addresses alike)."""
    n = len(lens)
    offs = np.concatenate(([0], np.cumsum(lens[:-1]))).astype(np.int64) + 1
    vec = (h.IoVec * n)(*[h.IoVec(arena.ptr + int(o), int(l)) for o, l in zip(offs, lens)])
    srcs = [arena.ptr + int(o) for o in offs]
    dsts = [packed.ptr + int(o) - 1 for o in offs]
    npk, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    args = (4321, 0, h.PROTO_V2, h.CSUM_CRC32C, 1)
    assert wlib.hdfs_writev_compose_packets(vec, n, *args, None, 0, None, 0, ctypes.byref(npk), ctypes.byref(used)) == 0
    cap_n, cap_b = npk.value, used.value
    hdr = [np.zeros(cap_b, dtype=np.uint8) for _ in range(2)]
    pk = [(OutPacket * cap_n)() for _ in range(2)]

    def in_place():
        t0 = time.perf_counter()
        rc = wlib.hdfs_writev_compose_packets(vec, n, *args, hdr[0].ctypes.data, cap_b, pk[0], cap_n, ctypes.byref(npk),
                                              ctypes.byref(used))
        t = time.perf_counter() - t0
        assert rc == 0, wlib.hdfs_writev_last_error()
        return t

    def pack_and_compose():
        t0 = time.perf_counter()
        for s, d, l in zip(srcs, dsts, lens):
            hip.hipMemcpyAsync(d, s, l, D2D, None)
        t1 = time.perf_counter()
        rc = lib.hdfs_crc32c_compose_packets(packed.ptr, total, *args, hdr[1].ctypes.data, cap_b, pk[1], cap_n,
                                             ctypes.byref(npk), ctypes.byref(used))
        t2 = time.perf_counter()
        assert rc == 0, lib.hdfs_crc32c_last_error()
        return t2 - t0, t1 - t0

    def empty_loop():
        t0 = time.perf_counter()
        for s, d, l in zip(srcs, dsts, lens):
            lib.hdfs_crc32c_abi_version()
        return time.perf_counter() - t0

    in_place()  # warm-up: code objects, scratch growth
    pack_and_compose()
    assert np.array_equal(hdr[0], hdr[1]) and bytes(pk[0]) == bytes(pk[1])
    a, b, c = [], [], []
    for _ in range(reps):  # alternate the two paths
        a.append(in_place())
        t, ti = pack_and_compose()
        b.append(t)
        c.append(ti)
    loop = _median([empty_loop() for _ in range(3)])
    info = writev.layout(lens, args[0])
    ms = lambda x: round(x * 1e3, 3)  # noqa: E731
    return {"total_mib": total / MIB, "fragments": n, "fragment_bytes": lens[0], "nsegments": info["nsegments"],
            "ngathered": info["ngathered"], "nchunks": info["nchunks"], "in_place_ms": ms(_median(a)),
            "in_place_min_ms": ms(min(a)), "in_place_max_ms": ms(max(a)), "packed_ms": ms(_median(b)),
            "packed_min_ms": ms(min(b)), "packed_max_ms": ms(max(b)), "packed_copy_issue_ms": ms(_median(c)),
            "loop_ms": ms(loop), "in_place_GiBps": round(total / _median(a) / (1 << 30), 1),
            "packed_GiBps": round(total / _median(b) / (1 << 30), 1)}


def measure(reps=5, quick=False):
    lib, wlib = h.load(), writev.load()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    arch, ncu = h.device_info()
    big = (128 if quick else 1024) * MIB
    arena = h.DeviceBuffer(big + 4096)
    packed = h.DeviceBuffer(big)
    h.fill_splitmix64(arena.ptr, (big + 4096) // 8, 12, 0)
    h.device_sync()
    t128 = 128 * MIB
    shapes = [("128MiB_x1", t128, equal_odd(t128, 1)), ("128MiB_x16", t128, equal_odd(t128, 16)),
              ("128MiB_x1024", t128, equal_odd(t128, 1024)), ("128MiB_of_4000B", t128, of_size(t128, 4000))]
    if not quick:
        shapes.append(("1GiB_x64", 1024 * MIB, equal_odd(1024 * MIB, 64)))
    sweep_sizes = [4097, 8193, 16385, 32769, 65537, 262145, 1048577]
    rows, sweep = [], []
    try:
        for name, total, lens in shapes:
            rows.append(dict(shape=name, **measure_shape(hip, lib, wlib, arena, packed, total, lens, reps)))
        for size in sweep_sizes:
            sweep.append(dict(shape=f"128MiB_of_{size}B",
                              **measure_shape(hip, lib, wlib, arena, packed, t128, of_size(t128, size), reps)))
    finally:
        arena.free()
        packed.free()
    # the smallest swept fragment size from which the in-place path stays the faster one
    allrows = sorted([r for r in rows + sweep if r["total_mib"] == 128 and r["fragments"] > 1],
                     key=lambda r: r["fragment_bytes"])
    cross = None
    for r in allrows:
        if all(q["in_place_ms"] < q["packed_ms"] for q in allrows if q["fragment_bytes"] >= r["fragment_bytes"]):
            cross = r["fragment_bytes"]
            break
    return {"arch": arch, "num_cu": ncu, "reps": reps, "rows": rows, "sweep": sweep,
            "in_place_faster_from_fragment_bytes": cross,
            "packing_faster_at_fragment_bytes": [r["fragment_bytes"] for r in allrows
                                                 if r["in_place_ms"] >= r["packed_ms"]]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="128 MiB shapes only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reps, a.quick)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
