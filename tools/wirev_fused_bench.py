"""A write held in device fragments as one wire stream in device memory, in one
pass: hdfs_wirev_fused_compose_packets against hdfs_wirev_compose_packets (the
two-pass gather it replaces) on the same fragments, for DESIGN.md section 18
and the comment of include/hadoofus_wirev_fused.h.

Shapes: section 15's eight (128 MiB in 1 fragment at block offsets 0 and 4321,
in 16, 128, 1 024, 16 383 and 33 555 fragments at 4321, 1 GiB in 64) and 1 MiB
and 8 MiB writes in 1 and 16 fragments at 4321; CRC32C, v2, finish; every
fragment at an odd address.  For each, in one process:
  A, fused:    hdfs_wirev_fused_compose_packets on the fragments;
  B, two-pass: hdfs_wirev_compose_packets on the same fragments;
  C (one fragment only): hdfs_wire_fused_compose_packets on the same bytes --
               what the fragment table and the lookup cost a write that needs
               neither.
Host clock around each whole call, which ends in a stream synchronise; all
buffers and the iovec array exist beforehand.  All give the same bytes
(asserted, the streams downloaded once per shape).  Medians of --reps (with
min and max) with the paths alternated, in the order A, B, C, after one warm-up
of each; then the same medians of each call alone, back to back (`*_alone_ms`):
a call that follows another library's call can pay for what that one left
behind, and the two orders tell the two costs apart.  And for
every shape the kernels alone (hdfs_wirev_fused_time, hdfs_wirev_frame_time
and, with one fragment, hdfs_wire_fused_time: HIP events around back-to-back
launches); the two-pass figure is its frame kernel only, the CRC pass ahead of
it is not in it.  GPU box only.

    python tools/wirev_fused_bench.py [--reps 5] [--quick] [--out file.json]
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
from hadoofus_amd import wire_fused, wirev, wirev_fused  # noqa: E402
from hadoofus_amd.abi import IoVec, OutPacket  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, h.CSUM_CRC32C, 1)  # proto, ctype, finish
GAP = 3  # bytes between two fragments in the source buffer: neighbours are not contiguous, residues differ


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def shapes(quick):
    """(write bytes, fragment lengths, block offset)."""
    n = 128 * MIB
    out = [(n, [n], 0), (n, [n], 4321), (n, [n // 16] * 16, 4321), (n, [n // 128] * 128, 4321),
           (n, [n // 1024] * 1024, 4321)]
    for frag in (8193, 4000):
        k = n // frag
        out.append((n, [frag] * k + ([n - k * frag] if n - k * frag else []), 4321))
    if not quick:
        out.append((1024 * MIB, [16 * MIB] * 64, 4321))
    for m in (MIB, 8 * MIB):
        out += [(m, [m], 4321), (m, [m // 16] * 16, 4321)]
    return out


def measure_shape(libs, src, dst_a, dst_b, n, lens, off, reps, iters):
    flib, vlib, clib = libs
    assert sum(lens) == n
    nf = len(lens)
    vec = (IoVec * nf)()
    at = src.ptr + 1
    for i, ln in enumerate(lens):
        vec[i].base, vec[i].len = at, ln
        at += ln + GAP + (ln + GAP) % 2  # an even step: the next one at an odd address too
    assert at <= src.ptr + src.nbytes
    ptrs = [(vec[i].base, vec[i].len) for i in range(nf)]
    info = wirev_fused.layout(lens, off, *ARGS)
    wire_len, cap_n = info["wire_len"], info["npkts"]
    pk_a, pk_b = (OutPacket * cap_n)(), (OutPacket * cap_n)()
    npk, wl = ctypes.c_size_t(0), ctypes.c_uint64(0)

    def path_a():
        t0 = time.perf_counter()
        rc = flib.hdfs_wirev_fused_compose_packets(vec, nf, off, 0, *ARGS, dst_a.ptr, wire_len, pk_a, cap_n,
                                                   ctypes.byref(npk), ctypes.byref(wl), None)
        t = time.perf_counter() - t0
        assert rc == 0, flib.hdfs_wirev_fused_last_error()
        return t

    def path_b():
        t0 = time.perf_counter()
        rc = vlib.hdfs_wirev_compose_packets(vec, nf, off, 0, *ARGS, dst_b.ptr, wire_len, pk_b, cap_n,
                                             ctypes.byref(npk), ctypes.byref(wl), None)
        t = time.perf_counter() - t0
        assert rc == 0, vlib.hdfs_wirev_last_error()
        return t

    def path_c():
        t0 = time.perf_counter()
        rc = clib.hdfs_wire_fused_compose_packets(ptrs[0][0], n, off, 0, *ARGS, dst_b.ptr, wire_len, pk_b, cap_n,
                                                  ctypes.byref(npk), ctypes.byref(wl), None)
        t = time.perf_counter() - t0
        assert rc == 0, clib.hdfs_wire_fused_last_error()
        return t

    path_a()  # code objects, scratch growth; the streams compared
    path_b()
    want = dst_a.download(wire_len)
    assert np.array_equal(want, dst_b.download(wire_len)), "the fused and the two-pass streams differ"
    assert bytes(pk_a) == bytes(pk_b), "the two paths' records differ"
    if nf == 1:
        path_c()
        assert np.array_equal(want, dst_b.download(wire_len)), "the gather and the single-write fused streams differ"
    path_a()  # the warm-up of each, behind the downloads
    path_b()
    if nf == 1:
        path_c()
    a, b, c = [], [], []
    for _ in range(reps):  # alternate the paths
        a.append(path_a())
        b.append(path_b())
        if nf == 1:
            c.append(path_c())

    def alone(path):  # the same call back to back: what it costs when nothing else ran just before it
        path()
        return [path() for _ in range(reps)]
    a2, b2, c2 = alone(path_a), alone(path_b), alone(path_c) if nf == 1 else []
    ka = _median([wirev_fused.fused_time(ptrs, dst_a.ptr, wire_len, off, *ARGS, 0, iters) for _ in range(3)])
    kb = _median([wirev.frame_time(ptrs, dst_b.ptr, wire_len, off, *ARGS, 0, iters) for _ in range(3)])
    ms = lambda x: round(x * 1e3, 3)  # noqa: E731
    row = {"write_mib": n / MIB, "fragments": nf, "fragment_bytes": lens[0], "offset_in_block": off,
           "packets": cap_n, "rounds": info["rounds"], "seamed_rounds": info["seamed_rounds"],
           "max_frags_per_round": info["max_frags_per_round"],
           "fused_ms": ms(_median(a)), "fused_min_ms": ms(min(a)), "fused_max_ms": ms(max(a)),
           "two_pass_ms": ms(_median(b)), "two_pass_min_ms": ms(min(b)), "two_pass_max_ms": ms(max(b)),
           "fused_alone_ms": ms(_median(a2)), "fused_alone_min_ms": ms(min(a2)), "fused_alone_max_ms": ms(max(a2)),
           "two_pass_alone_ms": ms(_median(b2)), "two_pass_alone_min_ms": ms(min(b2)),
           "two_pass_alone_max_ms": ms(max(b2)),
           "fused_kernel_ms": round(ka, 4), "two_pass_frame_kernel_ms": round(kb, 4),
           "fused_kernel_traffic_TBps": round((n + wire_len) / (ka * 1e-3) / 1e12, 2)}
    if c:
        kc = _median([wire_fused.fused_time(ptrs[0][0], n, dst_b.ptr, wire_len, off, *ARGS, 0, iters)
                      for _ in range(3)])
        row.update(single_fused_ms=ms(_median(c)), single_fused_min_ms=ms(min(c)), single_fused_max_ms=ms(max(c)),
                   single_fused_alone_ms=ms(_median(c2)), single_fused_alone_min_ms=ms(min(c2)),
                   single_fused_alone_max_ms=ms(max(c2)), single_fused_kernel_ms=round(kc, 4))
    return row


def measure(reps=5, quick=False):
    h.load()
    libs = (wirev_fused.load(), wirev.load(), wire_fused.load())
    arch, ncu = h.device_info()
    todo = shapes(quick)
    big = max(n for n, _, _ in todo)
    most = max(len(lens) for _, lens, _ in todo)
    room = wirev_fused.layout([big], 4321, *ARGS)["wire_len"] + 64
    src_bytes = (big + most * (GAP + 1) + 4096 + 7) // 8 * 8
    src, dst_a, dst_b = h.DeviceBuffer(src_bytes), h.DeviceBuffer(room), h.DeviceBuffer(room)
    h.fill_splitmix64(src.ptr, src_bytes // 8, 14, 0)
    h.device_sync()
    rows = []
    try:
        for n, lens, off in todo:
            rows.append(measure_shape(libs, src, dst_a, dst_b, n, lens, off, reps, 10))
    finally:
        for b in (src, dst_a, dst_b):
            b.free()
    return {"arch": arch, "num_cu": ncu, "reps": reps, "rows": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="no 1 GiB write")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reps, a.quick)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
