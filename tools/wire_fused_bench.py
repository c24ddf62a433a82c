"""A write's wire stream in one pass (hdfs_wire_fused_compose_packets) against
the two-pass call it mirrors (hdfs_wire_compose_packets), for DESIGN.md section
16 and the comment of include/hadoofus_wire_fused.h.

For each write (1 MiB, 8 MiB, 128 MiB and 1 GiB, at block offsets 0 and 4321,
CRC32C, v2, finish, source at an odd address), in one process:
  fused:     hdfs_wire_fused_compose_packets;
  two-pass:  hdfs_wire_compose_packets (a compute plan, then the frame kernel);
host clock around each whole call, which ends in its stream synchronise; all
buffers allocated beforehand; one warm-up of each, then the two alternated;
medians of --reps with min and max.  Both streams are downloaded and compared
in every case.

Beside the whole calls, from HIP events around back-to-back launches:
  fused_kernel_ms:  the fused kernel alone (hdfs_wire_fused_time);
  frame_kernel_ms:  the two-pass library's frame kernel alone
                    (hdfs_wire_frame_time, the CRC array filled);
  plan_ms:          a compute plan over the same chunk grid alone, created
                    beforehand, events around its executes.
Traffic of the fused kernel: len read plus the stream written.
GPU box only.

    python tools/wire_fused_bench.py [--reps 5] [--quick] [--out file.json]
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
from hadoofus_amd import wire, wire_fused  # noqa: E402
from hadoofus_amd.abi import OutPacket  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, h.CSUM_CRC32C, 1)  # proto, ctype, finish
ITERS = 10


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p
    for name, args in (("hipEventCreate", [ctypes.POINTER(vp)]), ("hipEventRecord", [vp, vp]),
                       ("hipEventSynchronize", [vp]), ("hipEventDestroy", [vp]),
                       ("hipEventElapsedTime", [ctypes.POINTER(ctypes.c_float), vp, vp])):
        f = getattr(hip, name)
        f.restype, f.argtypes = ctypes.c_int, args
    return hip


def plan_ms(hip, sp, n, off, crcs, stream):
    """A compute plan over the write's chunk grid (the short first chunk, then
    the 512-B grid), created beforehand; events around ITERS executes."""
    n0 = min(n, 512 - off % 512) if off % 512 else 0
    segs = []
    if n0:
        segs.append(h.Segment(data=sp, len=n0, chunk_size=512, flags=h.SEG_BE, crc_init=0, crcs=crcs.ptr, bitmap=None))
    if n > n0:
        segs.append(h.Segment(data=sp + n0, len=n - n0, chunk_size=512, flags=h.SEG_BE, crc_init=0,
                              crcs=crcs.ptr + (4 if n0 else 0), bitmap=None))
    plan = h.Plan(h.MODE_COMPUTE, segs)
    plan.execute(stream)
    h.stream_sync(stream)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    out = []
    for _ in range(3):
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(ITERS):
            plan.execute(stream)
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = ctypes.c_float(0)
        assert hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1) == 0
        out.append(ms.value / ITERS)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return _median(out)


def measure_write(hip, src, dst_f, dst_t, crcs, stream, n, off, reps):
    wlib, flib = wire.load(), wire_fused.load()
    npk, wl = ctypes.c_size_t(0), ctypes.c_uint64(0)
    assert flib.hdfs_wire_fused_compose_packets(None, n, off, 0, *ARGS, None, 0, None, 0, ctypes.byref(npk),
                                                ctypes.byref(wl), None) == 0
    cap_n, wire_len = npk.value, wl.value
    pk_f, pk_t = (OutPacket * cap_n)(), (OutPacket * cap_n)()
    sp = src.ptr + 1  # an odd source address

    def fused():
        t0 = time.perf_counter()
        rc = flib.hdfs_wire_fused_compose_packets(sp, n, off, 0, *ARGS, dst_f.ptr, wire_len, pk_f, cap_n,
                                                  ctypes.byref(npk), ctypes.byref(wl), None)
        t = time.perf_counter() - t0
        assert rc == 0, flib.hdfs_wire_fused_last_error()
        return t

    def two_pass():
        t0 = time.perf_counter()
        rc = wlib.hdfs_wire_compose_packets(sp, n, off, 0, *ARGS, dst_t.ptr, wire_len, pk_t, cap_n, ctypes.byref(npk),
                                            ctypes.byref(wl), None)
        t = time.perf_counter() - t0
        assert rc == 0, wlib.hdfs_wire_last_error()
        return t

    fused()  # warm-up: code objects, tables, scratch growth
    two_pass()
    f, t = [], []
    for _ in range(reps):  # alternate the two calls
        f.append(fused())
        t.append(two_pass())
    assert np.array_equal(dst_f.download(wire_len), dst_t.download(wire_len)), "the two streams differ"
    assert bytes(pk_f) == bytes(pk_t), "the two calls' records differ"
    fk = _median([wire_fused.fused_time(sp, n, dst_f.ptr, wire_len, off, *ARGS, 0, ITERS) for _ in range(3)])
    tk = _median([wire.frame_time(sp, n, dst_t.ptr, wire_len, off, *ARGS, 0, ITERS) for _ in range(3)])
    pm = plan_ms(hip, sp, n, off, crcs, stream)
    assert np.array_equal(dst_f.download(wire_len), dst_t.download(wire_len)), "the two streams differ after timing"
    ms = lambda x: round(x * 1e3, 3)  # noqa: E731
    clear = max(f) < min(t)
    return {"write_mib": n / MIB, "offset_in_block": off, "packets": cap_n, "wire_len": wire_len,
            "fused_ms": ms(_median(f)), "fused_min_ms": ms(min(f)), "fused_max_ms": ms(max(f)),
            "two_pass_ms": ms(_median(t)), "two_pass_min_ms": ms(min(t)), "two_pass_max_ms": ms(max(t)),
            "verdict": "fused faster" if clear else ("two-pass faster" if max(t) < min(f) else "ranges overlap"),
            "fused_kernel_ms": round(fk, 4), "frame_kernel_ms": round(tk, 4), "plan_ms": round(pm, 4),
            "fused_traffic_TBps": round((n + wire_len) / (fk * 1e-3) / 1e12, 2)}


def measure(reps=5, quick=False):
    h.load()
    hip = _hip()
    arch, ncu = h.device_info()
    sizes = [MIB, 8 * MIB, 128 * MIB] + ([] if quick else [1024 * MIB])
    big = sizes[-1]
    room = wire.layout(big, 4321, *ARGS)["wire_len"] + 64
    src = h.DeviceBuffer(big + 4096)
    dst_f, dst_t = h.DeviceBuffer(room), h.DeviceBuffer(room)
    crcs = h.DeviceBuffer(4 * (big // 512 + 2))
    h.fill_splitmix64(src.ptr, (big + 4096) // 8, 13, 0)
    h.device_sync()
    stream = h.stream_create()
    rows = []
    try:
        for n in sizes:
            for off in (0, 4321):
                rows.append(measure_write(hip, src, dst_f, dst_t, crcs, stream, n, off, reps))
    finally:
        h.load().hdfs_crc32c_stream_destroy(stream)
        for b in (src, dst_f, dst_t, crcs):
            b.free()
    return {"arch": arch, "num_cu": ncu, "reps": reps, "iters": ITERS, "rows": rows}


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
