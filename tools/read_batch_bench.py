"""A batch of block reads in one call: hdfs_read_batch_read_blocks against the
ways of doing the job without it, for DESIGN.md section 20 and the comment of
include/hadoofus_read_batch.h.

For each shape (a list of block sizes; v2, CRC32C; every block's packet stream
composed on the device beforehand by the fused batch write library, with the
empty last packet, at odd addresses; all buffers allocated beforehand), in one
process:
  A, batch:  hdfs_read_batch_read_blocks, one call for all blocks, records kept;
  B, loop:   hdfs_crc32c_read_packets (device stream to device buffer,
             READ_ALL), one call per block: the main library as it stands;
  C, verify: hdfs_crc32c_verify_blocks_submit / job_wait_blocks in jobs of 16,
             which delivers no byte: a floor for the verify part only.
The host clock runs around each whole path (each ends synchronised).  A and B
deliver the same bytes and the same records (asserted once per shape).
Medians of --reps with the three paths alternated after one warm-up of each,
with the min-max spread, per block.  `verdict` is "faster" only where A's
whole range lies below B's, "slower" where it lies above, else "overlaps".
Beside it the two launches alone, from the timing entry (HIP events around
back-to-back probe + main launches), and how many entries took each path.
The last shape corrupts one block of 64: it prices one fallback.
GPU box only.

    python tools/read_batch_bench.py [--reps 5] [--quick] [--shapes small|large|all] [--out file.json]
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
from hadoofus_read import read_batch  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, 512, h.CSUM_CRC32C)
# (name, block sizes, index of a block to corrupt or None)
LARGE = [("16 x 128 MiB", [128 * MIB] * 16, None), ("64 x 128 MiB", [128 * MIB] * 64, None),
         ("15 x 128 MiB + 5 MiB", [128 * MIB] * 15 + [5 * MIB], None),
         ("64 x 128 MiB, one corrupt", [128 * MIB] * 64, 37)]
SMALL = [("64 x 1 MiB", [MIB] * 64, None), ("256 x 64 KiB", [65536] * 256, None)]


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _stats(xs, n):
    us = lambda x: round(x * 1e6 / n, 3)  # noqa: E731  (per block)
    return {"us": us(_median(xs)), "min_us": us(min(xs)), "max_us": us(max(xs))}


def measure_shape(name, sizes, corrupt, src, wires, dsts, reps, iters):
    rlib, lib = read_batch.load(), h.load()
    nb = len(sizes)
    writes = [wire_fused_batch.write(nbytes=n, finish=True) for n in sizes]
    outs, _ = wire_fused_batch.layout(writes, ARGS[0], ARGS[2])
    wl, npk = [o["wire_len"] for o in outs], [o["npkts"] for o in outs]
    at_w, at_d, a, b = [], [], 5, 3
    for k in range(nb):
        at_w.append(a)
        at_d.append(b)
        a += (wl[k] + 64) // 16 * 16 + 1
        b += (sizes[k] + 64) // 16 * 16 + 2
    assert a <= wires.nbytes and b <= dsts[0].nbytes
    wire_fused_batch.compose([wire_fused_batch.write(src.ptr + 1, sizes[k], wires.ptr + at_w[k], wl[k], 0, 0, True)
                              for k in range(nb)], ARGS[0], ARGS[2])
    if corrupt is not None:  # one data bit in the middle of that block's stream
        at = at_w[corrupt] + wl[corrupt] // 2 + 4096  # inside a packet's data
        byte = wires.download(1, at)
        wires.upload(byte ^ np.uint8(0x10), at)
    mp = max(npk)
    ent = read_batch.entries([read_batch.entry(wires.ptr + at_w[k], wl[k], dsts[0].ptr + at_d[k], sizes[k])
                              for k in range(nb)])
    pk_a, pk_b = (Packet * (mp * nb))(), (Packet * (mp * nb))()
    cnt, used, got = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    want_rc = 0 if corrupt is None else h.ERR_BAD_CHECKSUM
    out_b = [None] * nb
    rec_b = [ctypes.cast(ctypes.addressof(pk_b) + k * mp * ctypes.sizeof(Packet), ctypes.POINTER(Packet))
             for k in range(nb)]

    def path_a():
        t0 = time.perf_counter()
        rc = rlib.hdfs_read_batch_read_blocks(ent, nb, *ARGS, pk_a, mp, None)
        t = time.perf_counter() - t0
        assert rc == want_rc, (rc, rlib.hdfs_read_batch_last_error())
        return t

    def path_b():
        t0 = time.perf_counter()
        for k in range(nb):
            iov = IoVec(dsts[1].ptr + at_d[k], sizes[k])
            rc = lib.hdfs_crc32c_read_packets(wires.ptr + at_w[k], wl[k], *ARGS, 0, h.READ_ALL, ctypes.byref(iov), 1,
                                              rec_b[k], mp, ctypes.byref(cnt), ctypes.byref(used), ctypes.byref(got))
            assert rc == (want_rc if k == corrupt else 0), (k, rc)
            out_b[k] = (rc, cnt.value, used.value, got.value)
        return time.perf_counter() - t0

    def path_c():
        t0 = time.perf_counter()
        for k0 in range(0, nb, 16):
            job = h.VerifyBlocksJob([(wires.ptr + at_w[k], wl[k]) for k in range(k0, min(nb, k0 + 16))], *ARGS, mp)
            arr = (Packet * (mp * job.n))()
            n_, u_, r_ = (ctypes.c_size_t * job.n)(), (ctypes.c_uint64 * job.n)(), (ctypes.c_int * job.n)()
            j, job.job = job.job, None
            assert lib.hdfs_crc32c_job_wait_blocks(j, arr, mp, n_, u_, r_) >= 0
        return time.perf_counter() - t0

    paths = (path_a, path_b, path_c)
    for p in paths:  # warm-up: code objects, scratch growth
        p()
    # A and B give the same outputs, records and bytes
    for k in range(nb):
        e = ent[k]
        assert (e.rc, e.npkts, e.consumed, e.delivered) == out_b[k], (k, out_b[k])
        assert bytes(pk_a)[k * mp * ctypes.sizeof(Packet):(k * mp + e.npkts) * ctypes.sizeof(Packet)] == \
            bytes(pk_b)[k * mp * ctypes.sizeof(Packet):(k * mp + e.npkts) * ctypes.sizeof(Packet)], k
        for o in range(0, e.delivered, 256 * MIB):
            n = min(256 * MIB, e.delivered - o)
            assert np.array_equal(dsts[0].download(n, at_d[k] + o), dsts[1].download(n, at_d[k] + o)), k
    n_kernel = sum(1 for k in range(nb) if ent[k].path == read_batch.PATH_KERNEL)
    t = [[], [], []]
    for _ in range(reps):  # alternate the three paths
        for i, p in enumerate(paths):
            t[i].append(p())
    sa, sb, sc = (_stats(x, nb) for x in t)
    verdict = "faster" if sa["max_us"] < sb["min_us"] else "slower" if sa["min_us"] > sb["max_us"] else "overlaps"
    ms = _median([read_batch.time([dict(stream_ptr=wires.ptr + at_w[k], nbytes=wl[k], dst_ptr=dsts[0].ptr + at_d[k],
                                        dst_cap=sizes[k]) for k in range(nb)], *ARGS, 0, iters)[0] for _ in range(3)])
    moved = sum(wl[k] + sizes[k] for k in range(nb) if ent[k].path == read_batch.PATH_KERNEL)
    return {"shape": name, "blocks": nb, "bytes": sum(sizes), "packets": sum(npk), "kernel_path": n_kernel,
            "fallback_path": nb - n_kernel, "batch": sa, "loop": sb, "verify_only_jobs_of_16": sc, "verdict": verdict,
            "launches_us_per_block": round(ms * 1e3 / nb, 3), "launches_TBps": round(moved / (ms * 1e-3) / 1e12, 3)}


def measure(reps=5, shapes="all", quick=False):
    h.load()
    arch, ncu = h.device_info()
    todo = {"small": SMALL, "large": LARGE, "all": LARGE + SMALL}[shapes]
    if quick:
        todo = [s for s in todo if sum(s[1]) <= 64 * MIB]
    most = max(sum(s[1]) for s in todo)
    blocks = max(len(s[1]) for s in todo)
    src = h.DeviceBuffer(max(max(s[1]) for s in todo) + 64)
    wires = h.DeviceBuffer(most + most // 100 + blocks * 4096 + MIB)
    dsts = [h.DeviceBuffer(most + blocks * 128 + MIB) for _ in range(2)]
    h.fill_splitmix64(src.ptr, src.nbytes // 8, 17, 0)
    h.device_sync()
    rows = []
    try:
        for name, sizes, corrupt in todo:
            rows.append(measure_shape(name, sizes, corrupt, src, wires, dsts, reps, 5))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    finally:
        for b in [src, wires] + dsts:
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
