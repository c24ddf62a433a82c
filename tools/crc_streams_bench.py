"""Composite CRCs taken from packet streams: hdfs_crc_streams_block_crcs against
what a caller does without it, for DESIGN.md section 24 and the comment of
include/hadoofus_crc_streams.h.

For each shape (v2, CRC32C; every block's payload its own bytes in device
memory, its packet stream composed beforehand at an odd address; all buffers
allocated beforehand), in one process:
  A, streams: hdfs_crc_streams_block_crcs, one call for all blocks;
  B, today:   a compute plan over the blocks' payloads (created beforehand,
              executed here) plus hdfs_crc32c_composite_crcs over the CRC arrays
              it leaves: a second pass over every payload byte and 4 B of
              scratch per chunk;
  C, floor:   hdfs_crc32c_composite_crcs alone over those CRC arrays, packed
              beforehand;
  D, md5crc:  hdfs_md5crc_streams_block_digests of the same streams (HDFS's
              other checksum mode from the same bytes).
The host clock runs around each whole path (each ends synchronised), and every
path is the raw library call on ctypes arrays built beforehand, as a C caller
would make it: no Python wrapper's marshalling is inside a timed region.  Medians
of --reps with the four paths alternated after one warm-up of each, with the
min-max spread, in milliseconds per call.  A, B and C give the same CRCs
(asserted once per shape).  `verdict` is "faster" only where A's whole range
lies below B's, "slower" where it lies above, else "overlaps"; `vs_floor` the
same against C, `vs_md5crc` against D.  Beside it the three launches alone, from
the timing entry (HIP events around back-to-back probe + fold + reduce
launches).

Streams of 64 KiB packets come from the fused batch write library.  No library
composes 5 120-byte packets, so that shape's stream is laid out on the host
from block 0's payload and the CRCs path B computed for it, uploaded once and
copied device to device for every block: the blocks' streams are distinct
memory with the same bytes, and only block 0's CRC is compared with B and C.
GPU box only.

    python tools/crc_streams_bench.py [--reps 5] [--quick] [--max-blocks 1024] [--out file.json]
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
from hadoofus_read import crc_streams, md5crc_streams  # noqa: E402

MIB = 1 << 20
BLOCK = 128 * MIB
ARGS = (h.PROTO_V2, 512, h.CSUM_CRC32C)


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _stats(xs):
    ms = lambda x: round(x * 1e3, 3)  # noqa: E731
    return {"ms": ms(_median(xs)), "min_ms": ms(min(xs)), "max_ms": ms(max(xs))}


def _verdict(a, b):
    return "faster" if a["max_ms"] < b["min_ms"] else "slower" if a["min_ms"] > b["max_ms"] else "overlaps"


def free_device_bytes():
    """Free memory of the current device, from the HIP runtime the libraries share."""
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def small_packet_stream(data, crcs_be, dlen=5120):
    """One block's v2 stream of dlen-byte packets, a shorter one and the empty
    last one, laid out with numpy.  data: the payload; crcs_be: its chunk CRCs
    as wire bytes.  -> uint8 array."""
    n = data.size
    K, tail = n // dlen, n % dlen
    wpp = dlen // 512

    def headers(offs, seqs, dl, last):
        k = offs.size
        hd = np.zeros((k, 31), dtype=np.uint8)
        plen = np.full(k, dl + 4 * ((dl + 511) // 512) + 4, dtype=">u4")
        hd[:, 0:4] = plen.view(np.uint8).reshape(k, 4)
        hd[:, 4:6] = (0, 25)
        hd[:, 6] = 0x09
        hd[:, 7:15] = offs.astype("<i8").view(np.uint8).reshape(k, 8)
        hd[:, 15] = 0x11
        hd[:, 16:24] = seqs.astype("<i8").view(np.uint8).reshape(k, 8)
        hd[:, 24] = 0x18
        hd[:, 25] = last
        hd[:, 26] = 0x25
        hd[:, 27:31] = np.full(k, dl, dtype="<u4").view(np.uint8).reshape(k, 4)
        return hd
    body = np.empty((K, 31 + 4 * wpp + dlen), dtype=np.uint8)
    body[:, :31] = headers(np.arange(K, dtype=np.int64) * dlen, np.arange(K, dtype=np.int64), dlen, 0)
    body[:, 31:31 + 4 * wpp] = crcs_be[:4 * wpp * K].reshape(K, 4 * wpp)
    body[:, 31 + 4 * wpp:] = data[:K * dlen].reshape(K, dlen)
    parts, seq = [body.reshape(-1)], K
    if tail:
        parts += [headers(np.array([K * dlen]), np.array([seq]), tail, 0).reshape(-1), crcs_be[4 * wpp * K:],
                  data[K * dlen:]]
        seq += 1
    parts.append(headers(np.array([n]), np.array([seq]), 0, 1).reshape(-1))
    return np.concatenate(parts)


def measure_shape(name, nb, size, pkt, payloads, wires, crcs, reps, iters):
    slib, mlib = crc_streams.load(), md5crc_streams.load()
    per_crc = (size + 511) // 512 * 4
    segs = [h.Segment(data=payloads.ptr + b * size, len=size, chunk_size=512, flags=h.SEG_BE, crc_init=0,
                      crcs=crcs.ptr + b * per_crc, bitmap=None) for b in range(nb)]
    plan = h.Plan(h.MODE_COMPUTE, segs)
    plan.execute(None)
    h.device_sync()
    if pkt == 65536:
        writes = [wire_fused_batch.write(nbytes=size, finish=True) for _ in range(nb)]
        outs, _ = wire_fused_batch.layout(writes, ARGS[0], ARGS[2])
        wl = [o["wire_len"] for o in outs]
        stride = (wl[0] + 64) // 16 * 16 + 1
        at = [5 + k * stride for k in range(nb)]
        assert at[-1] + wl[-1] <= wires.nbytes
        for k0 in range(0, nb, 256):
            wire_fused_batch.compose([wire_fused_batch.write(payloads.ptr + k * size, size, wires.ptr + at[k], wl[k],
                                                             0, 0, True) for k in range(k0, min(nb, k0 + 256))],
                                     ARGS[0], ARGS[2])
        same = nb
    else:
        one = small_packet_stream(payloads.download(size), crcs.download(per_crc), pkt)
        wl = [one.size] * nb
        stride = (one.size + 64) // 16 * 16 + 1
        at = [5 + k * stride for k in range(nb)]
        assert at[-1] + wl[-1] <= wires.nbytes
        wires.upload(one, at[0])
        for k in range(1, nb):
            assert h.load().hdfs_crc32c_memcpy(wires.ptr + at[k], wires.ptr + at[0], one.size, 2) == 0
        same = 1  # only block 0's stream carries its own payload's CRCs
    h.device_sync()
    ent = crc_streams.entries([crc_streams.entry(wires.ptr + at[k], wl[k]) for k in range(nb)])
    # every path is timed as a C caller would run it: the raw library call on arrays built beforehand
    mlib0 = h.load()
    seg_arr, out_b, out_c = (h.Segment * nb)(*segs), (ctypes.c_uint32 * nb)(), (ctypes.c_uint32 * nb)()
    ment = md5crc_streams.entries([md5crc_streams.entry(wires.ptr + at[k], wl[k]) for k in range(nb)])

    def path_a():
        t0 = time.perf_counter()
        rc = slib.hdfs_crc_streams_block_crcs(ent, nb, *ARGS, None)
        t = time.perf_counter() - t0
        assert rc == 0, (rc, slib.hdfs_crc_streams_last_error())
        return t

    def path_b():
        t0 = time.perf_counter()
        rc = mlib0.hdfs_crc32c_plan_execute(plan.ptr, None)
        rc = rc or mlib0.hdfs_crc32c_composite_crcs(seg_arr, nb, out_b)
        t = time.perf_counter() - t0
        assert rc == 0, (rc, mlib0.hdfs_crc32c_last_error())
        return t

    def path_c():
        t0 = time.perf_counter()
        rc = mlib0.hdfs_crc32c_composite_crcs(seg_arr, nb, out_c)
        t = time.perf_counter() - t0
        assert rc == 0, (rc, mlib0.hdfs_crc32c_last_error())
        return t

    def path_d():
        t0 = time.perf_counter()
        rc = mlib.hdfs_md5crc_streams_block_digests(ment, nb, *ARGS, None)
        t = time.perf_counter() - t0
        assert rc == 0, (rc, mlib.hdfs_md5crc_streams_last_error())
        return t

    paths = (path_a, path_b, path_c, path_d)
    for p in paths:  # warm-up: code objects, scratch growth
        p()
    got = [ent[k].crc for k in range(nb)]
    assert got[:same] == list(out_b)[:same] == list(out_c)[:same], name
    assert len(set(got[same:]) | {got[0]}) == 1 or same == nb, name
    assert all(ent[k].rc == 0 and ent[k].consumed == wl[k] and ent[k].payload == size and
               ent[k].nchunks == per_crc // 4 for k in range(nb)), name
    n_kernel = sum(1 for k in range(nb) if ent[k].path == crc_streams.PATH_KERNEL)
    t = [[], [], [], []]
    for _ in range(reps):  # alternate the four paths
        for i, p in enumerate(paths):
            t[i].append(p())
    sa, sb, sc, sd = (_stats(x) for x in t)
    batch = [dict(stream_ptr=wires.ptr + at[k], nbytes=wl[k]) for k in range(nb)]
    ms = _median([crc_streams.time(batch, *ARGS, 0, iters)[0] for _ in range(3)])
    return {"shape": name, "blocks": nb, "block_bytes": size, "packet_bytes": pkt, "crcs_per_block": per_crc // 4,
            "kernel_path": n_kernel, "fallback_path": nb - n_kernel, "streams": sa, "plan_plus_composite": sb,
            "composite_of_packed_crcs": sc, "md5crc_streams": sd, "verdict": _verdict(sa, sb),
            "vs_floor": _verdict(sa, sc), "vs_md5crc": _verdict(sa, sd), "launches_ms": round(ms, 3)}


def measure(reps=5, quick=False, max_blocks=1024):
    h.load()
    arch, ncu = h.device_info()
    # payloads + streams + CRC arrays per 128 MiB block, and a fifth of the device left alone
    most = int(free_device_bytes() * 0.8 // (2 * BLOCK + 3 * MIB))
    big = max(64, min(max_blocks, most // 64 * 64))
    shapes = [(f"{n} x 128 MiB", n, BLOCK, 65536) for n in sorted({1, 64, min(256, big), big})]
    shapes += [(f"{min(256, big)} x 128 MiB, 5 120-byte packets", min(256, big), BLOCK, 5120),
               ("1024 x 1 MiB", 1024, MIB, 65536)]
    if quick:
        shapes = [("4 x 8 MiB", 4, 8 * MIB, 65536), ("4 x 8 MiB, 5 120-byte packets", 4, 8 * MIB, 5120),
                  ("64 x 1 MiB", 64, MIB, 65536)]
    most_bytes = max(s[1] * s[2] for s in shapes)
    most_blocks = max(s[1] for s in shapes)
    payloads = h.DeviceBuffer(most_bytes)
    wires = h.DeviceBuffer(most_bytes + most_bytes // 64 + most_blocks * 4096 + MIB)
    crcs = h.DeviceBuffer(most_bytes // 128 + most_blocks * 16 + MIB)
    for o in range(0, most_bytes, 1 << 30):  # every block its own bytes
        h.fill_splitmix64(payloads.ptr + o, min(1 << 30, most_bytes - o) // 8, 23, o // 8)
    h.device_sync()
    rows = []
    try:
        for name, nb, size, pkt in shapes:
            rows.append(measure_shape(name, nb, size, pkt, payloads, wires, crcs, reps, 5))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    finally:
        for b in (payloads, wires, crcs):
            b.free()
    return {"arch": arch, "num_cu": ncu, "reps": reps, "rows": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="three small shapes only")
    ap.add_argument("--max-blocks", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reps, a.quick, a.max_blocks)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
