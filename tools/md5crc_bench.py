"""MD5CRC block digests: the device path against its host alternative, for
DESIGN.md section 11 and the comment of include/hadoofus_md5crc.h.

Shape: blocks of 128 MiB at 512 B per CRC, i.e. 1 MiB of chunk CRCs per block
(the data itself is not needed: the CRC arrays are filled with splitmix64
words on the device).  For each batch size, in one process:
  device: hdfs_md5crc_block_digests over the batch (host clock around the
          call, which ends in a stream synchronise; 16 bytes per block back);
  host:   the same CRC arrays copied device-to-host into pinned memory (one
          copy), then hashlib.md5 per block on 16 threads.
Both give the same digests (asserted).  The batch sizes 1, 64 and 1024 are the
reported ones; the powers of two between them locate the batch size from
which the device path is the faster one.  GPU box only.

    python tools/md5crc_bench.py [--blocks 1024] [--reps 5] [--out file.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hadoofus_amd as h  # noqa: E402

CRC_BYTES = 1 << 20  # per block: 128 MiB / 512 B * 4 B
THREADS = 16


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def measure(max_blocks=1024, reps=5, sizes=None):
    h.load()
    arch, ncu = h.device_info()
    crcs = h.DeviceBuffer(max_blocks * CRC_BYTES)
    h.fill_splitmix64(crcs.ptr, max_blocks * CRC_BYTES // 8, 11, 0)
    h.device_sync()
    pin = h.PinnedBuffer(max_blocks * CRC_BYTES)
    view = memoryview(pin.array)
    segs = [h.Segment(data=None, len=128 << 20, chunk_size=512, flags=h.SEG_BE, crc_init=0,
                      crcs=crcs.ptr + b * CRC_BYTES, bitmap=None) for b in range(max_blocks)]
    pool = ThreadPoolExecutor(THREADS)
    if sizes is None:
        sizes = [n for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024) if n <= max_blocks]

    def host_path(n):
        t0 = time.perf_counter()
        crcs.copy_to(pin.ptr, n * CRC_BYTES)
        t1 = time.perf_counter()
        out = list(pool.map(lambda b: hashlib.md5(view[b * CRC_BYTES:(b + 1) * CRC_BYTES]).digest(), range(n)))
        return out, t1 - t0, time.perf_counter() - t1

    rows = []
    try:
        for n in sizes:
            got = h.block_md5crcs(segs[:n])  # warm-up: code object, scratch
            want, _, _ = host_path(n)        # warm-up: page touch, threads
            assert got == want, n
            dev, cp, md = [], [], []
            for _ in range(reps):  # alternate the two paths
                t0 = time.perf_counter()
                h.block_md5crcs(segs[:n])
                dev.append(time.perf_counter() - t0)
                _, c, m = host_path(n)
                cp.append(c)
                md.append(m)
            d, hc, hm = _median(dev), _median(cp), _median(md)
            rows.append({"blocks": n, "device_ms": round(d * 1e3, 3), "host_copy_ms": round(hc * 1e3, 3),
                         "host_md5_ms": round(hm * 1e3, 3), "host_total_ms": round((hc + hm) * 1e3, 3),
                         "device_min_ms": round(min(dev) * 1e3, 3), "device_max_ms": round(max(dev) * 1e3, 3),
                         "device_GiBps_of_crcs": round(n * CRC_BYTES / d / (1 << 30), 2)})
    finally:
        pool.shutdown()
        pin.free()
        crcs.free()
    faster = [r["blocks"] for r in rows if r["device_ms"] < r["host_total_ms"]]
    slower = [r["blocks"] for r in rows if r["device_ms"] >= r["host_total_ms"]]
    # the smallest measured batch from which the device path stays the faster one
    cross = None
    for r in rows:
        if all(q["device_ms"] < q["host_total_ms"] for q in rows if q["blocks"] >= r["blocks"]):
            cross = r["blocks"]
            break
    return {"arch": arch, "num_cu": ncu, "crc_bytes_per_block": CRC_BYTES, "host_threads": THREADS, "reps": reps,
            "rows": rows, "device_faster_at": faster, "host_faster_at": slower, "crossover_blocks": cross}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.blocks, a.reps)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
