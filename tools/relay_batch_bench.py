"""A batch of verified reads re-framed as writes in one call:
hdfs_relay_batch_relay against the two calls it replaces, for DESIGN.md section
25 and the comment of include/hadoofus_relay_batch.h.

For each shape (a number of entries of one size and the data bytes of an input
packet; v2, CRC32C; every input stream composed on the device beforehand by the
fused batch write library -- one write per input packet, so packets of 64 512 B
come out as a datanode sends them -- with the empty last packet, each entry's
copy at its own odd address; all buffers allocated beforehand), in one process:
  A, relay:      hdfs_relay_batch_relay, one call for all entries;
  B, two calls:  hdfs_read_batch_read_blocks into a preallocated payload buffer
                 (no records), then hdfs_wire_fused_batch_compose of it (no
                 records): the libraries as they stand.
The host clock runs around each whole path (each ends synchronised).  Both
write the same streams (compared on the device once per shape, every byte of
every clean entry).  Medians of --reps with the two paths alternated after one
warm-up of each, with the min-max spread, per entry.  `verdict` is "faster"
only where A's whole range lies below B's, "slower" where it lies above, else
"overlaps".  Beside it the two launches alone, from the timing entry (HIP
events around back-to-back probe + main launches), and how many entries took
each path.  One shape corrupts one entry of 64: it prices one fallback (in B
the corrupt entry is read and not composed).
GPU box only.

    python tools/relay_batch_bench.py [--reps 5] [--quick] [--shapes small|large|all] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hadoofus_amd as h  # noqa: E402
from hadoofus_amd import wire_fused_batch as fb  # noqa: E402
from hadoofus_read import read_batch, relay_batch  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, 512, h.CSUM_CRC32C)
OFF, SEQ = 512, 3  # the writes': on the chunk grid
# (name, entries, bytes of an entry, data bytes of an input packet, index of an entry to corrupt or None)
LARGE = [("16 x 128 MiB, dlen0 65536", 16, 128 * MIB, 65536, None), ("16 x 128 MiB, dlen0 64512", 16, 128 * MIB, 64512, None),
         ("64 x 128 MiB, dlen0 65536", 64, 128 * MIB, 65536, None), ("64 x 128 MiB, dlen0 64512", 64, 128 * MIB, 64512, None),
         ("64 x 128 MiB, dlen0 64512, one corrupt", 64, 128 * MIB, 64512, 37)]
SMALL = [("64 x 1 MiB, dlen0 64512", 64, MIB, 64512, None), ("256 x 64 KiB, dlen0 64512", 256, 65536, 64512, None)]


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _stats(xs, n):
    us = lambda x: round(x * 1e6 / n, 3)  # noqa: E731  (per entry)
    return {"us": us(_median(xs)), "min_us": us(min(xs)), "max_us": us(max(xs))}


def input_stream(src, size, dlen0, dst_ptr):
    """One block transfer's stream of `size` payload bytes in packets of dlen0 at
    dst_ptr: a write per packet, the last one with finish.  -> its length."""
    cuts = list(range(0, size, dlen0))
    writes = [fb.write(nbytes=min(dlen0, size - o), offset_in_block=o, seqno=k, finish=k + 1 == len(cuts))
              for k, o in enumerate(cuts)]
    at = 0
    for i in range(0, len(writes), 512):
        part = writes[i:i + 512]
        outs, _ = fb.layout(part, ARGS[0], ARGS[2])
        todo = []
        for w, o in zip(part, outs):
            todo.append(fb.write(src.ptr + 1 + w["offset_in_block"], w["nbytes"], dst_ptr + at, o["wire_len"],
                                 w["offset_in_block"], w["seqno"], w["finish"]))
            at += o["wire_len"]
        fb.compose(todo, ARGS[0], ARGS[2])
    return at


def measure_shape(name, nb, size, dlen0, corrupt, src, ins, pay, outs, reps, iters):
    lib = h.load()
    slen = input_stream(src, size, dlen0, ins.ptr + 5)
    step_in = (slen + 64) // 16 * 16 + 1
    wl, npk = relay_batch.layout(size, OFF, ARGS[0], ARGS[2], True)
    step_out, step_pay = (wl + 64) // 16 * 16 + 3, (size + 64) // 16 * 16 + 2
    at_in = [5 + k * step_in for k in range(nb)]
    at_out, at_pay = [7 + k * step_out for k in range(nb)], [3 + k * step_pay for k in range(nb)]
    assert at_in[-1] + slen <= ins.nbytes and at_pay[-1] + size <= pay.nbytes and at_out[-1] + wl <= outs[0].numel()
    for k in range(1, nb):  # every entry its own copy
        assert lib.hdfs_crc32c_memcpy(ins.ptr + at_in[k], ins.ptr + at_in[0], slen, 2) == 0
    h.device_sync()
    if corrupt is not None:  # one data bit in the middle of that entry's stream
        at = at_in[corrupt] + slen // 2 + 4096
        byte = ins.download(1, at)
        ins.upload(byte ^ np.uint8(0x10), at)
    pa, pb = outs[0].data_ptr(), outs[1].data_ptr()
    batch_a = [relay_batch.entry(ins.ptr + at_in[k], slen, pa + at_out[k], wl, OFF, SEQ, True) for k in range(nb)]
    ent_a = relay_batch.entries(batch_a)
    ent_r = read_batch.entries([read_batch.entry(ins.ptr + at_in[k], slen, pay.ptr + at_pay[k], size) for k in range(nb)])
    keep = [k for k in range(nb) if k != corrupt]
    ent_w = fb.entries([fb.write(pay.ptr + at_pay[k], size, pb + at_out[k], wl, OFF, SEQ, True) for k in keep])
    rlib, blib, wlib = relay_batch.load(), read_batch.load(), fb.load()
    want_rc = 0 if corrupt is None else h.ERR_BAD_CHECKSUM

    def path_a():
        t0 = time.perf_counter()
        rc = rlib.hdfs_relay_batch_relay(ent_a, nb, *ARGS, None)
        t = time.perf_counter() - t0
        assert rc == want_rc, (rc, rlib.hdfs_relay_batch_last_error())
        return t

    def path_b():
        t0 = time.perf_counter()
        rc = blib.hdfs_read_batch_read_blocks(ent_r, nb, *ARGS, None, 0, None)
        rc2 = wlib.hdfs_wire_fused_batch_compose(ent_w, len(keep), ARGS[0], ARGS[2], None, 0, None, None)
        t = time.perf_counter() - t0
        assert rc == want_rc and rc2 == 0, (rc, rc2, wlib.hdfs_wire_fused_batch_last_error())
        return t

    paths = (path_a, path_b)
    for p in paths:  # warm-up: code objects, scratch growth
        p()
    # both wrote the same streams
    h.device_sync()
    torch.cuda.synchronize()
    for i, k in enumerate(keep):
        e = ent_a[k]
        assert (e.rc, e.consumed, e.delivered, e.wire_len, e.npkts) == (0, slen, size, wl, npk), (k, e.rc, e.wire_len)
        assert (ent_r[k].consumed, ent_r[k].delivered, ent_w[i].wire_len) == (slen, size, wl), k
        assert torch.equal(outs[0][at_out[k]:at_out[k] + wl], outs[1][at_out[k]:at_out[k] + wl]), k
    if corrupt is not None:
        e = ent_a[corrupt]
        assert (e.rc, e.wire_len, e.delivered) == (want_rc, 0, ent_r[corrupt].delivered), (e.rc, e.wire_len)
    n_kernel = sum(1 for k in range(nb) if ent_a[k].path == relay_batch.PATH_KERNEL)
    t = [[], []]
    for _ in range(reps):  # alternate the two paths
        for i, p in enumerate(paths):
            t[i].append(p())
    sa, sb = (_stats(x, nb) for x in t)
    verdict = "faster" if sa["max_us"] < sb["min_us"] else "slower" if sa["min_us"] > sb["max_us"] else "overlaps"
    ms = _median([relay_batch.time(batch_a, *ARGS, 0, iters)[0] for _ in range(3)])
    moved = sum(slen + wl for k in range(nb) if ent_a[k].path == relay_batch.PATH_KERNEL)
    return {"shape": name, "entries": nb, "payload_bytes": nb * size, "stream_bytes": slen, "wire_bytes": wl,
            "kernel_path": n_kernel, "fallback_path": nb - n_kernel, "relay": sa, "two_calls": sb, "verdict": verdict,
            "launches_us_per_entry": round(ms * 1e3 / nb, 3), "launches_TBps": round(moved / (ms * 1e-3) / 1e12, 3)}


def measure(reps=5, shapes="all", quick=False):
    h.load()
    arch, ncu = h.device_info()
    todo = {"small": SMALL, "large": LARGE, "all": LARGE + SMALL}[shapes]
    if quick:
        todo = [s for s in todo if s[1] * s[2] <= 64 * MIB]
    most = max(s[1] * s[2] for s in todo)
    room = most + most // 64 + max(s[1] for s in todo) * 4096 + MIB  # headers and CRCs are below 1 % of a stream
    src = h.DeviceBuffer(max(s[2] for s in todo) + 64)
    ins, pay = h.DeviceBuffer(room), h.DeviceBuffer(room)
    outs = [torch.empty(room, dtype=torch.uint8, device="cuda") for _ in range(2)]
    h.fill_splitmix64(src.ptr, src.nbytes // 8, 17, 0)
    h.device_sync()
    rows = []
    try:
        for name, nb, size, dlen0, corrupt in todo:
            rows.append(measure_shape(name, nb, size, dlen0, corrupt, src, ins, pay, outs, reps, 5))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    finally:
        for b in (src, ins, pay):
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
