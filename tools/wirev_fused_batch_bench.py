"""The wire streams of a batch of gather writes in one pass and one launch:
hdfs_wirev_fused_batch_compose against the way of doing the same job without
it and against a floor, for DESIGN.md section 19 and the comment of
include/hadoofus_wirev_fused_batch.h.

For each shape (writes x fragment lengths per write; block offset 4321, CRC32C,
v2, finish; every fragment of every write a range of its own at an odd address,
all buffers and argument arrays made beforehand), in one process:
  A, this call:   hdfs_wirev_fused_batch_compose, one call for all writes;
  B, gather loop: hdfs_wirev_fused_compose_packets, one call per write: what a
                  caller has without this library;
  C, floor:       hdfs_wire_fused_batch_compose on the same bytes already packed
                  contiguously (the packing is not timed).  No caller has this
                  for free; it shows what the fragment table and the seams
                  cost, not what a caller could do instead.
The host clock runs around each whole path (each ends synchronised).  All three
give the same bytes (asserted: every stream of every path is downloaded once
per shape and compared).  Medians of --reps with the three paths alternated
after a warm-up of each (one ahead of the comparison, one behind it), with the
min-max spread, per write.  `verdict` (A against B) and `verdict_floor` (A
against C) are "faster" only where A's whole range lies below the other's,
"slower" where it lies above, else "no difference shown".

Then the kernels alone through the timing entries (HIP events around ten
back-to-back launches, median of three): this library's on the product's grid,
the contiguous batch kernel's, and the single gather kernel's of the batch's
first write times the number of writes (what the loop's kernels add up to, the
writes of a shape being alike).  `layout_us` is hdfs_wirev_fused_batch_layout
alone, the host's walk over every fragment and packet.  GPU box only.

    python tools/wirev_fused_batch_bench.py [--reps 5] [--shapes small|large|all] [--out file.json]
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
from hadoofus_amd import wire_fused_batch, wirev_fused, wirev_fused_batch  # noqa: E402
from hadoofus_amd.abi import IoVec, OutPacket  # noqa: E402

MIB = 1 << 20
ARGS = (h.PROTO_V2, h.CSUM_CRC32C)
OFF = 4321
GAP = 3  # bytes between two fragments in the source buffer: neighbours are not contiguous, residues differ
# (writes, fragment lengths of each)
LARGE = [(16, [8 * MIB] * 16), (16, [128 * 1024] * 1024)]
SMALL = [(64, [65536] * 16), (1024, [4096] * 16), (1024, [65536]), (4096, [1365, 1366, 1365]), (64, [4097] * 2049)]


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _stats(xs, nwrites):
    us = lambda t: round(t * 1e6 / nwrites, 3)  # noqa: E731
    return {"us": us(_median(xs)), "min_us": us(min(xs)), "max_us": us(max(xs))}


def _verdict(a, b):
    if a["max_us"] < b["min_us"]:
        return "faster"
    if a["min_us"] > b["max_us"]:
        return "slower"
    return "no difference shown"


def _odd(x):
    return x | 1


def measure_shape(nw, lens, reps, iters):
    vlib, blib, clib = wirev_fused.load(), wirev_fused_batch.load(), wire_fused_batch.load()
    n, nf = sum(lens), len(lens)
    per = sum(ln + GAP + (ln + GAP) % 2 for ln in lens)  # an even step: every fragment at an odd address
    outs, tot = wirev_fused_batch.layout([dict(frags=[(None, ln) for ln in lens], offset_in_block=OFF, finish=True)] * nw,
                                         *ARGS)
    wl, npk = outs[0]["wire_len"], outs[0]["npkts"]
    wstep, pstep = (wl + 64) // 2 * 2, (n + 64) // 2 * 2
    src, pack = h.DeviceBuffer(nw * per + 64), h.DeviceBuffer(nw * pstep + 64)
    dst = [h.DeviceBuffer(nw * wstep + 64) for _ in range(3)]
    try:
        h.fill_splitmix64(src.ptr, (src.nbytes // 8), 19, 0)
        for d in dst:
            h.fill_splitmix64(d.ptr, d.nbytes // 8, 5, 0)  # not zeros: a byte left unwritten differs between the paths' buffers only by luck
        h.device_sync()
        vecs, writes, flat = [], [], []
        memcpy = h.load().hdfs_crc32c_memcpy
        for k in range(nw):
            vec, at, to = (IoVec * nf)(), _odd(src.ptr + k * per), _odd(pack.ptr + k * pstep)
            for i, ln in enumerate(lens):
                vec[i].base, vec[i].len = at, ln
                assert memcpy(to, at, ln, 2) == 0
                at, to = at + ln + GAP + (ln + GAP) % 2, to + ln
            vecs.append(vec)
            writes.append([dict(frags=vec, wire_ptr=_odd(d.ptr + k * wstep), wire_cap=wl, offset_in_block=OFF,
                                seqno=1000 * k, finish=True) for d in dst])
            flat.append(wire_fused_batch.write(dptr=_odd(pack.ptr + k * pstep), nbytes=n, wire_ptr=_odd(dst[2].ptr + k * wstep),
                                               wire_cap=wl, offset_in_block=OFF, seqno=1000 * k, finish=True))
        h.device_sync()
        arr_a, keep = wirev_fused_batch.entries([w[0] for w in writes])
        arr_c = wire_fused_batch.entries(flat)
        pk = [(OutPacket * (nw * npk))() for _ in range(3)]
        cnt, used = ctypes.c_size_t(0), ctypes.c_uint64(0)

        def path_a():
            t0 = time.perf_counter()
            rc = blib.hdfs_wirev_fused_batch_compose(arr_a, nw, *ARGS, pk[0], nw * npk, ctypes.byref(cnt), None)
            t = time.perf_counter() - t0
            assert rc == 0, blib.hdfs_wirev_fused_batch_last_error()
            return t

        b_args = [(vecs[k], nf, OFF, 1000 * k, *ARGS, 1, writes[k][1]["wire_ptr"], wl,
                   ctypes.cast(ctypes.addressof(pk[1]) + k * npk * ctypes.sizeof(OutPacket), ctypes.POINTER(OutPacket)), npk,
                   ctypes.byref(cnt), ctypes.byref(used), None) for k in range(nw)]

        def path_b():
            f = vlib.hdfs_wirev_fused_compose_packets
            t0 = time.perf_counter()
            for a in b_args:
                if f(*a) != 0:
                    raise AssertionError(vlib.hdfs_wirev_fused_last_error())
            return time.perf_counter() - t0

        def path_c():
            t0 = time.perf_counter()
            rc = clib.hdfs_wire_fused_batch_compose(arr_c, nw, *ARGS, pk[2], nw * npk, ctypes.byref(cnt), None)
            t = time.perf_counter() - t0
            assert rc == 0, clib.hdfs_wire_fused_batch_last_error()
            return t

        paths = (path_a, path_b, path_c)
        for p in paths:  # code objects, scratch growth; then every stream of every path compared
            p()
        want = dst[0].download()
        offs = [_odd(dst[0].ptr + k * wstep) - dst[0].ptr for k in range(nw)]
        for j in (1, 2):
            got = dst[j].download()
            o2 = [_odd(dst[j].ptr + k * wstep) - dst[j].ptr for k in range(nw)]
            for a, b in zip(offs, o2):
                assert np.array_equal(want[a:a + wl], got[b:b + wl]), f"path {'ABC'[j]}'s stream differs"
            del got
        del want
        assert bytes(pk[0]) == bytes(pk[2]), "the records of this call and of the floor differ"
        for k in range(0, nw, max(1, nw // 16)):  # the loop's records count in each write alone: the same per write
            assert bytes(pk[1])[k * npk * ctypes.sizeof(OutPacket):(k + 1) * npk * ctypes.sizeof(OutPacket)] == \
                bytes(pk[0])[k * npk * ctypes.sizeof(OutPacket):(k + 1) * npk * ctypes.sizeof(OutPacket)]
        for p in paths:  # the warm-up of each, behind the downloads
            p()
        ts = ([], [], [])
        for _ in range(reps):  # alternate the paths
            for t, p in zip(ts, paths):
                t.append(p())
        a, b, c = (_stats(t, nw) for t in ts)
        ka = _median([wirev_fused_batch.fused_batch_time([w[0] for w in writes], *ARGS, 0, iters) for _ in range(3)])
        kc = _median([wire_fused_batch.fused_batch_time(flat, *ARGS, 0, iters) for _ in range(3)])
        kb = _median([wirev_fused.fused_time([(vecs[0][i].base, vecs[0][i].len) for i in range(nf)],
                                             writes[0][1]["wire_ptr"], wl, OFF, *ARGS, True, 0, iters) for _ in range(3)])
        t0 = time.perf_counter()
        wirev_fused_batch.load().hdfs_wirev_fused_batch_layout(arr_a, nw, *ARGS, ctypes.byref(wirev_fused_batch.Totals()))
        lay = time.perf_counter() - t0
        return {"writes": nw, "write_bytes": n, "fragments": nf, "fragment_bytes": lens[0], "packets": tot["npkts"],
                "rounds": tot["rounds"], "seamed_rounds": tot["seamed_rounds"], "seamed_ragged": tot["seamed_ragged"],
                "this_call": a, "gather_loop": b, "floor": c, "verdict": _verdict(a, b), "verdict_floor": _verdict(a, c),
                "this_kernel_us": round(ka * 1e3 / nw, 3), "floor_kernel_us": round(kc * 1e3 / nw, 3),
                "gather_kernel_us": round(kb * 1e3, 3), "layout_us": round(lay * 1e6, 1)}
    finally:
        for b in [src, pack] + dst:
            b.free()


def measure(reps=5, which="all"):
    h.load()
    arch, ncu = h.device_info()
    todo = {"small": SMALL, "large": LARGE, "all": LARGE + SMALL}[which]
    return {"arch": arch, "num_cu": ncu, "reps": reps, "offset_in_block": OFF,
            "rows": [measure_shape(nw, lens, reps, 10) for nw, lens in todo]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", choices=("small", "large", "all"), default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.reps, a.shapes)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
