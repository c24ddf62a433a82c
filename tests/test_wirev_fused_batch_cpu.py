"""CPU tests of the fused gather-wire batch companion library
(include/hadoofus_wirev_fused_batch.h): its build, linkage and ABI, the host
layout and the size query's packet records against the oracle's compose_packets
of every entry's concatenation, against hdfs_wirev_fused_layout per entry and
against hdfs_wire_fused_batch_layout on the summed lengths, the rejections the
entry points decide without a GPU, the kernel's register and LDS metadata from
a cross-compile, and the index logic that connects the kernel's two lookups run
on the CPU against a brute-force model
(tests/consumer/wirev_fused_batch_selftest.cpp, built with ASan/UBSan, nothing
loaded into Python).  Everything is bit-exact."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from abi_symbols import c_functions as _c_functions, declared as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
DECLARED = {"hdfs_wirev_fused_batch_abi_version", "hdfs_wirev_fused_batch_last_error",
            "hdfs_wirev_fused_batch_compose", "hdfs_wirev_fused_batch_layout", "hdfs_wirev_fused_batch_time"}
# the eight other companions and their version nodes, as their own tests pin them
OTHERS = {"md5crc": "HADOOFUS_MD5CRC_1", "writev": "HADOOFUS_WRITEV_1", "wire": "HADOOFUS_WIRE_1",
          "wire_batch": "HADOOFUS_WIRE_BATCH_1", "wirev": "HADOOFUS_WIREV_1", "wire_fused": "HADOOFUS_WIRE_FUSED_1",
          "wire_fused_batch": "HADOOFUS_WIRE_FUSED_BATCH_1", "wirev_fused": "HADOOFUS_WIREV_FUSED_1"}
OWN = ["wirev_fused_batch_kernels.hip", "wirev_fused_batch.cpp", "wirev_fused_batch_internal.h",
       "wirev_fused_batch_lookup.h"]


@pytest.fixture(scope="module")
def libs():
    """(release library, fused gather-wire batch companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.WIREV_FUSED_BATCH_LIB


@pytest.fixture(scope="module")
def wvb(libs):
    from hadoofus_amd import wirev_fused_batch
    wirev_fused_batch.load()
    return wirev_fused_batch


# ---- what connects the kernel's two lookups, on the CPU -----------------------------------
def test_wirev_fused_batch_selftest(tmp_path):
    exe = tmp_path / "wirev_fused_batch_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "wirev_fused_batch_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout


# ---- layout and records against the oracle and the two parents ------------------------------
LENS = [0, 1, 511, 512, 513, 1100, 65536, 2 * 65536 + 700]
DATA = np.random.default_rng(81).integers(0, 256, max(LENS), dtype=np.uint8)
SPLITS = [1, 2, 7]


def split(n, k, seed):
    """n bytes cut into k fragment lengths at random places (empty fragments
    occur: cuts repeat, and k may exceed n)."""
    cuts = np.sort(np.random.default_rng(seed).integers(0, n + 1, k - 1))
    return [int(x) for x in np.diff(np.concatenate(([0], cuts, [n])))]


def expected(oracle, n, off, seq, proto, ctype, finish):
    """The oracle's packets of the write alone, hdr_off moved into its stream.
    -> (wire_len, records, nchunks)."""
    hdr, pkts = oracle.compose_packets(DATA[:n], off, seq, proto, ctype, finish)
    at, out, nchunks = 0, [], 0
    for p in pkts:
        out.append(dict(p, hdr_off=at))
        at += p["hdr_len"] + p["data_len"]
        nchunks += (p["data_len"] + 511) // 512
    assert at == len(hdr) + n
    return at, out, nchunks


def lens_write(wvb, lens, **kw):
    return wvb.write(frags=[(None, n) for n in lens], **kw)  # a size query reads no base


@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("proto", [1, 2])
def test_layout_and_size_query_match_the_oracle_and_both_parents(wvb, oracle, proto, ctype):
    """One batch of all eight lengths x both block offsets x finish, in 1, 2 and
    7 fragments per write (96 writes), each with a sequence number of its own."""
    from hadoofus_amd import wire_fused_batch, wirev_fused
    shapes = [(n, off, fin, k) for k in SPLITS for fin in (False, True) for off in (0, 4321) for n in LENS]
    frags = [split(n, k, 1000 * k + n % 997 + off) for n, off, fin, k in shapes]
    assert all(len(f) == s[3] and sum(f) == s[0] for f, s in zip(frags, shapes))
    writes = [lens_write(wvb, f, offset_in_block=off, seqno=1000 * i + 11, finish=fin)
              for i, (f, (n, off, fin, k)) in enumerate(zip(frags, shapes))]
    want = [expected(oracle, n, off, 1000 * i + 11, proto, ctype, fin) for i, (n, off, fin, k) in enumerate(shapes)]
    got = wvb.packet_records(writes, proto, ctype)
    outs, tot = wvb.layout(writes, proto, ctype)
    assert len(got) == len(want) == len(outs)
    first = 0
    sums = dict(nfrags=0, rounds=0, seamed_rounds=0, seamed_ragged=0)
    most = 0
    for i, (g, x, o, f, (n, off, fin, k)) in enumerate(zip(got, want, outs, frags, shapes)):
        assert g[0] == x[0] and len(g[1]) == len(x[1]), i
        for a, b in zip(g[1], x[1]):  # field by field
            assert set(a) == set(b) and all(a[fld] == b[fld] for fld in b), (i, a, b)
        assert o == {"len": n, "wire_len": x[0], "npkts": len(x[1]), "first_pkt": first}, i
        first += len(x[1])
        one = wirev_fused.layout(f, off, proto, ctype, fin)  # the single-write library's counters of this entry
        assert (one["npkts"], one["wire_len"]) == (len(x[1]), x[0]), i
        assert wirev_fused.packet_records(f, off, 1000 * i + 11, proto, ctype, fin) == g, i
        for fld in sums:
            sums[fld] += one[fld]
        most = max(most, one["max_frags_per_round"])
    common = {"npkts": first, "nchunks": sum(x[2] for x in want), "wire_bytes": sum(x[0] for x in want),
              "table_entries": sum(1 for x in want if x[1])}
    assert tot == dict(common, max_frags_per_round=most, **sums)
    assert tot["table_entries"] == len(writes) - 6 and tot["seamed_rounds"] > 0 and tot["seamed_ragged"] > 0
    # the contiguous fused batch library on the summed lengths: the common totals and the entries' out fields
    flat = [wire_fused_batch.write(nbytes=n, offset_in_block=off, seqno=1000 * i + 11, finish=fin)
            for i, (n, off, fin, k) in enumerate(shapes)]
    fouts, ftot = wire_fused_batch.layout(flat, proto, ctype)
    assert ftot == common and fouts == [{f: o[f] for f in ("wire_len", "npkts", "first_pkt")} for o in outs]
    assert wire_fused_batch.packet_records(flat, proto, ctype) == got


def test_empty_writes_anywhere_and_the_empty_batch(wvb):
    e = lens_write(wvb, [])
    e2 = lens_write(wvb, [0, 0])
    f = lens_write(wvb, [], finish=True, seqno=7)
    d = lens_write(wvb, [500, 0, 13], seqno=3)
    outs, tot = wvb.layout([e, f, e2, d, e])
    assert [o["npkts"] for o in outs] == [0, 1, 0, 1, 0] and [o["first_pkt"] for o in outs] == [0, 0, 1, 1, 2]
    assert outs[1]["wire_len"] == 31 and outs[3]["len"] == 513
    assert (tot["table_entries"], tot["npkts"], tot["nfrags"], tot["rounds"], tot["seamed_rounds"]) == (2, 2, 2, 1, 1)
    got = wvb.packet_records([e, f, e2, d, e])
    assert got[0] == (0, []) and got[1][1][0]["last"] == 1 and got[1][1][0]["seqno"] == 7
    assert got[3][1][0]["data_len"] == 513 and got[3][1][0]["hdr_off"] == 0
    zero = {"npkts": 0, "nchunks": 0, "wire_bytes": 0, "table_entries": 0, "nfrags": 0, "rounds": 0,
            "seamed_rounds": 0, "seamed_ragged": 0, "max_frags_per_round": 0}
    assert wvb.layout([]) == ([], zero) and wvb.packet_records([]) == []


def test_counters_of_known_batches(wvb):
    """Counts worked out by hand (tests/test_wirev_fused_cpu.py's, added up)."""
    n = 2 * 65536 + 700
    w = lambda lens, off=4321: lens_write(wvb, lens, offset_in_block=off, finish=True)  # noqa: E731
    f = lambda ws: tuple(wvb.layout(ws)[1][k] for k in  # noqa: E731
                         ("nfrags", "rounds", "seamed_rounds", "seamed_ragged", "max_frags_per_round"))
    assert f([w([n])]) == (1, 32, 0, 0, 1)
    assert f([w([n]), w([286, n - 286]), w([287 + 4097, n - 287 - 4097])]) == (5, 96, 1, 1, 2)
    assert f([w([1] * 1300), w([n]), w([1] * 1300, 0)]) == (2601, 34, 2, 3, 1024)
    assert f([w([1] * 1300, 0), w([]), w([0, 4000, 0, 0, 700, 0, 396], 0)]) == (1303, 3, 2, 2, 1024)


def test_the_limits_are_judged_in_closed_form(wvb):
    """MAX_WRITES + 1 writes, MAX_FRAGS + 1 fragments (the iovec array built
    with numpy; a size query reads no base), more than 1 TiB in one write and
    more than (2^31 - 1) / 4 packets (33 writes of 1 TiB, 2^24 packets each):
    each refused at once, before any write's packets are walked."""
    from hadoofus_amd.abi import IoVec
    lib, tot, npk = wvb.load(), wvb.Totals(), ctypes.c_size_t(9)
    err = lambda: lib.hdfs_wirev_fused_batch_last_error()  # noqa: E731
    one, _keep = wvb.entries([lens_write(wvb, [10])])
    assert lib.hdfs_wirev_fused_batch_layout(one, wvb.MAX_WRITES + 1, 2, 2, ctypes.byref(tot)) == EINVAL
    assert b"65536" in err()
    assert lib.hdfs_wirev_fused_batch_compose(one, wvb.MAX_WRITES + 1, 2, 2, None, 0, ctypes.byref(npk), None) == EINVAL
    assert npk.value == 0
    # MAX_FRAGS + 1 one-byte fragments with NULL bases, in two entries; MAX_FRAGS are allowed
    half = wvb.MAX_FRAGS // 2
    raw = np.zeros((half + 1, 2), dtype=np.uint64)
    raw[:, 1] = 1
    vec = (IoVec * (half + 1)).from_buffer(raw)
    big = [wvb.write(frags=vec, iovcnt=half), wvb.write(frags=vec, iovcnt=half + 1, finish=True)]
    arr, _keep = wvb.entries(big)
    assert lib.hdfs_wirev_fused_batch_layout(arr, 2, 2, 2, ctypes.byref(tot)) == EINVAL
    assert b"entry 1" in err() and b"4194304 fragments" in err()
    assert lib.hdfs_wirev_fused_batch_compose(arr, 2, 2, 2, None, 0, ctypes.byref(npk), None) == EINVAL
    assert npk.value == 0 and (arr[0].len, arr[0].npkts, arr[1].npkts) == (half, 0, 0)
    arr[1].iovcnt = half
    assert lib.hdfs_wirev_fused_batch_layout(arr, 2, 2, 2, ctypes.byref(tot)) == 0
    assert (tot.nfrags, tot.npkts, tot.max_frags_per_round) == (wvb.MAX_FRAGS, 2 * (half // 65536) + 1, 4096)
    assert tot.rounds == tot.seamed_rounds == 2 * (half // 4096) and tot.seamed_ragged == 0
    # 1 TiB per write: the sum of the fragments counts
    tib, _keep = wvb.entries([lens_write(wvb, [5]), lens_write(wvb, [1 << 39, (1 << 39) + 1])])
    assert lib.hdfs_wirev_fused_batch_layout(tib, 2, 2, 2, ctypes.byref(tot)) == EINVAL
    assert b"entry 1" in err() and b"1 TiB" in err()
    many, _keep = wvb.entries([lens_write(wvb, [1 << 39, 1 << 39])] * 33)
    assert lib.hdfs_wirev_fused_batch_layout(many, 33, 2, 2, ctypes.byref(tot)) == EINVAL
    assert b"packets in the batch" in err()


# ---- rejections that need no device ---------------------------------------------
def test_rejections_without_a_device(wvb):
    from hadoofus_amd.abi import OutPacket
    lib = wvb.load()
    fake = 0x1000  # never dereferenced: every call below is decided by its arguments
    pk = (OutPacket * 8)()
    before = bytes(pk)
    npk = ctypes.c_size_t(99)

    def call(writes, proto=2, ctype=2, maxp=8, query=False, n=None, out=pk):
        arr, keep = wvb.entries(writes, query)
        rc = lib.hdfs_wirev_fused_batch_compose(arr, len(writes) if n is None else n, proto, ctype, out, maxp,
                                                ctypes.byref(npk), None)
        return rc, arr, lib.hdfs_wirev_fused_batch_last_error().decode()

    def w(lens=(600, 400), bases=None, **kw):
        bases = bases if bases is not None else [fake + 0x10000 * (i + 1) for i in range(len(lens))]
        return wvb.write(**dict(dict(frags=list(zip(bases, lens)), wire_ptr=fake + (1 << 24), wire_cap=1 << 20), **kw))
    good = [w(), w(lens=(30000, 0, 40000)), w(lens=(), finish=True)]
    sizes = [(1000, 1039, 1, 0), (70000, 70000 + 2 * 31 + 4 * 137, 2, 1), (0, 31, 1, 3)]
    outs = lambda arr, n=3: [(e.len, e.wire_len, e.npkts, e.first_pkt) for e in arr[:n]]  # noqa: E731
    # arguments of the whole batch
    for kw in (dict(proto=0), dict(proto=3), dict(ctype=3), dict(ctype=-1)):
        rc, arr, err = call(good, **kw)
        assert rc == EINVAL and "entry 0" in err and npk.value == 0, (kw, err)
    rc, _, err = call(good, n=wvb.MAX_WRITES + 1)
    assert rc == EINVAL and "65536" in err and npk.value == 0
    # arguments of one entry: the text names it, and the fragment where one is at fault
    rc, _, err = call([good[0], good[1], w(offset_in_block=-1)])
    assert rc == EINVAL and "entry 2" in err, err
    rc, _, err = call([good[0], w(lens=(1 << 39, (1 << 39) + 1))])
    assert rc == EINVAL and "entry 1" in err and "1 TiB" in err, err
    rc, _, err = call([good[0], w(lens=(0, 1 << 62, 1))])
    assert rc == EINVAL and "entry 1" in err and "fragment 2" in err, err
    rc, _, err = call([good[0], good[1], w(iovcnt=-1)])
    assert rc == EINVAL and "entry 2" in err and "negative" in err and npk.value == 0, err
    arr, keep = wvb.entries([good[0], good[1]])
    arr[1].iov = None
    assert lib.hdfs_wirev_fused_batch_compose(arr, 2, 2, 2, pk, 8, ctypes.byref(npk), None) == EINVAL
    assert b"entry 1" in lib.hdfs_wirev_fused_batch_last_error() and npk.value == 0
    arr[1].iovcnt = 0  # a NULL list of no fragments is an empty write
    assert lib.hdfs_wirev_fused_batch_compose(arr, 2, 2, 2, pk, 8, ctypes.byref(npk), None) != 0  # (0x1000 is no device memory)
    assert npk.value == 1 and arr[1].len == 0
    rc, arr, err = call([good[0], w(lens=(5, 7), bases=[fake, None])])
    assert rc == EINVAL and "entry 1" in err and "fragment 1" in err and outs(arr, 2)[1] == (12, 47, 1, 1), err
    # undersized outputs: EINVAL, the sizes reported, nothing written
    rc, arr, err = call([good[0], w(lens=(30000, 0, 40000), wire_cap=sizes[1][1] - 1), good[2]])
    assert rc == EINVAL and "entry 1" in err, err
    assert npk.value == 4 and outs(arr) == sizes
    rc, arr, err = call(good, maxp=2)
    assert rc == EINVAL and "entry 1" in err and npk.value == 4 and outs(arr) == sizes, err
    rc, arr, err = call(good, maxp=3)
    assert rc == EINVAL and "entry 2" in err and npk.value == 4, err
    # some wires NULL, some not
    rc, arr, err = call([good[0], w(wire_ptr=None), good[2]])
    assert rc == EINVAL and "entry 1" in err and npk.value == 3 and arr[2].first_pkt == 2, err
    rc, arr, err = call([w(wire_ptr=None), w(wire_ptr=None), good[2]])
    assert rc == EINVAL and "entry 2" in err, err
    assert bytes(pk) == before
    # a size query with room for the records fills them and reads no base; without room it only counts
    rc, arr, _ = call([w(bases=[None, None]), good[1], good[2]], query=True)
    assert rc == 0 and npk.value == 4 and pk[0].hdr_len == 39 and pk[1].data_len == 65536 and pk[3].last == 1
    assert outs(arr) == sizes
    ctypes.memset(pk, 0, ctypes.sizeof(pk))
    rc, arr, _ = call(good, query=True, maxp=3)
    assert rc == 0 and npk.value == 4 and bytes(pk) == before
    # nothing but empty writes without finish: no packet, no work, no device, whatever wire is
    rc, arr, _ = call([w(lens=()), w(lens=(0, 0), bases=[None, None])] * 2)
    assert rc == 0 and npk.value == 0


def test_layout_and_timing_argument_errors(wvb):
    lib = wvb.load()
    one = [wvb.write(frags=[(0x1000, 10)], wire_ptr=0x2000, wire_cap=100)]
    arr, keep = wvb.entries(one)
    assert lib.hdfs_wirev_fused_batch_layout(arr, 1, 2, 2, None) == EINVAL
    tot = wvb.Totals()
    assert lib.hdfs_wirev_fused_batch_layout(arr, 1, 5, 2, ctypes.byref(tot)) == EINVAL
    assert lib.hdfs_wirev_fused_batch_layout(arr, 1, 2, 9, ctypes.byref(tot)) == EINVAL
    assert lib.hdfs_wirev_fused_batch_layout(None, 1, 2, 2, ctypes.byref(tot)) == EINVAL
    ms = ctypes.c_double(0)

    def call(flags=0, iters=1, out=ctypes.byref(ms), proto=2, query=False):
        a, keep = wvb.entries(one, query)
        rc = lib.hdfs_wirev_fused_batch_time(a, 1, proto, 2, flags, iters, out)
        return rc, (a[0].len, a[0].wire_len, a[0].npkts, a[0].first_pkt), lib.hdfs_wirev_fused_batch_last_error()
    # every one decided before a device is asked (0x1000 is no device memory: going on would say so)
    for kw in (dict(iters=0), dict(out=None), dict(query=True)):
        rc, outs, err = call(**kw)
        assert rc == EINVAL and outs == (10, 45, 1, 0) and b"device" not in err, (kw, err)
    assert call(proto=7)[0] == EINVAL
    # workgroups out of range, or a flag bit that means nothing
    for flags in (wvb.time_groups(wvb.MAX_GROUPS + 1), wvb.time_groups(1 << 23), 1, wvb.time_groups(2) | 4):
        rc, outs, err = call(flags=flags)
        assert rc == EINVAL and b"workgroups" in err and outs == (10, 45, 1, 0), (flags, err)


# ---- build, linkage and ABI -----------------------------------------------------------
def test_build_produces_the_library_beside_the_others(libs):
    lib, flib = libs
    from hadoofus_amd import build
    assert os.path.exists(flib) and os.path.basename(flib) == "libhadoofus_wirev_fused_batch.so"
    assert os.path.dirname(lib) == os.path.dirname(flib)
    for other in (build.MD5CRC_LIB, build.WRITEV_LIB, build.WIRE_LIB, build.WIRE_BATCH_LIB, build.WIREV_LIB,
                  build.WIRE_FUSED_LIB, build.WIRE_FUSED_BATCH_LIB, build.WIREV_FUSED_LIB):
        assert os.path.exists(other) and os.path.dirname(other) == os.path.dirname(flib), other


def test_build_lists_sources_and_headers():
    from hadoofus_amd import build
    assert build.WIREV_FUSED_BATCH_SOURCES == ["wirev_fused_batch_kernels.hip", "wirev_fused_batch.cpp"]
    assert {"wirev_fused_batch_internal.h", "wirev_fused_batch_lookup.h", "wirev_fused_internal.h",
            "wirev_fused_lookup.h", "wire_fused_batch_lookup.h", "wire_fused_round.h", "wire_fused_crc.h",
            "wire_fused_tables.h", "wire_fused_host.h", "wire_layout.h", "wire_batch_layout.h", "wire_internal.h",
            "companion_support.h", "crc32c_outpkt.h", "crc32c_tables.h",
            "wirev_fused_batch_exports.map"} <= set(build.WIREV_FUSED_BATCH_HEADERS)
    assert "hadoofus_wirev_fused_batch.h" in build.WIREV_FUSED_BATCH_PUBLIC and build.ARCH == "gfx950"
    for f in build.WIREV_FUSED_BATCH_SOURCES + build.WIREV_FUSED_BATCH_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f
        assert f not in ("writev_layout.h", "writev_kernels.hip", "writev_internal.h", "wirev_internal.h",
                         "wirev_fused_kernels.hip", "wire_fused_batch_kernels.hip"), f
    assert "A ninth companion, libhadoofus_wirev_fused_batch.so" in build.__doc__
    assert "An eighth companion, libhadoofus_wirev_fused.so" in build.__doc__ and "Six companion libraries" in build.__doc__


def test_sources_hold_no_plan_call_no_polynomial_and_no_gather_layout():
    """The CRCs are this library's own kernel's: no compute plan anywhere in
    it, the tables come from crc32c_tables.h, the one place the polynomials are
    written; the layout, the batch front end and the headers are the shared
    code's; nothing of the gather libraries is compiled into it."""
    from hadoofus_amd import build
    for f in OWN:
        src = open(os.path.join(build.CSRC, f)).read()
        assert "hdfs_crc32c_plan_" not in src, f
        assert "put_header_proto" not in src and "put_out_header" not in src, f
        for poly in ("82f63b78", "edb88320"):
            assert poly not in src.lower(), (f, poly)
        for name in ("writev_layout.h", "writev_kernels.hip", "writev_internal.h", "hadoofus_writev.h",
                     "hadoofus_wirev.h", "hadoofus_wirev_fused.h", "hadoofus_wire_fused_batch.h", "wire_frame.h",
                     "gather_plan(", "enqueue_gather("):
            assert name not in src, (f, name)
        assert not re.search(r"int build_layout\(const uint64_t \*lens", src), f
    host = open(os.path.join(build.CSRC, "wirev_fused_batch.cpp")).read()
    for inc in ("wire_layout.h", "wire_batch_layout.h", "wire_fused_host.h", "wire_fused_tables.h",
                "wirev_fused_lookup.h"):
        assert f'#include "{inc}"' in host, inc
    for name in ("count_batch(", "layout_entries(", "check_entries(", "fill_batch_records(", "layout_totals(",
                 "check_overlaps(", "count_packet(", "timed_frame_run(", "Allocations al", "TablePair tab",
                 "DeviceState<prepare_frame_fused_gather_batch, kBatchMaxGroups>", "kTableFloor"):
        assert name in host, name
    assert not re.search(r"^\w[\w ]*\b(build_layout|fill_records|count_batch|layout_entries|check_entries|"
                         r"check_overlaps|count_packet|frag_of|write_of)\(", host, flags=re.M)  # and defines none
    assert "plan_out_packets(" not in host and host.count("hipMemcpyAsync(") == 1
    und = subprocess.check_output(["nm", "-D", "--undefined-only", build.WIREV_FUSED_BATCH_LIB], text=True)
    assert "hdfs_crc32c_plan_" not in und


def test_one_definition_of_the_round_and_of_each_lookup():
    """The kernel file includes the shared round, the seamed round and the
    lookups and holds no copy of any, no buffer builtin, no permlane and no
    Unit of its own; what connects the lookups compiles without HIP."""
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    code = lambda f: "\n".join(l for l in read(f).splitlines() if not l.lstrip().startswith("//"))  # noqa: E731
    helpers = ["range_of(", "load16(", "store16(", "store32(", "load8(", "store8(", "fold8(", "transpose(",
               "unit_of(", "load_round(", "store_round(", "crc_round(", "header(", "ragged_chunk(", "ragged_finish(",
               "fill_image("]
    gather = ["edge_piece(", "seam_round(", "ragged_gather("]
    rnd, gat = read("wire_fused_round.h"), read("wirev_fused_internal.h")
    for name in helpers:
        assert len(re.findall(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), rnd)) == 1, name
    for name in gather:
        assert len(re.findall(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), gat)) == 1, name
    for f in OWN:
        src = code(f)
        assert "struct Unit" not in src and "__builtin_amdgcn_raw_buffer" not in src and "permlane" not in src, f
        for name in helpers + gather:
            assert not re.search(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), src), (f, name)
        assert "uint32_t frag_of(" not in src and "uint32_t write_of(" not in src and "atomic" not in src.lower(), f
        assert "struct Frag " not in src and "struct AtOf" not in src, f
    every = "".join(read(f) for f in sorted(os.listdir(build.CSRC)))
    assert every.count("uint32_t frag_of(") == 1 and every.count("uint32_t write_of(") == 1
    assert every.count("void count_packet(") == 1 and every.count("bool seek_write(") == 1
    kern = code("wirev_fused_batch_kernels.hip")
    for inc in ("wire_fused_round.h", "wirev_fused_batch_internal.h", "wirev_fused_batch_lookup.h"):
        assert f'#include "{inc}"' in kern, inc
    for name in ("load_round(", "store_round(", "crc_round<CSUM>(", "header(", "unit_of(", "seam_round(",
                 "ragged_gather<CSUM>(", "seek_write(", "slice_of(", "seek_frag(", "address_space(4)"):
        assert name in kern or name in code("wirev_fused_internal.h"), name
    assert kern.count("seek_write(") == 1 and kern.count("seek_frag(") == 1 and "Cursor kc = c;" in kern
    look = code("wirev_fused_batch_lookup.h")
    assert "hip" not in look.lower() and '#include "wire_fused_batch_lookup.h"' in look
    assert '#include "wirev_fused_lookup.h"' in look


def test_lookup_header_compiles_without_hip(tmp_path):
    src = tmp_path / "l.cpp"
    src.write_text('#include "wirev_fused_batch_lookup.h"\n'
                   "int main() { hdfs_wirev_fused_batch::Cursor c; const uint32_t pk0[3] = {0, 2, 5}, fr0[3] = {0, 4, 6};\n"
                   "const uint64_t at[6] = {0, 1, 2, 9, 0, 7};\n"
                   "bool in = hdfs_wirev_fused_batch::seek_write(pk0, 2u, 5u, 1u, c); c.kf = 2;\n"
                   "in = in && hdfs_wirev_fused_batch::seek_write(pk0, 2u, 5u, 3u, c) && c.kw == 1 && c.kf == 0;\n"
                   "const hdfs_wirev_fused_batch::Slice s = hdfs_wirev_fused_batch::slice_of(fr0, c.kw);\n"
                   "in = in && s.first == 4 && s.nf == 1 && hdfs_wirev_fused_batch::seek_frag(at + s.first, s.nf, 6, c) == 0;\n"
                   "return in && !hdfs_wirev_fused_batch::seek_write(pk0, 2u, 5u, 5u, c) ? 0 : 1; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_kernel_metadata(tmp_path):
    """hipcc cross-compiles the kernel file to gfx950 assembly, nothing runs:
    both instances keep everything in registers (no scratch, no VGPR spill) and
    have no static LDS; the dynamic LDS is the launcher's: the table image and
    the header with checksums (159 776 B), the header alone without (32 B)."""
    from hadoofus_amd import build
    out = tmp_path / "wirev_fused_batch_kernels.s"
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           "-I" + build.INCLUDE, "-I" + build.CSRC, "-o", str(out),
                           os.path.join(build.CSRC, "wirev_fused_batch_kernels.hip")], stderr=subprocess.DEVNULL)
    txt = out.read_text()
    meta = re.findall(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                      r"\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?"
                      r"\s+\.vgpr_spill_count:\s+(\d+)", txt)
    assert len(meta) == 2 and all("frame_fused_gather_batch_kernel" in m[1] for m in meta), meta
    for lds, name, scratch, vgpr, spill in meta:
        assert (int(lds), int(scratch), int(spill)) == (0, 0, 0), (name, lds, scratch, spill)
        assert int(vgpr) <= 128, (name, vgpr)  # 16 waves of a workgroup on one CU
    kern = open(os.path.join(build.CSRC, "wirev_fused_batch_kernels.hip")).read()
    assert kern.count("(crc::kImageWords + kHdrWords) * sizeof(uint32_t)") == 2  # prepare and the launch with checksums
    assert kern.count("kHdrWords * sizeof(uint32_t), stream") == 1
    # the sizes those expressions stand for, from the same headers (plain C++, nothing of HIP)
    src, exe = tmp_path / "lds.cpp", tmp_path / "lds"
    src.write_text('#include <cstdio>\n#include "wire_fused_tables.h"\n'
                   'int main() { std::printf("%u", unsigned((hdfs_wire_fused::crc::kImageWords + 8u) * 4u)); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I" + build.CSRC, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True) == "159776"
    assert "constexpr uint32_t kHdrWords = 8;" in open(os.path.join(build.CSRC, "wire_fused_round.h")).read()


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_wirev_fused_batch.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_wirev_fused_batch_write) - 80 + "
                   "(int)sizeof(hdfs_wirev_fused_batch_totals) - 72 + HDFS_WIREV_FUSED_BATCH_ABI_VERSION - 1 + "
                   "(int)HDFS_WIREV_FUSED_BATCH_TIME_GROUPS(0) + HDFS_WIREV_FUSED_BATCH_MAX_WRITES - 65536 + "
                   "(int)(HDFS_WIREV_FUSED_BATCH_MAX_FRAGS - 4194304u); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layouts_match_c(tmp_path):
    from hadoofus_amd.wirev_fused_batch import BatchWrite, Totals
    pinned = {"hdfs_wirev_fused_batch_write": (BatchWrite, [80, 0, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72]),
              "hdfs_wirev_fused_batch_totals": (Totals, [72, 0, 8, 16, 24, 32, 40, 48, 56, 64, 68])}
    for cname, (S, want) in pinned.items():
        names = [f for f, _ in S._fields_]
        src = tmp_path / (cname + ".c")
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_wirev_fused_batch.h"\n'
                       f'int main(void){{ printf("%zu", sizeof({cname}));\n' +
                       "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n in names) + "return 0; }\n")
        exe = tmp_path / cname
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                               "-o", str(exe)])
        got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
        assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names], cname
        assert got == want, cname  # pinned: the ABI of version 1
    assert [f for f, _ in BatchWrite._fields_] == ["iov", "iovcnt", "finish", "offset_in_block", "seqno", "wire",
                                                   "wire_cap", "len", "wire_len", "npkts", "first_pkt"]
    assert [f for f, _ in Totals._fields_] == ["npkts", "nchunks", "wire_bytes", "table_entries", "nfrags", "rounds",
                                               "seamed_rounds", "seamed_ragged", "max_frags_per_round", "reserved"]


def test_companion_exports_exactly_its_header(libs):
    _, flib = libs
    assert _declared("hadoofus_wirev_fused_batch.h") == DECLARED
    funcs = _c_functions(flib)
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_wirev_fused_batch.h")).read()
    v = int(re.search(r"#define HDFS_WIREV_FUSED_BATCH_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_WIREV_FUSED_BATCH_{v}"}, funcs
    assert "HADOOFUS_WIREV_FUSED_BATCH_1 {" in open(os.path.join(ROOT, "hadoofus_amd", "csrc",
                                                                "wirev_fused_batch_exports.map")).read()


def test_main_library_and_its_abi_are_unchanged(libs):
    lib, _ = libs
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert "hdfs_wirev_fused_batch" not in out and "HADOOFUS_WIREV_FUSED_BATCH" not in out
    main_hdr = open(os.path.join(ROOT, "include", "hadoofus_crc32c.h")).read()
    assert "wirev_fused_batch" not in main_hdr and "#define HDFS_CRC32C_ABI_VERSION 5" in main_hdr
    # the committed signature list still ends at version 5 and is the headers'
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_signatures
    txt = open(os.path.join(ROOT, "tests", "golden", "abi_signatures.txt")).read()
    assert "wirev_fused_batch" not in txt and max(int(x) for x in re.findall(r"^\[(\d+)\]$", txt, flags=re.M)) == 5
    cur = dict(l.split(": ", 1) for l in txt.split("[5]\n", 1)[1].splitlines() if l and not l.startswith("#"))
    assert abi_signatures.header_prototypes() == cur


def test_the_eight_other_companions_export_what_they_did(libs):
    """Each exports exactly its header's functions under its own version node,
    none of them has a symbol of this library, and their headers and export
    maps do not speak of it."""
    lib, _ = libs
    libdir = os.path.dirname(lib)
    for name, node in OTHERS.items():
        funcs = _c_functions(os.path.join(libdir, f"libhadoofus_{name}.so"))
        assert set(funcs) == _declared(f"hadoofus_{name}.h"), (name, set(funcs) ^ _declared(f"hadoofus_{name}.h"))
        assert set(funcs.values()) == {node}, (name, funcs)
        assert not any("wirev_fused_batch" in f for f in funcs), name
        for f in (f"include/hadoofus_{name}.h", f"hadoofus_amd/csrc/{name}_exports.map"):
            assert "wirev_fused_batch" not in open(os.path.join(ROOT, f)).read().lower(), f


def test_companion_links_the_one_engine_and_no_other_companion(libs):
    """It needs the release library, found beside it, and no other library of
    the project; it reaches the engine through three calls of its public API."""
    lib, flib = libs
    dyn = subprocess.check_output(["readelf", "-d", flib], text=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert [n for n in needed if "hadoofus" in n] == ["libhadoofus_crc32c.so"] and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", flib], text=True)
    engine = sorted(l.split()[-1].split("@")[0] for l in und.splitlines() if "hdfs_" in l)
    assert engine == ["hdfs_crc32c_bound_device", "hdfs_crc32c_init", "hdfs_crc32c_last_error"]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert all(s in main for s in engine)


def test_abi_version_call_and_binding_check(wvb):
    assert wvb.load().hdfs_wirev_fused_batch_abi_version() == wvb.ABI_VERSION == 1
    assert wvb.MAX_GROUPS == 1024 and wvb.time_groups(3) == 3 << 8
    assert wvb.MAX_WRITES == 65536 and wvb.MAX_FRAGS == 1 << 22

    class Other:
        @staticmethod
        def hdfs_wirev_fused_batch_abi_version():
            return 2
    with pytest.raises(ImportError):
        wvb.check_abi(Other())


def test_last_error_text_is_its_own(wvb):
    """An EINVAL provoked here leaves the single-write gather library's text
    alone, and the other way round."""
    from hadoofus_amd import wirev_fused
    vl, lib = wirev_fused.load(), wvb.load()
    lens = (ctypes.c_uint64 * 1)(10)
    assert vl.hdfs_wirev_fused_layout(lens, 1, 0, 7, 2, 0, ctypes.byref(wirev_fused.LayoutInfo())) == EINVAL
    before = vl.hdfs_wirev_fused_last_error()
    arr, keep = wvb.entries([lens_write(wvb, [1], offset_in_block=-1)], True)
    assert lib.hdfs_wirev_fused_batch_layout(arr, 1, 2, 2, ctypes.byref(wvb.Totals())) == EINVAL
    assert lib.hdfs_wirev_fused_batch_last_error() == b"entry 0: negative block offset"
    assert vl.hdfs_wirev_fused_last_error() == before == b"proto must be 1 or 2"


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, wirev_fused, wire_fused_batch, wirev_fused_batch\n"
            "assert abi._lib is None and wirev_fused._lib is None and wire_fused_batch._lib is None\n"
            "assert wirev_fused_batch._lib is None\n"
            "assert callable(h.compose_wirev_fused_batch) and callable(h.wirev_fused_batch_layout)\n"
            "assert callable(wirev_fused_batch.fused_batch_time) and callable(wirev_fused_batch.packet_records)\n"
            "assert callable(wirev_fused_batch.time_groups) and callable(wirev_fused_batch.check_abi)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "wirev_fused_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wirev_fused_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wirev_fused_batch", "-lhadoofus_crc32c"])
    assert exe.exists()
