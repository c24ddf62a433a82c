"""CPU tests of the wire-batch companion library
(include/hadoofus_wire_batch.h): the library's build and ABI, the host layout
and the size query's packet records of whole batches against the oracle's
compose_packets of each write alone, and the rejections the entry point decides
without a GPU.  Everything is bit-exact."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from abi_symbols import c_functions as _c_functions, declared as _declared, exported as _exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
DECLARED = {"hdfs_wire_batch_abi_version", "hdfs_wire_batch_last_error", "hdfs_wire_batch_compose",
            "hdfs_wire_batch_layout", "hdfs_wire_batch_frame_time"}
# the exported sets of the other companions, as their own tests pin them
OTHERS = {
    "libhadoofus_wire.so": ("HADOOFUS_WIRE_1", {"hdfs_wire_abi_version", "hdfs_wire_last_error",
                                                "hdfs_wire_compose_packets", "hdfs_wire_layout",
                                                "hdfs_wire_frame_time"}),
    "libhadoofus_writev.so": ("HADOOFUS_WRITEV_1", None),
    "libhadoofus_md5crc.so": ("HADOOFUS_MD5CRC_1", None),
}


@pytest.fixture(scope="module")
def libs():
    """(release library, wire-batch companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.WIRE_BATCH_LIB


@pytest.fixture(scope="module")
def wb(libs):
    from hadoofus_amd import wire_batch
    wire_batch.load()
    return wire_batch


# ---- layout and records against the oracle ----------------------------------------
LENS = [0, 1, 287, 511, 512, 513, 65536, 65537, 3 * 65536 + 123]
DATA = np.random.default_rng(78).integers(0, 256, max(LENS), dtype=np.uint8)


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


@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("proto", [1, 2])
def test_layout_and_size_query_match_the_oracle(wb, oracle, proto, ctype, finish):
    """One batch of all nine lengths at both block offsets, each write with a
    sequence number of its own."""
    writes = [wb.write(nbytes=n, offset_in_block=off, seqno=1000 * k + 11, finish=finish)
              for k, (n, off) in enumerate((n, off) for off in (0, 4321) for n in LENS)]
    want = [expected(oracle, w["nbytes"], w["offset_in_block"], w["seqno"], proto, ctype, finish) for w in writes]
    got = wb.packet_records(writes, proto, ctype)
    assert [(g[0], g[1]) for g in got] == [(x[0], x[1]) for x in want]
    outs, tot = wb.layout(writes, proto, ctype)
    first = 0
    for o, x in zip(outs, want):
        assert o == {"wire_len": x[0], "npkts": len(x[1]), "first_pkt": first}
        first += len(x[1])
    assert tot == {"npkts": first, "nchunks": sum(x[2] for x in want), "wire_bytes": sum(x[0] for x in want),
                   "table_entries": sum(1 for x in want if x[1])}
    assert tot["table_entries"] == (len(writes) if finish else len(writes) - 2)


def test_empty_writes_anywhere_and_the_empty_batch(wb):
    e = wb.write(nbytes=0)
    f = wb.write(nbytes=0, finish=True, seqno=7)
    d = wb.write(nbytes=513, seqno=3)
    outs, tot = wb.layout([e, f, e, d, e])
    assert [o["npkts"] for o in outs] == [0, 1, 0, 1, 0] and [o["first_pkt"] for o in outs] == [0, 0, 1, 1, 2]
    assert outs[1]["wire_len"] == 31 and tot["table_entries"] == 2 and tot["npkts"] == 2
    got = wb.packet_records([e, f, e, d, e])
    assert got[0] == (0, []) and got[1][1][0]["last"] == 1 and got[1][1][0]["seqno"] == 7
    assert got[3][1][0]["data_len"] == 513 and got[3][1][0]["hdr_off"] == 0
    assert wb.layout([]) == ([], {"npkts": 0, "nchunks": 0, "wire_bytes": 0, "table_entries": 0})
    assert wb.packet_records([]) == []


def test_size_query_of_large_writes(wb):
    """64 writes of 128 MiB, counts in closed form."""
    n = 128 << 20
    outs, tot = wb.layout([wb.write(nbytes=n, offset_in_block=4321 if k % 2 else 0, finish=True) for k in range(64)])
    assert [o["npkts"] for o in outs[:2]] == [2049, 2050] and outs[2]["first_pkt"] == 4099
    assert tot["npkts"] == 32 * (2049 + 2050) and tot["table_entries"] == 64
    assert tot["wire_bytes"] == 64 * n + 31 * tot["npkts"] + 4 * tot["nchunks"]


# ---- rejections that need no device ---------------------------------------------
def test_rejections_without_a_device(wb):
    from hadoofus_amd.abi import OutPacket
    lib = wb.load()
    fake = 0x1000  # never dereferenced: every call below is decided by its arguments
    pk = (OutPacket * 8)()
    before = bytes(pk)
    npk = ctypes.c_size_t(99)

    def call(writes, proto=2, ctype=2, maxp=8, query=False, n=None, out=pk):
        arr = wb.entries(writes, query)
        rc = lib.hdfs_wire_batch_compose(arr, len(writes) if n is None else n, proto, ctype, out, maxp,
                                         ctypes.byref(npk), None)
        return rc, arr, lib.hdfs_wire_batch_last_error().decode()

    def w(**kw):
        return wb.write(**dict(dict(dptr=fake, nbytes=1000, wire_ptr=fake + (1 << 20), wire_cap=1 << 20), **kw))
    good = [w(), w(nbytes=70000), w(nbytes=0, finish=True)]
    # arguments of the whole batch
    assert call(good, proto=0)[0] == EINVAL and call(good, proto=3)[0] == EINVAL
    assert call(good, ctype=3)[0] == EINVAL and call(good, ctype=-1)[0] == EINVAL
    rc, _, err = call(good, n=wb.MAX_WRITES + 1)
    assert rc == EINVAL and "65536" in err and npk.value == 0
    # arguments of one entry: the text names it
    for bad in (w(offset_in_block=-1), w(nbytes=(1 << 40) + 1)):
        rc, _, err = call([good[0], good[1], bad])
        assert rc == EINVAL and "entry 2" in err, err
    rc, arr, err = call([good[0], w(dptr=None, nbytes=5)])
    assert rc == EINVAL and "entry 1" in err  # null data; entries() keeps dptr None
    # undersized outputs: EINVAL, the sizes reported, nothing written
    rc, arr, err = call([good[0], w(nbytes=70000, wire_cap=70000 + 2 * 31 + 4 * 137 - 1), good[2]])
    assert rc == EINVAL and "entry 1" in err, err
    assert npk.value == 4 and [(e.wire_len, e.npkts, e.first_pkt) for e in arr[:3]] == \
        [(1039, 1, 0), (70000 + 2 * 31 + 4 * 137, 2, 1), (31, 1, 3)]
    rc, arr, err = call(good, maxp=2)
    assert rc == EINVAL and "entry 1" in err and npk.value == 4 and arr[2].first_pkt == 3, err
    rc, arr, err = call(good, maxp=3)
    assert rc == EINVAL and "entry 2" in err and npk.value == 4, err
    # some wires NULL, some not
    rc, arr, err = call([good[0], w(wire_ptr=None), good[2]])
    assert rc == EINVAL and "entry 1" in err and npk.value == 3 and arr[2].first_pkt == 2, err
    rc, arr, err = call([w(wire_ptr=None), w(wire_ptr=None), good[2]])
    assert rc == EINVAL and "entry 2" in err, err
    assert bytes(pk) == before
    # a size query with room for the records fills them; without room it only counts
    rc, arr, _ = call(good, query=True)
    assert rc == 0 and npk.value == 4 and pk[0].hdr_len == 39 and pk[1].data_len == 65536 and pk[3].last == 1
    ctypes.memset(pk, 0, ctypes.sizeof(pk))
    rc, arr, _ = call(good, query=True, maxp=3)
    assert rc == 0 and npk.value == 4 and bytes(pk) == before
    # nothing but empty writes without finish: no packet, no work, no device, whatever wire is
    rc, arr, _ = call([w(nbytes=0, dptr=None)] * 3)
    assert rc == 0 and npk.value == 0


def test_chunk_limit_of_the_batch(wb):
    """2^32 - 16 chunks at most, judged in closed form before any write's
    packets are walked: 2^32 - 15 and 2^32 chunks are refused."""
    lib = wb.load()
    tot = wb.Totals()
    npk = ctypes.c_size_t(0)
    tib = wb.write(nbytes=1 << 40)  # 2^31 chunks
    for other in (tib, wb.write(nbytes=(1 << 40) - 16 * 512 + 1),
                  wb.write(nbytes=(1 << 40) - 16 * 512, offset_in_block=511)):  # one more: the short first chunk
        arr = wb.entries([tib, other], True)
        assert lib.hdfs_wire_batch_layout(arr, 2, 2, 2, ctypes.byref(tot)) == EINVAL
        assert "chunks" in lib.hdfs_wire_batch_last_error().decode()
        assert lib.hdfs_wire_batch_compose(arr, 2, 2, 2, None, 0, ctypes.byref(npk), None) == EINVAL


def test_layout_and_timing_argument_errors(wb):
    lib = wb.load()
    arr = wb.entries([wb.write(dptr=0x1000, nbytes=10, wire_ptr=0x2000, wire_cap=100)])
    assert lib.hdfs_wire_batch_layout(arr, 1, 2, 2, None) == EINVAL
    tot = wb.Totals()
    assert lib.hdfs_wire_batch_layout(arr, 1, 5, 2, ctypes.byref(tot)) == EINVAL
    assert lib.hdfs_wire_batch_layout(arr, 1, 2, 9, ctypes.byref(tot)) == EINVAL
    assert lib.hdfs_wire_batch_layout(None, 1, 2, 2, ctypes.byref(tot)) == EINVAL
    ms = ctypes.c_double(0)
    assert lib.hdfs_wire_batch_frame_time(arr, 1, 2, 2, 0, ctypes.byref(ms)) == EINVAL
    assert lib.hdfs_wire_batch_frame_time(arr, 1, 2, 2, 1, None) == EINVAL
    assert lib.hdfs_wire_batch_frame_time(wb.entries([wb.write(nbytes=10)], True), 1, 2, 2, 1,
                                          ctypes.byref(ms)) == EINVAL


# ---- build and ABI ------------------------------------------------------------------
def test_build_produces_the_library(libs):
    lib, blib = libs
    assert os.path.exists(blib) and os.path.basename(blib) == "libhadoofus_wire_batch.so"
    assert os.path.dirname(lib) == os.path.dirname(blib)


def test_build_lists_sources_and_headers():
    from hadoofus_amd import build
    assert build.WIRE_BATCH_SOURCES == ["wire_batch_kernels.hip", "wire_batch.cpp"]
    assert {"wire_batch_internal.h", "wire_frame.h", "wire_layout.h", "wire_internal.h", "crc32c_outpkt.h",
            "wire_batch_exports.map"} <= set(build.WIRE_BATCH_HEADERS)
    for headers in (build.MD5CRC_HEADERS, build.WRITEV_HEADERS, build.WIRE_HEADERS, build.WIRE_BATCH_HEADERS):
        assert "companion_support.h" in headers
    assert "hadoofus_wire_batch.h" in build.WIRE_BATCH_PUBLIC and build.ARCH == "gfx950"
    assert build.WIRE_SOURCES == ["wire_kernels.hip", "wire.cpp"]
    assert {"wire_frame.h", "wire_layout.h"} <= set(build.WIRE_HEADERS)
    for f in build.WIRE_BATCH_SOURCES + build.WIRE_BATCH_HEADERS + build.WIRE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    for f in build.WIRE_BATCH_SOURCES + ["wire_batch_internal.h", "wire_frame.h", "wire_layout.h"]:
        src = open(os.path.join(build.CSRC, f)).read()
        # no CRC arithmetic of its own
        assert "crc32c_tables.h" not in src and "0x82F63B78" not in src and "0xEDB88320" not in src, f


def test_one_definition_of_the_framing_and_layout_code():
    """The framing body lives in wire_frame.h, the layout code, the plan
    segments of a write and the timed frame run in wire_layout.h, and what all
    four companions share in companion_support.h; the sources of the libraries
    include them and hold no copy, nor one of the header-writing code of
    crc32c_outpkt.h."""
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    device = ["copy_region(", "copy_header(", "cut16(", "shift_window(", "void issue(", "frame_packet("]
    host = ["int build_layout(", "void fill_records(", "bool args_ok(", "size_t grid_segments("]
    support = ["int device_range(", "int fail(", "int engine_fail(", "int prefix_fail(", "int engine_device(",
               "bool packet_args_ok(", "int sync_and_report(", "Placement placement("]
    frame, lay, sup = read("wire_frame.h"), read("wire_layout.h"), read("companion_support.h")
    cpps = ("md5crc.cpp", "writev.cpp", "wire.cpp", "wire_batch.cpp")
    for name in device:
        assert len(re.findall(r"WIRE_DEV [\w:<> ]*\b" + re.escape(name), frame)) == 1, name
    for name in host:
        assert frame.count(name) == 0 and sup.count(name) == 0 and lay.count("inline " + name) == 1, name
    assert lay.count("\nint timed_frame_run(") == 1 and "timed_frame_run" not in sup + frame
    # companion_support.h: exactly one definition, none in wire_layout.h or in any of the four sources
    for name in support:
        assert sup.count("inline " + name) == 1 and sup.count(name) == 1, name
        for f in ("wire_layout.h", "wire_frame.h") + cpps:
            assert name not in read(f), (f, name)
    for name in ("struct DeviceGuard", "struct DeviceScratch", "struct GrowOnly", "struct Allocations",
                 "thread_local char g_err"):
        assert sup.count(name) == 1, name
        for f in ("wire_layout.h", "wire_frame.h") + cpps:
            assert name not in read(f), (f, name)
    assert '#include "companion_support.h"' in lay
    for f in ("wire_kernels.hip", "wire_batch_kernels.hip"):
        src = read(f)
        assert '#include "wire_frame.h"' in src and "frame::frame_packet<" in src, f
        for name in device[:-1] + host + support:
            assert name not in src, (f, name)
        assert "v_alignbyte" not in src and "alignbyte(" not in src and "global_store" not in src, f
    for f in ("wire.cpp", "wire_batch.cpp"):
        src = read(f)
        assert '#include "wire_layout.h"' in src, f
        for name in host:
            assert not re.search(r"^\w[\w ]*\b" + re.escape(name), src, flags=re.M), (f, name)
        assert "plan_out_packets(" not in src and "timed_frame_run(" in src and "grid_segments(" in src, f
        for gone in ("hipStreamSynchronize", "hipEventRecord", "hdfs_crc32c_plan_execute", "HDFS_CRC32C_SEG_BE"):
            assert gone not in src, (f, gone)  # the run and the segments are wire_layout.h's alone
    # the pointer queries of all four libraries are companion_support.h's; no kernel file includes it
    companion = set(build.MD5CRC_SOURCES + build.MD5CRC_HEADERS + build.WRITEV_SOURCES + build.WRITEV_HEADERS +
                    build.WIRE_SOURCES + build.WIRE_HEADERS + build.WIRE_BATCH_SOURCES + build.WIRE_BATCH_HEADERS)
    for f in sorted(companion - {"companion_support.h"}):
        src = read(f)
        assert "hipPointerGetAttributes" not in src and "hipMemGetAddressRange" not in src, f
        assert f.endswith(".cpp") or f == "wire_layout.h" or "companion_support.h" not in src, f
    for f in cpps:
        assert "companion_support.h" in read(f) or '#include "wire_layout.h"' in read(f), f
    for f in build.WIRE_SOURCES + build.WIRE_BATCH_SOURCES + ["wire_frame.h", "wire_layout.h", "wire_batch_internal.h"]:
        src = read(f)
        assert "put_header_proto(uint8_t" not in src and "put_out_header(uint8_t" not in src, f
    assert "hdfs_crc32c::outpkt::put_out_header(" in frame


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_wire_batch.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_wire_batch_write) - 80 + "
                   "(int)sizeof(hdfs_wire_batch_totals) - 32 + HDFS_WIRE_BATCH_ABI_VERSION - 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


@pytest.mark.parametrize("cname,pyname", [("hdfs_wire_batch_write", "BatchWrite"),
                                          ("hdfs_wire_batch_totals", "Totals")])
def test_struct_layout_matches_c(tmp_path, cname, pyname):
    from hadoofus_amd import wire_batch
    S = getattr(wire_batch, pyname)
    names = [f for f, _ in S._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_wire_batch.h"\n'
                   f'int main(void){{ printf("%zu", sizeof({cname}));\n' +
                   "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    # pinned: the ABI of version 1
    want = {"BatchWrite": [80, 0, 8, 16, 24, 32, 36, 40, 48, 56, 64, 72], "Totals": [32, 0, 8, 16, 24]}[pyname]
    assert got == want


def test_companion_exports_exactly_its_header(libs):
    _, blib = libs
    assert _declared("hadoofus_wire_batch.h") == DECLARED
    funcs = _exported(blib)
    funcs = {n: v for n, v in funcs.items() if n not in ("_init", "_fini")}
    # the toolchain may export a kernel's host stub; nothing else is allowed
    funcs = {n: v for n, v in funcs.items() if not (n.startswith("_ZN9hdfs_wire") and "_kernel" in n)}
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_wire_batch.h")).read()
    v = int(re.search(r"#define HDFS_WIRE_BATCH_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_WIRE_BATCH_{v}"}, funcs


def test_main_library_and_its_abi_are_unchanged(libs):
    lib, _ = libs
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert "hdfs_wire" not in out and "HADOOFUS_WIRE" not in out
    main_hdr = open(os.path.join(ROOT, "include", "hadoofus_crc32c.h")).read()
    assert "hdfs_wire" not in main_hdr and "#define HDFS_CRC32C_ABI_VERSION 5" in main_hdr
    # the committed signature list still ends at version 5 and is the headers'
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_signatures
    txt = open(os.path.join(ROOT, "tests", "golden", "abi_signatures.txt")).read()
    assert "hdfs_wire" not in txt and max(int(x) for x in re.findall(r"^\[(\d+)\]$", txt, flags=re.M)) == 5
    cur = dict(l.split(": ", 1) for l in txt.split("[5]\n", 1)[1].splitlines() if l and not l.startswith("#"))
    assert abi_signatures.header_prototypes() == cur


def test_other_companions_export_what_they_did(libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    for name, (node, want) in OTHERS.items():
        funcs = _c_functions(os.path.join(libdir, name))
        header = "hadoofus_" + name[len("libhadoofus_"):-len(".so")] + ".h"
        assert set(funcs) == _declared(header), name
        assert want is None or set(funcs) == want, name
        assert set(funcs.values()) == {node}, (name, funcs)
        assert not any("batch" in f for f in funcs), name
    # their headers and export maps: nothing of the batch library in them
    for f in ("include/hadoofus_wire.h", "include/hadoofus_writev.h", "include/hadoofus_md5crc.h",
              "hadoofus_amd/csrc/wire_exports.map", "hadoofus_amd/csrc/writev_exports.map",
              "hadoofus_amd/csrc/md5crc_exports.map"):
        assert "wire_batch" not in open(os.path.join(ROOT, f)).read().lower(), f


def test_companion_links_the_one_engine(libs):
    """The companion holds no copy of the engine: it needs the release
    library, found beside it, and reaches it through its public API; it does
    not need the single-write library."""
    lib, blib = libs
    dyn = subprocess.check_output(["readelf", "-d", blib], text=True)
    assert "libhadoofus_crc32c.so" in dyn and "$ORIGIN" in dyn and "libhadoofus_wire.so" not in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", blib], text=True)
    for sym in ("hdfs_crc32c_init", "hdfs_crc32c_bound_device", "hdfs_crc32c_plan_create", "hdfs_crc32c_plan_execute",
                "hdfs_crc32c_plan_destroy"):
        assert sym in und, sym
    assert "hdfs_wire_" not in und
    engine = [l.split()[-1] for l in und.splitlines() if "hdfs_crc32c_" in l]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert engine and all(s.split("@")[0] in main for s in engine)


def test_abi_version_call_and_binding_check(wb):
    assert wb.load().hdfs_wire_batch_abi_version() == wb.ABI_VERSION == 1

    class Other:
        @staticmethod
        def hdfs_wire_batch_abi_version():
            return 2
    with pytest.raises(ImportError):
        wb.check_abi(Other())


def test_last_error_texts_are_separate(wb):
    """Each of the four libraries keeps its own text, though all compile
    companion_support.h and two of them wire_layout.h: an EINVAL provoked in
    one, on a path that needs no device, leaves the other three texts alone."""
    from hadoofus_amd import md5crc, wire, writev
    wl, bl, vl, ml = wire.load(), wb.load(), writev.load(), md5crc.load()
    info, tot, vinfo = wire.LayoutInfo(), wb.Totals(), writev.LayoutInfo()
    one = wb.entries([wb.write(nbytes=1)], True)
    provoke = {
        "wire": (lambda: wl.hdfs_wire_layout(10, -1, 2, 2, 0, ctypes.byref(info)), b"negative block offset"),
        "wire_batch": (lambda: bl.hdfs_wire_batch_layout(one, 1, 7, 2, ctypes.byref(tot)),
                       b"entry 0: proto must be 1 or 2"),
        "writev": (lambda: vl.hdfs_writev_layout(None, -1, 0, ctypes.byref(vinfo)), b"null or negative fragment list"),
        "md5crc": (lambda: ml.hdfs_md5crc_md5_host(None, 5, None), b"null buffer / out"),
    }
    text = {"wire": wl.hdfs_wire_last_error, "wire_batch": bl.hdfs_wire_batch_last_error,
            "writev": vl.hdfs_writev_last_error, "md5crc": ml.hdfs_md5crc_last_error}
    for name, (call, want) in provoke.items():
        before = {k: f() for k, f in text.items()}
        assert call() == EINVAL and text[name]() == want, name
        for k, f in text.items():
            assert k == name or f() == before[k], (name, k)
    assert len({f() for f in text.values()}) == 4
    # the two that compile wire_layout.h, on the same shared code path
    assert bl.hdfs_wire_batch_layout(wb.entries([wb.write(nbytes=1, offset_in_block=-1)], True), 1, 2, 2,
                                     ctypes.byref(tot)) == EINVAL
    assert bl.hdfs_wire_batch_last_error() == b"entry 0: negative block offset"
    assert wl.hdfs_wire_last_error() == b"negative block offset"
    assert wl.hdfs_wire_layout(10, 0, 7, 2, 0, ctypes.byref(info)) == EINVAL
    assert wl.hdfs_wire_last_error() == b"proto must be 1 or 2"
    assert bl.hdfs_wire_batch_last_error() == b"entry 0: negative block offset"


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, wire, wire_batch\n"
            "assert abi._lib is None and wire._lib is None and wire_batch._lib is None\n"
            "assert callable(h.compose_wire_batch) and callable(h.wire_batch_layout)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "wire_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wire_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wire_batch", "-lhadoofus_crc32c"])
    assert exe.exists()
