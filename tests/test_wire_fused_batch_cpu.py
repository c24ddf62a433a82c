"""CPU tests of the fused wire-batch companion library
(include/hadoofus_wire_fused_batch.h): its build and ABI, the host layout and
the size query's packet records of whole batches against the oracle's
compose_packets of each write alone and against the two-pass batch library on
the same entries, the rejections the entry points decide without a GPU, and
the kernel's lookup (write_of), run on the CPU against a linear scan
(tests/consumer/wire_fused_batch_selftest.cpp, built with ASan/UBSan, nothing
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
DECLARED = {"hdfs_wire_fused_batch_abi_version", "hdfs_wire_fused_batch_last_error", "hdfs_wire_fused_batch_compose",
            "hdfs_wire_fused_batch_layout", "hdfs_wire_fused_batch_time"}
# the six other companions: version node and exported set, as their own tests pin them
OTHERS = {
    "md5crc": ("HADOOFUS_MD5CRC_1", None),
    "writev": ("HADOOFUS_WRITEV_1", None),
    "wire": ("HADOOFUS_WIRE_1", {"hdfs_wire_abi_version", "hdfs_wire_last_error", "hdfs_wire_compose_packets",
                                 "hdfs_wire_layout", "hdfs_wire_frame_time"}),
    "wire_batch": ("HADOOFUS_WIRE_BATCH_1", {"hdfs_wire_batch_abi_version", "hdfs_wire_batch_last_error",
                                             "hdfs_wire_batch_compose", "hdfs_wire_batch_layout",
                                             "hdfs_wire_batch_frame_time"}),
    "wirev": ("HADOOFUS_WIREV_1", None),
    "wire_fused": ("HADOOFUS_WIRE_FUSED_1", {"hdfs_wire_fused_abi_version", "hdfs_wire_fused_last_error",
                                             "hdfs_wire_fused_compose_packets", "hdfs_wire_fused_time"}),
}


@pytest.fixture(scope="module")
def libs():
    """(release library, fused wire-batch companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.WIRE_FUSED_BATCH_LIB


@pytest.fixture(scope="module")
def fb(libs):
    from hadoofus_amd import wire_fused_batch
    wire_fused_batch.load()
    return wire_fused_batch


# ---- the kernel's lookup on the CPU ----------------------------------------------------
def test_wire_fused_batch_selftest(tmp_path):
    exe = tmp_path / "wire_fused_batch_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "wire_fused_batch_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout


# ---- layout and records against the oracle and the two-pass batch library ---------------
LENS = [0, 1, 287, 511, 512, 513, 65536, 65537, 3 * 65536 + 123]  # test_wire_fused_cpu.py's
DATA = np.random.default_rng(79).integers(0, 256, max(LENS), dtype=np.uint8)


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


@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("proto", [1, 2])
def test_layout_and_size_query_match_the_oracle_and_the_batch_library(fb, oracle, proto, ctype):
    """One batch of all nine lengths at both block offsets, with finish on
    every other write and on the second empty one (so empty writes with and
    without it), each write with a sequence number of its own."""
    from hadoofus_amd import wire_batch
    writes = [fb.write(nbytes=n, offset_in_block=off, seqno=1000 * k + 11, finish=k % 2 == 1 or k == 9)
              for k, (n, off) in enumerate((n, off) for off in (0, 4321) for n in LENS)]
    assert {(w["nbytes"], w["finish"]) for w in writes} >= {(0, True), (0, False)}
    want = [expected(oracle, w["nbytes"], w["offset_in_block"], w["seqno"], proto, ctype, w["finish"])
            for w in writes]
    got = fb.packet_records(writes, proto, ctype)
    assert len(got) == len(want)
    first = 0
    outs, tot = fb.layout(writes, proto, ctype)
    for k, (g, x, o) in enumerate(zip(got, want, outs)):
        assert g[0] == x[0] and len(g[1]) == len(x[1]), k
        for a, b in zip(g[1], x[1]):  # field by field
            assert set(a) == set(b) and all(a[f] == b[f] for f in b), (k, a, b)
        assert o == {"wire_len": x[0], "npkts": len(x[1]), "first_pkt": first}, k
        first += len(x[1])
    assert tot == {"npkts": first, "nchunks": sum(x[2] for x in want), "wire_bytes": sum(x[0] for x in want),
                   "table_entries": sum(1 for x in want if x[1])}
    assert tot["table_entries"] == len(writes) - 1  # the one empty write without finish
    # the two-pass batch library, same entries
    assert wire_batch.layout(writes, proto, ctype) == (outs, tot)
    assert wire_batch.packet_records(writes, proto, ctype) == got


def test_empty_writes_anywhere_and_the_empty_batch(fb):
    e = fb.write(nbytes=0)
    f = fb.write(nbytes=0, finish=True, seqno=7)
    d = fb.write(nbytes=513, seqno=3)
    outs, tot = fb.layout([e, f, e, d, e])
    assert [o["npkts"] for o in outs] == [0, 1, 0, 1, 0] and [o["first_pkt"] for o in outs] == [0, 0, 1, 1, 2]
    assert outs[1]["wire_len"] == 31 and tot["table_entries"] == 2 and tot["npkts"] == 2
    got = fb.packet_records([e, f, e, d, e])
    assert got[0] == (0, []) and got[1][1][0]["last"] == 1 and got[1][1][0]["seqno"] == 7
    assert got[3][1][0]["data_len"] == 513 and got[3][1][0]["hdr_off"] == 0
    assert fb.layout([]) == ([], {"npkts": 0, "nchunks": 0, "wire_bytes": 0, "table_entries": 0})
    assert fb.packet_records([]) == []


def test_size_query_of_large_writes(fb):
    """64 writes of 128 MiB, counts in closed form."""
    n = 128 << 20
    outs, tot = fb.layout([fb.write(nbytes=n, offset_in_block=4321 if k % 2 else 0, finish=True) for k in range(64)])
    assert [o["npkts"] for o in outs[:2]] == [2049, 2050] and outs[2]["first_pkt"] == 4099
    assert tot["npkts"] == 32 * (2049 + 2050) and tot["table_entries"] == 64
    assert tot["wire_bytes"] == 64 * n + 31 * tot["npkts"] + 4 * tot["nchunks"]


def test_packet_limit_of_the_batch_is_judged_in_closed_form(fb):
    """(2^31 - 1) / 4 packets at most: 33 writes of 1 TiB (2^24 packets each)
    are refused at once, before any write's packets are walked."""
    lib, tot = fb.load(), fb.Totals()
    arr = fb.entries([fb.write(nbytes=1 << 40)] * 33, True)
    assert lib.hdfs_wire_fused_batch_layout(arr, 33, 2, 2, ctypes.byref(tot)) == EINVAL
    assert b"packets in the batch" in lib.hdfs_wire_fused_batch_last_error()


# ---- rejections that need no device ---------------------------------------------
def test_rejections_without_a_device(fb):
    from hadoofus_amd.abi import OutPacket
    lib = fb.load()
    fake = 0x1000  # never dereferenced: every call below is decided by its arguments
    pk = (OutPacket * 8)()
    before = bytes(pk)
    npk = ctypes.c_size_t(99)

    def call(writes, proto=2, ctype=2, maxp=8, query=False, n=None, out=pk):
        arr = fb.entries(writes, query)
        rc = lib.hdfs_wire_fused_batch_compose(arr, len(writes) if n is None else n, proto, ctype, out, maxp,
                                               ctypes.byref(npk), None)
        return rc, arr, lib.hdfs_wire_fused_batch_last_error().decode()

    def w(**kw):
        return fb.write(**dict(dict(dptr=fake, nbytes=1000, wire_ptr=fake + (1 << 20), wire_cap=1 << 20), **kw))
    good = [w(), w(nbytes=70000), w(nbytes=0, finish=True)]
    sizes = [(1039, 1, 0), (70000 + 2 * 31 + 4 * 137, 2, 1), (31, 1, 3)]
    # arguments of the whole batch
    for kw in (dict(proto=0), dict(proto=3), dict(ctype=3), dict(ctype=-1)):
        rc, arr, err = call(good, **kw)
        assert rc == EINVAL and "entry 0" in err and npk.value == 0, (kw, err)
    rc, _, err = call(good, n=fb.MAX_WRITES + 1)
    assert rc == EINVAL and "65536" in err and npk.value == 0
    # arguments of one entry: the text names it
    for bad in (w(offset_in_block=-1), w(nbytes=(1 << 40) + 1)):
        rc, _, err = call([good[0], good[1], bad])
        assert rc == EINVAL and "entry 2" in err, err
    rc, arr, err = call([good[0], w(dptr=None, nbytes=5)])
    assert rc == EINVAL and "entry 1" in err and (arr[1].wire_len, arr[1].npkts, arr[1].first_pkt) == (40, 1, 1)
    # undersized outputs: EINVAL, the sizes reported, nothing written
    rc, arr, err = call([good[0], w(nbytes=70000, wire_cap=sizes[1][0] - 1), good[2]])
    assert rc == EINVAL and "entry 1" in err, err
    assert npk.value == 4 and [(e.wire_len, e.npkts, e.first_pkt) for e in arr[:3]] == sizes
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


def test_layout_and_timing_argument_errors(fb):
    lib = fb.load()
    one = [fb.write(dptr=0x1000, nbytes=10, wire_ptr=0x2000, wire_cap=100)]
    arr = fb.entries(one)
    assert lib.hdfs_wire_fused_batch_layout(arr, 1, 2, 2, None) == EINVAL
    tot = fb.Totals()
    assert lib.hdfs_wire_fused_batch_layout(arr, 1, 5, 2, ctypes.byref(tot)) == EINVAL
    assert lib.hdfs_wire_fused_batch_layout(arr, 1, 2, 9, ctypes.byref(tot)) == EINVAL
    assert lib.hdfs_wire_fused_batch_layout(None, 1, 2, 2, ctypes.byref(tot)) == EINVAL
    ms = ctypes.c_double(0)

    def call(flags=0, iters=1, out=ctypes.byref(ms), proto=2, query=False):
        a = fb.entries(one, query)
        rc = lib.hdfs_wire_fused_batch_time(a, 1, proto, 2, flags, iters, out)
        return rc, (a[0].wire_len, a[0].npkts, a[0].first_pkt), lib.hdfs_wire_fused_batch_last_error()
    # every one decided before a device is asked (0x1000 is no device memory: going on would say so)
    for kw in (dict(iters=0), dict(out=None), dict(query=True)):
        rc, outs, err = call(**kw)
        assert rc == EINVAL and outs == (45, 1, 0) and b"device" not in err, (kw, err)
    assert call(proto=7)[0] == EINVAL
    # workgroups out of range, or a flag bit that means nothing
    for flags in (fb.time_groups(fb.MAX_GROUPS + 1), fb.time_groups(1 << 23), 1, fb.time_groups(2) | 4):
        rc, outs, err = call(flags=flags)
        assert rc == EINVAL and b"workgroups" in err and outs == (45, 1, 0), (flags, err)


# ---- build and ABI ------------------------------------------------------------------
def test_build_produces_the_library(libs):
    lib, blib = libs
    assert os.path.exists(blib) and os.path.basename(blib) == "libhadoofus_wire_fused_batch.so"
    assert os.path.dirname(lib) == os.path.dirname(blib)


def test_build_lists_sources_and_headers():
    from hadoofus_amd import build
    assert build.WIRE_FUSED_BATCH_SOURCES == ["wire_fused_batch_kernels.hip", "wire_fused_batch.cpp"]
    assert {"wire_fused_batch_internal.h", "wire_fused_batch_lookup.h", "wire_fused_round.h", "wire_fused_crc.h",
            "wire_fused_tables.h", "wire_layout.h", "wire_internal.h", "companion_support.h", "crc32c_outpkt.h",
            "crc32c_tables.h", "wire_fused_batch_exports.map"} <= set(build.WIRE_FUSED_BATCH_HEADERS)
    assert "hadoofus_wire_fused_batch.h" in build.WIRE_FUSED_BATCH_PUBLIC and build.ARCH == "gfx950"
    for f in build.WIRE_FUSED_BATCH_SOURCES + build.WIRE_FUSED_BATCH_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    # the fused library keeps its sources and gains the shared round
    assert build.WIRE_FUSED_SOURCES == ["wire_fused_kernels.hip", "wire_fused.cpp"]
    assert "wire_fused_round.h" in build.WIRE_FUSED_HEADERS
    assert "Six companion libraries" in build.__doc__ and "libhadoofus_wire_fused_batch.so" in build.__doc__


def test_one_definition_of_the_round_and_of_the_lookup():
    """The round's device helpers live in wire_fused_round.h and the lookup in
    wire_fused_batch_lookup.h; both kernel files include the round and hold no
    copy of it."""
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    code = lambda f: "\n".join(l for l in read(f).splitlines() if not l.lstrip().startswith("//"))  # noqa: E731
    rnd = read("wire_fused_round.h")
    helpers = ["range_of(", "load16(", "store16(", "store32(", "load8(", "store8(", "fold8(", "transpose(",
               "unit_of(", "load_round(", "store_round(", "crc_round(", "header(", "ragged_chunk(", "fill_image("]
    for name in helpers:
        assert len(re.findall(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), rnd)) == 1, name
    assert rnd.count("struct Unit {") == 1
    for f in ("wire_fused_kernels.hip", "wire_fused_batch_kernels.hip"):
        src = code(f)
        assert '#include "wire_fused_round.h"' in src, f
        assert "struct Unit" not in src and "__builtin_amdgcn_raw_buffer" not in src and "permlane" not in src, f
        for name in helpers:
            assert not re.search(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), src), (f, name)
    look = code("wire_fused_batch_lookup.h")  # compiles without HIP: the selftest is plain C++
    assert look.count("uint32_t write_of(") == 1 and "hip" not in look.replace("__HIPCC__", "").lower()
    kern = code("wire_fused_batch_kernels.hip")
    assert '#include "wire_fused_batch_lookup.h"' in kern and kern.count("write_of(pk0, nw, g, k)") == 1
    assert "address_space(4)" in kern and "atomic" not in kern.lower()


def test_sources_hold_no_plan_call_and_no_polynomial():
    """The CRCs are this library's own: no compute plan anywhere in it, and the
    tables come from crc32c_tables.h, the one place the polynomials are
    written; the layout and the headers are the shared code's."""
    from hadoofus_amd import build
    for f in build.WIRE_FUSED_BATCH_SOURCES + ["wire_fused_batch_internal.h", "wire_fused_batch_lookup.h",
                                               "wire_fused_round.h", "wire_fused_crc.h", "wire_fused_tables.h"]:
        src = open(os.path.join(build.CSRC, f)).read()
        assert "hdfs_crc32c_plan_" not in src, f
        assert "put_header_proto(uint8_t" not in src and "put_out_header(uint8_t" not in src, f
        for poly in ("82f63b78", "edb88320"):
            assert poly not in src.lower(), (f, poly)
    host = open(os.path.join(build.CSRC, "wire_fused_batch.cpp")).read()
    assert '#include "wire_layout.h"' in host and '#include "wire_fused_tables.h"' in host
    # the batch front end, shared with the two-pass batch library, walks the writes with them
    front = open(os.path.join(build.CSRC, "wire_batch_layout.h")).read()
    assert '#include "wire_batch_layout.h"' in host and '#include "wire_layout.h"' in front
    assert "build_layout(" in front and "fill_records(" in front and "plan_out_packets(" not in host + front
    assert not re.search(r"^\w[\w ]*\b(build_layout|fill_records)\(", host + front, flags=re.M)  # and defines neither
    assert "put_header_proto" not in host and "hadoofus_wire_batch.h" not in host
    hdr = open(os.path.join(ROOT, "include", "hadoofus_wire_fused_batch.h")).read()
    assert '#include "hadoofus_wire_batch.h"' not in hdr and '#include "hadoofus_wire_fused.h"' not in hdr
    und = subprocess.check_output(["nm", "-D", "--undefined-only", build.WIRE_FUSED_BATCH_LIB], text=True)
    assert "hdfs_crc32c_plan_" not in und


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_wire_fused_batch.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_wire_fused_batch_write) - 80 + "
                   "(int)sizeof(hdfs_wire_fused_batch_totals) - 32 + HDFS_WIRE_FUSED_BATCH_ABI_VERSION - 1 + "
                   "(int)HDFS_WIRE_FUSED_BATCH_TIME_GROUPS(0) + HDFS_WIRE_FUSED_BATCH_MAX_WRITES - 65536; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


@pytest.mark.parametrize("cname,pyname", [("hdfs_wire_fused_batch_write", "BatchWrite"),
                                          ("hdfs_wire_fused_batch_totals", "Totals")])
def test_struct_layout_matches_c_and_the_batch_library(tmp_path, cname, pyname):
    from hadoofus_amd import wire_batch, wire_fused_batch
    S, T = getattr(wire_fused_batch, pyname), getattr(wire_batch, pyname)
    names = [f for f, _ in S._fields_]
    assert names == [f for f, _ in T._fields_]  # the same fields in the same order
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_wire_fused_batch.h"\n'
                   f'int main(void){{ printf("%zu", sizeof({cname}));\n' +
                   "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    assert got == [ctypes.sizeof(T)] + [getattr(T, n).offset for n in names]
    # pinned: the ABI of version 1
    want = {"BatchWrite": [80, 0, 8, 16, 24, 32, 36, 40, 48, 56, 64, 72], "Totals": [32, 0, 8, 16, 24]}[pyname]
    assert got == want


def test_companion_exports_exactly_its_header(libs):
    _, blib = libs
    assert _declared("hadoofus_wire_fused_batch.h") == DECLARED
    funcs = _c_functions(blib)
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_wire_fused_batch.h")).read()
    v = int(re.search(r"#define HDFS_WIRE_FUSED_BATCH_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_WIRE_FUSED_BATCH_{v}"}, funcs


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


def test_the_six_other_companions_export_what_they_did(libs):
    """Each exports exactly its header's functions under its own version node,
    none of them has a symbol of this library, and their headers and export
    maps do not speak of it."""
    lib, _ = libs
    libdir = os.path.dirname(lib)
    for name, (node, want) in OTHERS.items():
        funcs = _c_functions(os.path.join(libdir, f"libhadoofus_{name}.so"))
        assert set(funcs) == _declared(f"hadoofus_{name}.h"), (name, set(funcs) ^ _declared(f"hadoofus_{name}.h"))
        assert want is None or set(funcs) == want, name
        assert set(funcs.values()) == {node}, (name, funcs)
        assert not any("fused_batch" in f for f in funcs), name
        for f in (f"include/hadoofus_{name}.h", f"hadoofus_amd/csrc/{name}_exports.map"):
            assert "fused_batch" not in open(os.path.join(ROOT, f)).read().lower(), f


def test_companion_links_the_one_engine_and_no_other_companion(libs):
    """It needs the release library, found beside it, and no other library of
    the project; it reaches the engine through three calls of its public API."""
    lib, blib = libs
    dyn = subprocess.check_output(["readelf", "-d", blib], text=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert [n for n in needed if "hadoofus" in n] == ["libhadoofus_crc32c.so"] and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", blib], text=True)
    engine = sorted(l.split()[-1].split("@")[0] for l in und.splitlines() if "hdfs_" in l)
    assert engine == ["hdfs_crc32c_bound_device", "hdfs_crc32c_init", "hdfs_crc32c_last_error"]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert all(s in main for s in engine)


def test_abi_version_call_and_binding_check(fb):
    assert fb.load().hdfs_wire_fused_batch_abi_version() == fb.ABI_VERSION == 1
    assert fb.MAX_GROUPS == 1024 and fb.time_groups(3) == 3 << 8

    class Other:
        @staticmethod
        def hdfs_wire_fused_batch_abi_version():
            return 2
    with pytest.raises(ImportError):
        fb.check_abi(Other())


def test_last_error_text_is_its_own(fb):
    """An EINVAL provoked here leaves the two-pass batch library's and the
    fused library's texts alone, and the other way round."""
    from hadoofus_amd import wire_batch, wire_fused
    bl, fl, lib = wire_batch.load(), wire_fused.load(), fb.load()
    tot, btot = fb.Totals(), wire_batch.Totals()
    assert bl.hdfs_wire_batch_layout(wire_batch.entries([wire_batch.write(nbytes=1)], True), 1, 7, 2,
                                     ctypes.byref(btot)) == EINVAL
    before = (bl.hdfs_wire_batch_last_error(), fl.hdfs_wire_fused_last_error())
    assert lib.hdfs_wire_fused_batch_layout(fb.entries([fb.write(nbytes=1, offset_in_block=-1)], True), 1, 2, 2,
                                            ctypes.byref(tot)) == EINVAL
    assert lib.hdfs_wire_fused_batch_last_error() == b"entry 0: negative block offset"
    assert (bl.hdfs_wire_batch_last_error(), fl.hdfs_wire_fused_last_error()) == before
    assert before[0] == b"entry 0: proto must be 1 or 2"


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, wire_fused, wire_fused_batch\n"
            "assert abi._lib is None and wire_fused._lib is None and wire_fused_batch._lib is None\n"
            "assert callable(h.compose_wire_fused_batch) and callable(wire_fused_batch.fused_batch_time)\n"
            "assert callable(wire_fused_batch.layout) and callable(wire_fused_batch.compose)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "wire_fused_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wire_fused_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wire_fused_batch", "-lhadoofus_crc32c"])
    assert exe.exists()
