"""CPU tests of the wire-stream companion library (include/hadoofus_wire.h): the
library's build and ABI, the host layout and the size query's packet records
against the oracle's compose_packets on the same arguments, and the argument
errors the entry point decides without a GPU.  Everything is bit-exact."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from abi_symbols import declared as _declared, exported as _exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
DECLARED = {"hdfs_wire_abi_version", "hdfs_wire_last_error", "hdfs_wire_compose_packets", "hdfs_wire_layout",
            "hdfs_wire_frame_time"}


@pytest.fixture(scope="module")
def libs():
    """(release library, wire companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.WIRE_LIB


@pytest.fixture(scope="module")
def wr(libs):
    from hadoofus_amd import wire
    wire.load()
    return wire


# ---- layout and records against the oracle ----------------------------------------
LENS = [0, 1, 287, 511, 512, 513, 65536, 65537, 3 * 65536 + 123]
DATA = np.random.default_rng(77).integers(0, 256, max(LENS), dtype=np.uint8)


def expected(oracle, n, off, seq, proto, ctype, finish):
    """The oracle's packets of the write, hdr_off moved into the stream.
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
@pytest.mark.parametrize("off", [0, 4321])
def test_layout_and_size_query_match_the_oracle(wr, oracle, off, proto, ctype, finish):
    for n in LENS:
        want_len, want, nchunks = expected(oracle, n, off, 11, proto, ctype, finish)
        got_len, got = wr.packet_records(n, off, 11, proto, ctype, finish)
        assert (got_len, got) == (want_len, want), n
        info = wr.layout(n, off, proto, ctype, finish)
        hb = 25 if proto == 1 else 31
        assert info == {"npkts": len(want), "nchunks": nchunks, "wire_len": want_len,
                        "packet_stride": hb + (512 if ctype else 0) + 65536, "header_bytes": hb,
                        "head_bytes": min(n, 512 - off % 512) if n and off % 512 else 0}, n


def test_full_packet_strides(wr):
    assert wr.layout(1 << 20, 0, 2, 2)["packet_stride"] == 66079
    assert wr.layout(1 << 20, 0, 1, 1)["packet_stride"] == 66073
    # both odd: consecutive full packets start at every residue mod 16
    assert {(i * 66079) % 16 for i in range(16)} == set(range(16)) == {(i * 66073) % 16 for i in range(16)}


def test_size_query_of_a_large_write(wr):
    """1 GiB at an unaligned offset: counts in closed form, no oracle run."""
    n, off = 1 << 30, 4321
    n0 = 512 - off % 512
    info = wr.layout(n, off, 2, 2, True)
    body = -(-(n - n0) // 65536)
    assert info["npkts"] == 1 + body + 1 and info["nchunks"] == 1 + -(-(n - n0) // 512)
    assert info["wire_len"] == n + 31 * info["npkts"] + 4 * info["nchunks"]
    wl, pk = wr.packet_records(n, off, 5, 2, 2, True)
    assert wl == info["wire_len"] and len(pk) == info["npkts"]
    assert pk[2]["hdr_off"] - pk[1]["hdr_off"] == 66079 and pk[-1]["last"] == 1 and pk[-1]["data_len"] == 0
    assert pk[-1]["hdr_off"] + 31 == wl and pk[-1]["seqno"] == 5 + len(pk) - 1


# ---- argument errors that need no device ---------------------------------------------
def test_argument_errors_are_einval_without_a_device(wr):
    from hadoofus_amd.abi import OutPacket
    lib = wr.load()
    pk = (OutPacket * 4)()
    before = bytes(pk)
    npk, wl = ctypes.c_size_t(0), ctypes.c_uint64(0)
    fake = 0x1000  # never dereferenced: every call below is decided by its arguments

    def call(data=fake, n=1000, off=0, proto=2, ctype=2, wire=fake, cap=1 << 20, maxp=4):
        return lib.hdfs_wire_compose_packets(data, n, off, 0, proto, ctype, 0, wire, cap, pk, maxp, ctypes.byref(npk),
                                             ctypes.byref(wl), None)
    assert call(off=-1) == EINVAL and b"" != lib.hdfs_wire_last_error()
    assert call(proto=0) == EINVAL and call(proto=3) == EINVAL
    assert call(ctype=3) == EINVAL and call(ctype=-1) == EINVAL
    assert call(n=(1 << 40) + 1) == EINVAL
    assert call(data=None) == EINVAL
    # undersized outputs: EINVAL, the sizes reported, nothing written
    assert call(cap=1038) == EINVAL and (npk.value, wl.value) == (1, 31 + 8 + 1000)
    assert call(n=70000, maxp=1) == EINVAL and npk.value == 2
    assert bytes(pk) == before
    # a size query with room for the records fills them; without room it only counts
    assert call(wire=None, cap=0) == 0 and pk[0].hdr_len == 39 and pk[0].data_len == 1000
    pk[0].hdr_len = 0
    assert call(n=70000, wire=None, cap=0, maxp=1) == 0 and npk.value == 2 and pk[0].hdr_len == 0
    # an empty write without finish is no packet and no work, whatever wire is
    assert call(n=0, data=None) == 0 and (npk.value, wl.value) == (0, 0)


def test_layout_and_timing_argument_errors(wr):
    lib = wr.load()
    info = wr.LayoutInfo()
    assert lib.hdfs_wire_layout(10, 0, 2, 2, 0, None) == EINVAL
    assert lib.hdfs_wire_layout(10, -1, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wire_layout(10, 0, 5, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wire_layout(10, 0, 2, 9, 0, ctypes.byref(info)) == EINVAL
    ms = ctypes.c_double(0)
    assert lib.hdfs_wire_frame_time(0x1000, 10, 0, 2, 2, 0, 0x2000, 100, 0, 0, ctypes.byref(ms)) == EINVAL
    assert lib.hdfs_wire_frame_time(0x1000, 10, 0, 2, 2, 0, None, 100, 0, 1, ctypes.byref(ms)) == EINVAL
    assert lib.hdfs_wire_frame_time(0x1000, 10, 0, 2, 2, 0, 0x2000, 100, 0, 1, None) == EINVAL
    assert lib.hdfs_wire_frame_time(0x1000, 10, 0, 2, 2, 0, 0x2000, 100, wr.time_slices(17), 1,
                                    ctypes.byref(ms)) == EINVAL


# ---- build and ABI ------------------------------------------------------------------
def test_build_produces_the_library(libs):
    lib, wlib = libs
    assert os.path.exists(wlib) and os.path.basename(wlib) == "libhadoofus_wire.so"
    assert os.path.dirname(lib) == os.path.dirname(wlib)


def test_build_lists_sources_and_headers():
    from hadoofus_amd import build
    assert build.WIRE_SOURCES == ["wire_kernels.hip", "wire.cpp"]
    assert {"wire_internal.h", "crc32c_outpkt.h", "wire_exports.map"} <= set(build.WIRE_HEADERS)
    for headers in (build.MD5CRC_HEADERS, build.WRITEV_HEADERS, build.WIRE_HEADERS, build.WIRE_BATCH_HEADERS):
        assert "companion_support.h" in headers
    assert "hadoofus_wire.h" in build.WIRE_PUBLIC and build.ARCH == "gfx950"
    for f in build.WIRE_SOURCES + build.WIRE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    # one definition of the header-writing code, not a copy; no CRC arithmetic of its own
    for f in ("wire.cpp", "wire_kernels.hip"):
        src = open(os.path.join(build.CSRC, f)).read()
        assert '#include "crc32c_outpkt.h"' in src and "put_header_proto(uint8_t" not in src, f
        assert "crc32c_tables.h" not in src and "0x82F63B78" not in src, f


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_wire.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_wire_layout_info) - 40 + HDFS_WIRE_ABI_VERSION - 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_amd.wire import LayoutInfo as S
    names = [f for f, _ in S._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_wire.h"\n'
                   'int main(void){ printf("%zu", sizeof(hdfs_wire_layout_info));\n' +
                   "".join(f'printf(" %zu", offsetof(hdfs_wire_layout_info, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]


def test_companion_exports_exactly_its_header(libs):
    _, wlib = libs
    assert _declared("hadoofus_wire.h") == DECLARED
    funcs = {n: v for n, v in _exported(wlib).items() if n not in ("_init", "_fini")}
    # the toolchain may export a kernel's host stub; nothing else is allowed
    funcs = {n: v for n, v in funcs.items() if not (n.startswith("_ZN9hdfs_wire") and "_kernel" in n)}
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_wire.h")).read()
    v = int(re.search(r"#define HDFS_WIRE_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_WIRE_{v}"}, funcs


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


def test_companion_links_the_one_engine(libs):
    """The companion holds no copy of the engine: it needs the release
    library, found beside it, and reaches it through its public API."""
    lib, wlib = libs
    dyn = subprocess.check_output(["readelf", "-d", wlib], text=True)
    assert "libhadoofus_crc32c.so" in dyn and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", wlib], text=True)
    for sym in ("hdfs_crc32c_init", "hdfs_crc32c_bound_device", "hdfs_crc32c_plan_create", "hdfs_crc32c_plan_execute",
                "hdfs_crc32c_plan_destroy"):
        assert sym in und, sym
    engine = [l.split()[-1] for l in und.splitlines() if "hdfs_crc32c_" in l]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert engine and all(s.split("@")[0] in main for s in engine)


def test_abi_version_call_and_binding_check(wr):
    assert wr.load().hdfs_wire_abi_version() == wr.ABI_VERSION == 1

    class Other:
        @staticmethod
        def hdfs_wire_abi_version():
            return 2
    with pytest.raises(ImportError):
        wr.check_abi(Other())


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, wire\n"
            "assert abi._lib is None and wire._lib is None\n"
            "assert callable(h.compose_wire) and callable(h.wire_layout)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "wire_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wire_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wire", "-lhadoofus_crc32c"])
    assert exe.exists()
