"""CPU tests of the fused wire-stream companion library
(include/hadoofus_wire_fused.h): its build and ABI, the size query's packet
records against the oracle's compose_packets and against the two-pass
library's on the same arguments, the argument errors the entry points decide
without a GPU, and the CRC arithmetic of its kernel, run lane by lane on the
CPU (tests/consumer/wire_fused_selftest.cpp, built with ASan/UBSan, nothing
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
DECLARED = {"hdfs_wire_fused_abi_version", "hdfs_wire_fused_last_error", "hdfs_wire_fused_compose_packets",
            "hdfs_wire_fused_time"}


@pytest.fixture(scope="module")
def libs():
    """(release library, fused wire companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.WIRE_FUSED_LIB


@pytest.fixture(scope="module")
def wf(libs):
    from hadoofus_amd import wire_fused
    wire_fused.load()
    return wire_fused


# ---- the kernel's CRC arithmetic on the CPU ------------------------------------------
def test_wire_fused_selftest(tmp_path):
    exe = tmp_path / "wire_fused_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "wire_fused_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout


# ---- records against the oracle and the two-pass library ------------------------------
LENS = [0, 1, 287, 511, 512, 513, 65536, 65537, 3 * 65536 + 123]
DATA = np.random.default_rng(77).integers(0, 256, max(LENS), dtype=np.uint8)


def expected(oracle, n, off, seq, proto, ctype, finish):
    """The oracle's packets of the write, hdr_off moved into the stream.
    -> (wire_len, records)."""
    hdr, pkts = oracle.compose_packets(DATA[:n], off, seq, proto, ctype, finish)
    at, out = 0, []
    for p in pkts:
        out.append(dict(p, hdr_off=at))
        at += p["hdr_len"] + p["data_len"]
    assert at == len(hdr) + n
    return at, out


@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("proto", [1, 2])
@pytest.mark.parametrize("off", [0, 4321])
def test_size_query_matches_the_oracle_and_the_two_pass_library(wf, oracle, off, proto, ctype, finish):
    from hadoofus_amd import wire
    for n in LENS:
        want = expected(oracle, n, off, 11, proto, ctype, finish)
        assert wf.packet_records(n, off, 11, proto, ctype, finish) == want, n
        assert wire.packet_records(n, off, 11, proto, ctype, finish) == want, n


def test_size_query_of_a_large_write(wf):
    """1 GiB at an unaligned offset: counts in closed form, no oracle run."""
    n, off = 1 << 30, 4321
    n0 = 512 - off % 512
    npk = 1 + -(-(n - n0) // 65536) + 1
    wl, pk = wf.packet_records(n, off, 5, 2, 2, True)
    assert len(pk) == npk and wl == n + 31 * npk + 4 * (1 + -(-(n - n0) // 512))
    assert pk[2]["hdr_off"] - pk[1]["hdr_off"] == 66079 and pk[-1]["last"] == 1 and pk[-1]["data_len"] == 0
    assert pk[-1]["hdr_off"] + 31 == wl and pk[-1]["seqno"] == 5 + len(pk) - 1


# ---- argument errors that need no device ---------------------------------------------
def test_argument_errors_are_einval_without_a_device(wf):
    from hadoofus_amd.abi import OutPacket
    lib = wf.load()
    pk = (OutPacket * 4)()
    before = bytes(pk)
    npk, wl = ctypes.c_size_t(0), ctypes.c_uint64(0)
    fake = 0x1000  # never dereferenced: every call below is decided by its arguments

    def call(data=fake, n=1000, off=0, proto=2, ctype=2, wire=fake, cap=1 << 20, maxp=4):
        return lib.hdfs_wire_fused_compose_packets(data, n, off, 0, proto, ctype, 0, wire, cap, pk, maxp,
                                                   ctypes.byref(npk), ctypes.byref(wl), None)
    assert call(off=-1) == EINVAL and b"" != lib.hdfs_wire_fused_last_error()
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


def test_timing_argument_errors(wf):
    lib = wf.load()
    ms = ctypes.c_double(0)

    def call(wire=0x2000, flags=0, iters=1, out=ctypes.byref(ms), proto=2):
        return lib.hdfs_wire_fused_time(0x1000, 10, 0, proto, 2, 0, wire, 100, flags, iters, out)
    assert call(iters=0) == EINVAL and call(wire=None) == EINVAL and call(out=None) == EINVAL
    assert call(proto=7) == EINVAL
    # workgroups out of range, or a flag bit that means nothing: refused before any device is asked
    assert call(flags=wf.time_groups(wf.MAX_GROUPS + 1)) == EINVAL and b"workgroups" in lib.hdfs_wire_fused_last_error()
    assert call(flags=wf.time_groups(1 << 23)) == EINVAL and call(flags=1) == EINVAL


# ---- build and ABI ------------------------------------------------------------------
def test_build_produces_the_library(libs):
    lib, flib = libs
    assert os.path.exists(flib) and os.path.basename(flib) == "libhadoofus_wire_fused.so"
    assert os.path.dirname(lib) == os.path.dirname(flib)


def test_build_lists_sources_and_headers():
    from hadoofus_amd import build
    assert build.WIRE_FUSED_SOURCES == ["wire_fused_kernels.hip", "wire_fused.cpp"]
    assert {"wire_fused_internal.h", "wire_fused_crc.h", "wire_fused_tables.h", "wire_layout.h", "wire_internal.h",
            "companion_support.h", "crc32c_outpkt.h", "crc32c_tables.h",
            "wire_fused_exports.map"} <= set(build.WIRE_FUSED_HEADERS)
    assert "hadoofus_wire_fused.h" in build.WIRE_FUSED_PUBLIC and build.ARCH == "gfx950"
    for f in build.WIRE_FUSED_SOURCES + build.WIRE_FUSED_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    assert "Six companion libraries" in build.__doc__


def test_sources_hold_no_plan_call_and_no_polynomial():
    """The CRCs are this library's own: no compute plan anywhere in it, and the
    tables come from crc32c_tables.h, the one place the polynomials are written."""
    from hadoofus_amd import build
    for f in build.WIRE_FUSED_SOURCES + ["wire_fused_crc.h", "wire_fused_tables.h", "wire_fused_internal.h"]:
        src = open(os.path.join(build.CSRC, f)).read()
        assert "hdfs_crc32c_plan_" not in src, f
        for poly in ("82f63b78", "edb88320"):
            assert poly not in src.lower(), (f, poly)
    host = open(os.path.join(build.CSRC, "wire_fused.cpp")).read()
    assert '#include "wire_layout.h"' in host and '#include "wire_fused_tables.h"' in host
    assert "put_header_proto(uint8_t" not in host
    tables = open(os.path.join(build.CSRC, "wire_fused_tables.h")).read()
    assert all(w in tables for w in ('#include "crc32c_tables.h"', "make_slicing4", "zeros_op", "zeros_byte_tables"))
    und = subprocess.check_output(["nm", "-D", "--undefined-only", build.WIRE_FUSED_LIB], text=True)
    assert "hdfs_crc32c_plan_" not in und


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_wire_fused.h"\n'
                   "int main(void){ return HDFS_WIRE_FUSED_ABI_VERSION - 1 + (int)HDFS_WIRE_FUSED_TIME_GROUPS(0); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_companion_exports_exactly_its_header(libs):
    _, flib = libs
    assert _declared("hadoofus_wire_fused.h") == DECLARED
    funcs = _c_functions(flib)
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_wire_fused.h")).read()
    v = int(re.search(r"#define HDFS_WIRE_FUSED_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_WIRE_FUSED_{v}"}, funcs


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


def test_the_other_companions_export_what_they_did(libs):
    """Each of the five exports exactly its header's functions under its own
    version node, and none of them has a symbol of this library."""
    from hadoofus_amd import build
    for lib, header, node in ((build.MD5CRC_LIB, "hadoofus_md5crc.h", "HADOOFUS_MD5CRC_1"),
                              (build.WRITEV_LIB, "hadoofus_writev.h", "HADOOFUS_WRITEV_1"),
                              (build.WIRE_LIB, "hadoofus_wire.h", "HADOOFUS_WIRE_1"),
                              (build.WIRE_BATCH_LIB, "hadoofus_wire_batch.h", "HADOOFUS_WIRE_BATCH_1"),
                              (build.WIREV_LIB, "hadoofus_wirev.h", "HADOOFUS_WIREV_1")):
        funcs = _c_functions(lib)
        assert set(funcs) == _declared(header), (lib, set(funcs) ^ _declared(header))
        assert set(funcs.values()) == {node}, (lib, funcs)
        assert not any("wire_fused" in n for n in funcs), lib


def test_companion_links_the_one_engine_and_no_other_companion(libs):
    """It needs the release library, found beside it, and no other library of
    the project; it reaches the engine through its public API."""
    lib, flib = libs
    dyn = subprocess.check_output(["readelf", "-d", flib], text=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert [n for n in needed if "hadoofus" in n] == ["libhadoofus_crc32c.so"] and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", flib], text=True)
    for sym in ("hdfs_crc32c_init", "hdfs_crc32c_bound_device"):
        assert sym in und, sym
    engine = [l.split()[-1] for l in und.splitlines() if "hdfs_" in l]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert engine and all(s.split("@")[0] in main for s in engine)


def test_abi_version_call_and_binding_check(wf):
    assert wf.load().hdfs_wire_fused_abi_version() == wf.ABI_VERSION == 1

    class Other:
        @staticmethod
        def hdfs_wire_fused_abi_version():
            return 2
    with pytest.raises(ImportError):
        wf.check_abi(Other())


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, wire, wire_fused\n"
            "assert abi._lib is None and wire._lib is None and wire_fused._lib is None\n"
            "assert callable(h.compose_wire_fused) and callable(wire_fused.fused_time)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "wire_fused_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wire_fused_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wire_fused", "-lhadoofus_crc32c"])
    assert exe.exists()
