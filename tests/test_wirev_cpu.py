"""CPU tests of the gather-wire companion library (include/hadoofus_wirev.h):
the library's build and ABI, the host layout and the size query's packet
records against the oracle's compose_packets of the fragments' concatenation,
the gather counts against hdfs_writev_layout's, and the argument errors the
entry point decides without a GPU.  Everything is bit-exact."""
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
DECLARED = {"hdfs_wirev_abi_version", "hdfs_wirev_last_error", "hdfs_wirev_compose_packets", "hdfs_wirev_layout",
            "hdfs_wirev_frame_time"}


@pytest.fixture(scope="module")
def libs():
    """(release library, gather-wire companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.WIREV_LIB


@pytest.fixture(scope="module")
def wv(libs):
    from hadoofus_amd import wirev
    wirev.load()
    return wirev


# ---- layout and records against the oracle ----------------------------------------
LENS = [0, 1, 287, 511, 512, 513, 65536, 65537, 3 * 65536 + 123]
DATA = np.random.default_rng(78).integers(0, 256, max(LENS), dtype=np.uint8)
SPLITS = [1, 2, 7, 300]


def split(n, k, seed):
    """n bytes cut into k fragment lengths at random places (empty fragments
    occur: cuts repeat, and k may exceed n)."""
    cuts = np.sort(np.random.default_rng(seed).integers(0, n + 1, k - 1))
    return [int(x) for x in np.diff(np.concatenate(([0], cuts, [n])))]


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


def frags_under_packets(lens, recs):
    """Most non-empty fragments under one packet's data, from the definition."""
    ends = np.cumsum(lens)
    starts = ends - np.asarray(lens)
    most = 0
    for p in recs:
        a, b = p["data_off"], p["data_off"] + p["data_len"]
        if b > a:
            most = max(most, int(np.count_nonzero((starts < b) & (ends > a) & (ends > starts))))
    return most


@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("proto", [1, 2])
@pytest.mark.parametrize("off", [0, 4321])
def test_layout_and_size_query_match_the_oracle(wv, oracle, off, proto, ctype, finish):
    from hadoofus_amd import writev
    for n in LENS:
        want_len, want, nchunks = expected(oracle, n, off, 11, proto, ctype, finish)
        hb = 25 if proto == 1 else 31
        for k in SPLITS:
            lens = split(n, k, 1000 * k + n % 997)
            assert len(lens) == k and sum(lens) == n
            got_len, got = wv.packet_records(lens, off, 11, proto, ctype, finish)
            assert (got_len, got) == (want_len, want), (n, k)
            info = wv.layout(lens, off, proto, ctype, finish)
            g = writev.layout(lens, off)
            assert info == {"npkts": len(want), "nchunks": nchunks, "wire_len": want_len,
                            "packet_stride": hb + (512 if ctype else 0) + 65536, "header_bytes": hb,
                            "head_bytes": min(n, 512 - off % 512) if n and off % 512 else 0,
                            "nsegments": g["nsegments"], "seg_chunks": g["seg_chunks"], "ngathered": g["ngathered"],
                            "npieces": g["npieces"], "max_pieces": g["max_pieces"],
                            "nfrags": sum(1 for x in lens if x),
                            "max_frags_per_packet": frags_under_packets(lens, want)}, (n, k)
            assert g["nchunks"] == nchunks and g["total"] == n


def test_gather_counts_of_known_splits(wv):
    """Counts worked out by hand, not taken from the other library."""
    # 2 x 65 536 + 700 at 4321: chunks are 287, then the 512-B grid; a cut at 287 + 512 is on the grid
    n = 2 * 65536 + 700
    one = wv.layout([n], 4321)
    assert (one["nchunks"], one["nsegments"], one["seg_chunks"], one["ngathered"], one["npieces"]) == \
        (1 + 257, 1, 257, 1, 1) and (one["nfrags"], one["max_frags_per_packet"], one["npkts"]) == (1, 1, 4)
    two = wv.layout([287 + 512, n - 287 - 512], 4321)
    # the first fragment holds chunk 0 and one grid chunk: no run of 8, both gathered whole
    assert (two["nsegments"], two["seg_chunks"], two["ngathered"], two["npieces"], two["max_pieces"]) == \
        (1, 256, 2, 2, 1) and two["max_frags_per_packet"] == 2
    cut = wv.layout([287 + 513, n - 287 - 513], 4321)
    # one byte further: chunk 2 is cut after its first byte, two pieces
    assert (cut["nsegments"], cut["seg_chunks"], cut["ngathered"], cut["npieces"], cut["max_pieces"]) == \
        (1, 255, 3, 4, 2)
    tiny = wv.layout([1] * 700, 0, 2, 2, True)
    assert (tiny["nsegments"], tiny["ngathered"], tiny["npieces"], tiny["max_pieces"]) == (0, 2, 700, 512)
    assert (tiny["nfrags"], tiny["max_frags_per_packet"], tiny["npkts"]) == (700, 700, 2)
    # empty fragments are no table entries and no pieces
    holes = wv.layout([0, 1000, 0, 0, 24, 0], 0)
    assert (holes["nfrags"], holes["max_frags_per_packet"], holes["npieces"], holes["ngathered"]) == (2, 2, 3, 2)


def test_size_query_of_a_large_write(wv):
    """1 GiB in 64 fragments at an unaligned offset: counts in closed form, no oracle run."""
    n, off = 1 << 30, 4321
    n0 = 512 - off % 512
    lens = [n // 64] * 64
    info = wv.layout(lens, off, 2, 2, True)
    body = -(-(n - n0) // 65536)
    assert info["npkts"] == 1 + body + 1 and info["nchunks"] == 1 + -(-(n - n0) // 512)
    assert info["wire_len"] == n + 31 * info["npkts"] + 4 * info["nchunks"]
    # every fragment starts 287 bytes past the grid: 63 cut chunks and the first one are gathered
    assert (info["nfrags"], info["nsegments"], info["ngathered"], info["npieces"]) == (64, 64, 64, 1 + 2 * 63)
    assert info["max_frags_per_packet"] == 2
    wl, pk = wv.packet_records(lens, off, 5, 2, 2, True)
    assert wl == info["wire_len"] and len(pk) == info["npkts"]
    assert pk[2]["hdr_off"] - pk[1]["hdr_off"] == 66079 and pk[-1]["last"] == 1 and pk[-1]["data_len"] == 0
    assert pk[-1]["hdr_off"] + 31 == wl and pk[-1]["seqno"] == 5 + len(pk) - 1


# ---- argument errors that need no device ---------------------------------------------
def test_argument_errors_are_einval_without_a_device(wv):
    from hadoofus_amd.abi import IoVec, OutPacket
    lib = wv.load()
    pk = (OutPacket * 4)()
    before = bytes(pk)
    npk, wl = ctypes.c_size_t(0), ctypes.c_uint64(0)
    fake = 0x1000  # never dereferenced: every call below is decided by its arguments

    def call(lens=(600, 400), bases=None, cnt=None, off=0, proto=2, ctype=2, wire=fake, cap=1 << 20, maxp=4,
             null_list=False):
        bases = bases if bases is not None else [fake + 0x10000 * (i + 1) for i in range(len(lens))]
        vec = (IoVec * max(1, len(lens)))(*[IoVec(b, n) for b, n in zip(bases, lens)])
        return lib.hdfs_wirev_compose_packets(None if null_list else vec, len(lens) if cnt is None else cnt, off, 0,
                                              proto, ctype, 0, wire, cap, pk, maxp, ctypes.byref(npk),
                                              ctypes.byref(wl), None)
    assert call(off=-1) == EINVAL and b"" != lib.hdfs_wirev_last_error()
    assert call(proto=0) == EINVAL and call(proto=3) == EINVAL
    assert call(ctype=3) == EINVAL and call(ctype=-1) == EINVAL
    assert call(cnt=-1) == EINVAL and call(null_list=True) == EINVAL
    assert call(lens=(1 << 39, (1 << 39) + 1)) == EINVAL and b"1 TiB" in lib.hdfs_wirev_last_error()
    assert call(lens=(0, 1 << 62, 1)) == EINVAL and b"fragment 2" in lib.hdfs_wirev_last_error()
    assert call(bases=[fake, None]) == EINVAL and b"fragment 1" in lib.hdfs_wirev_last_error()
    # undersized outputs: EINVAL, the sizes reported, nothing written
    assert call(cap=1038) == EINVAL and (npk.value, wl.value) == (1, 31 + 8 + 1000)
    assert call(lens=(30000, 0, 40000), maxp=1) == EINVAL and npk.value == 2
    assert bytes(pk) == before
    # a size query with room for the records fills them and reads no base; without room it only counts
    assert call(bases=[None, None], wire=None, cap=0) == 0 and pk[0].hdr_len == 39 and pk[0].data_len == 1000
    pk[0].hdr_len = 0
    assert call(lens=(30000, 40000), wire=None, cap=0, maxp=1) == 0 and npk.value == 2 and pk[0].hdr_len == 0
    # an empty write without finish is no packet and no work, whatever wire is
    assert call(lens=(0, 0), bases=[None, None]) == 0 and (npk.value, wl.value) == (0, 0)
    assert call(lens=()) == 0 and (npk.value, wl.value) == (0, 0)


def test_layout_and_timing_argument_errors(wv):
    from hadoofus_amd.abi import IoVec
    lib = wv.load()
    info = wv.LayoutInfo()
    lens = (ctypes.c_uint64 * 2)(10, 20)
    assert lib.hdfs_wirev_layout(lens, 2, 0, 2, 2, 0, None) == EINVAL
    assert lib.hdfs_wirev_layout(None, 2, 0, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_layout(lens, -1, 0, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_layout(lens, 2, -1, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_layout(lens, 2, 0, 5, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_layout(lens, 2, 0, 2, 9, 0, ctypes.byref(info)) == EINVAL
    big = (ctypes.c_uint64 * 2)(1 << 40, 1)
    assert lib.hdfs_wirev_layout(big, 2, 0, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_layout(None, 0, 0, 2, 2, 1, ctypes.byref(info)) == 0 and info.npkts == 1 and info.nfrags == 0
    ms = ctypes.c_double(0)
    vec = (IoVec * 1)(IoVec(0x1000, 10))
    assert lib.hdfs_wirev_frame_time(vec, 1, 0, 2, 2, 0, 0x2000, 100, 0, 0, ctypes.byref(ms)) == EINVAL
    assert lib.hdfs_wirev_frame_time(vec, 1, 0, 2, 2, 0, None, 100, 0, 1, ctypes.byref(ms)) == EINVAL
    assert lib.hdfs_wirev_frame_time(vec, 1, 0, 2, 2, 0, 0x2000, 100, 0, 1, None) == EINVAL
    assert lib.hdfs_wirev_frame_time(vec, 1, 0, 2, 2, 0, 0x2000, 100, wv.time_slices(17), 1,
                                     ctypes.byref(ms)) == EINVAL


# ---- build and ABI ------------------------------------------------------------------
def test_build_produces_the_library(libs):
    lib, wlib = libs
    assert os.path.exists(wlib) and os.path.basename(wlib) == "libhadoofus_wirev.so"
    assert os.path.dirname(lib) == os.path.dirname(wlib)


def test_build_lists_sources_and_headers():
    from hadoofus_amd import build
    assert build.WIREV_SOURCES == ["wirev_kernels.hip", "writev_kernels.hip", "wirev.cpp"]
    assert {"wirev_internal.h", "wire_internal.h", "wire_frame.h", "wire_layout.h", "writev_internal.h",
            "writev_layout.h", "companion_support.h", "crc32c_outpkt.h", "wirev_exports.map"} <= set(build.WIREV_HEADERS)
    assert "writev_layout.h" in build.WRITEV_HEADERS
    assert "hadoofus_wirev.h" in build.WIREV_PUBLIC and build.ARCH == "gfx950"
    for f in build.WIREV_SOURCES + build.WIREV_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    for f in build.WIREV_PUBLIC:
        assert os.path.exists(os.path.join(build.INCLUDE, f)), f


def test_one_definition_of_the_gather_layout_and_the_frame_code():
    """writev.cpp and wirev.cpp both take the gather layout from
    writev_layout.h and hold no copy; the new library's own files hold no CRC
    arithmetic (gather_chunks_kernel's, in writev_kernels.hip, is its only
    one), no copy of the framing body and none of the header-writing code."""
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    lay = read("writev_layout.h")
    moved = ["int build_layout(", "hipError_t upload_slicing_tables(", "int gather_plan(", "int enqueue_gather("]
    for name in moved:
        assert lay.count("inline " + name) == 1, name
    for name in ("struct Run {", "struct Layout {", "constexpr uint32_t kMinSegChunks"):
        assert lay.count(name) == 1, name
    for f in ("writev.cpp", "wirev.cpp"):
        src = read(f)
        assert '#include "writev_layout.h"' in src, f
        for name in moved:
            assert not re.search(r"^\s*(inline |static )?" + re.escape(name), src, flags=re.M), (f, name)
        for name in ("struct Run", "struct Layout", "constexpr uint32_t kMinSegChunks", "make_slicing4",
                     "launch_gather_chunks("):
            assert name not in src, (f, name)
        assert "gather_plan(" in src and "enqueue_gather(" in src and "upload_slicing_tables(" in src, f
    # the gather's build_layout: one definition in the whole source directory
    defs = [f for f in sorted(os.listdir(build.CSRC))
            if re.search(r"int build_layout\(const uint64_t \*lens", open(os.path.join(build.CSRC, f)).read())]
    assert defs == ["writev_layout.h"]
    # the frame kernel: wire_frame.h's region copy and its CRC-and-header part, no copy of either
    frame, kern, cpp = read("wire_frame.h"), read("wirev_kernels.hip"), read("wirev.cpp")
    assert len(re.findall(r"WIRE_DEV [\w:<> ]*\bframe_crcs_and_header\(", frame)) == 1
    assert frame.count("frame_crcs_and_header<SC1>(") == 1  # frame_packet's call
    assert '#include "wire_frame.h"' in kern and "frame::copy_region<SC1>(" in kern
    assert "frame::frame_crcs_and_header<SC1>(" in kern and "packet_at(" in kern
    for name in ("cut16(", "shift_window(", "void issue(", "copy_header(", "put_out_header(", "put_header_proto("):
        assert name not in kern and name not in cpp, name
    code = re.sub(r"//[^\n]*", "", kern)  # (the comments say what the kernel does not do)
    assert "alignbyte" not in code and "global_store" not in code and "atomic" not in code.lower()
    assert "address_space(4)" in kern  # the table is read with scalar loads
    for f in ("wirev.cpp", "wirev_kernels.hip", "wirev_internal.h"):
        src = read(f)
        assert "0x82F63B78" not in src and "0xEDB88320" not in src and "crc32c_tables.h" not in src, f
        assert "hipPointerGetAttributes" not in src and "hipMemGetAddressRange" not in src, f
    assert '#include "wire_layout.h"' in cpp and '#include "companion_support.h"' in cpp
    assert "plan_out_packets(" not in cpp and "timed_frame_run(" in cpp and "fill_records(" in cpp
    assert "hadoofus_wire.h" not in cpp and "hadoofus_wire_batch.h" not in cpp and "hadoofus_md5crc.h" not in cpp


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_wirev.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_wirev_layout_info) - 88 + HDFS_WIREV_ABI_VERSION - 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_amd.wirev import LayoutInfo as S
    names = [f for f, _ in S._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_wirev.h"\n'
                   'int main(void){ printf("%zu", sizeof(hdfs_wirev_layout_info));\n' +
                   "".join(f'printf(" %zu", offsetof(hdfs_wirev_layout_info, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    # pinned: the ABI of version 1
    assert got == [88, 0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 80, 84]
    assert names == ["npkts", "nchunks", "wire_len", "nsegments", "seg_chunks", "ngathered", "npieces", "nfrags",
                     "packet_stride", "header_bytes", "head_bytes", "max_pieces", "max_frags_per_packet", "reserved"]


def test_companion_exports_exactly_its_header(libs):
    _, wlib = libs
    assert _declared("hadoofus_wirev.h") == DECLARED
    funcs = {n: v for n, v in _exported(wlib).items() if n not in ("_init", "_fini")}
    # the toolchain may export a kernel's host stub; nothing else is allowed
    funcs = {n: v for n, v in funcs.items()
             if not (n.startswith(("_ZN10hdfs_wirev", "_ZN11hdfs_writev")) and "_kernel" in n)}
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_wirev.h")).read()
    v = int(re.search(r"#define HDFS_WIREV_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_WIREV_{v}"}, funcs


def test_main_library_and_the_other_companions_are_unchanged(libs):
    lib, _ = libs
    from hadoofus_amd import build
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert "hdfs_wirev" not in out and "HADOOFUS_WIREV" not in out
    main_hdr = open(os.path.join(ROOT, "include", "hadoofus_crc32c.h")).read()
    assert "hdfs_wirev" not in main_hdr and "#define HDFS_CRC32C_ABI_VERSION 5" in main_hdr
    # the committed signature list still ends at version 5 and is the headers'
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_signatures
    txt = open(os.path.join(ROOT, "tests", "golden", "abi_signatures.txt")).read()
    assert "hdfs_wirev" not in txt and max(int(x) for x in re.findall(r"^\[(\d+)\]$", txt, flags=re.M)) == 5
    cur = dict(l.split(": ", 1) for l in txt.split("[5]\n", 1)[1].splitlines() if l and not l.startswith("#"))
    assert abi_signatures.header_prototypes() == cur
    # the four other companions export what their headers declare, each under its own node
    for other, hdr, node in ((build.MD5CRC_LIB, "hadoofus_md5crc.h", "HADOOFUS_MD5CRC_1"),
                             (build.WRITEV_LIB, "hadoofus_writev.h", "HADOOFUS_WRITEV_1"),
                             (build.WIRE_LIB, "hadoofus_wire.h", "HADOOFUS_WIRE_1"),
                             (build.WIRE_BATCH_LIB, "hadoofus_wire_batch.h", "HADOOFUS_WIRE_BATCH_1")):
        funcs = {n: v for n, v in _exported(other).items() if n not in ("_init", "_fini") and "_kernel" not in n}
        assert set(funcs) == _declared(hdr) and set(funcs.values()) == {node}, other
        assert not any("wirev" in n for n in funcs), other


def test_companion_links_the_one_engine_and_no_other_companion(libs):
    """The companion holds no copy of the engine: it needs the release
    library, found beside it, and reaches it through its public API; the code
    it shares with the other companions is compiled in, not linked."""
    lib, wlib = libs
    dyn = subprocess.check_output(["readelf", "-d", wlib], text=True)
    assert "libhadoofus_crc32c.so" in dyn and "$ORIGIN" in dyn
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", dyn)
    assert [n for n in needed if "hadoofus" in n] == ["libhadoofus_crc32c.so"], needed
    und = subprocess.check_output(["nm", "-D", "--undefined-only", wlib], text=True)
    for sym in ("hdfs_crc32c_init", "hdfs_crc32c_bound_device", "hdfs_crc32c_plan_create", "hdfs_crc32c_plan_execute",
                "hdfs_crc32c_plan_destroy"):
        assert sym in und, sym
    for sym in ("hdfs_wire_", "hdfs_writev_", "hdfs_wire_batch_", "hdfs_md5crc_"):
        assert sym not in und, sym
    engine = [l.split()[-1] for l in und.splitlines() if "hdfs_crc32c_" in l]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert engine and all(s.split("@")[0] in main for s in engine)


def test_abi_version_call_and_binding_check(wv):
    assert wv.load().hdfs_wirev_abi_version() == wv.ABI_VERSION == 1

    class Other:
        @staticmethod
        def hdfs_wirev_abi_version():
            return 2
    with pytest.raises(ImportError):
        wv.check_abi(Other())


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, wirev\n"
            "assert abi._lib is None and wirev._lib is None\n"
            "assert callable(h.compose_wire_iov) and callable(h.wirev_layout)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "wirev_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wirev_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wirev", "-lhadoofus_crc32c"])
    assert exe.exists()


def test_c_consumers_layout_figures(wv):
    """What tests/consumer/wirev_consumer.c expects of its own fragments."""
    info = wv.layout([65536 + 4000 + 77, 0, 3, 2 * 65536 - 3], 4321, 2, 2, True)
    assert (info["head_bytes"], info["nfrags"], info["max_frags_per_packet"], info["nsegments"]) == (287, 3, 3, 2)


def test_frame_gather_kernel_isa(tmp_path):
    """hipcc cross-compiles the kernel file to gfx950 assembly, nothing runs:
    both instances of frame_gather_kernel keep everything in registers (no
    scratch), use 32 B of LDS (the header), address global memory as global
    memory and read the fragment table with scalar loads."""
    from hadoofus_amd import build
    out = tmp_path / "wirev_kernels.s"
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           "-I" + build.INCLUDE, "-I" + build.CSRC, "-o", str(out),
                           os.path.join(build.CSRC, "wirev_kernels.hip")], stderr=subprocess.DEVNULL)
    txt = out.read_text()
    meta = re.findall(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                      r"\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?"
                      r"\s+\.vgpr_count:\s+(\d+)", txt)
    assert len(meta) == 2 and all("frame_gather_kernel" in m[1] for m in meta), meta
    for lds, name, scratch, sgpr, vgpr in meta:
        assert (int(lds), int(scratch)) == (32, 0), (name, lds, scratch)
        assert int(vgpr) <= 64 and int(sgpr) <= 96, (name, vgpr, sgpr)  # 8 waves per SIMD keep their registers
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+) ", txt, flags=re.M)
    assert not [o for o in ops if o.startswith(("flat_", "scratch_", "buffer_"))]
    assert not [o for o in ops if "atomic" in o]
    assert any(o.startswith("s_load_dword") for o in ops) and any(o == "global_store_dwordx4" for o in ops)
