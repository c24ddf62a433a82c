"""CPU tests of the preadv batch library (include/hadoofus_preadv_batch.h): its
build beside the others in a table of its own, its ABI, its bindings
(hadoofus_read.preadv_batch), the rejections its entry points decide without a
GPU, the kernels' metadata, what it shares with the pread batch library and
leaves unchanged there, and the scatter store's arithmetic
(preadv_batch_lookup.h) run on the CPU against a per-byte brute-force model
(tests/consumer/preadv_batch_selftest.cpp, built with ASan/UBSan, nothing
loaded into Python)."""
import ctypes
import os
import re
import subprocess
import sys
import types

import pytest

from abi_symbols import c_functions as _c_functions, declared as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
DECLARED = {"hdfs_preadv_batch_abi_version", "hdfs_preadv_batch_last_error", "hdfs_preadv_batch_read",
            "hdfs_preadv_batch_time"}
NINE = ["md5crc", "writev", "wire", "wire_batch", "wirev", "wire_fused", "wire_fused_batch", "wirev_fused",
        "wirev_fused_batch"]
OWN = ["preadv_batch_kernels.hip", "preadv_batch.cpp", "preadv_batch_internal.h", "preadv_batch_lookup.h",
       "read_batch_header.h"]


@pytest.fixture(scope="module")
def libs():
    """(release library, preadv batch library), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.PREADV_BATCH_LIB


@pytest.fixture(scope="module")
def pv(libs):
    from hadoofus_read import preadv_batch
    preadv_batch.load()
    return preadv_batch


# ---- the scatter store's arithmetic on the CPU -----------------------------------------------
def test_preadv_batch_selftest(tmp_path):
    exe = tmp_path / "preadv_batch_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "preadv_batch_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout
    plain, seamed, small = map(int, re.search(r"(\d+) unseamed rounds, (\d+) seamed rounds, (\d+) pieces below 16 B",
                                              p.stdout).groups())
    assert plain >= 1000 and seamed >= 1000 and small >= 1000, p.stdout


def test_lookup_header_compiles_without_hip(tmp_path):
    src = tmp_path / "l.cpp"
    src.write_text('#include "preadv_batch_lookup.h"\n'
                   "using namespace hdfs_preadv_batch;\n"
                   "int main() { const uint32_t fr0[3] = {0, 4, 6}; const uint64_t at[6] = {0, 1, 2, 9, 0, 7};\n"
                   "Cursor c; seek_slot(c, 0); Slice s = slice_of(fr0, 0u);\n"
                   "bool ok = s.first == 0 && s.nf == 3 && seek_frag(at, s.nf, 5, c) == 2 && c.kf == 2;\n"
                   "seek_slot(c, 1); ok = ok && c.kf == 0; s = slice_of(fr0, 1u); ok = ok && s.first == 4 && s.nf == 1;\n"
                   "Walk w{0, 3}; Piece p; ok = ok && next_piece(at, 3u, 0, 3, 12, w, p) && p.k == 0 && p.ps == 3 && "
                   "p.pe == 4 && p.foff == 0;\n"
                   "ok = ok && next_piece(at, 3u, 0, 3, 12, w, p) && p.k == 1 && p.pe == 5;\n"
                   "ok = ok && next_piece(at, 3u, 0, 3, 12, w, p) && p.k == 2 && p.ps == 5 && p.pe == 12 && "
                   "!next_piece(at, 3u, 0, 3, 12, w, p);\n"
                   "uint32_t q; ok = ok && whole_at(16, 0, 32) == 16 && whole_at(16, 17, 64) == kOutside && "
                   "byte_at(5, 5, 6) == 0 && byte_at(6, 5, 6) == kOutside && head_edge(17, 64, q) && q == 1 && "
                   "!head_edge(16, 64, q) && tail_edge(16, 70, q) && q == 4 && !tail_edge(16, 64, q);\n"
                   "return ok ? 0 : 1; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0
    from hadoofus_amd import build
    look = "\n".join(l for l in open(os.path.join(build.CSRC, "preadv_batch_lookup.h")).read().splitlines()
                     if not l.lstrip().startswith("//"))
    assert "hip" not in look.lower() and '#include "wirev_fused_lookup.h"' in look


# ---- build -----------------------------------------------------------------------------------
def test_build_produces_the_library_beside_the_others(libs):
    lib, plib = libs
    assert os.path.exists(plib) and os.path.basename(plib) == "libhadoofus_preadv_batch.so"
    assert os.path.dirname(lib) == os.path.dirname(plib)
    from hadoofus_amd import build
    assert os.path.exists(build.PREAD_BATCH_LIB) and os.path.exists(build.READ_BATCH_LIB)


def test_build_tables():
    """The nine companions, the read side's table and the positional reads'
    are untouched; scatter reads have a table of their own with rows of the
    same shape."""
    from hadoofus_amd import build
    assert [c[0] for c in build.COMPANIONS] == NINE
    assert [r[0] for r in build.READ_LIBRARIES] == ["read_batch"]
    assert [r[0] for r in build.PREAD_LIBRARIES] == ["pread_batch"]
    assert [r[0] for r in build.PREADV_LIBRARIES] == ["preadv_batch"]
    for stem, sources, headers, public in build.PREADV_LIBRARIES:
        up = stem.upper()
        assert build.companion_lib(stem) == getattr(build, up + "_LIB")
        assert (sources, headers, public) == (getattr(build, up + "_SOURCES"), getattr(build, up + "_HEADERS"),
                                              getattr(build, up + "_PUBLIC"))
        assert f"{stem}_exports.map" in headers and f"hadoofus_{stem}.h" in public
        assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in sources + headers)
        assert all(os.path.exists(os.path.join(build.INCLUDE, f)) for f in public)
    assert build.PREADV_BATCH_SOURCES == ["preadv_batch_kernels.hip", "preadv_batch.cpp"]
    assert {"preadv_batch_internal.h", "preadv_batch_lookup.h", "read_batch_header.h", "pread_batch_internal.h",
            "pread_batch_layout.h", "read_batch_layout.h", "read_batch_verify.h", "wirev_fused_internal.h",
            "wirev_fused_lookup.h", "wire_fused_round.h", "wire_fused_batch_lookup.h", "crc32c_frame.h",
            "companion_support.h"} <= set(build.PREADV_BATCH_HEADERS)
    assert "libhadoofus_preadv_batch.so" in build.__doc__ and "PREADV_LIBRARIES" in build.__doc__
    # every header the sources include is a dependency of the row
    for f in OWN:
        for inc in re.findall(r'#include "([\w.]+)"', open(os.path.join(build.CSRC, f)).read()):
            assert inc in build.PREADV_BATCH_HEADERS + build.PREADV_BATCH_PUBLIC, (f, inc)


def test_the_pread_batch_library_is_unchanged():
    """Its build row and the sources this library compiles beside it are the
    ones the pread batch library was merged with."""
    import hashlib
    from hadoofus_amd import build
    assert build.PREAD_BATCH_SOURCES == ["pread_batch_kernels.hip", "pread_batch.cpp"]
    assert build.PREAD_BATCH_HEADERS == [
        "pread_batch_internal.h", "pread_batch_layout.h", "read_batch_layout.h", "read_batch_verify.h",
        "wire_fused_batch_lookup.h", "wire_fused_round.h", "wire_fused_crc.h", "wire_fused_tables.h",
        "wire_fused_host.h", "wire_internal.h", "crc32c_frame.h", "crc32c_outpkt.h", "crc32c_tables.h",
        "companion_support.h", "read_batch_host.h", "pread_batch_exports.map"]
    assert not set(build.PREAD_BATCH_HEADERS + build.PREAD_BATCH_SOURCES) & set(OWN + ["preadv_batch_exports.map"])
    # (pread_batch.cpp has since moved onto the read side's shared host header, read_batch_host.h)
    want = {"pread_batch_kernels.hip": "f32110dd5b28e30a5f5c9775af47e36bd34e6efa4efe77b62180dde49ee2fac0", "pread_batch_internal.h": "def77bed855b7d4ffaf5195f39a7c3689c098a057847aa8a90c25281669b8638",
            "pread_batch_layout.h": "c684bcccc86fc1f2dcde9341fa56f8edd29421d68341569567ec8da779a73ab6", "read_batch_verify.h": "bc5664e6208aa6992fc11c2f96dc82f4c17a62323bc938581d848dc61376b0e1"}
    for f, digest in want.items():
        assert hashlib.sha256(open(os.path.join(build.CSRC, f), "rb").read()).hexdigest() == digest, f


def test_sources_share_the_round_the_layout_and_the_lookups_and_copy_none():
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    code = lambda f: "\n".join(l for l in read(f).splitlines() if not l.lstrip().startswith("//"))  # noqa: E731
    kern, host, look, hdr = (code(f) for f in ("preadv_batch_kernels.hip", "preadv_batch.cpp",
                                               "preadv_batch_lookup.h", "read_batch_header.h"))
    for inc in ("wire_fused_round.h", "wire_fused_batch_lookup.h", "crc32c_frame.h", "crc32c_outpkt.h",
                "pread_batch_layout.h", "read_batch_verify.h", "read_batch_header.h", "preadv_batch_lookup.h",
                "preadv_batch_internal.h"):
        assert f'#include "{inc}"' in kern, inc
    for inc in ("companion_support.h", "read_batch_host.h", "wire_fused_host.h", "wire_fused_tables.h",
                "pread_batch_layout.h"):
        assert f'#include "{inc}"' in host, inc
    assert '#include "wirev_fused_internal.h"' in code("preadv_batch_internal.h")
    # the four lookups' texts stay where they are, in files of their own, comments included
    for f in OWN:
        raw = read(f)
        for name in ("uint32_t frag_of(", "uint32_t write_of(", "void count_packet(", "bool seek_write("):
            assert name not in raw, (f, name)
    every = "".join(read(f) for f in sorted(os.listdir(build.CSRC)))
    for name in ("uint32_t frag_of(", "uint32_t write_of(", "void count_packet(", "bool seek_write("):
        assert every.count(name) == 1, name
    # nothing of the round, of the comparisons or of the window arithmetic is defined again
    for f in OWN:
        src = code(f)
        for name in ("range_of(", "load16(", "store16(", "store32(", "load8(", "store8(", "fold8(", "transpose(",
                     "unit_of(", "load_round(", "store_round(", "crc_round(", "ragged_chunk(", "fill_image(",
                     "load_crcs(", "verify_round(", "flag(", "edge_piece(", "seam_round(", "ragged_gather("):
            assert not re.search(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), src), (f, name)
        for name in ("probe_window(At", "probe_entry(At", "struct Unit {", "struct Frag ", "struct AtOf", "permlane",
                     "atomic", "hdfs_crc32c_plan_", "__builtin_amdgcn_raw_buffer"):
            assert name not in src, (f, name)
        for poly in ("82f63b78", "edb88320"):
            assert poly not in src.lower(), (f, poly)
    assert len(re.findall(r"FUSED_DEV bool verify_header\(", hdr)) == 1 and "verify_header(hdr, proto" in kern
    assert not re.search(r"FUSED_DEV \w+ verify_header\(", kern)
    for name in ("write_of(pk0, nw, g, k)", "load_round(", "store_round(", "store16(", "store8(", "range_of(",
                 "address_space(4)", "kNowhere", "probe_window(", "seek_slot(", "slice_of(", "seek_frag(",
                 "next_piece(", "whole_at(", "byte_at(", "head_edge(", "tail_edge(", "unseamed(",
                 "__launch_bounds__(1024)"):
        assert name in kern, name
    for name in ("seek_slot(", "slice_of(", "seek_frag(", "next_piece(", "whole_at(", "byte_at(", "head_edge(",
                 "tail_edge(", "unseamed("):
        assert len(re.findall(r"HDFS_WIREV_FUSED_HD \w+ " + re.escape(name), look)) == 1, name
        assert not re.search(r"(inline|FUSED_DEV|HD) \w+ " + re.escape(name), kern), name
    # the run, the outcomes and the main library's read are the shared header's, once for the six libraries
    shared = "\n".join(l for l in read("read_batch_host.h").splitlines() if not l.lstrip().startswith("//"))
    for call in ("hipMemcpyAsync(", "hipStreamSynchronize(", "hipEventRecord(", "hipEventElapsedTime(",
                 "hdfs_crc32c_read_packets("):
        assert call not in host, call
    assert '#include "read_batch_host.h"' in host and host.count("probed_run(") == 1
    assert host.count("read_unlimited(") == 1 and shared.count("hdfs_crc32c_read_packets(") == 2  # own room; grown
    assert shared.count("hipMemcpyHostToDevice, st)") == 1 and shared.count("hipMemcpyDeviceToHost, st)") == 1
    assert shared.count("hipMemcpyAsync(") == 2 and shared.count("hipStreamSynchronize(") == 1
    assert "x.read_len, x.iov," in host and "x.iovcnt" in host
    # the overlap check is the one sweep of companion_support.h; this file defines none
    assert host.count("check_overlaps(") == 1 and "struct Span" not in host and "far_d" not in host


# ---- ABI -------------------------------------------------------------------------------------
def test_library_exports_exactly_its_header(libs):
    _, plib = libs
    assert _declared("hadoofus_preadv_batch.h") == DECLARED
    funcs = _c_functions(plib)
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_preadv_batch.h")).read()
    v = int(re.search(r"#define HDFS_PREADV_BATCH_ABI_VERSION (\d+)", txt).group(1))
    assert v == 1 and set(funcs.values()) == {f"HADOOFUS_PREADV_BATCH_{v}"}, funcs


def test_library_links_the_one_engine_through_four_calls(libs):
    lib, plib = libs
    dyn = subprocess.check_output(["readelf", "-d", plib], text=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert [n for n in needed if "hadoofus" in n] == ["libhadoofus_crc32c.so"] and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", plib], text=True)
    engine = sorted(l.split()[-1].split("@")[0] for l in und.splitlines() if "hdfs_" in l)
    assert engine == ["hdfs_crc32c_bound_device", "hdfs_crc32c_init", "hdfs_crc32c_last_error",
                      "hdfs_crc32c_read_packets"]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert all(s in main for s in engine) and "hdfs_preadv_batch" not in main


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_preadv_batch.h"\n'
                   "typedef char entry_is_80_bytes[sizeof(hdfs_preadv_batch_entry) == 80 ? 1 : -1];\n"
                   "int main(void){ return (int)sizeof(hdfs_preadv_batch_entry) - 80 + HDFS_PREADV_BATCH_ABI_VERSION - 1 "
                   "+ (int)HDFS_PREADV_BATCH_TIME_GROUPS(0) + HDFS_PREADV_BATCH_MAX_ENTRIES - 1024 + "
                   "(int)(HDFS_PREADV_BATCH_MAX_FRAGS - (1u << 22)) + "
                   "HDFS_PREADV_BATCH_PATH_KERNEL + HDFS_PREADV_BATCH_PATH_FALLBACK - 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_read import preadv_batch
    S = preadv_batch.Entry
    names = [f for f, _ in S._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_preadv_batch.h"\n'
                   'int main(void){ printf("%zu", sizeof(hdfs_preadv_batch_entry));\n' +
                   "".join(f'printf(" %zu", offsetof(hdfs_preadv_batch_entry, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    assert got == [80, 0, 8, 16, 24, 28, 32, 40, 48, 56, 64, 72, 76]  # pinned: the ABI of version 1


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "preadv_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "preadv_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_preadv_batch", "-lhadoofus_crc32c"])
    assert exe.exists()


# ---- bindings ----------------------------------------------------------------------------------
def test_import_loads_nothing_and_the_package_keeps_its_names():
    code = ("import hadoofus_read as r\nfrom hadoofus_amd import abi\n"
            "from hadoofus_read import pread_batch, preadv_batch, read_batch\n"
            "assert abi._lib is None and read_batch._lib is None and pread_batch._lib is None\n"
            "assert preadv_batch._lib is None and r.preadv_batch is preadv_batch and r.pread_batch is pread_batch\n"
            "assert r.read_blocks is read_batch.read_blocks and r.time is read_batch.time\n"
            "for name in ('LIB_PATH', 'ABI_VERSION', 'MAX_ENTRIES', 'MAX_FRAGS', 'MAX_GROUPS', 'PATH_KERNEL',\n"
            "             'PATH_FALLBACK', 'Entry', 'entry', 'entries', 'read', 'time', 'time_groups', 'load',\n"
            "             'check_abi', 'bind', '_check'):\n"
            "    assert hasattr(preadv_batch, name), name\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_loading_is_cached_and_a_missing_library_is_refused(libs, pv, tmp_path):
    from hadoofus_amd import build
    lib = pv.load()
    assert lib is not None and pv.load() is lib and pv._lib is lib
    assert pv.LIB_PATH == build.PREADV_BATCH_LIB and lib.hdfs_preadv_batch_abi_version() == pv.ABI_VERSION == 1
    missing = str(tmp_path / "libhadoofus_preadv_batch.so")
    code = ("from hadoofus_read import preadv_batch as m\n"
            f"path = {missing!r}\n"
            "try:\n"
            "    m.load(path=path)\n"
            "except ImportError as e:\n"
            "    assert path in str(e) and 'hadoofus_amd.build' in str(e), e\n"
            "else:\n"
            "    raise SystemExit('a library that is not there was loaded')\n"
            "assert m._lib is None\n"
            "assert m.load() is m._lib is not None\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_a_wrong_abi_is_refused():
    from hadoofus_read import preadv_batch as m
    other = types.SimpleNamespace(hdfs_preadv_batch_abi_version=lambda: 2)
    with pytest.raises(ImportError) as e:
        m.check_abi(other)
    assert "preadv batch library ABI version 2, bindings written for 1" in str(e.value)
    same = types.SimpleNamespace(hdfs_preadv_batch_abi_version=lambda: 1)
    assert m.check_abi(same) is same


def test_entry_helper():
    from hadoofus_read import preadv_batch as m

    class T:  # what companion.ptr takes of a torch tensor
        def __init__(self, p, n):
            self.p, self.n = p, n

        def data_ptr(self):
            return self.p

        def numel(self):
            return self.n

        def element_size(self):
            return 1
    assert m.entry(0x1000, 10, [(0x2000, 20), (None, 0), (0x3000, 5)], 700, 5) == \
        dict(stream_ptr=0x1000, nbytes=10, frags=[(0x2000, 20), (None, 0), (0x3000, 5)], client_offset=700, read_len=5)
    # read_len None: the fragments' total, hdfs_datanode_readv's meaning
    assert m.entry(T(0x1000, 10), None, [T(0x2000, 20), (0x3000, 5)], client_offset=3) == \
        dict(stream_ptr=0x1000, nbytes=10, frags=[(0x2000, 20), (0x3000, 5)], client_offset=3, read_len=25)
    arr, keep = m.entries([m.entry(0x1000, 10, [(0x2000, 20), (0x3000, 5)], 1 << 40, 7)] * 2)
    assert (arr[1].stream, arr[1].len, arr[1].iovcnt, arr[1].reserved, arr[1].client_offset, arr[1].read_len) == \
        (0x1000, 10, 2, 0, 1 << 40, 7)
    assert (arr[1].iov[0].base, arr[1].iov[0].len, arr[1].iov[1].base, arr[1].iov[1].len) == (0x2000, 20, 0x3000, 5)
    assert len(keep) == 2
    assert m.time_groups(3) == 3 << 8 and m.MAX_GROUPS == 1024 and m.MAX_ENTRIES == 1024 and m.MAX_FRAGS == 1 << 22


# ---- rejections that need no device ---------------------------------------------------------------
def test_rejections_without_a_device(pv):
    from hadoofus_amd.abi import IoVec, Packet
    lib = pv.load()
    pk = (Packet * 8)()
    before = bytes(pk)
    # never dereferenced: every call is decided by its arguments
    good = [pv.entry(0x1000, 1000, [(0x100000, 600), (0x200000, 400)], 512, 100)] * 3

    def call(batch=good, n=None, proto=2, cs=512, ctype=2, arr=None):
        keep = None
        if arr is None:
            arr, keep = pv.entries(batch)
        for e in arr:
            e.rc, e.path, e.npkts, e.consumed, e.delivered = 7, 7, 7, 7, 7
        rc = lib.hdfs_preadv_batch_read(arr, len(batch) if n is None else n, proto, cs, ctype, pk, 2, None)
        del keep
        return rc, arr, lib.hdfs_preadv_batch_last_error().decode()
    zeros = [(0, 0, 0, 0, pv.PATH_FALLBACK)] * 3
    outs = lambda arr: [(e.rc, e.npkts, e.consumed, e.delivered, e.path) for e in arr]  # noqa: E731
    for kw, text in ((dict(proto=0), "proto"), (dict(proto=3), "proto"), (dict(ctype=3), "checksum type"),
                     (dict(ctype=-1), "checksum type"), (dict(ctype=0), "CRC32 or CRC32C"),
                     (dict(cs=0), "chunk_size")):
        rc, arr, err = call(**kw)
        assert rc == EINVAL and "entry 0" in err and text in err and b"device" not in err.encode(), (kw, err)
        assert outs(arr) == zeros
    for rl, text in ((0, "read_len 0"), (-5, "read_len -5"), (-1, "hdfs_read_batch_read_blocks")):
        rc, arr, err = call([good[0], pv.entry(0x1000, 1000, [(0x100000, 1000)], 512, rl), good[0]])
        assert rc == EINVAL and "entry 1" in err and text in err and b"device" not in err.encode(), (rl, err)
        assert outs(arr) == zeros
    rc, _, err = call(n=0)
    assert rc == EINVAL and "no entries" in err
    rc, _, err = call(n=pv.MAX_ENTRIES + 1, arr=(pv.Entry * (pv.MAX_ENTRIES + 1))())
    assert rc == EINVAL and "1025 entries" in err and "1024" in err
    assert lib.hdfs_preadv_batch_read(None, 3, 2, 512, 2, pk, 2, None) == EINVAL
    rc, _, err = call([good[0], pv.entry(None, 5, [(0x2000, 5)], 0, 1)])
    assert rc == EINVAL and "entry 1" in err and "stream" in err
    # no fragments, or no array of them
    rc, arr, err = call([good[0], good[0], pv.entry(0x1000, 5, [], 0, 1)])
    assert rc == EINVAL and "entry 2" in err and "iovcnt 0" in err and outs(arr) == zeros
    arr, keep = pv.entries(good)
    arr[1].iovcnt = -4
    rc, arr, err = call(arr=arr)
    assert rc == EINVAL and "entry 1" in err and "iovcnt -4" in err and outs(arr) == zeros
    arr, keep = pv.entries(good)
    arr[2].iov = None
    rc, arr, err = call(arr=arr)
    assert rc == EINVAL and "entry 2" in err and "null iov" in err and outs(arr) == zeros
    # a NULL base with a length (built by hand: the bindings' IoVec helper keeps what it is given)
    vec = (IoVec * 3)(IoVec(0x100000, 10), IoVec(None, 0), IoVec(None, 7))
    arr, keep = pv.entries(good)
    arr[1].iov, arr[1].iovcnt = vec, 3
    rc, arr, err = call(arr=arr)
    assert rc == EINVAL and "entry 1" in err and "fragment 2" in err and "null base" in err and outs(arr) == zeros
    # more non-empty fragments than a call takes: 1024 entries share one array of 4097 one-byte fragments
    per = pv.MAX_FRAGS // pv.MAX_ENTRIES + 1
    vec = (IoVec * per)(*[IoVec(0x100000 + 2 * i, 1) for i in range(per)])
    arr = (pv.Entry * pv.MAX_ENTRIES)()
    for e in arr:
        e.stream, e.len, e.iov, e.iovcnt, e.client_offset, e.read_len = 0x1000, 100, vec, per, 0, 10
    rc = lib.hdfs_preadv_batch_read(arr, pv.MAX_ENTRIES, 2, 512, 2, None, 0, None)
    err = lib.hdfs_preadv_batch_last_error().decode()
    assert rc == EINVAL and "entry 1023" in err and "fragment 3073" in err and str(pv.MAX_FRAGS) in err, err
    assert b"device" not in err.encode()
    assert bytes(pk) == before
    with pytest.raises(pv.abi.CRC32CError) as e:  # through the bindings: the call's own refusal raises
        pv.read(good, proto=7)
    assert e.value.code == EINVAL and "proto" in str(e.value)


def test_timing_argument_errors(pv):
    lib, ms = pv.load(), ctypes.c_double(5)
    one = [pv.entry(0x1000, 100, [(0x2000, 100)], 0, 50)]

    def call(flags=0, iters=1, out=ctypes.byref(ms), proto=2):
        arr, _keep = pv.entries(one)
        rc = lib.hdfs_preadv_batch_time(arr, 1, proto, 512, 2, flags, iters, out)
        assert (arr[0].rc, arr[0].npkts, arr[0].consumed, arr[0].delivered) == (0, 0, 0, 0)
        return rc, lib.hdfs_preadv_batch_last_error()
    # every one decided before a device is asked (0x1000 is no device memory: going on would say so)
    for kw in (dict(iters=0), dict(iters=-3), dict(out=None)):
        rc, err = call(**kw)
        assert rc == EINVAL and b"iters" in err and b"device" not in err, (kw, err)
    assert call(proto=7)[0] == EINVAL
    for flags in (pv.time_groups(pv.MAX_GROUPS + 1), pv.time_groups(1 << 23), 1, pv.time_groups(2) | 4):
        rc, err = call(flags=flags)
        assert rc == EINVAL and b"workgroups" in err, (flags, err)
    assert ms.value == 0  # set to 0 by every call that was given it


def test_last_error_text_is_its_own(pv):
    from hadoofus_read import pread_batch as pb
    pl, lib = pb.load(), pv.load()
    assert pl.hdfs_pread_batch_read(pb.entries([pb.entry(0x1000, 5, 0x2000, 5, 0, 1)]), 1, 7, 512, 2, None, 0,
                                    None) == EINVAL
    before = pl.hdfs_pread_batch_last_error()
    arr, _keep = pv.entries([pv.entry(0x1000, 5, [(0x2000, 5)], 0, 1)])
    assert lib.hdfs_preadv_batch_read(arr, 1, 2, 0, 2, None, 0, None) == EINVAL
    assert lib.hdfs_preadv_batch_last_error() == b"entry 0: chunk_size 0"
    assert pl.hdfs_pread_batch_last_error() == before and b"proto" in before


# ---- the kernels' metadata --------------------------------------------------------------------------
def test_kernel_metadata(tmp_path):
    """hipcc -S of the kernel file: neither kernel has a private segment (no
    scratch) or spills a vector register, both are bounded to 1024 threads, the
    main kernel's LDS is all dynamic (the table image and the expected header)
    and its registers leave room for 16 waves a workgroup (1024 threads are
    four waves a SIMD: at most 128 VGPRs), the probe's LDS is its two count
    arrays."""
    from hadoofus_amd import build
    asm = tmp_path / "preadv_batch_kernels.s"
    subprocess.check_call([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only",
                           "-S", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
                           os.path.join(build.CSRC, "preadv_batch_kernels.hip"), "-o", str(asm)])
    txt = asm.read_text()
    meta = {}
    for block in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(
            r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|"
            r"max_flat_workgroup_size):\s+(\d+)", block)}
    probe = next(v for k, v in meta.items() if "preadv_probe_kernel" in k)
    main = next(v for k, v in meta.items() if "unframe_scatter_batch_kernel" in k)
    assert len(meta) == 2
    for k in (probe, main):
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0
        assert k["max_flat_workgroup_size"] == 1024 and k["vgpr_count"] <= 128
    assert main["group_segment_fixed_size"] == 0 and probe["group_segment_fixed_size"] == 8192
