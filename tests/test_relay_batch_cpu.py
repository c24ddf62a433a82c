"""CPU tests of the relay batch library (include/hadoofus_relay_batch.h): its
build beside the others, its ABI, its bindings (hadoofus_read/relay_batch.py),
the refusals its entry points decide without a GPU, the host layout against the
fused batch write library's, the kernels' metadata, and the arithmetic that is
its own (relay_batch_lookup.h) run on the CPU against a per-byte model
(tests/consumer/relay_batch_selftest.cpp, built with ASan/UBSan, nothing loaded
into Python)."""
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
DECLARED = {"hdfs_relay_batch_abi_version", "hdfs_relay_batch_last_error", "hdfs_relay_batch_relay",
            "hdfs_relay_batch_layout", "hdfs_relay_batch_time"}
OWN = ["relay_batch_kernels.hip", "relay_batch.cpp", "relay_batch_internal.h", "relay_batch_lookup.h"]
SHARED = ["read_batch_layout.h", "read_batch_header.h", "read_batch_verify.h", "wire_fused_batch_lookup.h",
          "wire_fused_batch_internal.h", "wire_fused_round.h", "wire_layout.h", "crc32c_frame.h", "crc32c_outpkt.h",
          "companion_support.h"]
OUTS = ("consumed", "delivered", "src_offset_in_block", "wire_len", "npkts", "rc", "path")


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


@pytest.fixture(scope="module")
def libs():
    """(release library, relay batch library), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.RELAY_BATCH_LIB


@pytest.fixture(scope="module")
def rl(libs):
    from hadoofus_read import relay_batch
    relay_batch.load()
    return relay_batch


# ---- the arithmetic on the CPU ------------------------------------------------------------------
def test_relay_batch_selftest(tmp_path):
    exe = tmp_path / "relay_batch_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "relay_batch_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout


def test_the_lookup_header_compiles_without_hip(tmp_path):
    """Plain C++ with no include path but the header's own directory: integer
    arithmetic only, as the other lookup headers.  Three packets of 5120 and
    one of 1300: payload chunk 10 is chunk 0 of packet 1, chunk 30 chunk 0 of
    the shorter packet; the second output round (chunks 8..15) crosses the seam
    at chunk 10."""
    src = tmp_path / "l.cpp"
    src.write_text('#include "relay_batch_lookup.h"\n'
                   "using namespace hdfs_relay_batch;\n"
                   "int main() { const uint64_t stride = 31 + 40 + 5120;\n"
                   "  const Geom g{stride, 3 * stride, 3 * 5120 + 1300, 10, 31, 3, 1300, 33, 1};\n"
                   "  uint64_t wl = 0, np = 0; out_shape(g.payload, 31, true, wl, np);\n"
                   "  const Cursor a = seek(g, 9), b = next_chunk(g, a), s = seek(g, 32);\n"
                   "  return (a.ip == 0 && a.ch == 9 && b.ip == 1 && b.ch == 0 && s.ip == 3 && s.ch == 2 &&\n"
                   "          data_at(g, b) == stride + 31 + 40 && crc_at(g, a) == 31 + 36 &&\n"
                   "          data_at(g, s) == 3 * stride + 33 + 12 + 1024 && crc_at(g, s) == 3 * stride + 33 + 8 &&\n"
                   "          np == 2 && wl == 2 * 31 + 4 * 33 + g.payload && in_packets(g) == 5 &&\n"
                   "          first_header(g, 0) == 0 && end_header(g, 0, 2) == 4 && first_header(g, 1) == 4 &&\n"
                   "          end_header(g, 1, 2) == 5 && crc_words(1300) == 3) ? 0 : 1; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0
    txt = open(os.path.join(ROOT, "hadoofus_amd", "csrc", "relay_batch_lookup.h")).read()
    assert re.findall(r"#include\s+(\S+)", txt) == ["<stdint.h>"]


# ---- build ---------------------------------------------------------------------------------
def test_build_produces_the_library_beside_the_others(libs):
    lib, rlib = libs
    assert os.path.exists(rlib) and os.path.basename(rlib) == "libhadoofus_relay_batch.so"
    assert os.path.dirname(lib) == os.path.dirname(rlib)


def test_build_tables():
    """The other tables are untouched; this library has a table of its own with
    rows of the same shape."""
    from hadoofus_amd import build
    assert len(build.COMPANIONS) == 9
    assert [r[0] for r in build.READ_LIBRARIES + build.PREAD_LIBRARIES + build.PREADV_LIBRARIES +
            build.DIGEST_LIBRARIES + build.CRC_LIBRARIES] == ["read_batch", "pread_batch", "preadv_batch",
                                                              "md5crc_streams", "crc_streams"]
    assert [r[0] for r in build.RELAY_LIBRARIES] == ["relay_batch"]
    for stem, sources, headers, public in build.RELAY_LIBRARIES:
        up = stem.upper()
        assert build.companion_lib(stem) == getattr(build, up + "_LIB")
        assert (sources, headers, public) == (getattr(build, up + "_SOURCES"), getattr(build, up + "_HEADERS"),
                                              getattr(build, up + "_PUBLIC"))
        assert f"{stem}_exports.map" in headers and f"hadoofus_{stem}.h" in public
        assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in sources + headers)
        assert all(os.path.exists(os.path.join(build.INCLUDE, f)) for f in public)
    # the fallback's framing is the fused batch write library's kernel file, compiled in as it stands
    assert build.RELAY_BATCH_SOURCES == ["relay_batch_kernels.hip", "wire_fused_batch_kernels.hip", "relay_batch.cpp"]
    assert {"relay_batch_internal.h", "relay_batch_lookup.h", *SHARED} <= set(build.RELAY_BATCH_HEADERS)
    assert "libhadoofus_relay_batch.so" in build.__doc__ and "RELAY_LIBRARIES" in build.__doc__
    # every header the sources include is a dependency of the row
    for f in OWN + ["wire_fused_batch_kernels.hip"]:
        for inc in re.findall(r'#include "([\w.]+)"', open(os.path.join(build.CSRC, f)).read()):
            assert inc in build.RELAY_BATCH_HEADERS + build.RELAY_BATCH_PUBLIC, (f, inc)


def test_sources_include_the_shared_code_and_copy_none():
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    code = lambda f: "\n".join(l for l in read(f).splitlines() if not l.lstrip().startswith("//"))  # noqa: E731
    kern, host, look = code(OWN[0]), code(OWN[1]), code(OWN[3])
    for inc in ("relay_batch_lookup.h", "relay_batch_internal.h", "read_batch_layout.h", "read_batch_header.h",
                "read_batch_verify.h", "wire_fused_batch_lookup.h", "wire_fused_round.h", "crc32c_outpkt.h"):
        assert f'#include "{inc}"' in kern, inc
    for inc in ("companion_support.h", "read_batch_host.h", "hadoofus_relay_batch.h", "wire_fused_batch_internal.h",
                "wire_fused_host.h",
                "wire_layout.h", "relay_batch_lookup.h"):
        assert f'#include "{inc}"' in host, inc
    every = "".join(read(f) for f in sorted(os.listdir(build.CSRC)))
    for name in ("uint32_t write_of(", "uint32_t frag_of(", "void count_packet(", "bool seek_write(",
                 "FUSED_DEV bool verify_round(", "FUSED_DEV void flag(", "FUSED_DEV Unit unit_of(",
                 "FUSED_DEV void header(", "FUSED_DEV void fill_image("):
        assert every.count(name) == 1, name
    for f in OWN:
        src = code(f)
        # no framing arithmetic, no header composition, no round and no comparison of its own, and no atomics
        for name in ("probe_entry(At", "frame_step(const", "put_out_header(", "put_header_proto(", "struct Unit {",
                     "permlane", "atomic", "hdfs_crc32c_plan_", "__builtin_amdgcn_raw_buffer", "plan_out_packets("):
            assert name not in src, (f, name)
        for name in ("range_of(", "load16(", "store16(", "load8(", "store8(", "load32(", "store32(", "fold8(",
                     "transpose(", "unit_of(", "load_round(", "store_round(", "crc_round(", "header(", "fill_image(",
                     "load_crcs(", "verify_round(", "verify_header(", "flag(", "write_of(", "packet_at(",
                     "prefix_regular("):
            assert not re.search(r"(FUSED_DEV|HDFS_RELAY_HD|HDFS_HD|inline) [\w:<> ]*\b" + re.escape(name), src), (f, name)
        for poly in ("82f63b78", "edb88320"):
            assert poly not in src.lower(), (f, poly)
    for name in ("probe_entry(", "prefix_regular(", "write_of(pk0, nw, g, k)", "unit_of(w, s.j, wave)", "store_round(",
                 "verify_round(lds, cur, wcur", "verify_header(hdr, proto", "header(hdr, proto", "flag(s.r, bad)",
                 "range_of(", "address_space(4)", "fill_image(", "__launch_bounds__(1024)", "seek(", "next_chunk(",
                 "data_at(", "crc_at(", "first_header(", "end_header(", "out_shape(", "geom_of("):
        assert name in kern, name
    # the probe has no destination limit and wants no records
    assert "~uint64_t(0), proto, chunk_size, ctype, false, 0," in kern
    # the new arithmetic is the header's; the kernel file only loads, compares and stores
    for name in ("out_shape(", "seek(", "next_chunk(", "data_at(", "crc_at(", "first_header(", "end_header(",
                 "in_packets("):
        assert re.search(r"HDFS_RELAY_HD \w+ " + re.escape(name), look), name
        assert not re.search(r"(inline|FUSED_DEV|HD) \w+ " + re.escape(name) + r"[^;]*\{", kern), name
    # the fallback: the main library's read, then the fused batch write library's launch over wire_layout.h's layout
    # (read_unlimited of read_batch_host.h, which also holds the run: this file synchronises through it and through
    # sync_and_report alone)
    shared = code("read_batch_host.h")
    assert host.count("read_unlimited(") == 1 and "hdfs_crc32c_read_packets(" not in host
    assert shared.count("hdfs_crc32c_read_packets(") == 2 and "launch_frame_fused_batch(" in host  # own room; grown
    assert "build_layout(" in host and "hipStreamSynchronize(" not in host and host.count("probed_run(") == 1
    for call in ("hipEventRecord(", "hipEventElapsedTime("):
        assert call not in host, call
    assert shared.count("hipMemcpyHostToDevice, st)") == 1 and shared.count("hipMemcpyDeviceToHost, st)") == 1
    assert shared.count("hipMemcpyAsync(") == 2 and shared.count("hipStreamSynchronize(") == 1
    # the overlap check is the one sweep of companion_support.h; this file defines none
    assert host.count("check_overlaps(") == 1 and "struct Span" not in host and "far_d" not in host
    # no existing source changes for it: the fused batch write library's kernel file is the one that library builds
    assert "wire_fused_batch_kernels.hip" in build.WIRE_FUSED_BATCH_SOURCES


# ---- ABI -------------------------------------------------------------------------------------
def test_library_exports_exactly_its_header(libs):
    _, rlib = libs
    assert _declared("hadoofus_relay_batch.h") == DECLARED
    funcs = _c_functions(rlib)
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_relay_batch.h")).read()
    v = int(re.search(r"#define HDFS_RELAY_BATCH_ABI_VERSION (\d+)", txt).group(1))
    assert v == 1 and set(funcs.values()) == {f"HADOOFUS_RELAY_BATCH_{v}"}, funcs
    m = open(os.path.join(ROOT, "hadoofus_amd", "csrc", "relay_batch_exports.map")).read()
    assert "HADOOFUS_RELAY_BATCH_1 {" in m and "hdfs_relay_batch_*;" in m


def test_library_links_the_one_engine_and_no_companion(libs):
    lib, rlib = libs
    dyn = subprocess.check_output(["readelf", "-d", rlib], text=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert [n for n in needed if "hadoofus" in n] == ["libhadoofus_crc32c.so"] and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", rlib], text=True)
    engine = sorted(l.split()[-1].split("@")[0] for l in und.splitlines() if "hdfs_" in l)
    # (plan_destroy: sync_and_report's, as in the fused write libraries; this library makes no plan)
    assert engine == ["hdfs_crc32c_bound_device", "hdfs_crc32c_init", "hdfs_crc32c_last_error",
                      "hdfs_crc32c_plan_destroy", "hdfs_crc32c_read_packets"]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert all(s in main for s in engine) and "hdfs_relay_batch" not in main


def test_header_says_what_the_call_promises():
    txt = open(os.path.join(ROOT, "include", "hadoofus_relay_batch.h")).read()
    for text in ("WHEN IT PAYS", "ORDERING", "hdfs_wire_fused_compose_packets", "hdfs_crc32c_read_packets",
                 "src/datanode.c:2590", "negative offset_in_block or seqno", "Streams may overlap"):
        assert text in txt, text
    assert "@@" not in txt


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_relay_batch.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_relay_batch_entry) - 104 + "
                   "HDFS_RELAY_BATCH_ABI_VERSION - 1 + (int)HDFS_RELAY_BATCH_TIME_GROUPS(0) + "
                   "HDFS_RELAY_BATCH_MAX_ENTRIES - 1024 + HDFS_RELAY_BATCH_PATH_KERNEL + "
                   "HDFS_RELAY_BATCH_PATH_FALLBACK - 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_read import relay_batch
    S, cname = relay_batch.Entry, "hdfs_relay_batch_entry"
    names = [f for f, _ in S._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_relay_batch.h"\n'
                   f'int main(void){{ printf("%zu", sizeof({cname}));\n' +
                   "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    assert got == [104, 0, 8, 16, 24, 32, 36, 40, 48, 56, 64, 72, 80, 88, 96, 100]  # pinned: the ABI of version 1
    assert names == ["stream", "len", "offset_in_block", "seqno", "finish", "reserved", "wire", "wire_cap", "consumed",
                     "delivered", "src_offset_in_block", "wire_len", "npkts", "rc", "path"]


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "relay_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "relay_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_relay_batch", "-lhadoofus_crc32c"])
    assert exe.exists()


# ---- bindings ----------------------------------------------------------------------------------
def test_import_loads_nothing():
    code = ("import hadoofus_read as r\nfrom hadoofus_amd import abi\nfrom hadoofus_read import relay_batch as m\n"
            "assert abi._lib is None and m._lib is None and r.relay_batch is m\n"
            "assert callable(m.relay) and callable(m.layout) and callable(m.time) and callable(m.entry)\n"
            "assert r.read_blocks is r.read_batch.read_blocks  # the package's own names are the read batch's still\n"
            "for name in ('LIB_PATH', 'ABI_VERSION', 'load', 'check_abi', 'bind', '_check'):\n"
            "    assert hasattr(m, name), name\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_loading_is_cached_and_a_missing_library_is_refused(libs, rl, tmp_path):
    from hadoofus_amd import build
    lib = rl.load()
    assert lib is not None and rl.load() is lib and rl._lib is lib
    assert rl.LIB_PATH == build.RELAY_BATCH_LIB and lib.hdfs_relay_batch_abi_version() == rl.ABI_VERSION == 1
    missing = str(tmp_path / "libhadoofus_relay_batch.so")
    code = ("from hadoofus_read import relay_batch as m\n"
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
    from hadoofus_read import relay_batch as m
    other = types.SimpleNamespace(hdfs_relay_batch_abi_version=lambda: 2)
    with pytest.raises(ImportError) as e:
        m.check_abi(other)
    assert "relay batch library ABI version 2, bindings written for 1" in str(e.value)
    same = types.SimpleNamespace(hdfs_relay_batch_abi_version=lambda: 1)
    assert m.check_abi(same) is same


def test_entry_helper():
    from hadoofus_read import relay_batch as m

    class T:  # what companion.ptr takes of a torch tensor
        def data_ptr(self):
            return 0x1000

        def numel(self):
            return 10

        def element_size(self):
            return 1
    want = dict(stream_ptr=0x1000, nbytes=10, wire_ptr=0x1000, wire_cap=10, offset_in_block=0, seqno=0, finish=False)
    assert m.entry(0x1000, 10, 0x1000, 10) == want == m.entry(T(), wire_ptr=T())
    assert m.entry(T(), 4)["nbytes"] == 4 and m.entry()["wire_ptr"] is None
    arr = m.entries([m.entry(0x1000, 10, 0x2000, 20, 512, 7, True)] * 2)
    assert (arr[1].stream, arr[1].len, arr[1].wire, arr[1].wire_cap, arr[1].offset_in_block, arr[1].seqno,
            arr[1].finish, arr[1].wire_len) == (0x1000, 10, 0x2000, 20, 512, 7, 1, 0)
    assert (m.MAX_ENTRIES, m.MAX_GROUPS, m.PATH_KERNEL, m.PATH_FALLBACK) == (1024, 1024, 0, 1)


# ---- refusals that need no device -----------------------------------------------------------------
def _spoil(arr):
    for e in arr:
        for f in OUTS:
            setattr(e, f, 7)


def _outs(arr):
    return [tuple(getattr(e, f) for f in OUTS) for e in arr]


def test_refusals_without_a_device(rl):
    lib = rl.load()
    good = [rl.entry(0x1000, 1000, 0x9000, 2000)] * 3  # never dereferenced: every call is decided by its arguments
    zero = (0, 0, 0, 0, 0, 0, rl.PATH_FALLBACK)

    def call(batch=good, n=None, proto=2, chunk=512, ctype=2, arr=None):
        arr = rl.entries(batch) if arr is None else arr
        _spoil(arr)
        n = len(batch) if n is None else n
        rc = lib.hdfs_relay_batch_relay(arr, n, proto, chunk, ctype, None)
        return rc, arr, lib.hdfs_relay_batch_last_error().decode()
    for kw, text in ((dict(proto=0), "proto"), (dict(proto=3), "proto"), (dict(ctype=3), "checksum type"),
                     (dict(ctype=-1), "checksum type"), (dict(ctype=0), "CRC32 or CRC32C"),
                     (dict(chunk=0), "chunk_size")):
        rc, arr, err = call(**kw)
        assert rc == EINVAL and "entry 0" in err and text in err and "device" not in err, (kw, err)
        assert _outs(arr) == [zero] * 3, kw
    rc, _, err = call(n=0)
    assert rc == EINVAL and "no entries" in err
    rc, _, err = call(n=rl.MAX_ENTRIES + 1, arr=(rl.Entry * (rl.MAX_ENTRIES + 1))())
    assert rc == EINVAL and "1025 entries" in err and "1024" in err
    for bad, text in ((rl.entry(None, 5, 0x9000, 2000), "stream"), (rl.entry(0x1000, 5, None, 2000), "wire"),
                      (rl.entry(0x1000, 5, 0x9000, 2000, offset_in_block=-512), "negative block offset"),
                      (rl.entry(0x1000, 5, 0x9000, 2000, seqno=-1), "negative seqno")):
        rc, arr, err = call([good[0], bad])
        assert rc == EINVAL and "entry 1" in err and text in err and "device" not in err, err
        assert _outs(arr) == [zero] * 2
    assert lib.hdfs_relay_batch_relay(None, 3, 2, 512, 2, None) == EINVAL
    with pytest.raises(rl.abi.CRC32CError) as e:  # through the bindings: the call's own refusal raises
        rl.relay(good, proto=7)
    assert e.value.code == EINVAL and "proto" in str(e.value)


def test_timing_argument_errors(rl):
    lib, out = rl.load(), ctypes.c_double(5)
    one = [rl.entry(0x1000, 100, 0x9000, 200)]

    def call(flags=0, iters=1, res=ctypes.byref(out), proto=2):
        rc = lib.hdfs_relay_batch_time(rl.entries(one), 1, proto, 512, 2, flags, iters, res)
        return rc, lib.hdfs_relay_batch_last_error()
    # every one decided before a device is asked (0x1000 is no device memory: going on would say so)
    for kw in (dict(iters=0), dict(iters=-3), dict(res=None)):
        rc, err = call(**kw)
        assert rc == EINVAL and b"iters" in err and b"device" not in err, (kw, err)
    assert call(proto=7)[0] == EINVAL
    for flags in (1, 2, rl.time_groups(rl.MAX_GROUPS + 1), rl.time_groups(2) | 4):
        rc, err = call(flags=flags)
        assert rc == EINVAL and b"workgroups" in err and b"device" not in err, (flags, err)
    assert out.value == 0  # set to 0 by every call that was given it


def test_last_error_text_is_its_own(rl):
    from hadoofus_read import read_batch as rb
    bl, lib = rb.load(), rl.load()
    assert bl.hdfs_read_batch_read_blocks(rb.entries([rb.entry(0x1000, 5, 0x2000, 5)]), 1, 7, 512, 2, None, 0,
                                          None) == EINVAL
    before = bl.hdfs_read_batch_last_error()
    assert lib.hdfs_relay_batch_relay(rl.entries([rl.entry(0x1000, 5, 0x2000, 5)]), 1, 2, 0, 2, None) == EINVAL
    assert lib.hdfs_relay_batch_last_error() == b"entry 0: chunk_size 0"
    assert bl.hdfs_read_batch_last_error() == before == b"entry 0: proto must be 1 or 2"


# ---- the host layout ----------------------------------------------------------------------------------
def test_layout_is_the_fused_batch_write_librarys(rl):
    """hdfs_relay_batch_layout touches no device: over a grid of payloads and
    offsets, unaligned included, wire_len and npkts are
    hdfs_wire_fused_batch_layout's of the same write."""
    from hadoofus_amd import wire_fused_batch as fb
    payloads = [0, 1, 511, 512, 513, 4096, 65535, 65536, 65537, 3 * 64512 + 700, 2 * 65536 + 700, (8 << 20) + 777]
    offsets = [0, 512, 3584, 4321, 1, 511, (1 << 31) + 512, (1 << 31) + 777]
    for proto in (1, 2):
        for ctype in (1, 2):
            for finish in (False, True):
                writes = [fb.write(nbytes=n, offset_in_block=o, seqno=5, finish=finish) for n in payloads for o in offsets]
                outs, _ = fb.layout(writes, proto, ctype)
                got = [rl.layout(n, o, proto, ctype, finish) for n in payloads for o in offsets]
                assert got == [(w["wire_len"], w["npkts"]) for w in outs], (proto, ctype, finish)
    assert rl.layout(0, 0, finish=True) == (31, 1) and rl.layout(0, 0) == (0, 0)
    lib, a, b = rl.load(), ctypes.c_uint64(9), ctypes.c_uint64(9)
    for args in ((10, -1, 2, 2, 0), (10, 0, 3, 2, 0), (10, 0, 2, 7, 0)):
        assert lib.hdfs_relay_batch_layout(*args, ctypes.byref(a), ctypes.byref(b)) == EINVAL, args
        assert (a.value, b.value) == (0, 0)
    assert lib.hdfs_relay_batch_layout(10, 0, 2, 2, 0, None, ctypes.byref(b)) == EINVAL


# ---- the kernels' metadata --------------------------------------------------------------------------
def test_kernel_metadata(tmp_path):
    """hipcc -S of the kernel file: neither kernel has a private segment or a
    vector register spill.  The main kernel is 16 waves with dynamic LDS only
    (the table image and 64 bytes of expected header per wave), at most 128
    vector registers (four waves a SIMD), reads the streams through buffer
    ranges only and keeps the scalar registers it cannot hold in lanes of
    vector registers (v_writelane, no memory); the probe -- the read batch's
    probe_entry as it stands, one workgroup, run once a call -- has its two
    count arrays in LDS."""
    from hadoofus_amd import build
    asm = tmp_path / "relay_batch_kernels.s"
    subprocess.check_call([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only",
                           "-S", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
                           os.path.join(build.CSRC, "relay_batch_kernels.hip"), "-o", str(asm)])
    txt = asm.read_text()
    meta = {}
    for block in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(
            r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|"
            r"max_flat_workgroup_size):\s+(\d+)", block)}
    assert len(meta) == 2
    get = lambda part: next(v for k, v in meta.items() if part in k)  # noqa: E731
    probe, main = get("probe_relay_kernel"), get("relay_fused_batch_kernel")
    for k in (probe, main):
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
        assert k["max_flat_workgroup_size"] == 1024 and k["vgpr_count"] <= 128, k
    assert main["group_segment_fixed_size"] == 0  # dynamic LDS only
    assert probe["group_segment_fixed_size"] == 8192
    body = txt.split("relay_fused_batch_kernel", 2)[-1].split(".end_amdhsa_kernel")[0]
    assert "buffer_load_dwordx4" in body and "buffer_store_dwordx4" in body
    assert "flat_load" not in body and "flat_store" not in body and "global_store" not in body
    assert "atomic" not in txt and "scratch_" not in txt
    kern = open(os.path.join(build.CSRC, "relay_batch_kernels.hip")).read()
    assert "(crc::kImageWords + kExpectWords * kWaves) * sizeof(uint32_t)" in kern
