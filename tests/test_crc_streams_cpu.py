"""CPU tests of the CRC streams library (include/hadoofus_crc_streams.h): its
build beside the others, its ABI, its bindings (hadoofus_read/crc_streams.py),
the rejections its entry points decide without a GPU, the host combine against
the oracle's and zlib's, the kernels' metadata, and the fold and the reduce
(crc_streams_lookup.h) run on the CPU lane by lane against a byte-wise CRC
(tests/consumer/crc_streams_selftest.cpp, built with ASan/UBSan, nothing loaded
into Python)."""
import ctypes
import os
import re
import subprocess
import sys
import types
import zlib

import numpy as np
import pytest

from abi_symbols import c_functions as _c_functions, declared as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
DECLARED = {"hdfs_crc_streams_abi_version", "hdfs_crc_streams_last_error", "hdfs_crc_streams_block_crcs",
            "hdfs_crc_streams_file_checksum", "hdfs_crc_streams_combine", "hdfs_crc_streams_time"}
OWN = ["crc_streams_kernels.hip", "crc_streams.cpp", "crc_streams_internal.h", "crc_streams_lookup.h"]
SHARED = ["read_batch_layout.h", "read_batch_header.h", "read_batch_verify.h", "wire_fused_batch_lookup.h",
          "wire_fused_round.h", "crc32c_frame.h", "crc32c_outpkt.h", "crc32c_tables.h", "companion_support.h"]


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


@pytest.fixture(scope="module")
def libs():
    """(release library, CRC streams library), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.CRC_STREAMS_LIB


@pytest.fixture(scope="module")
def cs(libs):
    from hadoofus_read import crc_streams
    crc_streams.load()
    return crc_streams


# ---- the fold and the reduce on the CPU ---------------------------------------------------------
def test_crc_streams_selftest(tmp_path):
    exe = tmp_path / "crc_streams_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "crc_streams_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout


def test_the_lookup_header_compiles_without_hip(tmp_path):
    """Plain C++ with no include path but the header's own directory: integer
    arithmetic only, as the other lookup headers."""
    src = tmp_path / "l.cpp"
    src.write_text('#include "crc_streams_lookup.h"\n'
                   "using namespace hdfs_crc_streams;\n"
                   "int main() { const uint32_t P = 0x82f63b78u, x8 = 0x00800000u;  // x^8 needs no reduction\n"
                   "  const uint32_t pow2[2] = {x8, mulmod(x8, x8, P)};\n"
                   "  const Chunks c = chunks_of(10, 5120 - 511, 512);\n"
                   "  return (mulmod(kOne, 0x1234u, P) == 0x1234u && xpow8(pow2, 3, P) == mulmod(pow2[0], pow2[1], P) &&\n"
                   "          c.front == 9 && c.last_len == 1 && c.steps == 1 && c.pad == 55 && chunk_at(c, 0, 55) == 0 &&\n"
                   "          chunk_at(c, 0, 54) == kNoChunk && from_wire(0x04030201u) == 0x01020304u &&\n"
                   "          run_first(129, 1) == 3 && run_count(129, 0) == 3 && run_count(129, 1) == 2) ? 0 : 1; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0
    txt = open(os.path.join(ROOT, "hadoofus_amd", "csrc", "crc_streams_lookup.h")).read()
    assert re.findall(r"#include\s+(\S+)", txt) == ["<stdint.h>"]


# ---- build ---------------------------------------------------------------------------------
def test_build_produces_the_library_beside_the_others(libs):
    lib, slib = libs
    assert os.path.exists(slib) and os.path.basename(slib) == "libhadoofus_crc_streams.so"
    assert os.path.dirname(lib) == os.path.dirname(slib)


def test_build_tables():
    """The other tables are untouched; this library has a table of its own with
    rows of the same shape."""
    from hadoofus_amd import build
    assert len(build.COMPANIONS) == 9
    assert [r[0] for r in build.READ_LIBRARIES + build.PREAD_LIBRARIES + build.PREADV_LIBRARIES +
            build.DIGEST_LIBRARIES] == ["read_batch", "pread_batch", "preadv_batch", "md5crc_streams"]
    assert [r[0] for r in build.CRC_LIBRARIES] == ["crc_streams"]
    for stem, sources, headers, public in build.CRC_LIBRARIES:
        up = stem.upper()
        assert build.companion_lib(stem) == getattr(build, up + "_LIB")
        assert (sources, headers, public) == (getattr(build, up + "_SOURCES"), getattr(build, up + "_HEADERS"),
                                              getattr(build, up + "_PUBLIC"))
        assert f"{stem}_exports.map" in headers and f"hadoofus_{stem}.h" in public
        assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in sources + headers)
        assert all(os.path.exists(os.path.join(build.INCLUDE, f)) for f in public)
    assert build.CRC_STREAMS_SOURCES == ["crc_streams_kernels.hip", "crc_streams.cpp"]
    assert {"crc_streams_internal.h", "crc_streams_lookup.h", *SHARED} <= set(build.CRC_STREAMS_HEADERS)
    assert "libhadoofus_crc_streams.so" in build.__doc__ and "CRC_LIBRARIES" in build.__doc__


def test_sources_include_the_shared_code_and_copy_none():
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    code = lambda f: "\n".join(l for l in read(f).splitlines() if not l.lstrip().startswith("//"))  # noqa: E731
    kern, host, look = code(OWN[0]), code(OWN[1]), code(OWN[3])
    for inc in ("crc_streams_lookup.h", "read_batch_layout.h", "read_batch_header.h", "read_batch_verify.h",
                "wire_fused_batch_lookup.h", "crc32c_outpkt.h"):
        assert f'#include "{inc}"' in kern, inc
    for inc in ("companion_support.h", "hadoofus_crc_streams.h", "crc32c_tables.h", "read_batch_layout.h"):
        assert f'#include "{inc}"' in host, inc
    every = "".join(read(f) for f in sorted(os.listdir(build.CSRC)))
    for name in ("uint32_t write_of(", "uint32_t frag_of(", "void count_packet(", "bool seek_write("):
        assert every.count(name) == 1, name
    for f in OWN:
        src = code(f)
        # no framing arithmetic, no header composition, no comparison, no operator and no atomics of its own
        for name in ("probe_entry(At", "frame_step(const", "put_out_header(uint8_t", "put_header_proto(uint8_t",
                     "struct Unit {", "struct Gf2", "zeros_op(uint64_t", "atomic", "hdfs_crc32c_plan_",
                     "__builtin_amdgcn_raw_buffer", "hdfs_crc32c_composite_crcs"):
            assert name not in src, (f, name)
        for name in ("range_of(", "load8(", "load32(", "store32(", "verify_header(", "flag("):
            assert not re.search(r"(FUSED_DEV|HDFS_CRC_STREAMS_HD|inline) [\w:<> ]*\b" + re.escape(name), src), (f, name)
        for poly in ("82f63b78", "edb88320"):
            assert poly not in src.lower(), (f, poly)
    for name in ("probe_entry(", "prefix_regular(", "write_of(pk0, nw, g, k)", "verify_header(expect[wave], proto",
                 "hdfs_read_batch::flag(", "range_of(c0, 4u * ncrc)", "address_space(4)", "chunks_of(", "fold_step(",
                 "packet_crc(", "run_first(", "run_count(", "advance("):
        assert name in kern, name
    # the probe has no destination and wants no records
    assert "~uint64_t(0), proto, chunk_size, ctype, false," in kern
    # the arithmetic is the header's; the kernel file only loads, shuffles and stores
    for name in ("mulmod(", "xpow8(", "advance(", "chunks_of(", "chunk_at(", "fold_step(", "packet_crc(", "run_first("):
        assert re.search(r"HDFS_CRC_STREAMS_HD \w+ " + re.escape(name), look), name
        assert not re.search(r"\w+ " + re.escape(name) + r"[^;]*\{", kern), name
    assert "hip" not in look.lower().replace("__hipcc__", "").replace("__hip_device_compile__", "")
    # (through walk_pieces of read_batch_host.h, which also holds the run)
    shared = code("read_batch_host.h")
    assert host.count("walk_pieces(") == 1 and "hdfs_crc32c_parse_packets(" not in host
    assert shared.count("hdfs_crc32c_parse_packets(") == 1 and "hdfs_crc32c_read_packets" not in host
    for call in ("hipStreamSynchronize(", "hipEventRecord(", "hipEventElapsedTime("):
        assert call not in host, call
    assert '#include "read_batch_host.h"' in host and host.count("probed_run(") == 1
    assert shared.count("hipMemcpyHostToDevice, st)") == 1 and shared.count("hipMemcpyDeviceToHost, st)") == 1
    assert shared.count("hipMemcpyAsync(") == 2 and shared.count("hipStreamSynchronize(") == 1
    # no CRC arithmetic of a stream's chunks on the host: the host multiplies nothing, it applies the operator to blocks
    assert "mulmod(" not in host and "zeros_op(lens[i], poly).apply(acc)" in host


# ---- ABI -------------------------------------------------------------------------------------
def test_library_exports_exactly_its_header(libs):
    _, slib = libs
    assert _declared("hadoofus_crc_streams.h") == DECLARED
    funcs = _c_functions(slib)
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_crc_streams.h")).read()
    v = int(re.search(r"#define HDFS_CRC_STREAMS_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_CRC_STREAMS_{v}"}, funcs
    m = open(os.path.join(ROOT, "hadoofus_amd", "csrc", "crc_streams_exports.map")).read()
    assert "HADOOFUS_CRC_STREAMS_1 {" in m and "hdfs_crc_streams_*;" in m


def test_library_links_the_one_engine_and_no_companion(libs):
    lib, slib = libs
    dyn = subprocess.check_output(["readelf", "-d", slib], text=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert [n for n in needed if "hadoofus" in n] == ["libhadoofus_crc32c.so"] and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", slib], text=True)
    engine = sorted(l.split()[-1].split("@")[0] for l in und.splitlines() if "hdfs_" in l)
    assert engine == ["hdfs_crc32c_bound_device", "hdfs_crc32c_init", "hdfs_crc32c_last_error",
                      "hdfs_crc32c_parse_packets"]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert all(s in main for s in engine) and "hdfs_crc_streams" not in main


def test_header_says_what_is_not_verified():
    txt = open(os.path.join(ROOT, "include", "hadoofus_crc_streams.h")).read()
    assert "THE CRCS ARE NOT VERIFIED HERE" in txt and "offset_in_block == 0" in txt and "WHEN IT PAYS" in txt
    assert "COMPOSITE_CRC" in txt and "ORDERING" in txt and "@@" not in txt


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_crc_streams.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_crc_streams_entry) - 72 + "
                   "HDFS_CRC_STREAMS_ABI_VERSION - 1 + (int)HDFS_CRC_STREAMS_TIME_NONE + "
                   "HDFS_CRC_STREAMS_MAX_ENTRIES - 1024 + HDFS_CRC_STREAMS_PATH_KERNEL + "
                   "HDFS_CRC_STREAMS_PATH_FALLBACK - 1 + (int)sizeof(struct hdfs_crc_streams_file_checksum) - 24; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_read import crc_streams
    for S, cname, pinned in ((crc_streams.Entry, "hdfs_crc_streams_entry",
                              [72, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68]),  # pinned: the ABI of version 1
                             (crc_streams.FileChecksum, "struct hdfs_crc_streams_file_checksum",
                              [24, 0, 4, 8, 12, 16])):
        names = [f for f, _ in S._fields_]
        src = tmp_path / "l.c"
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_crc_streams.h"\n'
                       f'int main(void){{ printf("%zu", sizeof({cname}));\n' +
                       "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n in names) +
                       "return 0; }\n")
        exe = tmp_path / "l"
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                               "-o", str(exe)])
        got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
        assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
        assert got == pinned
    assert [f for f, _ in crc_streams.Entry._fields_] == \
        ["stream", "len", "consumed", "payload", "nchunks", "npkts", "offset_in_block", "rc", "path", "crc",
         "reserved"]


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "crc_streams_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "crc_streams_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_crc_streams", "-lhadoofus_crc32c"])
    assert exe.exists()


# ---- bindings ----------------------------------------------------------------------------------
def test_import_loads_nothing():
    code = ("import hadoofus_read as r\nfrom hadoofus_amd import abi\nfrom hadoofus_read import crc_streams as m\n"
            "assert abi._lib is None and m._lib is None and r.crc_streams is m\n"
            "assert callable(m.block_crcs) and callable(m.file_checksum) and callable(m.combine)\n"
            "assert callable(m.time) and callable(m.entry)\n"
            "for name in ('LIB_PATH', 'ABI_VERSION', 'load', 'check_abi', 'bind', '_check'):\n"
            "    assert hasattr(m, name), name\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_loading_is_cached_and_a_missing_library_is_refused(libs, cs, tmp_path):
    from hadoofus_amd import build
    lib = cs.load()
    assert lib is not None and cs.load() is lib and cs._lib is lib
    assert cs.LIB_PATH == build.CRC_STREAMS_LIB and lib.hdfs_crc_streams_abi_version() == cs.ABI_VERSION == 1
    missing = str(tmp_path / "libhadoofus_crc_streams.so")
    code = ("from hadoofus_read import crc_streams as m\n"
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
    from hadoofus_read import crc_streams as m
    other = types.SimpleNamespace(hdfs_crc_streams_abi_version=lambda: 2)
    with pytest.raises(ImportError) as e:
        m.check_abi(other)
    assert "crc streams library ABI version 2, bindings written for 1" in str(e.value)
    same = types.SimpleNamespace(hdfs_crc_streams_abi_version=lambda: 1)
    assert m.check_abi(same) is same


def test_entry_helper():
    from hadoofus_read import crc_streams as m

    class T:  # what companion.ptr takes of a torch tensor
        def data_ptr(self):
            return 0x1000

        def numel(self):
            return 10

        def element_size(self):
            return 1
    assert m.entry(0x1000, 10) == dict(stream_ptr=0x1000, nbytes=10) == m.entry(T())
    assert m.entry(T(), 4)["nbytes"] == 4 and m.entry() == dict(stream_ptr=None, nbytes=0)
    arr = m.entries([m.entry(0x1000, 10)] * 2)
    assert (arr[1].stream, arr[1].len, arr[1].nchunks, arr[1].crc) == (0x1000, 10, 0, 0)
    assert (m.MAX_ENTRIES, m.PATH_KERNEL, m.PATH_FALLBACK, m.TIME_NONE) == (1024, 0, 1, 0)


# ---- rejections that need no device ---------------------------------------------------------------
def _spoil(arr):
    for e in arr:
        e.rc, e.path, e.npkts, e.consumed, e.payload, e.nchunks, e.offset_in_block = 7, 7, 7, 7, 7, 7, 7
        e.crc, e.reserved = 7, 7


def _outs(arr):
    return [(e.rc, e.path, e.npkts, e.consumed, e.payload, e.nchunks, e.offset_in_block, e.crc, e.reserved)
            for e in arr]


def test_rejections_without_a_device(cs):
    lib = cs.load()
    good = [cs.entry(0x1000, 1000)] * 3  # never dereferenced: every call is decided by its arguments
    zero = (0,) * 9

    def call(batch=good, n=None, proto=2, chunk=512, ctype=2, arr=None, fc=False):
        arr = cs.entries(batch) if arr is None else arr
        _spoil(arr)
        n = len(batch) if n is None else n
        if fc:
            rc = lib.hdfs_crc_streams_file_checksum(arr, n, proto, chunk, ctype, None, ctypes.byref(cs.FileChecksum()))
        else:
            rc = lib.hdfs_crc_streams_block_crcs(arr, n, proto, chunk, ctype, None)
        return rc, arr, lib.hdfs_crc_streams_last_error().decode()
    for fc in (False, True):
        for kw, text in ((dict(proto=0), "proto"), (dict(proto=3), "proto"), (dict(ctype=3), "checksum type"),
                         (dict(ctype=-1), "checksum type"), (dict(ctype=0), "CRC32 or CRC32C"),
                         (dict(chunk=0), "chunk_size")):
            rc, arr, err = call(fc=fc, **kw)
            assert rc == EINVAL and "entry 0" in err and text in err and "device" not in err, (kw, err)
            assert _outs(arr) == [zero] * 3, kw
        rc, _, err = call(n=0, fc=fc)
        assert rc == EINVAL and "no entries" in err and "entry 0" in err
        rc, _, err = call(n=cs.MAX_ENTRIES + 1, arr=(cs.Entry * (cs.MAX_ENTRIES + 1))(), fc=fc)
        assert rc == EINVAL and "1025 entries" in err and "entry 1024" in err
        rc, arr, err = call([good[0], cs.entry(None, 5)], fc=fc)
        assert rc == EINVAL and "entry 1" in err and "stream" in err and _outs(arr) == [zero] * 2
    assert lib.hdfs_crc_streams_block_crcs(None, 3, 2, 512, 2, None) == EINVAL
    assert lib.hdfs_crc_streams_file_checksum(None, 3, 2, 512, 2, None, None) == EINVAL
    with pytest.raises(cs.abi.CRC32CError) as e:  # through the bindings: the call's own refusal raises
        cs.block_crcs(good, proto=7)
    assert e.value.code == EINVAL and "proto" in str(e.value)
    with pytest.raises(cs.abi.CRC32CError):
        cs.file_checksum(good, ctype=0)


def test_timing_argument_errors(cs):
    lib, out = cs.load(), ctypes.c_double(5)
    one = [cs.entry(0x1000, 100)]

    def call(flags=0, iters=1, res=ctypes.byref(out), proto=2):
        rc = lib.hdfs_crc_streams_time(cs.entries(one), 1, proto, 512, 2, flags, iters, res)
        return rc, lib.hdfs_crc_streams_last_error()
    # every one decided before a device is asked (0x1000 is no device memory: going on would say so)
    for kw in (dict(iters=0), dict(iters=-3), dict(res=None)):
        rc, err = call(**kw)
        assert rc == EINVAL and b"iters" in err and b"device" not in err, (kw, err)
    assert call(proto=7)[0] == EINVAL
    for flags in (1, 2, 1 << 8, 1 << 31):
        rc, err = call(flags=flags)
        assert rc == EINVAL and b"flags" in err and b"device" not in err, (flags, err)
    assert out.value == 0  # set to 0 by every call that was given it


def test_last_error_text_is_its_own(cs):
    from hadoofus_read import md5crc_streams as ms
    ml, lib = ms.load(), cs.load()
    assert ml.hdfs_md5crc_streams_block_digests(ms.entries([ms.entry(0x1000, 5)]), 1, 7, 512, 2, None) == EINVAL
    before = ml.hdfs_md5crc_streams_last_error()
    assert lib.hdfs_crc_streams_block_crcs(cs.entries([cs.entry(0x1000, 5)]), 1, 2, 0, 2, None) == EINVAL
    assert lib.hdfs_crc_streams_last_error() == b"entry 0: chunk_size 0"
    assert ml.hdfs_md5crc_streams_last_error() == before == b"entry 0: proto must be 1 or 2"


# ---- the host combine ----------------------------------------------------------------------------------
def test_combine_against_the_oracle_and_zlib(cs, oracle):
    """hdfs_crc_streams_combine touches no device: pieces of unequal length, an
    empty one among them, against oracle.combine and the oracle's CRC32C of the
    concatenation, and against zlib.crc32 for CRC32."""
    rng = np.random.default_rng(24)
    lens = [1, 0, 513, 70000, 3, 65536, 4096, 131072 + 7]
    pieces = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    crcs = [oracle.crc32c(0, p) for p in pieces]
    acc = 0
    for k, (c, n) in enumerate(zip(crcs, lens)):
        acc = oracle.combine(acc, c, n)
        assert cs.combine(crcs[:k + 1], lens[:k + 1]) == acc == oracle.crc32c(0, b"".join(pieces[:k + 1])), k
    z = [zlib.crc32(p) for p in pieces]
    for k in range(len(lens) + 1):
        assert cs.combine(z[:k], lens[:k], ctype=1) == zlib.crc32(b"".join(pieces[:k])), k
    assert cs.combine([], []) == 0
    # lengths past 2^32: Z_n composes, Z_a(Z_b(c)) == Z_(a + b)(c)
    big = (1 << 39) + 12345
    assert cs.combine([0xDEADBEEF, 0], [0, big]) == cs.combine([0xDEADBEEF, 0, 0], [0, 1 << 39, 12345])
    assert cs.combine([0xDEADBEEF, 0], [0, 5]) == oracle.combine(0xDEADBEEF, 0, 5)
    lib, out = cs.load(), ctypes.c_uint32(9)
    c2, l2 = (ctypes.c_uint32 * 2)(1, 2), (ctypes.c_uint64 * 2)(3, 4)
    for args in ((None, l2, 2, 2, ctypes.byref(out)), (c2, None, 2, 2, ctypes.byref(out)), (c2, l2, 2, 2, None),
                 (c2, l2, 2, 0, ctypes.byref(out)), (c2, l2, 2, 3, ctypes.byref(out))):
        assert lib.hdfs_crc_streams_combine(*args) == EINVAL, args
        assert b"combine" in lib.hdfs_crc_streams_last_error()
    assert out.value == 0


# ---- the kernels' metadata --------------------------------------------------------------------------
def test_kernel_metadata(tmp_path):
    """hipcc -S of the kernel file: no kernel has a private segment or a vector
    register spill, the fold and the reduce spill no scalar register either; the
    probe -- the read batch's probe_entry as it stands, one workgroup, run once a
    call -- keeps up to 59 scalar registers in lanes of vector registers
    (v_writelane, no memory), as the other libraries' probes do, and no more
    than that; the fold is four waves with a 64-byte expected header each
    and nothing else in LDS, the reduce one wave a workgroup without LDS, the
    probe one workgroup of 1 024 with its two count arrays."""
    from hadoofus_amd import build
    asm = tmp_path / "crc_streams_kernels.s"
    subprocess.check_call([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only",
                           "-S", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
                           os.path.join(build.CSRC, "crc_streams_kernels.hip"), "-o", str(asm)])
    txt = asm.read_text()
    meta = {}
    for block in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(
            r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|"
            r"max_flat_workgroup_size):\s+(\d+)", block)}
    assert len(meta) == 3
    get = lambda part: next(v for k, v in meta.items() if part in k)  # noqa: E731
    probe, fold, reduce_ = (get(k) for k in ("probe_streams_kernel", "fold_packets_kernel", "reduce_entries_kernel"))
    for k in (probe, fold, reduce_):
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert fold["sgpr_spill_count"] == 0 and reduce_["sgpr_spill_count"] == 0
    assert probe["sgpr_spill_count"] <= PROBE_SGPR_SPILLS, probe
    assert probe["group_segment_fixed_size"] == 8192 and probe["max_flat_workgroup_size"] == 1024
    assert probe["vgpr_count"] <= 128  # 1024 threads are 16 waves, four a SIMD
    assert fold["group_segment_fixed_size"] == 4 * 64 and fold["max_flat_workgroup_size"] == 256
    assert fold["vgpr_count"] <= 128 and fold["sgpr_count"] <= 102
    assert reduce_["group_segment_fixed_size"] == 0 and reduce_["max_flat_workgroup_size"] == 64
    # the fold reads the streams through buffer ranges only; no kernel has an atomic or touches scratch
    body = txt.split("fold_packets_kernel", 2)[-1].split(".end_amdhsa_kernel")[0]
    assert "buffer_load_dword" in body and "flat_load" not in body
    assert "atomic" not in txt and "scratch_" not in txt


PROBE_SGPR_SPILLS = 59  # scalar registers probe_streams_kernel keeps in vector lanes; none of them in memory
