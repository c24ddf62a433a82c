"""CPU tests of the read batch library (include/hadoofus_read_batch.h): its
build beside the companions, its ABI, its bindings (the package hadoofus_read),
the rejections its entry points decide without a GPU, the kernels' metadata,
and the probe's arithmetic (read_batch_layout.h) run on the CPU against a
brute-force frame_step walk (tests/consumer/read_batch_selftest.cpp, built
with ASan/UBSan, nothing loaded into Python)."""
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
DECLARED = {"hdfs_read_batch_abi_version", "hdfs_read_batch_last_error", "hdfs_read_batch_read_blocks",
            "hdfs_read_batch_time"}
NINE = ["md5crc", "writev", "wire", "wire_batch", "wirev", "wire_fused", "wire_fused_batch", "wirev_fused",
        "wirev_fused_batch"]
SHARED = ["wire_fused_round.h", "wire_fused_crc.h", "wire_fused_tables.h", "wire_fused_host.h",
          "wire_fused_batch_lookup.h", "crc32c_frame.h", "crc32c_outpkt.h", "companion_support.h"]


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


@pytest.fixture(scope="module")
def libs():
    """(release library, read batch library), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.READ_BATCH_LIB


@pytest.fixture(scope="module")
def rb(libs):
    from hadoofus_read import read_batch
    read_batch.load()
    return read_batch


# ---- the probe's arithmetic on the CPU -----------------------------------------------------
def test_read_batch_selftest(tmp_path):
    exe = tmp_path / "read_batch_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "read_batch_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout


# ---- build ---------------------------------------------------------------------------------
def test_build_produces_the_library_beside_the_others(libs):
    lib, rlib = libs
    assert os.path.exists(rlib) and os.path.basename(rlib) == "libhadoofus_read_batch.so"
    assert os.path.dirname(lib) == os.path.dirname(rlib)


def test_build_tables():
    """The nine companions are untouched; the read side has a table of its own
    with rows of the same shape."""
    from hadoofus_amd import build
    assert [c[0] for c in build.COMPANIONS] == NINE
    assert [r[0] for r in build.READ_LIBRARIES] == ["read_batch"]
    for stem, sources, headers, public in build.READ_LIBRARIES:
        up = stem.upper()
        assert build.companion_lib(stem) == getattr(build, up + "_LIB")
        assert (sources, headers, public) == (getattr(build, up + "_SOURCES"), getattr(build, up + "_HEADERS"),
                                              getattr(build, up + "_PUBLIC"))
        assert f"{stem}_exports.map" in headers and f"hadoofus_{stem}.h" in public
        assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in sources + headers)
    assert build.READ_BATCH_SOURCES == ["read_batch_kernels.hip", "read_batch.cpp"]
    assert {"read_batch_internal.h", "read_batch_layout.h", *SHARED} <= set(build.READ_BATCH_HEADERS)
    assert "libhadoofus_read_batch.so" in build.__doc__ and build.ARCH == "gfx950"


def test_sources_include_the_shared_code_and_copy_none():
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    own = ["read_batch_kernels.hip", "read_batch.cpp", "read_batch_internal.h", "read_batch_layout.h"]
    kern, host, lay = read(own[0]), read(own[1]), read(own[3])
    for inc in ("wire_fused_round.h", "wire_fused_batch_lookup.h", "crc32c_frame.h", "crc32c_outpkt.h",
                "read_batch_layout.h"):
        assert f'#include "{inc}"' in kern, inc
    for inc in ("companion_support.h", "read_batch_host.h", "wire_fused_host.h", "wire_fused_tables.h",
                "read_batch_layout.h"):
        assert f'#include "{inc}"' in host, inc
    helpers = ["range_of(", "load16(", "store16(", "store32(", "load8(", "store8(", "fold8(", "transpose(", "unit_of(",
               "load_round(", "store_round(", "crc_round(", "header(", "ragged_chunk(", "ragged_finish(",
               "fill_image("]
    for f in own:
        src = "\n".join(l for l in read(f).splitlines() if not l.lstrip().startswith("//"))
        for name in helpers:
            assert not re.search(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), src), (f, name)
        for name in ("uint32_t write_of(", "uint32_t frag_of(", "void count_packet(", "bool seek_write(",
                     "build_layout(", "struct Unit {", "permlane", "atomic", "hdfs_crc32c_plan_"):
            assert name not in src, (f, name)
        for poly in ("82f63b78", "edb88320"):
            assert poly not in src.lower(), (f, poly)
    for name in ("write_of(pk0, nw, g, k)", "load_round(", "store_round(", "frame_step", "probe_entry(",
                 "prefix_regular(", "address_space(4)", "put_out_header("):
        assert name in kern or name in lay, name
    assert "frame_step(" in lay and "hipMalloc" not in lay and "hipLaunch" not in lay and "hipMemcpy" not in lay
    # the run, the outcomes and the main library's read are the shared header's, once for the six libraries
    shared = "\n".join(l for l in read("read_batch_host.h").splitlines() if not l.lstrip().startswith("//"))
    for call in ("hipMemcpyAsync(", "hipStreamSynchronize(", "hipEventRecord(", "hipEventElapsedTime(",
                 "hdfs_crc32c_read_packets("):
        assert call not in host, call
    assert '#include "read_batch_host.h"' in host and host.count("probed_run(") == 1
    assert "HDFS_CRC32C_READ_ALL, &iov, 1" in host and host.count("read_unlimited(") == 1 and shared.count("hdfs_crc32c_read_packets(") == 2  # own room; grown
    assert shared.count("hipMemcpyHostToDevice, st)") == 1 and shared.count("hipMemcpyDeviceToHost, st)") == 1
    assert shared.count("hipMemcpyAsync(") == 2 and shared.count("hipStreamSynchronize(") == 1
    # the overlap check is the one sweep of companion_support.h; this file defines none
    assert host.count("check_overlaps(") == 1 and "struct Span" not in host and "far_d" not in host


# ---- ABI -------------------------------------------------------------------------------------
def test_library_exports_exactly_its_header(libs):
    _, rlib = libs
    assert _declared("hadoofus_read_batch.h") == DECLARED
    funcs = _c_functions(rlib)
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_read_batch.h")).read()
    v = int(re.search(r"#define HDFS_READ_BATCH_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_READ_BATCH_{v}"}, funcs


def test_library_links_the_one_engine_through_four_calls(libs):
    lib, rlib = libs
    dyn = subprocess.check_output(["readelf", "-d", rlib], text=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", dyn)
    assert [n for n in needed if "hadoofus" in n] == ["libhadoofus_crc32c.so"] and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", rlib], text=True)
    engine = sorted(l.split()[-1].split("@")[0] for l in und.splitlines() if "hdfs_" in l)
    assert engine == ["hdfs_crc32c_bound_device", "hdfs_crc32c_init", "hdfs_crc32c_last_error",
                      "hdfs_crc32c_read_packets"]
    main = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert all(s in main for s in engine) and "hdfs_read_batch" not in main


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_read_batch.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_read_batch_entry) - 64 + HDFS_READ_BATCH_ABI_VERSION - 1 + "
                   "(int)HDFS_READ_BATCH_TIME_GROUPS(0) + HDFS_READ_BATCH_MAX_ENTRIES - 1024 + "
                   "HDFS_READ_BATCH_PATH_KERNEL + HDFS_READ_BATCH_PATH_FALLBACK - 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_read import read_batch
    S = read_batch.Entry
    names = [f for f, _ in S._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_read_batch.h"\n'
                   'int main(void){ printf("%zu", sizeof(hdfs_read_batch_entry));\n' +
                   "".join(f'printf(" %zu", offsetof(hdfs_read_batch_entry, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    assert got == [64, 0, 8, 16, 24, 32, 40, 48, 56, 60]  # pinned: the ABI of version 1


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "read_batch_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "read_batch_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_read_batch", "-lhadoofus_crc32c"])
    assert exe.exists()


# ---- bindings ----------------------------------------------------------------------------------
def test_import_loads_nothing():
    code = ("import hadoofus_read as r\nfrom hadoofus_amd import abi\nfrom hadoofus_read import read_batch\n"
            "assert abi._lib is None and read_batch._lib is None\n"
            "assert callable(r.read_blocks) and callable(r.time) and callable(r.entry)\n"
            "for name in ('LIB_PATH', 'ABI_VERSION', 'load', 'check_abi', 'bind', '_check'):\n"
            "    assert hasattr(read_batch, name), name\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_the_package_of_the_nine_is_untouched():
    import pkgutil

    import hadoofus_amd
    names = {m.name for m in pkgutil.iter_modules(hadoofus_amd.__path__)}
    assert names == set(NINE) | {"abi", "build", "companion", "shard"}


def test_loading_is_cached_and_a_missing_library_is_refused(libs, rb, tmp_path):
    from hadoofus_amd import build
    lib = rb.load()
    assert lib is not None and rb.load() is lib and rb._lib is lib
    assert rb.LIB_PATH == build.READ_BATCH_LIB and lib.hdfs_read_batch_abi_version() == rb.ABI_VERSION == 1
    missing = str(tmp_path / "libhadoofus_read_batch.so")
    code = ("from hadoofus_read import read_batch as m\n"
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
    from hadoofus_read import read_batch as m
    other = types.SimpleNamespace(hdfs_read_batch_abi_version=lambda: 2)
    with pytest.raises(ImportError) as e:
        m.check_abi(other)
    assert "read batch library ABI version 2, bindings written for 1" in str(e.value)
    same = types.SimpleNamespace(hdfs_read_batch_abi_version=lambda: 1)
    assert m.check_abi(same) is same


def test_entry_helper():
    from hadoofus_read import read_batch as m

    class T:  # what companion.ptr takes of a torch tensor
        def __init__(self, p, n):
            self.p, self.n = p, n

        def data_ptr(self):
            return self.p

        def numel(self):
            return self.n

        def element_size(self):
            return 1
    assert m.entry(0x1000, 10, 0x2000, 20) == dict(stream_ptr=0x1000, nbytes=10, dst_ptr=0x2000, dst_cap=20)
    assert m.entry(T(0x1000, 10), None, T(0x2000, 20)) == dict(stream_ptr=0x1000, nbytes=10, dst_ptr=0x2000, dst_cap=20)
    assert m.entry(T(0x1000, 10), 4, T(0x2000, 20), 8)["nbytes"] == 4
    arr = m.entries([m.entry(0x1000, 10, 0x2000, 20)] * 2)
    assert (arr[1].stream, arr[1].len, arr[1].dst, arr[1].dst_cap) == (0x1000, 10, 0x2000, 20)
    assert m.time_groups(3) == 3 << 8 and m.MAX_GROUPS == 1024 and m.MAX_ENTRIES == 1024


# ---- rejections that need no device ---------------------------------------------------------------
def test_rejections_without_a_device(rb):
    from hadoofus_amd.abi import Packet
    lib = rb.load()
    pk = (Packet * 8)()
    before = bytes(pk)
    good = [rb.entry(0x1000, 1000, 0x100000, 1000)] * 3  # never dereferenced: every call is decided by its arguments

    def call(batch=good, n=None, proto=2, cs=512, ctype=2, arr=None):
        arr = rb.entries(batch) if arr is None else arr
        for e in arr:
            e.rc, e.path, e.npkts, e.consumed, e.delivered = 7, 7, 7, 7, 7
        rc = lib.hdfs_read_batch_read_blocks(arr, len(batch) if n is None else n, proto, cs, ctype, pk, 2, None)
        return rc, arr, lib.hdfs_read_batch_last_error().decode()
    for kw, text in ((dict(proto=0), "proto"), (dict(proto=3), "proto"), (dict(ctype=3), "checksum type"),
                     (dict(ctype=-1), "checksum type"), (dict(ctype=0), "CRC32 or CRC32C"),
                     (dict(cs=0), "chunk_size")):
        rc, arr, err = call(**kw)
        assert rc == EINVAL and "entry 0" in err and text in err and b"device" not in err.encode(), (kw, err)
        assert [(e.rc, e.npkts, e.consumed, e.delivered, e.path) for e in arr] == [(0, 0, 0, 0, rb.PATH_FALLBACK)] * 3
    rc, _, err = call(n=0)
    assert rc == EINVAL and "no entries" in err
    rc, _, err = call(n=rb.MAX_ENTRIES + 1, arr=(rb.Entry * (rb.MAX_ENTRIES + 1))())
    assert rc == EINVAL and "1025 entries" in err and "1024" in err
    assert lib.hdfs_read_batch_read_blocks(None, 3, 2, 512, 2, pk, 2, None) == EINVAL
    rc, _, err = call([good[0], rb.entry(None, 5, 0x2000, 5)])
    assert rc == EINVAL and "entry 1" in err and "stream" in err
    rc, _, err = call([good[0], good[0], rb.entry(0x1000, 5, None, 5)])
    assert rc == EINVAL and "entry 2" in err and "destination" in err
    assert bytes(pk) == before
    with pytest.raises(rb.abi.CRC32CError) as e:  # through the bindings: the call's own refusal raises
        rb.read_blocks(good, proto=7)
    assert e.value.code == EINVAL and "proto" in str(e.value)


def test_timing_argument_errors(rb):
    lib, ms = rb.load(), ctypes.c_double(5)
    one = [rb.entry(0x1000, 100, 0x2000, 100)]

    def call(flags=0, iters=1, out=ctypes.byref(ms), proto=2):
        rc = lib.hdfs_read_batch_time(rb.entries(one), 1, proto, 512, 2, flags, iters, out)
        return rc, lib.hdfs_read_batch_last_error()
    # every one decided before a device is asked (0x1000 is no device memory: going on would say so)
    for kw in (dict(iters=0), dict(iters=-3), dict(out=None)):
        rc, err = call(**kw)
        assert rc == EINVAL and b"iters" in err and b"device" not in err, (kw, err)
    assert call(proto=7)[0] == EINVAL
    for flags in (rb.time_groups(rb.MAX_GROUPS + 1), rb.time_groups(1 << 23), 1, rb.time_groups(2) | 4):
        rc, err = call(flags=flags)
        assert rc == EINVAL and b"workgroups" in err, (flags, err)
    assert ms.value == 0  # set to 0 by every call that was given it


def test_last_error_text_is_its_own(rb):
    from hadoofus_amd import wire_fused_batch as fb
    bl, lib = fb.load(), rb.load()
    assert bl.hdfs_wire_fused_batch_layout(fb.entries([fb.write(nbytes=1)], True), 1, 7, 2,
                                           ctypes.byref(fb.Totals())) == EINVAL
    before = bl.hdfs_wire_fused_batch_last_error()
    assert lib.hdfs_read_batch_read_blocks(rb.entries([rb.entry(0x1000, 5, 0x2000, 5)]), 1, 2, 0, 2, None, 0,
                                           None) == EINVAL
    assert lib.hdfs_read_batch_last_error() == b"entry 0: chunk_size 0"
    assert bl.hdfs_wire_fused_batch_last_error() == before == b"entry 0: proto must be 1 or 2"


# ---- the kernels' metadata --------------------------------------------------------------------------
def test_kernel_metadata(tmp_path):
    """hipcc -S of the kernel file: neither kernel has a private segment (no
    scratch), the main kernel's LDS is all dynamic (the table image and the
    expected header) and its registers leave room for 16 waves a workgroup,
    the probe's LDS is its two count arrays."""
    from hadoofus_amd import build
    asm = tmp_path / "read_batch_kernels.s"
    subprocess.check_call([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only",
                           "-S", f"-I{build.INCLUDE}", f"-I{build.CSRC}",
                           os.path.join(build.CSRC, "read_batch_kernels.hip"), "-o", str(asm)])
    txt = asm.read_text()
    meta = {}
    for block in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(
            r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|"
            r"max_flat_workgroup_size):\s+(\d+)", block)}
    probe = next(v for k, v in meta.items() if "probe_kernel" in k)
    main = next(v for k, v in meta.items() if "unframe_fused_batch_kernel" in k)
    assert len(meta) == 2
    assert main["private_segment_fixed_size"] == 0 and main["vgpr_spill_count"] == 0
    assert main["group_segment_fixed_size"] == 0 and main["max_flat_workgroup_size"] == 1024
    assert (main["vgpr_count"], main["sgpr_count"]) == MAIN_REGISTERS
    assert probe["private_segment_fixed_size"] == 0 and probe["vgpr_spill_count"] == 0
    assert probe["group_segment_fixed_size"] == 8192 and probe["max_flat_workgroup_size"] == 1024
    assert probe["vgpr_count"] <= 128  # 1024 threads are 16 waves, four a SIMD


MAIN_REGISTERS = (73, 106)  # VGPRs, SGPRs of unframe_fused_batch_kernel
