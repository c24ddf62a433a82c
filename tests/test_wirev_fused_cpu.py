"""CPU tests of the fused gather-wire companion library
(include/hadoofus_wirev_fused.h): its build and ABI, the host layout and the
size query's packet records against the oracle's compose_packets of the
fragments' concatenation and against the two-pass gather library, the round
counts against a few lines of Python, the rejections the entry points decide
without a GPU, and the kernel's lookup and the round counting run on the CPU
against a linear scan and a brute-force model
(tests/consumer/wirev_fused_selftest.cpp, built with ASan/UBSan, nothing loaded
into Python).  Everything is bit-exact."""
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
DECLARED = {"hdfs_wirev_fused_abi_version", "hdfs_wirev_fused_last_error", "hdfs_wirev_fused_compose_packets",
            "hdfs_wirev_fused_layout", "hdfs_wirev_fused_time"}
# the seven other companions and their version nodes, as their own tests pin them
OTHERS = {"md5crc": "HADOOFUS_MD5CRC_1", "writev": "HADOOFUS_WRITEV_1", "wire": "HADOOFUS_WIRE_1",
          "wire_batch": "HADOOFUS_WIRE_BATCH_1", "wirev": "HADOOFUS_WIREV_1", "wire_fused": "HADOOFUS_WIRE_FUSED_1",
          "wire_fused_batch": "HADOOFUS_WIRE_FUSED_BATCH_1"}


@pytest.fixture(scope="module")
def libs():
    """(release library, fused gather-wire companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.WIREV_FUSED_LIB


@pytest.fixture(scope="module")
def wvf(libs):
    from hadoofus_amd import wirev_fused
    wirev_fused.load()
    return wirev_fused


# ---- the kernel's lookup and the round counting on the CPU -------------------------------
def test_wirev_fused_selftest(tmp_path):
    exe = tmp_path / "wirev_fused_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "hadoofus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "consumer", "wirev_fused_selftest.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("0 failures"), p.stdout


# ---- layout and records against the oracle and the two-pass gather library ----------------
LENS = [0, 1, 287, 511, 512, 513, 65536, 65537, 3 * 65536 + 123]  # test_wirev_cpu.py's
DATA = np.random.default_rng(80).integers(0, 256, max(LENS), dtype=np.uint8)
SPLITS = [1, 2, 7]


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


def round_counts(lens, recs):
    """rounds, seamed_rounds, seamed_ragged, max_frags_per_round from the
    definition: a packet's full chunks in rounds of 4 KiB from its first data
    byte, then its chunk shorter than 512 B; the fragments under a range are
    the non-empty ones that share a byte with it."""
    ends = np.cumsum(lens)
    starts = ends - np.asarray(lens)
    under = lambda a, b: int(np.count_nonzero((starts < b) & (ends > a)))  # noqa: E731
    rounds = seamed = ragged = most = 0
    for p in recs:
        a, full = p["data_off"], p["data_len"] // 512 * 512
        for r in range(0, full, 4096):
            k = under(a + r, a + min(full, r + 4096))
            rounds, seamed, most = rounds + 1, seamed + (k > 1), max(most, k)
        if p["data_len"] % 512:
            ragged += under(a + full, a + p["data_len"]) > 1
    return rounds, seamed, ragged, most


@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("proto", [1, 2])
@pytest.mark.parametrize("off", [0, 4321])
def test_layout_and_size_query_match_the_oracle_and_the_gather_library(wvf, oracle, off, proto, ctype, finish):
    from hadoofus_amd import wirev
    for n in LENS:
        want_len, want, nchunks = expected(oracle, n, off, 11, proto, ctype, finish)
        hb = 25 if proto == 1 else 31
        for k in SPLITS:
            lens = split(n, k, 1000 * k + n % 997)
            assert len(lens) == k and sum(lens) == n
            got_len, got = wvf.packet_records(lens, off, 11, proto, ctype, finish)
            assert got_len == want_len and len(got) == len(want), (n, k)
            for a, b in zip(got, want):  # field by field
                assert set(a) == set(b) and all(a[f] == b[f] for f in b), (n, k, a, b)
            info = wvf.layout(lens, off, proto, ctype, finish)
            rounds, seamed, ragged, most = round_counts(lens, want)
            assert info == {"npkts": len(want), "nchunks": nchunks, "wire_len": want_len,
                            "nfrags": sum(1 for x in lens if x), "rounds": rounds, "seamed_rounds": seamed,
                            "seamed_ragged": ragged, "packet_stride": hb + (512 if ctype else 0) + 65536,
                            "header_bytes": hb, "head_bytes": min(n, 512 - off % 512) if n and off % 512 else 0,
                            "max_frags_per_round": most}, (n, k)
            two = wirev.layout(lens, off, proto, ctype, finish)  # the two-pass gather library's common fields
            for f in ("npkts", "nchunks", "wire_len", "nfrags", "packet_stride", "header_bytes", "head_bytes"):
                assert info[f] == two[f], (n, k, f)
            assert wirev.packet_records(lens, off, 11, proto, ctype, finish) == (got_len, got)


def test_round_counts_of_known_splits(wvf):
    """Counts worked out by hand."""
    n = 2 * 65536 + 700  # at 4321: packets of 287, 65536, 65536 and 413 bytes
    f = lambda lens, off=4321: tuple(wvf.layout(lens, off, 2, 2, True)[k] for k in  # noqa: E731
                                     ("rounds", "seamed_rounds", "seamed_ragged", "max_frags_per_round"))
    assert f([n]) == (32, 0, 0, 1)
    assert f([287, n - 287]) == (32, 0, 0, 1)          # the seam between the short packet and the next
    assert f([286, n - 286]) == (32, 0, 1, 1)          # inside the short packet's chunk
    assert f([287 + 4096, n - 287 - 4096]) == (32, 0, 0, 1)  # between two rounds
    assert f([287 + 4097, n - 287 - 4097]) == (32, 1, 0, 2)
    assert f([287 + 65536, 65536, 413]) == (32, 0, 0, 1)      # on the packet boundaries
    assert f([287 + 65536 + 65536 + 1, 412]) == (32, 0, 1, 1)  # inside the write's last chunk
    assert f([1] * 1300) == (1, 1, 2, 512)                  # 287, one full chunk, 501
    assert f([1] * 1300, 0) == (1, 1, 1, 1024)              # two full chunks, 276
    # 9 full chunks and 488 bytes, seams at 4000 and 4700; empty fragments are no fragments
    assert f([0, 4000, 0, 0, 700, 0, 396], 0) == (2, 1, 1, 2)
    assert f([]) == (0, 0, 0, 0) and f([0, 0]) == (0, 0, 0, 0)


def test_layout_of_a_large_write(wvf):
    """128 MiB in 33 555 fragments of 4 000 bytes: every round is seamed."""
    n = 128 << 20
    lens = [4000] * (n // 4000) + [n % 4000]
    info = wvf.layout(lens, 4321, 2, 2, True)
    assert info["nfrags"] == 33555 and info["npkts"] == 1 + 2047 + 1 + 1  # 287 bytes, full packets, 65 249 bytes, finish
    assert info["rounds"] == info["seamed_rounds"] == 2048 * 16 and info["max_frags_per_round"] == 3


# ---- rejections that need no device ---------------------------------------------
def test_argument_errors_are_einval_without_a_device(wvf):
    from hadoofus_amd.abi import IoVec, OutPacket
    lib = wvf.load()
    pk = (OutPacket * 4)()
    before = bytes(pk)
    npk, wl = ctypes.c_size_t(0), ctypes.c_uint64(0)
    fake = 0x1000  # never dereferenced: every call below is decided by its arguments

    def call(lens=(600, 400), bases=None, cnt=None, off=0, proto=2, ctype=2, wire=fake, cap=1 << 20, maxp=4,
             null_list=False):
        bases = bases if bases is not None else [fake + 0x10000 * (i + 1) for i in range(len(lens))]
        vec = (IoVec * max(1, len(lens)))(*[IoVec(b, n) for b, n in zip(bases, lens)])
        npk.value, wl.value = 77, 77
        return lib.hdfs_wirev_fused_compose_packets(None if null_list else vec, len(lens) if cnt is None else cnt,
                                                    off, 0, proto, ctype, 0, wire, cap, pk, maxp, ctypes.byref(npk),
                                                    ctypes.byref(wl), None)
    err = lib.hdfs_wirev_fused_last_error
    for kw in (dict(off=-1), dict(proto=0), dict(proto=3), dict(ctype=3), dict(ctype=-1), dict(cnt=-1),
               dict(null_list=True)):
        assert call(**kw) == EINVAL and err() and (npk.value, wl.value) == (0, 0), kw
    assert call(lens=(1 << 39, (1 << 39) + 1)) == EINVAL and b"1 TiB" in err()
    assert call(lens=(0, 1 << 62, 1)) == EINVAL and b"fragment 2" in err()
    assert call(bases=[fake, None]) == EINVAL and b"fragment 1" in err() and (npk.value, wl.value) == (1, 1039)
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


def test_layout_and_timing_argument_errors(wvf):
    from hadoofus_amd.abi import IoVec
    lib = wvf.load()
    info = wvf.LayoutInfo()
    lens = (ctypes.c_uint64 * 2)(10, 20)
    assert lib.hdfs_wirev_fused_layout(lens, 2, 0, 2, 2, 0, None) == EINVAL
    assert lib.hdfs_wirev_fused_layout(None, 2, 0, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_fused_layout(lens, -1, 0, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_fused_layout(lens, 2, -1, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_fused_layout(lens, 2, 0, 5, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_fused_layout(lens, 2, 0, 2, 9, 0, ctypes.byref(info)) == EINVAL
    big = (ctypes.c_uint64 * 2)(1 << 40, 1)
    assert lib.hdfs_wirev_fused_layout(big, 2, 0, 2, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_wirev_fused_layout(None, 0, 0, 2, 2, 1, ctypes.byref(info)) == 0
    assert info.npkts == 1 and info.nfrags == 0 and info.rounds == 0
    ms = ctypes.c_double(0)
    vec = (IoVec * 1)(IoVec(0x1000, 10))

    def call(flags=0, iters=1, out=ctypes.byref(ms), wire=0x2000, cap=100, proto=2):
        rc = lib.hdfs_wirev_fused_time(vec, 1, 0, proto, 2, 0, wire, cap, flags, iters, out)
        return rc, lib.hdfs_wirev_fused_last_error()
    # every one decided before a device is asked (0x1000 is no device memory: going on would say so)
    for kw in (dict(iters=0), dict(out=None), dict(wire=None), dict(cap=44),dict(proto=7)):
        rc, err = call(**kw)
        assert rc == EINVAL and err and b"device" not in err, (kw, err)
    for flags in (wvf.time_groups(wvf.MAX_GROUPS + 1), wvf.time_groups(1 << 23), 1, wvf.time_groups(2) | 4):
        rc, err = call(flags=flags)
        assert rc == EINVAL and b"workgroups" in err, (flags, err)


# ---- build and ABI ------------------------------------------------------------------
def test_build_produces_the_library_beside_the_others(libs):
    lib, flib = libs
    from hadoofus_amd import build
    assert os.path.exists(flib) and os.path.basename(flib) == "libhadoofus_wirev_fused.so"
    assert os.path.dirname(lib) == os.path.dirname(flib)
    for other in (build.MD5CRC_LIB, build.WRITEV_LIB, build.WIRE_LIB, build.WIRE_BATCH_LIB, build.WIREV_LIB,
                  build.WIRE_FUSED_LIB, build.WIRE_FUSED_BATCH_LIB):
        assert os.path.exists(other) and os.path.dirname(other) == os.path.dirname(flib), other


def test_build_lists_sources_and_headers():
    from hadoofus_amd import build
    assert build.WIREV_FUSED_SOURCES == ["wirev_fused_kernels.hip", "wirev_fused.cpp"]
    assert {"wirev_fused_internal.h", "wirev_fused_lookup.h", "wire_fused_round.h", "wire_fused_crc.h",
            "wire_fused_tables.h", "wire_layout.h", "wire_internal.h", "companion_support.h", "crc32c_outpkt.h",
            "crc32c_tables.h", "wirev_fused_exports.map"} <= set(build.WIREV_FUSED_HEADERS)
    assert "hadoofus_wirev_fused.h" in build.WIREV_FUSED_PUBLIC and build.ARCH == "gfx950"
    for f in build.WIREV_FUSED_SOURCES + build.WIREV_FUSED_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    for f in build.WIREV_FUSED_SOURCES + build.WIREV_FUSED_HEADERS:  # neither the gather layout nor its kernel
        assert f not in ("writev_layout.h", "writev_kernels.hip", "writev_internal.h", "wirev_internal.h"), f
    assert "An eighth companion, libhadoofus_wirev_fused.so" in build.__doc__


def test_sources_hold_no_plan_call_no_polynomial_and_no_gather_layout():
    """The CRCs are this library's own kernel's: no compute plan anywhere in
    it, the tables come from crc32c_tables.h, the one place the polynomials are
    written; the layout and the headers are the shared code's; nothing of the
    gather libraries is compiled into it."""
    from hadoofus_amd import build
    own = build.WIREV_FUSED_SOURCES + ["wirev_fused_internal.h", "wirev_fused_lookup.h"]
    for f in own + ["wire_fused_round.h", "wire_fused_crc.h", "wire_fused_tables.h"]:
        src = open(os.path.join(build.CSRC, f)).read()
        assert "hdfs_crc32c_plan_" not in src, f
        assert "put_header_proto(uint8_t" not in src and "put_out_header(uint8_t" not in src, f
        for poly in ("82f63b78", "edb88320"):
            assert poly not in src.lower(), (f, poly)
    for f in own:
        src = open(os.path.join(build.CSRC, f)).read()
        for name in ("writev_layout.h", "writev_kernels.hip", "writev_internal.h", "hadoofus_writev.h",
                     "hadoofus_wirev.h", "wire_frame.h", "gather_plan(", "enqueue_gather("):
            assert name not in src, (f, name)
        assert not re.search(r"int build_layout\(const uint64_t \*lens", src), f
    host = open(os.path.join(build.CSRC, "wirev_fused.cpp")).read()
    assert '#include "wire_layout.h"' in host and '#include "wire_fused_tables.h"' in host
    assert '#include "companion_support.h"' in host
    assert "build_layout(" in host and "fill_records(" in host and "args_ok(" in host
    assert "plan_out_packets(" not in host and "put_header_proto" not in host
    und = subprocess.check_output(["nm", "-D", "--undefined-only", build.WIREV_FUSED_LIB], text=True)
    assert "hdfs_crc32c_plan_" not in und


def test_one_definition_of_the_round_and_of_the_lookup():
    """The kernel file includes the shared round and the lookup and holds no
    copy of either, no buffer builtin, no permlane and no Unit of its own."""
    from hadoofus_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    code = lambda f: "\n".join(l for l in read(f).splitlines() if not l.lstrip().startswith("//"))  # noqa: E731
    helpers = ["range_of(", "load16(", "store16(", "store32(", "load8(", "store8(", "fold8(", "transpose(",
               "unit_of(", "load_round(", "store_round(", "crc_round(", "header(", "ragged_chunk(", "ragged_finish(",
               "fill_image("]
    rnd = read("wire_fused_round.h")
    for name in helpers:
        assert len(re.findall(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), rnd)) == 1, name
    kern = code("wirev_fused_kernels.hip")
    assert '#include "wire_fused_round.h"' in kern and '#include "wirev_fused_lookup.h"' in kern
    for f in ("wirev_fused_kernels.hip", "wirev_fused_internal.h"):
        src = code(f)
        assert "struct Unit" not in src and "__builtin_amdgcn_raw_buffer" not in src and "permlane" not in src, f
        for name in helpers:
            assert not re.search(r"FUSED_DEV [\w:<> ]*\b" + re.escape(name), src), (f, name)
        assert "uint32_t frag_of(" not in src and "atomic" not in src.lower(), f
    for name in ("load_round(", "store_round(", "crc_round<CSUM>(", "header(", "unit_of("):
        assert name in kern, name
    assert "ragged_finish<CSUM>(" in code("wirev_fused_internal.h")
    look = code("wirev_fused_lookup.h")  # compiles without HIP: the selftest is plain C++
    assert look.count("uint32_t frag_of(") == 1 and "hip" not in look.replace("__HIPCC__", "").lower()
    assert "frag_of(AtOf{ft}, nf, ra, k)" in kern and "address_space(4)" in code("wirev_fused_internal.h")


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_wirev_fused.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_wirev_fused_layout_info) - 72 + "
                   "HDFS_WIREV_FUSED_ABI_VERSION - 1 + (int)HDFS_WIREV_FUSED_TIME_GROUPS(0); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_amd.wirev_fused import LayoutInfo as S
    names = [f for f, _ in S._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_wirev_fused.h"\n'
                   'int main(void){ printf("%zu", sizeof(hdfs_wirev_fused_layout_info));\n' +
                   "".join(f'printf(" %zu", offsetof(hdfs_wirev_fused_layout_info, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    # pinned: the ABI of version 1
    assert got == [72, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68]
    assert names == ["npkts", "nchunks", "wire_len", "nfrags", "rounds", "seamed_rounds", "seamed_ragged",
                     "packet_stride", "header_bytes", "head_bytes", "max_frags_per_round"]


def test_companion_exports_exactly_its_header(libs):
    _, flib = libs
    assert _declared("hadoofus_wirev_fused.h") == DECLARED
    funcs = _c_functions(flib)
    assert set(funcs) == DECLARED, set(funcs) ^ DECLARED
    txt = open(os.path.join(ROOT, "include", "hadoofus_wirev_fused.h")).read()
    v = int(re.search(r"#define HDFS_WIREV_FUSED_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_WIREV_FUSED_{v}"}, funcs
    assert "HADOOFUS_WIREV_FUSED_1 {" in open(os.path.join(ROOT, "hadoofus_amd", "csrc",
                                                          "wirev_fused_exports.map")).read()


def test_main_library_and_its_abi_are_unchanged(libs):
    lib, _ = libs
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert "hdfs_wirev_fused" not in out and "HADOOFUS_WIREV_FUSED" not in out
    main_hdr = open(os.path.join(ROOT, "include", "hadoofus_crc32c.h")).read()
    assert "hdfs_wirev_fused" not in main_hdr and "#define HDFS_CRC32C_ABI_VERSION 5" in main_hdr
    # the committed signature list still ends at version 5 and is the headers'
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_signatures
    txt = open(os.path.join(ROOT, "tests", "golden", "abi_signatures.txt")).read()
    assert "hdfs_wirev_fused" not in txt and max(int(x) for x in re.findall(r"^\[(\d+)\]$", txt, flags=re.M)) == 5
    cur = dict(l.split(": ", 1) for l in txt.split("[5]\n", 1)[1].splitlines() if l and not l.startswith("#"))
    assert abi_signatures.header_prototypes() == cur


def test_the_seven_other_companions_export_what_they_did(libs):
    """Each exports exactly its header's functions under its own version node,
    none of them has a symbol of this library, and their headers and export
    maps do not speak of it."""
    lib, _ = libs
    libdir = os.path.dirname(lib)
    for name, node in OTHERS.items():
        funcs = _c_functions(os.path.join(libdir, f"libhadoofus_{name}.so"))
        assert set(funcs) == _declared(f"hadoofus_{name}.h"), (name, set(funcs) ^ _declared(f"hadoofus_{name}.h"))
        assert set(funcs.values()) == {node}, (name, funcs)
        assert not any("wirev_fused" in f for f in funcs), name
        for f in (f"include/hadoofus_{name}.h", f"hadoofus_amd/csrc/{name}_exports.map"):
            assert "wirev_fused" not in open(os.path.join(ROOT, f)).read().lower(), f


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


def test_abi_version_call_and_binding_check(wvf):
    assert wvf.load().hdfs_wirev_fused_abi_version() == wvf.ABI_VERSION == 1
    assert wvf.MAX_GROUPS == 1024 and wvf.time_groups(3) == 3 << 8

    class Other:
        @staticmethod
        def hdfs_wirev_fused_abi_version():
            return 2
    with pytest.raises(ImportError):
        wvf.check_abi(Other())


def test_last_error_text_is_its_own(wvf):
    """An EINVAL provoked here leaves the two-pass gather library's text alone,
    and the other way round."""
    from hadoofus_amd import wirev
    vl, lib = wirev.load(), wvf.load()
    lens = (ctypes.c_uint64 * 1)(10)
    assert vl.hdfs_wirev_layout(lens, 1, 0, 7, 2, 0, ctypes.byref(wirev.LayoutInfo())) == EINVAL
    before = vl.hdfs_wirev_last_error()
    assert lib.hdfs_wirev_fused_layout(lens, 1, -1, 2, 2, 0, ctypes.byref(wvf.LayoutInfo())) == EINVAL
    assert lib.hdfs_wirev_fused_last_error() == b"negative block offset"
    assert vl.hdfs_wirev_last_error() == before == b"proto must be 1 or 2"


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, wirev, wire_fused, wirev_fused\n"
            "assert abi._lib is None and wirev._lib is None and wire_fused._lib is None and wirev_fused._lib is None\n"
            "assert callable(h.compose_wirev_fused) and callable(h.wirev_fused_layout)\n"
            "assert callable(wirev_fused.fused_time) and callable(wirev_fused.layout)\n"
            "assert callable(wirev_fused.time_groups) and callable(wirev_fused.check_abi)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "wirev_fused_consumer"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "wirev_fused_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_wirev_fused", "-lhadoofus_crc32c"])
    assert exe.exists()
