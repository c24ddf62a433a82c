"""CPU tests of the gather-write companion library (include/hadoofus_writev.h):
the host layout of a write held in fragments against a brute-force model of
the chunk grid, the library's build and ABI, and everything the entry point
does without a GPU (size queries, HDFS_CRC32C_CSUM_NULL, argument errors).
The expected packets are the oracle's for the fragments' concatenation.
Everything is bit-exact."""
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
CS = 512


@pytest.fixture(scope="module")
def libs():
    """(release library, writev companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.WRITEV_LIB


@pytest.fixture(scope="module")
def wv(libs):
    from hadoofus_amd import writev
    writev.load()
    return writev


# ---- layout -------------------------------------------------------------------
def model(lens, off, min_seg):
    """Walks the chunk grid chunk by chunk: the fragments each chunk touches,
    maximal runs of grid chunks inside one fragment, runs of at least min_seg
    chunks kept as segments.  The short first chunk of an unaligned block
    offset is off the grid: never part of a run."""
    total = sum(lens)
    n0 = min(total, CS - off % CS) if total and off % CS else 0
    bounds = [0] + ([n0] if n0 else [])
    while bounds[-1] < total:
        bounds.append(min(bounds[-1] + CS, total))
    chunks = list(zip(bounds[:-1], bounds[1:]))
    frag_at, pos = [], 0  # (start, end, index) of non-empty fragments
    for i, n in enumerate(lens):
        if n:
            frag_at.append((pos, pos + n, i))
        pos += n
    touched = []  # per chunk: fragments it takes bytes from
    for s, e in chunks:
        touched.append([i for a, b, i in frag_at if a < e and b > s])
    runs, cur = [], None  # [first chunk, count, fragment]
    for k, t in enumerate(touched):
        on_grid = not (n0 and k == 0)
        if on_grid and len(t) == 1 and cur and cur[2] == t[0] and cur[0] + cur[1] == k:
            cur[1] += 1
            continue
        if cur:
            runs.append(cur)
        cur = [k, 1, t[0]] if on_grid and len(t) == 1 else None
    if cur:
        runs.append(cur)
    segs = [r for r in runs if r[1] >= min_seg]
    covered = set()
    for k, n, _ in segs:
        covered.update(range(k, k + n))
    gathered = [len(t) for k, t in enumerate(touched) if k not in covered]
    return {"total": total, "nchunks": len(chunks), "nsegments": len(segs), "seg_chunks": len(covered),
            "ngathered": len(gathered), "npieces": sum(gathered), "max_pieces": max(gathered, default=0),
            "min_seg_chunks": min_seg}


def _layout_cases():
    L = 200 * CS + 123
    cases = {
        "one": [L],
        "one_short": [77],
        "empty": [],
        "all_zero_len": [0, 0],
        "split_on_chunk": [64 * CS, L - 64 * CS],
        "split_mid_chunk": [64 * CS + 200, L - 64 * CS - 200],
        "split_at_1": [1, L - 1],
        "split_at_len_minus_1": [L - 1, 1],
        "zero_leading": [0, 5000, 7000],
        "zero_trailing": [5000, 7000, 0],
        "zero_interior": [5000, 0, 0, 7000],
        "one_byte_600": [1] * 600,
        "just_below_min_run": [7 * CS + 100] * 5,
        "exactly_min_run": [8 * CS] * 3,
        "frags_4000": [4000] * 40,
    }
    rng = np.random.default_rng(2024)
    for i in range(12):
        lens, tot = [], 0
        cap = int(rng.integers(1, 300 << 10))
        while tot < cap:
            n = int(rng.integers(1, 5001))
            lens.append(n)
            tot += n
        cases[f"random{i}"] = lens
    for i in range(4):  # larger fragments: segments and gathered chunks side by side
        cases[f"random_big{i}"] = [int(x) for x in rng.integers(1, 40000, int(rng.integers(2, 12)))]
    return cases


LAYOUT_CASES = _layout_cases()


@pytest.mark.parametrize("off", [0, 1, 511, 512, 4321])
@pytest.mark.parametrize("name", list(LAYOUT_CASES))
def test_layout_matches_model(wv, name, off):
    lens = LAYOUT_CASES[name]
    got = wv.layout(lens, off)
    assert got["min_seg_chunks"] >= 1
    want = model(lens, off, got["min_seg_chunks"])
    assert got == want
    assert got["seg_chunks"] + got["ngathered"] == got["nchunks"]
    assert got["total"] == sum(lens)


def test_layout_named_properties(wv):
    m = wv.layout([1], 0)["min_seg_chunks"]
    # a split on a chunk boundary leaves no gathered chunk (both runs long enough)
    a = wv.layout([64 * CS, 64 * CS], 0)
    assert (a["nsegments"], a["ngathered"], a["npieces"]) == (2, 0, 0) and 64 >= m
    # a split mid-chunk: exactly one gathered chunk of two pieces
    b = wv.layout([64 * CS + 200, 64 * CS - 200], 0)
    assert (b["nsegments"], b["ngathered"], b["npieces"], b["max_pieces"]) == (2, 1, 2, 2)
    # 600 one-byte fragments: a chunk of 512 pieces and one of 88
    c = wv.layout([1] * 600, 0)
    assert (c["seg_chunks"], c["ngathered"], c["npieces"], c["max_pieces"]) == (0, 2, 600, 512)
    # an unaligned block offset: the short first chunk is gathered, from one piece
    d = wv.layout([100 * CS], 4321)
    n0 = CS - 4321 % CS
    assert d["nchunks"] == 1 + (100 * CS - n0 + CS - 1) // CS
    assert (d["nsegments"], d["ngathered"], d["npieces"]) == (1, 1, 1)
    # a run one chunk short of the minimum is gathered, the minimum is a segment
    assert wv.layout([(m - 1) * CS], 0)["nsegments"] == 0
    assert wv.layout([m * CS], 0)["nsegments"] == 1


def test_layout_argument_errors(wv):
    lib = wv.load()
    info = wv.LayoutInfo()
    lens = (ctypes.c_uint64 * 2)(10, 20)
    assert lib.hdfs_writev_layout(lens, -1, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_writev_layout(None, 2, 0, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_writev_layout(lens, 2, -5, ctypes.byref(info)) == EINVAL
    assert lib.hdfs_writev_layout(lens, 2, 0, None) == EINVAL
    assert b"" != lib.hdfs_writev_last_error()


# ---- no-GPU behaviour ------------------------------------------------------------
def _frag(data, cuts):
    cuts = [0] + list(cuts) + [len(data)]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


FRAGMENTATIONS = {
    "two": [1000], "three_zero_mid": [70000, 70000], "many": list(range(997, 140000, 997)),
    "zero_ends": [0, 300, 140123],
}


@pytest.mark.parametrize("proto", [1, 2])
@pytest.mark.parametrize("off", [0, 4321])
@pytest.mark.parametrize("name", list(FRAGMENTATIONS))
def test_csum_null_matches_oracle_without_gpu(wv, oracle, name, off, proto):
    data = np.random.default_rng(5).integers(0, 256, 140123, dtype=np.uint8)
    frags = _frag(data, FRAGMENTATIONS[name])
    assert sum(len(f) for f in frags) == data.nbytes
    for finish in (False, True):
        got = wv.compose_packets_iov(frags, off, 7, proto, 0, finish)
        assert got == oracle.compose_packets(data, off, 7, proto, 0, finish)


def test_empty_write_needs_no_gpu(wv, oracle):
    for frags in ([], [b""], [b"", b""]):
        for ctype in (0, 1, 2):
            assert wv.compose_packets_iov(frags, 1024, 3, 2, ctype, True) == \
                oracle.compose_packets(b"", 1024, 3, 2, ctype, True)
            assert wv.compose_packets_iov(frags, 1024, 3, 2, ctype, False) == (b"", [])


@pytest.mark.parametrize("ctype", [0, 1, 2])
def test_size_query_needs_no_gpu(wv, oracle, ctype):
    data = np.random.default_rng(6).integers(0, 256, 200000, dtype=np.uint8)
    frags = _frag(data, [1, 65536, 65537, 199999])
    vec, n, keep = wv.iovecs(frags)
    npk, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    rc = wv.load().hdfs_writev_compose_packets(vec, n, 4321, 0, 2, ctype, 1, None, 0, None, 0, ctypes.byref(npk),
                                               ctypes.byref(used))
    assert rc == 0
    hdr, pkts = oracle.compose_packets(data, 4321, 0, 2, ctype, True)
    assert (npk.value, used.value) == (len(pkts), len(hdr))


def test_argument_errors_are_einval_without_a_device(wv):
    from hadoofus_amd.abi import IoVec, OutPacket
    lib = wv.load()
    buf = np.zeros(4096, dtype=np.uint8)
    hdr = np.full(4096, 0xEE, dtype=np.uint8)
    pk = (OutPacket * 16)()
    npk, used = ctypes.c_size_t(0), ctypes.c_uint64(0)
    good = (IoVec * 2)(IoVec(buf.ctypes.data, 1000), IoVec(buf.ctypes.data + 1000, 1000))
    null_base = (IoVec * 2)(IoVec(buf.ctypes.data, 1000), IoVec(None, 5))

    def call(vec, n, off=0, proto=2, ctype=2, cap=4096, maxp=16):
        return lib.hdfs_writev_compose_packets(vec, n, off, 0, proto, ctype, 0, hdr.ctypes.data, cap, pk, maxp,
                                               ctypes.byref(npk), ctypes.byref(used))
    assert call(good, -1) == EINVAL
    assert call(None, 2) == EINVAL
    assert call(null_base, 2) == EINVAL and b"fragment 1" in lib.hdfs_writev_last_error()
    assert call(good, 2, off=-1) == EINVAL
    assert call(good, 2, proto=0) == EINVAL and call(good, 2, proto=3) == EINVAL
    assert call(good, 2, ctype=3) == EINVAL and call(good, 2, ctype=-1) == EINVAL
    # undersized outputs: EINVAL, the sizes reported, nothing written
    assert call(good, 2, cap=10) == EINVAL and npk.value == 1 and used.value == 31 + 4 * 4
    assert call(good, 2, maxp=0) == EINVAL
    assert (hdr == 0xEE).all()
    # a NULL base with zero length is a valid (empty) fragment
    ok = (IoVec * 2)(IoVec(None, 0), IoVec(buf.ctypes.data, 100))
    assert call(ok, 2, ctype=0) == 0 and npk.value == 1


# ---- build and ABI ------------------------------------------------------------------
def test_build_produces_the_library(libs):
    lib, wlib = libs
    assert os.path.exists(wlib) and os.path.basename(wlib) == "libhadoofus_writev.so"
    assert os.path.dirname(lib) == os.path.dirname(wlib)


def test_build_lists_the_shared_header_for_both_libraries():
    from hadoofus_amd import build
    assert "crc32c_outpkt.h" in build.HEADERS and "crc32c_outpkt.h" in build.WRITEV_HEADERS
    for headers in (build.MD5CRC_HEADERS, build.WRITEV_HEADERS, build.WIRE_HEADERS, build.WIRE_BATCH_HEADERS):
        assert "companion_support.h" in headers
    assert "companion_support.h" not in build.HEADERS  # the main library has no part in it
    for f in build.WRITEV_SOURCES + build.WRITEV_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    # one definition of the header-writing code, not a copy
    for f in ("crc32c_packets.cpp", "writev.cpp"):
        src = open(os.path.join(build.CSRC, f)).read()
        assert '#include "crc32c_outpkt.h"' in src and "put_header_proto(uint8_t" not in src, f


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_writev.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_writev_layout_info) - 56 + HDFS_WRITEV_ABI_VERSION - 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_amd.writev import LayoutInfo as S
    names = [f for f, _ in S._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_writev.h"\n'
                   'int main(void){ printf("%zu", sizeof(hdfs_writev_layout_info));\n' +
                   "".join(f'printf(" %zu", offsetof(hdfs_writev_layout_info, {n}));\n' for n in names) +
                   "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]


def test_companion_exports_exactly_its_header(libs):
    _, wlib = libs
    decl = _declared("hadoofus_writev.h")
    assert decl == {"hdfs_writev_abi_version", "hdfs_writev_last_error", "hdfs_writev_compose_packets",
                    "hdfs_writev_layout"}
    funcs = {n: v for n, v in _exported(wlib).items() if n not in ("_init", "_fini")}
    # the toolchain may export a kernel's host stub; nothing else is allowed
    funcs = {n: v for n, v in funcs.items() if not (n.startswith("_ZN11hdfs_writev") and "_kernel" in n)}
    assert set(funcs) == decl, set(funcs) ^ decl
    txt = open(os.path.join(ROOT, "include", "hadoofus_writev.h")).read()
    v = int(re.search(r"#define HDFS_WRITEV_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_WRITEV_{v}"}, funcs


def test_main_library_gains_no_writev_symbol(libs):
    lib, _ = libs
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert "writev" not in out.lower()
    main_hdr = open(os.path.join(ROOT, "include", "hadoofus_crc32c.h")).read()
    assert "hdfs_writev" not in main_hdr and "#define HDFS_CRC32C_ABI_VERSION 5" in main_hdr


def test_companion_links_the_one_engine(libs):
    """The companion holds no copy of the engine: it needs the release
    library, found beside it, and reaches it through its public API."""
    lib, wlib = libs
    dyn = subprocess.check_output(["readelf", "-d", wlib], text=True)
    assert "libhadoofus_crc32c.so" in dyn and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", wlib], text=True)
    for sym in ("hdfs_crc32c_init", "hdfs_crc32c_bound_device", "hdfs_crc32c_plan_create", "hdfs_crc32c_plan_execute",
                "hdfs_crc32c_compose_packets", "hdfs_crc32c_host_alloc"):
        assert sym in und, sym


def test_abi_version_call_and_binding_check(wv):
    assert wv.load().hdfs_writev_abi_version() == wv.ABI_VERSION == 1

    class Other:
        @staticmethod
        def hdfs_writev_abi_version():
            return 2
    with pytest.raises(ImportError):
        wv.check_abi(Other())


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, writev\n"
            "assert abi._lib is None and writev._lib is None\n"
            "assert callable(h.compose_packets_iov) and callable(h.writev_layout)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "writev_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "writev_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_writev", "-lhadoofus_crc32c"])
    assert exe.exists()
