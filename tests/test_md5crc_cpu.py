"""CPU tests of the MD5CRC companion library (include/hadoofus_md5crc.h):
its host MD5, the file checksum built from block digests, and its build and
ABI.  Expected values are Python's hashlib.md5 over bytes built from the
definition (MD5 of the blocks' digests in block order; RFC 1321's own test
strings for the plain MD5).  No Hadoop-generated vector is available offline,
so none is used.  Everything is bit-exact."""
import ctypes
import hashlib
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from abi_symbols import declared as _declared, exported as _exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def libs():
    """(release library, md5crc companion), built if stale."""
    from hadoofus_amd import build
    return build.build(), build.MD5CRC_LIB


@pytest.fixture(scope="module")
def h(libs):
    import hadoofus_amd
    return hadoofus_amd


# ---- host MD5 ---------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128, 1000003])
def test_md5_host_matches_hashlib(h, n):
    buf = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert h.md5_host(buf) == hashlib.md5(buf).digest()


def test_md5_host_rfc1321_strings(h):
    kats = {b"": "d41d8cd98f00b204e9800998ecf8427e", b"a": "0cc175b9c0f1b6a831c399e269772661",
            b"abc": "900150983cd24fb0d6963f7d28e17f72", b"message digest": "f96b697d7cb7938d525a2f31aaf161d0"}
    for msg, want in kats.items():
        assert h.md5_host(msg).hex() == want, msg
        assert hashlib.md5(msg).hexdigest() == want  # the reference agrees with the RFC


# ---- file checksum ------------------------------------------------------------
def _digests(n):
    return [hashlib.md5(struct.pack("<I", i)).digest() for i in range(n)]


@pytest.mark.parametrize("nblocks", [1, 2, 1000])
def test_file_checksum_from_blocks(h, nblocks):
    md5s = _digests(nblocks)
    cpb = 262144 if nblocks > 1 else 0
    c = h.file_checksum_from_blocks(md5s, bytes_per_crc=512, crc_per_block=cpb)
    want = hashlib.md5(b"".join(md5s)).digest()
    assert c.md5 == want
    assert (c.bytes_per_crc, c.crc_per_block, c.ctype) == (512, cpb, h.CSUM_CRC32C)
    assert c.to_bytes() == struct.pack(">iq", 512, cpb) + want
    assert len(c.to_bytes()) == 28
    # the concatenated form is the same call
    assert h.file_checksum_from_blocks(b"".join(md5s), 512, cpb).to_bytes() == c.to_bytes()


def test_file_checksum_algorithm_names(h):
    one = h.file_checksum_from_blocks(_digests(1), bytes_per_crc=512, crc_per_block=0)
    assert one.algorithm == "MD5-of-0MD5-of-512CRC32C"
    two = h.file_checksum_from_blocks(_digests(2), bytes_per_crc=512, crc_per_block=(128 << 20) // 512)
    assert two.algorithm == "MD5-of-262144MD5-of-512CRC32C"
    old = h.file_checksum_from_blocks(_digests(2), bytes_per_crc=512, crc_per_block=262144, ctype=h.CSUM_CRC32)
    assert old.algorithm == "MD5-of-262144MD5-of-512CRC32"
    assert old.md5 == two.md5  # the digest does not depend on the polynomial's name


@pytest.mark.parametrize("ctype", [0, 3, -1])
def test_file_checksum_bad_ctype_is_einval(h, ctype):
    with pytest.raises(h.CRC32CError) as e:
        h.file_checksum_from_blocks(_digests(2), 512, 4, ctype=ctype)
    assert e.value.code == EINVAL


def test_empty_batch_needs_no_gpu(h):
    assert h.block_md5crcs([]) == []


# ---- build and ABI --------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hadoofus_md5crc.h"\n'
                   "int main(void){ return (int)sizeof(hdfs_md5crc_file_checksum) - 32 + HDFS_MD5CRC_LEN - 16; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_struct_layout_matches_c(tmp_path):
    from hadoofus_amd.md5crc import FileChecksumStruct as S
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hadoofus_md5crc.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu\\n", sizeof(hdfs_md5crc_file_checksum),'
                   " offsetof(hdfs_md5crc_file_checksum, ctype), offsetof(hdfs_md5crc_file_checksum, crc_per_block),"
                   " offsetof(hdfs_md5crc_file_checksum, md5)); return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(S), S.ctype.offset, S.crc_per_block.offset, S.md5.offset]


def test_companion_exports_exactly_its_header(libs):
    _, md5lib = libs
    decl = _declared("hadoofus_md5crc.h")
    assert {"hdfs_md5crc_block_digests", "hdfs_md5crc_file_checksum_dev", "hdfs_md5crc_md5_host"} <= decl
    assert all(n.startswith("hdfs_md5crc_") for n in decl), decl
    exported = _exported(md5lib)
    funcs = {n: v for n, v in exported.items() if n not in ("_init", "_fini")}
    # the toolchain may export a kernel's host stub; nothing else is allowed
    funcs = {n: v for n, v in funcs.items() if not (n.startswith("_ZN11hdfs_md5crc") and "_kernel" in n)}
    assert set(funcs) == decl, set(funcs) ^ decl
    txt = open(os.path.join(ROOT, "include", "hadoofus_md5crc.h")).read()
    v = int(re.search(r"#define HDFS_MD5CRC_ABI_VERSION (\d+)", txt).group(1))
    assert set(funcs.values()) == {f"HADOOFUS_MD5CRC_{v}"}, funcs


def test_main_library_gains_no_md5crc_symbol(libs):
    lib, _ = libs
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert "md5" not in out.lower()
    main_hdr = open(os.path.join(ROOT, "include", "hadoofus_crc32c.h")).read()
    assert "md5crc" not in main_hdr and "#define HDFS_CRC32C_ABI_VERSION 5" in main_hdr


def test_companion_links_the_one_engine(libs):
    """The companion holds no copy of the engine: it needs the release
    library, found beside it, and defines none of its symbols."""
    lib, md5lib = libs
    dyn = subprocess.check_output(["readelf", "-d", md5lib], text=True)
    assert "libhadoofus_crc32c.so" in dyn and "$ORIGIN" in dyn
    und = subprocess.check_output(["nm", "-D", "--undefined-only", md5lib], text=True)
    assert "hdfs_crc32c_init" in und and "hdfs_crc32c_bound_device" in und
    assert os.path.dirname(lib) == os.path.dirname(md5lib)


def test_abi_version_call_and_binding_check(libs):
    from hadoofus_amd import md5crc
    lib = md5crc.load()
    assert lib.hdfs_md5crc_abi_version() == md5crc.ABI_VERSION == 1

    class Other:
        @staticmethod
        def hdfs_md5crc_abi_version():
            return 2
    with pytest.raises(ImportError):
        md5crc.check_abi(Other())


def test_import_loads_nothing():
    code = ("import hadoofus_amd as h\nfrom hadoofus_amd import abi, md5crc\n"
            "assert abi._lib is None and md5crc._lib is None\n"
            "assert callable(h.block_md5crcs) and callable(h.file_checksum) and callable(h.md5_host)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_c_consumer_links(tmp_path, libs):
    lib, _ = libs
    libdir = os.path.dirname(lib)
    exe = tmp_path / "md5crc_consumer"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "consumer", "md5crc_consumer.c"), "-o", str(exe),
                           "-L", libdir, "-Wl,-rpath," + libdir, "-lhadoofus_md5crc", "-lhadoofus_crc32c"])
    assert exe.exists()
