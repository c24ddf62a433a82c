"""ctypes mirror of include/hadoofus_md5crc.h (libhadoofus_md5crc.so).

MD5CRC block checksums -- MD5 over a block's chunk CRCs in wire order -- from
the CRC arrays a compute plan left in device memory, and the file checksum
"MD5-of-N-MD5-of-512-CRC32C" made of them.  The companion library is loaded
on first use, after the product library (it links against it), and refused
when its hdfs_md5crc_abi_version() is not the one these bindings were written
for.  No compute here and no fallback.
"""
import ctypes

from . import abi, companion
from .abi import CSUM_CRC32C, Segment, _host, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_md5crc.h HDFS_MD5CRC_ABI_VERSION these bindings are written for
MD5_LEN = 16

_lib = None  # the loaded library: None until the first load()


class FileChecksumStruct(ctypes.Structure):
    """struct hdfs_md5crc_file_checksum."""
    _fields_ = [
        ("bytes_per_crc", _u32),
        ("ctype", _u32),
        ("crc_per_block", _u64),
        ("md5", ctypes.c_uint8 * MD5_LEN),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_md5crc.h on lib."""
    b = abi._bind
    b(lib, "hdfs_md5crc_abi_version", _int, [])
    b(lib, "hdfs_md5crc_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_md5crc_block_digests", _int, [ctypes.POINTER(Segment), _sz, _vp, _vp])
    b(lib, "hdfs_md5crc_file_from_blocks", _int,
      [_vp, _sz, _u32, _u64, _int, ctypes.POINTER(FileChecksumStruct)])
    b(lib, "hdfs_md5crc_file_checksum_dev", _int,
      [ctypes.POINTER(Segment), _sz, _vp, ctypes.POINTER(FileChecksumStruct)])
    b(lib, "hdfs_md5crc_algorithm_name", _int, [ctypes.POINTER(FileChecksumStruct), ctypes.c_char_p, _sz])
    b(lib, "hdfs_md5crc_file_bytes", _int, [ctypes.POINTER(FileChecksumStruct), _vp])
    b(lib, "hdfs_md5crc_md5_host", _int, [_vp, _u64, _vp])
    return check_abi(lib)


_so = companion.Library("md5crc", "md5crc", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the companion library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


class FileChecksum:
    """A file's MD5MD5CRC checksum: bytes_per_crc, crc_per_block, ctype, md5
    (16 bytes), algorithm ("MD5-of-<crc_per_block>MD5-of-<bytes_per_crc>CRC32C")
    and to_bytes() (the 28 bytes MD5MD5CRC32FileChecksum serialises)."""

    def __init__(self, c):
        self._c = c
        self.bytes_per_crc = c.bytes_per_crc
        self.crc_per_block = c.crc_per_block
        self.ctype = c.ctype
        self.md5 = bytes(c.md5)

    @property
    def algorithm(self):
        buf = ctypes.create_string_buffer(64)
        _check(load().hdfs_md5crc_algorithm_name(ctypes.byref(self._c), buf, 64))
        return buf.value.decode()

    def to_bytes(self):
        out = ctypes.create_string_buffer(28)
        _check(load().hdfs_md5crc_file_bytes(ctypes.byref(self._c), out))
        return out.raw

    def __repr__(self):
        return f"FileChecksum({self.algorithm}:{self.md5.hex()})"


def md5_host(buf):
    """Plain MD5 of host bytes by the library's host build of the kernel's
    round code.  -> 16 bytes."""
    keep, p, n = _host(buf)
    out = ctypes.create_string_buffer(MD5_LEN)
    _check(load().hdfs_md5crc_md5_host(p if n else None, n, out))
    return out.raw


def block_md5crcs(segments, stream=None, out_dptr=None):
    """hdfs_md5crc_block_digests: the MD5CRC block checksum of each segment
    from its device chunk-CRC array, enqueued on `stream` (None = the NULL
    stream).  -> [16 bytes per segment]; with out_dptr (device memory, 16 *
    len(segments) bytes) the digests are written there and None is returned."""
    n = len(segments)
    arr = (Segment * max(1, n))(*segments)
    if out_dptr is not None:
        _check(load().hdfs_md5crc_block_digests(arr, n, stream, out_dptr))
        return None
    out = ctypes.create_string_buffer(max(1, n * MD5_LEN))
    _check(load().hdfs_md5crc_block_digests(arr, n, stream, out))
    return [out.raw[i * MD5_LEN:(i + 1) * MD5_LEN] for i in range(n)]


def file_checksum(segments, stream=None):
    """hdfs_md5crc_file_checksum_dev: segments are the file's blocks in
    order.  -> FileChecksum."""
    n = len(segments)
    arr = (Segment * max(1, n))(*segments)
    c = FileChecksumStruct()
    _check(load().hdfs_md5crc_file_checksum_dev(arr, n, stream, ctypes.byref(c)))
    return FileChecksum(c)


def file_checksum_from_blocks(block_md5s, bytes_per_crc=512, crc_per_block=0, ctype=CSUM_CRC32C):
    """hdfs_md5crc_file_from_blocks (host only): block_md5s is a list of
    16-byte digests, or their concatenation.  -> FileChecksum."""
    raw = block_md5s if isinstance(block_md5s, (bytes, bytearray, memoryview)) else b"".join(block_md5s)
    raw = bytes(raw)
    if len(raw) % MD5_LEN:
        raise ValueError("block digests are 16 bytes each")
    c = FileChecksumStruct()
    _check(load().hdfs_md5crc_file_from_blocks(raw if raw else None, len(raw) // MD5_LEN, bytes_per_crc,
                                               crc_per_block, ctype, ctypes.byref(c)))
    return FileChecksum(c)
