"""ctypes mirror of include/hadoofus_crc_streams.h (libhadoofus_crc_streams.so).

Composite CRCs (HDFS's COMPOSITE_CRC mode) of blocks and of a file taken from
packet streams in device memory: every entry's chunk CRCs are combined where
they lie in the stream, with the framing outputs of hdfs_crc32c_parse_packets
of that entry alone.  The CRCs are not verified against the data here.  The
library is loaded on first use, after the product library (it links against
it), and refused when its hdfs_crc_streams_abi_version() is not the one these
bindings were written for.  No compute here.

An entry is a dict (or the keyword arguments of `entry`): stream_ptr, nbytes.
stream_ptr is a raw device pointer or a torch device tensor (its data_ptr() is
taken; nbytes then defaults to the tensor's size).
"""
import ctypes

from hadoofus_amd import abi, companion
from hadoofus_amd.abi import CSUM_CRC32C, PROTO_V2, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_crc_streams.h HDFS_CRC_STREAMS_ABI_VERSION these bindings are written for
MAX_ENTRIES = 1024  # HDFS_CRC_STREAMS_MAX_ENTRIES
PATH_KERNEL, PATH_FALLBACK = 0, 1  # HDFS_CRC_STREAMS_PATH_*
TIME_NONE = 0  # HDFS_CRC_STREAMS_TIME_NONE

_lib = None  # the loaded library: None until the first load()


class Entry(ctypes.Structure):
    """struct hdfs_crc_streams_entry."""
    _fields_ = [
        ("stream", _vp),
        ("len", _u64),
        ("consumed", _u64),
        ("payload", _u64),
        ("nchunks", _u64),
        ("npkts", _u64),
        ("offset_in_block", ctypes.c_int64),
        ("rc", ctypes.c_int32),
        ("path", ctypes.c_int32),
        ("crc", _u32),
        ("reserved", _u32),
    ]


class FileChecksum(companion.Record):
    """struct hdfs_crc_streams_file_checksum."""
    _fields_ = [
        ("bytes_per_crc", _u32),
        ("ctype", _u32),
        ("crc", _u32),
        ("bytes", ctypes.c_uint8 * 4),
        ("length", _u64),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_crc_streams.h on lib."""
    b = abi._bind
    ep = ctypes.POINTER(Entry)
    b(lib, "hdfs_crc_streams_abi_version", _int, [])
    b(lib, "hdfs_crc_streams_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_crc_streams_block_crcs", _int, [ep, _sz, _int, _u32, _int, _vp])
    b(lib, "hdfs_crc_streams_file_checksum", _int, [ep, _sz, _int, _u32, _int, _vp, ctypes.POINTER(FileChecksum)])
    b(lib, "hdfs_crc_streams_combine", _int,
      [ctypes.POINTER(_u32), ctypes.POINTER(_u64), _sz, _int, ctypes.POINTER(_u32)])
    b(lib, "hdfs_crc_streams_time", _int,
      [ep, _sz, _int, _u32, _int, ctypes.c_uint, _int, ctypes.POINTER(ctypes.c_double)])
    return check_abi(lib)


_so = companion.Library("crc_streams", "crc streams", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def entry(stream_ptr=None, nbytes=None):
    """One block's packet stream, as the dict the functions below take."""
    stream_ptr, sn = companion.ptr(stream_ptr)
    return dict(stream_ptr=stream_ptr, nbytes=(sn or 0) if nbytes is None else nbytes)


def entries(batch):
    """The C array of a list of entry dicts."""
    arr = (Entry * max(1, len(batch)))()
    for e, x in zip(arr, batch):
        x = entry(**x)
        e.stream, e.len = x["stream_ptr"], x["nbytes"]
    return arr


def _results(arr, n):
    return [dict(rc=arr[b].rc, consumed=arr[b].consumed, payload=arr[b].payload, nchunks=arr[b].nchunks,
                 npkts=arr[b].npkts, offset_in_block=arr[b].offset_in_block, path=arr[b].path, crc=arr[b].crc)
            for b in range(n)]


def _refused(rc, arr, n):
    """The call's own refusal, not an entry's."""
    return rc < 0 and not any(arr[b].rc < 0 for b in range(n))


def block_crcs(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, stream=None):
    """hdfs_crc_streams_block_crcs.  The call's own refusal raises; what an
    entry ends in -- a packet error, or the main call's negative status for it
    -- is that entry's rc.
    -> [dict(rc, consumed, payload, nchunks, npkts, offset_in_block, path, crc) per entry]."""
    arr, n = entries(batch), len(batch)
    rc = load().hdfs_crc_streams_block_crcs(arr, n, proto, chunk_size, ctype, stream)
    if _refused(rc, arr, n):
        _check(rc)
    return _results(arr, n)


def file_checksum(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, stream=None):
    """hdfs_crc_streams_file_checksum: the batch is a file's blocks in order.
    Raises when the call does (an entry with a packet error or a stream that
    does not start at block offset 0 among them).
    -> (dict(bytes_per_crc, ctype, crc, bytes, length), [dict per entry])."""
    arr, n, out = entries(batch), len(batch), FileChecksum()
    _check(load().hdfs_crc_streams_file_checksum(arr, n, proto, chunk_size, ctype, stream, ctypes.byref(out)))
    d = out.as_dict()
    d["bytes"] = bytes(out.bytes)
    return d, _results(arr, n)


def combine(crcs, lens, ctype=CSUM_CRC32C):
    """hdfs_crc_streams_combine: the CRC of pieces of lens[i] bytes with CRCs crcs[i], in order.  Host only."""
    n, out = len(crcs), _u32(0)
    if len(lens) != n:
        raise ValueError("as many lengths as CRCs")
    _check(load().hdfs_crc_streams_combine((_u32 * max(1, n))(*crcs), (_u64 * max(1, n))(*lens), n, ctype,
                                           ctypes.byref(out)))
    return out.value


def time(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, flags=TIME_NONE, iters=10):
    """hdfs_crc_streams_time: the call once, then the three launches alone iters times.
    -> (milliseconds of one probe + fold + reduce, [dict per entry] of the first call)."""
    arr, n, ms = entries(batch), len(batch), ctypes.c_double(0)
    rc = load().hdfs_crc_streams_time(arr, n, proto, chunk_size, ctype, flags, iters, ctypes.byref(ms))
    if _refused(rc, arr, n):
        _check(rc)
    return ms.value, _results(arr, n)
