"""ctypes mirror of include/hadoofus_pread_batch.h (libhadoofus_pread_batch.so).

A batch of positional reads in one call: every entry's packet stream, in
device memory, is verified as far as its read goes and the block's bytes
[client_offset, client_offset + read_len) are delivered to the entry's device
buffer, with the outputs of hdfs_crc32c_read_packets(..., client_offset,
read_len, ...) of that entry alone.  The library is loaded on first use, after
the product library (it links against it), and refused when its
hdfs_pread_batch_abi_version() is not the one these bindings were written for.
No compute here.

An entry is a dict (or the keyword arguments of `entry`): stream_ptr, nbytes,
dst_ptr, dst_cap, client_offset, read_len.  stream_ptr and dst_ptr are raw
device pointers or torch device tensors (their data_ptr() is taken; nbytes and
dst_cap then default to the tensors' sizes).
"""
import ctypes

from hadoofus_amd import abi, companion
from hadoofus_amd.abi import CSUM_CRC32C, PROTO_V2, Packet, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_pread_batch.h HDFS_PREAD_BATCH_ABI_VERSION these bindings are written for
MAX_ENTRIES = 1024  # HDFS_PREAD_BATCH_MAX_ENTRIES
MAX_GROUPS = 1024  # workgroups HDFS_PREAD_BATCH_TIME_GROUPS accepts
PATH_KERNEL, PATH_FALLBACK = 0, 1  # HDFS_PREAD_BATCH_PATH_*
time_groups = companion.time_groups  # HDFS_PREAD_BATCH_TIME_GROUPS(n)

_lib = None  # the loaded library: None until the first load()


class Entry(ctypes.Structure):
    """struct hdfs_pread_batch_entry."""
    _fields_ = [
        ("stream", _vp),
        ("len", _u64),
        ("dst", _vp),
        ("dst_cap", _u64),
        ("client_offset", ctypes.c_int64),
        ("read_len", ctypes.c_int64),
        ("consumed", _u64),
        ("delivered", _u64),
        ("npkts", _u64),
        ("rc", ctypes.c_int32),
        ("path", ctypes.c_int32),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_pread_batch.h on lib."""
    b = abi._bind
    ep = ctypes.POINTER(Entry)
    b(lib, "hdfs_pread_batch_abi_version", _int, [])
    b(lib, "hdfs_pread_batch_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_pread_batch_read", _int, [ep, _sz, _int, _u32, _int, ctypes.POINTER(Packet), _sz, _vp])
    b(lib, "hdfs_pread_batch_time", _int,
      [ep, _sz, _int, _u32, _int, ctypes.c_uint, _int, ctypes.POINTER(ctypes.c_double)])
    return check_abi(lib)


_so = companion.Library("pread_batch", "pread batch", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def entry(stream_ptr=None, nbytes=None, dst_ptr=None, dst_cap=None, client_offset=0, read_len=0):
    """One positional read of a batch, as the dict the functions below take."""
    stream_ptr, sn = companion.ptr(stream_ptr)
    dst_ptr, dn = companion.ptr(dst_ptr)
    return dict(stream_ptr=stream_ptr, nbytes=(sn or 0) if nbytes is None else nbytes, dst_ptr=dst_ptr,
                dst_cap=(dn or 0) if dst_cap is None else dst_cap, client_offset=client_offset, read_len=read_len)


def entries(batch):
    """The C array of a list of entry dicts."""
    arr = (Entry * max(1, len(batch)))()
    for e, x in zip(arr, batch):
        x = entry(**x)
        e.stream, e.len, e.dst, e.dst_cap = x["stream_ptr"], x["nbytes"], x["dst_ptr"], x["dst_cap"]
        e.client_offset, e.read_len = x["client_offset"], x["read_len"]
    return arr


def _results(arr, n, pk, max_pkts):
    return [dict(rc=arr[b].rc, consumed=arr[b].consumed, delivered=arr[b].delivered, path=arr[b].path,
                 records=None if pk is None else [pk[b * max_pkts + i].as_dict() for i in range(arr[b].npkts)])
            for b in range(n)]


def read(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, max_pkts=None, stream=None):
    """hdfs_pread_batch_read.  max_pkts: room for every entry's records (None:
    no records are wanted, `records` is None).  The call's own refusal
    raises; what an entry ends in -- a packet error, AGAIN, or the main call's
    negative status for it -- is that entry's rc.
    -> [dict(rc, records, consumed, delivered, path) per entry]."""
    arr, n = entries(batch), len(batch)
    pk = None if max_pkts is None else (Packet * max(1, n * max_pkts))()
    rc = load().hdfs_pread_batch_read(arr, n, proto, chunk_size, ctype, pk, max_pkts or 0, stream)
    if rc < 0 and not any(arr[b].rc < 0 for b in range(n)):  # the call's own refusal, not an entry's
        _check(rc)
    return _results(arr, n, pk, max_pkts or 0)


def time(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, flags=0, iters=10):
    """hdfs_pread_batch_time: the call once, then both launches alone iters times.
    -> (milliseconds of one probe + main launch, [dict per entry] of the first call)."""
    arr, n, ms = entries(batch), len(batch), ctypes.c_double(0)
    rc = load().hdfs_pread_batch_time(arr, n, proto, chunk_size, ctype, flags, iters, ctypes.byref(ms))
    if rc < 0 and not any(arr[b].rc < 0 for b in range(n)):
        _check(rc)
    return ms.value, _results(arr, n, None, 0)
