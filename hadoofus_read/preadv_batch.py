"""ctypes mirror of include/hadoofus_preadv_batch.h (libhadoofus_preadv_batch.so).

A batch of scatter reads in one call: every entry's packet stream, in device
memory, is verified as far as its read goes and the block's bytes
[client_offset, client_offset + read_len) are laid, in order, over the entry's
list of device fragments, with the outputs of hdfs_crc32c_read_packets(...,
client_offset, read_len, iov, iovcnt, ...) of that entry alone.  The library is
loaded on first use, after the product library (it links against it), and
refused when its hdfs_preadv_batch_abi_version() is not the one these bindings
were written for.  No compute here.

An entry is a dict (or the arguments of `entry`): stream_ptr, nbytes, frags,
client_offset, read_len.  stream_ptr is a raw device pointer or a torch device
tensor (its data_ptr() is taken; nbytes then defaults to the tensor's size);
frags is a list of (device pointer or None, nbytes) pairs or of torch device
tensors.  read_len None means the fragments' total, which is
hdfs_datanode_readv's meaning.
"""
import ctypes

from hadoofus_amd import abi, companion
from hadoofus_amd.abi import CSUM_CRC32C, PROTO_V2, IoVec, Packet, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_preadv_batch.h HDFS_PREADV_BATCH_ABI_VERSION these bindings are written for
MAX_ENTRIES = 1024  # HDFS_PREADV_BATCH_MAX_ENTRIES
MAX_FRAGS = 1 << 22  # HDFS_PREADV_BATCH_MAX_FRAGS
MAX_GROUPS = 1024  # workgroups HDFS_PREADV_BATCH_TIME_GROUPS accepts
PATH_KERNEL, PATH_FALLBACK = 0, 1  # HDFS_PREADV_BATCH_PATH_*
time_groups = companion.time_groups  # HDFS_PREADV_BATCH_TIME_GROUPS(n)

_lib = None  # the loaded library: None until the first load()


class Entry(ctypes.Structure):
    """struct hdfs_preadv_batch_entry."""
    _fields_ = [
        ("stream", _vp),
        ("len", _u64),
        ("iov", ctypes.POINTER(IoVec)),
        ("iovcnt", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("client_offset", ctypes.c_int64),
        ("read_len", ctypes.c_int64),
        ("consumed", _u64),
        ("delivered", _u64),
        ("npkts", _u64),
        ("rc", ctypes.c_int32),
        ("path", ctypes.c_int32),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_preadv_batch.h on lib."""
    b = abi._bind
    ep = ctypes.POINTER(Entry)
    b(lib, "hdfs_preadv_batch_abi_version", _int, [])
    b(lib, "hdfs_preadv_batch_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_preadv_batch_read", _int, [ep, _sz, _int, _u32, _int, ctypes.POINTER(Packet), _sz, _vp])
    b(lib, "hdfs_preadv_batch_time", _int,
      [ep, _sz, _int, _u32, _int, ctypes.c_uint, _int, ctypes.POINTER(ctypes.c_double)])
    return check_abi(lib)


_so = companion.Library("preadv_batch", "preadv batch", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def _frag(f):
    if hasattr(f, "data_ptr"):
        return companion.ptr(f)
    p, n = f
    return (None if p is None else int(p)), int(n)


def entry(stream_ptr=None, nbytes=None, frags=(), client_offset=0, read_len=None):
    """One scatter read of a batch, as the dict the functions below take.
    read_len None: the fragments' total."""
    stream_ptr, sn = companion.ptr(stream_ptr)
    frags = [_frag(f) for f in frags]
    return dict(stream_ptr=stream_ptr, nbytes=(sn or 0) if nbytes is None else nbytes, frags=frags,
                client_offset=client_offset, read_len=sum(n for _, n in frags) if read_len is None else read_len)


def entries(batch):
    """The C array of a list of entry dicts.
    -> (array, the fragment arrays its entries point to: keep them alive with it)."""
    arr, keep = (Entry * max(1, len(batch)))(), []
    for e, x in zip(arr, batch):
        x = entry(**x)
        vec = (IoVec * max(1, len(x["frags"])))(*[IoVec(p, n) for p, n in x["frags"]])
        keep.append(vec)
        e.stream, e.len, e.iov, e.iovcnt = x["stream_ptr"], x["nbytes"], vec, len(x["frags"])
        e.client_offset, e.read_len = x["client_offset"], x["read_len"]
    return arr, keep


def _results(arr, n, pk, max_pkts):
    return [dict(rc=arr[b].rc, consumed=arr[b].consumed, delivered=arr[b].delivered, path=arr[b].path,
                 records=None if pk is None else [pk[b * max_pkts + i].as_dict() for i in range(arr[b].npkts)])
            for b in range(n)]


def read(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, max_pkts=None, stream=None):
    """hdfs_preadv_batch_read.  max_pkts: room for every entry's records (None:
    no records are wanted, `records` is None).  The call's own refusal
    raises; what an entry ends in -- a packet error, AGAIN, or the main call's
    negative status for it -- is that entry's rc.
    -> [dict(rc, records, consumed, delivered, path) per entry]."""
    (arr, _keep), n = entries(batch), len(batch)
    pk = None if max_pkts is None else (Packet * max(1, n * max_pkts))()
    rc = load().hdfs_preadv_batch_read(arr, n, proto, chunk_size, ctype, pk, max_pkts or 0, stream)
    if rc < 0 and not any(arr[b].rc < 0 for b in range(n)):  # the call's own refusal, not an entry's
        _check(rc)
    return _results(arr, n, pk, max_pkts or 0)


def time(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, flags=0, iters=10):
    """hdfs_preadv_batch_time: the call once, then both launches alone iters times.
    -> (milliseconds of one probe + main launch, [dict per entry] of the first call)."""
    (arr, _keep), n, ms = entries(batch), len(batch), ctypes.c_double(0)
    rc = load().hdfs_preadv_batch_time(arr, n, proto, chunk_size, ctype, flags, iters, ctypes.byref(ms))
    if rc < 0 and not any(arr[b].rc < 0 for b in range(n)):
        _check(rc)
    return ms.value, _results(arr, n, None, 0)
