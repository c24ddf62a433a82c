"""ctypes mirror of include/hadoofus_wirev_fused_batch.h
(libhadoofus_wirev_fused_batch.so).

The wire streams of a batch of writes, each held in a list of device buffers,
in one call, one launch and one pass over the fragments: the library's own
kernel computes every write's chunk CRCs while it copies, and finds the writes
and their fragments through tables uploaded once.  Write k's stream and
records are wirev_fused.compose_wirev_fused's.  The companion library is
loaded on first use, after the product library (it links against it), and
refused when its hdfs_wirev_fused_batch_abi_version() is not the one these
bindings were written for.  No compute here and no fallback.

A write is a dict (or keyword arguments of `write`): frags, wire_ptr,
wire_cap, offset_in_block, seqno, finish.  frags is a list of (device ptr or
None, nbytes) pairs, or an abi.IoVec array made beforehand (with iovcnt).
wire_ptr is a raw device pointer or a torch device tensor (its data_ptr() is
taken; wire_cap then defaults to the tensor's size).
"""
import ctypes

from . import abi, companion
from .abi import CSUM_CRC32C, PROTO_V2, IoVec, OutPacket, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_wirev_fused_batch.h HDFS_WIREV_FUSED_BATCH_ABI_VERSION these bindings are written for
MAX_WRITES = 65536  # HDFS_WIREV_FUSED_BATCH_MAX_WRITES
MAX_FRAGS = 1 << 22  # HDFS_WIREV_FUSED_BATCH_MAX_FRAGS
MAX_GROUPS = 1024  # workgroups HDFS_WIREV_FUSED_BATCH_TIME_GROUPS accepts
time_groups = companion.time_groups  # HDFS_WIREV_FUSED_BATCH_TIME_GROUPS(n)
_split = companion.split

_lib = None  # the loaded library: None until the first load()


class BatchWrite(ctypes.Structure):
    """struct hdfs_wirev_fused_batch_write."""
    _fields_ = [
        ("iov", ctypes.POINTER(IoVec)),
        ("iovcnt", ctypes.c_int32),
        ("finish", ctypes.c_int32),
        ("offset_in_block", ctypes.c_int64),
        ("seqno", ctypes.c_int64),
        ("wire", _vp),
        ("wire_cap", _u64),
        ("len", _u64),
        ("wire_len", _u64),
        ("npkts", _u64),
        ("first_pkt", _u64),
    ]

    def out(self):
        return {"len": self.len, "wire_len": self.wire_len, "npkts": self.npkts, "first_pkt": self.first_pkt}

    def source(self, w):
        """-> the IoVec array the entry now points to."""
        fr = w["frags"]
        vec = fr if isinstance(fr, ctypes.Array) else companion.iovecs(fr)[0]
        self.iov = ctypes.cast(vec, ctypes.POINTER(IoVec))
        self.iovcnt = len(fr) if w["iovcnt"] is None else w["iovcnt"]
        return vec


class Totals(companion.Record):
    """struct hdfs_wirev_fused_batch_totals."""
    _fields_ = [
        ("npkts", _u64),
        ("nchunks", _u64),
        ("wire_bytes", _u64),
        ("table_entries", _u64),
        ("nfrags", _u64),
        ("rounds", _u64),
        ("seamed_rounds", _u64),
        ("seamed_ragged", _u64),
        ("max_frags_per_round", _u32),
        ("reserved", _u32),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_wirev_fused_batch.h on lib."""
    b = abi._bind
    wp = ctypes.POINTER(BatchWrite)
    b(lib, "hdfs_wirev_fused_batch_abi_version", _int, [])
    b(lib, "hdfs_wirev_fused_batch_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_wirev_fused_batch_compose", _int,
      [wp, _sz, _int, _int, ctypes.POINTER(OutPacket), _sz, ctypes.POINTER(_sz), _vp])
    b(lib, "hdfs_wirev_fused_batch_layout", _int, [wp, _sz, _int, _int, ctypes.POINTER(Totals)])
    b(lib, "hdfs_wirev_fused_batch_time", _int,
      [wp, _sz, _int, _int, ctypes.c_uint, _int, ctypes.POINTER(ctypes.c_double)])
    return check_abi(lib)


_so = companion.Library("wirev_fused_batch", "fused wirev batch", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the companion library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def write(frags=(), wire_ptr=None, wire_cap=None, offset_in_block=0, seqno=0, finish=False, iovcnt=None):
    """One write of a batch, as the dict the functions below take."""
    wire_ptr, wn = companion.ptr(wire_ptr)
    return dict(frags=frags, wire_ptr=wire_ptr, wire_cap=(wn or 0) if wire_cap is None else wire_cap,
                offset_in_block=offset_in_block, seqno=seqno, finish=finish, iovcnt=iovcnt)


def entries(writes, query=False):
    """The C array of a list of write dicts.  query: wire NULL in every entry.
    -> (array, the IoVec arrays it points to: keep them alive with it)."""
    return companion.entries(writes, query, BatchWrite, write)


def layout(writes, proto=PROTO_V2, ctype=CSUM_CRC32C):
    """hdfs_wirev_fused_batch_layout (host only; only the fragments' lengths count).
    -> ([{len, wire_len, npkts, first_pkt} per write], dict of struct hdfs_wirev_fused_batch_totals' fields)."""
    return companion.batch_layout(_so, load(), writes, proto, ctype, entries, Totals)


def packet_records(writes, proto=PROTO_V2, ctype=CSUM_CRC32C):
    """The size query of hdfs_wirev_fused_batch_compose (no GPU; no base is read).
    -> [(wire_len, [packet dicts]) per write], hdr_off counting in the write's
    own stream, data_off in its fragments' concatenation."""
    return companion.batch_packet_records(_so, load(), writes, proto, ctype, entries)


def compose(writes, proto=PROTO_V2, ctype=CSUM_CRC32C, stream=None):
    """hdfs_wirev_fused_batch_compose: the stream of every write of the batch,
    write k's at its wire_ptr.  -> [(wire_len, [packet dicts]) per write];
    packet i's header buffer starts at wire_ptr + hdr_off, its data at hdr_off
    + hdr_len."""
    return companion.batch_compose(_so, load(), writes, proto, ctype, stream, entries, Totals)


def fused_batch_time(writes, proto=PROTO_V2, ctype=CSUM_CRC32C, flags=0, iters=10):
    """hdfs_wirev_fused_batch_time: milliseconds of one launch of the fused gather batch kernel."""
    ms = ctypes.c_double(0)
    arr, _keep = entries(writes)
    _check(load().hdfs_wirev_fused_batch_time(arr, len(writes), proto, ctype, flags, iters, ctypes.byref(ms)))
    return ms.value
