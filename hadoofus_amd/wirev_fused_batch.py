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
import os

from . import abi
from .abi import CSUM_CRC32C, PROTO_V2, CRC32CError, IoVec, OutPacket, _int, _sz, _u32, _u64, _vp

LIB_PATH = os.path.join(os.path.dirname(abi.LIB_PATH), "libhadoofus_wirev_fused_batch.so")
ABI_VERSION = 1  # include/hadoofus_wirev_fused_batch.h HDFS_WIREV_FUSED_BATCH_ABI_VERSION these bindings are written for
MAX_WRITES = 65536  # HDFS_WIREV_FUSED_BATCH_MAX_WRITES
MAX_FRAGS = 1 << 22  # HDFS_WIREV_FUSED_BATCH_MAX_FRAGS
MAX_GROUPS = 1024  # workgroups HDFS_WIREV_FUSED_BATCH_TIME_GROUPS accepts

_lib = None


def time_groups(n):
    """HDFS_WIREV_FUSED_BATCH_TIME_GROUPS(n)."""
    return n << 8


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


class Totals(ctypes.Structure):
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

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved"}


def check_abi(lib):
    v = lib.hdfs_wirev_fused_batch_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"fused wirev batch library ABI version {v}, bindings written for {ABI_VERSION}")
    return lib


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


def load(path=LIB_PATH):
    """Load the companion library (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    abi.load()  # first: the companion links against the product library
    if not os.path.exists(path):
        raise ImportError(f"{path} not built; run `python -m hadoofus_amd.build` "
                          "(or __graft_entry__.build())")
    _lib = bind(ctypes.CDLL(path))
    return _lib


def _check(rc):
    if rc != 0:
        raise CRC32CError(rc, load().hdfs_wirev_fused_batch_last_error().decode(errors="replace"))


def write(frags=(), wire_ptr=None, wire_cap=None, offset_in_block=0, seqno=0, finish=False, iovcnt=None):
    """One write of a batch, as the dict the functions below take."""
    wn = None
    if hasattr(wire_ptr, "data_ptr"):
        wire_ptr, wn = wire_ptr.data_ptr(), wire_ptr.numel() * wire_ptr.element_size()
    return dict(frags=frags, wire_ptr=None if wire_ptr is None else int(wire_ptr),
                wire_cap=(wn or 0) if wire_cap is None else wire_cap, offset_in_block=offset_in_block, seqno=seqno,
                finish=finish, iovcnt=iovcnt)


def entries(writes, query=False):
    """The C array of a list of write dicts.  query: wire NULL in every entry.
    -> (array, the IoVec arrays it points to: keep them alive with it)."""
    arr, keep = (BatchWrite * max(1, len(writes)))(), []
    for e, w in zip(arr, writes):
        w = write(**w)
        fr = w["frags"]
        if isinstance(fr, ctypes.Array):
            vec = fr
        else:
            vec = (IoVec * max(1, len(fr)))(*[IoVec(p if n else None, n) for p, n in fr])
        cnt = len(fr) if w["iovcnt"] is None else w["iovcnt"]
        keep.append(vec)
        e.iov = ctypes.cast(vec, ctypes.POINTER(IoVec))
        e.iovcnt = cnt
        e.offset_in_block = w["offset_in_block"]
        e.seqno = w["seqno"]
        e.finish = int(bool(w["finish"]))
        e.wire = None if query else w["wire_ptr"]
        e.wire_cap = 0 if query else w["wire_cap"]
    return arr, keep


def layout(writes, proto=PROTO_V2, ctype=CSUM_CRC32C):
    """hdfs_wirev_fused_batch_layout (host only; only the fragments' lengths count).
    -> ([{len, wire_len, npkts, first_pkt} per write], dict of struct hdfs_wirev_fused_batch_totals' fields)."""
    (arr, _keep), tot = entries(writes, query=True), Totals()
    _check(load().hdfs_wirev_fused_batch_layout(arr, len(writes), proto, ctype, ctypes.byref(tot)))
    return [arr[k].out() for k in range(len(writes))], tot.as_dict()


def _split(arr, n, recs):
    return [(arr[k].wire_len, recs[arr[k].first_pkt:arr[k].first_pkt + arr[k].npkts]) for k in range(n)]


def packet_records(writes, proto=PROTO_V2, ctype=CSUM_CRC32C):
    """The size query of hdfs_wirev_fused_batch_compose (no GPU; no base is read).
    -> [(wire_len, [packet dicts]) per write], hdr_off counting in the write's
    own stream, data_off in its fragments' concatenation."""
    lib, n = load(), len(writes)
    (arr, _keep), npk = entries(writes, query=True), _sz(0)
    _check(lib.hdfs_wirev_fused_batch_compose(arr, n, proto, ctype, None, 0, ctypes.byref(npk), None))
    pk = (OutPacket * max(1, npk.value))()
    _check(lib.hdfs_wirev_fused_batch_compose(arr, n, proto, ctype, pk, npk.value, ctypes.byref(npk), None))
    return _split(arr, n, [pk[i].as_dict() for i in range(npk.value)])


def compose(writes, proto=PROTO_V2, ctype=CSUM_CRC32C, stream=None):
    """hdfs_wirev_fused_batch_compose: the stream of every write of the batch,
    write k's at its wire_ptr.  -> [(wire_len, [packet dicts]) per write];
    packet i's header buffer starts at wire_ptr + hdr_off, its data at hdr_off
    + hdr_len."""
    lib, n = load(), len(writes)
    tot = Totals()
    arr, _keep = entries(writes, query=True)
    _check(lib.hdfs_wirev_fused_batch_layout(arr, n, proto, ctype, ctypes.byref(tot)))
    (arr, _keep), npk = entries(writes), _sz(0)
    pk = (OutPacket * max(1, tot.npkts))()
    _check(lib.hdfs_wirev_fused_batch_compose(arr, n, proto, ctype, pk, tot.npkts, ctypes.byref(npk), stream))
    return _split(arr, n, [pk[i].as_dict() for i in range(npk.value)])


def fused_batch_time(writes, proto=PROTO_V2, ctype=CSUM_CRC32C, flags=0, iters=10):
    """hdfs_wirev_fused_batch_time: milliseconds of one launch of the fused gather batch kernel."""
    ms = ctypes.c_double(0)
    arr, _keep = entries(writes)
    _check(load().hdfs_wirev_fused_batch_time(arr, len(writes), proto, ctype, flags, iters, ctypes.byref(ms)))
    return ms.value
