"""ctypes mirror of include/hadoofus_wire_fused_batch.h
(libhadoofus_wire_fused_batch.so).

The wire streams of a batch of writes in one call, one launch and one pass
over the data: the library's own kernel computes every write's chunk CRCs
while it copies.  Same arguments, same records, same bytes as
wire_batch.compose_wire_batch.  The companion library is loaded on first use,
after the product library (it links against it), and refused when its
hdfs_wire_fused_batch_abi_version() is not the one these bindings were written
for.  No compute here and no fallback.

A write is a dict (or keyword arguments of `write`): dptr, nbytes, wire_ptr,
wire_cap, offset_in_block, seqno, finish.  dptr and wire_ptr are raw device
pointers or torch device tensors (their data_ptr() is taken; nbytes and
wire_cap then default to the tensors' sizes).
"""
import ctypes
import os

from . import abi
from .abi import CSUM_CRC32C, PROTO_V2, CRC32CError, OutPacket, _int, _sz, _u64, _vp

LIB_PATH = os.path.join(os.path.dirname(abi.LIB_PATH), "libhadoofus_wire_fused_batch.so")
ABI_VERSION = 1  # include/hadoofus_wire_fused_batch.h HDFS_WIRE_FUSED_BATCH_ABI_VERSION these bindings are written for
MAX_WRITES = 65536  # HDFS_WIRE_FUSED_BATCH_MAX_WRITES
MAX_GROUPS = 1024  # workgroups HDFS_WIRE_FUSED_BATCH_TIME_GROUPS accepts

_lib = None


def time_groups(n):
    """HDFS_WIRE_FUSED_BATCH_TIME_GROUPS(n)."""
    return n << 8


class BatchWrite(ctypes.Structure):
    """struct hdfs_wire_fused_batch_write."""
    _fields_ = [
        ("data", _vp),
        ("len", _u64),
        ("offset_in_block", ctypes.c_int64),
        ("seqno", ctypes.c_int64),
        ("finish", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("wire", _vp),
        ("wire_cap", _u64),
        ("wire_len", _u64),
        ("npkts", _u64),
        ("first_pkt", _u64),
    ]

    def out(self):
        return {"wire_len": self.wire_len, "npkts": self.npkts, "first_pkt": self.first_pkt}


class Totals(ctypes.Structure):
    """struct hdfs_wire_fused_batch_totals."""
    _fields_ = [
        ("npkts", _u64),
        ("nchunks", _u64),
        ("wire_bytes", _u64),
        ("table_entries", _u64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


def check_abi(lib):
    v = lib.hdfs_wire_fused_batch_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"fused wire batch library ABI version {v}, bindings written for {ABI_VERSION}")
    return lib


def bind(lib):
    """Bind the C ABI of include/hadoofus_wire_fused_batch.h on lib."""
    b = abi._bind
    wp = ctypes.POINTER(BatchWrite)
    b(lib, "hdfs_wire_fused_batch_abi_version", _int, [])
    b(lib, "hdfs_wire_fused_batch_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_wire_fused_batch_compose", _int,
      [wp, _sz, _int, _int, ctypes.POINTER(OutPacket), _sz, ctypes.POINTER(_sz), _vp])
    b(lib, "hdfs_wire_fused_batch_layout", _int, [wp, _sz, _int, _int, ctypes.POINTER(Totals)])
    b(lib, "hdfs_wire_fused_batch_time", _int,
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
        raise CRC32CError(rc, load().hdfs_wire_fused_batch_last_error().decode(errors="replace"))


def _ptr(x):
    """(raw pointer, bytes or None) of a raw pointer or a torch device tensor."""
    if hasattr(x, "data_ptr"):
        return x.data_ptr(), x.numel() * x.element_size()
    return (None if x is None else int(x)), None


def write(dptr=None, nbytes=None, wire_ptr=None, wire_cap=None, offset_in_block=0, seqno=0, finish=False):
    """One write of a batch, as the dict the functions below take."""
    dptr, dn = _ptr(dptr)
    wire_ptr, wn = _ptr(wire_ptr)
    return dict(dptr=dptr, nbytes=(dn or 0) if nbytes is None else nbytes, wire_ptr=wire_ptr,
                wire_cap=(wn or 0) if wire_cap is None else wire_cap, offset_in_block=offset_in_block, seqno=seqno,
                finish=finish)


def entries(writes, query=False):
    """The C array of a list of write dicts.  query: wire NULL in every entry."""
    arr = (BatchWrite * max(1, len(writes)))()
    for e, w in zip(arr, writes):
        w = write(**w)
        e.data = w["dptr"] if w["nbytes"] else None
        e.len = w["nbytes"]
        e.offset_in_block = w["offset_in_block"]
        e.seqno = w["seqno"]
        e.finish = int(bool(w["finish"]))
        e.wire = None if query else w["wire_ptr"]
        e.wire_cap = 0 if query else w["wire_cap"]
    return arr


def layout(writes, proto=PROTO_V2, ctype=CSUM_CRC32C):
    """hdfs_wire_fused_batch_layout (host only).
    -> ([{wire_len, npkts, first_pkt} per write], dict of struct hdfs_wire_fused_batch_totals' fields)."""
    arr, tot = entries(writes, query=True), Totals()
    _check(load().hdfs_wire_fused_batch_layout(arr, len(writes), proto, ctype, ctypes.byref(tot)))
    return [arr[k].out() for k in range(len(writes))], tot.as_dict()


def _split(arr, n, recs):
    return [(arr[k].wire_len, recs[arr[k].first_pkt:arr[k].first_pkt + arr[k].npkts]) for k in range(n)]


def packet_records(writes, proto=PROTO_V2, ctype=CSUM_CRC32C):
    """The size query of hdfs_wire_fused_batch_compose (no GPU).
    -> [(wire_len, [packet dicts]) per write], hdr_off counting in the write's own stream."""
    lib, n = load(), len(writes)
    arr, npk = entries(writes, query=True), _sz(0)
    _check(lib.hdfs_wire_fused_batch_compose(arr, n, proto, ctype, None, 0, ctypes.byref(npk), None))
    pk = (OutPacket * max(1, npk.value))()
    _check(lib.hdfs_wire_fused_batch_compose(arr, n, proto, ctype, pk, npk.value, ctypes.byref(npk), None))
    return _split(arr, n, [pk[i].as_dict() for i in range(npk.value)])


def compose(writes, proto=PROTO_V2, ctype=CSUM_CRC32C, stream=None):
    """hdfs_wire_fused_batch_compose: the stream of every write of the batch,
    write k's at its wire_ptr.  -> [(wire_len, [packet dicts]) per write];
    packet i's header buffer starts at wire_ptr + hdr_off, its data at hdr_off
    + hdr_len."""
    lib, n = load(), len(writes)
    tot = Totals()
    _check(lib.hdfs_wire_fused_batch_layout(entries(writes, query=True), n, proto, ctype, ctypes.byref(tot)))
    arr, npk = entries(writes), _sz(0)
    pk = (OutPacket * max(1, tot.npkts))()
    _check(lib.hdfs_wire_fused_batch_compose(arr, n, proto, ctype, pk, tot.npkts, ctypes.byref(npk), stream))
    return _split(arr, n, [pk[i].as_dict() for i in range(npk.value)])


def fused_batch_time(writes, proto=PROTO_V2, ctype=CSUM_CRC32C, flags=0, iters=10):
    """hdfs_wire_fused_batch_time: milliseconds of one launch of the fused batch kernel."""
    ms = ctypes.c_double(0)
    _check(load().hdfs_wire_fused_batch_time(entries(writes), len(writes), proto, ctype, flags, iters,
                                             ctypes.byref(ms)))
    return ms.value
