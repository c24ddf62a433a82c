"""What the bindings of the companion libraries share.

Every companion libhadoofus_<stem>.so lies beside the product library, links
against it, and exports hdfs_<stem>_abi_version and hdfs_<stem>_last_error
next to its own entry points.  Here is what follows from that alone: the
loader (Library), the two-call idiom of the *_compose_packets entry points
(compose_packets), the front end of the batch libraries (write, entries,
batch_layout, batch_packet_records, batch_compose) and a few small helpers.
What a library has of its own (its structures, the signatures it binds, the
argument order of its calls) stays in hadoofus_amd/<stem>.py.  No compute here
and no fallback.
"""
import ctypes
import os

from . import abi
from .abi import CRC32CError, IoVec, OutPacket, _sz, _u64, _vp


class Library:
    """The loader of libhadoofus_<stem>.so.  noun: what the ABI error message
    calls the library; abi_version: the version the bindings are written for;
    bind: binds the library's C ABI on a handle and returns it."""

    def __init__(self, stem, noun, abi_version, bind):
        self.stem, self.noun, self.abi_version, self.bind = stem, noun, abi_version, bind
        self.path = os.path.join(os.path.dirname(abi.LIB_PATH), f"libhadoofus_{stem}.so")
        self.lib = None

    def check_abi(self, lib):
        v = getattr(lib, f"hdfs_{self.stem}_abi_version")()
        if v != self.abi_version:
            raise ImportError(f"{self.noun} library ABI version {v}, bindings written for {self.abi_version}")
        return lib

    def load(self, path=None):
        """Load the companion library (raises if it was not built)."""
        if self.lib is not None:
            return self.lib
        path = self.path if path is None else path
        abi.load()  # first: the companion links against the product library
        if not os.path.exists(path):
            raise ImportError(f"{path} not built; run `python -m hadoofus_amd.build` "
                              "(or __graft_entry__.build())")
        self.lib = self.bind(ctypes.CDLL(path))
        return self.lib

    def check(self, rc):
        if rc != 0:
            raise CRC32CError(rc, getattr(self.load(), f"hdfs_{self.stem}_last_error")().decode(errors="replace"))

    def call(self, lib, name, *args):
        """hdfs_<stem>_<name>(*args) on the loaded library lib, checked."""
        self.check(getattr(lib, f"hdfs_{self.stem}_{name}")(*args))


# ---- small helpers -------------------------------------------------------------------------
class Record(ctypes.Structure):
    """A structure whose as_dict() gives its fields without `reserved`."""

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved"}


def time_groups(n):
    """HDFS_<STEM>_TIME_GROUPS(n) / HDFS_<STEM>_TIME_SLICES(n): n in a timing call's flags."""
    return n << 8


def iovecs(frags):
    """frags: (device ptr or None, nbytes) pairs -> (IoVec array, count)."""
    vec = [IoVec(p if n else None, n) for p, n in frags]
    return (IoVec * max(1, len(vec)))(*vec), len(vec)


def lengths(lens):
    """Fragment lengths -> (uint64 array, count)."""
    return (_u64 * max(1, len(lens)))(*lens), len(lens)


def ptr(x):
    """(raw pointer, bytes or None) of a raw pointer or a torch device tensor."""
    if hasattr(x, "data_ptr"):
        return x.data_ptr(), x.numel() * x.element_size()
    return (None if x is None else int(x)), None


# ---- one write: size query, allocate, compose ----------------------------------------------
def compose_packets(check, call, wire_ptr=None, wire_cap=0, stream=None):
    """The two calls of a *_compose_packets entry point.  call takes the
    trailing (wire_ptr, wire_cap, pkts, max_pkts, &npkts, &wire_len, stream) of
    its arguments.  Without wire_ptr the second call is a size query too: it
    only fills the records.  -> (wire_len, [packet dicts])."""
    npk, wl = _sz(0), _u64(0)
    check(call(None, 0, None, 0, ctypes.byref(npk), ctypes.byref(wl), None))
    arr = (OutPacket * max(1, npk.value))()
    check(call(wire_ptr, wire_cap, arr, npk.value, ctypes.byref(npk), ctypes.byref(wl), stream))
    return wl.value, [arr[i].as_dict() for i in range(npk.value)]


# ---- a batch of writes ---------------------------------------------------------------------
class BatchWrite(ctypes.Structure):
    """struct hdfs_wire_batch_write and struct hdfs_wire_fused_batch_write."""
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

    def source(self, w):
        self.data = w["dptr"] if w["nbytes"] else None
        self.len = w["nbytes"]


class Totals(Record):
    """struct hdfs_wire_batch_totals and struct hdfs_wire_fused_batch_totals."""
    _fields_ = [
        ("npkts", _u64),
        ("nchunks", _u64),
        ("wire_bytes", _u64),
        ("table_entries", _u64),
    ]


def write(dptr=None, nbytes=None, wire_ptr=None, wire_cap=None, offset_in_block=0, seqno=0, finish=False):
    """One write of a batch, as the dict the functions below take."""
    dptr, dn = ptr(dptr)
    wire_ptr, wn = ptr(wire_ptr)
    return dict(dptr=dptr, nbytes=(dn or 0) if nbytes is None else nbytes, wire_ptr=wire_ptr,
                wire_cap=(wn or 0) if wire_cap is None else wire_cap, offset_in_block=offset_in_block, seqno=seqno,
                finish=finish)


def entries(writes, query=False, struct=BatchWrite, write=write):
    """The C array of a list of write dicts.  query: wire NULL in every entry.
    struct.source(w) fills an entry's source from the dict write(**w) and
    returns what the entry then points to, if anything.
    -> (array, what its entries point to: keep it alive with the array)."""
    arr, keep = (struct * max(1, len(writes)))(), []
    for e, w in zip(arr, writes):
        w = write(**w)
        keep.append(e.source(w))
        e.offset_in_block = w["offset_in_block"]
        e.seqno = w["seqno"]
        e.finish = int(bool(w["finish"]))
        e.wire = None if query else w["wire_ptr"]
        e.wire_cap = 0 if query else w["wire_cap"]
    return arr, keep


def split(arr, n, recs):
    return [(arr[k].wire_len, recs[arr[k].first_pkt:arr[k].first_pkt + arr[k].npkts]) for k in range(n)]


def batch_layout(so, lib, writes, proto, ctype, entries=entries, totals=Totals):
    """hdfs_<stem>_layout (host only).  -> ([out() per write], dict of the totals' fields)."""
    (arr, _keep), tot = entries(writes, True), totals()
    so.call(lib, "layout", arr, len(writes), proto, ctype, ctypes.byref(tot))
    return [arr[k].out() for k in range(len(writes))], tot.as_dict()


def _records(so, lib, arr, n, proto, ctype, npkts, stream):
    pk, npk = (OutPacket * max(1, npkts))(), _sz(0)
    so.call(lib, "compose", arr, n, proto, ctype, pk, npkts, ctypes.byref(npk), stream)
    return split(arr, n, [pk[i].as_dict() for i in range(npk.value)])


def batch_packet_records(so, lib, writes, proto, ctype, entries=entries):
    """The size query of hdfs_<stem>_compose (no GPU).  -> [(wire_len, [packet dicts]) per write]."""
    (arr, _keep), n, npk = entries(writes, True), len(writes), _sz(0)
    so.call(lib, "compose", arr, n, proto, ctype, None, 0, ctypes.byref(npk), None)
    return _records(so, lib, arr, n, proto, ctype, npk.value, None)


def batch_compose(so, lib, writes, proto, ctype, stream, entries=entries, totals=Totals):
    """hdfs_<stem>_compose, its records sized by hdfs_<stem>_layout.
    -> [(wire_len, [packet dicts]) per write]."""
    (arr, _keep), n, tot = entries(writes, True), len(writes), totals()
    so.call(lib, "layout", arr, n, proto, ctype, ctypes.byref(tot))
    arr, _keep = entries(writes)
    return _records(so, lib, arr, n, proto, ctype, tot.npkts, stream)
