"""ctypes mirror of include/hadoofus_wirev_fused.h (libhadoofus_wirev_fused.so).

A write held in a list of device buffers as one wire stream in device memory,
as wirev.py gives it, but in one pass over the fragments: the library's own
kernel computes the chunk CRCs while it copies, and finds the fragments through
one table.  Same arguments, same records, same bytes as wirev.compose_wire.
The companion library is loaded on first use, after the product library (it
links against it), and refused when its hdfs_wirev_fused_abi_version() is not
the one these bindings were written for.  No compute here and no fallback.
"""
import ctypes
import os

from . import abi
from .abi import CSUM_CRC32C, PROTO_V2, CRC32CError, IoVec, OutPacket, _int, _sz, _u32, _u64, _vp

LIB_PATH = os.path.join(os.path.dirname(abi.LIB_PATH), "libhadoofus_wirev_fused.so")
ABI_VERSION = 1  # include/hadoofus_wirev_fused.h HDFS_WIREV_FUSED_ABI_VERSION these bindings are written for
MAX_GROUPS = 1024  # workgroups HDFS_WIREV_FUSED_TIME_GROUPS accepts

_lib = None


def time_groups(n):
    """HDFS_WIREV_FUSED_TIME_GROUPS(n)."""
    return n << 8


class LayoutInfo(ctypes.Structure):
    """struct hdfs_wirev_fused_layout_info."""
    _fields_ = [
        ("npkts", _u64),
        ("nchunks", _u64),
        ("wire_len", _u64),
        ("nfrags", _u64),
        ("rounds", _u64),
        ("seamed_rounds", _u64),
        ("seamed_ragged", _u64),
        ("packet_stride", _u32),
        ("header_bytes", _u32),
        ("head_bytes", _u32),
        ("max_frags_per_round", _u32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


def check_abi(lib):
    v = lib.hdfs_wirev_fused_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"fused wirev library ABI version {v}, bindings written for {ABI_VERSION}")
    return lib


def bind(lib):
    """Bind the C ABI of include/hadoofus_wirev_fused.h on lib."""
    b = abi._bind
    i64 = ctypes.c_int64
    b(lib, "hdfs_wirev_fused_abi_version", _int, [])
    b(lib, "hdfs_wirev_fused_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_wirev_fused_compose_packets", _int,
      [ctypes.POINTER(IoVec), _int, i64, i64, _int, _int, _int, _vp, _u64, ctypes.POINTER(OutPacket), _sz,
       ctypes.POINTER(_sz), ctypes.POINTER(_u64), _vp])
    b(lib, "hdfs_wirev_fused_layout", _int,
      [ctypes.POINTER(_u64), _int, i64, _int, _int, _int, ctypes.POINTER(LayoutInfo)])
    b(lib, "hdfs_wirev_fused_time", _int,
      [ctypes.POINTER(IoVec), _int, i64, _int, _int, _int, _vp, _u64, ctypes.c_uint, _int,
       ctypes.POINTER(ctypes.c_double)])
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
        raise CRC32CError(rc, load().hdfs_wirev_fused_last_error().decode(errors="replace"))


def iovecs(frags):
    """frags: (device ptr or None, nbytes) pairs -> (IoVec array, count)."""
    vec = [IoVec(p if n else None, n) for p, n in frags]
    return (IoVec * max(1, len(vec)))(*vec), len(vec)


def layout(lens, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """hdfs_wirev_fused_layout (host only): the shape of the stream of a write
    of these fragment lengths and the paths its rounds take in the kernel.
    -> dict of struct hdfs_wirev_fused_layout_info's fields."""
    n = len(lens)
    arr = (_u64 * max(1, n))(*lens)
    info = LayoutInfo()
    _check(load().hdfs_wirev_fused_layout(arr, n, offset_in_block, proto, ctype, int(finish), ctypes.byref(info)))
    return info.as_dict()


def packet_records(lens, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """The size query of hdfs_wirev_fused_compose_packets (no GPU; only the
    fragments' lengths count).  -> (wire_len, [packet dicts]), hdr_off
    counting in the stream, data_off in the fragments' concatenation."""
    lib = load()
    n = len(lens)
    vec = (IoVec * max(1, n))(*[IoVec(None, l) for l in lens])  # a size query reads no base
    npk, wl = _sz(0), _u64(0)
    args = (vec, n, offset_in_block, seqno, proto, ctype, int(finish))
    _check(lib.hdfs_wirev_fused_compose_packets(*args, None, 0, None, 0, ctypes.byref(npk), ctypes.byref(wl), None))
    arr = (OutPacket * max(1, npk.value))()
    _check(lib.hdfs_wirev_fused_compose_packets(*args, None, 0, arr, npk.value, ctypes.byref(npk), ctypes.byref(wl),
                                                None))
    return wl.value, [arr[i].as_dict() for i in range(npk.value)]


def compose_wirev_fused(frags, wire_ptr, wire_cap, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C,
                        finish=False, stream=None):
    """hdfs_wirev_fused_compose_packets: the packets of the write held in
    frags, a list of (device ptr, nbytes) pairs, as one stream at device
    pointer wire_ptr (wire_cap bytes of room).  -> (wire_len, [packet dicts]);
    packet i's header buffer starts at wire_ptr + hdr_off, its data at hdr_off
    + hdr_len."""
    lib = load()
    vec, n = iovecs(frags)
    npk, wl = _sz(0), _u64(0)
    args = (vec, n, offset_in_block, seqno, proto, ctype, int(finish))
    _check(lib.hdfs_wirev_fused_compose_packets(*args, None, 0, None, 0, ctypes.byref(npk), ctypes.byref(wl), None))
    arr = (OutPacket * max(1, npk.value))()
    _check(lib.hdfs_wirev_fused_compose_packets(*args, wire_ptr, wire_cap, arr, npk.value, ctypes.byref(npk),
                                                ctypes.byref(wl), stream))
    return wl.value, [arr[i].as_dict() for i in range(npk.value)]


def fused_time(frags, wire_ptr, wire_cap, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False,
               flags=0, iters=10):
    """hdfs_wirev_fused_time: milliseconds of one launch of the fused gather kernel."""
    vec, n = iovecs(frags)
    ms = ctypes.c_double(0)
    _check(load().hdfs_wirev_fused_time(vec, n, offset_in_block, proto, ctype, int(finish), wire_ptr, wire_cap,
                                        flags, iters, ctypes.byref(ms)))
    return ms.value
