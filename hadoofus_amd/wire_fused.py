"""ctypes mirror of include/hadoofus_wire_fused.h (libhadoofus_wire_fused.so).

A write's outgoing packets as one wire stream in device memory, as wire.py
gives them, but in one pass over the data: the library's own kernel computes
the chunk CRCs while it copies.  Same arguments, same records, same bytes as
wire.compose_wire.  The companion library is loaded on first use, after the
product library (it links against it), and refused when its
hdfs_wire_fused_abi_version() is not the one these bindings were written for.
No compute here and no fallback.
"""
import ctypes
import os

from . import abi
from .abi import CSUM_CRC32C, PROTO_V2, CRC32CError, OutPacket, _int, _sz, _u64, _vp

LIB_PATH = os.path.join(os.path.dirname(abi.LIB_PATH), "libhadoofus_wire_fused.so")
ABI_VERSION = 1  # include/hadoofus_wire_fused.h HDFS_WIRE_FUSED_ABI_VERSION these bindings are written for
MAX_GROUPS = 1024  # workgroups HDFS_WIRE_FUSED_TIME_GROUPS accepts

_lib = None


def time_groups(n):
    """HDFS_WIRE_FUSED_TIME_GROUPS(n)."""
    return n << 8


def check_abi(lib):
    v = lib.hdfs_wire_fused_abi_version()
    if v != ABI_VERSION:
        raise ImportError(f"fused wire library ABI version {v}, bindings written for {ABI_VERSION}")
    return lib


def bind(lib):
    """Bind the C ABI of include/hadoofus_wire_fused.h on lib."""
    b = abi._bind
    i64 = ctypes.c_int64
    b(lib, "hdfs_wire_fused_abi_version", _int, [])
    b(lib, "hdfs_wire_fused_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_wire_fused_compose_packets", _int,
      [_vp, _u64, i64, i64, _int, _int, _int, _vp, _u64, ctypes.POINTER(OutPacket), _sz, ctypes.POINTER(_sz),
       ctypes.POINTER(_u64), _vp])
    b(lib, "hdfs_wire_fused_time", _int,
      [_vp, _u64, i64, _int, _int, _int, _vp, _u64, ctypes.c_uint, _int, ctypes.POINTER(ctypes.c_double)])
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
        raise CRC32CError(rc, load().hdfs_wire_fused_last_error().decode(errors="replace"))


def packet_records(nbytes, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """The size query of hdfs_wire_fused_compose_packets (no GPU).
    -> (wire_len, [packet dicts]), hdr_off counting in the stream."""
    lib = load()
    npk, wl = _sz(0), _u64(0)
    args = (None, nbytes, offset_in_block, seqno, proto, ctype, int(finish))  # a size query reads no data
    _check(lib.hdfs_wire_fused_compose_packets(*args, None, 0, None, 0, ctypes.byref(npk), ctypes.byref(wl), None))
    arr = (OutPacket * max(1, npk.value))()
    _check(lib.hdfs_wire_fused_compose_packets(*args, None, 0, arr, npk.value, ctypes.byref(npk), ctypes.byref(wl),
                                               None))
    return wl.value, [arr[i].as_dict() for i in range(npk.value)]


def compose_wire(dptr, nbytes, wire_ptr, wire_cap, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C,
                 finish=False, stream=None):
    """hdfs_wire_fused_compose_packets: the packets of the write of nbytes at
    device pointer dptr, as one stream at device pointer wire_ptr (wire_cap
    bytes of room).  -> (wire_len, [packet dicts]); packet i's header buffer
    starts at wire_ptr + hdr_off, its data at hdr_off + hdr_len."""
    lib = load()
    npk, wl = _sz(0), _u64(0)
    args = (dptr if nbytes else None, nbytes, offset_in_block, seqno, proto, ctype, int(finish))
    _check(lib.hdfs_wire_fused_compose_packets(*args, None, 0, None, 0, ctypes.byref(npk), ctypes.byref(wl), None))
    arr = (OutPacket * max(1, npk.value))()
    _check(lib.hdfs_wire_fused_compose_packets(*args, wire_ptr, wire_cap, arr, npk.value, ctypes.byref(npk),
                                               ctypes.byref(wl), stream))
    return wl.value, [arr[i].as_dict() for i in range(npk.value)]


def fused_time(dptr, nbytes, wire_ptr, wire_cap, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C,
               finish=False, flags=0, iters=10):
    """hdfs_wire_fused_time: milliseconds of one launch of the fused kernel."""
    ms = ctypes.c_double(0)
    _check(load().hdfs_wire_fused_time(dptr, nbytes, offset_in_block, proto, ctype, int(finish), wire_ptr, wire_cap,
                                       flags, iters, ctypes.byref(ms)))
    return ms.value
