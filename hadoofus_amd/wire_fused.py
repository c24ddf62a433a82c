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
from functools import partial

from . import abi, companion
from .abi import CSUM_CRC32C, PROTO_V2, OutPacket, _int, _sz, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_wire_fused.h HDFS_WIRE_FUSED_ABI_VERSION these bindings are written for
MAX_GROUPS = 1024  # workgroups HDFS_WIRE_FUSED_TIME_GROUPS accepts
time_groups = companion.time_groups  # HDFS_WIRE_FUSED_TIME_GROUPS(n)

_lib = None  # the loaded library: None until the first load()


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


_so = companion.Library("wire_fused", "fused wire", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the companion library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def packet_records(nbytes, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """The size query of hdfs_wire_fused_compose_packets (no GPU).
    -> (wire_len, [packet dicts]), hdr_off counting in the stream."""
    args = (None, nbytes, offset_in_block, seqno, proto, ctype, int(finish))  # a size query reads no data
    return companion.compose_packets(_check, partial(load().hdfs_wire_fused_compose_packets, *args))


def compose_wire(dptr, nbytes, wire_ptr, wire_cap, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C,
                 finish=False, stream=None):
    """hdfs_wire_fused_compose_packets: the packets of the write of nbytes at
    device pointer dptr, as one stream at device pointer wire_ptr (wire_cap
    bytes of room).  -> (wire_len, [packet dicts]); packet i's header buffer
    starts at wire_ptr + hdr_off, its data at hdr_off + hdr_len."""
    args = (dptr if nbytes else None, nbytes, offset_in_block, seqno, proto, ctype, int(finish))
    return companion.compose_packets(_check, partial(load().hdfs_wire_fused_compose_packets, *args), wire_ptr,
                                     wire_cap, stream)


def fused_time(dptr, nbytes, wire_ptr, wire_cap, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C,
               finish=False, flags=0, iters=10):
    """hdfs_wire_fused_time: milliseconds of one launch of the fused kernel."""
    ms = ctypes.c_double(0)
    _check(load().hdfs_wire_fused_time(dptr, nbytes, offset_in_block, proto, ctype, int(finish), wire_ptr, wire_cap,
                                       flags, iters, ctypes.byref(ms)))
    return ms.value
