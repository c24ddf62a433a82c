"""ctypes mirror of include/hadoofus_wire.h (libhadoofus_wire.so).

A write's outgoing packets as one wire stream in device memory: the bytes the
read side (abi.verify_packets / read_packets with dptr=) consumes.  The
companion library is loaded on first use, after the product library (it links
against it), and refused when its hdfs_wire_abi_version() is not the one these
bindings were written for.  No compute here and no fallback.
"""
import ctypes
from functools import partial

from . import abi, companion
from .abi import CSUM_CRC32C, PROTO_V2, OutPacket, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_wire.h HDFS_WIRE_ABI_VERSION these bindings are written for
TIME_SC1 = 1  # HDFS_WIRE_TIME_SC1
time_slices = companion.time_groups  # HDFS_WIRE_TIME_SLICES(n)

_lib = None  # the loaded library: None until the first load()


class LayoutInfo(companion.Record):
    """struct hdfs_wire_layout_info."""
    _fields_ = [
        ("npkts", _u64),
        ("nchunks", _u64),
        ("wire_len", _u64),
        ("packet_stride", _u32),
        ("header_bytes", _u32),
        ("head_bytes", _u32),
        ("reserved", _u32),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_wire.h on lib."""
    b = abi._bind
    i64 = ctypes.c_int64
    b(lib, "hdfs_wire_abi_version", _int, [])
    b(lib, "hdfs_wire_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_wire_compose_packets", _int,
      [_vp, _u64, i64, i64, _int, _int, _int, _vp, _u64, ctypes.POINTER(OutPacket), _sz, ctypes.POINTER(_sz),
       ctypes.POINTER(_u64), _vp])
    b(lib, "hdfs_wire_layout", _int, [_u64, i64, _int, _int, _int, ctypes.POINTER(LayoutInfo)])
    b(lib, "hdfs_wire_frame_time", _int,
      [_vp, _u64, i64, _int, _int, _int, _vp, _u64, ctypes.c_uint, _int, ctypes.POINTER(ctypes.c_double)])
    return check_abi(lib)


_so = companion.Library("wire", "wire", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the companion library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def layout(nbytes, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """hdfs_wire_layout (host only): the shape of the stream of a write of
    nbytes.  -> dict of struct hdfs_wire_layout_info's fields."""
    info = LayoutInfo()
    _check(load().hdfs_wire_layout(nbytes, offset_in_block, proto, ctype, int(finish), ctypes.byref(info)))
    return info.as_dict()


def packet_records(nbytes, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """The size query of hdfs_wire_compose_packets (no GPU).
    -> (wire_len, [packet dicts]), hdr_off counting in the stream."""
    args = (None, nbytes, offset_in_block, seqno, proto, ctype, int(finish))  # a size query reads no data
    return companion.compose_packets(_check, partial(load().hdfs_wire_compose_packets, *args))


def compose_wire(dptr, nbytes, wire_ptr, wire_cap, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C,
                 finish=False, stream=None):
    """hdfs_wire_compose_packets: the packets of the write of nbytes at device
    pointer dptr, as one stream at device pointer wire_ptr (wire_cap bytes of
    room).  -> (wire_len, [packet dicts]); packet i's header buffer starts at
    wire_ptr + hdr_off, its data at hdr_off + hdr_len."""
    args = (dptr if nbytes else None, nbytes, offset_in_block, seqno, proto, ctype, int(finish))
    return companion.compose_packets(_check, partial(load().hdfs_wire_compose_packets, *args), wire_ptr, wire_cap,
                                     stream)


def frame_time(dptr, nbytes, wire_ptr, wire_cap, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C,
               finish=False, flags=0, iters=10):
    """hdfs_wire_frame_time: milliseconds of one launch of the frame kernel."""
    ms = ctypes.c_double(0)
    _check(load().hdfs_wire_frame_time(dptr, nbytes, offset_in_block, proto, ctype, int(finish), wire_ptr, wire_cap,
                                       flags, iters, ctypes.byref(ms)))
    return ms.value
