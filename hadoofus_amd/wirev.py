"""ctypes mirror of include/hadoofus_wirev.h (libhadoofus_wirev.so).

A write held in a list of device buffers as one wire stream in device memory:
byte for byte what wire.compose_wire writes for the fragments' concatenation,
without packing them first.  The companion library is loaded on first use,
after the product library (it links against it), and refused when its
hdfs_wirev_abi_version() is not the one these bindings were written for.  No
compute here and no fallback.
"""
import ctypes
from functools import partial

from . import abi, companion
from .abi import CSUM_CRC32C, PROTO_V2, IoVec, OutPacket, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_wirev.h HDFS_WIREV_ABI_VERSION these bindings are written for
TIME_SC1 = 1  # HDFS_WIREV_TIME_SC1
time_slices = companion.time_groups  # HDFS_WIREV_TIME_SLICES(n)
iovecs = companion.iovecs  # (device ptr or None, nbytes) pairs -> (IoVec array, count)

_lib = None  # the loaded library: None until the first load()


class LayoutInfo(companion.Record):
    """struct hdfs_wirev_layout_info."""
    _fields_ = [
        ("npkts", _u64),
        ("nchunks", _u64),
        ("wire_len", _u64),
        ("nsegments", _u64),
        ("seg_chunks", _u64),
        ("ngathered", _u64),
        ("npieces", _u64),
        ("nfrags", _u64),
        ("packet_stride", _u32),
        ("header_bytes", _u32),
        ("head_bytes", _u32),
        ("max_pieces", _u32),
        ("max_frags_per_packet", _u32),
        ("reserved", _u32),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_wirev.h on lib."""
    b = abi._bind
    i64 = ctypes.c_int64
    b(lib, "hdfs_wirev_abi_version", _int, [])
    b(lib, "hdfs_wirev_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_wirev_compose_packets", _int,
      [ctypes.POINTER(IoVec), _int, i64, i64, _int, _int, _int, _vp, _u64, ctypes.POINTER(OutPacket), _sz,
       ctypes.POINTER(_sz), ctypes.POINTER(_u64), _vp])
    b(lib, "hdfs_wirev_layout", _int, [ctypes.POINTER(_u64), _int, i64, _int, _int, _int, ctypes.POINTER(LayoutInfo)])
    b(lib, "hdfs_wirev_frame_time", _int,
      [ctypes.POINTER(IoVec), _int, i64, _int, _int, _int, _vp, _u64, ctypes.c_uint, _int,
       ctypes.POINTER(ctypes.c_double)])
    return check_abi(lib)


_so = companion.Library("wirev", "wirev", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the companion library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def layout(lens, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """hdfs_wirev_layout (host only): the shape of the stream of a write of
    these fragment lengths and the split of its chunk grid over them.
    -> dict of struct hdfs_wirev_layout_info's fields."""
    (arr, n), info = companion.lengths(lens), LayoutInfo()
    _check(load().hdfs_wirev_layout(arr, n, offset_in_block, proto, ctype, int(finish), ctypes.byref(info)))
    return info.as_dict()


def packet_records(lens, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """The size query of hdfs_wirev_compose_packets (no GPU; only the
    fragments' lengths count).  -> (wire_len, [packet dicts]), hdr_off
    counting in the stream, data_off in the fragments' concatenation."""
    vec, n = iovecs([(None, l) for l in lens])  # a size query reads no base
    args = (vec, n, offset_in_block, seqno, proto, ctype, int(finish))
    return companion.compose_packets(_check, partial(load().hdfs_wirev_compose_packets, *args))


def compose_wire(frags, wire_ptr, wire_cap, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C,
                 finish=False, stream=None):
    """hdfs_wirev_compose_packets: the packets of the write held in frags, a
    list of (device ptr, nbytes) pairs, as one stream at device pointer
    wire_ptr (wire_cap bytes of room).  -> (wire_len, [packet dicts]); packet
    i's header buffer starts at wire_ptr + hdr_off, its data at hdr_off +
    hdr_len."""
    vec, n = iovecs(frags)
    args = (vec, n, offset_in_block, seqno, proto, ctype, int(finish))
    return companion.compose_packets(_check, partial(load().hdfs_wirev_compose_packets, *args), wire_ptr, wire_cap,
                                     stream)


def frame_time(frags, wire_ptr, wire_cap, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False,
               flags=0, iters=10):
    """hdfs_wirev_frame_time: milliseconds of one launch of the frame kernel."""
    vec, n = iovecs(frags)
    ms = ctypes.c_double(0)
    _check(load().hdfs_wirev_frame_time(vec, n, offset_in_block, proto, ctype, int(finish), wire_ptr, wire_cap,
                                        flags, iters, ctypes.byref(ms)))
    return ms.value
