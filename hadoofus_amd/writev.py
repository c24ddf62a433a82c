"""ctypes mirror of include/hadoofus_writev.h (libhadoofus_writev.so).

Gather writes: the outgoing packets of a write held in a list of device (or
host) buffers, byte-identical to abi.compose_packets of their concatenation.
The companion library is loaded on first use, after the product library (it
links against it), and refused when its hdfs_writev_abi_version() is not the
one these bindings were written for.  No compute here and no fallback.
"""
import ctypes

import numpy as np

from . import abi, companion
from .abi import CSUM_CRC32C, PROTO_V2, IoVec, OutPacket, _host, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_writev.h HDFS_WRITEV_ABI_VERSION these bindings are written for

_lib = None  # the loaded library: None until the first load()


class LayoutInfo(companion.Record):
    """struct hdfs_writev_layout_info."""
    _fields_ = [
        ("total", _u64),
        ("nchunks", _u64),
        ("nsegments", _u64),
        ("seg_chunks", _u64),
        ("ngathered", _u64),
        ("npieces", _u64),
        ("max_pieces", _u32),
        ("min_seg_chunks", _u32),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_writev.h on lib."""
    b = abi._bind
    b(lib, "hdfs_writev_abi_version", _int, [])
    b(lib, "hdfs_writev_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_writev_compose_packets", _int,
      [ctypes.POINTER(IoVec), _int, ctypes.c_int64, ctypes.c_int64, _int, _int, _int, _vp, _u64,
       ctypes.POINTER(OutPacket), _sz, ctypes.POINTER(_sz), ctypes.POINTER(_u64)])
    b(lib, "hdfs_writev_layout", _int, [ctypes.POINTER(_u64), _int, ctypes.c_int64, ctypes.POINTER(LayoutInfo)])
    return check_abi(lib)


_so = companion.Library("writev", "writev", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the companion library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def iovecs(frags):
    """frags: (device ptr, nbytes) pairs and / or host arrays (bytes, numpy)
    -> (IoVec array, count, objects to keep alive)."""
    keep, vec = [], []
    for f in frags:
        if isinstance(f, tuple):
            vec.append(IoVec(f[0], f[1]))
        else:
            a, p, n = _host(f)
            keep.append(a)
            vec.append(IoVec(p if n else None, n))
    return (IoVec * max(1, len(vec)))(*vec), len(vec), keep


def compose_packets_iov(frags, offset_in_block=0, seqno=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """hdfs_writev_compose_packets: the outgoing packets of one write held in
    frags, a list of (device ptr, nbytes) pairs or of host arrays.
    -> (header bytes, [packet dicts]), data_off counting in the fragments'
    concatenation: what abi.compose_packets returns for it."""
    lib = load()
    vec, n, keep = iovecs(frags)
    npk, used = _sz(0), _u64(0)
    args = (vec, n, offset_in_block, seqno, proto, ctype, int(finish))
    _check(lib.hdfs_writev_compose_packets(*args, None, 0, None, 0, ctypes.byref(npk), ctypes.byref(used)))
    hdr = np.zeros(max(1, used.value), dtype=np.uint8)
    arr = (OutPacket * max(1, npk.value))()
    _check(lib.hdfs_writev_compose_packets(*args, hdr.ctypes.data, used.value, arr, npk.value, ctypes.byref(npk),
                                           ctypes.byref(used)))
    return hdr[: used.value].tobytes(), [arr[i].as_dict() for i in range(npk.value)]


def layout(lens, offset_in_block=0):
    """hdfs_writev_layout (host only): how a write of these fragment lengths
    is split between in-place segments and gathered chunks.  -> dict of
    struct hdfs_writev_layout_info's fields."""
    (arr, n), info = companion.lengths(lens), LayoutInfo()
    _check(load().hdfs_writev_layout(arr, n, offset_in_block, ctypes.byref(info)))
    return info.as_dict()
