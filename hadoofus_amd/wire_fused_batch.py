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

from . import abi, companion
from .abi import CSUM_CRC32C, PROTO_V2, OutPacket, _int, _sz, _vp
from .companion import BatchWrite, Totals, write  # noqa: F401  (struct hdfs_wire_fused_batch_write, ..._totals)

ABI_VERSION = 1  # include/hadoofus_wire_fused_batch.h HDFS_WIRE_FUSED_BATCH_ABI_VERSION these bindings are written for
MAX_WRITES = 65536  # HDFS_WIRE_FUSED_BATCH_MAX_WRITES
MAX_GROUPS = 1024  # workgroups HDFS_WIRE_FUSED_BATCH_TIME_GROUPS accepts
time_groups = companion.time_groups  # HDFS_WIRE_FUSED_BATCH_TIME_GROUPS(n)
_split = companion.split

_lib = None  # the loaded library: None until the first load()


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


_so = companion.Library("wire_fused_batch", "fused wire batch", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the companion library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def entries(writes, query=False):
    """The C array of a list of write dicts.  query: wire NULL in every entry."""
    return companion.entries(writes, query)[0]


def layout(writes, proto=PROTO_V2, ctype=CSUM_CRC32C):
    """hdfs_wire_fused_batch_layout (host only).
    -> ([{wire_len, npkts, first_pkt} per write], dict of struct hdfs_wire_fused_batch_totals' fields)."""
    return companion.batch_layout(_so, load(), writes, proto, ctype)


def packet_records(writes, proto=PROTO_V2, ctype=CSUM_CRC32C):
    """The size query of hdfs_wire_fused_batch_compose (no GPU).
    -> [(wire_len, [packet dicts]) per write], hdr_off counting in the write's own stream."""
    return companion.batch_packet_records(_so, load(), writes, proto, ctype)


def compose(writes, proto=PROTO_V2, ctype=CSUM_CRC32C, stream=None):
    """hdfs_wire_fused_batch_compose: the stream of every write of the batch,
    write k's at its wire_ptr.  -> [(wire_len, [packet dicts]) per write];
    packet i's header buffer starts at wire_ptr + hdr_off, its data at hdr_off
    + hdr_len."""
    return companion.batch_compose(_so, load(), writes, proto, ctype, stream)


def fused_batch_time(writes, proto=PROTO_V2, ctype=CSUM_CRC32C, flags=0, iters=10):
    """hdfs_wire_fused_batch_time: milliseconds of one launch of the fused batch kernel."""
    ms = ctypes.c_double(0)
    _check(load().hdfs_wire_fused_batch_time(entries(writes), len(writes), proto, ctype, flags, iters,
                                             ctypes.byref(ms)))
    return ms.value
