"""ctypes mirror of include/hadoofus_relay_batch.h (libhadoofus_relay_batch.so).

A batch of verified reads re-framed as writes in one call: every entry's packet
stream, in device memory, is verified and its payload written out again as the
packet stream of a write (the writer's offsetInBlock, seqno and
lastPacketInBlock, packets of 65536 B), with the read's outputs of
hdfs_crc32c_read_packets(..., READ_ALL, ...) and the bytes of
hdfs_wire_fused_compose_packets of that payload.  The library is loaded on
first use, after the product library (it links against it), and refused when
its hdfs_relay_batch_abi_version() is not the one these bindings were written
for.  No compute here.

An entry is a dict (or the keyword arguments of `entry`): stream_ptr, nbytes,
wire_ptr, wire_cap, offset_in_block, seqno, finish.  stream_ptr and wire_ptr are
raw device pointers or torch device tensors (their data_ptr() is taken; nbytes
and wire_cap then default to the tensors' sizes).
"""
import ctypes

from hadoofus_amd import abi, companion
from hadoofus_amd.abi import CSUM_CRC32C, PROTO_V2, _int, _sz, _u32, _u64, _vp

ABI_VERSION = 1  # include/hadoofus_relay_batch.h HDFS_RELAY_BATCH_ABI_VERSION these bindings are written for
MAX_ENTRIES = 1024  # HDFS_RELAY_BATCH_MAX_ENTRIES
MAX_GROUPS = 1024  # workgroups HDFS_RELAY_BATCH_TIME_GROUPS accepts
PATH_KERNEL, PATH_FALLBACK = 0, 1  # HDFS_RELAY_BATCH_PATH_*
time_groups = companion.time_groups  # HDFS_RELAY_BATCH_TIME_GROUPS(n)
OUT = ("rc", "consumed", "delivered", "src_offset_in_block", "wire_len", "npkts", "path")

_lib = None  # the loaded library: None until the first load()


class Entry(ctypes.Structure):
    """struct hdfs_relay_batch_entry."""
    _fields_ = [
        ("stream", _vp),
        ("len", _u64),
        ("offset_in_block", ctypes.c_int64),
        ("seqno", ctypes.c_int64),
        ("finish", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("wire", _vp),
        ("wire_cap", _u64),
        ("consumed", _u64),
        ("delivered", _u64),
        ("src_offset_in_block", ctypes.c_int64),
        ("wire_len", _u64),
        ("npkts", _u64),
        ("rc", ctypes.c_int32),
        ("path", ctypes.c_int32),
    ]


def bind(lib):
    """Bind the C ABI of include/hadoofus_relay_batch.h on lib."""
    b = abi._bind
    ep, u64p = ctypes.POINTER(Entry), ctypes.POINTER(_u64)
    b(lib, "hdfs_relay_batch_abi_version", _int, [])
    b(lib, "hdfs_relay_batch_last_error", ctypes.c_char_p, [])
    b(lib, "hdfs_relay_batch_relay", _int, [ep, _sz, _int, _u32, _int, _vp])
    b(lib, "hdfs_relay_batch_layout", _int, [_u64, ctypes.c_int64, _int, _int, _int, u64p, u64p])
    b(lib, "hdfs_relay_batch_time", _int,
      [ep, _sz, _int, _u32, _int, ctypes.c_uint, _int, ctypes.POINTER(ctypes.c_double)])
    return check_abi(lib)


_so = companion.Library("relay_batch", "relay batch", ABI_VERSION, bind)
LIB_PATH, check_abi, _check = _so.path, _so.check_abi, _so.check


def load(path=LIB_PATH):
    """Load the library (raises if it was not built)."""
    global _lib
    _lib = _so.load(path)
    return _lib


def entry(stream_ptr=None, nbytes=None, wire_ptr=None, wire_cap=None, offset_in_block=0, seqno=0, finish=False):
    """One read re-framed as one write, as the dict the functions below take."""
    stream_ptr, sn = companion.ptr(stream_ptr)
    wire_ptr, wn = companion.ptr(wire_ptr)
    return dict(stream_ptr=stream_ptr, nbytes=(sn or 0) if nbytes is None else nbytes, wire_ptr=wire_ptr,
                wire_cap=(wn or 0) if wire_cap is None else wire_cap, offset_in_block=offset_in_block, seqno=seqno,
                finish=finish)


def entries(batch):
    """The C array of a list of entry dicts."""
    arr = (Entry * max(1, len(batch)))()
    for e, x in zip(arr, batch):
        x = entry(**x)
        e.stream, e.len, e.wire, e.wire_cap = x["stream_ptr"], x["nbytes"], x["wire_ptr"], x["wire_cap"]
        e.offset_in_block, e.seqno, e.finish = x["offset_in_block"], x["seqno"], int(bool(x["finish"]))
    return arr


def _results(arr, n):
    return [{f: getattr(arr[b], f) for f in OUT} for b in range(n)]


def layout(payload, offset_in_block=0, proto=PROTO_V2, ctype=CSUM_CRC32C, finish=False):
    """hdfs_relay_batch_layout (host only).  -> (wire_len, npkts) of the write's stream."""
    wl, npk = _u64(0), _u64(0)
    _check(load().hdfs_relay_batch_layout(payload, offset_in_block, proto, ctype, int(bool(finish)), ctypes.byref(wl),
                                          ctypes.byref(npk)))
    return wl.value, npk.value


def relay(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, stream=None):
    """hdfs_relay_batch_relay.  The call's own refusal raises; what an entry
    ends in -- a packet error, a stream that does not fit, or the main call's
    negative status for it -- is that entry's rc.
    -> [dict(rc, consumed, delivered, src_offset_in_block, wire_len, npkts, path) per entry]."""
    arr, n = entries(batch), len(batch)
    rc = load().hdfs_relay_batch_relay(arr, n, proto, chunk_size, ctype, stream)
    if rc < 0 and not any(arr[b].rc < 0 for b in range(n)):  # the call's own refusal, not an entry's
        _check(rc)
    return _results(arr, n)


def time(batch, proto=PROTO_V2, chunk_size=512, ctype=CSUM_CRC32C, flags=0, iters=10):
    """hdfs_relay_batch_time: the call once, then both launches alone iters times.
    -> (milliseconds of one probe + main launch, [dict per entry] of the first call)."""
    arr, n, ms = entries(batch), len(batch), ctypes.c_double(0)
    rc = load().hdfs_relay_batch_time(arr, n, proto, chunk_size, ctype, flags, iters, ctypes.byref(ms))
    if rc < 0 and not any(arr[b].rc < 0 for b in range(n)):
        _check(rc)
    return ms.value, _results(arr, n)
