"""hadoofus_amd -- MI355X-native CRC32C chunk engine for hadoofus's datanode path.

The product is the C-ABI shared library ``hadoofus_amd/lib/libhadoofus_crc32c.so``
(include/hadoofus_crc32c.h, include/crc32c.h).  This package is a thin ctypes
mirror of that ABI used by the tests and bench; it has no compute of its own
and no fallback: if the library or a gfx950 device is missing, calls fail.
Tuning knobs live only in the separate diagnostic build (tools/diaglib.py).
The MD5CRC block / file checksums (include/hadoofus_md5crc.h) live in the
companion library libhadoofus_md5crc.so, loaded on first use (md5crc.py).
Gather writes (include/hadoofus_writev.h: a write's packets composed from a
list of device buffers) live in libhadoofus_writev.so, loaded the same way
(writev.py).  A write's packets as one wire stream in device memory
(include/hadoofus_wire.h: what verify_packets / read_packets consume) live in
libhadoofus_wire.so, loaded the same way (wire.py); the streams of a batch of
writes in one call (include/hadoofus_wire_batch.h) in
libhadoofus_wire_batch.so (wire_batch.py); a write held in a list of device
buffers as one such stream (include/hadoofus_wirev.h) in libhadoofus_wirev.so
(wirev.py); a write's stream made in one pass, the chunk CRCs computed by the
framing kernel (include/hadoofus_wire_fused.h), in libhadoofus_wire_fused.so
(wire_fused.py); the streams of a batch of writes made that way in one launch
(include/hadoofus_wire_fused_batch.h) in libhadoofus_wire_fused_batch.so
(wire_fused_batch.py); a write held in a list of device buffers made that way
(include/hadoofus_wirev_fused.h) in libhadoofus_wirev_fused.so
(wirev_fused.py); the streams of a batch of such writes in one launch
(include/hadoofus_wirev_fused_batch.h) in libhadoofus_wirev_fused_batch.so
(wirev_fused_batch.py).
"""
from .abi import (  # noqa: F401
    LIB_PATH, bind_product, bind_diag, CSUM_NULL, CSUM_CRC32, CSUM_CRC32C, ERR_BAD_CHECKSUM, ERR_CRC_LEN,
    ERR_PACKET_SIZE, ERR_INVALID_PACKETHEADERPROTO, ERR_UNEXPECTED_CRC_LEN, ERR_UNEXPECTED_READ_OFFSET,
    ERR_BAD_LASTPACKET, READ_ALL, PROTO_V1, PROTO_V2, Packet, parse_packets, verify_packets, read_packets,
    AGAIN, IoVec, ERR_UNSUPPORTED_CHECKSUM, MODE_COMPUTE, MODE_VERIFY, SEG_BE, SEG_RAW, SEG_CRC32,
    CRC32CError, DeviceBuffer, Mailbox, Plan, Segment, Session, crc32c, compose_crcs, compose_packets,
    composite_crcs, compute_host, verify_host, PinnedBuffer, corrupt, fill_splitmix64, stream_create,
    stream_sync, device_info, init, bound_device, device_sync, load, stream_crc_dev, stream_ex,
    verify_crcdata, VerifyJob, VerifyBlocksJob, Reader, read_packets_fd, EIO,
)
from .md5crc import (  # noqa: F401  (binds nothing until first use)
    FileChecksum, block_md5crcs, file_checksum, file_checksum_from_blocks, md5_host,
)
from .writev import compose_packets_iov, layout as writev_layout  # noqa: F401  (binds nothing until first use)
from .wire import compose_wire, layout as wire_layout  # noqa: F401  (binds nothing until first use)
from .wire_batch import compose_wire_batch, layout as wire_batch_layout  # noqa: F401  (binds nothing until first use)
from .wirev import compose_wire as compose_wire_iov, layout as wirev_layout  # noqa: F401  (binds nothing until first use)
from .wire_fused import compose_wire as compose_wire_fused  # noqa: F401  (binds nothing until first use)
from .wire_fused_batch import compose as compose_wire_fused_batch  # noqa: F401  (binds nothing until first use)
from .wirev_fused import compose_wirev_fused, layout as wirev_fused_layout  # noqa: F401  (binds nothing until first use)
from .wirev_fused_batch import compose as compose_wirev_fused_batch, layout as wirev_fused_batch_layout  # noqa: F401  (binds nothing until first use)

__all__ = [n for n in dir() if not n.startswith("_")]
