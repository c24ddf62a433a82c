"""hadoofus_read -- the read side's batch library, beside hadoofus_amd.

A batch of block reads in one call (include/hadoofus_read_batch.h: the packet
streams of many block transfers verified and de-framed into device buffers by
one launch) lives in libhadoofus_read_batch.so, built by hadoofus_amd.build
beside the product library and loaded on first use (read_batch.py).  A thin
ctypes mirror of that ABI on hadoofus_amd.companion's loader: no compute here
and no fallback of its own.  A batch of positional reads
(include/hadoofus_pread_batch.h: each read's window of its stream) lives in
libhadoofus_pread_batch.so, built and loaded the same way (pread_batch.py, the
module hadoofus_read.pread_batch).  A batch of scatter reads
(include/hadoofus_preadv_batch.h: each read's window laid over a list of device
fragments) lives in libhadoofus_preadv_batch.so, built and loaded the same way
(preadv_batch.py, the module hadoofus_read.preadv_batch).  The MD5CRC block
digests and the file checksum taken from packet streams
(include/hadoofus_md5crc_streams.h: the chunk CRCs digested where they lie in
the streams) live in libhadoofus_md5crc_streams.so, built and loaded the same
way (md5crc_streams.py, the module hadoofus_read.md5crc_streams).  The
composite CRCs of blocks and files taken from the same streams
(include/hadoofus_crc_streams.h: the chunk CRCs folded where they lie, HDFS's
COMPOSITE_CRC mode) live in libhadoofus_crc_streams.so, built and loaded the
same way (crc_streams.py, the module hadoofus_read.crc_streams).  A batch of
verified reads re-framed as writes (include/hadoofus_relay_batch.h: each
stream's payload verified and written out again as a write's packet stream in
one pass) lives in libhadoofus_relay_batch.so, built and loaded the same way
(relay_batch.py, the module hadoofus_read.relay_batch).  Importing the package
loads nothing.
"""
from . import crc_streams  # noqa: F401  (binds nothing until first use)
from . import md5crc_streams  # noqa: F401  (binds nothing until first use)
from . import pread_batch  # noqa: F401  (binds nothing until first use)
from . import preadv_batch  # noqa: F401  (binds nothing until first use)
from . import relay_batch  # noqa: F401  (binds nothing until first use)
from .read_batch import (  # noqa: F401  (binds nothing until first use)
    ABI_VERSION, LIB_PATH, MAX_ENTRIES, MAX_GROUPS, PATH_FALLBACK, PATH_KERNEL, Entry, entry, read_blocks, time,
    time_groups,
)

__all__ = [n for n in dir() if not n.startswith("_")]
