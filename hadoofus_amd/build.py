"""Build libhadoofus_crc32c.so in-tree for gfx950 (MI355X) with hipcc.

The shared library is the product: the C ABI of include/hadoofus_crc32c.h and
the drop-in symbols of include/crc32c.h.  It is built in-tree so the .so
travels with the repository snapshot to the GPU box.

A second library, libhadoofus_crc32c_diag.so, is the same sources compiled
with -DHDFS_CRC32C_DIAG: tuning shapes, read probes, the load-only twin and
result-dropping store policies (include/hadoofus_crc32c_diag.h).  Only
tools/ experiments and bench.py's ceiling measurement load it; the product
library contains none of that code and reads no tuning knob from the
environment.

Six companion libraries link against the release library and are built
after it: libhadoofus_md5crc.so (include/hadoofus_md5crc.h),
libhadoofus_writev.so (include/hadoofus_writev.h), libhadoofus_wire.so
(include/hadoofus_wire.h), libhadoofus_wire_batch.so
(include/hadoofus_wire_batch.h), libhadoofus_wirev.so
(include/hadoofus_wirev.h) and libhadoofus_wire_fused.so
(include/hadoofus_wire_fused.h), each with its own sources and export map.
All six share the host support of companion_support.h (last error, the
engine's device, grow-only buffers, scratch bound to a device, pointer
placement, the end of a call); the wire libraries also share the framing and
layout code of wire_frame.h and wire_layout.h, and the gather libraries
(writev, wirev) the gather layout of writev_layout.h and the kernel of
writev_kernels.hip.  The fused wire library uses the layout code of
wire_layout.h with a kernel and CRC tables of its own (wire_fused_crc.h,
wire_fused_tables.h).  These files are compiled into every library that uses
them, each keeping its own copy; no companion links another.

A seventh companion, libhadoofus_wire_fused_batch.so
(include/hadoofus_wire_fused_batch.h), is built the same way from its own
sources and export map: the fused kernel's round (wire_fused_round.h, compiled
into it and into the fused wire library) over the packets of a batch of
writes, with the lookup of wire_fused_batch_lookup.h.

An eighth companion, libhadoofus_wirev_fused.so
(include/hadoofus_wirev_fused.h), is built the same way from its own sources
and export map: the same round over the packets of a write held in device
fragments, found through a fragment table with the lookup of
wirev_fused_lookup.h.  It compiles neither the gather layout nor the gather
kernel of the gather libraries.

A ninth companion, libhadoofus_wirev_fused_batch.so
(include/hadoofus_wirev_fused_batch.h), is built the same way from its own
sources and export map: the same round over the packets of a batch of writes
held in device fragments, with both lookups and what connects them
(wirev_fused_batch_lookup.h), the seamed round of wirev_fused_internal.h and
the batch front end of wire_batch_layout.h.  It compiles neither the gather
layout nor the gather kernel of the gather libraries either.

The read side has a table of its own, READ_LIBRARIES, with rows of the same
shape: libhadoofus_read_batch.so (include/hadoofus_read_batch.h) is built with
the companions, the same way, from its own sources and export map.  It runs the
fused round the other way (wire_fused_round.h) over the packets of a batch of
block reads, found with the lookup of wire_fused_batch_lookup.h from the probe
arithmetic of read_batch_layout.h, and hands what it does not take to the
release library's hdfs_crc32c_read_packets.  Its bindings are the package
hadoofus_read beside this one.

Positional reads have a third table, PREAD_LIBRARIES, again with rows of that
shape: libhadoofus_pread_batch.so (include/hadoofus_pread_batch.h) is built
with the others, the same way, from its own sources and export map.  It runs
the read batch's round with a windowed store over the packets a batch of
client reads takes, from the window arithmetic of pread_batch_layout.h (which
builds on read_batch_layout.h), shares the round's comparisons with the read
batch library (read_batch_verify.h, compiled into both) and hands what it does
not take to hdfs_crc32c_read_packets with the entry's window.  Its bindings
are hadoofus_read/pread_batch.py.

Scatter reads have a fourth table, PREADV_LIBRARIES, rows of that shape again:
libhadoofus_preadv_batch.so (include/hadoofus_preadv_batch.h) is built with the
others, the same way, from its own sources and export map.  It runs the pread
batch's round with a scatter store over a list of device fragments per read:
the window arithmetic of pread_batch_layout.h, the comparisons of
read_batch_verify.h and read_batch_header.h, both lookups
(wire_fused_batch_lookup.h, wirev_fused_lookup.h) and the piece walk of
preadv_batch_lookup.h, and hands what it does not take to
hdfs_crc32c_read_packets with the entry's window and fragment list.  Its
bindings are hadoofus_read/preadv_batch.py.  No source of the pread batch
library changes for it.

Checksums taken from packet streams have a fifth table, DIGEST_LIBRARIES, rows
of that shape once more: libhadoofus_md5crc_streams.so
(include/hadoofus_md5crc_streams.h) is built with the others, the same way,
from its own sources and export map.  It digests the chunk CRCs where the fused
write libraries and the read batch libraries leave them, inside the wire
streams: the read batch's probe arithmetic (read_batch_layout.h) and header
comparison (read_batch_header.h, read_batch_verify.h), the MD5 rounds of
md5_core.h and the cursor of md5crc_streams_lookup.h over the packets' CRC
regions, and hands what is not of the regular shape to
hdfs_crc32c_parse_packets.  It links neither the MD5CRC library nor any other
companion.  Its bindings are hadoofus_read/md5crc_streams.py.

Composite CRCs taken from packet streams have a sixth table, CRC_LIBRARIES, rows
of that shape: libhadoofus_crc_streams.so (include/hadoofus_crc_streams.h) is
built with the others, the same way, from its own sources and export map.  It
folds the chunk CRCs where they lie inside the wire streams into block CRCs
(HDFS's COMPOSITE_CRC mode): the read batch's probe arithmetic
(read_batch_layout.h) and header comparison (read_batch_header.h,
read_batch_verify.h), the GF(2) arithmetic of crc_streams_lookup.h with
multipliers made by crc32c_tables.h's operator, and hands what is not of the
regular shape to hdfs_crc32c_parse_packets.  It links no other companion.  Its
bindings are hadoofus_read/crc_streams.py.

Reads re-framed as writes have a seventh table, RELAY_LIBRARIES, rows of that
shape: libhadoofus_relay_batch.so (include/hadoofus_relay_batch.h) is built
with the others, the same way, from its own sources and export map.  It runs
the fused round once for both sides (wire_fused_round.h): the registers are
loaded from a read's packet stream at the places relay_batch_lookup.h gives,
verified with the read batch's comparisons (read_batch_verify.h,
read_batch_header.h) from its probe arithmetic (read_batch_layout.h), and
stored as the packets of a write, found with wire_fused_batch_lookup.h.  What
it does not take it hands to hdfs_crc32c_read_packets and then to the fused
batch write library's kernel, wire_fused_batch_kernels.hip, compiled into it as
it stands (as the gather-wire library compiles writev_kernels.hip).  It links
no other companion.  Its bindings are hadoofus_read/relay_batch.py.

The six read-side libraries share the host skeleton of a probed batch call,
read_batch_host.h (the run, the entries' outcomes, the main library's read and
walk with unlimited record room, the scratch), compiled into each.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libhadoofus_crc32c.so")
DIAG_LIB = os.path.join(LIBDIR, "libhadoofus_crc32c_diag.so")
SOURCES = ["crc32c_kernels.hip", "crc32c_engine.cpp", "crc32c_packets.cpp"]
DIAG_SOURCES = SOURCES + ["crc32c_probes.hip"]
HEADERS = ["crc32c_internal.h", "crc32c_tables.h", "crc32c_packets.h", "crc32c_engine.h", "crc32c_frame.h",
           "crc32c_hostpin.h", "crc32c_diag_ep.h", "crc32c_deal.h", "crc32c_outpkt.h", "exports.map"]
PUBLIC = ["hadoofus_crc32c.h", "crc32c.h", "hadoofus_crc32c_diag.h"]


def companion_lib(stem):
    """The companion library of that stem: libhadoofus_<stem>.so beside the release library."""
    return os.path.join(LIBDIR, f"libhadoofus_{stem}.so")


MD5CRC_LIB = companion_lib("md5crc")
MD5CRC_SOURCES = ["md5crc_kernels.hip", "md5crc.cpp"]
MD5CRC_HEADERS = ["md5_core.h", "md5crc_internal.h", "companion_support.h", "md5crc_exports.map"]
MD5CRC_PUBLIC = ["hadoofus_md5crc.h", "hadoofus_crc32c.h"]
WRITEV_LIB = companion_lib("writev")
WRITEV_SOURCES = ["writev_kernels.hip", "writev.cpp"]
WRITEV_HEADERS = ["writev_internal.h", "writev_layout.h", "crc32c_outpkt.h", "crc32c_tables.h",
                  "companion_support.h", "writev_exports.map"]
WRITEV_PUBLIC = ["hadoofus_writev.h", "hadoofus_crc32c.h"]
WIRE_LIB = companion_lib("wire")
WIRE_SOURCES = ["wire_kernels.hip", "wire.cpp"]
WIRE_HEADERS = ["wire_internal.h", "wire_frame.h", "wire_layout.h", "companion_support.h", "crc32c_outpkt.h",
                "wire_exports.map"]
WIRE_PUBLIC = ["hadoofus_wire.h", "hadoofus_crc32c.h"]
WIRE_BATCH_LIB = companion_lib("wire_batch")
WIRE_BATCH_SOURCES = ["wire_batch_kernels.hip", "wire_batch.cpp"]
WIRE_BATCH_HEADERS = ["wire_batch_internal.h", "wire_internal.h", "wire_frame.h", "wire_layout.h",
                      "wire_batch_layout.h", "companion_support.h", "crc32c_outpkt.h", "wire_batch_exports.map"]
WIRE_BATCH_PUBLIC = ["hadoofus_wire_batch.h", "hadoofus_crc32c.h"]
WIREV_LIB = companion_lib("wirev")
WIREV_SOURCES = ["wirev_kernels.hip", "writev_kernels.hip", "wirev.cpp"]
WIREV_HEADERS = ["wirev_internal.h", "wire_internal.h", "wire_frame.h", "wire_layout.h", "writev_internal.h",
                 "writev_layout.h", "companion_support.h", "crc32c_outpkt.h", "crc32c_tables.h", "wirev_exports.map"]
WIREV_PUBLIC = ["hadoofus_wirev.h", "hadoofus_writev.h", "hadoofus_crc32c.h"]
WIRE_FUSED_LIB = companion_lib("wire_fused")
WIRE_FUSED_SOURCES = ["wire_fused_kernels.hip", "wire_fused.cpp"]
WIRE_FUSED_HEADERS = ["wire_fused_internal.h", "wire_fused_round.h", "wire_fused_crc.h", "wire_fused_tables.h",
                      "wire_fused_host.h", "wire_internal.h", "wire_layout.h", "companion_support.h", "crc32c_outpkt.h", "crc32c_tables.h",
                      "wire_fused_exports.map"]
WIRE_FUSED_PUBLIC = ["hadoofus_wire_fused.h", "hadoofus_crc32c.h"]
WIRE_FUSED_BATCH_LIB = companion_lib("wire_fused_batch")
WIRE_FUSED_BATCH_SOURCES = ["wire_fused_batch_kernels.hip", "wire_fused_batch.cpp"]
WIRE_FUSED_BATCH_HEADERS = ["wire_fused_batch_internal.h", "wire_fused_batch_lookup.h", "wire_fused_round.h",
                            "wire_fused_crc.h", "wire_fused_tables.h", "wire_fused_host.h", "wire_internal.h",
                            "wire_layout.h", "wire_batch_layout.h", "companion_support.h", "crc32c_outpkt.h", "crc32c_tables.h",
                            "wire_fused_batch_exports.map"]
WIRE_FUSED_BATCH_PUBLIC = ["hadoofus_wire_fused_batch.h", "hadoofus_crc32c.h"]
WIREV_FUSED_LIB = companion_lib("wirev_fused")
WIREV_FUSED_SOURCES = ["wirev_fused_kernels.hip", "wirev_fused.cpp"]
WIREV_FUSED_HEADERS = ["wirev_fused_internal.h", "wirev_fused_lookup.h", "wire_fused_round.h", "wire_fused_crc.h",
                       "wire_fused_tables.h", "wire_fused_host.h", "wire_internal.h", "wire_layout.h",
                       "companion_support.h", "crc32c_outpkt.h", "crc32c_tables.h", "wirev_fused_exports.map"]
WIREV_FUSED_PUBLIC = ["hadoofus_wirev_fused.h", "hadoofus_crc32c.h"]
WIREV_FUSED_BATCH_LIB = companion_lib("wirev_fused_batch")
WIREV_FUSED_BATCH_SOURCES = ["wirev_fused_batch_kernels.hip", "wirev_fused_batch.cpp"]
WIREV_FUSED_BATCH_HEADERS = ["wirev_fused_batch_internal.h", "wirev_fused_batch_lookup.h", "wirev_fused_internal.h",
                             "wirev_fused_lookup.h", "wire_fused_batch_lookup.h", "wire_fused_round.h",
                             "wire_fused_crc.h", "wire_fused_tables.h", "wire_fused_host.h", "wire_internal.h",
                             "wire_layout.h", "wire_batch_layout.h", "companion_support.h", "crc32c_outpkt.h",
                             "crc32c_tables.h", "wirev_fused_batch_exports.map"]
WIREV_FUSED_BATCH_PUBLIC = ["hadoofus_wirev_fused_batch.h", "hadoofus_crc32c.h"]
# Every companion, in build order: (stem, sources, headers, public headers).  Its library is
# companion_lib(stem), its export map <stem>_exports.map, its bindings hadoofus_amd/<stem>.py.
COMPANIONS = (
    ("md5crc", MD5CRC_SOURCES, MD5CRC_HEADERS, MD5CRC_PUBLIC),
    ("writev", WRITEV_SOURCES, WRITEV_HEADERS, WRITEV_PUBLIC),
    ("wire", WIRE_SOURCES, WIRE_HEADERS, WIRE_PUBLIC),
    ("wire_batch", WIRE_BATCH_SOURCES, WIRE_BATCH_HEADERS, WIRE_BATCH_PUBLIC),
    ("wirev", WIREV_SOURCES, WIREV_HEADERS, WIREV_PUBLIC),
    ("wire_fused", WIRE_FUSED_SOURCES, WIRE_FUSED_HEADERS, WIRE_FUSED_PUBLIC),
    ("wire_fused_batch", WIRE_FUSED_BATCH_SOURCES, WIRE_FUSED_BATCH_HEADERS, WIRE_FUSED_BATCH_PUBLIC),
    ("wirev_fused", WIREV_FUSED_SOURCES, WIREV_FUSED_HEADERS, WIREV_FUSED_PUBLIC),
    ("wirev_fused_batch", WIREV_FUSED_BATCH_SOURCES, WIREV_FUSED_BATCH_HEADERS, WIREV_FUSED_BATCH_PUBLIC),
)
READ_BATCH_LIB = companion_lib("read_batch")
READ_BATCH_SOURCES = ["read_batch_kernels.hip", "read_batch.cpp"]
READ_BATCH_HEADERS = ["read_batch_internal.h", "read_batch_layout.h", "wire_fused_batch_lookup.h", "wire_fused_round.h",
                      "wire_fused_crc.h", "wire_fused_tables.h", "wire_fused_host.h", "wire_internal.h",
                      "crc32c_frame.h", "crc32c_outpkt.h", "crc32c_tables.h", "companion_support.h",
                      "read_batch_host.h", "read_batch_verify.h", "read_batch_exports.map"]
READ_BATCH_PUBLIC = ["hadoofus_read_batch.h", "hadoofus_crc32c.h"]
# The read side's libraries, rows as in COMPANIONS; their bindings are hadoofus_read/<stem>.py.
READ_LIBRARIES = (
    ("read_batch", READ_BATCH_SOURCES, READ_BATCH_HEADERS, READ_BATCH_PUBLIC),
)
PREAD_BATCH_LIB = companion_lib("pread_batch")
PREAD_BATCH_SOURCES = ["pread_batch_kernels.hip", "pread_batch.cpp"]
PREAD_BATCH_HEADERS = ["pread_batch_internal.h", "pread_batch_layout.h", "read_batch_layout.h", "read_batch_verify.h",
                       "wire_fused_batch_lookup.h", "wire_fused_round.h", "wire_fused_crc.h", "wire_fused_tables.h",
                       "wire_fused_host.h", "wire_internal.h", "crc32c_frame.h", "crc32c_outpkt.h", "crc32c_tables.h",
                       "companion_support.h", "read_batch_host.h", "pread_batch_exports.map"]
PREAD_BATCH_PUBLIC = ["hadoofus_pread_batch.h", "hadoofus_crc32c.h"]
# The positional-read libraries, rows as in COMPANIONS; their bindings are hadoofus_read/<stem>.py.
PREAD_LIBRARIES = (
    ("pread_batch", PREAD_BATCH_SOURCES, PREAD_BATCH_HEADERS, PREAD_BATCH_PUBLIC),
)
PREADV_BATCH_LIB = companion_lib("preadv_batch")
PREADV_BATCH_SOURCES = ["preadv_batch_kernels.hip", "preadv_batch.cpp"]
PREADV_BATCH_HEADERS = ["preadv_batch_internal.h", "preadv_batch_lookup.h", "read_batch_header.h",
                        "pread_batch_internal.h", "pread_batch_layout.h", "read_batch_layout.h", "read_batch_verify.h",
                        "wirev_fused_internal.h", "wirev_fused_lookup.h", "wire_fused_batch_lookup.h",
                        "wire_fused_round.h", "wire_fused_crc.h", "wire_fused_tables.h", "wire_fused_host.h",
                        "wire_internal.h", "crc32c_frame.h", "crc32c_outpkt.h", "crc32c_tables.h",
                        "companion_support.h", "read_batch_host.h", "preadv_batch_exports.map"]
PREADV_BATCH_PUBLIC = ["hadoofus_preadv_batch.h", "hadoofus_crc32c.h"]
# The scatter-read libraries, rows as in COMPANIONS; their bindings are hadoofus_read/<stem>.py.
PREADV_LIBRARIES = (
    ("preadv_batch", PREADV_BATCH_SOURCES, PREADV_BATCH_HEADERS, PREADV_BATCH_PUBLIC),
)
MD5CRC_STREAMS_LIB = companion_lib("md5crc_streams")
MD5CRC_STREAMS_SOURCES = ["md5crc_streams_kernels.hip", "md5crc_streams.cpp"]
MD5CRC_STREAMS_HEADERS = ["md5crc_streams_internal.h", "md5crc_streams_lookup.h", "md5_core.h", "read_batch_layout.h",
                          "read_batch_header.h", "read_batch_verify.h", "wire_fused_batch_lookup.h",
                          "wire_fused_round.h", "wire_fused_crc.h", "wire_internal.h", "crc32c_frame.h",
                          "crc32c_outpkt.h", "companion_support.h", "read_batch_host.h",
                          "md5crc_streams_exports.map"]
MD5CRC_STREAMS_PUBLIC = ["hadoofus_md5crc_streams.h", "hadoofus_md5crc.h", "hadoofus_crc32c.h"]
# The libraries that digest packet streams, rows as in COMPANIONS; their bindings are hadoofus_read/<stem>.py.
DIGEST_LIBRARIES = (
    ("md5crc_streams", MD5CRC_STREAMS_SOURCES, MD5CRC_STREAMS_HEADERS, MD5CRC_STREAMS_PUBLIC),
)
CRC_STREAMS_LIB = companion_lib("crc_streams")
CRC_STREAMS_SOURCES = ["crc_streams_kernels.hip", "crc_streams.cpp"]
CRC_STREAMS_HEADERS = ["crc_streams_internal.h", "crc_streams_lookup.h", "read_batch_layout.h", "read_batch_header.h",
                       "read_batch_verify.h", "wire_fused_batch_lookup.h", "wire_fused_round.h", "wire_fused_crc.h",
                       "wire_internal.h", "crc32c_frame.h", "crc32c_outpkt.h", "crc32c_tables.h",
                       "companion_support.h", "read_batch_host.h", "crc_streams_exports.map"]
CRC_STREAMS_PUBLIC = ["hadoofus_crc_streams.h", "hadoofus_crc32c.h"]
# The libraries that combine the CRCs of packet streams, rows as in COMPANIONS; their bindings are
# hadoofus_read/<stem>.py.
CRC_LIBRARIES = (
    ("crc_streams", CRC_STREAMS_SOURCES, CRC_STREAMS_HEADERS, CRC_STREAMS_PUBLIC),
)
RELAY_BATCH_LIB = companion_lib("relay_batch")
RELAY_BATCH_SOURCES = ["relay_batch_kernels.hip", "wire_fused_batch_kernels.hip", "relay_batch.cpp"]
RELAY_BATCH_HEADERS = ["relay_batch_internal.h", "relay_batch_lookup.h", "read_batch_layout.h", "read_batch_header.h",
                       "read_batch_verify.h", "wire_fused_batch_internal.h", "wire_fused_batch_lookup.h",
                       "wire_fused_round.h", "wire_fused_crc.h", "wire_fused_tables.h", "wire_fused_host.h",
                       "wire_internal.h", "wire_layout.h", "crc32c_frame.h", "crc32c_outpkt.h", "crc32c_tables.h",
                       "companion_support.h", "read_batch_host.h", "relay_batch_exports.map"]
RELAY_BATCH_PUBLIC = ["hadoofus_relay_batch.h", "hadoofus_crc32c.h"]
# The libraries that connect the read side to the write side, rows as in COMPANIONS; their bindings are
# hadoofus_read/<stem>.py.
RELAY_LIBRARIES = (
    ("relay_batch", RELAY_BATCH_SOURCES, RELAY_BATCH_HEADERS, RELAY_BATCH_PUBLIC),
)
ARCH = os.environ.get("HADOOFUS_OFFLOAD_ARCH", "gfx950")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(lib, sources, headers=HEADERS, public=PUBLIC, others=()):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = [os.path.join(CSRC, f) for f in sources + headers] + [os.path.join(INCLUDE, f) for f in public]
    return any(os.path.getmtime(d) > t for d in deps + list(others))


def _cmd(out, sources, extra):
    # -amdgpu-atomic-optimizer-strategy=None: the kernels' atomics are
    # already single-lane (ticket counters, pool claims) or pre-reduced per
    # wave; the optimizer's ballot/mbcnt scaffolding around each one cost
    # VALU in the hot loop (verify +0.6-0.9 % in a binary A/B,
    # tools/exp_ab_libs.py, profiles/r01/exp_ab_libs_atomic_optimizer.json).
    return [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared",
            "-mllvm", "-amdgpu-atomic-optimizer-strategy=None",
            "-Wall", "-Wno-unused-function", f"-Wl,--version-script={os.path.join(CSRC, 'exports.map')}",
            f"-I{INCLUDE}", f"-I{CSRC}"] + extra + ["-o", out] + [os.path.join(CSRC, f) for f in sources]


def _companion_cmd(out, sources, exports):
    return [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall",
            "-Wno-unused-function", f"-Wl,--version-script={os.path.join(CSRC, exports)}",
            f"-I{INCLUDE}", f"-I{CSRC}", "-o", out] + [os.path.join(CSRC, f) for f in sources] + [
            f"-L{LIBDIR}", "-lhadoofus_crc32c", "-Wl,-rpath,$ORIGIN"]


def build(force=False, verbose=False, diag=True):
    """Build the release library (and, with diag=True, the diagnostic one,
    in parallel), then the MD5CRC, gather-write, wire-stream, wire-batch,
    gather-wire, fused-wire, fused-wire-batch, fused-gather-wire and
    fused-gather-wire-batch companions, the read side's libraries, the
    positional-read libraries, the scatter-read libraries, the libraries
    that digest packet streams, the libraries that combine their CRCs and the
    libraries that relay a read into a write (in parallel).
    Returns the release library's path."""
    os.makedirs(LIBDIR, exist_ok=True)
    jobs = []
    if force or _stale(LIB, SOURCES):
        jobs.append((LIB, _cmd(LIB + ".tmp", SOURCES, [])))
    if diag and (force or _stale(DIAG_LIB, DIAG_SOURCES)):
        jobs.append((DIAG_LIB, _cmd(DIAG_LIB + ".tmp", DIAG_SOURCES, ["-DHDFS_CRC32C_DIAG"])))
    procs = []
    for out, cmd in jobs:
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((out, cmd, subprocess.Popen(cmd)))
    for out, cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
        os.replace(out + ".tmp", out)
    # the companions link against the release library, so after it is in place
    procs = []
    for stem, sources, headers, public in COMPANIONS + READ_LIBRARIES + PREAD_LIBRARIES + PREADV_LIBRARIES + DIGEST_LIBRARIES + \
            CRC_LIBRARIES + RELAY_LIBRARIES:
        out = companion_lib(stem)
        if force or _stale(out, sources, headers, public, [LIB]):
            cmd = _companion_cmd(out + ".tmp", sources, f"{stem}_exports.map")
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((out, cmd, subprocess.Popen(cmd)))
    for out, cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
        os.replace(out + ".tmp", out)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
