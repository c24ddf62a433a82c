/*
 * hadoofus_writev.h -- gather writes: the outgoing packets of a write held in
 * a list of buffers (libhadoofus_writev.so, a companion of
 * libhadoofus_crc32c.so built from hadoofus_amd/csrc/writev*).
 *
 * The reference's write entry points take an iovec array
 * (hdfs_datanode_writev / hdfs_datanode_writev_nb, include/lowlevel.h:627,
 * 853); the CRC loop of _compose_data_packet_header (src/datanode.c:2836-2859)
 * chains every 512-B chunk's CRC across fragment boundaries.
 * hdfs_crc32c_compose_packets of the main library takes one contiguous
 * buffer.  This library composes the same packets from the fragments where
 * they lie: runs of whole chunks inside one fragment are segments of one
 * compute plan of the main library (read once, in place, at any byte
 * alignment); the chunks that cross a fragment boundary, and the chunks of
 * runs too short for a segment, are assembled piece by piece by this
 * library's own kernel (gather_chunks_kernel).  One device-to-host copy
 * brings the CRCs back; the header buffers are written by the code
 * hdfs_crc32c_compose_packets uses (hadoofus_amd/csrc/crc32c_outpkt.h).
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.
 *
 * WHEN IT PAYS.  The alternative is packing: one hipMemcpyAsync
 * device-to-device per fragment into a contiguous buffer (a second allocation
 * of the write's size), then hdfs_crc32c_compose_packets on it.  Measured on
 * one MI355X (tools/writev_bench.py; medians of 5, host
 * clock around each whole call, block offset 4321, fragments at odd addresses,
 * the packed buffer allocated beforehand):
 *     write      fragments             in place      packed (of it: issuing the copies)
 *     128 MiB        1                  0.24 ms       0.32 ms  (0.005)
 *     128 MiB       16 x 8 MiB          0.25 ms       0.37 ms  (0.05)
 *     128 MiB    1 024 x 128 KiB        0.42 ms       3.46 ms  (3.17)
 *     128 MiB   33 555 x 4 000 B        6.92 ms     112.1 ms   (111.5)
 *       1 GiB       64 x 16 MiB         1.07 ms       1.80 ms  (0.21)
 * In place was the faster path at every size measured, 4 000 B fragments
 * included: there is no fragment size below which packing this way wins,
 * because packing costs about 3.3 us of host time per copy issued, which
 * outweighs what the gather kernel loses.  What the table also says: with
 * every chunk gathered (fragments below 4 KiB hold no run of 8 whole chunks)
 * the call runs at 18 GiB/s, one lane per chunk, against 300-940 GiB/s where
 * segments carry the write.  Whether a packing kernel of the caller's own
 * (one launch for all fragments) would beat that was not measured; neither
 * library offers one.  Calls of 128 MiB are dominated by fixed costs
 * (tables, plan, the copy back: about 0.2 ms), not by the time the bytes take.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_writev_last_error()).
 */
#ifndef HADOOFUS_WRITEV_H
#define HADOOFUS_WRITEV_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_WRITEV_<n>
 * (hadoofus_amd/csrc/writev_exports.map); run-time bindings compare
 * hdfs_writev_abi_version() with the version they were written for.  The
 * main library's ABI version is not affected by this one. */
#define HDFS_WRITEV_ABI_VERSION 1

int hdfs_writev_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_writev_last_error(void);

/* hdfs_crc32c_compose_packets for a write held in iovcnt fragments: the packets
 * and header buffers are byte-identical to what hdfs_crc32c_compose_packets
 * returns for the fragments' concatenation.  out_packet.data_off is an offset
 * into that concatenation.  Fragments: all device memory of the engine's
 * device, or all host memory (mixed: EINVAL); any byte alignment, any length,
 * zero-length fragments allowed (base may then be NULL).  Size query, finish,
 * proto, ctype, offset_in_block, seqno: as hdfs_crc32c_compose_packets.
 *
 * Device fragments are read only inside [base, base + len); a fragment that
 * does not lie inside one device allocation is EINVAL.  The work runs on a
 * stream of this library that waits for the NULL stream (a blocking stream):
 * bytes written by other non-blocking streams must be complete before the
 * call.  The call returns after that stream has been synchronised.
 * Host fragments (the reference's own writev; PCIe-bound) are packed window
 * by window, at most 64 MiB each and ending on a packet boundary, into a host
 * buffer handed to hdfs_crc32c_compose_packets; any total length.
 * HDFS_CRC32C_CSUM_NULL, a size query and an empty write do no GPU work.
 * iovcnt == 1 is hdfs_crc32c_compose_packets.  Nothing is written on a
 * failure that the arguments decide (EINVAL).  Calls from several threads are
 * serialised inside the library. */
int hdfs_writev_compose_packets(const hdfs_crc32c_iovec *iov, int iovcnt,
    int64_t offset_in_block, int64_t seqno, int proto, int ctype, int finish,
    void *hdr_out, uint64_t hdr_cap, hdfs_crc32c_out_packet *pkts, size_t max_pkts,
    size_t *npkts, uint64_t *hdr_used);

/* Host only, no GPU: how a write of these fragment lengths at this block
 * offset is split (what the device path will launch).  The short first chunk
 * of an unaligned block offset is off the 512-B grid of the chunks after it,
 * so it is never part of a segment: it is a gathered chunk. */
typedef struct hdfs_writev_layout_info {
	uint64_t total, nchunks;        /* bytes; chunks on the write's chunk grid */
	uint64_t nsegments, seg_chunks; /* in-place segments and the chunks they cover */
	uint64_t ngathered, npieces;    /* chunks assembled from pieces; their pieces */
	uint32_t max_pieces;            /* most pieces in one gathered chunk */
	uint32_t min_seg_chunks;        /* smallest run of whole chunks kept as a segment */
} hdfs_writev_layout_info;
int hdfs_writev_layout(const uint64_t *lens, int iovcnt, int64_t offset_in_block,
    hdfs_writev_layout_info *out);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_WRITEV_H */
