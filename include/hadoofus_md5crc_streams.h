/*
 * hadoofus_md5crc_streams.h -- MD5CRC block digests and the MD5MD5CRC file
 * checksum taken from packet streams in device memory
 * (libhadoofus_md5crc_streams.so, a companion of libhadoofus_crc32c.so built
 * from hadoofus_amd/csrc/md5crc_streams*).
 *
 * libhadoofus_md5crc.so (hadoofus_md5crc.h) digests the chunk CRCs a compute
 * plan left in a device array.  The fused write libraries
 * (hdfs_wire_fused_batch_compose and its kin) and the read batch libraries
 * (hdfs_read_batch_read_blocks and its kin) have no compute plan and no CRC
 * array: their chunk CRCs exist only inside the wire streams, between the
 * packets' headers and data.  They lie there in exactly the byte order MD5CRC
 * is defined over -- big-endian, chunk order -- so this library digests them
 * where they lie: a caller who has just written or read a file's blocks gets
 * the checksum to compare with the namenode's getFileChecksum (what distcp
 * does after every copy) without a second pass over the data and without a
 * CRC array.  Of a stream it reads the headers and the CRC bytes, 1/128 of it
 * at 512 bytes per CRC.
 *
 * THE CRCS ARE NOT VERIFIED HERE.  No data byte is read, so a CRC that does
 * not belong to its chunk is digested as it stands.  Verification is the read
 * batch's (hdfs_read_batch_read_blocks compares every CRC with its chunk) or
 * not needed (the fused write computed the CRCs from the data it framed).
 * The digest is the block's MD5CRC when the stream carries the whole block:
 * offset_in_block == 0, whole chunks of chunk_size bytes up to the block's
 * last one, nothing missing at the end (rc == 0 and consumed == len, or a
 * payload the caller knows).  The caller sees all of that in the entry's out
 * fields; hdfs_md5crc_streams_file_checksum insists on offset_in_block == 0.
 *
 * A datanode's stream is predictable from its first packet (K packets of one
 * size, at most one shorter one, at most one empty last one).  A probe launch
 * frames only packet 0 and the tail of every stream; a second launch compares
 * every packet's header with the one the prediction composes; a third digests
 * the CRC regions at the predicted places, one MD5 chain per lane.  An entry
 * whose stream is not of that shape, or whose headers are not the predicted
 * ones, is handed inside the call to hdfs_crc32c_parse_packets, its CRC
 * regions are gathered as that walk framed them and digested by the same
 * kernel (path = HDFS_MD5CRC_STREAMS_PATH_FALLBACK).  No entry's result
 * depends on which path it took.
 *
 * It holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.  It links no other
 * companion library; hadoofus_md5crc.h is included for
 * hdfs_md5crc_file_checksum alone.
 *
 * WHEN IT PAYS.  In memory always -- no 4 B per chunk of CRC array (1 GiB for
 * 1 024 blocks of 128 MiB) and no payload needed any more -- in time only for
 * many small blocks, or where the payloads are no longer at hand.  One MI355X
 * (tools/md5crc_streams_bench.py; v2, CRC32C, every
 * block its own payload and its own stream at an odd address; medians of 5
 * (min-max) with the paths alternated in one process after a warm-up of each,
 * host clock around each whole path, which ends in its synchronise; digests of
 * the three paths compared), milliseconds per call:
 *     blocks x size              this call           plan + block_digests   block_digests alone   launches alone
 *        1 x 128 MiB             19.0 (16.1-20.9)    13.2 (10.9-14.9)       13.8 (10.8-14.8)      18.5
 *       64 x 128 MiB             28.2 (27.9-28.4)    12.6 (12.5-12.8)       10.9 (10.9-10.9)      28.1
 *      256 x 128 MiB             31.5 (31.1-31.6)    17.9 (17.8-18.0)       10.9 (10.9-10.9)      31.2
 *      896 x 128 MiB             32.1 (32.1-32.4)    32.0 (31.8-32.1)       11.5 (11.5-11.5)      32.2
 *      256 x 128 MiB, 5 KiB pkts 115.4 (115.0-115.9) 18.0 (17.8-18.0)       10.9 (10.9-10.9)      115.3
 *     1024 x   1 MiB             0.33 (0.33-0.35)    0.51 (0.49-0.52)       0.46 (0.46-0.48)      0.26
 * "plan + block_digests" is what a caller does without this library: a compute
 * plan over the payloads (created beforehand, executed in the measurement) and
 * hdfs_md5crc_block_digests over the CRC arrays it leaves; "block_digests
 * alone" the same digests over CRC arrays packed beforehand, a floor: the MD5
 * chains without any gather.  896 blocks are what the device's memory held of
 * payloads and streams together.  Row by row: this call is SLOWER than the
 * compute plan plus hdfs_md5crc_block_digests for 1, 64 and 256 blocks of 128
 * MiB (1.4, 2.2 and 1.8 times), level with it at 896 blocks (the ranges
 * overlap: the plan's second pass over 112 GiB costs what the gather costs),
 * and 1.5 times faster for 1 024 blocks of 1 MiB, where it is below the floor
 * too (one call's fixed costs instead of two).  It is nowhere near the floor
 * for large blocks: one chain's trip costs 1.1 us (one block) to 1.9 us (a full
 * wave) here against 0.7 us over a packed array -- the lanes of a wave read 64
 * unrelated streams 512 B at a time, and one trip's prefetch does not hide
 * that.  Streams of 5 120-byte packets, where every MD5 block begins in one
 * packet and ends in another and is taken word by word, are 3.7 times slower
 * again.  One block is better sent to the host in every case (hadoofus_md5crc.h:
 * 1.1 ms for copy and MD5 of 1 MiB of CRCs; not measured for CRCs picked out of
 * a stream).  So: with the payloads at hand and room for the CRC arrays, the
 * compute plan is the faster way up to several hundred large blocks; this call
 * is for when they are not, and for files of many small blocks.  Not measured:
 * CRC32, v1, a caller's stream, entries that fall back, a second run of the
 * command.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_md5crc_streams_last_error()).
 */
#ifndef HADOOFUS_MD5CRC_STREAMS_H
#define HADOOFUS_MD5CRC_STREAMS_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"
#include "hadoofus_md5crc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_MD5CRC_STREAMS_<n>
 * (hadoofus_amd/csrc/md5crc_streams_exports.map); run-time bindings compare
 * hdfs_md5crc_streams_abi_version() with the version they were written for.
 * The main library's ABI version and the other companions' are not affected. */
#define HDFS_MD5CRC_STREAMS_ABI_VERSION 1

/* Most entries in one call. */
#define HDFS_MD5CRC_STREAMS_MAX_ENTRIES 1024

#define HDFS_MD5CRC_STREAMS_PATH_KERNEL   0   /* framed by the probe, digested where the CRCs lie */
#define HDFS_MD5CRC_STREAMS_PATH_FALLBACK 1   /* framed by hdfs_crc32c_parse_packets inside the call */

int hdfs_md5crc_streams_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_md5crc_streams_last_error(void);

/* One block's packet stream, and what the call reports back about it. */
typedef struct hdfs_md5crc_streams_entry {
	const void *stream;          /* in: packet stream, device memory, any byte alignment */
	uint64_t    len;             /* in: its bytes */
	/* out */
	uint64_t    consumed;        /* bytes of complete, framing-clean packets */
	uint64_t    payload;         /* their data bytes */
	uint64_t    nchunks;         /* CRCs digested */
	uint64_t    npkts;           /* packets walked */
	int64_t     offset_in_block; /* packet 0's header field (0 when there is no packet) */
	int32_t     rc;              /* this entry's hdfs_crc32c_parse_packets result */
	int32_t     path;            /* HDFS_MD5CRC_STREAMS_PATH_* */
	uint8_t     md5[16];         /* MD5 over the nchunks CRCs, 4 wire bytes each, packet order */
} hdfs_md5crc_streams_entry;

/* Digests the CRCs of the n streams e[0..n).  For every entry b: rc, consumed
 * and npkts are those of hdfs_crc32c_parse_packets(stream, len, proto,
 * chunk_size, ctype, ...) of that stream alone with unlimited record room;
 * payload is the sum of the framing-clean records' data_len and nchunks the
 * sum of their crc_len / 4.  When rc == 0, md5 is the MD5 of the
 * concatenation, in packet order, of the bytes [stream_off + header_len, +
 * crc_len) of every recorded packet: the empty last packet contributes
 * nothing, an incomplete last packet ends the walk ahead of it.  A stream
 * without a complete packet, or len == 0 (stream may then be NULL), gives rc 0,
 * nchunks 0 and the MD5 of the empty message (d41d8cd9...427e), as
 * hdfs_md5crc_block_digests does for len == 0.  When rc != 0 (a framing
 * error) md5 is 16 zero bytes and nchunks is 0; consumed, npkts and payload
 * stay the walk's.  The call returns the first negative entry rc, else the
 * first nonzero one, else 0.  proto, chunk_size and ctype hold for the whole
 * batch.
 *
 * Only [stream, stream + consumed) is read, and of it no data byte.  Nothing
 * is written to device memory the caller owns.
 *
 * Every stream is device memory of the engine's device at any byte alignment,
 * inside one device allocation; an entry with len == 0 names no range.  Each of
 * these is HDFS_CRC32C_EINVAL for the whole call, decided before any device
 * work, with every entry's out fields zero and the text naming the offending
 * entry's index ("entry <k>"; the batch's own arguments count as entry 0's):
 * n == 0, e == NULL, more than HDFS_MD5CRC_STREAMS_MAX_ENTRIES entries, a host
 * pointer, a range that leaves its allocation, chunk_size == 0, a proto that is
 * none, a ctype that is not CRC32 or CRC32C (HDFS_CRC32C_CSUM_NULL has no CRCs
 * to digest).  Streams may overlap each other or be identical.
 *
 * ORDERING.  The work (one table upload, the probe, the header check and the
 * digest launch, one copy of the tables back) is enqueued on `stream`, a
 * hipStream_t of the engine's device; NULL is a stream of this library that
 * waits for the NULL stream (a blocking stream): bytes written by other
 * non-blocking streams must then be complete before the call.  With a stream
 * of the caller's, the streams' bytes must be ordered ahead of the call on
 * that stream: hdfs_read_batch_read_blocks or hdfs_wire_fused_batch_compose
 * followed at once by this call with the same stream needs no
 * synchronisation in between.  The call returns after the stream has been
 * synchronised.  Entries handed to hdfs_crc32c_parse_packets are framed after
 * that synchronise, one by one, under that call's own rules; their gather and
 * digest launches run on `stream` again and are synchronised before return.
 * Calls from several threads are serialised inside the library by one mutex
 * (one device table and one pinned staging area, the fallback's scratch,
 * grown on demand and kept). */
int hdfs_md5crc_streams_block_digests(hdfs_md5crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size,
    int ctype, void *stream);

/* hdfs_md5crc_streams_block_digests, then the file's MD5MD5CRC checksum on the
 * host: e[0..n) are the file's blocks in order, *out gets bytes_per_crc =
 * chunk_size, ctype, crc_per_block = e[0].nchunks when n > 1, else 0
 * (hadoofus_md5crc.h's rule) and the MD5 over the n block digests.  Returns
 * what the block digests return when that is negative; else
 * HDFS_CRC32C_EINVAL, with the entries' out fields filled and the text naming
 * the entry, when out is NULL or any entry has rc != 0 or offset_in_block !=
 * 0 (its stream does not start at the block's start); else 0. */
int hdfs_md5crc_streams_file_checksum(hdfs_md5crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size,
    int ctype, void *stream, hdfs_md5crc_file_checksum *out);

/* Measurement (tools/md5crc_streams_bench.py): hdfs_md5crc_streams_block_digests
 * once on the library's stream, then the three launches alone iters more times
 * between two HIP events; *ms_per_iter is their distance over iters.  flags:
 * none is defined (HDFS_MD5CRC_STREAMS_TIME_NONE); any flag bit, iters < 1 or
 * a NULL ms_per_iter is HDFS_CRC32C_EINVAL before any device is touched, with
 * nothing written. */
#define HDFS_MD5CRC_STREAMS_TIME_NONE 0u
int hdfs_md5crc_streams_time(hdfs_md5crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
    unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_MD5CRC_STREAMS_H */
