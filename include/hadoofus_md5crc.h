/*
 * hadoofus_md5crc.h -- MD5CRC block and file checksums on the device
 * (libhadoofus_md5crc.so, a companion of libhadoofus_crc32c.so built from
 * hadoofus_amd/csrc/md5*).
 *
 * OP_BLOCK_CHECKSUM has two forms (src/proto/hdfs.proto:483-495).
 * COMPOSITE_CRC is hdfs_crc32c_composite_crcs of the main library.  MD5CRC,
 * the DEFAULT, is "BlockChecksum obtained by taking the MD5 digest of chunk
 * CRCs": MD5 over the block's chunk CRCs as they go on the wire, 4 bytes
 * each, big-endian, in chunk order.  The file checksum made of it,
 * "MD5-of-<crcPerBlock>MD5-of-<bytesPerCrc>CRC32C", is the MD5 over the
 * blocks' digests in block order; OpBlockChecksumResponseProto
 * (src/proto/datatransfer.proto:316-322) carries bytesPerCrc, crcPerBlock,
 * the digest and crcType.
 *
 * This library computes the block digests from the chunk CRCs a compute plan
 * (hdfs_crc32c_plan_execute, HDFS_CRC32C_MODE_COMPUTE) left in device memory:
 * the CRC arrays never leave the device, 16 bytes per block come back.  It
 * holds no second engine: it binds the device the main library is bound to
 * through that library's public API (hdfs_crc32c_init,
 * hdfs_crc32c_bound_device) and shares its HIP runtime.
 *
 * WHEN IT PAYS.  One MD5 chain is serial; the device runs one chain per lane,
 * one block per chain, so a call takes as long as its longest block however
 * many blocks it holds, and a single block is slower than on the host.
 * Measured on one MI355X (tools/md5crc_bench.py; 1 MiB
 * of CRCs per block = a 128 MiB block at 512 B per CRC; host alternative =
 * the same arrays copied to the host and hashed by 16 threads):
 *     blocks    device call    host alternative (copy + MD5)
 *          1      13.1 ms         1.1 ms  (0.04 + 1.1)
 *         64      11.1 ms         6.2 ms  (1.2 + 5.0)
 *        128      11.3 ms        11.7 ms
 *        256      11.4 ms        23.4 ms
 *       1024      12.2 ms        93.9 ms  (18.9 + 75.0)
 * The device call costs 11-13 ms whatever the batch (0.70 us per 64 bytes of
 * CRCs on each chain); the host alternative grows with it.  They meet at
 * about 128 blocks; from 256 blocks on the device path is at least twice as
 * fast, and at 1 024 blocks 7.7 times.  Below about 100 blocks of this size,
 * or for one block, copy the CRCs out and use the host.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_md5crc_last_error()).
 */
#ifndef HADOOFUS_MD5CRC_H
#define HADOOFUS_MD5CRC_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_MD5CRC_<n>
 * (hadoofus_amd/csrc/md5crc_exports.map); run-time bindings compare
 * hdfs_md5crc_abi_version() with the version they were written for.  The
 * main library's ABI version is not affected by this one. */
#define HDFS_MD5CRC_ABI_VERSION 1
#define HDFS_MD5CRC_LEN 16        /* bytes of an MD5 digest */
#define HDFS_MD5CRC_FILE_BYTES 28 /* bytes hdfs_md5crc_file_bytes writes */

int hdfs_md5crc_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_md5crc_last_error(void);

/* MD5CRC block checksum of each segment: MD5 over the segment's nchunks =
 * ceil(len / chunk_size) chunk CRCs as 4 * nchunks wire bytes (each CRC
 * big-endian, chunk order), read from segs[i].crcs in device memory as a
 * compute plan wrote them (wire order if HDFS_CRC32C_SEG_BE, else host order:
 * the kernel swaps).  segs[i].data and .bitmap are not used and the data is
 * not read.  crcs needs 4-byte alignment only; nothing outside
 * [crcs, crcs + nchunks) is read.
 *
 * md5_out: host (pageable or pinned) or device memory, 16 * nseg bytes, any
 * alignment; digest i at md5_out + 16 * i.
 *
 * nseg == 0 is OK and writes nothing.  A segment with len == 0 has no chunks:
 * its digest is the MD5 of the empty message (d41d8cd9...427e) and its crcs
 * may be NULL.  HDFS_CRC32C_EINVAL for HDFS_CRC32C_SEG_RAW, a non-zero
 * crc_init (MD5CRC is defined over finished CRCs started from 0), a
 * chunk_size of 0, more than 2^32 - 1 chunks, or crcs that is NULL,
 * misaligned or not device-accessible when len > 0.  CRC32 and CRC32C
 * segments may mix: the digest does not depend on the polynomial.  A
 * partial-block checksum needs nothing special: run the compute plan over the
 * prefix wanted and pass that length.
 *
 * ORDERING.  The work is enqueued on `stream` (a hipStream_t of the engine's
 * device; NULL = the NULL stream) and the call returns after that stream has
 * been synchronised, the digests in md5_out.
 *   - It IS ordered after everything enqueued earlier on `stream`: a
 *     hdfs_crc32c_plan_execute(plan, stream) followed at once by this call
 *     with the same stream needs no synchronisation in between.
 *   - With stream == NULL it is also ordered after
 *     hdfs_crc32c_plan_execute(plan, NULL): that runs on the engine's own
 *     stream, a blocking stream, which the NULL stream waits for.
 *   - It is NOT ordered after work on any other non-blocking stream
 *     (hdfs_crc32c_stream_create hands out non-blocking streams, and so do
 *     the engine's job, session and reader paths): synchronise such a stream
 *     (hdfs_crc32c_stream_sync) before passing CRCs it wrote, or pass that
 *     stream here.
 * Calls from several threads are serialised inside the library. */
int hdfs_md5crc_block_digests(const hdfs_crc32c_segment *segs, size_t nseg, void *stream, void *md5_out);

/* A file's MD5MD5CRC checksum (the fields of MD5MD5CRC32FileChecksum). */
typedef struct hdfs_md5crc_file_checksum {
	uint32_t bytes_per_crc;   /* chunk_size of the blocks */
	uint32_t ctype;           /* HDFS_CRC32C_CSUM_CRC32 or HDFS_CRC32C_CSUM_CRC32C */
	uint64_t crc_per_block;   /* chunks of block 0 if the file has more than one block, else 0 */
	uint8_t md5[HDFS_MD5CRC_LEN]; /* MD5 over the nblocks * 16 block digests, block order */
} hdfs_md5crc_file_checksum;

/* Host only, no GPU: the file checksum from block digests already in hand
 * (block_md5s: host memory, 16 * nblocks bytes; nblocks == 0 gives the MD5 of
 * the empty message).  EINVAL for a ctype other than CRC32 / CRC32C or a
 * bytes_per_crc over INT32_MAX (the wire field is signed). */
int hdfs_md5crc_file_from_blocks(const void *block_md5s, size_t nblocks, uint32_t bytes_per_crc,
    uint64_t crc_per_block, int ctype, hdfs_md5crc_file_checksum *out);
/* Both steps: blocks[] are the file's blocks in order, nblocks >= 1, all with
 * the same chunk_size and checksum type (else EINVAL); block digests under
 * hdfs_md5crc_block_digests' rules and ordering, then the file checksum with
 * bytes_per_crc = blocks[0].chunk_size and crc_per_block = chunks of
 * blocks[0] when nblocks > 1. */
int hdfs_md5crc_file_checksum_dev(const hdfs_crc32c_segment *blocks, size_t nblocks, void *stream,
    hdfs_md5crc_file_checksum *out);
/* "MD5-of-<crc_per_block>MD5-of-<bytes_per_crc>CRC32C" (or ...CRC32),
 * NUL-terminated; EINVAL when buf is too small (64 bytes always suffice). */
int hdfs_md5crc_algorithm_name(const hdfs_md5crc_file_checksum *c, char *buf, size_t len);
/* The 28 bytes MD5MD5CRC32FileChecksum serialises: bytes_per_crc s32 BE,
 * crc_per_block s64 BE, md5[16]. */
int hdfs_md5crc_file_bytes(const hdfs_md5crc_file_checksum *c, void *out28);
/* Plain MD5 of a host buffer (the round code the kernel runs, compiled for
 * the host); no GPU. */
int hdfs_md5crc_md5_host(const void *buf, uint64_t len, void *out16);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_MD5CRC_H */
