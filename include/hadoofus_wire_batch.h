/*
 * hadoofus_wire_batch.h -- the wire streams of a batch of writes in one call
 * (libhadoofus_wire_batch.so, a companion of libhadoofus_crc32c.so built from
 * hadoofus_amd/csrc/wire_batch*).
 *
 * hdfs_wire_compose_packets (hadoofus_wire.h) turns one write that lives in
 * device memory into one wire stream [plen][hlen][PacketHeaderProto][BE CRCs]
 * [data]... per call, and most of a 128 MiB call is fixed cost: the plan's
 * creation and destruction, two launches, a synchronise.  A client that
 * writes a file, or a node that re-frames replicas, has many blocks in device
 * memory at once.  hdfs_wire_batch_compose pays that fixed cost once per
 * batch, as hdfs_crc32c_verify_blocks_submit does on the read side: one
 * compute plan of the main library over every write's chunk grid, one upload
 * of a table of the writes, one launch of frame_batch_kernel over every packet
 * of every write, one synchronise.  Each write's stream is byte for byte the
 * one hdfs_wire_compose_packets writes for it.
 *
 * It holds no second engine and no CRC arithmetic: it binds the device the
 * main library is bound to through that library's public API
 * (hdfs_crc32c_init, hdfs_crc32c_bound_device), takes its chunk CRCs from a
 * plan of that library and shares its HIP runtime.  The framing code is the
 * single-write library's (hadoofus_amd/csrc/wire_frame.h, wire_layout.h), one
 * definition compiled into both.
 *
 * WHEN IT PAYS.  Against a loop of hdfs_wire_compose_packets calls over the
 * same writes, which is what a caller has without this library.  Measured on
 * one MI355X (tools/wire_batch_bench.py; medians of 5
 * with the two paths alternated in one process after a warm-up of each, host
 * clock around each whole path, 128 MiB writes, CRC32C, v2, finish, distinct
 * sources at odd addresses, every stream of both paths compared), per block,
 * with the min-max spread:
 *     writes   block offset   this call                the loop                 ratio
 *       16          0          93.2 us  (92.0-125.3)   155.7 us (155.4-213.9)   1.67
 *       16       4321          94.5 us  (93.8-111.2)   173.1 us (172.1-177.3)   1.83
 *       64          0          92.0 us  (91.6-101.2)   156.2 us (155.0-158.0)   1.70
 *       64       4321          91.2 us  (90.7-99.3)    171.7 us (171.5-173.5)   1.88
 * Another run of the same command gave ratios of 1.64 to 1.88; the loop won
 * nowhere.  Of a batch's 92 us per block about 54 us are the frame kernel
 * (alone: 52.5-55.7 us per block, 4.9-5.2 TB/s of traffic; a batch does not
 * fit the last-level cache as one 128 MiB write does), some 20 us the CRC
 * pass, and 9.5-11 us the host's walk over every packet of every write
 * (hdfs_wire_batch_layout alone), which runs before anything is enqueued.
 * Batches of smaller writes were not measured.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_wire_batch_last_error()).
 */
#ifndef HADOOFUS_WIRE_BATCH_H
#define HADOOFUS_WIRE_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_WIRE_BATCH_<n>
 * (hadoofus_amd/csrc/wire_batch_exports.map); run-time bindings compare
 * hdfs_wire_batch_abi_version() with the version they were written for.  The
 * main library's ABI version and the other companions' are not affected. */
#define HDFS_WIRE_BATCH_ABI_VERSION 1

/* Most writes in one call. */
#define HDFS_WIRE_BATCH_MAX_WRITES 65536

int hdfs_wire_batch_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_wire_batch_last_error(void);

/* One write of a batch: hdfs_wire_compose_packets' arguments of it, and what
 * the call reports back about it. */
typedef struct hdfs_wire_batch_write {
	const void *data;         /* device, len bytes, any alignment */
	uint64_t    len;          /* at most 1 TiB */
	int64_t     offset_in_block;
	int64_t     seqno;        /* of the write's first packet */
	int32_t     finish;       /* != 0: the empty lastPacketInBlock packet ends the write */
	int32_t     reserved;
	void       *wire;         /* device, any alignment; NULL in every entry = size query */
	uint64_t    wire_cap;     /* bytes of room at wire */
	/* out */
	uint64_t    wire_len;     /* bytes of this write's stream */
	uint64_t    npkts;        /* its packets */
	uint64_t    first_pkt;    /* index of its first record in pkts */
} hdfs_wire_batch_write;

/* The streams of the nwrites writes w[0..nwrites): after a successful call
 * w[k].wire[0, w[k].wire_len) is byte for byte what hdfs_wire_compose_packets
 * writes for (data, len, offset_in_block, seqno, proto, ctype, finish) of
 * entry k, and the records pkts[w[k].first_pkt .. first_pkt + npkts) (pkts may
 * be NULL) equal that call's records, hdr_off counting inside write k's own
 * stream.  The records lie in batch order; *npkts is their total.  proto and
 * ctype hold for the whole batch.  An empty write with finish is one
 * header-only packet; an empty write without it is no packet and no work, and
 * may sit anywhere in the batch.
 *
 * Every data and wire range is device memory of the engine's device at any
 * byte alignment, inside one device allocation.  No wire range may overlap
 * another wire range or any data range of the batch; data ranges may overlap
 * each other or be identical (two replicas of one block).  Each of these is
 * HDFS_CRC32C_EINVAL for the whole call with nothing written anywhere, the out
 * fields of every entry and *npkts still set, and the error text naming the
 * offending entry's index ("entry <k>"): a host pointer, a range that leaves
 * its allocation, an overlap, wire_cap < wire_len, (with pkts) max_pkts
 * smaller than *npkts, and some entries with wire == NULL while others have
 * one.  If every wire is NULL the call is a size query that touches no
 * device: the out fields and *npkts are set, and the records too when pkts
 * has room.  At most HDFS_WIRE_BATCH_MAX_WRITES writes, 1 TiB per write,
 * (2^31 - 1) / 4 packets and 2^32 - 16 chunks in all.
 *
 * Only the data ranges are read and only the wire ranges [wire, wire +
 * wire_len) are written, every byte of them once.
 *
 * ORDERING.  The work (one table upload, the plan, then the frame kernel) is
 * enqueued on `stream`, a hipStream_t of the engine's device; NULL is a stream
 * of this library that waits for the NULL stream (a blocking stream): bytes
 * written by other non-blocking streams must then be complete before the call.
 * With a stream of the caller's, the data must be ordered ahead of the call on
 * that stream.  The call returns after the stream has been synchronised: the
 * streams' bytes are then visible to every later operation on the device.
 * Calls from several threads are serialised inside the library (one CRC
 * array, one device table and one pinned staging area, grown on demand and
 * kept). */
int hdfs_wire_batch_compose(hdfs_wire_batch_write *w, size_t nwrites, int proto, int ctype,
    hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, void *stream);

/* Host only, no GPU: fills the out fields of every entry (wire and wire_cap
 * are not looked at) and the totals of the batch. */
typedef struct hdfs_wire_batch_totals {
	uint64_t npkts;          /* packets of all writes */
	uint64_t nchunks;        /* chunks of all writes (CRCs computed unless CSUM_NULL) */
	uint64_t wire_bytes;     /* sum of the streams' lengths */
	uint64_t table_entries;  /* writes with at least one packet: entries of the device table */
} hdfs_wire_batch_totals;
int hdfs_wire_batch_layout(hdfs_wire_batch_write *w, size_t nwrites, int proto, int ctype,
    hdfs_wire_batch_totals *out);

/* Measurement (tools/wire_batch_bench.py): hdfs_wire_batch_compose once on the
 * library's stream, then frame_batch_kernel alone iters more times between two
 * HIP events; *ms_per_iter is their distance over iters.  The streams written
 * are the same. */
int hdfs_wire_batch_frame_time(hdfs_wire_batch_write *w, size_t nwrites, int proto, int ctype, int iters,
    double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_WIRE_BATCH_H */
