/*
 * hadoofus_wire_fused_batch.h -- the wire streams of a batch of writes in one
 * call, one launch and ONE pass over the data
 * (libhadoofus_wire_fused_batch.so, a companion of libhadoofus_crc32c.so built
 * from hadoofus_amd/csrc/wire_fused_batch*).
 *
 * Two libraries each have half of this.  hdfs_wire_batch_compose
 * (hadoofus_wire_batch.h) pays a call's fixed cost once per batch, but reads
 * every write twice: a compute plan of the main library leaves the chunk CRCs
 * in an array, then a frame kernel reads the write again.
 * hdfs_wire_fused_compose_packets (hadoofus_wire_fused.h) reads every byte
 * once and computes the CRCs from the registers it copies, but takes one write
 * per call, and every workgroup of every call fills 156 KiB of tables before
 * its first load.  This library's kernel, frame_fused_batch_kernel, runs the
 * fused kernel's round over the packets of all writes of a batch: one upload
 * of a table of the writes, one launch, one synchronise, the table image
 * filled once per workgroup, no compute plan and no CRC array.  Each write's
 * stream is byte for byte the one hdfs_wire_fused_compose_packets writes for
 * it, which is hdfs_wire_compose_packets' stream.
 *
 * The interface is hadoofus_wire_batch.h's with another prefix: the same entry
 * struct, the same contract, the same error texts.  It holds no second engine:
 * it binds the device the main library is bound to through that library's
 * public API (hdfs_crc32c_init, hdfs_crc32c_bound_device) and shares its HIP
 * runtime.  It links no other companion library.
 *
 * WHEN IT PAYS.  At every shape measured, against both ways of doing the job
 * without it: a loop of hdfs_wire_fused_compose_packets calls, and
 * hdfs_wire_batch_compose.  One MI355X (tools/wire_fused_batch_bench.py,
 * DESIGN.md section 17; medians of 5 (min-max) per write with the three paths
 * alternated in one process after two warm-ups of each, host clock around each
 * whole path, which ends in its synchronise, CRC32C, v2, finish, distinct
 * sources at odd addresses, every stream of all three paths downloaded and
 * compared), microseconds per write:
 *     writes x size    offset   this call            fused loop          two-pass batch
 *       16 x 128 MiB       0    78.8 (78.2-84.4)     98.6 (97.6-98.9)    89.5 (89.2-90.0)
 *       16 x 128 MiB    4321    77.8 (77.6-78.0)     90.3 (90.0-90.6)    91.2 (90.7-91.7)
 *       64 x 128 MiB       0    83.5 (83.1-84.0)     98.2 (97.8-98.6)    94.5 (94.3-94.9)
 *       64 x 128 MiB    4321    83.0 (82.3-83.5)     90.7 (90.5-91.4)    95.5 (95.1-99.1)
 *       64 x   1 MiB       0    1.09 (1.08-1.23)     25.5 (25.4-25.6)    1.87 (1.83-1.90)
 *       64 x   8 MiB       0    5.70 (5.66-5.83)     27.8 (27.7-28.1)    6.52 (6.46-6.82)
 *     1024 x  64 KiB       0    0.169 (0.164-0.178)  25.0 (24.9-25.0)    0.345 (0.323-0.356)
 *    65536 x 512 B (*)     0    0.095 (0.095-0.097)  19.3 (19.3-19.3)    0.230 (0.227-0.232)
 * (*) one packet per write, no finish.  This call's range is clear of both
 * others in all eight rows, and was in a second run of the same command.  For
 * 128 MiB writes (1.07 to 1.33 times) the second pass over the data is what is
 * saved against the two-pass batch, the per-call launch and synchronise against
 * the loop.  For small writes the loop pays 25 to 28 us per call whatever the
 * size (4.9 to 200 times), and the two-pass batch its compute plan (1.14 to 2.4
 * times), although this library's kernel alone is slower than that library's
 * frame kernel alone (0.64 against 0.37 us per 1 MiB write).  Where it is weak:
 * a workgroup takes one packet a step, so a batch of one-packet writes costs
 * about 2.2 us per packet and workgroup; 65 536 writes of 512 B take the kernel
 * 0.57 ms where the same 32 MiB as one write take the single fused kernel
 * 0.022 ms.  A caller who can present such bytes as one write should.  Not
 * measured: CRC32, v1, CSUM_NULL, a caller's stream, batches of mixed sizes.
 *
 * Status codes are the main library's HDFS_CRC32C_* (0 = OK, negative =
 * failure, text in hdfs_wire_fused_batch_last_error()).
 */
#ifndef HADOOFUS_WIRE_FUSED_BATCH_H
#define HADOOFUS_WIRE_FUSED_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "hadoofus_crc32c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every export carries the version node HADOOFUS_WIRE_FUSED_BATCH_<n>
 * (hadoofus_amd/csrc/wire_fused_batch_exports.map); run-time bindings compare
 * hdfs_wire_fused_batch_abi_version() with the version they were written for.
 * The main library's ABI version and the other companions' are not affected. */
#define HDFS_WIRE_FUSED_BATCH_ABI_VERSION 1

/* Most writes in one call. */
#define HDFS_WIRE_FUSED_BATCH_MAX_WRITES 65536

int hdfs_wire_fused_batch_abi_version(void);
/* Text of the calling thread's last failure in this library. */
const char *hdfs_wire_fused_batch_last_error(void);

/* One write of a batch: hdfs_wire_fused_compose_packets' arguments of it, and
 * what the call reports back about it.  Field for field struct
 * hdfs_wire_batch_write. */
typedef struct hdfs_wire_fused_batch_write {
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
} hdfs_wire_fused_batch_write;

/* The streams of the nwrites writes w[0..nwrites): after a successful call
 * w[k].wire[0, w[k].wire_len) is byte for byte what
 * hdfs_wire_fused_compose_packets writes for (data, len, offset_in_block,
 * seqno, proto, ctype, finish) of entry k, and the records
 * pkts[w[k].first_pkt .. first_pkt + npkts) (pkts may be NULL) equal that
 * call's records, hdr_off counting inside write k's own stream.  The records
 * lie in batch order; *npkts is their total.  proto and ctype hold for the
 * whole batch.  An empty write with finish is one header-only packet; an empty
 * write without it is no packet and no work, and may sit anywhere in the
 * batch.
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
 * has room.  At most HDFS_WIRE_FUSED_BATCH_MAX_WRITES writes, 1 TiB per write
 * and (2^31 - 1) / 4 packets in all.
 *
 * Only the data ranges are read and only the wire ranges [wire, wire +
 * wire_len) are written, every byte of them once.
 *
 * ORDERING.  The work (one table upload, then one kernel) is enqueued on
 * `stream`, a hipStream_t of the engine's device; NULL is a stream of this
 * library that waits for the NULL stream (a blocking stream): bytes written by
 * other non-blocking streams must then be complete before the call.  With a
 * stream of the caller's, the data must be ordered ahead of the call on that
 * stream.  The call returns after the stream has been synchronised: the
 * streams' bytes are then visible to every later operation on the device.
 * Calls from several threads are serialised inside the library by one mutex
 * (the CRC tables, uploaded once per device and kept; one device table and one
 * pinned staging area, grown on demand and kept). */
int hdfs_wire_fused_batch_compose(hdfs_wire_fused_batch_write *w, size_t nwrites, int proto, int ctype,
    hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, void *stream);

/* Host only, no GPU: fills the out fields of every entry (wire and wire_cap
 * are not looked at) and the totals of the batch. */
typedef struct hdfs_wire_fused_batch_totals {
	uint64_t npkts;          /* packets of all writes */
	uint64_t nchunks;        /* chunks of all writes (CRCs computed unless CSUM_NULL) */
	uint64_t wire_bytes;     /* sum of the streams' lengths */
	uint64_t table_entries;  /* writes with at least one packet: entries of the device table */
} hdfs_wire_fused_batch_totals;
int hdfs_wire_fused_batch_layout(hdfs_wire_fused_batch_write *w, size_t nwrites, int proto, int ctype,
    hdfs_wire_fused_batch_totals *out);

/* Measurement (tools/wire_fused_batch_bench.py): hdfs_wire_fused_batch_compose
 * once on the library's stream, then frame_fused_batch_kernel alone iters more
 * times between two HIP events; *ms_per_iter is their distance over iters.
 * flags: HDFS_WIRE_FUSED_BATCH_TIME_GROUPS(n) launches n workgroups (1..1024)
 * instead of the product's grid (one per compute unit, at most one per
 * packet), so that every workgroup walks many packets across the writes; any
 * other flag bit, n above 1024, iters < 1 or a NULL ms_per_iter is
 * HDFS_CRC32C_EINVAL before any device is touched, with nothing written.  The
 * streams written are the same under every flag. */
#define HDFS_WIRE_FUSED_BATCH_TIME_GROUPS(n) ((unsigned)(n) << 8)
int hdfs_wire_fused_batch_time(hdfs_wire_fused_batch_write *w, size_t nwrites, int proto, int ctype,
    unsigned flags, int iters, double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif /* HADOOFUS_WIRE_FUSED_BATCH_H */
