/*
 * C consumer of the fused wire-batch companion library
 * (include/hadoofus_wire_fused_batch.h), written the way a node that re-frames
 * replicas would use it: three writes at odd addresses of one device
 * allocation -- one at an unaligned block offset with finish, one empty
 * without finish (no packet), one short -- are composed into three wire
 * streams in one call and one pass, and each stream is handed, still in device
 * memory, to hdfs_crc32c_verify_packets, which checks the CRCs this library
 * computed.  Return codes and lengths are checked against
 * hdfs_wire_fused_batch_layout and the size query; the timing entry with two
 * workgroups writes the same streams.
 * Prints the totals and "0 failures" on success.
 * Test infrastructure (tests/test_wire_fused_batch_cpu.py links it on CPU,
 * tests/test_gpu_wire_fused_batch.py runs it on the GPU).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_wire_fused_batch.h"

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; wire batch: %s)\n", what, hdfs_crc32c_last_error(),
		    hdfs_wire_fused_batch_last_error());
		failures++;
	}
}

#define NW 3

int main(void)
{
	const uint64_t arena_bytes = 2 << 20, lens[NW] = { 3 * 65536 + 4077, 0, 1000 };
	const int64_t offs[NW] = { 4321, 0, 0 };
	const int fin[NW] = { 1, 0, 0 };
	const int V2 = HDFS_CRC32C_PROTO_V2, C = HDFS_CRC32C_CSUM_CRC32C;
	void *arena = NULL;
	size_t n = 0, n_q = 0;
	hdfs_wire_fused_batch_write w[NW], q[NW];
	hdfs_wire_fused_batch_totals tot;

	check(hdfs_wire_fused_batch_abi_version() == HDFS_WIRE_FUSED_BATCH_ABI_VERSION, "abi version");
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0, "dev_alloc");
	check(hdfs_crc32c_fill_splitmix64(arena, arena_bytes / 8, 11, 0, NULL) == 0, "fill");
	memset(w, 0, sizeof(w));
	for (int k = 0; k < NW; k++) {
		w[k].data = (uint8_t *)arena + 3 + k * 300000;
		w[k].len = lens[k];
		w[k].offset_in_block = offs[k];
		w[k].seqno = 100 * k;
		w[k].finish = fin[k];
	}

	/* host only: the layout, then the size query (every wire NULL) */
	memcpy(q, w, sizeof(w));
	check(hdfs_wire_fused_batch_layout(q, NW, V2, C, &tot) == 0 && tot.table_entries == 2 &&
	    tot.npkts == q[0].npkts + q[2].npkts && q[1].npkts == 0 && q[1].wire_len == 0 &&
	    q[2].wire_len == 31 + 8 + 1000 && q[2].first_pkt == q[0].npkts && q[0].npkts == 6, "layout");
	printf("layout: %llu packets, %llu chunks, %llu stream bytes, %llu table entries\n",
	    (unsigned long long)tot.npkts, (unsigned long long)tot.nchunks, (unsigned long long)tot.wire_bytes,
	    (unsigned long long)tot.table_entries);
	check(hdfs_wire_fused_batch_compose(w, NW, V2, C, NULL, 0, &n_q, NULL) == 0 && n_q == tot.npkts, "size query");
	check(w[0].wire_len == q[0].wire_len && w[2].wire_len == q[2].wire_len &&
	    w[0].wire_len + w[2].wire_len == tot.wire_bytes, "size query lengths");

	/* the call */
	hdfs_crc32c_out_packet *pk = calloc(n_q ? n_q : 1, sizeof(*pk));
	uint8_t *at = (uint8_t *)arena + (1 << 20) + 5;
	for (int k = 0; k < NW; k++) {
		w[k].wire = at;
		w[k].wire_cap = w[k].wire_len;
		at += w[k].wire_len + 33;
	}
	check(hdfs_wire_fused_batch_compose(w, NW, V2, C, pk, n_q, &n, NULL) == 0 && n == n_q, "batch compose");
	check(pk[0].data_len == 287 && pk[w[0].npkts - 1].last == 1 && pk[w[2].first_pkt].hdr_off == 0 &&
	    pk[w[2].first_pkt].data_len == 1000 && pk[w[2].first_pkt].seqno == 200, "records");
	printf("%zu packets\n", n);

	/* the next hop: each stream verified where it lies */
	hdfs_crc32c_packet *vp = calloc(n ? n : 1, sizeof(*vp));
	for (int k = 0; k < NW; k += 2) {
		size_t n_v = 0;
		uint64_t consumed = 0;
		check(hdfs_crc32c_verify_packets(w[k].wire, w[k].wire_len, V2, 512, C, vp, n, &n_v, &consumed) == 0 &&
		    n_v == w[k].npkts && consumed == w[k].wire_len, "verify_packets on a device stream");
	}

	/* refused, each naming its entry: one byte of room too few, a stream over another's, a host wire */
	w[2].wire_cap--;
	check(hdfs_wire_fused_batch_compose(w, NW, V2, C, pk, n_q, &n, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wire_fused_batch_last_error(), "entry 2") && n == n_q, "short wire refused");
	w[2].wire_cap++;
	void *keep = w[2].wire;
	w[2].wire = (uint8_t *)w[0].wire + 10;
	check(hdfs_wire_fused_batch_compose(w, NW, V2, C, pk, n_q, &n, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wire_fused_batch_last_error(), "entry 2"), "overlap refused");
	w[2].wire = malloc(w[2].wire_len);
	check(hdfs_wire_fused_batch_compose(w, NW, V2, C, pk, n_q, &n, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wire_fused_batch_last_error(), "entry 2"), "host wire refused");
	free(w[2].wire);
	w[2].wire = keep;
	check(hdfs_wire_fused_batch_compose(w, NW, V2, C, pk, n_q, &n, NULL) == 0, "and again, unspoilt");

	/* the timing entry: two workgroups walk all packets; the streams still verify */
	double ms = 0;
	check(hdfs_wire_fused_batch_time(w, NW, V2, C, HDFS_WIRE_FUSED_BATCH_TIME_GROUPS(2), 2, &ms) == 0 && ms > 0,
	    "timing entry");
	check(hdfs_wire_fused_batch_time(w, NW, V2, C, HDFS_WIRE_FUSED_BATCH_TIME_GROUPS(1025), 2, &ms) ==
	    HDFS_CRC32C_EINVAL, "1025 workgroups refused");
	for (int k = 0; k < NW; k += 2) {
		size_t n_v = 0;
		uint64_t consumed = 0;
		check(hdfs_crc32c_verify_packets(w[k].wire, w[k].wire_len, V2, 512, C, vp, n, &n_v, &consumed) == 0 &&
		    n_v == w[k].npkts && consumed == w[k].wire_len, "verify_packets after the timing entry");
	}

	free(vp);
	free(pk);
	hdfs_crc32c_dev_free(arena);
	printf("%d failures\n", failures);
	return failures != 0;
}
