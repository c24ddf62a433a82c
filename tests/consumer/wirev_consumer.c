/*
 * C consumer of the gather-wire companion library (include/hadoofus_wirev.h),
 * written the way hdfs_datanode_writev would use it with a device-resident
 * stream as the goal: a write held in four fragments at odd
 * addresses of a device allocation, one of them empty, given in descending
 * address order, is composed into one wire stream at another odd address, and
 * the stream is handed, still in device memory, to hdfs_crc32c_verify_packets.
 * As a check the same stream is assembled on the host from
 * hdfs_crc32c_compose_packets' header buffers of the fragments' concatenation
 * and its bytes: the two must be identical, records included (hdr_off apart,
 * which counts in the stream).
 * Prints the layout, the packet count and "0 failures" on success.
 * Test infrastructure (tests/test_wirev_cpu.py links it on CPU,
 * tests/test_gpu_wirev.py runs it on the GPU).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_wirev.h"

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; wirev: %s)\n", what, hdfs_crc32c_last_error(), hdfs_wirev_last_error());
		failures++;
	}
}

#define NFRAG 4

int main(void)
{
	const uint64_t lens[NFRAG] = { 65536 + 4000 + 77, 0, 3, 2 * 65536 - 3 };
	const uint64_t at[NFRAG] = { 300001, 0, 150007, 5 };  /* descending addresses, all odd */
	const uint64_t arena_bytes = 1 << 20;
	const int64_t block_off = 4321, seqno = 17;
	const int V2 = HDFS_CRC32C_PROTO_V2, C = HDFS_CRC32C_CSUM_CRC32C;
	void *arena = NULL;
	size_t n = 0, n_c = 0, n_v = 0;
	uint64_t len = 0, wire_len = 0, used = 0, consumed = 0;
	hdfs_wirev_layout_info li;
	hdfs_crc32c_iovec iov[NFRAG];

	check(hdfs_wirev_abi_version() == HDFS_WIREV_ABI_VERSION, "abi version");
	check(hdfs_wirev_layout(lens, NFRAG, block_off, V2, C, 1, &li) == 0 && li.packet_stride == 66079 &&
	    li.header_bytes == 31 && li.head_bytes == 287 && li.nfrags == 3 && li.max_frags_per_packet == 3 &&
	    li.nsegments == 2 && li.seg_chunks + li.ngathered == li.nchunks, "layout");
	printf("layout: %llu packets, %llu chunks (%llu gathered), %llu stream bytes\n", (unsigned long long)li.npkts,
	    (unsigned long long)li.nchunks, (unsigned long long)li.ngathered, (unsigned long long)li.wire_len);
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0, "dev_alloc");
	check(hdfs_crc32c_fill_splitmix64(arena, arena_bytes / 8, 11, 0, NULL) == 0, "fill");
	for (int i = 0; i < NFRAG; i++) {
		iov[i].base = lens[i] ? (uint8_t *)arena + at[i] : NULL;
		iov[i].len = lens[i];
		len += lens[i];
	}
	uint8_t *wire = (uint8_t *)arena + 512 * 1024 + 5;

	/* size query (no device work), then the call */
	check(hdfs_wirev_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, NULL, 0, NULL, 0, &n, &wire_len,
	    NULL) == 0 && n == li.npkts && wire_len == li.wire_len, "size query");
	hdfs_crc32c_out_packet *pk = calloc(n, sizeof(*pk)), *pk_c = calloc(n, sizeof(*pk_c));
	check(hdfs_wirev_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, wire, wire_len, pk, n, &n, &wire_len,
	    NULL) == 0, "wirev compose");

	/* the same stream from the main library's header buffers of the concatenation, on the host */
	uint8_t *hdr = malloc(wire_len), *want = malloc(wire_len), *got = malloc(wire_len), *host = malloc(len);
	uint64_t pos = 0;
	for (int i = 0; i < NFRAG; i++) {
		if (lens[i])
			check(hdfs_crc32c_memcpy(host + pos, iov[i].base, lens[i], 1) == 0, "d2h of a fragment");
		pos += lens[i];
	}
	check(hdfs_crc32c_compose_packets(host, len, block_off, seqno, V2, C, 1, hdr, wire_len, pk_c, n, &n_c,
	    &used) == 0 && n_c == n && used + len == wire_len, "compose_packets of the concatenation");
	check(hdfs_crc32c_memcpy(got, wire, wire_len, 1) == 0, "d2h of the stream");
	uint64_t w = 0;
	for (size_t i = 0; i < n_c && i < n; i++) {
		check(pk[i].hdr_off == w, "hdr_off counts in the stream");
		memcpy(want + w, hdr + pk_c[i].hdr_off, pk_c[i].hdr_len);
		w += pk_c[i].hdr_len;
		memcpy(want + w, host + pk_c[i].data_off, (size_t)pk_c[i].data_len);
		w += (uint64_t)pk_c[i].data_len;
		pk_c[i].hdr_off = pk[i].hdr_off;
	}
	check(w == wire_len && memcmp(got, want, wire_len) == 0, "stream identical");
	check(memcmp(pk, pk_c, n * sizeof(*pk)) == 0, "packet records identical");
	printf("%zu packets, %llu stream bytes\n", n, (unsigned long long)wire_len);

	/* the next hop: the stream verified where it lies */
	hdfs_crc32c_packet *vp = calloc(n, sizeof(*vp));
	check(hdfs_crc32c_verify_packets(wire, wire_len, V2, 512, C, vp, n, &n_v, &consumed) == 0 && n_v == n &&
	    consumed == wire_len, "verify_packets on the device stream");

	/* refused: a host destination, a host fragment, a stream over a fragment, one byte of room too few */
	check(hdfs_wirev_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, got, wire_len, pk, n, &n, &wire_len,
	    NULL) == HDFS_CRC32C_EINVAL, "host wire refused");
	iov[2].base = host;
	check(hdfs_wirev_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, wire, wire_len, pk, n, &n, &wire_len,
	    NULL) == HDFS_CRC32C_EINVAL && strstr(hdfs_wirev_last_error(), "fragment 2"), "host fragment refused");
	iov[2].base = (uint8_t *)arena + at[2];
	check(hdfs_wirev_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, (uint8_t *)iov[0].base + lens[0] - 1,
	    wire_len, pk, n, &n, &wire_len, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wirev_last_error(), "fragment 0"), "overlap refused");
	check(hdfs_wirev_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, wire, wire_len - 1, pk, n, &n,
	    &wire_len, NULL) == HDFS_CRC32C_EINVAL, "short wire refused");

	free(vp);
	free(hdr);
	free(want);
	free(got);
	free(host);
	free(pk);
	free(pk_c);
	hdfs_crc32c_dev_free(arena);
	printf("%d failures\n", failures);
	return failures != 0;
}
