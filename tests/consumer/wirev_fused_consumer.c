/*
 * C consumer of the fused gather-wire companion library
 * (include/hadoofus_wirev_fused.h), written the way hdfs_datanode_writev
 * would use it with a device-resident stream as the goal: a
 * write held in five fragments at odd addresses of a device allocation, one of
 * them empty and one of three bytes, given in descending address order, is
 * composed into one wire stream at another odd address in one pass, and the
 * stream is handed, still in device memory, to hdfs_crc32c_verify_packets.
 * As a check the same stream is assembled on the host from
 * hdfs_crc32c_compose_packets' header buffers of the fragments' concatenation
 * and its bytes: the two must be identical, records included (hdr_off apart,
 * which counts in the stream).
 * Prints the layout, the packet count and "0 failures" on success.
 * Test infrastructure (tests/test_wirev_fused_cpu.py links it on CPU,
 * tests/test_gpu_wirev_fused.py runs it on the GPU).  C99.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_wirev_fused.h"

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; wirev_fused: %s)\n", what, hdfs_crc32c_last_error(),
		    hdfs_wirev_fused_last_error());
		failures++;
	}
}

#define NFRAG 5

int main(void)
{
	const uint64_t lens[NFRAG] = { 65536 + 4000 + 77, 0, 3, 2 * 65536 - 3 - 200, 200 };
	const uint64_t at[NFRAG] = { 400001, 0, 350007, 150005, 5 };  /* descending addresses, all odd */
	const uint64_t arena_bytes = 1 << 20;
	const int64_t block_off = 4321, seqno = 17;
	const int V2 = HDFS_CRC32C_PROTO_V2, C = HDFS_CRC32C_CSUM_CRC32C;
	void *arena = NULL;
	size_t n = 0, n_c = 0, n_v = 0, i;
	uint64_t len = 0, wire_len = 0, used = 0, consumed = 0, pos = 0, w = 0;
	hdfs_wirev_fused_layout_info li;
	hdfs_crc32c_iovec iov[NFRAG];
	hdfs_crc32c_out_packet *pk, *pk_c;
	hdfs_crc32c_packet *vp;
	uint8_t *wire, *hdr, *want, *got, *host;
	int f;

	check(hdfs_wirev_fused_abi_version() == HDFS_WIREV_FUSED_ABI_VERSION, "abi version");
	check(hdfs_wirev_fused_layout(lens, NFRAG, block_off, V2, C, 1, &li) == 0 && li.packet_stride == 66079 &&
	    li.header_bytes == 31 && li.head_bytes == 287 && li.nfrags == 4 && li.seamed_rounds == 1 &&
	    li.max_frags_per_round == 3 && li.seamed_ragged == 1 && li.rounds > li.seamed_rounds, "layout");
	printf("layout: %llu packets, %llu chunks, %llu rounds (%llu seamed), %llu stream bytes\n",
	    (unsigned long long)li.npkts, (unsigned long long)li.nchunks, (unsigned long long)li.rounds,
	    (unsigned long long)li.seamed_rounds, (unsigned long long)li.wire_len);
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0, "dev_alloc");
	check(hdfs_crc32c_fill_splitmix64(arena, arena_bytes / 8, 11, 0, NULL) == 0, "fill");
	for (f = 0; f < NFRAG; f++) {
		iov[f].base = lens[f] ? (uint8_t *)arena + at[f] : NULL;
		iov[f].len = lens[f];
		len += lens[f];
	}
	wire = (uint8_t *)arena + 640 * 1024 + 5;

	/* size query (no device work), then the call */
	check(hdfs_wirev_fused_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, NULL, 0, NULL, 0, &n, &wire_len,
	    NULL) == 0 && n == li.npkts && wire_len == li.wire_len, "size query");
	pk = calloc(n, sizeof(*pk));
	pk_c = calloc(n, sizeof(*pk_c));
	check(hdfs_wirev_fused_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, wire, wire_len, pk, n, &n,
	    &wire_len, NULL) == 0, "fused wirev compose");

	/* the same stream from the main library's header buffers of the concatenation, on the host */
	hdr = malloc(wire_len);
	want = malloc(wire_len);
	got = malloc(wire_len);
	host = malloc(len);
	for (f = 0; f < NFRAG; f++) {
		if (lens[f])
			check(hdfs_crc32c_memcpy(host + pos, iov[f].base, lens[f], 1) == 0, "d2h of a fragment");
		pos += lens[f];
	}
	check(hdfs_crc32c_compose_packets(host, len, block_off, seqno, V2, C, 1, hdr, wire_len, pk_c, n, &n_c,
	    &used) == 0 && n_c == n && used + len == wire_len, "compose_packets of the concatenation");
	check(hdfs_crc32c_memcpy(got, wire, wire_len, 1) == 0, "d2h of the stream");
	for (i = 0; i < n_c && i < n; i++) {
		check(pk[i].hdr_off == w, "hdr_off counts in the stream");
		memcpy(want + w, hdr + pk_c[i].hdr_off, pk_c[i].hdr_len);
		w += pk_c[i].hdr_len;
		memcpy(want + w, host + pk_c[i].data_off, (size_t)pk_c[i].data_len);
		w += (uint64_t)pk_c[i].data_len;
		pk_c[i].hdr_off = pk[i].hdr_off;
	}
	check(w == wire_len && memcmp(got, want, wire_len) == 0, "stream identical");
	check(memcmp(pk, pk_c, n * sizeof(*pk)) == 0, "packet records identical");
	printf("%lu packets, %llu stream bytes\n", (unsigned long)n, (unsigned long long)wire_len);

	/* the next hop: the stream verified where it lies */
	vp = calloc(n, sizeof(*vp));
	check(hdfs_crc32c_verify_packets(wire, wire_len, V2, 512, C, vp, n, &n_v, &consumed) == 0 && n_v == n &&
	    consumed == wire_len, "verify_packets on the device stream");

	/* refused: a host destination, a host fragment, a stream over a fragment, one byte of room too few */
	check(hdfs_wirev_fused_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, got, wire_len, pk, n, &n,
	    &wire_len, NULL) == HDFS_CRC32C_EINVAL, "host wire refused");
	iov[2].base = host;
	check(hdfs_wirev_fused_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, wire, wire_len, pk, n, &n,
	    &wire_len, NULL) == HDFS_CRC32C_EINVAL && strstr(hdfs_wirev_fused_last_error(), "fragment 2"),
	    "host fragment refused");
	iov[2].base = (uint8_t *)arena + at[2];
	check(hdfs_wirev_fused_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1,
	    (uint8_t *)iov[0].base + lens[0] - 1, wire_len, pk, n, &n, &wire_len, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wirev_fused_last_error(), "fragment 0"), "overlap refused");
	check(hdfs_wirev_fused_compose_packets(iov, NFRAG, block_off, seqno, V2, C, 1, wire, wire_len - 1, pk, n, &n,
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
