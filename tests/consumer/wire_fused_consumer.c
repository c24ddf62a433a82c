/*
 * C consumer of the fused wire-stream companion library
 * (include/hadoofus_wire_fused.h), written the way a device-to-device replica
 * hop would use it: a write at an odd address of a device
 * allocation is composed into one wire stream at another odd address in one
 * pass, and the stream is handed, still in device memory, to
 * hdfs_crc32c_verify_packets.  As a check
 * the same stream is assembled on the host from hdfs_crc32c_compose_packets'
 * header buffers and the data: the two must be identical, records included
 * (hdr_off apart, which counts in the stream).
 * Prints the packet count and "0 failures" on success.
 * Test infrastructure (tests/test_wire_fused_cpu.py links it on CPU,
 * tests/test_gpu_wire_fused.py runs it on the GPU).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_wire_fused.h"

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; wire_fused: %s)\n", what, hdfs_crc32c_last_error(), hdfs_wire_fused_last_error());
		failures++;
	}
}

int main(void)
{
	const uint64_t len = 3 * 65536 + 4000 + 77, src_at = 3, arena_bytes = 1 << 20;
	const int64_t block_off = 4321, seqno = 17;
	void *arena = NULL;
	size_t n = 0, n_c = 0, n_v = 0;
	uint64_t wire_len = 0, used = 0, consumed = 0;

	check(hdfs_wire_fused_abi_version() == HDFS_WIRE_FUSED_ABI_VERSION, "abi version");
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0, "dev_alloc");
	check(hdfs_crc32c_fill_splitmix64(arena, arena_bytes / 8, 11, 0, NULL) == 0, "fill");
	uint8_t *data = (uint8_t *)arena + src_at;
	uint8_t *wire = (uint8_t *)arena + 512 * 1024 + 5;

	/* size query (no device work), then the call */
	check(hdfs_wire_fused_compose_packets(data, len, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    NULL, 0, NULL, 0, &n, &wire_len, NULL) == 0 && n == 6 && wire_len == len + 6 * 31 + 4 * 393, "size query");
	hdfs_crc32c_out_packet *pk = calloc(n, sizeof(*pk)), *pk_c = calloc(n, sizeof(*pk_c));
	check(hdfs_wire_fused_compose_packets(data, len, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    wire, wire_len, pk, n, &n, &wire_len, NULL) == 0, "wire compose");

	/* the same stream from the main library's header buffers, on the host */
	uint8_t *hdr = malloc(wire_len), *want = malloc(wire_len), *got = malloc(wire_len), *host = malloc(len);
	check(hdfs_crc32c_compose_packets(data, len, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    hdr, wire_len, pk_c, n, &n_c, &used) == 0 && n_c == n && used + len == wire_len, "compose_packets");
	check(hdfs_crc32c_memcpy(host, data, len, 1) == 0 && hdfs_crc32c_memcpy(got, wire, wire_len, 1) == 0, "d2h");
	uint64_t at = 0;
	for (size_t i = 0; i < n_c && i < n; i++) {
		check(pk[i].hdr_off == at, "hdr_off counts in the stream");
		memcpy(want + at, hdr + pk_c[i].hdr_off, pk_c[i].hdr_len);
		at += pk_c[i].hdr_len;
		memcpy(want + at, host + pk_c[i].data_off, (size_t)pk_c[i].data_len);
		at += (uint64_t)pk_c[i].data_len;
		pk_c[i].hdr_off = pk[i].hdr_off;
	}
	check(at == wire_len && memcmp(got, want, wire_len) == 0, "stream identical");
	check(memcmp(pk, pk_c, n * sizeof(*pk)) == 0, "packet records identical");
	printf("%zu packets, %llu stream bytes\n", n, (unsigned long long)wire_len);

	/* the next hop: the stream verified where it lies */
	hdfs_crc32c_packet *vp = calloc(n, sizeof(*vp));
	check(hdfs_crc32c_verify_packets(wire, wire_len, HDFS_CRC32C_PROTO_V2, 512, HDFS_CRC32C_CSUM_CRC32C, vp, n, &n_v,
	    &consumed) == 0 && n_v == n && consumed == wire_len, "verify_packets on the device stream");

	/* refused: a host destination, a stream over its own source, one byte of room too few */
	check(hdfs_wire_fused_compose_packets(data, len, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    got, wire_len, pk, n, &n, &wire_len, NULL) == HDFS_CRC32C_EINVAL, "host wire refused");
	check(hdfs_wire_fused_compose_packets(data, len, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    data + len - 1, wire_len, pk, n, &n, &wire_len, NULL) == HDFS_CRC32C_EINVAL, "overlap refused");
	check(hdfs_wire_fused_compose_packets(data, len, block_off, seqno, HDFS_CRC32C_PROTO_V2, HDFS_CRC32C_CSUM_CRC32C, 1,
	    wire, wire_len - 1, pk, n, &n, &wire_len, NULL) == HDFS_CRC32C_EINVAL, "short wire refused");

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
