/*
 * C consumer of the fused gather-wire batch companion library
 * (include/hadoofus_wirev_fused_batch.h), written the way a datanode with many
 * hdfs_datanode_writev calls outstanding would use it with device-resident
 * streams as the goal: four writes, held in fragments at odd
 * addresses of one device allocation -- five fragments in descending address
 * order with an empty one and one of three bytes; no fragment at all with
 * finish; two fragments with the seam inside the short first packet; one
 * fragment -- are composed into four wire streams in one call and one pass,
 * and every stream is handed, still in device memory, to
 * hdfs_crc32c_verify_packets.  As a check every stream is assembled on the
 * host from hdfs_crc32c_compose_packets' header buffers of the write's
 * concatenation and its bytes: the two must be identical, records included
 * (hdr_off apart, which counts in the write's own stream).
 * Prints the totals and "0 failures" on success.
 * Test infrastructure (tests/test_wirev_fused_batch_cpu.py links it on CPU,
 * tests/test_gpu_wirev_fused_batch.py runs it on the GPU).  C99.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hadoofus_wirev_fused_batch.h"

static int failures;

static void check(int cond, const char *what)
{
	if (!cond) {
		printf("FAIL: %s (crc32c: %s; wirev_fused_batch: %s)\n", what, hdfs_crc32c_last_error(),
		    hdfs_wirev_fused_batch_last_error());
		failures++;
	}
}

#define NW 4
#define MAXF 5

int main(void)
{
	static const int cnt[NW] = { 5, 0, 2, 1 };
	static const uint64_t lens[NW][MAXF] = {
		{ 65536 + 4000 + 77, 0, 3, 2 * 65536 - 3 - 200, 200 }, { 0 }, { 100, 70000 }, { 1300 } };
	static const uint64_t at[NW][MAXF] = {
		{ 400001, 0, 350007, 150005, 5 }, { 0 }, { 500003, 520001 }, { 600009 } };
	static const int64_t block_off[NW] = { 4321, 1024, 4321, 0 };
	static const int finish[NW] = { 1, 1, 0, 1 };
	const uint64_t arena_bytes = 2 << 20;
	const int V2 = HDFS_CRC32C_PROTO_V2, C = HDFS_CRC32C_CSUM_CRC32C;
	void *arena = NULL;
	hdfs_crc32c_iovec iov[NW][MAXF];
	hdfs_wirev_fused_batch_write w[NW];
	hdfs_wirev_fused_batch_totals tot;
	hdfs_crc32c_out_packet *pk, *pk_c;
	hdfs_crc32c_packet *vp;
	uint8_t *hdr, *want, *got, *host;
	size_t n = 0, n_c = 0, n_v = 0, i;
	uint64_t wire_at = (1 << 20) + 5, used = 0, consumed = 0;
	int k, f;

	check(hdfs_wirev_fused_batch_abi_version() == HDFS_WIREV_FUSED_BATCH_ABI_VERSION, "abi version");
	check(hdfs_crc32c_dev_alloc(&arena, arena_bytes) == 0, "dev_alloc");
	check(hdfs_crc32c_fill_splitmix64(arena, arena_bytes / 8, 11, 0, NULL) == 0, "fill");
	memset(w, 0, sizeof(w));
	for (k = 0; k < NW; k++) {
		for (f = 0; f < cnt[k]; f++) {
			iov[k][f].base = lens[k][f] ? (uint8_t *)arena + at[k][f] : NULL;
			iov[k][f].len = lens[k][f];
		}
		w[k].iov = iov[k];
		w[k].iovcnt = cnt[k];
		w[k].finish = finish[k];
		w[k].offset_in_block = block_off[k];
		w[k].seqno = 100 * k;
	}

	/* layout and size query (no device work), then the call */
	check(hdfs_wirev_fused_batch_layout(w, NW, V2, C, &tot) == 0 && tot.table_entries == 4 && tot.nfrags == 7 &&
	    tot.seamed_rounds == 1 && tot.seamed_ragged == 2 && tot.max_frags_per_round == 3 &&
	    tot.rounds > tot.seamed_rounds && w[1].npkts == 1 && w[1].wire_len == 31 && w[2].len == 70100, "layout");
	printf("layout: %llu packets, %llu chunks, %llu fragments, %llu rounds (%llu seamed), %llu stream bytes\n",
	    (unsigned long long)tot.npkts, (unsigned long long)tot.nchunks, (unsigned long long)tot.nfrags,
	    (unsigned long long)tot.rounds, (unsigned long long)tot.seamed_rounds, (unsigned long long)tot.wire_bytes);
	check(hdfs_wirev_fused_batch_compose(w, NW, V2, C, NULL, 0, &n, NULL) == 0 && n == tot.npkts, "size query");
	for (k = 0; k < NW; k++) {
		w[k].wire = (uint8_t *)arena + wire_at;
		w[k].wire_cap = w[k].wire_len;
		wire_at += w[k].wire_len + 37;
	}
	check(wire_at <= arena_bytes, "the streams fit");
	pk = calloc(n, sizeof(*pk));
	pk_c = calloc(n, sizeof(*pk_c));
	vp = calloc(n, sizeof(*vp));
	check(hdfs_wirev_fused_batch_compose(w, NW, V2, C, pk, n, &n, NULL) == 0, "fused wirev batch compose");

	/* every stream from the main library's header buffers of the write's concatenation, on the host */
	for (k = 0; k < NW; k++) {
		const uint64_t wl = w[k].wire_len;
		hdfs_crc32c_out_packet *p = pk + w[k].first_pkt;
		uint64_t pos = 0, o = 0;

		hdr = malloc(wl + 1);
		want = malloc(wl + 1);
		got = malloc(wl + 1);
		host = malloc(w[k].len + 1);
		for (f = 0; f < cnt[k]; f++) {
			if (lens[k][f])
				check(hdfs_crc32c_memcpy(host + pos, iov[k][f].base, lens[k][f], 1) == 0, "d2h of a fragment");
			pos += lens[k][f];
		}
		check(pos == w[k].len, "len is the fragments' sum");
		check(hdfs_crc32c_compose_packets(host, w[k].len, block_off[k], 100 * k, V2, C, finish[k], hdr, wl, pk_c, n,
		    &n_c, &used) == 0 && n_c == w[k].npkts && used + w[k].len == wl, "compose_packets of the concatenation");
		check(hdfs_crc32c_memcpy(got, w[k].wire, wl, 1) == 0, "d2h of the stream");
		for (i = 0; i < n_c && i < w[k].npkts; i++) {
			check(p[i].hdr_off == o, "hdr_off counts in the write's stream");
			memcpy(want + o, hdr + pk_c[i].hdr_off, pk_c[i].hdr_len);
			o += pk_c[i].hdr_len;
			memcpy(want + o, host + pk_c[i].data_off, (size_t)pk_c[i].data_len);
			o += (uint64_t)pk_c[i].data_len;
			pk_c[i].hdr_off = p[i].hdr_off;
		}
		check(o == wl && memcmp(got, want, wl) == 0, "stream identical");
		check(memcmp(p, pk_c, w[k].npkts * sizeof(*p)) == 0, "packet records identical");
		/* the next hop: the stream verified where it lies */
		check(hdfs_crc32c_verify_packets(w[k].wire, wl, V2, 512, C, vp, n, &n_v, &consumed) == 0 &&
		    n_v == w[k].npkts && consumed == wl, "verify_packets on the device stream");
		free(hdr);
		free(want);
		free(got);
		free(host);
	}
	printf("%lu packets, %llu stream bytes\n", (unsigned long)n, (unsigned long long)tot.wire_bytes);

	/* refused: a host fragment, a stream over another entry's fragment, one byte of room too few, a lone NULL wire */
	host = malloc(64);
	iov[2][0].base = host;
	check(hdfs_wirev_fused_batch_compose(w, NW, V2, C, pk, n, &n, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wirev_fused_batch_last_error(), "entry 2") &&
	    strstr(hdfs_wirev_fused_batch_last_error(), "fragment 0"), "host fragment refused");
	iov[2][0].base = (uint8_t *)arena + at[2][0];
	got = w[3].wire;
	w[3].wire = (uint8_t *)iov[0][3].base + lens[0][3] - 1;
	check(hdfs_wirev_fused_batch_compose(w, NW, V2, C, pk, n, &n, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wirev_fused_batch_last_error(), "entry 3") &&
	    strstr(hdfs_wirev_fused_batch_last_error(), "fragment 3 of entry 0"), "overlap refused");
	w[3].wire = got;
	w[0].wire_cap--;
	check(hdfs_wirev_fused_batch_compose(w, NW, V2, C, pk, n, &n, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wirev_fused_batch_last_error(), "entry 0"), "short wire refused");
	w[0].wire_cap++;
	w[1].wire = NULL;
	check(hdfs_wirev_fused_batch_compose(w, NW, V2, C, pk, n, &n, NULL) == HDFS_CRC32C_EINVAL &&
	    strstr(hdfs_wirev_fused_batch_last_error(), "entry 1"), "mixed NULL wires refused");

	free(host);
	free(vp);
	free(pk);
	free(pk_c);
	hdfs_crc32c_dev_free(arena);
	printf("%d failures\n", failures);
	return failures != 0;
}
