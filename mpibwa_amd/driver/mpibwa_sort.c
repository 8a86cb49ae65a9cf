/* mpibwa_sort.c — a finished BAM file to coordinate order: the step between `mpibwa_gpu --bam` and a duplicate marker or
 * a variant caller, for which the reference hands its per-contig files to a companion program (mpiSORT).
 *
 *     mpibwa_sort [--device] [--level L] [--index] -o OUT.bam IN.bam
 *     mpibwa_sort --index-only [--device] IN.bam
 *
 * maps IN.bam, sorts it with mi355x_bam_sort (the rank's host threads, zlib at --level, default 3) or with --device by
 * mi355x_bam_sort_dev (inflate, record walk, radix sort, record gather and deflate kernels on the MI355X), and writes OUT.bam: the header
 * with SO:coordinate, the records in samtools' coordinate order, the empty end block.  One line and a non-zero exit for an input that
 * is not BAM (plain gzip and SAM text included), for IN equal to OUT, and for a file that the device refuses for memory.
 * --index also writes OUT.bam.bai, the BAI index of OUT.bam: with --device from the sort itself
 * (mi355x_bam_sort_index_dev), else by mi355x_bam_index on the bytes about to be written.  --index-only writes IN.bam.bai for a file
 * that is in coordinate order already (mi355x_bam_index, with --device mi355x_bam_index_dev).  An input that is not in coordinate order
 * and a position beyond 2^29, BAI's limit, give one line, a non-zero exit and no .bai.
 * No MPI.  Plain C99 on include/mpibwa_amd.h; built by mpibwa_amd/build.py. */
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include "mpibwa_amd.h"

static int same_file(const char *a, const char *b)
{
	struct stat sa, sb;
	if (!strcmp(a, b)) return 1;
	if (stat(a, &sa) || stat(b, &sb)) return 0;
	return sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

static int write_file(const char *path, const uint8_t *bytes, size_t n)
{
	FILE *f = fopen(path, "wb");
	if (!f || fwrite(bytes, 1, n, f) != n || fclose(f)) {
		fprintf(stderr, "[mpibwa_sort] cannot write %s\n", path);
		return 1;
	}
	return 0;
}

/* the one line for a file that cannot be indexed */
static void index_refusal(const char *in, int64_t code, int reason)
{
	if (reason == 3) fprintf(stderr, "[mpibwa_sort] %s is not in coordinate order: the record at offset %lld of its inflated stream sorts before its predecessor\n", in, (long long)(-code - 1));
	else if (reason == 4) fprintf(stderr, "[mpibwa_sort] %s has a record (offset %lld of its inflated stream) that ends beyond 2^29, the limit of a BAI index\n", in, (long long)(-code - 1));
	else fprintf(stderr, "[mpibwa_sort] %s is not a BAM file (code %lld)\n", in, (long long)code);
}

static void memory_refusal(const char *in, const char *how)
{
	size_t free_b = 0, total_b = 0;
	mi355x_device_memory(&free_b, &total_b);
	fprintf(stderr, "[mpibwa_sort] %s does not fit the device: %llu bytes needed, %zu free (%s it without --device)\n", in,
	        (unsigned long long)mi355x_bam_sort_dev_refused_need(), free_b, how);
}

int main(int argc, char **argv)
{
	int device = 0, level = 3, level_given = 0, usage = 0, index = 0, index_only = 0;
	const char *in = 0, *out = 0;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "--device")) device = 1;
		else if (!strcmp(argv[i], "--level") && i + 1 < argc) { level = atoi(argv[++i]); level_given = 1; }
		else if (!strcmp(argv[i], "--index")) index = 1;
		else if (!strcmp(argv[i], "--index-only")) index_only = 1;
		else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
		else if (argv[i][0] == '-' || in) usage = 1;
		else in = argv[i];
	}
	if (usage || !in || (index_only ? out || index || level_given : !out)) {
		fprintf(stderr, "usage: %s [--device] [--level L] [--index] -o OUT.bam IN.bam\n"
		                "       %s --index-only [--device] IN.bam\n"
		                "  writes IN.bam in coordinate order to OUT.bam; --device: on the GPU (one compression setting), else on the cores at zlib's --level (3)\n"
		                "  --index: also OUT.bam.bai, its BAI index; --index-only: IN.bam.bai for an IN.bam that is in coordinate order already\n", argv[0], argv[0]);
		return 1;
	}
	if (!index_only && same_file(in, out)) {
		fprintf(stderr, "[mpibwa_sort] %s is both the input and the output\n", in);
		return 1;
	}
	if (device && level_given) fprintf(stderr, "[mpibwa_sort] --level has no effect on the blocks with --device (the device encoder has one setting)\n");
	const int fd = open(in, O_RDONLY);
	struct stat st;
	if (fd < 0 || fstat(fd, &st)) {
		fprintf(stderr, "[mpibwa_sort] cannot open %s\n", in);
		return 1;
	}
	const size_t len = (size_t)st.st_size;
	const uint8_t *bam = len ? (const uint8_t *)mmap(0, len, PROT_READ, MAP_PRIVATE, fd, 0) : (const uint8_t *)"";
	if (bam == (const uint8_t *)MAP_FAILED) {
		fprintf(stderr, "[mpibwa_sort] cannot map %s\n", in);
		return 1;
	}
	char *bai_path = (char *)malloc(strlen(index_only ? in : out) + 5);
	if (!bai_path) return 1;
	sprintf(bai_path, "%s.bai", index_only ? in : out);
	uint8_t *bai = 0;
	size_t bai_len = 0;
	int reason = 0;
	if (index_only) {
		const int64_t r = device ? mi355x_bam_index_dev(bam, len, &bai, &bai_len, &reason) : mi355x_bam_index(bam, len, &bai, &bai_len, &reason);
		if (r == INT64_MIN) { memory_refusal(in, "index"); return 1; }
		if (r < 0) { index_refusal(in, r, reason); return 1; }
		if (write_file(bai_path, bai, bai_len)) return 1;
		fprintf(stderr, "[mpibwa_sort] wrote %s: %zu bytes for %lld records\n", bai_path, bai_len, (long long)r);
		if (device) mi355x_finalize();
		free(bai); free(bai_path);
		return 0;
	}
	const int64_t cap = mi355x_bam_sort_bound(bam, len);
	uint8_t *buf = cap > 0 ? (uint8_t *)malloc((size_t)cap) : 0;
	if (cap > 0 && !buf) {
		fprintf(stderr, "[mpibwa_sort] no memory for %lld bytes of output\n", (long long)cap);
		return 1;
	}
	const int64_t n = cap <= 0 ? cap
	                : device ? (index ? mi355x_bam_sort_index_dev(bam, len, buf, (size_t)cap, &bai, &bai_len, &reason) : mi355x_bam_sort_dev(bam, len, buf, (size_t)cap))
	                         : mi355x_bam_sort(bam, len, level, buf, (size_t)cap);
	if (n == INT64_MIN) { memory_refusal(in, "sort"); return 1; }
	if (n <= 0) {
		index_refusal(in, n, reason == 4 ? 4 : 0);
		return 1;
	}
	if (index && !device) {   // the host path: the index of the bytes about to be written
		const int64_t r = mi355x_bam_index(buf, (size_t)n, &bai, &bai_len, &reason);
		if (r < 0) { index_refusal(in, r, reason); return 1; }
	}
	if (write_file(out, buf, (size_t)n)) return 1;
	if (index && write_file(bai_path, bai, bai_len)) return 1;
	if (index) fprintf(stderr, "[mpibwa_sort] wrote %s: %lld bytes, and %s: %zu bytes\n", out, (long long)n, bai_path, bai_len);
	else fprintf(stderr, "[mpibwa_sort] wrote %s: %lld bytes\n", out, (long long)n);
	if (device) mi355x_finalize();
	free(buf); free(bai); free(bai_path);
	return 0;
}
