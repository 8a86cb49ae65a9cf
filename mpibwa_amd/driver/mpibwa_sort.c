/* mpibwa_sort.c — a finished BAM file to coordinate order: the step between `mpibwa_gpu --bam` and a duplicate marker or
 * a variant caller, for which the reference hands its per-contig files to a companion program (mpiSORT).
 *
 *     mpibwa_sort [--device] [--level L] -o OUT.bam IN.bam
 *
 * maps IN.bam, sorts it with mi355x_bam_sort (the rank's host threads, zlib at --level, default 3) or with --device by
 * mi355x_bam_sort_dev (inflate, record walk, radix sort, record gather and deflate kernels on the MI355X), and writes OUT.bam: the header
 * with SO:coordinate, the records in samtools' coordinate order, the empty end block.  One line and a non-zero exit for an input that
 * is not BAM (plain gzip and SAM text included), for IN equal to OUT, and for a file that the device refuses for memory.
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

int main(int argc, char **argv)
{
	int device = 0, level = 3, level_given = 0, usage = 0;
	const char *in = 0, *out = 0;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "--device")) device = 1;
		else if (!strcmp(argv[i], "--level") && i + 1 < argc) { level = atoi(argv[++i]); level_given = 1; }
		else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
		else if (argv[i][0] == '-' || in) usage = 1;
		else in = argv[i];
	}
	if (usage || !in || !out) {
		fprintf(stderr, "usage: %s [--device] [--level L] -o OUT.bam IN.bam\n"
		                "  writes IN.bam in coordinate order to OUT.bam; --device: on the GPU (one compression setting), else on the cores at zlib's --level (3)\n", argv[0]);
		return 1;
	}
	if (same_file(in, out)) {
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
	const int64_t cap = mi355x_bam_sort_bound(bam, len);
	uint8_t *buf = cap > 0 ? (uint8_t *)malloc((size_t)cap) : 0;
	if (cap > 0 && !buf) {
		fprintf(stderr, "[mpibwa_sort] no memory for %lld bytes of output\n", (long long)cap);
		return 1;
	}
	const int64_t n = cap <= 0 ? cap : device ? mi355x_bam_sort_dev(bam, len, buf, (size_t)cap) : mi355x_bam_sort(bam, len, level, buf, (size_t)cap);
	if (n == INT64_MIN) {
		size_t free_b = 0, total_b = 0;
		mi355x_device_memory(&free_b, &total_b);
		fprintf(stderr, "[mpibwa_sort] %s does not fit the device: %llu bytes needed, %zu free (sort it without --device)\n", in,
		        (unsigned long long)mi355x_bam_sort_dev_refused_need(), free_b);
		return 1;
	}
	if (n <= 0) {
		fprintf(stderr, "[mpibwa_sort] %s is not a BAM file (code %lld)\n", in, (long long)n);
		return 1;
	}
	FILE *f = fopen(out, "wb");
	if (!f || fwrite(buf, 1, (size_t)n, f) != (size_t)n || fclose(f)) {
		fprintf(stderr, "[mpibwa_sort] cannot write %s\n", out);
		return 1;
	}
	fprintf(stderr, "[mpibwa_sort] wrote %s: %lld bytes\n", out, (long long)n);
	if (device) mi355x_finalize();
	free(buf);
	return 0;
}
