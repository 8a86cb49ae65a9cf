// bam_kernel.hip — a piece of SAM text to BAM records on the device, and the BGZF cuts of those records: the passes between the upload of
// a chunk's text and bgzf_deflate_kernel.  The layout and every per-line decision are bam_util.h's, shared with the host encoder
// (sampost.cpp); this file adds what needs a wavefront.  DESIGN §8.4.
//
//   1. line starts   bam_count_kernel: newlines per 64-byte window by ballot and popcount, summed per chunk of 4 KiB (a wavefront);
//                    bam_scan_kernel over the chunks; bam_starts_kernel walks its chunk's windows again and writes where every line starts.
//   2. size pass     bam_size_kernel, a line per lane: bam::plan_line (fields, numbers, contig lookup, tag sizes) -> the plan, the record's
//                    size, the verdict.  An error leaves the smallest offset in ctl->err (an atomic per malformed line: rare), a declined
//                    line sets ctl->decline.  A wavefront adds its 64 sizes up into group[].
//   3. scan          bam_scan_kernel over the groups; it also decides whether the piece is the device's (ctl->n_write).
//   4. write pass    bam_write_kernel, a wavefront per 64 lines: every lane writes its line's frame (core, QNAME, CIGAR, tags), then the
//                    wavefront goes through the 64 lines together and packs SEQ and QUAL - 33, two thirds of the bytes, with consecutive
//                    lanes on consecutive bytes.
//   5. cuts          bam_fit_kernel: for every record the last record end within 0xff00 bytes of its start (bam::last_fit, a binary search
//                    per lane); bam_chain_kernel: one lane follows that chain from record 0, at most 512 steps, and writes cut[].
//
// No atomic is shared per item; ballot and shuffle stand in wave-uniform code only; a workgroup is one wavefront wherever lines differ
// in length.  Every store is bounded by ctl->n_write <= BAM_DEV_LINES and ctl->bam_bytes <= BAM_DEV_BYTES, decided in pass 3 before
// anything is written.
#include "hip_util.h"
#include "device.h"
#include "bam_util.h"

namespace mbw {
namespace {

constexpr uint32_t NONE = 0xffffffffu;

__device__ inline uint32_t wave_scan_u32(uint32_t x, int lane)   // inclusive; uniform code only
{
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = (uint32_t)__shfl_up((int)x, d, 64);
		x += t & (0u - (uint32_t)(lane >= d));
	}
	return x;
}

__global__ __launch_bounds__(64) void bam_count_kernel(const uint8_t *__restrict__ text, uint32_t len, uint32_t *__restrict__ chunk_cnt)
{
	const int lane = (int)threadIdx.x;
	const uint32_t base = (uint32_t)blockIdx.x * BAM_DEV_CHUNK;
	uint32_t cnt = 0;
	for (uint32_t w = 0; w < BAM_DEV_CHUNK; w += 64) {
		const uint32_t p = base + w + (uint32_t)lane;
		const bool nl = p < len && text[p] == '\n';
		cnt += (uint32_t)__popcll(__ballot(nl));
	}
	if (lane == 0) chunk_cnt[blockIdx.x] = cnt;
}

// a[0 .. n) to its exclusive prefix sums in place, a[n] = the total; one workgroup.  what = 0: the chunks' newline counts (n = n_host; the
// total is the piece's number of lines), 1: the groups' record bytes (n from ctl->n_lines; the total is the piece's BAM bytes, and the
// piece's fate is decided).
__global__ __launch_bounds__(1024) void bam_scan_kernel(uint32_t *__restrict__ a, uint32_t n_host, BamDevCtl *__restrict__ ctl, int what)
{
	__shared__ uint32_t part[1024];
	const uint32_t t = threadIdx.x, n = what ? (ctl->n_lines + 63) / 64 : n_host;
	const uint32_t per = (n + 1023) / 1024, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
	uint32_t sum = 0;
	for (uint32_t k = lo; k < hi; ++k) sum += a[k];
	part[t] = sum;
	__syncthreads();
	for (uint32_t d = 1; d < 1024; d <<= 1) {
		const uint32_t v = t >= d ? part[t - d] : 0u;
		__syncthreads();
		part[t] += v;
		__syncthreads();
	}
	uint32_t run = part[t] - sum;
	for (uint32_t k = lo; k < hi; ++k) { const uint32_t v = a[k]; a[k] = run; run += v; }
	if (t == 1023) {
		const uint32_t total = part[1023];
		a[n] = total;
		if (!what) {
			const bool fits = total <= BAM_DEV_LINES;
			ctl->n_lines = fits ? total : 0u;
			if (!fits) ctl->decline = 1;
		} else {
			const bool mine = ctl->err == NONE && !ctl->decline && total <= BAM_DEV_BYTES;
			if (!mine && ctl->err == NONE) ctl->decline = 1;
			ctl->bam_bytes = mine ? total : 0u;
			ctl->n_write = mine ? ctl->n_lines : 0u;
		}
	}
}

__global__ __launch_bounds__(64) void bam_starts_kernel(const uint8_t *__restrict__ text, uint32_t len, const uint32_t *__restrict__ chunk_cnt,
                                                        uint32_t *__restrict__ line_start, const BamDevCtl *__restrict__ ctl)
{
	const int lane = (int)threadIdx.x;
	const uint32_t n_lines = ctl->n_lines;   // 0: too many for line_start[]
	if (!n_lines) return;
	const uint32_t base = (uint32_t)blockIdx.x * BAM_DEV_CHUNK;
	uint32_t line = chunk_cnt[blockIdx.x];   // newlines before this chunk = index of the line the chunk's first byte is in
	if (blockIdx.x == 0 && lane == 0) line_start[0] = 0;
	for (uint32_t w = 0; w < BAM_DEV_CHUNK; w += 64) {
		const uint32_t p = base + w + (uint32_t)lane;
		const bool nl = p < len && text[p] == '\n';
		const uint64_t m = __ballot(nl);
		if (nl) {
			const uint32_t idx = line + (uint32_t)__popcll(m & ((1ull << lane) - 1)) + 1;   // the line behind this newline
			if (idx <= n_lines) line_start[idx] = p + 1;
		}
		line += (uint32_t)__popcll(m);
	}
}

__global__ __launch_bounds__(64) void bam_size_kernel(const uint8_t *__restrict__ text, const void *__restrict__ contigs, const uint32_t *__restrict__ line_start,
                                                      bam::LinePlan *__restrict__ plan, uint32_t *__restrict__ group, BamDevCtl *__restrict__ ctl)
{
	const int lane = (int)threadIdx.x;
	const uint32_t n = ctl->n_lines, i = (uint32_t)blockIdx.x * 64 + (uint32_t)lane;
	if ((uint32_t)blockIdx.x * 64 >= n) return;   // (uniform)
	uint32_t size = 0;
	if (i < n) {
		const bam::ContigTable tab = bam::contig_table_at(contigs);
		const uint32_t at = line_start[i], end = line_start[i + 1];
		bam::LinePlan P;
		const int verdict = bam::plan_line(text + at, end - at - 1, tab, P);
		if (verdict == bam::BAM_ERROR) atomicMin(&ctl->err, at);
		else if (verdict == bam::BAM_DECLINE) atomicOr(&ctl->decline, 1u);
		plan[i] = P;
		size = P.size;
	}
	const uint32_t incl = wave_scan_u32(size, lane);
	if (lane == 63) group[blockIdx.x] = incl;
}

__global__ __launch_bounds__(64) void bam_write_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_start,
                                                       const bam::LinePlan *__restrict__ plan, const uint32_t *__restrict__ group,
                                                       uint32_t *__restrict__ rec_off, uint8_t *__restrict__ bam_out, const BamDevCtl *__restrict__ ctl)
{
	const int lane = (int)threadIdx.x;
	const uint32_t n = ctl->n_write, first = (uint32_t)blockIdx.x * 64, i = first + (uint32_t)lane;
	if (first >= n) return;   // (uniform)
	const bool active = i < n;
	bam::LinePlan P;
	P.size = 0; P.l_seq = 0; P.o_seq = 0; P.o_qual = 0; P.qual_star = 0; P.l_qname = 0; P.n_cigar = 0;
	uint32_t at = 0;
	if (active) { P = plan[i]; at = line_start[i]; }
	const uint32_t incl = wave_scan_u32(P.size, lane);
	const uint32_t off = group[blockIdx.x] + incl - P.size;
	if (active) {
		rec_off[i] = off;
		if (i == n - 1) rec_off[n] = off + P.size;
		bam::write_frame(text + at, P, bam_out + off);
	}
	// SEQ and QUAL of the wavefront's lines, one line at a time, all lanes
	const uint32_t cnt = n - first < 64 ? n - first : 64;
	const uint32_t my_seq_in = at + P.o_seq, my_qual_in = at + P.o_qual, my_seq_out = off + bam::rec_seq_at(P), my_l = (uint32_t)P.l_seq, my_star = P.qual_star;
	for (uint32_t j = 0; j < cnt; ++j) {
		const uint32_t l_seq = (uint32_t)__shfl((int)my_l, (int)j, 64);
		const uint32_t seq_in = (uint32_t)__shfl((int)my_seq_in, (int)j, 64), qual_in = (uint32_t)__shfl((int)my_qual_in, (int)j, 64);
		const uint32_t seq_out = (uint32_t)__shfl((int)my_seq_out, (int)j, 64), star = (uint32_t)__shfl((int)my_star, (int)j, 64);
		const uint32_t n_packed = (l_seq + 1) / 2, qual_out = seq_out + n_packed;
		const uint8_t *seq = text + seq_in;
		for (uint32_t k = (uint32_t)lane; k < n_packed; k += 64) bam_out[seq_out + k] = bam::seq_byte(seq, l_seq, k);
		if (star) for (uint32_t k = (uint32_t)lane; k < l_seq; k += 64) bam_out[qual_out + k] = 0xff;
		else for (uint32_t k = (uint32_t)lane; k < l_seq; k += 64) bam_out[qual_out + k] = (uint8_t)(text[qual_in + k] - 33);
	}
}

__global__ __launch_bounds__(256) void bam_fit_kernel(const uint32_t *__restrict__ rec_off, uint32_t *__restrict__ next, const BamDevCtl *__restrict__ ctl)
{
	const uint32_t n = ctl->n_write, i = (uint32_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) next[i] = bam::last_fit(rec_off, n, i);
}

__global__ __launch_bounds__(64) void bam_chain_kernel(const uint32_t *__restrict__ rec_off, const uint32_t *__restrict__ next, uint32_t *__restrict__ cut,
                                                       BamDevCtl *__restrict__ ctl)
{
	if (threadIdx.x != 0) return;
	const uint32_t n = ctl->n_write;
	uint32_t nb = 0, i = 0;
	cut[0] = 0;
	while (i < n && nb < BAM_DEV_BLOCKS) {
		const uint32_t j = next[i];   // > i: no record of the device's is larger than a block
		cut[++nb] = rec_off[j];
		i = j;
	}
	if (i < n) { nb = 0; ctl->decline = 1; ctl->n_write = 0; ctl->bam_bytes = 0; }   // more blocks than slots: the host's piece
	ctl->n_blocks = nb;
}

} // namespace

size_t bam_plan_bytes() { return sizeof(bam::LinePlan); }

void launch_bam_encode(void *stream, const BamDevBufs &B)
{
	hipStream_t st = (hipStream_t)stream;
	const uint32_t n_chunks = (B.text_len + BAM_DEV_CHUNK - 1) / BAM_DEV_CHUNK;
	if (!n_chunks || B.text_len > BAM_DEV_TEXT) return;
	hipLaunchKernelGGL(bam_count_kernel, dim3(n_chunks), dim3(64), 0, st, B.text, B.text_len, B.chunk_cnt);
	hipLaunchKernelGGL(bam_scan_kernel, dim3(1), dim3(1024), 0, st, B.chunk_cnt, n_chunks, B.ctl, 0);
	hipLaunchKernelGGL(bam_starts_kernel, dim3(n_chunks), dim3(64), 0, st, B.text, B.text_len, B.chunk_cnt, B.line_start, B.ctl);
	// a launch covers every line the piece can have (a newline per byte at the worst), up to BAM_DEV_LINES: workgroups behind ctl->n_lines return at once
	uint32_t max_lines = B.text_len;
	if (max_lines > BAM_DEV_LINES) max_lines = BAM_DEV_LINES;
	const uint32_t groups = (max_lines + 63) / 64;
	hipLaunchKernelGGL(bam_size_kernel, dim3(groups), dim3(64), 0, st, B.text, B.contigs, B.line_start, (bam::LinePlan *)B.plan, B.group, B.ctl);
	hipLaunchKernelGGL(bam_scan_kernel, dim3(1), dim3(1024), 0, st, B.group, 0u, B.ctl, 1);
	hipLaunchKernelGGL(bam_write_kernel, dim3(groups), dim3(64), 0, st, B.text, B.line_start, (const bam::LinePlan *)B.plan, B.group, B.rec_off, B.bam, B.ctl);
	HIP_OK(hipGetLastError());
}

void launch_bam_cuts(void *stream, const BamDevBufs &B)
{
	hipStream_t st = (hipStream_t)stream;
	uint32_t max_lines = B.text_len;
	if (max_lines > BAM_DEV_LINES) max_lines = BAM_DEV_LINES;
	hipLaunchKernelGGL(bam_fit_kernel, dim3((max_lines + 255) / 256), dim3(256), 0, st, B.rec_off, B.next, B.ctl);
	hipLaunchKernelGGL(bam_chain_kernel, dim3(1), dim3(64), 0, st, B.rec_off, B.next, B.cut, B.ctl);
	HIP_OK(hipGetLastError());
}

} // namespace mbw
