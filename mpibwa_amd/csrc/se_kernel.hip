// se_kernel.hip — the decisions of the single-end branch of worker2 for the reads that end in ONE record, a read per lane.
//
// Device counterpart, for two shapes of read, of
//   worker2, single-end branch  src/bwamem.c:1187-1196   (mem_mark_primary_se with id = n_processed + i, then mem_reg2sam)
//   mem_reg2sam                 src/bwamem.c:1003-1049   (which regions become lines)
//   mem_gen_alt                 src/bwamem_extra.c:91-110 (only its test "does any secondary hit get an XA entry?")
//   mem_approx_mapq_se          src/bwamem.c:952-976     (csub = 0: only mate rescue sets it)
//   mem_reg2aln                 src/bwamem.c:1089-1105   (the band of the final global alignment)
//   mem_sort_dedup_patch        src/bwamem.c:437-489     (up to PR_MAXREG regions, as long as no two get as far as mem_patch_reg's alignment)
// The shapes: a read none of whose regions reaches the score threshold T (one "unmapped" record, flag 4), and a read with exactly
// one primary region of at least T, no secondary region close enough to its primary for an XA entry and no region on an ALT contig
// (one record, no SA / XA / pa tag).  For such a read the kernel writes what the host's COLLECT pass would have listed — the request
// for aln_kernel and the line descriptor for sam_emit_kernel — so its record is made without the host touching the read; every
// other read is left to the host with its full logic (mem_mark_primary_se, mem_gen_alt, mem_reg2sam in host_regs.cpp).
// The helpers (pair_common.cuh) are the pairing kernel's own, the arithmetic (pairmath.h) the host's: its types and order are the reference's.
#include <hip/hip_runtime.h>
#include "pair_common.cuh"

namespace mbw {

// status[i]: SE_DECIDED = decided here; every other value: the host's read, and the number says which test sent it there
// (device.h lists the codes; they follow pair_simple_kernel's where the test is the same)
__global__ void __launch_bounds__(64)
se_simple_kernel(PairParams P, int n_reads, const DevReg *__restrict__ first, const int *__restrict__ nfirst, const uint8_t *__restrict__ read_ok,
                 const uint8_t *__restrict__ ann_alt, const double *__restrict__ ltab, uint8_t *__restrict__ status, AlnReq *__restrict__ reqs,
                 SamDesc *__restrict__ desc)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_reads) return;
	AlnReq none;
	none.rb = none.re = 0; none.read = -1; none.qb = none.qe = none.w2 = none.truesc = none.pad = 0;
	reqs[i] = none;
	desc[i].req = -1;
	status[i] = SE_HOST;
	if (!read_ok[i]) { status[i] = SE_HOST_COMMENT; return; }
	int n = nfirst[i];
	if (n < 0) return;
	if (n > PR_MAXREG) { status[i] = SE_HOST_MAXREG; return; }
	PReg a[PR_MAXREG];
	{
		DevReg r[PR_MAXREG];
		for (int j = 0; j < n; ++j) r[j] = first[(size_t)i * PR_MAXREG + j];
		n = dedup_small(P, r, n);
		if (n < 0) { status[i] = SE_HOST_PATCH; return; }   // two hits the host has to try to patch
		for (int j = 0; j < n; ++j) {
			a[j].d = r[j]; a[j].sub = a[j].sub_n = 0; a[j].secondary = a[j].secondary_all = -1; a[j].hash = 0;
			if (ann_alt[r[j].rid]) { status[i] = SE_HOST_ALT; return; }
			const int l = r[j].qe - r[j].qb > r[j].re - r[j].rb ? r[j].qe - r[j].qb : (int)(r[j].re - r[j].rb);
			if (l >= P.ltab_n || l <= 0) { status[i] = SE_HOST_LENGTH; return; }
		}
	}
	if (n > 0) mark_primary(P, a, n, P.id0 + (u64)i);
	// the lines of mem_reg2sam (src/bwamem.c:1015-1032) without MEM_F_ALL: the primary regions of at least T
	int n_lines = 0, z = -1;
	for (int j = 0; j < n; ++j)
		if (a[j].secondary < 0 && a[j].d.score >= P.T) { if (n_lines == 0) z = j; ++n_lines; }
	if (n_lines == 0) {   // "no alignments good enough": the unaligned record (:1033-1037); XA strings are attached to lines only
		SamDesc d;
		d.rb = d.re = 0; d.qb = d.qe = 0; d.req = -3; d.rid = -1;
		d.flag = 0x4; d.mapq = 0; d.score = 0; d.sub = 0;
		desc[i] = d;
		status[i] = SE_DECIDED;
		return;
	}
	if (n_lines > 1) { status[i] = SE_HOST_SUPP; return; }   // a supplementary line (SA tags, the MAPQ cap of :1029)
	// a secondary hit close enough to its primary gets an XA entry (src/bwamem_extra.c:91-110): the host's kind of record
	for (int j = 0; j < n; ++j) {
		const int kk = a[j].secondary_all;
		if (kk >= 0 && a[j].d.score >= a[kk].d.score * (double)P.XA_drop_ratio) { status[i] = SE_HOST_XA; return; }
	}
	const PReg &R = a[z];
	const int w2 = reg2aln_band(R.d.qe - R.d.qb, (int)(R.d.re - R.d.rb), R.d.truesc, P.a, P.o_del, P.e_del, P.o_ins, P.e_ins, P.w, R.d.w);
	AlnReq q;
	q.rb = R.d.rb; q.re = R.d.re; q.read = i; q.qb = R.d.qb; q.qe = R.d.qe; q.w2 = w2; q.truesc = R.d.truesc; q.pad = 0;
	reqs[i] = q;
	SamDesc d;
	d.rb = R.d.rb; d.re = R.d.re; d.qb = R.d.qb; d.qe = R.d.qe; d.req = 0; d.rid = R.d.rid;
	d.flag = 0; d.mapq = mapq_se(P, R, ltab, 0) & 0xff; d.score = R.d.score; d.sub = R.sub;
	desc[i] = d;
	status[i] = SE_DECIDED;
}

void launch_se_simple(void *stream, const PairParams &P, int n_reads, const DevReg *d_first, const int *d_nfirst, const uint8_t *d_ok,
                      const uint8_t *d_ann_alt, const double *d_ltab, uint8_t *d_status, AlnReq *d_reqs, SamDesc *d_desc)
{
	if (n_reads <= 0) return;
	hipLaunchKernelGGL(se_simple_kernel, dim3((n_reads + 63) / 64), dim3(64), 0, (hipStream_t)stream, P, n_reads, d_first, d_nfirst, d_ok, d_ann_alt,
	                   d_ltab, d_status, d_reqs, d_desc);
}

} // namespace mbw
