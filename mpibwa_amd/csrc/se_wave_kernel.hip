// se_wave_kernel.hip — the decisions of the single-end branch of worker2 for the reads with up to 64 regions or an XA tag: a read per
// wavefront.
//
// Device counterpart of
//   worker2, single-end branch  src/bwamem.c:1187-1196   (mem_mark_primary_se with id = n_processed + i, then mem_reg2sam)
//   mem_mark_primary_se         src/bwamem.c:493-569     (reads without ALT hits)
//   mem_reg2sam                 src/bwamem.c:1003-1049   (which regions become lines; without MEM_F_ALL)
//   mem_gen_alt                 src/bwamem_extra.c:98-118 (which hits the line's XA string lists: their CIGAR requests; the text is
//                                                          sam_emit_kernel's)
//   mem_approx_mapq_se          src/bwamem.c:952-976     (csub = 0: only mate rescue sets it)
//   mem_reg2aln                 src/bwamem.c:1089-1105   (the band of the final global alignment)
// The reads are the ones se_simple_kernel (se_kernel.hip) leaves with "more than eight regions" or "a secondary region with an XA
// entry".  The host hands over each read's list as it stands after mem_sort_dedup_patch (a fixed point of the pass: there is neither a
// redundancy pass nor a patch alignment here), at most PW_MAXREG regions.  It is pair_wave_kernel (pair_wave_kernel.hip) without the
// rescue replay and without mem_pair: one region per lane, the list in LDS as one array per field, the rank-sort mem_mark_primary_se
// and the XA listing of wave_common.cuh.  A read ends in one record — unmapped, plain, or with an XA tag of 1 .. PW_XA_CAP entries —
// or is left to the host with a code that says why (device.h: SE_HOST_*).  With the side arrays of device.h: SeLines a read whose record
// has 2 .. SE_LINES_CAP lines (a primary line and supplementary lines, src/bwamem.c:1015-1032) is decided too, a lane per line: every
// line's descriptor, MAPQ after the cap of :1029, request and XA requests; sam_lines_kernel.hip writes the text.
//
// 5 120 B of LDS per wave (the list 4 096 B, the sort keys 1 024 B), no scratch; the VGPR count is in DESIGN §4.5d / §4.5e.
// Floating point: as in pair_kernel.hip — the reference's types and order, -ffp-contract=off, the transcendental sites tabulated.
#include <hip/hip_runtime.h>
#include "wave_common.cuh"

namespace mbw {

#define SW_GIVE_UP(code) do { if (lane == 0) wstatus[t] = (uint8_t)(code); return; } while (0)

// work[t]: the read (number in the chunk: id = P.id0 + work[t], reqs.read = work[t]); its list: lists[loff[t] .. loff[t + 1]).
// wstatus[t] = SE_DECIDED: desc[t] and (unless the record is the unmapped one, desc.req = -3) reqs[t] are the read's, as
// se_simple_kernel writes them; SE_DECIDED_XA (xa_reqs given): the same with xa_cnt[t] XA entries, their requests at
// xa_reqs[t * PW_XA_CAP ..] in list order and the count in bits 16-19 of desc[t].flag; every other value: the host's read, nothing
// but wstatus[t] is written.
// LN.desc given: a read with 2 .. SE_LINES_CAP lines (src/bwamem.c:1015-1032) gets SE_DECIDED_LINES instead of SE_HOST_SUPP: LN.n_lines[t]
// lines in list order, line j in slot x = t * SE_LINES_CAP + j of LN.desc / LN.reqs / LN.xa_cnt, its XA requests at
// LN.xa_reqs[x * PW_XA_CAP ..]; desc[t], reqs[t] and xa_cnt[t] are left alone.  (LN.xa_reqs of a read that ends in another code may
// have been written; no count says so.)
__global__ void __launch_bounds__(64)
se_wave_kernel(PairParams P, int n_work, const int *__restrict__ work, const DevReg *__restrict__ lists, const int *__restrict__ loff,
               const uint8_t *__restrict__ ann_alt, const double *__restrict__ ltab, uint8_t *__restrict__ wstatus, AlnReq *__restrict__ reqs,
               SamDesc *__restrict__ desc, AlnReq *__restrict__ xa_reqs, uint8_t *__restrict__ xa_cnt, SeLines LN)
{
	__shared__ WList L;
	__shared__ Pair64 H[PW_MAXREG];
	const int t = blockIdx.x, lane = threadIdx.x;
	if (t >= n_work) return;
	const int k = work[t];
	const int b = loff[t], n = loff[t + 1] - b;
	if (n > PW_MAXREG) SW_GIVE_UP(SE_HOST_FULL);   // (nothing beyond the 64th entry is read: nothing of the list is)
	bool too_long = false, on_alt = false;
	if (lane < n) {
		const DevReg d = lists[b + lane];
		const int l = d.qe - d.qb > d.re - d.rb ? d.qe - d.qb : (int)(d.re - d.rb);
		too_long = l >= P.ltab_n || l <= 0;
		on_alt = ann_alt[d.rid] != 0;
		wl_put(L, lane, wl_from(d));
	}
	if (__ballot(too_long)) SW_GIVE_UP(SE_HOST_LENGTH);
	if (__ballot(on_alt)) SW_GIVE_UP(SE_HOST_ALT);
	__syncthreads();
	if (!pw_mark_primary(P, L, n, P.id0 + (u64)k, H, lane)) SW_GIVE_UP(SE_HOST_TIE);

	// the lines of mem_reg2sam (src/bwamem.c:1015-1037) without MEM_F_ALL: the primary regions of at least T
	const u64 lines = __ballot(lane < n && L.secondary[lane] < 0 && L.score[lane] >= P.T);
	if (!lines) {   // "no alignments good enough": the unaligned record (:1033-1037); XA strings are attached to lines only
		if (lane == 0) {
			SamDesc d;
			d.rb = d.re = 0; d.qb = d.qe = 0; d.req = -3; d.rid = -1;
			d.flag = 0x4; d.mapq = 0; d.score = 0; d.sub = 0;
			desc[t] = d;
			if (xa_cnt) xa_cnt[t] = 0;
			wstatus[t] = SE_DECIDED;
		}
		return;
	}
	if (lines & (lines - 1)) {   // supplementary lines (:1027-1030): SA tags, the MAPQ cap
		const int n_lines = __popcll(lines);
		if (!LN.desc || n_lines > SE_LINES_CAP) SW_GIVE_UP(SE_HOST_SUPP);
		// a lane per line (wave_common.cuh: wave_lines, shared with pair_wave_kernel)
		if (wave_lines<false>(P, LN, L, n, lines, n_lines, k, (size_t)t * SE_LINES_CAP, 0, 0, ltab, lane) < 0) SW_GIVE_UP(SE_HOST_XA);
		if (lane == 0) { LN.n_lines[t] = (uint8_t)n_lines; wstatus[t] = SE_DECIDED_LINES; }
		return;
	}
	const int z = __ffsll((long long)lines) - 1;
	const int n_xa = pw_xa_list(P, L, n, z, k, xa_reqs ? xa_reqs + (size_t)t * PW_XA_CAP : nullptr, lane);
	if (n_xa < 0) SW_GIVE_UP(SE_HOST_XA);
	if (lane == 0) {
		const WReg R = wl_get(L, z);
		const int l = R.qe - R.qb > R.re - R.rb ? R.qe - R.qb : (int)(R.re - R.rb);
		const int w2 = reg2aln_band(R.qe - R.qb, (int)(R.re - R.rb), R.truesc, P.a, P.o_del, P.e_del, P.o_ins, P.e_ins, P.w, R.w);
		AlnReq q;
		q.rb = R.rb; q.re = R.re; q.read = k; q.qb = R.qb; q.qe = R.qe; q.w2 = w2; q.truesc = R.truesc; q.pad = 0;
		reqs[t] = q;
		SamDesc d;
		d.rb = R.rb; d.re = R.re; d.qb = R.qb; d.qe = R.qe; d.req = 0; d.rid = R.rid;
		d.flag = n_xa << SAM_XA_SHIFT; d.mapq = mapq_se_of(P, R.score, R.sub, R.sub_n, 0, l, R.frac_rep, ltab) & 0xff; d.score = R.score; d.sub = R.sub;
		desc[t] = d;
		if (xa_cnt) xa_cnt[t] = (uint8_t)n_xa;
		wstatus[t] = n_xa ? SE_DECIDED_XA : SE_DECIDED;
	}
}

void launch_se_wave(void *stream, const PairParams &P, int n_work, const int *d_work, const DevReg *d_lists, const int *d_loff, const uint8_t *d_ann_alt,
                    const double *d_ltab, uint8_t *d_wstatus, AlnReq *d_reqs, SamDesc *d_desc, AlnReq *d_xa_reqs, uint8_t *d_xa_cnt, const SeLines *lines)
{
	if (n_work <= 0) return;
	if (!d_xa_cnt || !d_xa_reqs || P.max_XA_hits > PW_XA_CAP) d_xa_reqs = nullptr, d_xa_cnt = nullptr;   // (XA listing off)
	SeLines LN;
	if (lines && lines->desc && lines->reqs && lines->n_lines && lines->xa_cnt) LN = *lines;
	if (P.max_XA_hits > PW_XA_CAP) LN.xa_reqs = nullptr;
	hipLaunchKernelGGL(se_wave_kernel, dim3(n_work), dim3(64), 0, (hipStream_t)stream, P, n_work, d_work, d_lists, d_loff, d_ann_alt, d_ltab, d_wstatus,
	                   d_reqs, d_desc, d_xa_reqs, d_xa_cnt, LN);
}

// ---- the units a wave kernel decided, into a CIGAR-and-SAM job of their own: pair_wave_kernel's pairs (ENDS = 2) and this file's reads ----
// dst[t] = first request of work item t's unit in `reqs`, or < 0 (not a unit of the job); per end [the end's request, its XA requests
// (none without xa_cnt)]; desc: chunk-wide, by read.  A thread per work item.
__global__ void wave_desc_clear_kernel(int r0, int n_reads, SamDesc *__restrict__ desc)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_reads) desc[r0 + i].req = -1;
}
template <int ENDS>
__global__ void wave_scatter_kernel(int n_work, const int *__restrict__ work, const int *__restrict__ dst, const AlnReq *__restrict__ w_reqs,
                                    const SamDesc *__restrict__ w_desc, const AlnReq *__restrict__ xa_reqs, const uint8_t *__restrict__ xa_cnt,
                                    AlnReq *__restrict__ reqs, SamDesc *__restrict__ desc)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n_work || dst[t] < 0) return;
	int at = dst[t];
	for (int e = 0; e < ENDS; ++e) {
		const int x = ENDS * t + e;
		const SamDesc d = w_desc[x];
		desc[ENDS * work[t] + e] = d;
		// the unmapped record (se_wave_kernel alone writes one: pair_wave_kernel leaves a pair with an end without a hit to the host): its
		// slot is an unused one (read = -1), as se_simple_kernel leaves it
		if (ENDS == 1 && d.req < 0) {
			AlnReq none;
			none.rb = none.re = 0; none.read = -1; none.qb = none.qe = none.w2 = none.truesc = none.pad = 0;
			reqs[at] = none;
			return;
		}
		reqs[at++] = w_reqs[x];
		if (!xa_cnt) continue;
		const int c = xa_cnt[x] < PW_XA_CAP ? xa_cnt[x] : PW_XA_CAP;
		for (int j = 0; j < c; ++j) reqs[at++] = xa_reqs[(size_t)x * PW_XA_CAP + j];
	}
}
// (ENDS = 2: pair_wave_kernel's pairs reported end by end, the lines of end 0, then those of end 1; an end may have none)
template <int ENDS>
__global__ void lines_scatter_kernel(int n_work, const int *__restrict__ dst, const uint8_t *__restrict__ n_lines, const AlnReq *__restrict__ lreq,
                                     const uint8_t *__restrict__ lxcnt, const AlnReq *__restrict__ lxreq, AlnReq *__restrict__ reqs)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n_work || dst[t] < 0) return;
	int at = dst[t];
	for (int e = 0; e < ENDS; ++e) {
		const size_t l = (size_t)ENDS * t + e;
		const int nl = n_lines[l] < SE_LINES_CAP ? n_lines[l] : SE_LINES_CAP;
		for (int j = 0; j < nl; ++j) {
			const size_t x = l * SE_LINES_CAP + j;
			reqs[at++] = lreq[x];
			const int c = lxcnt[x] < PW_XA_CAP ? lxcnt[x] : PW_XA_CAP;
			for (int i = 0; i < c; ++i) reqs[at++] = lxreq[x * PW_XA_CAP + i];
		}
	}
}
void launch_lines_job_scatter(void *stream, int ends, int n_work, const int *d_dst, const uint8_t *d_n_lines, const AlnReq *d_lreq, const uint8_t *d_lxcnt,
                              const AlnReq *d_lxreq, AlnReq *d_reqs)
{
	if (n_work > 0)
		hipLaunchKernelGGL(ends == 2 ? lines_scatter_kernel<2> : lines_scatter_kernel<1>, dim3((n_work + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_work, d_dst, d_n_lines, d_lreq, d_lxcnt, d_lxreq,
		                   d_reqs);
}
void launch_wave_job_scatter(void *stream, int ends, int n_work, const int *d_work, const int *d_dst, const AlnReq *d_w_reqs, const SamDesc *d_w_desc,
                             const AlnReq *d_xa_reqs, const uint8_t *d_xa_cnt, AlnReq *d_reqs, SamDesc *d_desc, int clear_r0, int clear_n)
{
	if (clear_n > 0) hipLaunchKernelGGL(wave_desc_clear_kernel, dim3((clear_n + 255) / 256), dim3(256), 0, (hipStream_t)stream, clear_r0, clear_n, d_desc);
	if (n_work > 0)
		hipLaunchKernelGGL(ends == 2 ? wave_scatter_kernel<2> : wave_scatter_kernel<1>, dim3((n_work + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_work,
		                   d_work, d_dst, d_w_reqs, d_w_desc, d_xa_reqs, d_xa_cnt, d_reqs, d_desc);
}

} // namespace mbw
