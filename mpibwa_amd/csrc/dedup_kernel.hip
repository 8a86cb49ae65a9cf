// dedup_kernel.hip — the redundancy pass of mem_sort_dedup_patch (src/bwamem.c:437-489) on the raw region lists of a sub-batch, behind
// reg_pack and first_reg on the lane's stream.  The result is a permutation, not moved records: per read the places, in its raw list, of
// the regions the reference keeps, in the reference's final order.  A read for which the reference would go on to mem_patch_reg's
// global alignment (:406-435: two regions that pass its cheap tests :411-423) is declined, and the host runs its own pass on it.
//
//  * reads with up to PR_MAXREG regions: a lane per read, dedup_small (pair_common.cuh) unchanged — the raw place of a region rides in
//    DevReg::pad, which the pass copies with the record and never reads (dedup_small_kernel).  The same launch lists the longer reads;
//  * reads with PR_MAXREG + 1 .. DD_MAXREG regions: a read per wavefront over that list (dedup_wave_kernel).  What the pass reads of a
//    region lives in LDS as structure-of-arrays at the region's raw place — rb, re (8 bytes each), qb, qe, rid, score (4 each), an alive
//    byte — with a 16-bit order array: 17.7 KB per workgroup of one wavefront, 9 workgroups per CU by LDS.
//      - both sorts are ks_introsort on the order array (sortutil.h, its frame stack in LDS), lane 0: its order of equal keys shows in
//        the result (equal `re` in the first sort; which of two (score, rb, qb)-equal hits is dropped after the second);
//      - the scan is serial in i and lane-parallel in j.  For p = a[i] the inner loop of :451-474 visits the contiguous run
//        J = {j < i : same rid, p.rb < a[j].re + max_chain_gap}, ending at the first j that fails whatever the alive marks say; p is
//        alive at its turn (only earlier elements are ever marked) and unchanged until it dies.  So, a lane per j: R[j] = alive and
//        redundant (:459); stop = the largest j with R[j] and p.score < a[j].score (there the reference marks p and breaks); every j > stop
//        with R[j] is marked; an alive, not redundant j > stop with a[j].rb < p.rb that passes mem_patch_reg's cheap tests declines the
//        read.  A marked region is never read again by the reference (q: `continue`; p: `break`), so the mark is a byte and qe stays;
//      - the compactions and the adjacent (score, rb, qb) test of :482-484 — which reads only fields the marking does not change — are
//        ballot arithmetic; the first element of the last compaction is always kept.
//    Every trip count is wave-uniform (ballot results, n) and bounded by n; ballots stand outside divergent code.  No
//    persistent loop, no work counter: a grid-stride walk over the list.
// Floating point: the reference's expression (int64 against float * int64) in its types and order, as pairmath.h states it for the host too.
#include <hip/hip_runtime.h>
#include "hip_util.h"
#include "pair_common.cuh"
#include "sortutil.h"

namespace mbw {

#define DSORT_FRAMES 16

extern "C" int mi355x_dedup_maxreg(void) { return DD_MAXREG; }

DedupParams dedup_params(const mem_opt_t *opt, int64_t l_pac)
{
	DedupParams D;
	D.l_pac = l_pac; D.max_chain_gap = opt->max_chain_gap; D.w = opt->w; D.mask_level_redun = opt->mask_level_redun; D.pad = 0;
	return D;
}

namespace {

__global__ void __launch_bounds__(64)
dedup_small_kernel(DedupParams D, int n_reads, const DevReg *__restrict__ packed, const int *__restrict__ reg_pos, const int *__restrict__ nregs,
                   uint8_t *__restrict__ status, int *__restrict__ m_out, int *__restrict__ keep, int *__restrict__ list, unsigned int *__restrict__ count)
{
	const int i = blockIdx.x * 64 + threadIdx.x;
	const int n = i < n_reads ? nregs[i] : 0;
	// the reads of dedup_wave_kernel, listed the way chain_pick_kernel lists (one atomic per wavefront)
	const bool wave_read = n > PR_MAXREG && n <= DD_MAXREG;
	const unsigned long long wm = __ballot(wave_read);
	const int lane = threadIdx.x & 63, lead = wm ? __ffsll((long long)wm) - 1 : 0;
	unsigned int at = 0;
	if (wm && lane == lead) at = atomicAdd(count, (unsigned int)__popcll(wm));
	at = __shfl(at, lead) + (unsigned int)__popcll(wm & ((1ull << lane) - 1));
	if (i >= n_reads) return;
	if (wave_read) {
		list[at] = i;   // (at < n_reads: every read is listed at most once)
		status[i] = DD_HOST; m_out[i] = -1;
		return;
	}
	if (n > DD_MAXREG) { status[i] = DD_HOST_MAXREG; m_out[i] = -1; return; }
	const int base = reg_pos[i];
	if (n <= 1) {
		if (n == 1) keep[base] = 0;
		status[i] = DD_TAKEN; m_out[i] = n > 0 ? n : 0;
		return;
	}
	DevReg r[PR_MAXREG];
	for (int j = 0; j < n; ++j) { r[j] = packed[(size_t)base + j]; r[j].pad = j; }
	PairParams P;   // (what dedup_small reads of it)
	P.l_pac = D.l_pac; P.max_chain_gap = D.max_chain_gap; P.w = D.w; P.mask_level_redun = D.mask_level_redun;
	const int m = dedup_small(P, r, n);
	if (m < 0) { status[i] = DD_HOST_PATCH; m_out[i] = -1; return; }
	for (int k = 0; k < m; ++k) keep[base + k] = r[k].pad;
	status[i] = DD_TAKEN; m_out[i] = m;
}

__global__ void __launch_bounds__(64)
dedup_wave_kernel(DedupParams D, const int *__restrict__ list, const unsigned int *__restrict__ list_n, int list_cap, const DevReg *__restrict__ packed,
                  const int *__restrict__ reg_pos, const int *__restrict__ nregs, uint8_t *__restrict__ status, int *__restrict__ m_out,
                  int *__restrict__ keep)
{
	__shared__ i64 s_rb[DD_MAXREG], s_re[DD_MAXREG];
	__shared__ int s_qb[DD_MAXREG], s_qe[DD_MAXREG], s_rid[DD_MAXREG], s_sc[DD_MAXREG];
	__shared__ unsigned short s_ord[DD_MAXREG];
	__shared__ unsigned char s_alive[DD_MAXREG];
	__shared__ int s_stk[3 * DSORT_FRAMES];   // the sorts' frames, 16 per array, in LDS as before (private arrays were not tried in this kernel)
	static_assert(DD_MAXREG <= 16 << DSORT_FRAMES, "ks_introsort_at: n <= 16 << FRAMES");
	const KsFramesAt frames = {s_stk, s_stk + DSORT_FRAMES, s_stk + 2 * DSORT_FRAMES};
	auto ord_at = [&](int k) -> unsigned short & { return s_ord[k]; };
	const int lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1;
	unsigned int cnt = *list_n;
	if (cnt > (unsigned int)list_cap) cnt = (unsigned int)list_cap;
	for (unsigned int t = blockIdx.x; t < cnt; t += gridDim.x) {
		const int rd = list[t];
		int n = nregs[rd];
		if (n > DD_MAXREG) n = DD_MAXREG;   // (never: the list holds the reads up to the cap)
		const int base = reg_pos[rd];
		__syncthreads();   // the previous read's arrays are done with
		for (int k = lane; k < n; k += 64) {
			const DevReg g = packed[(size_t)base + k];
			s_rb[k] = g.rb; s_re[k] = g.re; s_qb[k] = g.qb; s_qe[k] = g.qe; s_rid[k] = g.rid; s_sc[k] = g.score;
			s_alive[k] = g.qe > g.qb;
			s_ord[k] = (unsigned short)k;
		}
		__syncthreads();
		if (lane == 0) ks_introsort_at(n, ord_at, frames, [&](int x, int y) { return s_re[x] < s_re[y]; });   // by END position
		__syncthreads();
		bool declined = false;
		for (int i = 1; i < n && !declined; ++i) {
			const int pi = s_ord[i];
			const i64 p_rb = s_rb[pi], p_re = s_re[pi];
			const int p_qb = s_qb[pi], p_qe = s_qe[pi], p_rid = s_rid[pi], p_sc = s_sc[pi];
			bool p_dies = false;
			for (int top = i - 1; top >= 0; top -= 64) {
				const int j = top - lane;
				const int qi = j >= 0 ? s_ord[j] : 0;
				const i64 q_rb = s_rb[qi], q_re = s_re[qi];
				const int q_qb = s_qb[qi], q_qe = s_qe[qi], q_sc = s_sc[qi];
				const bool in_loop = j >= 0 && s_rid[qi] == p_rid && p_rb < q_re + D.max_chain_gap;
				const unsigned long long fail = __ballot(!in_loop);
				const unsigned long long run = fail ? (1ull << (__ffsll((long long)fail) - 1)) - 1 : ~0ull;   // the lanes before the first that fails
				const bool alive = ((run >> lane) & 1) && s_alive[qi];
				const bool redun = alive && redundant_overlap(D.mask_level_redun, q_rb, q_re, q_qb, q_qe, p_rb, p_re, p_qb, p_qe);
				const unsigned long long stop = __ballot(redun && p_sc < q_sc);
				const unsigned long long vis = stop ? (1ull << (__ffsll((long long)stop) - 1)) - 1 : run;   // visited before the break
				const bool visited = (vis >> lane) & 1;
				const bool patch = visited && alive && !redun && q_rb < p_rb && patch_reg_w(D.l_pac, D.w, q_rb, q_re, q_qb, q_qe, p_rb, p_re, p_qb, p_qe) >= 0;
				if (__ballot(patch)) { declined = true; break; }
				if (visited && redun) s_alive[qi] = 0;
				if (stop) { p_dies = true; break; }
				if (fail) break;
			}
			if (p_dies && lane == 0) s_alive[pi] = 0;
			__syncthreads();
		}
		if (declined) {
			if (lane == 0) { status[rd] = DD_HOST_PATCH; m_out[rd] = -1; }
			continue;
		}
		// the survivors, still in the order of the first sort
		int m1 = 0;
		for (int c = 0; c < n; c += 64) {
			const int k = c + lane;
			const int v = k < n ? s_ord[k] : 0;
			const bool a = k < n && s_alive[v];
			const unsigned long long mk = __ballot(a);
			__syncthreads();   // (the chunk is in registers before its part of the array is overwritten)
			if (a) s_ord[m1 + __popcll(mk & below)] = (unsigned short)v;
			m1 += __popcll(mk);
		}
		__syncthreads();
		if (lane == 0)
			ks_introsort_at(m1, ord_at, frames, [&](int x, int y) {   // by score, then position
				return s_sc[x] > s_sc[y] || (s_sc[x] == s_sc[y] && (s_rb[x] < s_rb[y] || (s_rb[x] == s_rb[y] && s_qb[x] < s_qb[y])));
			});
		__syncthreads();
		// an element equal to its predecessor in (score, rb, qb) goes (:482-484); the first one always stays
		int m2 = 0;
		for (int c = 0; c < m1; c += 64) {
			const int k = c + lane;
			const int v = k < m1 ? s_ord[k] : 0, u = k > 0 && k < m1 ? s_ord[k - 1] : 0;
			const bool a = k < m1 && !(k > 0 && s_sc[v] == s_sc[u] && s_rb[v] == s_rb[u] && s_qb[v] == s_qb[u]);
			const unsigned long long mk = __ballot(a);
			if (a) keep[base + m2 + __popcll(mk & below)] = v;
			m2 += __popcll(mk);
		}
		if (lane == 0) { status[rd] = DD_TAKEN; m_out[rd] = m2; }
	}
}

} // namespace

void launch_dedup(void *stream, const DedupParams &D, int n_reads, const DevReg *d_packed, const int *d_reg_pos, const int *d_nregs, uint8_t *d_status,
                  int *d_m, int *d_keep, int *d_list)
{
	if (n_reads <= 0) return;
	hipStream_t st = (hipStream_t)stream;
	unsigned int *d_count = (unsigned int *)(d_list + n_reads);
	HIP_OK(hipMemsetAsync(d_count, 0, 4, st));
	hipLaunchKernelGGL(dedup_small_kernel, dim3((n_reads + 63) / 64), dim3(64), 0, st, D, n_reads, d_packed, d_reg_pos, d_nregs, d_status, d_m, d_keep, d_list,
	                   d_count);
	// a read per wavefront over the list: as many workgroups as the chip holds at 17.7 KB of LDS each, and no more than there can be reads
	const int waves = n_reads < 2048 ? n_reads : 2048;
	hipLaunchKernelGGL(dedup_wave_kernel, dim3(waves), dim3(64), 0, st, D, (const int *)d_list, (const unsigned int *)d_count, n_reads, d_packed, d_reg_pos,
	                   d_nregs, d_status, d_m, d_keep);
	HIP_OK(hipGetLastError());
}

} // namespace mbw
