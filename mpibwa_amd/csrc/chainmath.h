// chainmath.h — the arithmetic of mem_chain and of what it calls (test_and_merge, mem_chain_weight, mem_chain_flt), of the contig lookup
// (bns_depos, bns_pos2rid, bns_intv2rid) and of mem_chain2aln's reference window, stated ONCE for the host (host_chain.cpp) and for both
// chaining kernels (chain_kernel.hip: chain_read, a lane per read, and chain_heavy_kernel, a wavefront per read).  Which of the three
// chains a read depends on its seeds, chains, length and the options, and a read that changes hands must keep its SAM line: every
// function keeps the reference's TYPES and ORDER of operations, and the two single-precision compares of mem_chain_flt stand in the
// reference's expression shape with their int-to-float conversions spelled out (the library is built with -ffp-contract=off).
// The functions take scalars, the small POD defined here and accessor callables, never an options, index or chain struct: the host and
// the kernels unpack their own at the call, and keep their own ordered maps, loops and stores.  Results come back through scalars.
// Plain C++ for the host compilers (no HIP header); __host__ __device__ in a HIP translation unit (KS_FN, sortutil.h).
#ifndef MBW_CHAINMATH_H
#define MBW_CHAINMATH_H
#include <cstdint>
#include "sortutil.h"

namespace mbw {

// ---- contigs in the doubled coordinate (src/bntseq.c:349-376, src/bntseq.h:83-86) ----
KS_FN int64_t depos(int64_t l_pac, int64_t pos) { return pos >= l_pac ? (l_pac << 1) - 1 - pos : pos; }

// the contig of a forward-strand position; off(i): where contig i starts
template <class Off>
KS_FN int pos2rid(Off off, int n_seqs, int64_t l_pac, int64_t pos_f)
{
	if (pos_f >= l_pac) return -1;
	int left = 0, mid = 0, right = n_seqs;
	while (left < right) {
		mid = (left + right) >> 1;
		if (pos_f >= off(mid)) {
			if (mid == n_seqs - 1 || pos_f < off(mid + 1)) break;
			left = mid + 1;
		} else right = mid;
	}
	return mid;
}
// the contig of [rb, re): -2 across the strand boundary, -1 across two contigs
template <class Off>
KS_FN int intv2rid(Off off, int n_seqs, int64_t l_pac, int64_t rb, int64_t re)
{
	if (rb < l_pac && re > l_pac) return -2;
	const int rid_b = pos2rid(off, n_seqs, l_pac, depos(l_pac, rb));
	const int rid_e = rb < re ? pos2rid(off, n_seqs, l_pac, depos(l_pac, re - 1)) : rid_b;
	return rid_b == rid_e ? rid_b : -1;
}
// [*beg, *end): the contig at `off` of `len` bases as it lies on the forward or the reverse strand (src/bntseq.c:413-418)
KS_FN void strand_span(int64_t l_pac, int64_t off, int64_t len, bool is_rev, int64_t *beg, int64_t *end)
{
	*beg = is_rev ? (l_pac << 1) - off - len : off;
	*end = is_rev ? (l_pac << 1) - off : off + len;
}

// ---- test_and_merge (src/bwamem.c:190-211) on a chain of the seed's own contig: that test is the caller's ----
enum { MERGE_NEW = 0, MERGE_CONTAINED, MERGE_APPEND };   // the seed opens a chain / lies inside this one and is dropped / becomes its last seed
KS_FN int merge_verdict(int64_t l_pac, int w, int max_chain_gap, int64_t first_r, int first_q, int64_t last_r, int last_q, int last_len,
                        int64_t rb, int qb, int len)
{
	const int64_t qend = last_q + last_len, rend = last_r + last_len;
	if (qb >= first_q && qb + len <= qend && rb >= first_r && rb + len <= rend) return MERGE_CONTAINED;
	if ((last_r < l_pac || first_r < l_pac) && rb >= l_pac) return MERGE_NEW;   // never chain across strands
	const int64_t x = qb - last_q, y = rb - last_r;
	if (y >= 0 && x - y <= w && y - x <= w && x - last_len < max_chain_gap && y - last_len < max_chain_gap) return MERGE_APPEND;
	return MERGE_NEW;
}

// ---- mem_chain_weight (src/bwamem.c:213-237) ----
// one of its two sums: the bases the member seeds cover, add() once per seed in chain order — over the query, and again over the reference
struct CoverSum {
	int64_t end = 0;
	int w = 0;
	KS_FN void add(int64_t beg, int len)
	{
		if (beg >= end) w += len;
		else if (beg + len > end) w += (int)(beg + len - end);
		end = end > beg + len ? end : beg + len;
	}
};
KS_FN int chain_weight_of(int w_query, int w_ref)
{
	const int w = w_ref < w_query ? w_ref : w_query;
	return w < 1 << 30 ? w : (1 << 30) - 1;
}

// ---- mem_chain_flt's pairwise pass (src/bwamem.c:346-362): chain i against the heavier chain j kept before it ----
// [b, e): a chain's span on the query; alt: it lies on an ALT contig
KS_FN bool flt_large_overlap(float mask_level, int max_chain_gap, int bj, int ej, int alt_j, int bi, int ei, int alt_i)
{
	const int b_max = bj > bi ? bj : bi;
	const int e_min = ej < ei ? ej : ei;
	if (!(e_min > b_max && (!alt_j || alt_i))) return false;
	const int li = ei - bi, lj = ej - bj;
	const int min_l = li < lj ? li : lj;
	return (float)(e_min - b_max) >= (float)min_l * mask_level && min_l < max_chain_gap;
}
// ... and, where they overlap that much, whether j ends i's scan: i is dropped
KS_FN bool flt_drops(float drop_ratio, int min_seed_len, int wj, int wi) { return (float)wi < (float)wj * drop_ratio && wj - wi >= min_seed_len << 1; }

// at most max_chain_extend chains with kept = 1 or 2 are extended (:372-379); kept(i): a reference to the flag of chain i in filter order
template <class Kept>
KS_FN void flt_cut_extend(int n, Kept kept, int max_chain_extend)
{
	int i = 0, cnt = 0;
	for (; i < n; ++i) {
		if (kept(i) == 0 || kept(i) == 3) continue;
		if (++cnt >= max_chain_extend) break;
	}
	for (; i < n; ++i)
		if (kept(i) < 3) kept(i) = 0;
}

// ---- the reference window of mem_chain2aln (src/bwamem.c:642-661) ----
// [*b, *e): the widest reference span a seed could reach; lq: the read's length, gap(q): cal_max_gap of q query bases
template <class Gap>
KS_FN void seed_reach(int64_t rbeg, int qbeg, int len, int lq, Gap gap, int64_t *b, int64_t *e)
{
	*b = rbeg - (qbeg + gap(qbeg));
	const int tail = lq - qbeg - len;
	*e = rbeg + len + (tail + gap(tail));
}
// lo, hi: the smallest b and largest e over the chain's seeds; first_r: where its first seed starts; [far_beg, far_end): strand_span of
// its contig, to which bns_fetch_seq clamps
KS_FN void chain_window(int64_t l_pac, int64_t lo, int64_t hi, int64_t first_r, int64_t far_beg, int64_t far_end, int64_t *rmax0, int64_t *rmax1)
{
	int64_t r0 = lo > 0 ? lo : 0;
	int64_t r1 = hi < l_pac << 1 ? hi : l_pac << 1;
	if (r0 < l_pac && l_pac < r1) {   // never cross the strand boundary
		if (first_r < l_pac) r1 = l_pac;
		else r0 = l_pac;
	}
	*rmax0 = r0 > far_beg ? r0 : far_beg;
	*rmax1 = r1 < far_end ? r1 : far_end;
}

} // namespace mbw
#endif
