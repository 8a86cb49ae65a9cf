// pair_common.cuh — device helpers shared by the pairing kernel (pair_kernel.hip) and the single-end decision kernel
// (se_kernel.hip): the reference's region clean-up, primary marking and single-end MAPQ for the short region lists both look at.
//   mem_sort_dedup_patch  src/bwamem.c:437-489   (dedup_small, with ks_introsort's order for up to 16 elements: sortutil.h)
//   mem_mark_primary_se   src/bwamem.c:493-569   (mark_primary, reads without ALT hits; hash_64: src/utils.h:98-109)
//   mem_approx_mapq_se    src/bwamem.c:952-976   (mapq_se; the two short-list kernels pass csub = 0)
//   infer_bw              src/bwamem.c:792-800   (the band of mem_reg2aln's global alignment)
// Floating point: the expressions are evaluated in the reference's types and order (the library is built with -ffp-contract=off).
#ifndef MBW_PAIR_COMMON_CUH
#define MBW_PAIR_COMMON_CUH
#include <hip/hip_runtime.h>
#include "device.h"
#include "sortutil.h"

namespace mbw {

typedef long long i64;
typedef unsigned long long u64;


// mem_sort_dedup_patch (src/bwamem.c:437-489) for n <= PR_MAXREG regions of one read.  Returns the number of regions left, or -1 when two regions pass the
// cheap tests of mem_patch_reg (:411-423) and the reference would go on to align across them (the host's case).
// The sorts are ks_introsort's small form (sortutil.h) over an order array: `o` holds the element numbers, lt compares two of them.
static_assert(PR_MAXREG <= 16, "ks_small_introsort_at is ks_introsort for at most 16 elements");
template <class LT>
__device__ __forceinline__ void sort_regs(int n, DevReg *a, LT lt)
{
	int o[PR_MAXREG];
	DevReg t[PR_MAXREG];
	for (int i = 0; i < n; ++i) { o[i] = i; t[i] = a[i]; }
	ks_small_introsort_at(n, [&](int k) -> int & { return o[k]; }, [&](int x, int y) { return lt(t[x], t[y]); });
	for (int i = 0; i < n; ++i) a[i] = t[o[i]];
}

__device__ __forceinline__ int dedup_small(const PairParams &P, DevReg *a, int n)
{
	if (n <= 1) return n;
	sort_regs(n, a, [](const DevReg &x, const DevReg &y) { return x.re < y.re; });   // by END position
	for (int i = 1; i < n; ++i) {
		DevReg *p = &a[i];
		if (p->rid != a[i - 1].rid || p->rb >= a[i - 1].re + P.max_chain_gap) continue;
		for (int j = i - 1; j >= 0 && p->rid == a[j].rid && p->rb < a[j].re + P.max_chain_gap; --j) {
			DevReg *q = &a[j];
			if (q->qe == q->qb) continue;   // already excluded
			const i64 orr = q->re - p->rb;
			const i64 oq = q->qb < p->qb ? q->qe - p->qb : p->qe - q->qb;
			const i64 mr = q->re - q->rb < p->re - p->rb ? q->re - q->rb : p->re - p->rb;
			const i64 mq = q->qe - q->qb < p->qe - p->qb ? q->qe - q->qb : p->qe - p->qb;
			if (orr > P.mask_level_redun * mr && oq > P.mask_level_redun * mq) {   // one of the two is redundant
				if (p->score < q->score) { p->qe = p->qb; break; }
				else q->qe = q->qb;
			} else if (q->rb < p->rb) {   // mem_patch_reg(q, p): would it align?
				const DevReg *x = q, *y = p;
				if (x->rb < P.l_pac && y->rb >= P.l_pac) continue;
				if (x->qb >= y->qb || x->qe >= y->qe || x->re >= y->re) continue;   // not colinear
				int w = (int)((x->re - y->rb) - (x->qe - y->qb));
				w = w > 0 ? w : -w;
				double r = (double)(x->re - y->rb) / (y->re - x->rb) - (double)(x->qe - y->qb) / (y->qe - x->qb);
				r = r > 0. ? r : -r;
				if (x->re < y->rb || x->qe < y->qb) {
					if (w > P.w << 1 || r >= 0.05f) continue;
				} else if (w > P.w << 2 || r >= 0.05f * 2) continue;
				return -1;
			}
		}
	}
	int m = 0;
	for (int i = 0; i < n; ++i)
		if (a[i].qe > a[i].qb) { if (m != i) a[m] = a[i]; ++m; }
	n = m;
	sort_regs(n, a, [](const DevReg &x, const DevReg &y) {   // by score, then position
		return x.score > y.score || (x.score == y.score && (x.rb < y.rb || (x.rb == y.rb && x.qb < y.qb)));
	});
	for (int i = 1; i < n; ++i)
		if (a[i].score == a[i - 1].score && a[i].rb == a[i - 1].rb && a[i].qb == a[i - 1].qb) a[i].qe = a[i].qb;
	m = n > 0 ? 1 : 0;
	for (int i = 1; i < n; ++i)
		if (a[i].qe > a[i].qb) { if (m != i) a[m] = a[i]; ++m; }
	return m;
}

// a region with the fields the pairing stage adds to it (mem_alnreg_t: sub, sub_n, secondary, secondary_all, hash)
struct PReg {
	DevReg d;
	int sub, sub_n, secondary, secondary_all;
	u64 hash;
};
__device__ __forceinline__ u64 hash_64(u64 key)   // src/utils.h:98-109
{
	key += ~(key << 32); key ^= (key >> 22); key += ~(key << 13); key ^= (key >> 8);
	key += (key << 3);   key ^= (key >> 15); key += ~(key << 27); key ^= (key >> 31);
	return key;
}
#define RAW_MAPQ(diff, a) ((int)(6.02 * (diff) / (a) + .499))
// mem_approx_mapq_se (src/bwamem.c:952-976); l = max(query span, reference span); csub: the score of a tandem copy (a hit that comes from
// mate rescue carries one, src/bwamem_pair.c:163; 0 for every other hit)
__device__ __forceinline__ int mapq_se_of(const PairParams &P, int score, int sub_, int sub_n, int csub, int l, float frac_rep, const double *__restrict__ ltab)
{
	int sub = sub_ ? sub_ : P.min_seed_len * P.a;
	sub = csub > sub ? csub : sub;
	if (sub >= score) return 0;
	const double identity = 1. - (double)(l * P.a - score) / (P.a + P.b) / l;
	int mapq;
	if (score == 0) mapq = 0;
	else {
		double tmp = ltab[l];
		tmp *= identity * identity;
		mapq = (int)(6.02 * (score - sub) / P.a * tmp * tmp + .499);
	}
	if (sub_n > 0) mapq -= P.lnq[sub_n];
	if (mapq > 60) mapq = 60;
	if (mapq < 0) mapq = 0;
	mapq = (int)(mapq * (1. - frac_rep) + .499);
	return mapq;
}
__device__ __forceinline__ int mapq_se(const PairParams &P, const PReg &r, const double *__restrict__ ltab, int csub)
{
	const int l = r.d.qe - r.d.qb > r.d.re - r.d.rb ? r.d.qe - r.d.qb : (int)(r.d.re - r.d.rb);
	return mapq_se_of(P, r.d.score, r.sub, r.sub_n, csub, l, r.d.frac_rep, ltab);
}
__device__ __forceinline__ int infer_bw(int l1, int l2, int score, int a, int q, int r)
{
	if (l1 == l2 && l1 * a - score < (q + r - a) << 1) return 0;
	int w = (int)((double)((l1 < l2 ? l1 : l2) * a - score - q) / r + 2.);
	const int d = l1 > l2 ? l1 - l2 : l2 - l1;
	if (w < d) w = d;
	return w;
}
// mem_mark_primary_se (src/bwamem.c:521-569) for a read without ALT hits; mem_mark_primary_se_core :493-519
__device__ __forceinline__ void mark_primary(const PairParams &P, PReg *a, int n, u64 id)
{
	for (int i = 0; i < n; ++i) { a[i].sub = 0; a[i].secondary = a[i].secondary_all = -1; a[i].hash = hash_64(id + i); }
	{
		int o[PR_MAXREG];
		PReg t[PR_MAXREG];
		for (int i = 0; i < n; ++i) { o[i] = i; t[i] = a[i]; }
		ks_small_introsort_at(n, [&](int k) -> int & { return o[k]; }, [&](int x, int y) { return t[x].d.score > t[y].d.score || (t[x].d.score == t[y].d.score && t[x].hash < t[y].hash); });
		for (int i = 0; i < n; ++i) a[i] = t[o[i]];
	}
	int tmp = P.a + P.b;
	tmp = P.o_del + P.e_del > tmp ? P.o_del + P.e_del : tmp;
	tmp = P.o_ins + P.e_ins > tmp ? P.o_ins + P.e_ins : tmp;
	int z[PR_MAXREG], nz = 1;
	z[0] = 0;
	for (int i = 1; i < n; ++i) {
		int k;
		for (k = 0; k < nz; ++k) {
			const int j = z[k];
			const int b_max = a[j].d.qb > a[i].d.qb ? a[j].d.qb : a[i].d.qb;
			const int e_min = a[j].d.qe < a[i].d.qe ? a[j].d.qe : a[i].d.qe;
			if (e_min > b_max) {
				const int min_l = a[i].d.qe - a[i].d.qb < a[j].d.qe - a[j].d.qb ? a[i].d.qe - a[i].d.qb : a[j].d.qe - a[j].d.qb;
				if (e_min - b_max >= min_l * P.mask_level) {   // significant overlap on the query
					if (a[j].sub == 0) a[j].sub = a[i].d.score;
					if (a[j].d.score - a[i].d.score <= tmp) ++a[j].sub_n;
					break;
				}
			}
		}
		if (k == nz) z[nz++] = i;
		else a[i].secondary = z[k];
	}
	for (int i = 0; i < n; ++i) a[i].secondary_all = a[i].secondary;
}

} // namespace mbw
#endif
