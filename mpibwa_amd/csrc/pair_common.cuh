// pair_common.cuh — what is device-only of the helpers shared by the pairing kernels (pair_kernel.hip, pair_wave_kernel.hip), the
// single-end decision kernel (se_kernel.hip) and the redundancy kernels (dedup_kernel.hip): the reference's region clean-up and
// primary marking for the short region lists a lane holds, and the single-end MAPQ with the device's tables.
//   mem_sort_dedup_patch  src/bwamem.c:437-489   (dedup_small, with ks_introsort's order for up to 16 elements: sortutil.h)
//   mem_mark_primary_se   src/bwamem.c:493-569   (mark_primary, reads without ALT hits)
//   mem_approx_mapq_se    src/bwamem.c:952-976   (mapq_se; the two short-list kernels pass csub = 0)
// The arithmetic itself — the overlap tests, the hash, the MAPQ expressions, the band — is pairmath.h's, the host's own statement.
#ifndef MBW_PAIR_COMMON_CUH
#define MBW_PAIR_COMMON_CUH
#include <hip/hip_runtime.h>
#include "device.h"
#include "pairmath.h"
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
			if (redundant_overlap(P.mask_level_redun, q->rb, q->re, q->qb, q->qe, p->rb, p->re, p->qb, p->qe)) {   // one of the two is redundant
				if (p->score < q->score) { p->qe = p->qb; break; }
				else q->qe = q->qb;
			} else if (q->rb < p->rb && patch_reg_w(P.l_pac, P.w, q->rb, q->re, q->qb, q->qe, p->rb, p->re, p->qb, p->qe) >= 0)
				return -1;   // mem_patch_reg(q, p) would align
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
// mem_approx_mapq_se (src/bwamem.c:952-976) with the per-length table and PairParams::lnq; l = max(query span, reference span) < P.ltab_n,
// sub_n < 40
__device__ __forceinline__ int mapq_se_of(const PairParams &P, int score, int sub, int sub_n, int csub, int l, float frac_rep, const double *__restrict__ ltab)
{
	return mapq_se_q(score, sub, sub_n, csub, l, frac_rep, P.a, P.b, P.min_seed_len, ltab[l], P.lnq[sub_n]);
}
__device__ __forceinline__ int mapq_se(const PairParams &P, const PReg &r, const double *__restrict__ ltab, int csub)
{
	const int l = r.d.qe - r.d.qb > r.d.re - r.d.rb ? r.d.qe - r.d.qb : (int)(r.d.re - r.d.rb);
	return mapq_se_of(P, r.d.score, r.sub, r.sub_n, csub, l, r.d.frac_rep, ltab);
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
	const int tmp = sub_n_margin(P.a, P.b, P.o_del, P.e_del, P.o_ins, P.e_ins);
	int z[PR_MAXREG], nz = 1;
	z[0] = 0;
	for (int i = 1; i < n; ++i) {
		int k;
		for (k = 0; k < nz; ++k) {
			const int j = z[k];
			if (query_overlap(P.mask_level, a[i].d.qb, a[i].d.qe, a[j].d.qb, a[j].d.qe)) {
				if (a[j].sub == 0) a[j].sub = a[i].d.score;
				if (a[j].d.score - a[i].d.score <= tmp) ++a[j].sub_n;
				break;
			}
		}
		if (k == nz) z[nz++] = i;
		else a[i].secondary = z[k];
	}
	for (int i = 0; i < n; ++i) a[i].secondary_all = a[i].secondary;
}

} // namespace mbw
#endif
