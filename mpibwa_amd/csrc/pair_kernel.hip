// pair_kernel.hip — the pairing decisions of mem_sam_pe for the pairs that need none of its machinery, a pair per lane.
//
// Device counterpart, for ONE shape of pair, of
//   mem_sam_pe            src/bwamem_pair.c:250-393   (rescue loop, primary marking, pairing, MAPQ, the two records)
//   mem_matesw            src/bwamem_pair.c:111-128   (only its test "is every orientation already explained or failed?")
//   mem_pair              src/bwamem_pair.c:182-243   (one hit per end: one candidate pair)
//   mem_approx_mapq_se    src/bwamem.c:952-976
//   mem_reg2aln           src/bwamem.c:1089-1105      (the band of the final global alignment: infer_bw, :792-800)
//   mem_sort_dedup_patch  src/bwamem.c:437-489        (up to PR_MAXREG = 8 regions per end, as long as no two of them get as far as
//                                                       mem_patch_reg's global alignment, :406-435)
//   mem_mark_primary_se   src/bwamem.c:493-569        (reads without ALT hits)
// The shape: each end has at most PR_MAXREG = 8 regions (typically the hit and a few 19-25 bp chance matches), none on an ALT
// contig, and the two ends give at most PR_MAXPAIR = 16 candidate pairs; mem_matesw would return without aligning for every candidate hit; mem_pair finds a pair; no end has a second
// good primary hit (the single-end logic's case) and no secondary hit is close enough to its primary for an XA entry
// (src/bwamem_extra.c:91-110).  The unstable sorts (ks_introsort) and the hash tie-breaks are the reference's.  That is the bulk of a chunk (three pairs in four on the bench
// workload).  For such a pair the kernel writes what the host's COLLECT pass would have produced — the two requests for
// aln_kernel and the two line descriptors for sam_emit_kernel — so its SAM records are made without the host touching the
// pair at all; every other pair is left to the host (status 0) with its full logic.
//
// Floating point: the reference decides in double (and two float adds).  The expressions are evaluated here in the same
// types and order (the library is built with -ffp-contract=off, IEEE division); the two transcendental sites are host-built
// tables: the double term of a candidate pair's score per insert size and orientation (src/bwamem_pair.c:218-219, pair_score_term), and
// mapQ_coef_fac / log(l) per length (src/bwamem.c:964).
#include <hip/hip_runtime.h>
#include "pair_common.cuh"

namespace mbw {

// per read: its first PR_MAXREG regions and how many it has
__global__ void first_reg_kernel(int n, const int *__restrict__ reg_pos, const int *__restrict__ nregs, const DevReg *__restrict__ packed,
                                 DevReg *__restrict__ first, int *__restrict__ nfirst)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int m = nregs[i];
	nfirst[i] = m;
	for (int j = 0; j < m && j < PR_MAXREG; ++j) first[(size_t)i * PR_MAXREG + j] = packed[reg_pos[i] + j];
}
void launch_first_reg(void *stream, int n, const int *d_reg_pos, const int *d_nregs, const DevReg *d_packed, DevReg *d_first, int *d_nfirst)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(first_reg_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_reg_pos, d_nregs, d_packed, d_first, d_nfirst);
}

// true when mem_matesw(hit, the mate's hits) returns at once: every orientation failed or explained by a mate hit (:118-128)
__device__ __forceinline__ bool no_rescue_needed(const PairParams &P, const DevReg &hit, const PReg *ma, int n_ma)
{
	int skip[4];
	for (int r = 0; r < 4; ++r) skip[r] = P.failed[r] ? 1 : 0;
	for (int i = 0; i < n_ma; ++i) {
		int64_t dist;
		const int r = infer_dir(P.l_pac, hit.rb, ma[i].d.rb, &dist);
		if (dist >= P.low[r] && dist <= P.high[r]) skip[r] = 1;
	}
	return skip[0] + skip[1] + skip[2] + skip[3] == 4;
}

#define PR_MAXPAIR 16
template <int CAP>
__device__ __forceinline__ void sort_pairs(int n, Pair64 *v)
{
	static_assert(CAP <= 16, "ks_small_introsort_at is ks_introsort for at most 16 elements");
	int o[CAP];
	Pair64 t[CAP];
	for (int i = 0; i < n; ++i) { o[i] = i; t[i] = v[i]; }
	ks_small_introsort_at(n, [&](int k) -> int & { return o[k]; }, [&](int x, int y) { return pair_lt(t[x], t[y]); });
	for (int i = 0; i < n; ++i) v[i] = t[o[i]];
}

// status[k]: PR_DECIDED = decided here; else the host's pair (device.h: PR_HOST_* says which test sent it there)
__global__ void __launch_bounds__(64)
pair_simple_kernel(PairParams P, int n_pairs, const DevReg *__restrict__ first, const int *__restrict__ nfirst, const uint8_t *__restrict__ pair_ok,
                   const i64 *__restrict__ ann_off, const uint8_t *__restrict__ ann_alt, const double *__restrict__ ptab, const double *__restrict__ ltab,
                   uint8_t *__restrict__ status, AlnReq *__restrict__ reqs, SamDesc *__restrict__ desc)
{
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n_pairs) return;
	AlnReq none;
	none.rb = none.re = 0; none.read = -1; none.qb = none.qe = none.w2 = none.truesc = none.pad = 0;
	reqs[2 * k] = none; reqs[2 * k + 1] = none;
	desc[2 * k].req = -1; desc[2 * k + 1].req = -1;
	status[k] = PR_HOST;
	int n[2] = {nfirst[2 * k], nfirst[2 * k + 1]};
	if (!pair_ok[k]) { status[k] = PR_HOST_NO_HIT; return; }
	if (n[0] == 0 && n[1] == 0) {   // no hit on either end: the two "unmapped" records need no decision at all (src/bwamem_pair.c:363-391, flags 77 / 141)
		for (int e = 0; e < 2; ++e) {
			SamDesc d;
			d.rb = d.re = 0; d.qb = d.qe = 0; d.req = -3; d.rid = -1;
			d.flag = 0x1 | 0x4 | 0x8 | 0x40 << e; d.mapq = 0; d.score = 0; d.sub = 0;
			desc[2 * k + e] = d;
		}
		status[k] = PR_DECIDED;
		return;
	}
	if (n[0] < 1 || n[1] < 1) { status[k] = PR_HOST_NO_HIT; return; }
	if (n[0] > PR_MAXREG || n[1] > PR_MAXREG) { status[k] = PR_HOST_MAXREG; return; }
	PReg a[2][PR_MAXREG];
	for (int e = 0; e < 2; ++e) {
		DevReg r[PR_MAXREG];
		for (int j = 0; j < n[e]; ++j) r[j] = first[(size_t)(2 * k + e) * PR_MAXREG + j];
		n[e] = dedup_small(P, r, n[e]);
		if (n[e] < 0) { status[k] = PR_HOST_PATCH; return; }   // two hits the host has to try to patch
		for (int j = 0; j < n[e]; ++j) {
			a[e][j].d = r[j]; a[e][j].sub = a[e][j].sub_n = 0; a[e][j].secondary = a[e][j].secondary_all = -1; a[e][j].hash = 0;
			if (ann_alt[r[j].rid]) { status[k] = PR_HOST_LENGTH; return; }
			const int l = r[j].qe - r[j].qb > r[j].re - r[j].rb ? r[j].qe - r[j].qb : (int)(r[j].re - r[j].rb);
			if (l >= P.ltab_n || l <= 0) { status[k] = PR_HOST_LENGTH; return; }
		}
	}
	// the rescue loop would not align anything (src/bwamem_pair.c:263-272): every candidate hit is explained by the mate's hits
	if (!P.no_rescue)
		for (int e = 0; e < 2; ++e) {
			int nb = 0;
			for (int j = 0; j < n[e] && nb < P.max_matesw; ++j) {
				if (a[e][j].d.score < a[e][0].d.score - P.pen_unpaired) continue;
				++nb;
				if (!no_rescue_needed(P, a[e][j].d, a[!e], n[!e])) { status[k] = PR_HOST_RESCUE; return; }
			}
		}
	const u64 id = P.id0 + (u64)k;
	mark_primary(P, a[0], n[0], id << 1 | 0);
	mark_primary(P, a[1], n[1], id << 1 | 1);
	// mem_pair (src/bwamem_pair.c:182-243)
	Pair64 v[2 * PR_MAXREG], u[PR_MAXPAIR];
	int nv = 0, nu = 0;
	for (int r = 0; r < 2; ++r)
		for (int i = 0; i < n[r]; ++i) {
			const DevReg &e = a[r][i].d;
			v[nv++] = pair_key(P.l_pac, e.rb, e.rid, ann_off[e.rid], e.score, i, r);
		}
	sort_pairs<2 * PR_MAXREG>(nv, v);
	int y[4] = {-1, -1, -1, -1};
	const int idi = pair_id_mix(id);
	for (int i = 0; i < nv; ++i) {   // (y[which]: the last key of that kind before i, -1 = none: nothing is scanned)
		pair_candidates_of(v, i, P.low, P.high, P.failed, idi, [&](int which) { return y[which]; },
		                   [&](int dir, i64 dist) { return ptab[P.tab_off[dir] + (int)(dist - P.low[dir])]; }, [&](const Pair64 &p) {
			if (nu < PR_MAXPAIR) u[nu] = p;
			++nu;
		});
		y[v[i].y & 3] = i;
	}
	if (nu > PR_MAXPAIR) { status[k] = PR_HOST_MAXREG; return; }   // (ks_small_introsort_at: at most 16 elements)
	if (nu == 0) { status[k] = PR_HOST_NO_PAIR; return; }   // no pair in a proper orientation and distance: the host reports the ends independently
	const int tmp = sub_n_margin(P.a, P.b, P.o_del, P.e_del, P.o_ins, P.e_ins);
	sort_pairs<PR_MAXPAIR>(nu, u);
	int z[2];
	{
		const int i = (int)(u[nu - 1].y >> 32), kk = (int)(u[nu - 1].y << 32 >> 32);
		z[v[i].y & 1] = (int)(v[i].y << 32 >> 34);
		z[v[kk].y & 1] = (int)(v[kk].y << 32 >> 34);
	}
	const int o = (int)(u[nu - 1].x >> 32);
	int subo = nu > 1 ? (int)(u[nu - 2].x >> 32) : 0, n_sub = 0;
	for (int j = nu - 2; j >= 0; --j)
		if (subo - (int)(u[j].x >> 32) <= tmp) ++n_sub;
	if (o <= 0) { status[k] = PR_HOST_SCORE; return; }
	for (int e = 0; e < 2; ++e)   // an end with several good primary hits is left to the single-end logic (src/bwamem_pair.c:303-309)
		for (int j = 1; j < n[e]; ++j)
			if (a[e][j].secondary < 0 && a[e][j].d.score >= P.T) { status[k] = PR_HOST_SUPP; return; }
	const int score_un = a[0][0].d.score + a[1][0].d.score - P.pen_unpaired;
	const int q_pe = mapq_pe(o, subo, score_un, P.lnq[n_sub], P.a, a[0][0].d.frac_rep, a[1][0].d.frac_rep);   // (n_sub < PR_MAXPAIR; lnq[0] = 0)
	int q_se[2], extra_flag = 1;   // (0x1: PairPlan::extra_flag starts at 1)
	if (o > score_un) {   // the pair beats the two best single-end hits
		for (int e = 0; e < 2; ++e) {
			PReg &c = a[e][z[e]];
			if (c.secondary >= 0) { c.sub = a[e][c.secondary].d.score; c.secondary = -2; }
			q_se[e] = mapq_se_in_pair(mapq_se(P, c, ltab, 0), q_pe, c.d.score, 0, P.a);   // (the tandem-repeat cap with csub = 0)
		}
		extra_flag |= 2;
	} else {
		z[0] = z[1] = 0;
		q_se[0] = mapq_se(P, a[0][0], ltab, 0);
		q_se[1] = mapq_se(P, a[1][0], ltab, 0);
	}
	for (int e = 0; e < 2; ++e) {   // the chosen hit was secondary: swap roles with its parent (src/bwamem_pair.c:332-339)
		const int kk = a[e][z[e]].secondary_all;
		if (kk >= 0 && kk < n[e]) {
			for (int j = 0; j < n[e]; ++j)
				if (a[e][j].secondary_all == kk || j == kk) a[e][j].secondary_all = z[e];
			a[e][z[e]].secondary_all = -1;
		}
	}
	// a secondary hit close enough to its primary gets an XA entry (src/bwamem_extra.c:91-110): the host's kind of record
	for (int e = 0; e < 2; ++e)
		for (int j = 0; j < n[e]; ++j) {
			const int kk = a[e][j].secondary_all;
			if (kk >= 0 && a[e][j].d.score >= a[e][kk].d.score * (double)P.XA_drop_ratio) { status[k] = PR_HOST_XA; return; }
		}
	for (int e = 0; e < 2; ++e) {
		const PReg &R = a[e][z[e]];
		const int w2 = reg2aln_band(R.d.qe - R.d.qb, (int)(R.d.re - R.d.rb), R.d.truesc, P.a, P.o_del, P.e_del, P.o_ins, P.e_ins, P.w, R.d.w);
		AlnReq q;
		q.rb = R.d.rb; q.re = R.d.re; q.read = 2 * k + e; q.qb = R.d.qb; q.qe = R.d.qe; q.w2 = w2; q.truesc = R.d.truesc; q.pad = 0;
		reqs[2 * k + e] = q;
		SamDesc d;
		d.rb = R.d.rb; d.re = R.d.re; d.qb = R.d.qb; d.qe = R.d.qe; d.req = e; d.rid = R.d.rid;
		d.flag = 0x40 << e | extra_flag; d.mapq = q_se[e] & 0xff; d.score = R.d.score; d.sub = R.sub;
		desc[2 * k + e] = d;
	}
	status[k] = PR_DECIDED;
}

void launch_pair_simple(void *stream, const PairParams &P, int n_pairs, const DevReg *d_first, const int *d_nfirst, const uint8_t *d_ok,
                        const int64_t *d_ann_off, const uint8_t *d_ann_alt, const double *d_ptab, const double *d_ltab, uint8_t *d_status,
                        AlnReq *d_reqs, SamDesc *d_desc)
{
	if (n_pairs <= 0) return;
	hipLaunchKernelGGL(pair_simple_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, (hipStream_t)stream, P, n_pairs, d_first, d_nfirst, d_ok,
	                   (const i64 *)d_ann_off, d_ann_alt, d_ptab, d_ltab, d_status, d_reqs, d_desc);
}

} // namespace mbw
