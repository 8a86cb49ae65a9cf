// pairmath.h — the arithmetic of mem_sam_pe and of what it calls (mem_pair, mem_matesw, mem_sort_dedup_patch, mem_mark_primary_se,
// mem_approx_mapq_se, mem_reg2aln), stated ONCE for the host and for the pairing, single-end and redundancy kernels.  An off-by-one or
// a re-ordered product in any of these moves a MAPQ or a tie, so every function keeps the reference's TYPES and ORDER of operations:
// float options stay float (mask_level_redun * int64, min_l * mask_level, 0.05f), double expressions stay double in the same order (the
// library is built with -ffp-contract=off).  The functions take scalars and the small PODs defined here, never an options or region
// struct: the host and the kernels unpack their own at the call.  Where the reference calls libm (log, erfc) the value comes in as an
// argument or a callable: libm on the host, a host-built table on the device.
// Plain C++ for the host compilers (no HIP header); __host__ __device__ in a HIP translation unit (KS_FN, sortutil.h).
#ifndef MBW_PAIRMATH_H
#define MBW_PAIRMATH_H
#include <cstdint>
#include "sortutil.h"

namespace mbw {

KS_FN uint64_t hash_64(uint64_t key)   // Thomas Wang's 64-bit mix, src/utils.h:98-109
{
	key += ~(key << 32); key ^= (key >> 22); key += ~(key << 13); key ^= (key >> 8);
	key += (key << 3);   key ^= (key >> 15); key += ~(key << 27); key ^= (key >> 31);
	return key;
}

// orientation (0 FF, 1 FR, 2 RF, 3 RR) and distance of two hits given in the doubled coordinate (src/bwamem_pair.c:23-30)
KS_FN int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist)
{
	const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
	const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;   // mate projected on read 1's strand
	*dist = p2 > b1 ? p2 - b1 : b1 - p2;
	return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

KS_FN int infer_bw(int l1, int l2, int score, int a, int q, int r)   // src/bwamem.c:792-800
{
	if (l1 == l2 && l1 * a - score < (q + r - a) << 1) return 0;   // equal lengths need at least two gaps
	int w = (int)((double)((l1 < l2 ? l1 : l2) * a - score - q) / r + 2.);
	const int d = l1 > l2 ? l1 - l2 : l2 - l1;
	if (w < d) w = d;
	return w;
}
// the band mem_reg2aln starts its global alignment with (src/bwamem.c:1099-1102); l1, l2: query and reference span; w_reg: the region's
// band (0 for a hit that comes from mate rescue)
KS_FN int reg2aln_band(int l1, int l2, int truesc, int a, int o_del, int e_del, int o_ins, int e_ins, int w_opt, int w_reg)
{
	const int tmp = infer_bw(l1, l2, truesc, a, o_del, e_del);
	int w2 = infer_bw(l1, l2, truesc, a, o_ins, e_ins);
	w2 = w2 > tmp ? w2 : tmp;
	if (w2 > w_opt) w2 = w2 < w_reg ? w2 : w_reg;
	return w2;
}

// two scores this close count as equally good: max(a + b, o_del + e_del, o_ins + e_ins) (src/bwamem.c:497-499, src/bwamem_pair.c:230-232)
KS_FN int sub_n_margin(int a, int b, int o_del, int e_del, int o_ins, int e_ins)
{
	int tmp = a + b;
	tmp = o_del + e_del > tmp ? o_del + e_del : tmp;
	tmp = o_ins + e_ins > tmp ? o_ins + e_ins : tmp;
	return tmp;
}

// mem_sort_dedup_patch: do q and p — q ends first, p looks back at it — overlap enough for one of them to be redundant
// (src/bwamem.c:448-455)?  The reach test p_rb < q_re + max_chain_gap is the caller's.
KS_FN bool redundant_overlap(float mask_level_redun, int64_t q_rb, int64_t q_re, int q_qb, int q_qe, int64_t p_rb, int64_t p_re, int p_qb, int p_qe)
{
	const int64_t orr = q_re - p_rb;
	const int64_t oq = q_qb < p_qb ? q_qe - p_qb : p_qe - q_qb;
	const int64_t mr = q_re - q_rb < p_re - p_rb ? q_re - q_rb : p_re - p_rb;
	const int64_t mq = q_qe - q_qb < p_qe - p_qb ? q_qe - q_qb : p_qe - p_qb;
	return orr > mask_level_redun * mr && oq > mask_level_redun * mq;
}
// mem_patch_reg(x, y) up to its alignment (src/bwamem.c:411-423), x.rb <= y.rb on one contig: -1 = the reference returns without
// aligning; otherwise it aligns across the two, and the value is its w at that point (:415)
KS_FN int patch_reg_w(int64_t l_pac, int w_opt, int64_t x_rb, int64_t x_re, int x_qb, int x_qe, int64_t y_rb, int64_t y_re, int y_qb, int y_qe)
{
	if (x_rb < l_pac && y_rb >= l_pac) return -1;   // on different strands
	if (x_qb >= y_qb || x_qe >= y_qe || x_re >= y_re) return -1;   // not colinear
	int w = (int)((x_re - y_rb) - (x_qe - y_qb));
	w = w > 0 ? w : -w;
	double r = (double)(x_re - y_rb) / (y_re - x_rb) - (double)(x_qe - y_qb) / (y_qe - x_qb);
	r = r > 0. ? r : -r;
	if (x_re < y_rb || x_qe < y_qb) {
		if (w > w_opt << 1 || r >= 0.05f) return -1;
	} else if (w > w_opt << 2 || r >= 0.05f * 2) return -1;
	return w;
}

// mem_mark_primary_se_core, cal_sub: "significant overlap on the query" of hits i and j (src/bwamem.c:503-507, src/bwamem_pair.c:37-42)
KS_FN bool query_overlap(float mask_level, int i_qb, int i_qe, int j_qb, int j_qe)
{
	const int b_max = j_qb > i_qb ? j_qb : i_qb;
	const int e_min = j_qe < i_qe ? j_qe : i_qe;
	if (e_min <= b_max) return false;
	const int min_l = i_qe - i_qb < j_qe - j_qb ? i_qe - i_qb : j_qe - j_qb;
	return e_min - b_max >= min_l * mask_level;
}

// ---- mem_pair (src/bwamem_pair.c:182-243) ----
struct Pair64 { uint64_t x, y; };   // pair64_t
KS_FN bool pair_lt(const Pair64 &a, const Pair64 &b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

// the key of hit i of end r (:191-196): x = contig and forward-strand position in it, y = score, i, strand, end
KS_FN Pair64 pair_key(int64_t l_pac, int64_t rb, int rid, int64_t contig_offset, int score, int i, int r)
{
	Pair64 key;
	key.x = (uint64_t)(rb < l_pac ? rb : (l_pac << 1) - 1 - rb);
	key.x = (uint64_t)rid << 32 | (key.x - (uint64_t)contig_offset);
	key.y = (uint64_t)score << 32 | (uint64_t)(i << 2 | (rb >= l_pac) << 1 | r);
	return key;
}
// what the pair's number contributes to the hash tie-break (:222, `id << 8` on the reference's int id), as defined arithmetic
KS_FN int pair_id_mix(uint64_t id) { return (int)((unsigned)(int)id << 8); }

// the candidate pairs (v[k], v[i]) for one i (:203-227): f(p) for each, p as the reference builds it.  v: the sorted keys;
// start(which): where the backward scan for keys of kind `which` (end and strand, v.y & 3) begins — the reference's y[which], the last
// such key before i, or any index from there to i - 1 (the keys between are of other kinds and skipped); term(dir, dist): the double
// .721 * log(2 * erfc(|dist - avg| / std / sqrt 2)) * a of :218-219
template <class Start, class Term, class F>
KS_FN void pair_candidates_of(const Pair64 *v, int i, const int *low, const int *high, const int *failed, int id_mix, Start start, Term term, F f)
{
	const Pair64 vi = v[i];
	for (int r = 0; r < 2; ++r) {
		const int dir = r << 1 | (int)(vi.y >> 1 & 1);
		if (failed[dir]) continue;
		const int which = r << 1 | (int)((vi.y & 1) ^ 1);
		for (int k = start(which); k >= 0; --k) {
			const Pair64 vk = v[k];
			if ((int)(vk.y & 3) != which) continue;
			const int64_t dist = (int64_t)vi.x - (int64_t)vk.x;
			if (dist > high[dir]) break;
			if (dist < low[dir]) continue;
			int q = (int)((double)((vi.y >> 32) + (vk.y >> 32)) + term(dir, dist) + .499);
			if (q < 0) q = 0;
			Pair64 p;
			p.y = (uint64_t)k << 32 | (uint64_t)i;
			p.x = (uint64_t)q << 32 | (hash_64(p.y ^ (uint64_t)(int64_t)id_mix) & 0xffffffffU);
			f(p);
		}
	}
}

// ---- MAPQ ----
KS_FN int raw_mapq(int diff, int a) { return (int)(6.02 * diff / a + .499); }   // src/bwamem_pair.c:245

// mem_approx_mapq_se with mapQ_coef_len > 0, the -Q form (src/bwamem.c:952-976).  l = max(query span, reference span); csub: the score
// of a tandem copy (a hit from mate rescue carries one, src/bwamem_pair.c:163);
// len_fac = l < mapQ_coef_len ? 1 : mapQ_coef_fac / log(l) (:964); sub_n_pen = (int)(4.343 * log(sub_n + 1) + .499) (:972)
KS_FN int mapq_se_q(int score, int sub_, int sub_n, int csub, int l, float frac_rep, int a, int b, int min_seed_len, double len_fac, int sub_n_pen)
{
	int sub = sub_ ? sub_ : min_seed_len * a;
	sub = csub > sub ? csub : sub;
	if (sub >= score) return 0;
	const double identity = 1. - (double)(l * a - score) / (a + b) / l;
	int mapq;
	if (score == 0) mapq = 0;
	else {
		double tmp = len_fac;
		tmp *= identity * identity;
		mapq = (int)(6.02 * (score - sub) / a * tmp * tmp + .499);
	}
	if (sub_n > 0) mapq -= sub_n_pen;
	if (mapq > 60) mapq = 60;
	if (mapq < 0) mapq = 0;
	mapq = (int)(mapq * (1. - frac_rep) + .499);
	return mapq;
}

// mem_sam_pe's q_pe (src/bwamem_pair.c:310-316): o, subo: best and second-best pair score; score_un: the two best single-end hits
// unpaired; n_sub_pen = n_sub > 0 ? (int)(4.343 * log(n_sub + 1) + .499) : 0; frac_rep0/1: of the ends' best hits
KS_FN int mapq_pe(int o, int subo, int score_un, int n_sub_pen, int a, float frac_rep0, float frac_rep1)
{
	subo = subo > score_un ? subo : score_un;
	int q_pe = raw_mapq(o - subo, a);
	q_pe -= n_sub_pen;
	if (q_pe < 0) q_pe = 0;
	if (q_pe > 60) q_pe = 60;
	return (int)(q_pe * (1. - .5 * (frac_rep0 + frac_rep1)) + .499);
}
// q_se of an end of a pair that beats the unpaired hits (:322-330): raised to q_pe, by 40 at most, and capped by the tandem-repeat score
KS_FN int mapq_se_in_pair(int q_se, int q_pe, int score, int csub, int a)
{
	q_se = q_se > q_pe ? q_se : q_pe < q_se + 40 ? q_pe : q_se + 40;
	const int cap = raw_mapq(score - csub, a);
	return q_se < cap ? q_se : cap;
}

} // namespace mbw
#endif
