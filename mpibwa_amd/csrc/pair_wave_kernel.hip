// pair_wave_kernel.hip — mem_sam_pe for the pairs that need mate rescue or carry up to 64 hits per end: a pair per wavefront.
//
// Device counterpart of
//   mem_sam_pe            src/bwamem_pair.c:250-393   (rescue loop :265-276, primary marking, pairing, MAPQ, the two records)
//   mem_matesw            src/bwamem_pair.c:111-180   (everything but the window and ksw_align2: the windows are listed by the host,
//                                                       the alignments are msw2_kernel's results, already on the device)
//   mem_sort_dedup_patch  src/bwamem.c:437-489        (as :176 calls it — no reference sequence, so nothing is patched — on a list that
//                                                       is a fixed point of the pass plus one new hit: host_pair.cpp insert_into_settled)
//   mem_mark_primary_se   src/bwamem.c:493-569        (reads without ALT hits)
//   mem_pair              src/bwamem_pair.c:182-243
//   mem_approx_mapq_se    src/bwamem.c:952-976        (with csub: a rescued hit carries the score of its tandem copy)
//   mem_gen_alt           src/bwamem_extra.c:98-118   (which hits the chosen hit's XA string lists: their CIGAR requests; the text is
//                                                       sam_emit_kernel's)
//   mem_reg2aln           src/bwamem.c:1089-1105      (the band of the final global alignment)
//   no_pairing:           src/bwamem_pair.c:371-392   (with the side arrays of device.h: SeLines — the pairs reported end by end: which hits
//                                                       of each end become lines, src/bwamem.c:1015-1032, the proper-pair flag of :382-387;
//                                                       sam_lines_kernel.hip writes the text)
// The pairs are the ones pair_simple_kernel leaves with "rescue", "more than eight hits" or "one end without a hit".  The host hands over
// both ends' lists as they stand after mem_sort_dedup_patch (fixed points of the pass: HRegV::settled), at most PW_MAXREG regions each,
// none on an ALT contig, and per (end, candidate hit, orientation) a tag: the number of the alignment in the pair's slice of the
// mate-rescue results, "the window is invalid: the reference aligns nothing", or "not on the device".
//
// The list in LDS, the wave reductions, mem_mark_primary_se and the XA listing are wave_common.cuh's, shared with se_wave_kernel.hip.
// One region per lane, both lists in LDS as one array per field (no bank conflicts, 2 x 64 x 64 B), mem_pair's keys behind them
// (128 x 16 B) and the rescue candidates: 11 776 B of LDS per wave, 63 VGPRs, no scratch (the compiler's resource usage for gfx950).  The two sorts are rank sorts: mem_pair's keys are unique, so any sort gives the reference's array; two
// hits with equal (score, hash) in mem_mark_primary_se — where the reference's unstable sort would decide — send the pair to the host.
// The list u of mem_pair is never stored: only its maximum, the second-largest score and n_sub are used, so it is enumerated twice
// and reduced.  Anything the wave cannot settle the way the reference does leaves the pair to the host with a code that says why.
//
// Floating point: as in pair_kernel.hip — the reference's types and order, -ffp-contract=off, the two transcendental sites tabulated.
#include <hip/hip_runtime.h>
#include "wave_common.cuh"

namespace mbw {

// q ends first; p looks back at it (src/bwamem.c:448-455)
__device__ __forceinline__ bool pw_redundant(const PairParams &P, i64 q_rb, i64 q_re, int q_qb, int q_qe, i64 p_rb, i64 p_re, int p_qb, int p_qe)
{
	return p_rb < q_re + P.max_chain_gap && redundant_overlap(P.mask_level_redun, q_rb, q_re, q_qb, q_qe, p_rb, p_re, p_qb, p_qe);
}

// The redundancy pass on "a fixed point of it + the new hit b" (host_pair.cpp insert_into_settled; the argument why this is
// the reference's list is there).  Every lane holds a hit of the list M.  Returns 0, or the code of why the pair is the host's.
__device__ __forceinline__ int pw_insert(const PairParams &P, WList &M, int &n, const WReg &b, int lane)
{
	bool red = false;
	i64 e_re = 0;
	int e_sc = 0;
	if (lane < n && M.rid[lane] == b.rid) {
		const i64 e_rb = M.rb[lane];
		const int e_qb = M.qb[lane], e_qe = M.qe[lane];
		e_re = M.re[lane]; e_sc = M.score[lane];
		// (equal end positions: either may be the one the pass visits first)
		red = e_re < b.re ? pw_redundant(P, e_rb, e_re, e_qb, e_qe, b.rb, b.re, b.qb, b.qe)
		    : e_re > b.re ? pw_redundant(P, b.rb, b.re, b.qb, b.qe, e_rb, e_re, e_qb, e_qe)
		    : (pw_redundant(P, e_rb, e_re, e_qb, e_qe, b.rb, b.re, b.qb, b.qe) || pw_redundant(P, b.rb, b.re, b.qb, b.qe, e_rb, e_re, e_qb, e_qe));
	}
	const u64 R = __ballot(red);
	bool b_alive = true;
	u64 dead = 0;
	if (R) {
		if (!__ballot(red && e_sc >= b.score)) dead = R;   // all of them score less: they die, b stays, whatever the order
		else {
			// the order of the events is that of the end positions: defined when these are distinct
			if (__ballot(red && e_re == b.re)) return PW_HOST_TIE;
			for (u64 m = R; m; m &= m - 1) {
				const int j = __ffsll((long long)m) - 1;
				const i64 re_j = M.re[j];
				if (__ballot(red && lane != j && e_re == re_j)) return PW_HOST_TIE;
			}
			const i64 NONE_LO = (i64)0x8000000000000000ull, NONE_HI = ~NONE_LO;
			// b looks back, nearest first: the hits that end before it die until one scores more, which kills b
			const i64 killer_b = wave_max(red && e_re < b.re && e_sc > b.score ? e_re : NONE_LO);
			if (killer_b != NONE_LO) { b_alive = false; dead = __ballot(red && e_re < b.re && e_re > killer_b); }
			else {
				dead = __ballot(red && e_re < b.re);
				// the hits behind b meet it in turn: they die until one scores at least b's, which kills b
				const i64 killer_a = wave_min(red && e_re > b.re && e_sc >= b.score ? e_re : NONE_HI);
				if (killer_a != NONE_HI) { b_alive = false; dead |= __ballot(red && e_re > b.re && e_re < killer_a); }
				else dead |= __ballot(red && e_re > b.re);
			}
		}
	}
	if (!dead && !b_alive) return 0;
	// the survivors keep their order; b goes to its place by (score desc, rb, qb)
	const u64 valid = n >= 64 ? ~(u64)0 : ((u64)1 << n) - 1;
	const u64 alive = valid & ~dead;
	const int n_new = __popcll(alive) + (b_alive ? 1 : 0);
	if (n_new > PW_MAXREG) return PW_HOST_FULL;
	const bool keep = (alive >> lane) & 1;
	WReg me;
	bool before_b = false;
	if (keep) {
		me = wl_get(M, lane);
		before_b = me.score > b.score || (me.score == b.score && (me.rb < b.rb || (me.rb == b.rb && me.qb < b.qb)));
	}
	const int at = __popcll(__ballot(before_b));
	const int pos = __popcll(alive & (((u64)1 << lane) - 1)) + (b_alive && !before_b ? 1 : 0);
	__syncthreads();
	if (keep) wl_put(M, pos, me);
	if (b_alive && lane == 0) wl_put(M, at, b);
	__syncthreads();
	n = n_new;
	return 0;
}

// the candidate pairs (v[kk], v[i]) of mem_pair for one i (pairmath.h) with the device's score table; the scan starts at i - 1 (the
// reference starts at the last key of kind `which` before i: the ones between are skipped)
template <class F>
__device__ __forceinline__ void pw_pairs_of(const PairParams &P, const Pair64 *V, int i, int idi, const double *__restrict__ ptab, F f)
{
	pair_candidates_of(V, i, P.low, P.high, P.failed, idi, [&](int) { return i - 1; },
	                   [&](int dir, i64 dist) { return ptab[P.tab_off[dir] + (int)(dist - P.low[dir])]; }, f);
}

#define PW_GIVE_UP(code) do { if (lane == 0) wstatus[t] = (uint8_t)(code); return; } while (0)

// work[t]: the pair (number in the chunk); its lists: lists[loff[2t + e] .. loff[2t + e + 1]); its mate-rescue alignments:
// mreq / mres[mfirst[t] ..]; tags[toff[t] + 4 * (candidate) + orientation], the candidates of end 0 first, then end 1's (toff: n_work + 1 entries).
// wstatus[t] = PR_DECIDED: reqs / desc [2t + e] are the pair's, as pair_simple_kernel writes them (reqs.read = 2 work[t] + e); else untouched.
// xa_reqs given: a chosen hit with XA entries no longer sends the pair to the host.  wstatus[t] = PW_DECIDED_XA, xa_cnt[2t + e] entries
// of end e with their requests at xa_reqs[(2t + e) * PW_XA_CAP ..], in list order; desc[2t + e].flag carries the count in bits 16-19 and
// desc[2t + 1].req = 1 + xa_cnt[2t] (the pair's requests in a job: read 0's, its XA entries', read 1's, its XA entries').
// LN.desc given: a pair mem_sam_pe reports through no_pairing: (src/bwamem_pair.c:371-392: an end without a hit, no pair in a proper
// orientation and distance, a best pair that scores nothing, an end with several primary hits of at least T) is decided too, instead of
// PW_HOST_NO_PAIR / _SCORE / _SUPP: wstatus[t] = PW_DECIDED_LINES, LN.n_lines[2t + e] = the lines of end e (0: the unaligned record,
// which has no descriptor; up to SE_LINES_CAP, more leave the pair with PW_HOST_SUPP), line j of end e in slot
// x = (2t + e) * SE_LINES_CAP + j of LN.desc / LN.reqs / LN.xa_cnt with its XA requests at LN.xa_reqs[x * PW_XA_CAP ..].  desc.flag =
// 0x40 << e | 1, | 2 when the two top hits make a proper pair (:382-387), | LN.supp_flag behind the first line, the XA count in bits
// 16-19; desc.req counts from the pair's first request: [end 0: line 0, its XA entries, line 1, ...; end 1: ...]; reqs.read = 2 work[t] + e.
// reqs / desc / xa_cnt [2t + e] are not written for such a pair.  LN.xa_reqs = nullptr: a line with XA entries gives PW_HOST_XA.
__global__ void __launch_bounds__(64)
pair_wave_kernel(PairParams P, int n_work, const int *__restrict__ work, const DevReg *__restrict__ lists, const int *__restrict__ loff,
                 const int *__restrict__ len, const MswReq *__restrict__ mreq, const MswRes *__restrict__ mres, const unsigned *__restrict__ mfirst,
                 const short *__restrict__ tags, const int *__restrict__ toff, const i64 *__restrict__ ann_off, const double *__restrict__ ptab,
                 const double *__restrict__ ltab, uint8_t *__restrict__ wstatus, AlnReq *__restrict__ reqs, SamDesc *__restrict__ desc,
                 AlnReq *__restrict__ xa_reqs, uint8_t *__restrict__ xa_cnt, SeLines LN)
{
	__shared__ WList L[2];
	__shared__ Pair64 V[2 * PW_MAXREG];
	__shared__ i64 c_rb[2][PW_MAXREG];   // the candidate hits of the rescue loop: what mem_matesw reads of them
	__shared__ int c_rid[2][PW_MAXREG];
	const int t = blockIdx.x, lane = threadIdx.x;
	if (t >= n_work) return;
	const int k = work[t];
	int n[2];
	for (int e = 0; e < 2; ++e) {
		const int b = loff[2 * t + e];
		n[e] = loff[2 * t + e + 1] - b;
		if (n[e] > PW_MAXREG) PW_GIVE_UP(PW_HOST_FULL);
		if (lane < n[e]) {
			wl_put(L[e], lane, wl_from(lists[b + lane]));
		}
	}
	__syncthreads();

	// ---- the rescue loop (src/bwamem_pair.c:265-276): the candidates are copied before any rescue, end 0's are used first ----
	if (!P.no_rescue) {
		int nc[2];
		for (int e = 0; e < 2; ++e) {
			const bool cand = lane < n[e] && L[e].score[lane] >= L[e].score[0] - P.pen_unpaired;
			const u64 m = __ballot(cand);
			const int ord = __popcll(m & (((u64)1 << lane) - 1));
			if (cand && ord < P.max_matesw) { c_rb[e][ord] = L[e].rb[lane]; c_rid[e][ord] = L[e].rid[lane]; }
			nc[e] = __popcll(m) < P.max_matesw ? __popcll(m) : P.max_matesw;
		}
		__syncthreads();
		if (4 * (nc[0] + nc[1]) != toff[t + 1] - toff[t]) PW_GIVE_UP(PW_HOST_NO_RESULT);   // (the host listed other candidates: no tag is read)
		const unsigned mb = mfirst[t];
		for (int e = 0; e < 2; ++e) {
			const int ma = !e;   // the mate's list takes the rescued hits
			const int tb = toff[t] + (e ? 4 * nc[0] : 0);
			for (int c = 0; c < nc[e]; ++c) {
				const i64 a_rb = c_rb[e][c];
				// mem_matesw :118-128: the orientations that failed or that a hit of the mate's CURRENT list explains
				int r_l = -1;
				if (lane < n[ma]) {
					int64_t dist;
					const int r = infer_dir(P.l_pac, a_rb, L[ma].rb[lane], &dist);
					if (dist >= P.low[r] && dist <= P.high[r]) r_l = r;
				}
				bool skip[4];
				for (int r = 0; r < 4; ++r) skip[r] = P.failed[r] || __ballot(r_l == r) != 0;
				if (skip[0] && skip[1] && skip[2] && skip[3]) continue;
				const int l_ms = len[2 * k + ma];
				for (int r = 0; r < 4; ++r) {
					if (skip[r]) continue;
					const int tag = tags[tb + 4 * c + r];
					if (tag == PW_TAG_NO_WINDOW) continue;   // the reference aligns nothing here (:150)
					if (tag < 0) PW_GIVE_UP(PW_HOST_NO_RESULT);
					const MswRes res = mres[mb + tag];
					const MswReq rq = mreq[mb + tag];
					if (res.flags) PW_GIVE_UP(PW_HOST_NO_RESULT);
					if (!(res.score >= P.min_seed_len && res.qb >= 0)) continue;
					WReg b;   // :155-170
					const bool is_rev = rq.is_rev != 0;
					b.rid = c_rid[e][c];
					b.qb = is_rev ? l_ms - (res.qe + 1) : res.qb;
					b.qe = is_rev ? l_ms - res.qb : res.qe + 1;
					b.rb = is_rev ? (P.l_pac << 1) - (rq.rb + res.te + 1) : rq.rb + res.tb;
					b.re = is_rev ? (P.l_pac << 1) - (rq.rb + res.tb) : rq.rb + res.te + 1;
					b.score = res.score; b.csub = res.score2; b.secondary = -1;
					b.truesc = b.w = b.sub = b.sub_n = 0; b.secondary_all = 0; b.frac_rep = 0.f;
					const int why = pw_insert(P, L[ma], n[ma], b, lane);
					if (why) PW_GIVE_UP(why);
				}
			}
		}
	}
	const u64 id = P.id0 + (u64)k;
	int why = PW_HOST_NO_PAIR;   // which of mem_sam_pe's exits to no_pairing: the pair takes (the code it has without the side arrays)
	bool marked = false;
	if (n[0] == 0 || n[1] == 0) goto no_pairing;   // (n_pri = 0: the ends are reported independently)
	{
		if (!pw_mark_primary(P, L[0], n[0], id << 1 | 0, V, lane)) PW_GIVE_UP(PW_HOST_TIE);
		if (!pw_mark_primary(P, L[1], n[1], id << 1 | 1, V, lane)) PW_GIVE_UP(PW_HOST_TIE);
		marked = true;

		// ---- mem_pair (src/bwamem_pair.c:182-243) ----
		const int nv = n[0] + n[1];
		{
			Pair64 key[2];
			for (int r = 0; r < 2; ++r)
				if (lane < n[r]) {
					const int rid = L[r].rid[lane];
					key[r] = pair_key(P.l_pac, L[r].rb[lane], rid, ann_off[rid], L[r].score[lane], lane, r);
					V[r * n[0] + lane] = key[r];
				}
			__syncthreads();
			int rank[2] = {0, 0};
			for (int j = 0; j < nv; ++j) {   // (unique keys: the rank is the place in the reference's sorted array)
				const Pair64 o = V[j];
				if (lane < n[0] && pair_lt(o, key[0])) ++rank[0];
				if (lane < n[1] && pair_lt(o, key[1])) ++rank[1];
			}
			__syncthreads();
			for (int r = 0; r < 2; ++r)
				if (lane < n[r]) V[rank[r]] = key[r];
			__syncthreads();
		}
		const int idi = pair_id_mix(id);
		// u is not stored: its maximum under (x, y), the second-largest score and n_sub are reductions
		Pair64 best;
		best.x = best.y = 0;
		int cnt = 0, q2 = -1;   // of this lane's candidates: how many, the best, the largest score among the others
		for (int i = lane; i < nv; i += 64)
			pw_pairs_of(P, V, i, idi, ptab, [&](const Pair64 &p) {
				if (cnt == 0) best = p;
				else if (pair_lt(best, p)) { const int qb_ = (int)(best.x >> 32); q2 = q2 > qb_ ? q2 : qb_; best = p; }
				else { const int qp = (int)(p.x >> 32); q2 = q2 > qp ? q2 : qp; }
				++cnt;
			});
		const int nu = wave_sum(cnt);
		if (nu == 0) goto no_pairing;   // no pair in a proper orientation and distance
		const u64 gx = wave_maxu(cnt ? best.x : 0);
		const bool top_x = cnt && best.x == gx;
		const u64 gy = wave_maxu(top_x ? best.y : 0);   // (several candidates can share x; y = (kk, i) is unique)
		const bool mine = top_x && best.y == gy;
		int subo = (int)wave_max((i64)(mine ? q2 : cnt ? (int)(best.x >> 32) : -1));
		if (nu < 2) subo = 0;
		const int tmp = sub_n_margin(P.a, P.b, P.o_del, P.e_del, P.o_ins, P.e_ins);
		int n_sub = 0;
		if (nu > 1) {
			int c2 = 0;
			for (int i = lane; i < nv; i += 64)
				pw_pairs_of(P, V, i, idi, ptab, [&](const Pair64 &p) {
					if (!(p.x == gx && p.y == gy) && subo - (int)(p.x >> 32) <= tmp) ++c2;
				});
			n_sub = wave_sum(c2);
		}
		int z[2];
		{
			const int i = (int)(gy >> 32), kk = (int)(gy << 32 >> 32);
			const Pair64 vi = V[i], vk = V[kk];
			z[vi.y & 1] = (int)(vi.y << 32 >> 34);
			z[vk.y & 1] = (int)(vk.y << 32 >> 34);
		}
		const int o = (int)(gx >> 32);
		if (o <= 0) { why = PW_HOST_SCORE; goto no_pairing; }

		// ---- is_multi, q_pe, q_se, the caps, the swap (:289-339); every lane computes the same numbers ----
		for (int e = 0; e < 2; ++e)   // an end with several good primary hits is left to the single-end logic
			if (__ballot(lane >= 1 && lane < n[e] && L[e].secondary[lane] < 0 && L[e].score[lane] >= P.T)) { why = PW_HOST_SUPP; goto no_pairing; }
		const int score_un = L[0].score[0] + L[1].score[0] - P.pen_unpaired;
		if (n_sub >= 40) PW_GIVE_UP(PW_HOST_LENGTH);   // (beyond the table of (int)(4.343 * log(n + 1) + .499), whose entry 0 is 0)
		const int q_pe = mapq_pe(o, subo, score_un, P.lnq[n_sub], P.a, L[0].frac_rep[0], L[1].frac_rep[0]);
		int q_se[2], extra_flag = 1, sub_z[2];
		const bool pair_wins = o > score_un;
		if (!pair_wins) z[0] = z[1] = 0;
		for (int e = 0; e < 2; ++e) {
			const WReg c = wl_get(L[e], z[e]);
			int sub = c.sub;
			if (pair_wins && c.secondary >= 0) sub = L[e].score[c.secondary];   // (c.secondary = -2 in the reference: it is not read again)
			sub_z[e] = sub;
			const int l = c.qe - c.qb > c.re - c.rb ? c.qe - c.qb : (int)(c.re - c.rb);
			if (l >= P.ltab_n || l <= 0 || c.sub_n >= 40) PW_GIVE_UP(PW_HOST_LENGTH);
			q_se[e] = mapq_se_of(P, c.score, sub, c.sub_n, c.csub, l, c.frac_rep, ltab);
			if (pair_wins) q_se[e] = mapq_se_in_pair(q_se[e], q_pe, c.score, c.csub, P.a);
		}
		if (pair_wins) extra_flag |= 2;
		__syncthreads();
		for (int e = 0; e < 2; ++e) {   // the chosen hit was secondary: swap roles with its parent
			const int kk = L[e].secondary_all[z[e]];
			__syncthreads();
			if (kk >= 0 && kk < n[e]) {
				if (lane < n[e] && (L[e].secondary_all[lane] == kk || lane == kk)) L[e].secondary_all[lane] = z[e];
				__syncthreads();
				if (lane == 0) L[e].secondary_all[z[e]] = -1;
				__syncthreads();
			}
		}
		// ---- the XA entries of the two chosen hits and their requests (wave_common.cuh: pw_xa_list) ----
		int n_xa[2];
		for (int e = 0; e < 2; ++e) {
			n_xa[e] = pw_xa_list(P, L[e], n[e], z[e], 2 * k + e, xa_reqs ? xa_reqs + (size_t)(2 * t + e) * PW_XA_CAP : nullptr, lane);
			if (n_xa[e] < 0) PW_GIVE_UP(PW_HOST_XA);
		}
		if (lane < 2) {
			const int e = lane;
			const WReg R = wl_get(L[e], z[e]);
			const int w2 = reg2aln_band(R.qe - R.qb, (int)(R.re - R.rb), R.truesc, P.a, P.o_del, P.e_del, P.o_ins, P.e_ins, P.w, R.w);   // (a rescued hit has w = 0)
			AlnReq q;
			q.rb = R.rb; q.re = R.re; q.read = 2 * k + e; q.qb = R.qb; q.qe = R.qe; q.w2 = w2; q.truesc = R.truesc; q.pad = 0;
			reqs[2 * t + e] = q;
			SamDesc d;
			d.rb = R.rb; d.re = R.re; d.qb = R.qb; d.qe = R.qe; d.req = e ? 1 + n_xa[0] : 0; d.rid = R.rid;
			d.flag = 0x40 << e | extra_flag | n_xa[e] << SAM_XA_SHIFT; d.mapq = q_se[e] & 0xff; d.score = R.score;
			d.sub = sub_z[e] > R.csub ? sub_z[e] : R.csub;   // mem_reg2aln: sub = max(sub, csub)
			desc[2 * t + e] = d;
			if (xa_cnt) xa_cnt[2 * t + e] = (uint8_t)n_xa[e];
		}
		if (lane == 0) wstatus[t] = n_xa[0] + n_xa[1] ? PW_DECIDED_XA : PR_DECIDED;
		return;
	}

no_pairing:
	// ---- no_pairing: (src/bwamem_pair.c:371-392): each end goes through mem_reg2sam with the other end's top hit as its mate ----
	if (!LN.desc) PW_GIVE_UP(why);
	if (!marked)
		for (int e = 0; e < 2; ++e)   // (an empty list is marked at once)
			if (!pw_mark_primary(P, L[e], n[e], id << 1 | e, V, lane)) PW_GIVE_UP(PW_HOST_TIE);
	u64 lines[2];
	int nl[2];
	for (int e = 0; e < 2; ++e) {   // the lines of mem_reg2sam (src/bwamem.c:1015-1032) without MEM_F_ALL: the primary hits of at least T
		lines[e] = __ballot(lane < n[e] && L[e].secondary[lane] < 0 && L[e].score[lane] >= P.T);
		nl[e] = __popcll(lines[e]);
		if (nl[e] > SE_LINES_CAP) PW_GIVE_UP(PW_HOST_SUPP);
	}
	int extra_flag = 1;
	// :382-387: both ends have a top hit of at least T (hit 0 of a marked list scores most), on one contig and at a proper distance
	if ((lines[0] & lines[1] & 1) && L[0].rid[0] == L[1].rid[0]) {
		int64_t dist;
		const int d = infer_dir(P.l_pac, L[0].rb[0], L[1].rb[0], &dist);
		if (!P.failed[d] && dist >= P.low[d] && dist <= P.high[d]) extra_flag |= 2;
	}
	int at = 0;   // the pair's requests: [end 0: line 0, its XA entries, line 1, ...; end 1: ...]
	for (int e = 0; e < 2; ++e) {
		if (!nl[e]) continue;   // the unaligned record (:1033-1037) has neither request nor descriptor: it is the writer's
		const int r = wave_lines<true>(P, LN, L[e], n[e], lines[e], nl[e], 2 * k + e, (size_t)(2 * t + e) * SE_LINES_CAP, at, 0x40 << e | extra_flag, ltab, lane);
		if (r == -1) PW_GIVE_UP(PW_HOST_XA);
		if (r < 0) PW_GIVE_UP(PW_HOST_LENGTH);
		at += r;
	}
	if (lane < 2) LN.n_lines[2 * t + lane] = (uint8_t)(lane ? nl[1] : nl[0]);
	if (lane == 0) wstatus[t] = PW_DECIDED_LINES;
}

void launch_pair_wave(void *stream, const PairParams &P, int n_work, const int *d_work, const DevReg *d_lists, const int *d_loff, const int *d_len,
                      const MswReq *d_mreq, const MswRes *d_mres, const unsigned *d_mfirst, const short *d_tags, const int *d_toff,
                      const int64_t *d_ann_off, const double *d_ptab, const double *d_ltab, uint8_t *d_wstatus, AlnReq *d_reqs, SamDesc *d_desc,
                      AlnReq *d_xa_reqs, uint8_t *d_xa_cnt, const SeLines *lines)
{
	if (n_work <= 0) return;
	if (!d_xa_cnt || P.max_XA_hits > PW_XA_CAP) d_xa_reqs = nullptr, d_xa_cnt = nullptr;   // (XA off: the kernel as it was)
	SeLines LN;   // (no side arrays: the pairs of no_pairing: are the host's, as they were)
	if (lines && lines->desc && lines->reqs && lines->n_lines && lines->xa_cnt) LN = *lines;
	if (P.max_XA_hits > PW_XA_CAP) LN.xa_reqs = nullptr;
	hipLaunchKernelGGL(pair_wave_kernel, dim3(n_work), dim3(64), 0, (hipStream_t)stream, P, n_work, d_work, d_lists, d_loff, d_len, d_mreq, d_mres, d_mfirst,
	                   d_tags, d_toff, (const i64 *)d_ann_off, d_ptab, d_ltab, d_wstatus, d_reqs, d_desc, d_xa_reqs, d_xa_cnt, LN);
}

// the decided pairs' requests and descriptors into the chunk-wide arrays the CIGAR-and-SAM job reads
__global__ void pair_wave_clear_kernel(int r0, int n_reads, AlnReq *__restrict__ reqs, SamDesc *__restrict__ desc)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_reads) return;
	reqs[r0 + i].read = -1;
	desc[r0 + i].req = -1;
}
__global__ void pair_wave_scatter_kernel(int n_work, const int *__restrict__ work, const uint8_t *__restrict__ wstatus, const AlnReq *__restrict__ w_reqs,
                                         const SamDesc *__restrict__ w_desc, AlnReq *__restrict__ reqs, SamDesc *__restrict__ desc)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= 2 * n_work) return;
	const int t = i >> 1, e = i & 1;
	if (wstatus[t] != PR_DECIDED) return;
	reqs[2 * work[t] + e] = w_reqs[i];
	desc[2 * work[t] + e] = w_desc[i];
}
void launch_pair_wave_scatter(void *stream, int n_work, const int *d_work, const uint8_t *d_wstatus, const AlnReq *d_w_reqs, const SamDesc *d_w_desc,
                              AlnReq *d_reqs, SamDesc *d_desc, int clear_r0, int clear_n)
{
	if (clear_n > 0) hipLaunchKernelGGL(pair_wave_clear_kernel, dim3((clear_n + 255) / 256), dim3(256), 0, (hipStream_t)stream, clear_r0, clear_n, d_reqs, d_desc);
	if (n_work > 0)
		hipLaunchKernelGGL(pair_wave_scatter_kernel, dim3((2 * n_work + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_work, d_work, d_wstatus, d_w_reqs, d_w_desc,
		                   d_reqs, d_desc);
}

} // namespace mbw
