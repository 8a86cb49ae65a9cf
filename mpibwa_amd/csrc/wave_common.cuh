// wave_common.cuh — what the two wave-per-unit deciding kernels share (pair_wave_kernel.hip: a pair per wavefront; se_wave_kernel.hip:
// a single-end read per wavefront): a region list in LDS with one region per lane, the wave reductions, and the steps both replay
//   mem_mark_primary_se   src/bwamem.c:493-569        (reads without ALT hits; a rank sort, one hit per lane)
//   mem_gen_alt           src/bwamem_extra.c:98-118   (which hits the chosen hit's XA string lists, and their CIGAR requests)
//   mem_reg2aln           src/bwamem.c:1089-1105      (the band of the final global alignment)
//   mem_reg2sam           src/bwamem.c:1015-1032      (the lines of a read with supplementary lines: wave_lines)
// The arithmetic is pairmath.h's through pair_common.cuh, as in every deciding kernel.
#ifndef MBW_WAVE_COMMON_CUH
#define MBW_WAVE_COMMON_CUH
#include <hip/hip_runtime.h>
#include "pair_common.cuh"

namespace mbw {

struct WList {   // the regions of one end, one array per field of mem_alnreg_t that mem_sam_pe reads
	i64 rb[PW_MAXREG], re[PW_MAXREG];
	int qb[PW_MAXREG], qe[PW_MAXREG], rid[PW_MAXREG], score[PW_MAXREG], truesc[PW_MAXREG], w[PW_MAXREG], csub[PW_MAXREG];
	int sub[PW_MAXREG], sub_n[PW_MAXREG], secondary[PW_MAXREG], secondary_all[PW_MAXREG];
	float frac_rep[PW_MAXREG];
};
struct WReg {
	i64 rb, re;
	int qb, qe, rid, score, truesc, w, csub, sub, sub_n, secondary, secondary_all;
	float frac_rep;
};
__device__ __forceinline__ WReg wl_get(const WList &L, int i)
{
	WReg r;
	r.rb = L.rb[i]; r.re = L.re[i]; r.qb = L.qb[i]; r.qe = L.qe[i]; r.rid = L.rid[i]; r.score = L.score[i]; r.truesc = L.truesc[i]; r.w = L.w[i];
	r.csub = L.csub[i]; r.sub = L.sub[i]; r.sub_n = L.sub_n[i]; r.secondary = L.secondary[i]; r.secondary_all = L.secondary_all[i]; r.frac_rep = L.frac_rep[i];
	return r;
}
__device__ __forceinline__ void wl_put(WList &L, int i, const WReg &r)
{
	L.rb[i] = r.rb; L.re[i] = r.re; L.qb[i] = r.qb; L.qe[i] = r.qe; L.rid[i] = r.rid; L.score[i] = r.score; L.truesc[i] = r.truesc; L.w[i] = r.w;
	L.csub[i] = r.csub; L.sub[i] = r.sub; L.sub_n[i] = r.sub_n; L.secondary[i] = r.secondary; L.secondary_all[i] = r.secondary_all; L.frac_rep[i] = r.frac_rep;
}
// a region as the host hands it over: nothing marked yet
__device__ __forceinline__ WReg wl_from(const DevReg &d)
{
	WReg r;
	r.rb = d.rb; r.re = d.re; r.qb = d.qb; r.qe = d.qe; r.rid = d.rid; r.score = d.score; r.truesc = d.truesc; r.w = d.w; r.frac_rep = d.frac_rep;
	r.csub = r.sub = r.sub_n = 0; r.secondary = r.secondary_all = -1;
	return r;
}

__device__ __forceinline__ i64 wave_max(i64 v)
{
	for (int d = 32; d; d >>= 1) { const i64 o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
	return v;
}
__device__ __forceinline__ i64 wave_min(i64 v)
{
	for (int d = 32; d; d >>= 1) { const i64 o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
	return v;
}
__device__ __forceinline__ u64 wave_maxu(u64 v)
{
	for (int d = 32; d; d >>= 1) { const u64 o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
	return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
	for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
	return v;
}

// mem_mark_primary_se (src/bwamem.c:521-569, its core :493-519) on one end, a hit per lane; H: 64 x 2 u64 of scratch.  false: two hits
// compare equal in the sort by (score desc, hash)
__device__ __forceinline__ bool pw_mark_primary(const PairParams &P, WList &A, int n, u64 id, Pair64 *H, int lane)
{
	if (n == 0) return true;
	WReg me;
	u64 h = 0;
	if (lane < n) {
		me = wl_get(A, lane);
		h = hash_64(id + (u64)lane);
		H[lane].x = h; H[lane].y = (u64)(unsigned)me.score;
	}
	__syncthreads();
	int rank = 0;
	bool tie = false;
	if (lane < n)
		for (int j = 0; j < n; ++j) {
			const int sc = (int)H[j].y;
			const u64 hj = H[j].x;
			if (sc > me.score || (sc == me.score && hj < h)) ++rank;
			else if (j != lane && sc == me.score && hj == h) tie = true;
		}
	if (__ballot(tie)) return false;
	__syncthreads();
	if (lane < n) { me.sub = 0; me.secondary = me.secondary_all = -1; wl_put(A, rank, me); }
	__syncthreads();
	const int tmp = sub_n_margin(P.a, P.b, P.o_del, P.e_del, P.o_ins, P.e_ins);
	int qb = 0, qe = 0, sc = 0, sub = 0, sub_n = 0, sec = -1;
	if (lane < n) { qb = A.qb[lane]; qe = A.qe[lane]; sc = A.score[lane]; sub_n = A.sub_n[lane]; }
	for (int i = 1; i < n; ++i) {   // hit i against the primary hits before it, in their order: the first it overlaps is its parent
		const int qb_i = A.qb[i], qe_i = A.qe[i], sc_i = A.score[i];
		const u64 m = __ballot(lane < i && sec < 0 && query_overlap(P.mask_level, qb_i, qe_i, qb, qe));
		if (m) {
			const int j = __ffsll((long long)m) - 1;
			if (lane == j) {
				if (sub == 0) sub = sc_i;
				if (sc - sc_i <= tmp) ++sub_n;
			}
			if (lane == i) sec = j;
		}
	}
	if (lane < n) { A.sub[lane] = sub; A.sub_n[lane] = sub_n; A.secondary[lane] = sec; A.secondary_all[lane] = sec; }
	__syncthreads();
	return true;
}

// Does the chosen hit z of the list get an XA string (src/bwamem_extra.c:105-118, no ALT hit here)?  Only with 1 .. max_XA_hits qualifying
// secondary hits under it; more than that and the reference writes none.  Its entries are those hits in list order (:115-131): a lane per
// listed hit writes the request mem_reg2aln would make for it (src/bwamem.c:1089-1105; pad = the hit's contig) into slots[0 ..], `read`
// as its read.  Returns the number of entries (0: a plain record), or -1: entries, but no room for them (no slots, or more than PW_XA_CAP).
__device__ __forceinline__ int pw_xa_list(const PairParams &P, const WList &L, int n, int z, int read, AlnReq *slots, int lane)
{
	u64 hits = __ballot(lane < n && L.secondary_all[lane] == z && L.score[lane] >= L.score[z] * (double)P.XA_drop_ratio);
	int n_xa = __popcll(hits);
	if (n_xa > P.max_XA_hits) { n_xa = 0; hits = 0; }
	if (n_xa > 0 && (!slots || n_xa > PW_XA_CAP)) return -1;
	if (hits >> lane & 1) {
		const WReg R = wl_get(L, lane);
		const int w2 = reg2aln_band(R.qe - R.qb, (int)(R.re - R.rb), R.truesc, P.a, P.o_del, P.e_del, P.o_ins, P.e_ins, P.w, R.w);
		AlnReq q;
		q.rb = R.rb; q.re = R.re; q.read = read; q.qb = R.qb; q.qe = R.qe; q.w2 = w2; q.truesc = R.truesc; q.pad = R.rid;
		slots[__popcll(hits & (((u64)1 << lane) - 1))] = q;
	}
	return n_xa;
}

// The lines of one read as mem_reg2sam makes them (src/bwamem.c:1015-1032 without MEM_F_ALL, no ALT hit): `lines` = the n_lines (1 ..
// SE_LINES_CAP) primary hits of at least T of the marked list L, in list order.  Line j is lane j's: its XA listing (every line's string
// is mem_gen_alt's for its own hit), MAPQ with the cap of :1029, band, request and descriptor go to slot slot0 + j of LN.desc / LN.reqs /
// LN.xa_cnt, its XA requests to LN.xa_reqs[(slot0 + j) * PW_XA_CAP ..].  The requests are laid out as [line 0, its XA entries, line 1,
// ...] from req0 on (SamDesc::req), `read` is their read, flag0 goes on every line and LN.supp_flag on the lines behind the first.
// PAIR: the read is an end of a pair — MAPQ and sub take the hit's csub (a rescued hit carries one; a single-end list has none) and the
// limits of the per-length and sub_n tables are tested per line, as pair_wave_kernel tests them for its chosen hits.
// Returns the number of requests (lines and XA entries), -1: XA entries without room for them, -2 (PAIR): a line beyond the tables.
// Every call in it is wave-uniform: the ballots of pw_xa_list stay outside divergent code.
template <bool PAIR>
__device__ __forceinline__ int wave_lines(const PairParams &P, const SeLines &LN, const WList &L, int n, u64 lines, int n_lines, int read, size_t slot0,
                                          int req0, int flag0, const double *__restrict__ ltab, int lane)
{
	int my_z = 0, my_xa = 0;
	u64 rest = lines;
	for (int j = 0; j < n_lines; ++j) {
		const int z = __ffsll((long long)rest) - 1;
		rest &= rest - 1;
		const int c = pw_xa_list(P, L, n, z, read, LN.xa_reqs ? LN.xa_reqs + (slot0 + j) * PW_XA_CAP : nullptr, lane);
		if (c < 0) return -1;
		if (lane == j) { my_z = z; my_xa = c; }
	}
	const bool mine = lane < n_lines;
	WReg R = wl_get(L, my_z);
	const int l = R.qe - R.qb > R.re - R.rb ? R.qe - R.qb : (int)(R.re - R.rb);
	if (PAIR && __ballot(mine && (l >= P.ltab_n || l <= 0 || R.sub_n >= 40))) return -2;
	int mq = mine ? mapq_se_of(P, R.score, R.sub, R.sub_n, PAIR ? R.csub : 0, l, R.frac_rep, ltab) & 0xff : 0;
	const int mq0 = __shfl(mq, 0);
	int at = mine ? 1 + my_xa : 0;   // the line's request follows the requests of the lines before it and of their XA entries
	for (int d = 1; d < SE_LINES_CAP; d <<= 1) {
		const int up = __shfl_up(at, d);
		if (lane >= d) at += up;
	}
	if (mine) {
		if (lane && !LN.keep_mapq && mq > mq0) mq = mq0;   // (:1029; no ALT hit here)
		const size_t x = slot0 + lane;
		AlnReq q;
		q.rb = R.rb; q.re = R.re; q.read = read; q.qb = R.qb; q.qe = R.qe; q.truesc = R.truesc; q.pad = 0;
		q.w2 = reg2aln_band(R.qe - R.qb, (int)(R.re - R.rb), R.truesc, P.a, P.o_del, P.e_del, P.o_ins, P.e_ins, P.w, R.w);
		LN.reqs[x] = q;
		SamDesc d;
		d.rb = R.rb; d.re = R.re; d.qb = R.qb; d.qe = R.qe; d.req = req0 + at - 1 - my_xa; d.rid = R.rid;
		d.flag = flag0 | (lane ? LN.supp_flag : 0) | my_xa << SAM_XA_SHIFT; d.mapq = mq; d.score = R.score;
		d.sub = PAIR && R.csub > R.sub ? R.csub : R.sub;   // mem_reg2aln: sub = max(sub, csub)
		LN.desc[x] = d;
		LN.xa_cnt[x] = (uint8_t)my_xa;
	}
	return __shfl(at, SE_LINES_CAP - 1);
}

} // namespace mbw
#endif
