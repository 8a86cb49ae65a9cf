// msw_kernel.hip — mate-rescue local alignment on the device: ksw_align2() as mem_matesw() calls it
// (src/bwamem_pair.c:150-177 -> src/ksw.c:321-356, kernels ksw_u8 src/ksw.c:111-237 and ksw_i16 src/ksw.c:239-319).
//
// What has to be reproduced is not textbook Smith-Waterman.  The reference runs Farrar's striped SSE2 kernel, in which a
// query of qlen bases is cut into P segments of slen = ceil(qlen / P) positions (P = 16 byte lanes when qlen * a < 250,
// else 8 word lanes) and
//   * inside the main loop F only propagates within a segment (every lane starts a row with F = 0);
//   * E(i+1,j) is computed there, from the H that main loop sees ("we disallow adjacent insertion and then
//     deletion", src/ksw.c:176) — i.e. from Hpre = max(Hdiag + s, E, Fseg), not from the final H;
//   * the lazy-F loop afterwards carries F across segment borders and only raises H.  With o_ins > 0 its early exit
//     (f - e_ins <= max(h, f) - (o_ins + e_ins) in every lane) never drops a carry that could still matter.  With o_ins = 0
//     that test holds at once: the loop ends after the first position of every segment, a carry raises that position only,
//     and what follows does NOT hold — msw_on_device (device.hip) keeps such options away from these kernels;
//   * positions qlen .. slen*P-1 are padding that scores 0 against everything, and they do take part in the row maximum;
//   * the row maximum feeds a run-length list b[] whose "consecutive row" test looks at the row stored in the last
//     entry, not at the previous row.
// All of this is observable in (score, te, qe, score2, te2), so the kernel keeps two F values per cell — Fseg (reset
// at every segment start) and Ffull (never reset) — and computes
//     Hpre = max(Hdiag + s, E, Fseg)      H = max(Hpre, Ffull)
//     E'   = max(E - e_del, Hpre - oe_del, 0)
//     F*'  = max(F* - e_ins, Hpre - oe_ins, 0)
// which, for o_ins > 0, is value-for-value what the striped kernel leaves in its H / E arrays once a row is finished (held against the
// reference under fifteen sets of scoring options by tests/test_gpu_msw_options.py; tests/msw_model.py is this recurrence in Python
// and shows the departure under o_ins = 0).  No value can
// saturate in the byte flavour (qlen * a < 250 and shift = -min(mat)); a request whose scores could reach the 8-bit
// ceiling is flagged and recomputed on the host.
//
// Mapping: one request per QUAD of lanes, 16 requests per wave, one wave per workgroup.  The query positions of a
// request are dealt to its four lanes in contiguous quarters, and the quad works as a skewed pipeline: lane j computes its
// quarter of target row i at step i + j.  What a quarter needs from its left neighbour is what the neighbour held after the
// last cell of the same row one step earlier — H(i-1) of that cell (the diagonal), both running F values and the running
// row maximum — four registers handed over with DPP quad_perm, no LDS.  Lane 3 sees the finished row: row maximum into the
// b[] scratch, best score / te / qe, the stop conditions (broadcast back through the quad).  A wave's serial length is a
// quarter of a request's and its LDS 10 KB for reads of 150 bp, so a launch of 28 000 requests gives every SIMD work and
// several waves to hide LDS latency behind.
// The row state of a position — H(i-1,k), E(i,k), the query base of position k and a segment-end flag packed in one dword
// (13 + 13 + 3 bits, bit 31) — lives in LDS as cell[kk][lane] (kk = position inside the lane's quarter), so the 64 lanes of a
// wave touch 64 consecutive dwords (no bank conflicts) and the whole DP runs out of LDS and registers.  HBM traffic is the
// target window (2 bits per row) and one u16 per row for the b[] pass.  The work is VALU-bound: ~30 integer ops per cell.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include "hip_util.h"
#include "device.h"

namespace mbw {

namespace {

#define MSW_PAD 7u

__device__ __forceinline__ int msw_base(const uint8_t *__restrict__ pac, int64_t l_pac, int64_t p)
{
	if (p >= l_pac) {
		int64_t f = (l_pac << 1) - 1 - p;
		return 3 - ((pac[f >> 2] >> ((~f & 3) << 1)) & 3);
	}
	return (pac[p >> 2] >> ((~p & 3) << 1)) & 3;
}

struct MswPassOut { int score, te, qe; };

#define MSW_QP(a, b, c, d) ((a) | (b) << 2 | (c) << 4 | (d) << 6)
template <int CTRL>
__device__ __forceinline__ int msw_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ int msw_from_lane3(int v) { return msw_dpp<MSW_QP(3, 3, 3, 3)>(v); }

// the result of a pass, which lane 3 holds, in every lane of the quad
__device__ __forceinline__ MswPassOut msw_quad_result(int gmax, int te, int qe)
{
	MswPassOut o;
	o.score = msw_from_lane3(gmax); o.te = msw_from_lane3(te); o.qe = msw_from_lane3(qe);
	return o;
}

// query code of position k of a request: the mate as it is or reverse-complemented, N = 4, beyond the read = padding
__device__ __forceinline__ uint32_t msw_code(const uint8_t *__restrict__ ms, int qlen, int is_rev, int k)
{
	if (k >= qlen) return MSW_PAD;
	if (is_rev) { const uint32_t b = ms[qlen - 1 - k]; return b < 4 ? 3 - b : 4; }
	const uint32_t c = ms[k];
	return c > 4 ? 4 : c;
}

// One striped-SW pass for the 16 requests of the wave (a quad of lanes each).  `S` positions per lane already laid out in LDS
// (query codes, H = E = 0; position k = j * S + kk sits at cell[kk * 64 + lane]), `tn` target rows, row i reads
// doubled-coordinate position t0 + i * tdir.  rows != nullptr: lane 3 writes the row maxima to rows[i * row_stride] (the b[]
// list is rebuilt from them afterwards).  The result is valid in every lane of the quad.
__device__ __forceinline__ MswPassOut msw_pass(uint32_t *cell, const MswParams &P, const uint8_t *__restrict__ pac, bool live, int S, int tn,
                                               int64_t t0, int tdir, int endsc, int sat_limit, uint16_t *rows, size_t row_stride, int *sat_hit)
{
	const int lane = threadIdx.x, j = lane & 3;
	int gmax = 0, te = -1, qe = -1;
	bool run = live && tn > 0 && S > 0;
	const int oe_del = P.o_del + P.e_del, oe_ins = P.o_ins + P.e_ins, e_del = P.e_del, e_ins = P.e_ins;
	// uniform trip count of the cell loop: the longest quarter in the wave
	int Swave = run ? S : 0;
	for (int o = 32; o; o >>= 1) Swave = max(Swave, __shfl_xor(Swave, o));
	int co_diag = 0, co_fseg = 0, co_ffull = 0, co_key = 0;   // what this lane held after its last cell of the previous step
	int tb_next = (run && j == 0) ? msw_base(pac, P.l_pac, t0) : 0;
	for (int t = 0; __any(run); ++t) {
		const int i = t - j;                                   // the row this lane works on in this step
		const bool act = run && i >= 0 && i < tn;
		const int tb = tb_next;
		if (run && i + 1 >= 0 && i + 1 < tn) tb_next = msw_base(pac, P.l_pac, t0 + (int64_t)(i + 1) * tdir);   // in flight during this step
		// scores of this row's target base against query codes 0..3 (one byte each) and 4
		const uint32_t slo = tb == 0 ? P.slo[0] : tb == 1 ? P.slo[1] : tb == 2 ? P.slo[2] : P.slo[3];
		// ... and against code 4 in byte 0 of the high half; bytes 5..7 (codes 5, 6 and the padding code 7) score 0
		const uint32_t shi = (uint32_t)(uint8_t)(tb == 0 ? P.s4[0] : tb == 1 ? P.s4[1] : tb == 2 ? P.s4[2] : P.s4[3]);
		// hand-over from the left neighbour (its state after the same row, one step ago); lane 0 starts the row
		const int ci_diag = msw_dpp<MSW_QP(0, 0, 1, 2)>(co_diag), ci_fseg = msw_dpp<MSW_QP(0, 0, 1, 2)>(co_fseg);
		const int ci_ffull = msw_dpp<MSW_QP(0, 0, 1, 2)>(co_ffull), ci_key = msw_dpp<MSW_QP(0, 0, 1, 2)>(co_key);
		int diag = j ? ci_diag : 0, fseg = j ? ci_fseg : 0, ffull = j ? ci_ffull : 0;
		uint32_t key = j ? (uint32_t)ci_key : 0u;   // (row maximum << 16) | (0xffff - first position reaching it)
		const int kbase = j * S;
		const int kmax = act ? S : 0;
		auto step = [&](uint32_t &w, int kk) {
			const int hk = w & 0x1fff;
			int e = (int)__builtin_amdgcn_ubfe(w, 13, 13);
			const uint32_t q = __builtin_amdgcn_ubfe(w, 26, 3);
			// byte q of {shi, slo}: one v_perm_b32 instead of a data-dependent branch per cell
			const int s = (int)(int8_t)__builtin_amdgcn_perm(shi, slo, q | 0x0c0c0c00u);
			const int h = max(max(diag + s, e), fseg);               // Hpre(i,k)
			key = max(key, (uint32_t)h << 16 | (uint32_t)(0xffff - (kbase + kk)));
			const int hfin = max(h, ffull);                          // H(i,k) after the lazy-F pass
			e = max(max(e - e_del, h - oe_del), 0);
			const int t2 = h - oe_ins;
			fseg = max(max(fseg - e_ins, t2), 0);
			ffull = max(max(ffull - e_ins, t2), 0);
			fseg &= ~((int)w >> 31);                                 // bit 31: last position of a segment, F restarts at 0
			diag = hk;
			w = (w & 0xfc000000u) | ((uint32_t)e << 13 | (uint32_t)hfin);
		};
		for (int k = 0; k < Swave; k += 2) {   // quarters are even (the padded query length is a multiple of 8)
			if (k < kmax) {
				uint32_t w0 = cell[k * 64 + lane], w1 = cell[(k + 1) * 64 + lane];
				step(w0, k); step(w1, k + 1);
				cell[k * 64 + lane] = w0; cell[(k + 1) * 64 + lane] = w1;
			}
		}
		if (act) { co_diag = diag; co_fseg = fseg; co_ffull = ffull; co_key = (int)key; }
		// lane 3 has just finished row i: bookkeeping of the whole row, then the verdict goes back to the quad
		int stop = 0;
		if (act && j == 3) {
			const int imax = (int)(key >> 16);
			if (rows) rows[(size_t)i * row_stride] = (uint16_t)imax;
			if (imax > gmax) {
				gmax = imax; te = i; qe = 0xffff - (int)(key & 0xffff);
				if (gmax >= sat_limit) { *sat_hit = 1; stop = 1; }
				if (gmax >= endsc) stop = 1;
			}
			if (i + 1 >= tn) stop = 1;
		}
		stop = msw_from_lane3(stop);
		if (stop) run = false;
	}
	*sat_hit = msw_from_lane3(*sat_hit);
	return msw_quad_result(gmax, te, qe);
}

// The b[] list of src/ksw.c:196-226, rebuilt from the row maxima in row order: runs of consecutive rows whose maximum reaches minsc,
// each run kept as its best row, where "consecutive" looks at the row kept for the run, not at the previous row.  The second-best hit
// (sc2, te2) is the best run whose kept row lies outside te +- ceil(score / max_sc).
struct MswRuns {
	int last_sc = -1, last_i = -1, sc2 = -1, te2 = -1, low, high, minsc;
	__device__ __forceinline__ MswRuns(int score, int te, int max_sc, int minsc_) : minsc(minsc_)
	{
		const int d = (score + max_sc - 1) / max_sc;
		low = te - d; high = te + d;
	}
	__device__ __forceinline__ void row(int i, int im)
	{
		if (im < minsc) return;
		if (last_i < 0 || last_i + 1 != i) { finish(); last_sc = im; last_i = i; }
		else if (last_sc < im) { last_sc = im; last_i = i; }
	}
	__device__ __forceinline__ void finish()   // the run in hand is complete
	{
		if (last_i >= 0 && (last_i < low || last_i > high) && last_sc > sc2) { sc2 = last_sc; te2 = last_i; }
	}
};

// score2 / te2 of request r (if `has`) into `out`, the quad working together: each lane fetches 16 of the next 64 row maxima
// (independent loads, all in flight at once), the quad parks them in its block `qblk` of 64 LDS entries and every lane applies MswRuns
// to them in row order.  All 64 lanes call it together: the trip count is the wave's longest window, and a block in which no quad has
// a row at minsc is skipped.
__device__ __forceinline__ void msw_scan_rows(uint16_t *qblk, const uint16_t *__restrict__ rows, int n_req, int r, int tlen, bool has, int minsc,
                                              int max_sc, MswRes &out)
{
	const int j = threadIdx.x & 3;
	if (!has) tlen = 0;
	MswRuns b(out.score, out.te, max_sc, minsc);
	int twave = tlen;
	for (int o = 32; o; o >>= 1) twave = max(twave, __shfl_xor(twave, o));
	for (int i0 = 0; i0 < twave; i0 += 64) {
		uint16_t v[16];
#pragma unroll
		for (int u = 0; u < 16; ++u) {
			const int i = i0 + u * 4 + j;
			v[u] = i < tlen ? rows[(size_t)i * n_req + r] : (uint16_t)0;
		}
		bool any = false;
#pragma unroll
		for (int u = 0; u < 16; ++u) {
			qblk[u * 4 + j] = v[u];
			any |= i0 + u * 4 + j < tlen && (int)v[u] >= minsc;
		}
		if (!__any(any)) continue;
		wave_lds_sync();
		const int kend = min(64, tlen - i0);
		for (int k = 0; k < kend; ++k) b.row(i0 + k, qblk[k]);
		wave_lds_sync();
	}
	b.finish();
	out.score2 = b.sc2; out.te2 = b.te2;
}

// The reverse pass of one request on its quad and the end of its record: where does the best local alignment start (KSW_XSTART,
// src/ksw.c:344-352) — the forward pass again over the reversed prefixes, query positions qe .. 0 against rows te .. 0, until the
// forward score is reached.  `second`: the request has such a pass; `cell` is laid out anew for it (layout of msw_pass).  All four
// lanes of the quad call it with the same arguments; lane 0 stores the record of a live request.
__device__ __forceinline__ void msw_reverse_one(uint32_t *cell, const MswParams &P, const uint8_t *__restrict__ pac, bool live, bool second,
                                                const MswReq &rq, int qlen, const uint8_t *__restrict__ ms, MswRes &out, MswRes *__restrict__ res, int r)
{
	const int lane = threadIdx.x, j = lane & 3;
	const bool byte_flavour = qlen * P.a < 250;
	const int PP = byte_flavour ? 16 : 8;
	const int sat_limit = byte_flavour ? 255 - P.shift : 0x10000;
	int qlen2 = second ? out.qe + 1 : 0;
	if (second && out.qe >= qlen) qlen2 = 0;   // cannot happen (the maximum of a row is reached on a real base first); stay in bounds
	const int slen2 = (qlen2 + PP - 1) / PP, npos2 = slen2 * PP, S2 = npos2 >> 2;
	if (qlen2 > 0)   // the codes of positions qe .. 0, padded, dealt to the quad; H and E cleared
		for (int kk = 0; kk < S2; ++kk) {
			const int k = j * S2 + kk;
			const uint32_t c = k < qlen2 ? msw_code(ms, qlen, rq.is_rev, qlen2 - 1 - k) : MSW_PAD;
			cell[kk * 64 + lane] = c << 26 | ((k + 1) % slen2 == 0 ? 0x80000000u : 0u);
		}
	int sat2 = 0;
	const MswPassOut g = msw_pass(cell, P, pac, qlen2 > 0, S2, out.te + 1, rq.rb + out.te, -1, out.score, sat_limit, nullptr, 0, &sat2);
	if (qlen2 > 0 && g.score == out.score) { out.tb = out.te - g.te; out.qb = out.qe - g.qe; }
	if (second && qlen2 == 0) out.flags = 1;
	if (sat2) out.flags = 1;
	if (live && j == 0) res[r] = out;
}

// What follows the forward pass of one request in msw_kernel: score2 / te2 from the row maxima, the reverse pass, the record.  All
// four lanes of the quad call it with the same arguments.
__device__ __forceinline__ void msw_tail(uint32_t *cell, const MswParams &P, const uint8_t *__restrict__ pac, bool live, const MswReq &rq, int qlen,
                                         const uint8_t *__restrict__ ms, int r, int n_req, MswPassOut f, int sat, uint16_t *__restrict__ rows,
                                         MswRes *__restrict__ res)
{
	const int j = threadIdx.x & 3;
	const int tlen = (int)(rq.re - rq.rb);
	const int minsc = P.min_seed_len * P.a;              // KSW_XSUBO | min_seed_len * a
	MswRes out;
	out.score = f.score; out.te = f.te; out.qe = f.qe; out.score2 = -1; out.te2 = -1; out.tb = -1; out.qb = -1; out.flags = sat;
	// lane 0 walks the rows on its own (the quad's own stores to rows[]: same wave, same addresses, program order; the forward pass
	// never stops early — no KSW_XSTOP, no saturation — so all tlen rows are there).  A window whose best row stays below minsc has no
	// row for b[] at all — nine rescue windows in ten of a repeat read's anchors — and is not walked.
	if (live && j == 0 && !sat && f.te >= 0 && f.score >= minsc) {
		MswRuns b(f.score, f.te, P.max_sc, minsc);
		for (int i = 0; i < tlen; ++i) b.row(i, rows[(size_t)i * n_req + r]);
		b.finish();
		out.score2 = b.sc2; out.te2 = b.te2;
	}
	msw_reverse_one(cell, P, pac, live, live && !sat && f.score >= minsc && f.qe >= 0 && f.te >= 0, rq, qlen, ms, out, res, r);
}

// list: the requests this launch works on (null: all of them, in order)
__global__ __launch_bounds__(64) void msw_kernel(MswParams P, int n_work, int n_req, const int *__restrict__ list, const MswReq *__restrict__ req,
                                                 const uint8_t *__restrict__ seq, const int64_t *__restrict__ off, const int *__restrict__ lens,
                                                 const uint8_t *__restrict__ pac, MswRes *__restrict__ res, uint16_t *__restrict__ rows)
{
	extern __shared__ uint32_t cell[];   // [positions of a quarter][64 lanes]
	const int lane = threadIdx.x, j = lane & 3;
	const int slot = blockIdx.x * 16 + (lane >> 2);
	const bool live = slot < n_work;
	const int r = live ? (list ? list[slot] : slot) : 0;
	MswReq rq;
	rq.rb = rq.re = 0; rq.read = 0; rq.is_rev = 0;
	if (live) rq = req[r];
	const int qlen = live ? lens[rq.read] : 0;
	const int tlen = (int)(rq.re - rq.rb);
	const bool byte_flavour = qlen * P.a < 250;          // KSW_XBYTE as mem_matesw sets it
	const int PP = byte_flavour ? 16 : 8;
	const int slen = (qlen + PP - 1) / PP;
	const int npos = slen * PP, S = npos >> 2;           // positions per lane (npos is a multiple of 8)
	const uint8_t *ms = seq + (live ? off[rq.read] : 0);
	// query codes -> LDS (reverse-complemented for the orientations that need it), H = E = 0
	if (live)
		for (int kk = 0; kk < S; ++kk) {
			const int k = j * S + kk;
			cell[kk * 64 + lane] = msw_code(ms, qlen, rq.is_rev, k) << 26 | ((k + 1) % slen == 0 ? 0x80000000u : 0u);
		}
	const int sat_limit = byte_flavour ? 255 - P.shift : 0x10000;
	int sat = 0;
	MswPassOut f = msw_pass(cell, P, pac, live, S, tlen, rq.rb, 1, 0x10000, sat_limit, live ? rows + r : nullptr, (size_t)n_req, &sat);
	msw_tail(cell, P, pac, live, rq, qlen, ms, r, n_req, f, sat, rows, res);
}

// ---------------------------------------------------------------------------------------------------------------------
// msw2_kernel: TWO requests of the same mate in the same orientation per quad — the rescue windows of a repeat read's
// anchors: 50 windows for one mate — in the byte flavour (qlen * a < 250: every H, E, F below 256).  The forward pass (the whole
// window; four fifths of the work) runs both alignments in the two 16-bit halves of every register: v_pk_add_i16 / v_pk_sub_i16 /
// v_pk_max_i16 on {H, E, Fseg, Ffull}, 13 vector instructions per cell instead of 25.  What makes that cheap is what the two share:
// the query (one set of codes and segment flags: a dword of eight 4-bit codes per eight positions, read once per eight cells) and
// the row loop; what differs per row — the two target bases — selects one of 16 rows of a 128-entry table in LDS that holds, per
// query code, the two substitution scores as a packed pair.  The row state of a position is one dword: H and E of both alignments
// as four bytes, unpacked and repacked with one v_perm_b32 each.  Row maxima, best cell, saturation are kept per alignment as in
// msw_pass.  The kernel ends with the forward pass: an alignment that needs no second pass gets its final record here, the others
// (score >= minsc, not saturated) get a class byte; a sort makes lists of them and msw_rev2_kernel runs the b[] scan and the reverse
// pass densely behind it, two of a class per quad.
// ---------------------------------------------------------------------------------------------------------------------
typedef short msw_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ msw_s2 s2_of(uint32_t v) { return __builtin_bit_cast(msw_s2, v); }
__device__ __forceinline__ uint32_t u_of(msw_s2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ msw_s2 s2_max(msw_s2 a, msw_s2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ msw_s2 s2_splat(int v) { msw_s2 r; r.x = (short)v; r.y = (short)v; return r; }
typedef unsigned short msw_u2 __attribute__((ext_vector_type(2)));
// max(a - b, 0) per half for values that are never negative: v_pk_sub_u16 with the clamp bit, no separate maximum with 0
__device__ __forceinline__ msw_s2 s2_sub0(msw_s2 a, msw_s2 b)
{
	return __builtin_bit_cast(msw_s2, __builtin_elementwise_sub_sat(__builtin_bit_cast(msw_u2, a), __builtin_bit_cast(msw_u2, b)));
}

// scores of target base t against query codes 0..3 / code 4, without indexing the parameter block at run time (no scratch copy of it)
__device__ __forceinline__ uint32_t msw_slo(const MswParams &P, int t) { return t == 0 ? P.slo[0] : t == 1 ? P.slo[1] : t == 2 ? P.slo[2] : P.slo[3]; }
__device__ __forceinline__ int msw_s4(const MswParams &P, int t) { return t == 0 ? P.s4[0] : t == 1 ? P.s4[1] : t == 2 ? P.s4[2] : P.s4[3]; }

// The class of an alignment that needs the second pass, one byte per request (0: it needs none): the segment length of
// its reverse pass, slen2 = ceil((qe + 1) / 16) = 1..16 — which fixes the positions per lane, the segment ends and the hand-over points
// of a quad, so that two alignments of one class can share a quad whatever reads they belong to — and the score class of
// the forward score (below 40 a, below 80 a, from there on: rows ~ score / a), which keeps a wave's lockstep length uniform.  A larger class is a longer pass.
__device__ __forceinline__ int msw_rev_class(int score, int qe, int a)
{
	const int sb = score >= 80 * a ? 2 : score >= 40 * a ? 1 : 0;
	return 1 + (qe >> 4) * 3 + sb;
}

// ---- the packed arithmetic: two alignments of a quad in the 16-bit halves of every register (msw2_kernel, msw_rev2_kernel) ----
struct Msw2Gap {
	msw_s2 oe_del, oe_ins, e_del, e_ins;
	__device__ __forceinline__ explicit Msw2Gap(const MswParams &P)
		: oe_del(s2_splat(P.o_del + P.e_del)), oe_ins(s2_splat(P.o_ins + P.e_ins)), e_del(s2_splat(P.e_del)), e_ins(s2_splat(P.e_ins)) {}
};

// One cell of the recurrence at the top of this file, for both alignments: hd = H(i-1,k), e = E(i,k) (becomes E(i+1,k)), s = the two
// substitution scores; diag / fseg / ffull run along the row.  H(i,k) is returned.  H, E, both F and h = Hpre are never negative, so
// "max(x - c, 0)" is one saturating subtraction.  mblk: the maximum of the block of eight cells and the first of them to reach it as
// one 16-bit key per alignment, h * 256 + 7 - u (u = the cell's place in the block; c256: see msw2_pass_lds).  seg_end(F_seg): what
// is left of F_seg behind this cell — nothing behind the last position of a segment.
template <class SegEnd>
__device__ __forceinline__ msw_s2 msw2_recur(msw_s2 hd, msw_s2 &e, msw_s2 s, int u, const Msw2Gap &G, msw_u2 c256, msw_s2 &diag, msw_s2 &fseg,
                                             msw_s2 &ffull, msw_u2 &mblk, SegEnd seg_end)
{
	const msw_s2 h = s2_max(s2_max(diag + s, e), fseg);                    // Hpre(i, k) of both
	const msw_u2 rel = {(unsigned short)(7 - u), (unsigned short)(7 - u)};
	mblk = __builtin_elementwise_max(mblk, __builtin_bit_cast(msw_u2, h) * c256 + rel);
	const msw_s2 hfin = s2_max(h, ffull);
	e = s2_max(s2_sub0(e, G.e_del), s2_sub0(h, G.oe_del));
	const msw_s2 t2 = s2_sub0(h, G.oe_ins);
	fseg = seg_end(s2_max(s2_sub0(fseg, G.e_ins), t2));
	ffull = s2_max(s2_sub0(ffull, G.e_ins), t2);
	diag = hd;
	return hfin;
}

// The same cell with the row state in one dword, as it lies in LDS: w = H, E of both as four bytes, unpacked and repacked with one
// v_perm_b32 each.  The last position of a segment: seg_end, a wave-uniform fact (UNI), or bit 3 of entry u of cd.
template <bool UNI>
__device__ __forceinline__ void msw2_cell(uint32_t &w, msw_s2 s, uint32_t cd, int u, bool seg_end, const Msw2Gap &G, msw_u2 c256, msw_s2 &diag,
                                          msw_s2 &fseg, msw_s2 &ffull, msw_u2 &mblk)
{
	const msw_s2 hd = s2_of(__builtin_amdgcn_perm(0u, w, 0x0c020c00u));   // H_A | H_B << 16   (row i - 1)
	msw_s2 e = s2_of(__builtin_amdgcn_perm(0u, w, 0x0c030c01u));          // E_A | E_B << 16
	const msw_s2 hfin = msw2_recur(hd, e, s, u, G, c256, diag, fseg, ffull, mblk, [&](msw_s2 f) {
		if constexpr (UNI) return seg_end ? s2_splat(0) : f;
		else return s2_of(u_of(f) & ~(uint32_t)__builtin_amdgcn_sbfe((int)cd, 4 * u + 3, 1));   // -1 at the last position of a segment
	});
	w = __builtin_amdgcn_perm(u_of(e), u_of(hfin), 0x06020400u);            // bytes: H_A, E_A, H_B, E_B
}

// The target base of row i of a window of tn rows at rb — read upwards, or downwards from its last row (a reverse pass: row i is
// rb + tn - 1 - i).  Rows past the end of the shorter window of a quad: its last row again, results unused.
__device__ __forceinline__ int msw2_base_at(const uint8_t *__restrict__ pac, int64_t l_pac, int64_t rb, int tn, int i, bool down)
{
	const int ii = i < tn ? i : tn - 1;
	return ii >= 0 ? msw_base(pac, l_pac, rb + (down ? tn - 1 - ii : ii)) : 0;
}

// What a lane holds after its last cell of a row and hands to its right neighbour: the diagonal, both F and the row's key so far
struct Msw2Carry {
	uint32_t diag = 0, fseg = 0, ffull = 0, key = 0;
	__device__ __forceinline__ Msw2Carry from_left() const   // the left neighbour's, one step ago (every lane takes part: DPP)
	{
		Msw2Carry ci;
		ci.diag = (uint32_t)msw_dpp<MSW_QP(0, 0, 1, 2)>((int)diag); ci.fseg = (uint32_t)msw_dpp<MSW_QP(0, 0, 1, 2)>((int)fseg);
		ci.ffull = (uint32_t)msw_dpp<MSW_QP(0, 0, 1, 2)>((int)ffull);
		ci.key = (uint32_t)msw_dpp<MSW_QP(0, 0, 1, 2)>((int)key);
		return ci;
	}
	// the start of lane j's quarter of a row: lane 0 starts the row itself
	__device__ __forceinline__ void open(int j, msw_s2 &d, msw_s2 &fs, msw_s2 &ff, msw_u2 &k) const
	{
		d = s2_of(j ? diag : 0u); fs = s2_of(j ? fseg : 0u); ff = s2_of(j ? ffull : 0u);
		k = __builtin_bit_cast(msw_u2, j ? key : 0u);
	}
	__device__ __forceinline__ void close(msw_s2 d, msw_s2 fs, msw_s2 ff, msw_u2 k)
	{
		diag = u_of(d); fseg = u_of(fs); ffull = u_of(ff); key = __builtin_bit_cast(uint32_t, k);
	}
};

// One alignment of a quad as lane 3 follows it over the rows of a pass: the best cell so far, and whether it is finished ahead of
// its rows — at the 8-bit ceiling (sat), or with a row that raises the maximum to stop_score (KSW_XSTOP; INT_MAX: never)
struct Msw2Half {
	int gmax = 0, te = -1, qe = -1;
	bool done = false;
	__device__ __forceinline__ void take(int imax, int pos, int i, int sat_limit, int stop_score)   // row i: maximum imax, first at position pos
	{
		if (imax > gmax) {
			gmax = imax; te = i; qe = pos;
			if (gmax >= sat_limit || gmax >= stop_score) done = true;
		}
	}
	// (the maximum moves in take() alone and stays once it is there: no flag of its own to carry over the rows)
	__device__ __forceinline__ int sat(int sat_limit) const { return gmax >= sat_limit; }
};

// Lane 3's verdict on row i of both alignments.  keyAB: per alignment the row maximum * 256 + (255 - first position reaching it) —
// the byte flavour has h < 250 and at most 256 positions.  Alignment X takes part while it has rows (tnX of them) and is not done;
// KEEP_ROWS: its row maxima go to rowsX for the b[] scan, one per row at stride n_req.  True: neither has anything left to do.
template <bool KEEP_ROWS>
__device__ __forceinline__ bool msw2_row_verdict(Msw2Half &A, Msw2Half &B, uint32_t keyAB, int i, int tnA, int tnB, int sat_limit, int stopA, int stopB,
                                                 uint16_t *rowsA, uint16_t *rowsB, int n_req)
{
	auto half = [&](Msw2Half &X, uint32_t key, int tn, int stop_score, uint16_t *rows) -> bool {
		if (i < tn && !X.done) {
			const int imax = (int)(key >> 8 & 0xff);
			if constexpr (KEEP_ROWS) rows[(size_t)i * n_req] = (uint16_t)imax;
			X.take(imax, 255 - (int)(key & 0xff), i, sat_limit, stop_score);
		}
		return i + 1 >= tn || X.done;
	};
	const bool a = half(A, keyAB, tnA, stopA, rowsA), b = half(B, keyAB >> 16, tnB, stopB, rowsB);
	return a && b;
}

// The query side of a packed pass with the row state in LDS — where a cell's two scores come from:
//   row(ta, tb)    the target bases of the row in hand
//   block(c, on)   the code word(s) of the lane's block c of eight positions (eight 4-bit entries: query code, bit 3 = end of a segment)
//   flags()        the code word that carries the segment ends
//   score(u)       the two scores of position u of the block, as a packed pair
// Msw2SharedQuery (msw2_kernel): both alignments have the same query — one code set, and per pair of target bases a row of eight
// packed pairs in a 128-entry table.  Msw2OwnQueries (msw_rev2_kernel): each has its own — two code sets (the segment flags in A's
// alone) and two tables of four rows, A's with the score in the low half and B's in the high half, or'ed together.
struct Msw2SharedQuery {
	const uint32_t *codes, *stab, *srow;
	uint32_t cd;
	__device__ __forceinline__ void row(int ta, int tb) { srow = stab + ((ta << 2 | tb) << 3); }
	__device__ __forceinline__ void block(int c, bool on) { cd = on ? codes[c * 64 + (int)threadIdx.x] : 0u; }
	__device__ __forceinline__ uint32_t flags() const { return cd; }
	__device__ __forceinline__ msw_s2 score(int u) const
	{
		uint32_t q = __builtin_amdgcn_ubfe(cd, 4 * u, 3);
		asm("" : "+v"(q));   // (opaque: v_bfe_u32 + v_lshl_add_u32 for the table address; folded, it is shift + and + add)
		return s2_of(srow[q]);
	}
};
struct Msw2OwnQueries {
	const uint32_t *codesA, *codesB, *tabA, *tabB, *srowA, *srowB;
	uint32_t cda, cdb;
	__device__ __forceinline__ void row(int ta, int tb) { srowA = tabA + (ta << 3); srowB = tabB + (tb << 3); }
	__device__ __forceinline__ void block(int c, bool on)
	{
		const int lane = threadIdx.x;
		cda = on ? codesA[c * 64 + lane] : 0u; cdb = on ? codesB[c * 64 + lane] : 0u;
	}
	__device__ __forceinline__ uint32_t flags() const { return cda; }
	__device__ __forceinline__ msw_s2 score(int u) const
	{
		uint32_t qA = __builtin_amdgcn_ubfe(cda, 4 * u, 3), qB = __builtin_amdgcn_ubfe(cdb, 4 * u, 3);
		asm("" : "+v"(qA));
		asm("" : "+v"(qB));
		return s2_of(srowA[qA] | srowB[qB]);
	}
};

// One packed pass for the 16 quads of the wave with the row state in LDS: the skewed pipeline of msw_pass, two alignments per quad.
// cell[kk * 64 + lane]: H, E of both at position kk of the lane's S (cleared by the caller); tn rows (the longer of the two);
// base(half, i): the target base of row i of alignment `half`; lane 3 gives verdict(i, keyAB) on every finished row, true = the quad
// stops.  UNI: every live quad of the wave has segment length slen_u, the ends are known to the scalar unit; else bit 3 of the codes
// decides — two copies of the pass, so that neither has a branch per cell.
template <bool UNI, class Query, class Base, class Verdict>
__device__ __forceinline__ void msw2_pass_lds(uint32_t *cell, const MswParams &P, bool live, int S, int tn, int slen_u, Query query, Base base,
                                              Verdict verdict)
{
	const int lane = threadIdx.x, j = lane & 3;
	bool run = live && tn > 0 && S > 0;
	const Msw2Gap G(P);
	int Swave = run ? S : 0;   // uniform trip count of the cell loop: the longest quarter in the wave
	for (int o = 32; o; o >>= 1) Swave = max(Swave, __shfl_xor(Swave, o));
	Msw2Carry co;
	int ta_next = (run && j == 0) ? base(0, 0) : 0, tb_next = (run && j == 0) ? base(1, 0) : 0;
	for (int t = 0; __any(run); ++t) {
		const int i = t - j;                                   // the row this lane works on in this step
		const bool act = run && i >= 0 && i < tn;
		const int ta = ta_next, tb = tb_next;
		if (run && i + 1 >= 0 && i + 1 < tn) { ta_next = base(0, i + 1); tb_next = base(1, i + 1); }   // in flight during this step
		query.row(ta, tb);
		const Msw2Carry ci = co.from_left();
		msw_s2 diag, fseg, ffull;
		msw_u2 key;
		ci.open(j, diag, fseg, ffull, key);
		// the key of a cell is taken relative to its block of eight (one packed multiply-add with constants and one packed maximum per
		// cell), the block's offset is added once per block
		msw_u2 c256 = {256, 256};
		asm volatile("" : "+v"(c256));   // (opaque: h * 256 + rel is to be one v_pk_mad_u16, not a shift and an or)
		msw_u2 poscv = {(unsigned short)(248 - j * S), (unsigned short)(248 - j * S)};   // 255 - 7 - (first position of the block)
		const int kmax = act ? S : 0;
		int seg_pos = 0;   // position inside the segment (a lane's quarter is four whole segments: the same in every lane)
		const msw_u2 eight = {8, 8};
		for (int c = 0; c * 8 < Swave; ++c, poscv -= eight) {
			query.block(c, c * 8 < kmax);
			msw_u2 mblk = {0, 0};
#pragma unroll
			for (int u = 0; u < 8; u += 2) {   // (quarters are even)
				const int k = c * 8 + u;
				bool end0 = false, end1 = false;
				if constexpr (UNI) {
					end0 = ++seg_pos == slen_u; if (end0) seg_pos = 0;
					end1 = ++seg_pos == slen_u; if (end1) seg_pos = 0;
				}
				if (k < kmax) {
					uint32_t w0 = cell[k * 64 + lane], w1 = cell[(k + 1) * 64 + lane];
					msw2_cell<UNI>(w0, query.score(u), query.flags(), u, end0, G, c256, diag, fseg, ffull, mblk);
					msw2_cell<UNI>(w1, query.score(u + 1), query.flags(), u + 1, end1, G, c256, diag, fseg, ffull, mblk);
					cell[k * 64 + lane] = w0; cell[(k + 1) * 64 + lane] = w1;
				}
			}
			if (c * 8 < kmax) key = __builtin_elementwise_max(key, mblk + poscv);
		}
		if (act) co.close(diag, fseg, ffull, key);
		int stop = 0;
		if (act && j == 3) stop = verdict(i, __builtin_bit_cast(uint32_t, key));
		stop = msw_from_lane3(stop);
		if (stop) run = false;
	}
}

// cls[n_req] (zeroed before the launch): the class of every alignment that msw_rev2_kernel / msw_tail_kernel completes
//
// SLEN = 0: the general form — the row state in LDS, any segment length, the lengths of a wave may differ.
// SLEN > 0: every work item of the launch has that segment length (launch_msw sorts them), so a lane's S = 4 SLEN positions are a
// compile-time fact: the state words and the code words are register arrays, the cell loop is unrolled in full, a segment ends where
// (kk + 1) % SLEN == 0 (F_seg restarts by assignment) and the three skew steps without a row are one branch around the sweep.  LDS
// then holds the score table alone, and the eight lookups of a block are issued ahead of the block's arithmetic.  H and E of a position
// are two packed 16-bit registers (TWO: no v_perm_b32 to unpack and repack them) where that leaves three waves per SIMD or measured
// faster with two (SLEN <= 13), else four bytes in one register as in LDS (SLEN = 16: 146 instead of 206 VGPRs) — DESIGN 4.4.
template <int SLEN>
__global__ __launch_bounds__(64) void msw2_kernel(MswParams P, int n_pairs, int n_req, const int *__restrict__ pairs, const MswReq *__restrict__ req,
                                                  const uint8_t *__restrict__ seq, const int64_t *__restrict__ off, const int *__restrict__ lens,
                                                  const uint8_t *__restrict__ pac, MswRes *__restrict__ res, uint16_t *__restrict__ rows, int s_max,
                                                  uint8_t *__restrict__ cls)
{
	constexpr bool REGS = SLEN > 0, TWO = REGS && SLEN < 16;
	extern __shared__ uint32_t lds2[];
	uint32_t *cell = lds2;                                   // [s_max][64]: H_A, E_A, H_B, E_B as bytes
	uint32_t *codes = lds2 + (size_t)s_max * 64;             // [(s_max + 7) / 8][64]: eight 4-bit entries per dword: query code, bit 3 = end of a segment
	uint32_t *stab = REGS ? lds2 : codes + (size_t)((s_max + 7) >> 3) * 64;   // [16][8]: (target base A, target base B) x query code -> the two scores, packed
	const int lane = threadIdx.x, j = lane & 3;
	for (int e = lane; e < 128; e += 64) {
		const int ta = e >> 5, tb = (e >> 3) & 3, q = e & 7;
		const int sa = q < 4 ? (int)(int8_t)(msw_slo(P, ta) >> (8 * q)) : q == 4 ? msw_s4(P, ta) : 0;
		const int sb = q < 4 ? (int)(int8_t)(msw_slo(P, tb) >> (8 * q)) : q == 4 ? msw_s4(P, tb) : 0;
		stab[e] = (uint32_t)(uint16_t)(int16_t)sa | (uint32_t)(uint16_t)(int16_t)sb << 16;
	}
	const int slot = blockIdx.x * 16 + (lane >> 2);
	const bool live = slot < n_pairs;
	// (rB < 0: a request without a partner rides alone — its own launch of a few hundred waves would be as long as one wave's walk
	// through a window, behind this one)
	const int rA = live ? pairs[2 * slot] : 0, rB = live ? pairs[2 * slot + 1] : -1;
	const bool hasB = rB >= 0;
	MswReq qa, qb;
	qa.rb = qa.re = 0; qa.read = 0; qa.is_rev = 0; qb = qa;
	if (live) { qa = req[rA]; if (hasB) qb = req[rB]; else { qb = qa; qb.re = qb.rb; } }
	const int qlen = live ? lens[qa.read] : 0;
	const int tnA = (int)(qa.re - qa.rb), tnB = (int)(qb.re - qb.rb);
	const int slen = (qlen + 15) / 16, npos = slen * 16, S = npos >> 2;   // byte flavour: 16 segments
	const uint8_t *ms = seq + (live ? off[qa.read] : 0);
	// the register form's state: RS positions of this lane, and their query codes as byte offsets into a row of the score table
	// (code * 4, four to a dword: the address of a lookup is one v_add_u32 with a byte select; no segment flags: the ends are known to
	// the compiler)
	constexpr int RS = REGS ? 4 * SLEN : 1, RC = RS / 4 + (RS % 4 != 0);
	uint32_t st0[RS], st1[TWO ? RS : 1], cdreg[RC];
	if constexpr (REGS) {
#pragma unroll
		for (int kk = 0; kk < RS; ++kk) st0[kk] = 0;
#pragma unroll
		for (int kk = 0; kk < (TWO ? RS : 1); ++kk) st1[kk] = 0;
#pragma unroll
		for (int c = 0; c < RC; ++c) {
			uint32_t cd = 0;
#pragma unroll
			for (int u = 0; u < 4; ++u) cd |= msw_code(ms, qlen, qa.is_rev, j * RS + c * 4 + u) << (8 * u + 2);   // (not live: qlen = 0, padding)
			cdreg[c] = cd;
		}
	} else if (live) {
		for (int kk = 0; kk < S; ++kk) cell[kk * 64 + lane] = 0;
		for (int c = 0; c * 8 < S; ++c) {
			uint32_t cd = 0;
			for (int u = 0; u < 8 && c * 8 + u < S; ++u) {
				const int k = j * S + c * 8 + u;
				cd |= (msw_code(ms, qlen, qa.is_rev, k) | ((k + 1) % slen == 0 ? 8u : 0u)) << (4 * u);
			}
			codes[c * 64 + lane] = cd;
		}
	}
	wave_lds_sync();
	const int sat_limit = 255 - P.shift;
	// ---- the forward pass of both: every row of the longer window (no KSW_XSTOP), the row maxima kept for the b[] scan ----
	const int tn = tnA > tnB ? tnA : tnB;
	Msw2Half hA, hB;
	uint16_t *rowsA = rows + rA, *rowsB = rows + (hasB ? rB : rA);
	auto base = [&](int half, int i) -> int {
		return half ? msw2_base_at(pac, P.l_pac, qb.rb, tnB, i, false) : msw2_base_at(pac, P.l_pac, qa.rb, tnA, i, false);
	};
	auto verdict = [&](int i, uint32_t keyAB) -> bool {
		return msw2_row_verdict<true>(hA, hB, keyAB, i, tnA, tnB, sat_limit, INT_MAX, INT_MAX, rowsA, rowsB, n_req);
	};
	if constexpr (REGS) {
		// The pass of msw2_pass_lds with the state in registers: the recurrence, the order of the cells and every key are the same.
		bool run = live && tn > 0;
		const Msw2Gap G(P);
		Msw2Carry co;
		int ta_next = (run && j == 0) ? base(0, 0) : 0, tb_next = (run && j == 0) ? base(1, 0) : 0;
		const msw_u2 posc0 = {(unsigned short)(248 - j * RS), (unsigned short)(248 - j * RS)};   // 255 - 7 - (first position of the lane)
		for (int t = 0; __any(run); ++t) {
			const int i = t - j;
			const bool act = run && i >= 0 && i < tn;
			const int ta = ta_next, tb = tb_next;
			if (run && i + 1 >= 0 && i + 1 < tn) { ta_next = base(0, i + 1); tb_next = base(1, i + 1); }
			const uint32_t *srow = stab + ((ta << 2 | tb) << 3);
			const Msw2Carry ci = co.from_left();
			if (act) {   // (the skew steps in which a lane has no row: one branch, not a select per cell)
				msw_s2 diag, fseg, ffull;
				msw_u2 key;
				ci.open(j, diag, fseg, ffull, key);
				msw_u2 c256 = {256, 256};
				asm volatile("" : "+v"(c256));
				// the score lookups of a block depend on the codes and the row's two bases only: all of a block's in flight ahead of its
				// arithmetic, the next block's behind this one's
				auto lookups = [&](int c, uint32_t *sv) {
#pragma unroll
					for (int u = 0; u < 8 && c * 8 + u < RS; ++u)
						sv[u] = *(const uint32_t *)((const char *)srow + __builtin_amdgcn_ubfe(cdreg[(c * 8 + u) >> 2], 8 * (u & 3), 8));
					__builtin_amdgcn_sched_barrier(0);   // (the reads stay ahead of the arithmetic they were issued for)
				};
				auto step = [&](int kk, int u, uint32_t sq, msw_u2 &mblk) {
					const bool seg_end = (kk + 1) % SLEN == 0;   // (known to the compiler: F_seg restarts by assignment)
					if constexpr (TWO) {
						msw_s2 e = s2_of(st1[kk]);
						st0[kk] = u_of(msw2_recur(s2_of(st0[kk]), e, s2_of(sq), u, G, c256, diag, fseg, ffull, mblk,
						                          [&](msw_s2 f) { return seg_end ? s2_splat(0) : f; }));
						st1[kk] = u_of(e);
					} else msw2_cell<true>(st0[kk], s2_of(sq), 0u, u, seg_end, G, c256, diag, fseg, ffull, mblk);
				};
				constexpr int NB = (RS + 7) / 8;   // blocks of eight cells, the last one may be half a block
				// (the code words are opaque once per row, in place: else the RS byte selects are hoisted into RS registers held over the rows)
#pragma unroll
				for (int c = 0; c < RC; ++c) asm volatile("" : "+v"(cdreg[c]));
				uint32_t sv[2][8];
				lookups(0, sv[0]);
#pragma unroll
				for (int c = 0; c < NB; ++c) {
					if (c + 1 < NB) lookups(c + 1, sv[(c + 1) & 1]);
					msw_u2 mblk = {0, 0};
#pragma unroll
					for (int u = 0; u < 8 && c * 8 + u < RS; ++u) step(c * 8 + u, u, sv[c & 1][u], mblk);
					const msw_u2 blk0 = {(unsigned short)(8 * c), (unsigned short)(8 * c)};
					key = __builtin_elementwise_max(key, mblk + (posc0 - blk0));
				}
				co.close(diag, fseg, ffull, key);
			}
			int stop = 0;
			if (act && j == 3) stop = verdict(i, co.key);
			stop = msw_from_lane3(stop);
			if (stop) run = false;
		}
	} else {
		// the segment length when every live quad of the wave has the same one — the rule: the reads of a chunk are of one length —
		// else 0: the flags in the codes decide
		int slen_u = 0;
		const unsigned long long lv = __builtin_amdgcn_ballot_w64(live);
		if (lv) {
			const int first = __builtin_amdgcn_readlane(slen, __ffsll((long long)lv) - 1);
			slen_u = __builtin_amdgcn_ballot_w64(live && slen != first) ? 0 : first;
		}
		const Msw2SharedQuery query = {codes, stab, stab, 0u};
		if (slen_u > 0) msw2_pass_lds<true>(cell, P, live, S, tn, slen_u, query, base, verdict);
		else msw2_pass_lds<false>(cell, P, live, S, tn, slen_u, query, base, verdict);
	}
	const MswPassOut fA = msw_quad_result(hA.gmax, hA.te, hA.qe), fB = msw_quad_result(hB.gmax, hB.te, hB.qe);
	const int satA = msw_from_lane3(hA.sat(sat_limit)), satB = msw_from_lane3(hB.sat(sat_limit));
	// Every alignment gets its record as msw_tail would leave it without a second pass (lane 0: A, lane 1: B).  One that reaches minsc
	// unsaturated needs the b[] scan and the reverse pass: it gets its class byte, from which the sort kernels below make the lists of
	// msw_rev2_kernel, which completes the record.  No list is appended to here: the lists are a function of the results alone.
	const int minsc = P.min_seed_len * P.a;
	const bool mineA = live && j == 0, mineB = live && hasB && j == 1;
	const MswPassOut f = j == 0 ? fA : fB;
	const int sat = j == 0 ? satA : satB;
	const bool tail = (mineA || mineB) && !sat && f.score >= minsc && f.qe >= 0 && f.te >= 0;
	if (mineA || mineB) {
		MswRes out;
		out.score = f.score; out.te = f.te; out.qe = f.qe; out.score2 = -1; out.te2 = -1; out.tb = -1; out.qb = -1; out.flags = sat;
		res[j == 0 ? rA : rB] = out;
		if (tail) cls[j == 0 ? rA : rB] = (uint8_t)msw_rev_class(f.score, f.qe, P.a);   // (qe < qlen <= 249: slen2 <= 16)
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// The lists of the second pass: a stable counting sort of the requests by class byte, the largest class (the longest pass) first, in
// three small kernels without atomics — per block of MSW_SORT_CHUNK requests a histogram; one wave that turns the histograms into
// every block's first place per class and the class offsets; the scatter.  A wave ranks its 64 requests with one ballot per class
// present, lane c - 1 keeps the count of class c.  What comes out, in d_tail (msw_tail_ints):
//   off[o], o = 0..MSW_NCLS: where the members of class MSW_NCLS - o start in sorted[] (off[MSW_NCLS]: how many there are)
//   ioff[o]: the same in work items of msw_rev2_kernel: consecutive members of a class are a pair, an odd last one rides alone
//   sorted[]: the request indices, every class in request order
// ---------------------------------------------------------------------------------------------------------------------
template <bool SCATTER>
__global__ __launch_bounds__(64) void msw_cls_sort_kernel(int n_req, const uint8_t *__restrict__ cls, int *__restrict__ hist, const int *__restrict__ off,
                                                          int *__restrict__ sorted)
{
	const int lane = threadIdx.x;
	const int k0 = blockIdx.x * MSW_SORT_CHUNK, k1 = min(n_req, k0 + MSW_SORT_CHUNK);
	// lane c - 1: how many of class c so far (histogram), or where the next one of class c goes (scatter)
	int mine = 0;
	if (SCATTER && lane < MSW_NCLS) mine = off[MSW_NCLS - 1 - lane] + hist[(size_t)blockIdx.x * MSW_NCLS + lane];
	for (int kb = k0; kb < k1; kb += 64) {
		const int k = kb + lane;
		const int c = k < k1 ? (int)cls[k] : 0;
		unsigned long long todo = __builtin_amdgcn_ballot_w64(c > 0 && c <= MSW_NCLS);
		while (todo) {
			const int cl = __shfl(c, __ffsll((long long)todo) - 1);
			const unsigned long long m = __builtin_amdgcn_ballot_w64(c == cl);
			if (SCATTER) {
				const int at = __shfl(mine, cl - 1);
				if (c == cl) sorted[at + __popcll(m & ((1ull << lane) - 1))] = k;
			}
			if (lane == cl - 1) mine += __popcll(m);
			todo &= ~m;
		}
	}
	if (!SCATTER && lane < MSW_NCLS) hist[(size_t)blockIdx.x * MSW_NCLS + lane] = mine;
}

// hist[b][c]: the count of class c + 1 in block b -> how many of that class the blocks before b hold; off[] / ioff[]
__global__ __launch_bounds__(64) void msw_cls_scan_kernel(int n_blocks, int *__restrict__ hist, int *__restrict__ off, int *__restrict__ ioff)
{
	__shared__ int tot[MSW_NCLS];
	const int lane = threadIdx.x;
	if (lane < MSW_NCLS) {
		int run = 0;
		for (int b = 0; b < n_blocks; ++b) {
			const int t = hist[(size_t)b * MSW_NCLS + lane];
			hist[(size_t)b * MSW_NCLS + lane] = run;
			run += t;
		}
		tot[lane] = run;
	}
	__syncthreads();
	if (lane == 0) {
		int at = 0, iat = 0;
		for (int o = 0; o < MSW_NCLS; ++o) {
			off[o] = at; ioff[o] = iat;
			const int n = tot[MSW_NCLS - 1 - o];
			at += n; iat += (n + 1) >> 1;
		}
		off[MSW_NCLS] = at; ioff[MSW_NCLS] = iat;
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// msw_tail_kernel: what follows the forward pass of the alignments msw2_kernel listed (score >= minsc, not saturated) — score2 / te2
// from the row maxima and the reverse pass that finds where the alignment starts — 16 alignments per wave, one per quad, all of them
// live.  A wave runs in lockstep as long as its longest reverse pass (rows ~ score / a, cells ~ qe), so it takes the alignments in
// the order of the class sort, the long ones first.  This is the path of MPIBWA_MSW_REV2=0; msw_rev2_kernel is the default.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void msw_tail_kernel(MswParams P, int n_req, const int *__restrict__ cls_off, const int *__restrict__ sorted,
                                                      const MswReq *__restrict__ req, const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                      const int *__restrict__ lens, const uint8_t *__restrict__ pac, MswRes *__restrict__ res,
                                                      const uint16_t *__restrict__ rows)
{
	extern __shared__ uint32_t lds_t[];
	uint16_t *blk = (uint16_t *)lds_t;                       // [16 quads][64 rows]: the row maxima of the b[] block in hand
	uint32_t *cell = lds_t + 16 * 64 / 2;                    // msw_pass's layout
	const int quad = threadIdx.x >> 2;
	// the slot in the sorted list, long reverse passes first
	const int slot = blockIdx.x * 16 + quad;
	const bool live = slot < cls_off[MSW_NCLS];
	if (!__any(live)) return;
	const int r = live ? sorted[slot] : 0;
	MswReq rq;
	rq.rb = rq.re = 0; rq.read = 0; rq.is_rev = 0;
	MswRes out;
	out.score = 0; out.te = -1; out.qe = -1; out.score2 = -1; out.te2 = -1; out.tb = -1; out.qb = -1; out.flags = 0;
	if (live) { rq = req[r]; out = res[r]; }
	const int qlen = live ? lens[rq.read] : 0;
	const int tlen = live ? (int)(rq.re - rq.rb) : 0;
	const uint8_t *ms = seq + (live ? off[rq.read] : 0);
	msw_scan_rows(blk + quad * 64, rows, n_req, r, tlen, live, P.min_seed_len * P.a, P.max_sc, out);
	msw_reverse_one(cell, P, pac, live, live, rq, qlen, ms, out, res, r);
}

// ---------------------------------------------------------------------------------------------------------------------
// msw_rev2_kernel: what msw_tail_kernel does, for TWO alignments of one class per quad, the reverse passes in the packed arithmetic of
// msw2_kernel's forward pass (msw2_pass_lds with Msw2OwnQueries).  The two rarely share a query — the query of a reverse pass is the reversed prefix 0..qe of
// its own mate — but they share slen2, and with it S2, the segment ends and the hand-over points.  So every half has its own request,
// its own te and qe from res[], its own code set (codesA / codesB, positions qe .. 0 padded to 16 slen2 with MSW_PAD; the segment flags
// in codesA alone) and its own target bases, and the score of a cell is two lookups or'ed together: (target base, code) of A in a
// table that holds the score in the low half, of B in one that holds it in the high half.  Half X has te_X + 1 rows (row i reads
// rb_X + te_X - i); past them it repeats its last row and nothing of it is kept.  KSW_XSTOP is per half: once a row raises X's maximum
// to its forward score (or to the 8-bit ceiling: flags = 1 for X alone) X is done and frozen; the quad stops when both are done or out of
// rows.  The b[] scan (msw_scan_rows) runs for A and then for B; its block of row maxima shares LDS with the pass's row state.
// A work item is (class, pair): slot -> class by ioff[], the pair's members are neighbours in sorted[].
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void msw_rev2_kernel(MswParams P, int n_req, const int *__restrict__ cls_off, const int *__restrict__ cls_ioff,
                                                      const int *__restrict__ sorted, const MswReq *__restrict__ req, const uint8_t *__restrict__ seq,
                                                      const int64_t *__restrict__ off, const int *__restrict__ lens, const uint8_t *__restrict__ pac,
                                                      MswRes *__restrict__ res, const uint16_t *__restrict__ rows, int s_max)
{
	extern __shared__ uint32_t lds_r[];
	const int cell_words = max(s_max * 64, 16 * 64 / 2), code_words = ((s_max + 7) >> 3) * 64;
	uint32_t *cell = lds_r;                                  // [s_max][64]: H_A, E_A, H_B, E_B as bytes
	uint16_t *blk = (uint16_t *)lds_r;                       // [16 quads][64 rows]: the b[] block in hand (before the pass)
	uint32_t *codesA = lds_r + cell_words, *codesB = codesA + code_words;   // eight 4-bit entries per dword, as in msw2_kernel
	uint32_t *tabA = codesB + code_words, *tabB = tabA + 32;                // [4 target bases][8 codes] -> score (low half), score << 16
	const int lane = threadIdx.x, j = lane & 3, quad = lane >> 2;
	if (lane < 32) {
		const int t = lane >> 3, q = lane & 7;
		const int s = q < 4 ? (int)(int8_t)(msw_slo(P, t) >> (8 * q)) : q == 4 ? msw_s4(P, t) : 0;
		tabA[lane] = (uint32_t)(uint16_t)(int16_t)s;
		tabB[lane] = (uint32_t)(uint16_t)(int16_t)s << 16;
	}
	// the work item: slot -> class (the largest first) -> two neighbours of the class's stretch of sorted[]
	const int slot = blockIdx.x * 16 + quad;
	const bool live = slot < cls_ioff[MSW_NCLS];
	if (!__any(live)) return;
	int o = 0;
	if (live) while (slot >= cls_ioff[o + 1]) ++o;
	const int m0 = live ? cls_off[o] + 2 * (slot - cls_ioff[o]) : 0;
	const bool hasB = live && m0 + 1 < cls_off[o + 1];
	const int rA = live ? sorted[m0] : 0, rB = hasB ? sorted[m0 + 1] : 0;
	MswReq qa, qb;
	qa.rb = qa.re = 0; qa.read = 0; qa.is_rev = 0; qb = qa;
	MswRes oA, oB;
	oA.score = 0; oA.te = -1; oA.qe = -1; oA.score2 = -1; oA.te2 = -1; oA.tb = -1; oA.qb = -1; oA.flags = 0; oB = oA;
	if (live) { qa = req[rA]; oA = res[rA]; }
	if (hasB) { qb = req[rB]; oB = res[rB]; }
	const int qlenA = live ? lens[qa.read] : 0, qlenB = hasB ? lens[qb.read] : 0;
	const uint8_t *msA = seq + (live ? off[qa.read] : 0), *msB = seq + (hasB ? off[qb.read] : 0);
	const int minsc = P.min_seed_len * P.a;
	const int sat_limit = 255 - P.shift;
	msw_scan_rows(blk + quad * 64, rows, n_req, rA, (int)(qa.re - qa.rb), live, minsc, P.max_sc, oA);
	msw_scan_rows(blk + quad * 64, rows, n_req, rB, (int)(qb.re - qb.rb), hasB, minsc, P.max_sc, oB);
	// ---- set-up of the reverse pass: the codes of positions qe .. 0 of each half, padded, dealt to the quad; H and E cleared ----
	int qlen2A = live ? oA.qe + 1 : 0, qlen2B = hasB ? oB.qe + 1 : 0;
	if (oA.qe >= qlenA) qlen2A = 0;   // cannot happen (the maximum of a row is reached on a real base first); stay in bounds
	if (oB.qe >= qlenB) qlen2B = 0;
	const int slen2 = (max(qlen2A, qlen2B) + 15) / 16, S2 = slen2 * 4;   // (one class: the same for both)
	const int tnA = qlen2A > 0 ? oA.te + 1 : 0, tnB = qlen2B > 0 ? oB.te + 1 : 0;
	wave_lds_sync();
	if (live) {
		for (int kk = 0; kk < S2; ++kk) cell[kk * 64 + lane] = 0;
		for (int c = 0; c * 8 < S2; ++c) {
			uint32_t ca = 0, cb = 0;
			for (int u = 0; u < 8 && c * 8 + u < S2; ++u) {
				const int k = j * S2 + c * 8 + u;
				const uint32_t a = k < qlen2A ? msw_code(msA, qlenA, qa.is_rev, qlen2A - 1 - k) : MSW_PAD;
				const uint32_t b = k < qlen2B ? msw_code(msB, qlenB, qb.is_rev, qlen2B - 1 - k) : MSW_PAD;
				ca |= (a | ((k + 1) % slen2 == 0 ? 8u : 0u)) << (4 * u);
				cb |= b << (4 * u);
			}
			codesA[c * 64 + lane] = ca; codesB[c * 64 + lane] = cb;
		}
	}
	wave_lds_sync();
	// the segment length when every live quad of the wave has the same one (the rule: a wave is of one class but where two meet)
	int slen_u = 0;
	{
		const unsigned long long lv = __builtin_amdgcn_ballot_w64(live);
		const int first = __builtin_amdgcn_readlane(slen2, __ffsll((long long)lv) - 1);
		slen_u = __builtin_amdgcn_ballot_w64(live && slen2 != first) ? 0 : first;
	}
	// ---- the reverse pass of both: rows te_X .. 0, each until its forward score is reached (KSW_XSTOP) ----
	Msw2Half hA, hB;
	hA.done = tnA <= 0; hB.done = tnB <= 0;
	auto base = [&](int half, int i) -> int {
		return half ? msw2_base_at(pac, P.l_pac, qb.rb, tnB, i, true) : msw2_base_at(pac, P.l_pac, qa.rb, tnA, i, true);
	};
	auto verdict = [&](int i, uint32_t keyAB) -> bool {
		return msw2_row_verdict<false>(hA, hB, keyAB, i, tnA, tnB, sat_limit, oA.score, oB.score, nullptr, nullptr, 0);
	};
	const Msw2OwnQueries query = {codesA, codesB, tabA, tabB, tabA, tabB, 0u, 0u};
	if (slen_u > 0) msw2_pass_lds<true>(cell, P, live, S2, max(tnA, tnB), slen_u, query, base, verdict);
	else msw2_pass_lds<false>(cell, P, live, S2, max(tnA, tnB), slen_u, query, base, verdict);
	// ---- the records: lane 0 completes A's, lane 1 B's ----
	const MswPassOut gA = msw_quad_result(hA.gmax, hA.te, hA.qe), gB = msw_quad_result(hB.gmax, hB.te, hB.qe);
	const int satA = msw_from_lane3(hA.sat(sat_limit)), satB = msw_from_lane3(hB.sat(sat_limit));
	auto complete = [&](MswRes &out, int qlen2, const MswPassOut &g, int gsat) {
		if (qlen2 > 0 && g.score == out.score) { out.tb = out.te - g.te; out.qb = out.qe - g.qe; }
		if (qlen2 == 0 || gsat) out.flags = 1;
	};
	if (live && j == 0) { complete(oA, qlen2A, gA, satA); res[rA] = oA; }
	if (hasB && j == 1) { complete(oB, qlen2B, gB, satB); res[rB] = oB; }
}

} // namespace

// positions per lane for the longest read: a quarter of the padded query (padding to 16 covers both lane widths)
static int msw_s_max(int max_len) { return (max_len + 15) / 16 * 16 / 4; }

size_t msw_lds_bytes(int max_len)
{
	return (size_t)msw_s_max(max_len) * 64 * 4;
}

size_t msw2_lds_bytes(int max_len)
{
	const int s_max = msw_s_max(max_len);
	return ((size_t)s_max * 64 + (size_t)((s_max + 7) / 8) * 64 + 128) * 4;
}

size_t msw_tail_lds_bytes(int max_len)
{
	return 16 * 64 * sizeof(uint16_t) + msw_lds_bytes(max_len);   // the b[] block of every quad + msw_pass's rows
}

size_t msw_rev2_lds_bytes(int max_len)
{
	const int s_max = msw_s_max(max_len);
	// the row state (the b[] block of every quad before it, in the same place), two code sets, two score tables
	return ((size_t)std::max(s_max * 64, 16 * 64 / 2) + 2 * (size_t)((s_max + 7) / 8) * 64 + 64) * 4;
}

// MPIBWA_CPUSEC diagnostic (waits for the launch): how many alignments of msw2_kernel's work items reach min_seed_len * a — those go
// through the b[] scan and the reverse pass — and how many waves of 16 work items hold at least one such alignment as their first (A)
// or second (B) request, i.e. would run that tail in lockstep if the tails ran in the forward kernel
static void msw_tail_census(void *stream, const MswParams &P, int n_req, int n_pairs, const int *h_list, const MswRes *d_res, const int *d_tail)
{
	std::vector<MswRes> res((size_t)n_req);
	HIP_OK(hipStreamSynchronize((hipStream_t)stream));
	HIP_OK(hipMemcpy(res.data(), d_res, (size_t)n_req * sizeof(MswRes), hipMemcpyDeviceToHost));
	const int minsc = P.min_seed_len * P.a;
	long hits_a = 0, hits_b = 0, waves_a = 0, waves_b = 0;
	for (int w = 0; w * 16 < n_pairs; ++w) {
		bool any_a = false, any_b = false;
		for (int s = w * 16; s < std::min(n_pairs, w * 16 + 16); ++s) {
			const int ra = h_list[2 * s], rb = h_list[2 * s + 1];
			if (res[ra].score >= minsc) { ++hits_a; any_a = true; }
			if (rb >= 0 && res[rb].score >= minsc) { ++hits_b; any_b = true; }
		}
		waves_a += any_a; waves_b += any_b;
	}
	fprintf(stderr, "[msw] packed work items: %ld + %ld alignments reach min_seed_len*a (%d); of %d waves, %ld hold an A hit, %ld a B hit\n", hits_a, hits_b,
	        minsc, (n_pairs + 15) / 16, waves_a, waves_b);
	// the second passes by class, as the device sorted them: members by slen2 and by score class, pairs and alone-riders
	int off[MSW_NCLS + 1], ioff[MSW_NCLS + 1];
	HIP_OK(hipMemcpy(off, d_tail, sizeof(off), hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(ioff, d_tail + MSW_OFF_INTS, sizeof(ioff), hipMemcpyDeviceToHost));
	long by_sc[3] = {0, 0, 0};
	fprintf(stderr, "[msw] second passes: %d in %d quads (%d pairs, %d alone); by slen2 1..16:", off[MSW_NCLS], ioff[MSW_NCLS], off[MSW_NCLS] - ioff[MSW_NCLS],
	        2 * ioff[MSW_NCLS] - off[MSW_NCLS]);
	for (int sl = 1; sl <= 16; ++sl) {
		long n = 0;
		for (int sb = 0; sb < 3; ++sb) {
			const int o = MSW_NCLS - (1 + (sl - 1) * 3 + sb);
			n += off[o + 1] - off[o]; by_sc[sb] += off[o + 1] - off[o];
		}
		fprintf(stderr, " %ld", n);
	}
	fprintf(stderr, "; by score class: %ld %ld %ld\n", by_sc[0], by_sc[1], by_sc[2]);
}

// MPIBWA_MSW_REV2=0: every second pass on its own quad through msw_tail_kernel (the A/B of msw_rev2_kernel); read once per process
static bool msw_rev2_on()
{
	static const bool on = !(getenv("MPIBWA_MSW_REV2") && atoi(getenv("MPIBWA_MSW_REV2")) == 0);
	return on;
}

void msw_tail_counts(const int *d_tail, uint64_t out[4])
{
	int off[MSW_NCLS + 1], ioff[MSW_NCLS + 1];
	HIP_OK(hipMemcpy(off, d_tail, sizeof(off), hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(ioff, d_tail + MSW_OFF_INTS, sizeof(ioff), hipMemcpyDeviceToHost));
	const uint64_t members = (uint64_t)off[MSW_NCLS], items = msw_rev2_on() ? (uint64_t)ioff[MSW_NCLS] : members;
	out[0] = members - items; out[1] = 2 * items - members;   // members = 2 pairs + alone, items = pairs + alone
	out[2] = 0; out[3] = items;                               // (no second pass has a register form)
}

// The segment lengths msw2_kernel is instantiated for with its state in registers (reads of 65-80, 97-112, 113-128, 145-160, 193-208 and
// 241-249 bp); the work items of every other length run in the general form.
#define MSW_REGS_CLASSES 6
static const int msw_regs_slen[MSW_REGS_CLASSES] = {5, 7, 8, 10, 13, 16};
static int msw_regs_class(int slen)
{
	for (int c = 0; c < MSW_REGS_CLASSES; ++c)
		if (msw_regs_slen[c] == slen) return c;
	return MSW_REGS_CLASSES;
}

// h_req: the requests as the host holds them (for the pairing), or null: every request on its own.  h_list / d_list: room for
// 2 n_req ints each (host side page-locked in the pipeline): the pairs first (2 ints each), then the single requests.
void launch_msw(void *stream, const MswParams &P, int n_req, const MswReq *d_req, const uint8_t *d_seq, const int64_t *d_off, const int *d_len,
                const uint8_t *d_pac, MswRes *d_res, uint16_t *d_rows, int max_len, const MswReq *h_req, const int *h_len, int *h_list, int *d_list,
                int *d_tail)
{
	if (n_req <= 0) return;
	const size_t lds = msw_lds_bytes(max_len), lds2 = msw2_lds_bytes(max_len), lds_t = msw_tail_lds_bytes(max_len);
	const size_t lds_r = msw_rev2_lds_bytes(max_len);
	if (lds > 160 * 1024) die("mate-rescue kernel: reads of %d bp do not fit the LDS row buffers", max_len);
	static size_t s_attr = 0, s_attr2 = 0, s_attr_t = 0, s_attr_r = 0;
	// a kernel's dynamic LDS limit follows the longest read seen so far
	auto allow_lds = [](const void *kernel, size_t bytes, size_t &allowed) {
		if (bytes <= allowed) return;
		HIP_OK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
		allowed = bytes;
	};
	allow_lds((const void *)msw_kernel, lds, s_attr);
	static const bool pairing = !(getenv("MPIBWA_MSW_PAIRS") && atoi(getenv("MPIBWA_MSW_PAIRS")) == 0);
	static const bool regs_form = !(getenv("MPIBWA_MSW_REGS") && atoi(getenv("MPIBWA_MSW_REGS")) == 0);   // 0: every work item in the general form (the A/B)
	const bool rev2 = msw_rev2_on();
	int n_pairs = 0, n_single = n_req;
	const int *d_single = nullptr;
	if (pairing && h_req && h_len && h_list && d_list && d_tail && lds2 <= 160 * 1024 && lds_t <= 160 * 1024 && lds_r <= 160 * 1024) {
		// two requests next to each other for the same mate in the same orientation (mem_sam_pe lists an end's anchors one after the
		// other: the windows of a repeat read's anchors are such runs), both in the byte flavour
		// work items of msw2_kernel from the front of the list (two ints each; a byte-flavour request without a partner: (k, -1)), the
		// requests of the word flavour (reads of 250 bp and more) for msw_kernel from its back.
		// The work items are laid out launch by launch: those of a segment length with a register instantiation (msw_regs_class), one
		// launch per length present, the most frequent first; then those of the general form.  Two walks over the requests — count,
		// then place — so that nothing but the list itself is needed.
		int np = 0, ns = 0, n_alone = 0;
		int cls_n[MSW_REGS_CLASSES + 1], cls_at[MSW_REGS_CLASSES + 1], order[MSW_REGS_CLASSES + 1];   // (class MSW_REGS_CLASSES: the general form)
		int *sl_end = h_list + 2 * (size_t)n_req;
		auto item = [&](int k, int &cls) -> int {   // the work item that starts at request k: 0 = word flavour, 1 = alone, 2 = a pair
			const int qlen = h_len[h_req[k].read];
			if (!(qlen * P.a < 250)) return 0;
			cls = regs_form ? msw_regs_class((qlen + 15) / 16) : MSW_REGS_CLASSES;
			return k + 1 < n_req && h_req[k].read == h_req[k + 1].read && h_req[k].is_rev == h_req[k + 1].is_rev && h_req[k].re > h_req[k].rb &&
			       h_req[k + 1].re > h_req[k + 1].rb ? 2 : 1;
		};
		for (int c = 0; c <= MSW_REGS_CLASSES; ++c) cls_n[c] = 0;
		for (int k = 0; k < n_req;) {
			int cls = 0;
			const int w = item(k, cls);
			if (w) ++cls_n[cls];
			k += w ? w : 1;
		}
		for (int c = 0; c < MSW_REGS_CLASSES; ++c) order[c] = c;
		for (int a = 1; a < MSW_REGS_CLASSES; ++a)   // by falling count, ties in the order of the classes
			for (int b = a; b > 0 && cls_n[order[b]] > cls_n[order[b - 1]]; --b) std::swap(order[b], order[b - 1]);
		order[MSW_REGS_CLASSES] = MSW_REGS_CLASSES;
		for (int o = 0, at = 0; o <= MSW_REGS_CLASSES; ++o) { cls_at[order[o]] = at; at += cls_n[order[o]]; }
		int cur[MSW_REGS_CLASSES + 1];
		for (int c = 0; c <= MSW_REGS_CLASSES; ++c) cur[c] = cls_at[c];
		for (int k = 0; k < n_req;) {
			int cls = 0;
			const int w = item(k, cls);
			if (!w) { *--sl_end = k; ++ns; ++k; continue; }
			int *pl = h_list + 2 * (size_t)cur[cls]++;
			pl[0] = k; pl[1] = w == 2 ? k + 1 : -1;
			++np; n_alone += w == 1; k += w;
		}
		n_pairs = np; n_single = ns;
		static const bool say = getenv("MPIBWA_CPUSEC") != nullptr;
		if (say) fprintf(stderr, "[msw] %d requests: %d quads of two windows for one mate, %d of one, %d in the word flavour\n", n_req, np - n_alone, n_alone, ns);
		HIP_OK(hipMemcpyAsync(d_list, h_list, (size_t)2 * n_req * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
		d_single = d_list + (sl_end - h_list);
		if (n_pairs) {
			allow_lds((const void *)msw2_kernel<0>, lds2, s_attr2);
			allow_lds((const void *)msw_tail_kernel, lds_t, s_attr_t);
			allow_lds((const void *)msw_rev2_kernel, lds_r, s_attr_r);
			// the forward passes, then — same stream, before the next batch reuses d_rows — the second passes of the alignments they
			// gave a class: the class bytes sorted into lists (three small launches), then two of a class per quad (msw_rev2_kernel).
			// Grids from the worst case — every byte-flavour request has a class, and every class an odd member — nothing is read
			// back; the waves without work return.
			const int s_max = msw_s_max(max_len);
			int *d_coff = d_tail, *d_cioff = d_tail + MSW_OFF_INTS, *d_sorted = d_tail + 2 * MSW_OFF_INTS;
			uint8_t *d_cls = (uint8_t *)(d_sorted + n_req);
			int *d_hist = d_sorted + n_req + ((size_t)n_req + 3) / 4;
			HIP_OK(hipMemsetAsync(d_cls, 0, (size_t)n_req, (hipStream_t)stream));
			for (int o = 0; o <= MSW_REGS_CLASSES; ++o) {
				const int c = order[o], n = cls_n[c];
				if (!n) continue;
				const int *d_items = d_list + 2 * (size_t)cls_at[c];
				const dim3 grid((n + 15) / 16);
#define MSW2_LAUNCH(SLEN) \
	hipLaunchKernelGGL(msw2_kernel<SLEN>, grid, dim3(64), (SLEN) ? 128 * sizeof(uint32_t) : lds2, (hipStream_t)stream, P, n, n_req, d_items, d_req, d_seq, d_off, d_len, \
	                   d_pac, d_res, d_rows, s_max, d_cls)
				switch (c < MSW_REGS_CLASSES ? msw_regs_slen[c] : 0) {
				case 5: MSW2_LAUNCH(5); break;
				case 7: MSW2_LAUNCH(7); break;
				case 8: MSW2_LAUNCH(8); break;
				case 10: MSW2_LAUNCH(10); break;
				case 13: MSW2_LAUNCH(13); break;
				case 16: MSW2_LAUNCH(16); break;
				default: MSW2_LAUNCH(0);
				}
#undef MSW2_LAUNCH
			}
			const int n_byte = 2 * n_pairs - n_alone, n_blocks = (n_req + MSW_SORT_CHUNK - 1) / MSW_SORT_CHUNK;
			hipLaunchKernelGGL(msw_cls_sort_kernel<false>, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream, n_req, (const uint8_t *)d_cls, d_hist,
			                   (const int *)d_coff, d_sorted);
			hipLaunchKernelGGL(msw_cls_scan_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, n_blocks, d_hist, d_coff, d_cioff);
			hipLaunchKernelGGL(msw_cls_sort_kernel<true>, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream, n_req, (const uint8_t *)d_cls, d_hist,
			                   (const int *)d_coff, d_sorted);
			if (rev2)
				hipLaunchKernelGGL(msw_rev2_kernel, dim3((n_byte / 2 + MSW_NCLS + 15) / 16), dim3(64), lds_r, (hipStream_t)stream, P, n_req, (const int *)d_coff,
				                   (const int *)d_cioff, (const int *)d_sorted, d_req, d_seq, d_off, d_len, d_pac, d_res, (const uint16_t *)d_rows, s_max);
			else
				hipLaunchKernelGGL(msw_tail_kernel, dim3((n_byte + 15) / 16), dim3(64), lds_t, (hipStream_t)stream, P, n_req, (const int *)d_coff,
				                   (const int *)d_sorted, d_req, d_seq, d_off, d_len, d_pac, d_res, (const uint16_t *)d_rows);
		}
	}
	if (n_single)
		hipLaunchKernelGGL(msw_kernel, dim3((n_single + 15) / 16), dim3(64), lds, (hipStream_t)stream, P, n_single, n_req, d_single, d_req, d_seq, d_off, d_len, d_pac,
		                   d_res, d_rows);
	HIP_OK(hipGetLastError());
	static const bool say = getenv("MPIBWA_CPUSEC") != nullptr;
	if (say && n_pairs) msw_tail_census(stream, P, n_req, n_pairs, h_list, d_res, d_tail);
}

} // namespace mbw
