// chain_kernel.hip — seeds -> chains -> filtered chains on the device.
//
// Device counterpart of mem_chain (src/bwamem.c:251-315), test_and_merge (:190-211), mem_chain_weight (:213-237) and
// mem_chain_flt (:327-385).  Who chains a read is decided by how much of the reference's ordered map it needs:
//  * the reads the reference's own data structure keeps trivial, one LANE per read (chain_kernel, body chain_read): its map is a
//    B-tree whose root holds up to 9 keys (src/kbtree.h, node size 512 B), so a read that never has more than 9 chains lives in one
//    sorted array — MapArray, with the B-tree's rules for equal keys (a new key goes right behind the FIRST equal one; a lookup that
//    hits equal keys returns the first), state in LDS (StoreLds).  Three launches with growing LDS footprints
//    (chain_kernel<seeds, chains, ...>: up to 16, 64 and 255 seeds);
//  * the reads with more chains than one node holds, or with more than 255 seeds: one WAVEFRONT per read, the map as a sorted array
//    in LDS (chain_heavy_kernel<256 / 1024 / 2048 / 4096 seeds>, further down);
//  * the rest stays flagged (n_chains < 0) and takes the host path (host_chain.cpp): more than 4 096 seeds, two chains at one
//    position (where the shape of the reference's tree shows), or long enough for mem_flt_chained_seeds to act (l_query >= ~700 bp).
//
// The unstable sort of mem_chain_flt is ks_introsort (src/ksort.h:176-226) statement by statement (sortutil.h: its small form for the
// at most 9 chains of a lane's read, the full sort with its frames in LDS in chain_heavy_kernel).
// The arithmetic both kernels share with each other and with the host path — contig lookup, test_and_merge's verdict, the weight's
// coverage sums, the filter's two predicates and its cut, the reference window — stands once, in chainmath.h; the kernels keep their
// maps, loops and stores.  Floating-point compares (mask_level, drop_ratio, frac_rep) are IEEE single precision in the same
// expression shapes as the reference (no contraction, no fast-math).
//
// Output per read, in the slots the read's seeds already own (seed_off[r] .. seed_off[r] + n_seeds[r]): the kept chains
// (DevChain, in mem_chain_flt's order, with the reference window of mem_chain2aln), their seeds in the order
// mem_chain2aln visits them (ascending (score, index) — src/bwamem.c:662-667), and the identity visiting order.
// Latency-bound integer work: ~1.5 k instructions per ordinary read, a few hundred bytes of HBM per read.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <utility>
#include <vector>
#include "hip_util.h"
#include "device.h"
#include "sortutil.h"
#include "chainmath.h"

namespace mbw {

namespace {

typedef long long i64;

#define CK_MAXCH 9
#define CK_MAXCH_SMALL 4
#define CK_MAXSEEDS_SMALL 16   // first launch: every read, up to this many seeds and CK_MAXCH_SMALL chains
#define CK_MAXSEEDS 64         // second launch: what the first declined, up to this many seeds
#define CK_MAXSEEDS_BIG 255    // third launch: reads with more seeds than that (seed numbers are bytes, 255 = in no chain)
enum { F_POS_LO = 0, F_POS_HI, F_FIRST_Q, F_LAST_R_LO, F_LAST_R_HI, F_LAST_Q, F_LAST_LEN, F_RID, F_N, F_W, F_KEPT, F_FIRSTOV, F_NFIELDS };

// ---- where a read's working set lives ----
// The reads the reference's ordered map keeps in ONE node (at most 9 chains): everything in LDS, [..][lane].
template <int MAXCH>
struct StoreLds {
	uint32_t *tab;    // [F_NFIELDS * MAXCH][64]
	uint8_t *cid_;    // [MAXS + 1][64]     chain id of every seed (255 = in no chain)
	uint8_t *ord_;    // [16][64]           chain ids in tree order, later in filter order
	uint8_t *tmp_;    // [MAXS + 1][64]     scratch: members of one chain
	int lane;
	__device__ __forceinline__ uint32_t &f(int field, int id) const { return tab[(field * MAXCH + id) * 64 + lane]; }
	__device__ __forceinline__ uint8_t &cid(int k) const { return cid_[k * 64 + lane]; }
	__device__ __forceinline__ uint8_t &ord(int k) const { return ord_[k * 64 + lane]; }
	__device__ __forceinline__ uint8_t &tmp(int k) const { return tmp_[k * 64 + lane]; }
};

template <int MAXCH> __device__ __forceinline__ i64 st_pos(const StoreLds<MAXCH> &L, int id) { return (i64)((unsigned long long)L.f(F_POS_HI, id) << 32 | L.f(F_POS_LO, id)); }
template <int MAXCH> __device__ __forceinline__ i64 st_last_r(const StoreLds<MAXCH> &L, int id) { return (i64)((unsigned long long)L.f(F_LAST_R_HI, id) << 32 | L.f(F_LAST_R_LO, id)); }

// ---- the ordered map of mem_chain (src/bwamem.c:263, 288-300; src/kbtree.h) ----
// One node: a sorted array with the B-tree's rules for equal keys (a new key goes right behind the first key that is not
// smaller ... stepped back; a lookup that hits equal keys returns the first of them).
template <int MAXCH>
struct MapArray {
	int n = 0;
	__device__ __forceinline__ int lower(const StoreLds<MAXCH> &L, i64 pos) const   // closest chain at or before pos, or -1
	{
		int f = 0;
		while (f < n && st_pos(L, L.ord(f)) < pos) ++f;
		const int li = (f < n && st_pos(L, L.ord(f)) == pos) ? f : f - 1;
		return li >= 0 ? (int)L.ord(li) : -1;
	}
	__device__ __forceinline__ bool put(const StoreLds<MAXCH> &L, int id, i64 pos)   // ord[] stays in key order
	{
		if (n == MAXCH) return false;   // the reference's root node would split here
		int f = 0;
		while (f < n && st_pos(L, L.ord(f)) < pos) ++f;
		const int li = (f < n && st_pos(L, L.ord(f)) == pos) ? f : f - 1;
		for (int t = n; t > li + 1; --t) L.ord(t) = L.ord(t - 1);
		L.ord(li + 1) = (uint8_t)id;
		++n;
		return true;
	}
};

// mem_chain + mem_chain_flt + emission for ONE read (one lane).  Returns the number of kept chains, or -1: host path.
template <int MAXCH>
__device__ __forceinline__ int chain_read(const StoreLds<MAXCH> &L, const ChainParams &P, int rd, int ns, int lq, i64 so, const int *__restrict__ l_rep,
                                          const unsigned long long *__restrict__ sa, const int32_t *__restrict__ qbl, const i64 *__restrict__ ann_off,
                                          const uint8_t *__restrict__ ann_alt, int n_seqs, const int *__restrict__ gap, DevChain *__restrict__ chains,
                                          DevSeed *__restrict__ seeds, unsigned int *__restrict__ srt)
{
	const i64 l_pac = P.l_pac;
	auto S_R = [&](int k) -> i64 { return (i64)sa[so + k]; };
	auto S_Q = [&](int k) -> int { return qbl[2 * (so + k)]; };
	auto S_L = [&](int k) -> int { return qbl[2 * (so + k) + 1]; };
	auto ANN_OFF = [ann_off](int i) -> int64_t { return ann_off[i]; };
	auto GAP = [gap](int q) -> int { return gap[q]; };
	// the seeds of chain `id` in arrival order
	auto members = [&](int id, auto fn) {
		for (int k = 0; k < ns; ++k)
			if (L.cid(k) == id) fn(k);
	};

	// ---------------- mem_chain: seeds into the ordered map ----------------
	MapArray<MAXCH> map;
	int n_ch = 0;
	int64_t c_lo = 0, c_hi = -1;
	int c_rid = -1;
	for (int k = 0; k < ns; ++k) {
		const i64 rb = S_R(k);
		const int qb = S_Q(k), len = S_L(k);
		L.cid(k) = 255;
		int rid;
		if (rb >= c_lo && rb + len <= c_hi && len > 0) rid = c_rid;
		else {
			rid = intv2rid(ANN_OFF, n_seqs, l_pac, rb, rb + len);
			if (rid >= 0) {
				strand_span(l_pac, ann_off[rid], ann_off[rid + 1] - ann_off[rid], rb >= l_pac, &c_lo, &c_hi);
				c_rid = rid;
			}
		}
		if (rid < 0) continue;   // bridges two contigs or the strand boundary
		const int id0 = map.lower(L, rb);   // closest chain at or before the seed (kb_intervalp)
		int verdict = MERGE_NEW;
		if (id0 >= 0 && (int)L.f(F_RID, id0) == rid) {   // test_and_merge
			verdict = merge_verdict(l_pac, P.w, P.max_chain_gap, st_pos(L, id0), (int)L.f(F_FIRST_Q, id0), st_last_r(L, id0), (int)L.f(F_LAST_Q, id0),
			                        (int)L.f(F_LAST_LEN, id0), rb, qb, len);
			if (verdict == MERGE_APPEND) {
				L.f(F_LAST_R_LO, id0) = (uint32_t)rb; L.f(F_LAST_R_HI, id0) = (uint32_t)((unsigned long long)rb >> 32);
				L.f(F_LAST_Q, id0) = (uint32_t)qb; L.f(F_LAST_LEN, id0) = (uint32_t)len;
				L.f(F_N, id0) += 1;
				L.cid(k) = (uint8_t)id0;
			}
		}
		if (verdict != MERGE_NEW) continue;
		const int id = n_ch;
		if (id >= MAXCH) return -1;
		// (the record first: the map compares positions through it)
		L.f(F_POS_LO, id) = (uint32_t)rb; L.f(F_POS_HI, id) = (uint32_t)((unsigned long long)rb >> 32);
		L.f(F_FIRST_Q, id) = (uint32_t)qb;
		L.f(F_LAST_R_LO, id) = (uint32_t)rb; L.f(F_LAST_R_HI, id) = (uint32_t)((unsigned long long)rb >> 32);
		L.f(F_LAST_Q, id) = (uint32_t)qb; L.f(F_LAST_LEN, id) = (uint32_t)len;
		L.f(F_RID, id) = (uint32_t)rid; L.f(F_N, id) = 1;
		if (!map.put(L, id, rb)) return -1;   // more chains than this launch keeps: a later launch, or the host path
		L.cid(k) = (uint8_t)id;
		++n_ch;
	}

	// ---------------- mem_chain_flt ----------------
	int n = 0;
	for (int t = 0; t < n_ch; ++t) {
		const int id = L.ord(t);
		// mem_chain_weight: seed coverage of the query, of the reference, the smaller one
		CoverSum on_query, on_ref;
		members(id, [&](int k) { on_query.add(S_Q(k), S_L(k)); });
		members(id, [&](int k) { on_ref.add(S_R(k), S_L(k)); });
		const uint32_t w29 = (uint32_t)chain_weight_of(on_query.w, on_ref.w) & 0x1fffffffu;
		L.f(F_W, id) = w29; L.f(F_KEPT, id) = 0; L.f(F_FIRSTOV, id) = 0xffffffffu;
		if ((int)w29 < P.min_chain_weight) continue;
		L.ord(n++) = (uint8_t)id;
	}
	if (n == 0) return 0;
	// the unstable sort (:341), "less" = heavier first; n <= MAXCH chains (MapArray::put refuses one more): ks_introsort's small form
	static_assert(MAXCH <= 16, "ks_small_introsort_at is ks_introsort for at most 16 elements");
	ks_small_introsort_at(n, [&](int k) -> uint8_t & { return L.ord(k); },
	                      [&](int a_id, int b_id) -> bool { return (int)L.f(F_W, a_id) > (int)L.f(F_W, b_id); });
	// pairwise overlap marking; tmp holds the positions (in ord) of the chains kept so far
	auto BEG = [&](int t) -> int { return (int)L.f(F_FIRST_Q, L.ord(t)); };
	auto END = [&](int t) -> int { const int id = L.ord(t); return (int)L.f(F_LAST_Q, id) + (int)L.f(F_LAST_LEN, id); };
	auto ALT = [&](int t) -> int { return ann_alt[L.f(F_RID, L.ord(t))]; };
	int n_kept = 0;
	L.f(F_KEPT, L.ord(0)) = 3;
	L.tmp(n_kept++) = 0;
	for (int i = 1; i < n; ++i) {
		bool large_ovlp = false;
		int kk;
		for (kk = 0; kk < n_kept; ++kk) {
			const int j = L.tmp(kk);
			if (flt_large_overlap(P.mask_level, P.max_chain_gap, BEG(j), END(j), ALT(j), BEG(i), END(i), ALT(i))) {
				large_ovlp = true;
				if (L.f(F_FIRSTOV, L.ord(j)) == 0xffffffffu) L.f(F_FIRSTOV, L.ord(j)) = (uint32_t)i;
				if (flt_drops(P.drop_ratio, P.min_seed_len, (int)L.f(F_W, L.ord(j)), (int)L.f(F_W, L.ord(i)))) break;
			}
		}
		if (kk == n_kept) {
			L.tmp(n_kept++) = (uint8_t)i;
			L.f(F_KEPT, L.ord(i)) = large_ovlp ? 2 : 3;
		}
	}
	for (int kk = 0; kk < n_kept; ++kk) {
		const uint32_t fo = L.f(F_FIRSTOV, L.ord(L.tmp(kk)));
		if (fo != 0xffffffffu) L.f(F_KEPT, L.ord(fo)) = 1;
	}
	flt_cut_extend(n, [&](int i) -> uint32_t & { return L.f(F_KEPT, L.ord(i)); }, P.max_chain_extend);

	// ---------------- emit the kept chains and their seeds ----------------
	const float frac_rep = (float)l_rep[rd] / (float)lq;
	int n_out = 0;
	i64 cursor = so;
	for (int t = 0; t < n; ++t) {
		const int id = L.ord(t);
		if (L.f(F_KEPT, id) == 0) continue;
		// members in arrival order, then sorted by (length, arrival index): keys are distinct
		int cs = 0;
		members(id, [&](int k) { L.tmp(cs++) = (uint8_t)k; });
		// tmp was also the kept list: it is no longer needed at this point
		for (int a = 1; a < cs; ++a) {
			const uint8_t v = L.tmp(a);
			const int lv = S_L(v);
			int b = a;
			while (b > 0 && S_L(L.tmp(b - 1)) > lv) { L.tmp(b) = L.tmp(b - 1); --b; }   // stable: equal lengths keep arrival order
			L.tmp(b) = v;
		}
		const int rid = (int)L.f(F_RID, id);
		const i64 first_r = st_pos(L, id);
		i64 lo = l_pac << 1, hi = 0;
		for (int a = 0; a < cs; ++a) {
			const int k = L.tmp(a);
			DevSeed ds;
			ds.rbeg = S_R(k); ds.qbeg = S_Q(k); ds.len = S_L(k);
			seeds[cursor + a] = ds;
			srt[cursor + a] = (unsigned int)a;
			int64_t b, e;
			seed_reach(ds.rbeg, ds.qbeg, ds.len, lq, GAP, &b, &e);
			lo = b < lo ? b : lo;
			hi = e > hi ? e : hi;
		}
		DevChain d;
		strand_span(l_pac, ann_off[rid], ann_off[rid + 1] - ann_off[rid], first_r >= l_pac, &d.far_beg, &d.far_end);
		d.seed_beg = (int)cursor; d.n_seeds = cs; d.rid = rid; d.frac_rep = frac_rep;
		chain_window(l_pac, lo, hi, first_r, d.far_beg, d.far_end, &d.rmax0, &d.rmax1);
		chains[so + n_out] = d;
		++n_out;
		cursor += cs;
	}
	return n_out;
}

// Three launches with growing LDS footprints, because a lane's working set decides how many waves a CU holds and the kernel
// lives on latency hiding: <16 seeds, 4 chains> takes every read first (15.5 KB per wave: 10 waves per CU; nine reads in ten stay
// here), <64, 9> (37 KB: 4 waves) retries what that declined, <255, 9> (62 KB) the reads with 65-255 seeds.
// MAXS / MAXCH: seeds / chains per read the instantiation has LDS for.  LO >= 0: a retry — only reads an earlier launch declined
// (n_chains = -1) with more than LO seeds.
template <int MAXS, int MAXCH, int LO>
__global__ void __launch_bounds__(64)
chain_kernel(ChainParams P, int n_reads, const int *__restrict__ lens, const int *__restrict__ n_seeds, const int *__restrict__ l_rep,
             const i64 *__restrict__ seed_off, const unsigned long long *__restrict__ sa, const int32_t *__restrict__ qbl,
             const i64 *__restrict__ ann_off, const uint8_t *__restrict__ ann_alt, int n_seqs, const int *__restrict__ tab, int tab_stride,
             DevChain *__restrict__ chains, DevSeed *__restrict__ seeds, unsigned int *__restrict__ srt, int *__restrict__ n_chains,
             const int *__restrict__ list, const unsigned int *__restrict__ list_n)
{
	extern __shared__ uint32_t lds_raw[];
	StoreLds<MAXCH> L;
	L.lane = threadIdx.x;
	L.tab = lds_raw;
	L.cid_ = (uint8_t *)(lds_raw + F_NFIELDS * MAXCH * 64);
	L.ord_ = L.cid_ + (MAXS + 1) * 64;
	L.tmp_ = L.ord_ + 16 * 64;
	// a retry walks the list of the reads it is for (chain_pick_kernel), so that its waves are full: handed the whole batch, nearly
	// every wave would hold one or two such reads and run the whole serial path for them
	int rd = blockIdx.x * 64 + threadIdx.x;
	if (list) { if (rd >= (int)*list_n) return; rd = list[rd]; }
	if (rd >= n_reads) return;
	const int ns = n_seeds[rd], lq = lens[rd];
	const int *gap = tab, *noflt = tab + 5 * tab_stride;
	if (LO >= 0) { if (n_chains[rd] != -1 || ns <= LO) return; }
	else if (ns == 0) { n_chains[rd] = 0; return; }
	if (ns > MAXS || !noflt[lq]) { n_chains[rd] = -1; return; }
	n_chains[rd] = chain_read(L, P, rd, ns, lq, seed_off[rd], l_rep, sa, qbl, ann_off, ann_alt, n_seqs, gap, chains, seeds, srt);
}

// chain_pick_kernel lists the reads a later launch is for: declined so far (n_chains = -1), lo < seeds <= hi, at most cap of them.
__global__ void __launch_bounds__(256)
chain_pick_kernel(int n_reads, const int *__restrict__ lens, const int *__restrict__ n_seeds, const int *__restrict__ n_chains,
                  const int *__restrict__ noflt, int lo, int hi, int cap, int *__restrict__ list, unsigned int *__restrict__ count)
{
	const int rd = blockIdx.x * 256 + threadIdx.x;
	const bool mine = rd < n_reads && n_chains[rd] == -1 && n_seeds[rd] > lo && n_seeds[rd] <= hi && noflt[lens[rd]] != 0;
	const unsigned long long m = __ballot(mine);
	if (!m) return;
	const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
	unsigned int base = 0;
	if (lane == lead) base = atomicAdd(count, (unsigned int)__popcll(m));
	base = __shfl(base, lead);
	const unsigned int at = base + (unsigned int)__popcll(m & ((1ull << lane) - 1));
	if (mine && at < (unsigned int)cap) list[at] = rd;
}

// ---------------------------------------------------------------------------------------------------------------------
// chain_heavy_kernel (round 4): the reads with MORE than 255 seeds — reads of high-copy repeats: max_occ (500) occurrences
// of each of several intervals, hundreds to a few thousand seeds and nearly as many chains — one WAVEFRONT per read.
//   * mem_chain (src/bwamem.c:251-315) is sequential in the seeds (every seed meets the ordered map as the earlier ones left it), but
//     what a seed does to the map is a job for 64 lanes: the map is a sorted array in LDS, the closest chain at or before the seed
//     is one or two ballots, a new chain makes room with all lanes (while the chain positions of a read are distinct this is the
//     reference's B-tree to the letter; a read with two chains at one position goes to the host's restatement of the tree);
//   * mem_chain_weight (:213-237) runs a chain per lane;
//   * mem_chain_flt's unstable sort (:341) is ks_introsort on (weight, chain) words in LDS, lane 0;
//   * its pairwise pass (:346-367) — every chain against every chain kept so far, n^2 / 2 tests for a repeat whose chains all
//     overlap and all survive: the host spent 300 k cycles per such read here — runs 64 kept chains per step, the columns of the
//     kept chains (query span, weight, ALT flag, first shadowed chain) in the LDS the tree no longer needs, a break found by ballot;
//   * emission as chain_read above, a kept chain per lane, output positions by a wave prefix sum.
// Persistent waves take reads from a list (chain_pick_kernel) through a counter.  CAP = seeds (hence chains) a read may have in
// the instantiation: 256 (7.9 KB of LDS per wave: the reads of up to 255 seeds with more than 9 chains), 1024 (26 KB), 2048 (50 KB) and
// 4096 (98 KB); more seeds than that, or reads long enough for mem_flt_chained_seeds to act, stay with the host.
// ---------------------------------------------------------------------------------------------------------------------
#define HV_NONE 0xFFFFu
// LDS while the seeds are walked: the ordered map (chain positions in ascending order, 8 bytes, and whose they are, 2) and per chain
// the last seed's offset from its position (4), first_q / last_q / last_len / tail / nmem (5 x 2) — everything test_and_merge reads;
// afterwards the same bytes hold the filter's columns; behind them the three frame arrays of the sort
#define HV_FRAMES 32   // frames of the sort per array, in LDS: only lane 0 sorts, and 96 private ints held every wave to one per SIMD
__host__ __device__ constexpr size_t hv_map_bytes(int cap) { return (size_t)(cap + 64) * 24; }   // (+ 64: the map's shifts write one entry past its end)
__host__ __device__ constexpr size_t hv_lds_bytes(int cap) { return hv_map_bytes(cap) + 3 * HV_FRAMES * 4; }
__host__ __device__ constexpr size_t hv_scratch_bytes(int cap) { return (size_t)cap * (4 + 7 * 2 + 8 + 4) + 512; }
struct HvStore {   // what only the later phases read (HBM, the wave's slice): contig and first seed of every chain, the seeds' links, the tree order
	uint32_t *rid;
	uint16_t *head, *cid, *next, *ord;
	// LDS
	uint32_t *last_off;
	uint16_t *first_q, *last_q, *last_len, *tail, *nmem;
};
// "less" of mem_chain_flt's sort over the sort words: the heavier chain first (the weight is the word's upper half)
__device__ __forceinline__ bool hv_lt(uint32_t a, uint32_t b) { return (a >> 16) > (b >> 16); }
#define HV_SHIFT_K 4    // map entries a lane moves per LDS round trip when a new chain makes room
// frames: 3 * HV_FRAMES ints of LDS (pushes are rare next to element compares)
__device__ __forceinline__ void hv_sort(uint32_t *a, int n, int *frames)
{
	ks_introsort_at(n, [a](int k) -> uint32_t & { return a[k]; }, KsFramesAt{frames, frames + HV_FRAMES, frames + 2 * HV_FRAMES}, hv_lt);
}
__device__ __forceinline__ void hv_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int hv_bcast(int v) { return __builtin_amdgcn_readfirstlane(v); }

// MPIBWA_CHAIN_PROF=1: where a read's time goes, as clock64() differences that lane 0 adds to a table [class][HV_P_N] at the phase
// borders of every read (HV_P_SHIFT is part of HV_P_WALK: the loops that make room for a new chain), and what the class was handed:
// reads, seeds, chains in the map, sort words.  The kernel gets a null pointer otherwise and only tests it.
enum { HV_P_PRE = 0, HV_P_WALK, HV_P_SHIFT, HV_P_WEIGHT, HV_P_SORT, HV_P_PAIR, HV_P_EMIT, HV_P_READS, HV_P_SEEDS, HV_P_CHAINS, HV_P_WORDS, HV_P_N };

template <int CAP>
__global__ void __launch_bounds__(64)
chain_heavy_kernel(ChainParams P, const int *__restrict__ list, const unsigned int *__restrict__ list_n, unsigned int *work, int list_cap,
                   const int *__restrict__ lens, const int *__restrict__ n_seeds, const int *__restrict__ l_rep, const i64 *__restrict__ seed_off,
                   const unsigned long long *__restrict__ sa, const int32_t *__restrict__ qbl, const i64 *__restrict__ ann_off,
                   const uint8_t *__restrict__ ann_alt, int n_seqs, const int *__restrict__ gap, uint8_t *__restrict__ scratch,
                   DevChain *__restrict__ chains, DevSeed *__restrict__ seeds, unsigned int *__restrict__ srt, int *__restrict__ n_chains, unsigned long long *prof)
{
	extern __shared__ uint8_t hv_lds[];
	const int lane = threadIdx.x;
	// phase A: the tree
	i64 *spos = (i64 *)hv_lds;                                    // [CAP + 64] chain positions in ascending order
	uint16_t *sid = (uint16_t *)(hv_lds + (size_t)(CAP + 64) * 22);   // [CAP + 64] ... and whose they are
	// phases C-D (the tree is dead by then): sort words, then the columns of the chains in sorted order and of the kept list
	uint32_t *skey = (uint32_t *)hv_lds;                 // [CAP]
	uint16_t *cbeg = (uint16_t *)(skey + CAP);           // [CAP] each
	uint16_t *cend = cbeg + CAP, *kidx = cend + CAP, *kfirst = kidx + CAP;
	uint8_t *calt = (uint8_t *)(kfirst + CAP), *ckept = calt + CAP;   // [CAP] each: 4 + 8 + 2 = 14 bytes per chain <= the 20.5 of the tree
	// the sort's frames, behind both: phase A ends with sid at (CAP + 64) * 24 bytes, phases C-D with ckept at CAP * 14
	int *frames = (int *)(hv_lds + hv_map_bytes(CAP));
	static_assert((size_t)(CAP + 64) * 22 + (size_t)(CAP + 64) * 2 == hv_map_bytes(CAP) && (size_t)(CAP + 64) * 8 + (size_t)CAP * 14 <= (size_t)(CAP + 64) * 22 &&
	              (size_t)CAP * 14 <= hv_map_bytes(CAP) && hv_map_bytes(CAP) % 4 == 0 && hv_lds_bytes(CAP) == hv_map_bytes(CAP) + 3 * HV_FRAMES * sizeof(int),
	              "the frames lie behind the map and behind the filter's columns");
	uint8_t *sb = scratch + (size_t)blockIdx.x * hv_scratch_bytes(CAP);
	HvStore S;
	S.rid = (uint32_t *)sb;
	S.head = (uint16_t *)(S.rid + CAP); S.cid = S.head + CAP; S.next = S.cid + CAP; S.ord = S.next + CAP;
	S.last_off = (uint32_t *)(hv_lds + (size_t)(CAP + 64) * 8);
	S.first_q = (uint16_t *)(S.last_off + CAP); S.last_q = S.first_q + CAP; S.last_len = S.last_q + CAP; S.tail = S.last_len + CAP; S.nmem = S.tail + CAP;
	// (the filter reads first_q / last_q / last_len / nmem of the chains after the tree is gone: they are copied to the wave's HBM slice
	// before the LDS is reused — hv_spill below)
	uint16_t *g_first_q = S.ord + CAP, *g_end_q = g_first_q + CAP, *g_nmem = g_end_q + CAP;
	i64 *g_clo = (i64 *)(sb + (((size_t)CAP * 18 + 15) & ~(size_t)15));   // per seed: start of its contig on its strand (-1: no contig), its contig
	int *g_rid = (int *)(g_clo + CAP);
	const i64 l_pac = P.l_pac;
	auto ANN_OFF = [ann_off](int i) -> int64_t { return ann_off[i]; };
	auto GAP = [gap](int q) -> int { return gap[q]; };
	const int n_list =(int)(*list_n < (unsigned int)list_cap ? *list_n : (unsigned int)list_cap);
	i64 pf_last = 0, pf_shift = 0;
	auto pf_add = [&](int what, i64 v) { if (lane == 0) atomicAdd(prof + what, (unsigned long long)v); };
	auto pf_tick = [&](int phase) {   // the time since the last border goes to `phase`
		if (prof) { const i64 now = clock64(); pf_add(phase, now - pf_last); pf_last = now; }
	};
	for (;;) {
		int t = 0;
		if (lane == 0) t = (int)atomicAdd(work, 1u);
		t = hv_bcast(t);
		if (t >= n_list) break;
		const int rd = hv_bcast(list[t]);
		const int ns = hv_bcast(n_seeds[rd]), lq = hv_bcast(lens[rd]);
		const i64 so = seed_off[rd];
		auto S_R = [&](int k) -> i64 { return (i64)sa[so + k]; };
		auto S_Q = [&](int k) -> int { return qbl[2 * (so + k)]; };
		auto S_L = [&](int k) -> int { return qbl[2 * (so + k) + 1]; };
		if (ns > CAP) continue;   // (the list only holds reads that fit; n_chains stays -1: host)
		if (prof) { pf_last = clock64(); pf_shift = 0; pf_add(HV_P_READS, 1); pf_add(HV_P_SEEDS, ns); }
		// ---------------- mem_chain: the whole wave per seed ----------------
		// The ordered map of src/bwamem.c:263 is only ever asked for the closest chain at or before a position and walked in order at
		// the end; while all chain positions of the read are DISTINCT, a sorted array answers both exactly like the reference's B-tree
		// (whose shape only shows when keys are equal).  The array lives in LDS; the wave finds the predecessor with one or two ballots
		// and makes room for a new chain with all lanes.  A new chain at the position of an existing one ends the attempt: such a read
		// (rare: two seeds at one reference position more than w apart on the read) is chained by the host's restatement of the tree.
		int n_ch = 0, ok = 1;
		{
			// the contig of every seed first (bns_intv2rid, src/bntseq.c:365-376: two binary searches over the contig table in HBM), a
			// seed per lane — the seeds of a repeat hop from contig to contig, and ten dependent loads per seed in the walk below were
			// most of its time: the walk gets each seed's contig and where that contig starts on the seed's strand along with the seed
			for (int k = lane; k < ns; k += 64) {
				const i64 rb = S_R(k);
				const int len = S_L(k);
				const int rid = intv2rid(ANN_OFF, n_seqs, l_pac, rb, rb + len);
				int64_t lo = -1, hi;
				if (rid >= 0) strand_span(l_pac, ann_off[rid], ann_off[rid + 1] - ann_off[rid], rb >= l_pac, &lo, &hi);
				g_rid[k] = rid; g_clo[k] = lo;
			}
			hv_sync();
			pf_tick(HV_P_PRE);
			i64 nx_rb = S_R(0), nx_clo = g_clo[0];   // (the next seed is fetched while this one meets the map: the walk itself only touches LDS)
			int nx_qb = S_Q(0), nx_len = S_L(0), nx_rid = g_rid[0];
			for (int k = 0; k < ns; ++k) {
				const i64 rb = nx_rb, c_lo = nx_clo;
				const int qb = nx_qb, len = nx_len, rid = nx_rid;
				if (k + 1 < ns) { nx_rb = S_R(k + 1); nx_qb = S_Q(k + 1); nx_len = S_L(k + 1); nx_rid = g_rid[k + 1]; nx_clo = g_clo[k + 1]; }
				if (rid < 0) { if (lane == 0) S.cid[k] = HV_NONE; continue; }
				// chains at or before rb: a prefix of the sorted array -> its length
				int cnt;
				if (n_ch <= 64) cnt = __popcll(__ballot(lane < n_ch && spos[lane] <= rb));
				else {
					const int stride = (n_ch + 63) >> 6;
					const int at = lane * stride;
					const int blk = __popcll(__ballot(at < n_ch && spos[at] <= rb));   // samples 0, stride, 2 stride, ... at or before rb
					if (blk == 0) cnt = 0;
					else {
						const int base = (blk - 1) * stride, e = base + lane;       // the answer lies in [base, base + stride)
						cnt = base + __popcll(__ballot(lane < stride && e < n_ch && spos[e] <= rb));
					}
				}
				bool merged = false;
				int id0 = -1;
				if (cnt > 0) {
					id0 = sid[cnt - 1];
					const i64 first_r = spos[cnt - 1];
					// (a chain lies in the contig of its first seed, hence of its position: the chain found is in this seed's contig — and on its
					// strand — exactly when its position is not before the contig's start)
					if (first_r >= c_lo) {   // test_and_merge, src/bwamem.c:190-211
						const int verdict = merge_verdict(l_pac, P.w, P.max_chain_gap, first_r, S.first_q[id0], first_r + (i64)S.last_off[id0], S.last_q[id0],
						                                  S.last_len[id0], rb, qb, len);
						// (branching on the verdict first and on the lane inside, as here, costs 6 VGPRs less than the other way round)
						if (verdict == MERGE_CONTAINED) { merged = true; if (lane == 0) S.cid[k] = HV_NONE; }
						else if (verdict == MERGE_APPEND) {
							if (lane == 0) {
								S.last_off[id0] = (uint32_t)(rb - first_r); S.last_q[id0] = (uint16_t)qb; S.last_len[id0] = (uint16_t)len;
								S.nmem[id0] += 1;
								S.cid[k] = (uint16_t)id0;
								S.next[S.tail[id0]] = (uint16_t)k; S.next[k] = HV_NONE; S.tail[id0] = (uint16_t)k;
							}
							merged = true;
						}
					}
				}
				if (!merged) {
					if (cnt > 0 && spos[cnt - 1] == rb) { ok = 0; break; }   // equal keys: the reference's tree decides, on the host
					const int id = n_ch;
					// room at position cnt: the entries behind it move up by one, the top 64 * HV_SHIFT_K first, HV_SHIFT_K per lane and LDS round
					// trip.  A batch is read whole before any of it is written, and the next one lies below everything this one wrote (it ends
					// at hi - 64 K - 1, the lowest write went to hi - 64 K + 1).  The highest write is to entry n_ch, whatever K: only entries
					// e <= hi - 1 = n_ch - 1 move, and n_ch < ns <= CAP here (a seed opens at most one chain) — inside the map's pad.
					i64 pf_t0 = 0;
					if (prof) pf_t0 = clock64();
					for (int hi = n_ch; hi > cnt; hi -= 64 * HV_SHIFT_K) {
						i64 v[HV_SHIFT_K]; uint16_t w[HV_SHIFT_K];
#pragma unroll
						for (int j = 0; j < HV_SHIFT_K; ++j) {
							const int e = hi - 1 - (j * 64 + lane);
							v[j] = 0; w[j] = 0;
							if (e >= cnt) { v[j] = spos[e]; w[j] = sid[e]; }
						}
						hv_sync();
#pragma unroll
						for (int j = 0; j < HV_SHIFT_K; ++j) {
							const int e = hi - 1 - (j * 64 + lane);
							if (e >= cnt) { spos[e + 1] = v[j]; sid[e + 1] = w[j]; }
						}
						hv_sync();
					}
					if (prof) pf_shift += clock64() - pf_t0;
					if (lane == 0) {
						spos[cnt] = rb; sid[cnt] = (uint16_t)id;
						S.last_off[id] = 0; S.rid[id] = (uint32_t)rid;
						S.first_q[id] = (uint16_t)qb; S.last_q[id] = (uint16_t)qb; S.last_len[id] = (uint16_t)len; S.nmem[id] = 1;
						S.head[id] = (uint16_t)k; S.tail[id] = (uint16_t)k; S.next[k] = HV_NONE;
						S.cid[k] = (uint16_t)id;
					}
					++n_ch;
				}
				hv_sync();
			}
			if (ok)
				for (int t0 = lane; t0 < n_ch; t0 += 64) S.ord[t0] = sid[t0];   // the chains in position order (kb_itr of src/bwamem.c:304)
		}
		ok = hv_bcast(ok); n_ch = hv_bcast(n_ch);
		hv_sync();
		if (prof) { pf_tick(HV_P_WALK); pf_add(HV_P_SHIFT, pf_shift); pf_add(HV_P_CHAINS, n_ch); }
		if (!ok) { if (lane == 0) n_chains[rd] = -2; continue; }
		for (int id = lane; id < n_ch; id += 64) {   // hv_spill: query span and size of every chain, out of the LDS that is about to be reused
			g_first_q[id] = S.first_q[id]; g_end_q[id] = (uint16_t)(S.last_q[id] + S.last_len[id]); g_nmem[id] = S.nmem[id];
		}
		hv_sync();
		// ---------------- mem_chain_weight: a chain per lane; the chains that weigh enough, in tree order, as sort words ----------------
		int n = 0;
		for (int t0 = 0; t0 < n_ch; t0 += 64) {
			const int tt = t0 + lane;
			int w = 0, id = 0;
			if (tt < n_ch) {
				id = S.ord[tt];
				CoverSum on_query, on_ref;
				for (int k = S.head[id]; k != HV_NONE; k = S.next[k]) on_query.add(S_Q(k), S_L(k));
				for (int k = S.head[id]; k != HV_NONE; k = S.next[k]) on_ref.add(S_R(k), S_L(k));
				w = chain_weight_of(on_query.w, on_ref.w);
			}
			const bool pass = tt < n_ch && w >= P.min_chain_weight && w < 65536;
			if (__ballot(tt < n_ch && w >= 65536)) ok = 0;   // (a weight beyond the sort word: reads of more than 65 kbp never come here)
			const unsigned long long m = __ballot(pass);
			if (pass) skey[n + __popcll(m & ((1ull << lane) - 1))] = (uint32_t)w << 16 | (uint32_t)id;
			n += __popcll(m);
		}
		hv_sync();
		if (prof) { pf_tick(HV_P_WEIGHT); pf_add(HV_P_WORDS, n); }
		if (!ok) { if (lane == 0) n_chains[rd] = -2; continue; }
		if (n == 0) { if (lane == 0) n_chains[rd] = 0; continue; }
		static_assert((unsigned long long)CAP <= 16ull << HV_FRAMES, "ks_introsort_at: n <= 16 << FRAMES");
		if (lane == 0) hv_sort(skey, n, frames);
		hv_sync();
		pf_tick(HV_P_SORT);
		// ---------------- mem_chain_flt's pairwise pass: 64 kept chains per step ----------------
		for (int t0 = 0; t0 < n; t0 += 64) {
			const int tt = t0 + lane;
			if (tt < n) {
				const int id = skey[tt] & 0xffff;
				cbeg[tt] = g_first_q[id];
				cend[tt] = g_end_q[id];
				calt[tt] = ann_alt[S.rid[id]];
				ckept[tt] = 0;
			}
		}
		if (lane == 0) { ckept[0] = 3; kidx[0] = 0; kfirst[0] = HV_NONE; }
		hv_sync();
		int nk = 1;
		for (int i = 1; i < n; ++i) {
			const int bi = cbeg[i], ei = cend[i], wi = (int)(skey[i] >> 16), alt_i = calt[i];
			bool large = false, broke = false;
			for (int k0 = 0; k0 < nk && !broke; k0 += 64) {
				const int kk = k0 + lane;
				bool sig = false, brk = false;
				if (kk < nk) {
					const int j = kidx[kk];
					if (flt_large_overlap(P.mask_level, P.max_chain_gap, cbeg[j], cend[j], calt[j], bi, ei, alt_i)) {
						sig = true;
						brk = flt_drops(P.drop_ratio, P.min_seed_len, (int)(skey[j] >> 16), wi);
					}
				}
				unsigned long long sm = __ballot(sig);
				const unsigned long long bm = __ballot(brk);
				if (bm) {   // the reference stops at the first such chain: what lies behind it is not looked at
					const int fb = __ffsll((long long)bm) - 1;
					sm &= fb == 63 ? ~0ull : ((2ull << fb) - 1);
					broke = true;
				}
				if (sm) {
					large = true;
					if ((sm >> lane) & 1) { if (kfirst[kk] == HV_NONE) kfirst[kk] = (uint16_t)i; }
				}
			}
			if (!broke) {
				if (lane == 0) { kidx[nk] = (uint16_t)i; kfirst[nk] = HV_NONE; ckept[i] = large ? 2 : 3; }
				++nk;
			}
			hv_sync();
		}
		for (int k0 = 0; k0 < nk; k0 += 64) {
			const int kk = k0 + lane;
			if (kk < nk && kfirst[kk] != HV_NONE) ckept[kfirst[kk]] = 1;
		}
		hv_sync();
		if (P.max_chain_extend < n) {   // at most max_chain_extend chains with kept = 1 or 2 are extended (src/bwamem.c:372-379)
			if (lane == 0) flt_cut_extend(n, [ckept](int i) -> uint8_t & { return ckept[i]; }, P.max_chain_extend);
			hv_sync();
		}
		pf_tick(HV_P_PAIR);
		// ---------------- emission: a kept chain per lane, where it goes by prefix sums ----------------
		const float frac_rep = (float)l_rep[rd] / (float)lq;
		int n_out = 0;
		i64 cursor = so;
		for (int t0 = 0; t0 < n; t0 += 64) {
			const int tt = t0 + lane;
			const bool kept = tt < n && ckept[tt] != 0;
			const int id = kept ? (int)(skey[tt] & 0xffff) : 0;
			const int cs = kept ? (int)g_nmem[id] : 0;
			int pre = cs;   // inclusive prefix sum over the lanes
			for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(pre, o); if (lane >= o) pre += v; }
			const unsigned long long km = __ballot(kept);
			const i64 my_cur = cursor + (pre - cs);
			const int my_out = n_out + __popcll(km & ((1ull << lane) - 1));
			if (kept) {
				// members in arrival order, then (stable) by length: the order mem_chain2aln visits them backwards in (src/bwamem.c:662-667)
				int a = 0;
				for (int k = S.head[id]; k != HV_NONE; k = S.next[k], ++a) {
					DevSeed ds;
					ds.rbeg = S_R(k); ds.qbeg = S_Q(k); ds.len = S_L(k);
					int b = a;
					while (b > 0 && seeds[my_cur + b - 1].len > ds.len) { seeds[my_cur + b] = seeds[my_cur + b - 1]; --b; }
					seeds[my_cur + b] = ds;
				}
				i64 lo = l_pac << 1, hi = 0;
				for (a = 0; a < cs; ++a) {
					const DevSeed ds = seeds[my_cur + a];
					srt[my_cur + a] = (unsigned int)a;
					int64_t b, e;
					seed_reach(ds.rbeg, ds.qbeg, ds.len, lq, GAP, &b, &e);
					lo = b < lo ? b : lo;
					hi = e > hi ? e : hi;
				}
				const int rid = (int)S.rid[id];
				const i64 first_r = S_R(S.head[id]);
				DevChain d;
				strand_span(l_pac, ann_off[rid], ann_off[rid + 1] - ann_off[rid], first_r >= l_pac, &d.far_beg, &d.far_end);
				d.seed_beg = (int)my_cur; d.n_seeds = cs; d.rid = rid; d.frac_rep = frac_rep;
				chain_window(l_pac, lo, hi, first_r, d.far_beg, d.far_end, &d.rmax0, &d.rmax1);
				chains[so + my_out] = d;
			}
			cursor += __shfl(pre, 63);
			n_out += __popcll(km);
		}
		if (lane == 0) n_chains[rd] = n_out;
		hv_sync();   // (the next read reuses the LDS)
		pf_tick(HV_P_EMIT);
	}
}

// regions from their per-read slots into one dense array (reg_pos = exclusive prefix of n_regs)
// (a read whose chains were extended as independent units, c2a_groups.hip: its regions lie per chain, and go back into the read's
// chain order — the order the serial walk of src/bwamem.c:632-786 produces them in)
__global__ void reg_pack_kernel(int n_reads, const int *__restrict__ reg_beg, const int *__restrict__ n_regs, const int *__restrict__ reg_pos,
                                const DevReg *__restrict__ regs, DevReg *__restrict__ packed, C2aUnits U, const int *__restrict__ chain_beg,
                                const int *__restrict__ chain_cnt)
{
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	const int m = n_regs[r];
	DevReg *dst = packed + reg_pos[r];
	if (U.max_units > 0 && chain_cnt[r] > U.heavy_t) {
		int k = 0;
		for (int ci = chain_beg[r]; ci < chain_beg[r] + chain_cnt[r]; ++ci) {
			const DevReg *src = regs + U.c_rabs[ci];
			for (int j = 0; j < U.c_rcnt[ci]; ++j) dst[k++] = src[j];
		}
		return;
	}
	const DevReg *src = regs + reg_beg[r];
	for (int k = 0; k < m; ++k) dst[k] = src[k];
}

} // namespace

size_t reg_pack_tmp_bytes(int n_reads)
{
	size_t t = 0;
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const int *)nullptr, (int *)nullptr, n_reads + 1));
	return t + 256;
}

// d_nregs must hold n_reads + 1 entries (the last one is ignored and may be anything); d_reg_pos gets n_reads + 1
// entries, the last one being the total.  Everything is queued on `stream`: no host round trip between c2a and the copy.
void launch_reg_pack(void *stream, int n_reads, const int *d_reg_beg, const int *d_nregs, int *d_reg_pos, const DevReg *d_regs, DevReg *d_packed,
                     void *d_tmp, size_t tmp_bytes, const C2aUnits *units, const int *d_chain_beg, const int *d_chain_cnt)
{
	C2aUnits U;
	if (units) U = *units;
	if (n_reads <= 0) return;
	HIP_OK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_nregs, d_reg_pos, n_reads + 1, (hipStream_t)stream));
	hipLaunchKernelGGL(reg_pack_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_reads, d_reg_beg, d_nregs, d_reg_pos, d_regs,
	                   d_packed, U, d_chain_beg, d_chain_cnt);
	HIP_OK(hipGetLastError());
}

static size_t chain_lds_bytes(int maxs, int maxch) { return (size_t)F_NFIELDS * maxch * 64 * 4 + (size_t)(2 * (maxs + 1) + 16) * 64; }

// scratch of launch_chain: [two retry lists][counters, 512 bytes][three lists of reads with more than 255 seeds][the slices of
// chain_heavy_kernel's persistent waves]
// The fixed grids are what 256 CUs with 160 KB of LDS each can hold of an instantiation (its registers allow 5 waves per SIMD): a wave
// beyond that would only wait for a slot, and every wave has a slice of scratch.
#define HV_CUS 256
#define HV_WAVES_T (20 * HV_CUS)   // waves of the 256-seed instantiation (8 064 B of LDS each: 20 per CU): the reads with more than 9 chains
#define HV_WAVES_S (6 * HV_CUS)    // ... of the 1024-seed instantiation (26 496 B: 6 per CU)
#define HV_WAVES_M (3 * HV_CUS)    // ... of the 2048-seed one (51 072 B: 3 per CU)
#define HV_WAVES_L (1 * HV_CUS)    // ... of the 4096-seed one (100 224 B: one per CU)
static_assert(HV_WAVES_T / HV_CUS * hv_lds_bytes(256) <= 160 * 1024 && HV_WAVES_S / HV_CUS * hv_lds_bytes(1024) <= 160 * 1024 &&
              HV_WAVES_M / HV_CUS * hv_lds_bytes(2048) <= 160 * 1024 && hv_lds_bytes(4096) <= 160 * 1024, "resident waves per CU by LDS");
static size_t heavy_scratch_bytes()
{
	return HV_WAVES_T * hv_scratch_bytes(256) + HV_WAVES_S * hv_scratch_bytes(1024) + HV_WAVES_M * hv_scratch_bytes(2048) + HV_WAVES_L * hv_scratch_bytes(4096);
}
size_t chain_scratch_bytes(int n_reads) { return (size_t)n_reads * 8 + 512 + (size_t)n_reads * 12 + 256 + heavy_scratch_bytes(); }

// three side streams of a call's stream (created once per stream), with the events that fork them off it and join them back
#define HV_SIDES 3
struct ChainSide { hipStream_t s[HV_SIDES]; hipEvent_t fork, join[HV_SIDES]; };
static ChainSide chain_side_streams(hipStream_t st)
{
	static std::mutex side_mu;
	static std::vector<std::pair<hipStream_t, ChainSide>> sides;
	std::lock_guard<std::mutex> lk(side_mu);
	for (auto &e : sides) if (e.first == st) return e.second;
	ChainSide sd;
	for (int k = 0; k < HV_SIDES; ++k) { HIP_OK(hipStreamCreateWithFlags(&sd.s[k], hipStreamNonBlocking)); HIP_OK(hipEventCreateWithFlags(&sd.join[k], hipEventDisableTiming)); }
	HIP_OK(hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming));
	sides.emplace_back(st, sd);
	return sd;
}

void launch_chain(void *stream, const ChainParams &P, int n_reads, const int *d_len, const int *d_nseeds, const int *d_lrep,
                  const int64_t *d_seed_off, const uint64_t *d_sa, const int32_t *d_qbl, const int64_t *d_ann_off, const uint8_t *d_ann_alt,
                  int n_seqs, const int *d_tab, int tab_stride, DevChain *d_chains, DevSeed *d_seeds, unsigned int *d_srt, int *d_nchains,
                  void *d_scratch)
{
	if (n_reads <= 0) return;
	const size_t lds_s = chain_lds_bytes(CK_MAXSEEDS_SMALL, CK_MAXCH_SMALL), lds = chain_lds_bytes(CK_MAXSEEDS, CK_MAXCH), lds_big = chain_lds_bytes(CK_MAXSEEDS_BIG, CK_MAXCH);
	static bool s_attr = false;
	if (!s_attr) {
		if (lds > 64 * 1024) HIP_OK(hipFuncSetAttribute((const void *)chain_kernel<CK_MAXSEEDS, CK_MAXCH, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
		if (lds_big > 64 * 1024) HIP_OK(hipFuncSetAttribute((const void *)chain_kernel<CK_MAXSEEDS_BIG, CK_MAXCH, CK_MAXSEEDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_big));
		s_attr = true;
	}
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid((n_reads + 63) / 64), block(64);
#define CHAIN_ARGS P, n_reads, d_len, d_nseeds, d_lrep, (const i64 *)d_seed_off, (const unsigned long long *)d_sa, d_qbl, (const i64 *)d_ann_off, d_ann_alt, n_seqs, d_tab, \
	               tab_stride, d_chains, d_seeds, d_srt, d_nchains
	// chain_heavy_kernel<CAP> on stream `s`: the reads of `list` (`n` of them, handed out through `work`), the slices of its waves at `scr`
#define LAUNCH_HEAVY(CAP, waves, s, list, n, work, scr, pf)                                                                                                     \
	hipLaunchKernelGGL((chain_heavy_kernel<CAP>), dim3(waves), dim3(64), hv_lds_bytes(CAP), s, P, (const int *)(list), (const unsigned int *)(n), work,      \
	                   n_reads, d_len, d_nseeds, d_lrep, (const i64 *)d_seed_off, (const unsigned long long *)d_sa, d_qbl, (const i64 *)d_ann_off, d_ann_alt, \
	                   n_seqs, d_tab, scr, d_chains, d_seeds, d_srt, d_nchains, pf)
	const int big = getenv("MPIBWA_CHAIN_BIG") ? atoi(getenv("MPIBWA_CHAIN_BIG")) : 2;   // 0: up to 64 seeds only, 1: + 255 seeds, 2: + a wavefront per read
	int *list_a = (int *)d_scratch, *list_b = list_a + n_reads;
	unsigned int *count = (unsigned int *)(list_b + n_reads);   // [0] more than 9 chains, [1] 64-seed retry, [2] 255-seed retry, [4], [6], [8] heavy (up to 1024, 4096, 2048 seeds): list sizes; [3], [5], [7], [9] work counters
	int *list_h1 = (int *)((uint8_t *)count + 512), *list_h2 = list_h1 + n_reads, *list_h3 = list_h2 + n_reads;
	uint8_t *scr_t = (uint8_t *)(((uintptr_t)(list_h3 + n_reads) + 255) & ~(uintptr_t)255);
	uint8_t *scr_s = scr_t + HV_WAVES_T * hv_scratch_bytes(256), *scr_m = scr_s + HV_WAVES_S * hv_scratch_bytes(1024);
	uint8_t *scr_l = scr_m + HV_WAVES_M * hv_scratch_bytes(2048);
	// MPIBWA_CHAIN_PROF=1: the phase table of chain_heavy_kernel, [class][HV_P_N] behind the counters (count[32] on: 8-byte aligned, as
	// d_scratch and the two lists before it are); printed below, which waits for the launches
	const bool s_prof = getenv("MPIBWA_CHAIN_PROF") && atoi(getenv("MPIBWA_CHAIN_PROF")) != 0;   // (read at every call, as MPIBWA_CHAIN_BIG is)
	static const int prof_caps[] = {256, 1024, 2048, 4096};
	constexpr int N_PROF = (int)(sizeof(prof_caps) / sizeof(prof_caps[0]));
	static_assert(128 + N_PROF * HV_P_N * 8 <= 512, "the phase table lies in the 512 bytes of the counters");
	unsigned long long *prof = s_prof ? (unsigned long long *)(count + 32) : nullptr;
	auto prof_of = [&](int k) { return prof ? prof + k * HV_P_N : nullptr; };
	HIP_OK(hipMemsetAsync(count, 0, s_prof ? 512 : 64, st));
	// the reads declined so far with lo < seeds <= hi, listed for the launch that takes them
	auto pick = [&](int lo, int hi, int *list, unsigned int *n) {
		hipLaunchKernelGGL(chain_pick_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, st, n_reads, d_len, d_nseeds, (const int *)d_nchains, d_tab + 5 * tab_stride, lo, hi,
		                   n_reads, list, n);
	};
	hipLaunchKernelGGL((chain_kernel<CK_MAXSEEDS_SMALL, CK_MAXCH_SMALL, -1>), grid, block, lds_s, st, CHAIN_ARGS, (const int *)nullptr, (const unsigned int *)nullptr);
	pick(0, CK_MAXSEEDS, list_a, count + 1);
	hipLaunchKernelGGL((chain_kernel<CK_MAXSEEDS, CK_MAXCH, 0>), grid, block, lds, st, CHAIN_ARGS, (const int *)list_a, (const unsigned int *)(count + 1));
	if (big >= 1) {
		pick(CK_MAXSEEDS, CK_MAXSEEDS_BIG, list_b, count + 2);
		hipLaunchKernelGGL((chain_kernel<CK_MAXSEEDS_BIG, CK_MAXCH, CK_MAXSEEDS>), grid, block, lds_big, st, CHAIN_ARGS, (const int *)list_b, (const unsigned int *)(count + 2));
	}
	if (big >= 2) {
		// the reads with more than 9 chains (up to 255 seeds): a wavefront per read with the map in LDS (on a low-complexity reference a
		// third of the reads are of this kind)
		int *list_t = list_a;   // (the 64-seed retry is done with it)
		pick(0, CK_MAXSEEDS_BIG, list_t, count);
		// ... and the reads with more than 255 seeds (high-copy repeats), three more LDS footprints (max_occ = 500 makes them come as about
		// 500 k seeds: the 2048 class keeps the reads of 1 000, 1 500 and 2 000 out of the one-wave-per-CU class); MPIBWA_CHAIN_HEAVY=0 leaves those to the host
		const bool heavy = !(getenv("MPIBWA_CHAIN_HEAVY") && atoi(getenv("MPIBWA_CHAIN_HEAVY")) == 0);
		ChainSide sd = {};
		if (heavy) {
			static bool s_attr2 = false;
			if (!s_attr2) {
				HIP_OK(hipFuncSetAttribute((const void *)chain_heavy_kernel<4096>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hv_lds_bytes(4096)));
				s_attr2 = true;
			}
			pick(CK_MAXSEEDS_BIG, 1024, list_h1, count + 4);
			pick(1024, 2048, list_h3, count + 8);
			pick(2048, 4096, list_h2, count + 6);
			// The instantiations are latency-bound launches of a few hundred to a few thousand waves each: side by side on three side streams
			// of the call's stream instead of one after the other — 23 -> 10 ms per sub-batch with one call in flight.
			sd = chain_side_streams(st);
			HIP_OK(hipEventRecord(sd.fork, st));
			for (int k = 0; k < HV_SIDES; ++k) HIP_OK(hipStreamWaitEvent(sd.s[k], sd.fork, 0));
			LAUNCH_HEAVY(4096, HV_WAVES_L, sd.s[0], list_h2, count + 6, count + 7, scr_l, prof_of(3));
			LAUNCH_HEAVY(2048, HV_WAVES_M, sd.s[2], list_h3, count + 8, count + 9, scr_m, prof_of(2));
			LAUNCH_HEAVY(1024, HV_WAVES_S, sd.s[1], list_h1, count + 4, count + 5, scr_s, prof_of(1));
		}
		LAUNCH_HEAVY(256, HV_WAVES_T, st, list_t, count, count + 3, scr_t, prof_of(0));
		if (heavy)
			for (int k = 0; k < HV_SIDES; ++k) { HIP_OK(hipEventRecord(sd.join[k], sd.s[k])); HIP_OK(hipStreamWaitEvent(st, sd.join[k], 0)); }
	}
#undef LAUNCH_HEAVY
#undef CHAIN_ARGS
	HIP_OK(hipGetLastError());
	if (prof && big >= 2) {
		unsigned long long h[N_PROF * HV_P_N];
		HIP_OK(hipStreamSynchronize(st));
		HIP_OK(hipMemcpy(h, prof, sizeof(h), hipMemcpyDeviceToHost));
		for (int k = 0; k < N_PROF; ++k) {
			const unsigned long long *c = h + k * HV_P_N;
			double all = 0;
			for (int ph = HV_P_PRE; ph <= HV_P_EMIT; ++ph) if (ph != HV_P_SHIFT) all += (double)c[ph];
			const double pc = all > 0 ? 100.0 / all : 0.0;
			fprintf(stderr, "[chain] heavy<%d>: %llu reads, %llu seeds, %llu chains, %llu sort words; %.0f ticks of lane 0: contigs %.1f %%, walk %.1f %% "
			        "(of it shifts %.1f %%), weight %.1f %%, sort %.1f %%, pairwise %.1f %%, emission %.1f %%\n", prof_caps[k], c[HV_P_READS], c[HV_P_SEEDS],
			        c[HV_P_CHAINS], c[HV_P_WORDS], all, pc * c[HV_P_PRE], pc * c[HV_P_WALK], pc * c[HV_P_SHIFT], pc * c[HV_P_WEIGHT], pc * c[HV_P_SORT],
			        pc * c[HV_P_PAIR], pc * c[HV_P_EMIT]);
		}
	}
}

} // namespace mbw
