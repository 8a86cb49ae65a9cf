// phase1.hip — phase 1 of mem_process_seqs() for one sub-batch: seeding -> SA lookup -> chaining -> extension -> region clean-up
// (DESIGN §2.1), and the sub-batches of a chunk over the lanes.
#include "pipeline.h"

namespace mbw {

// MPIBWA_C2A_EARLY: 1 (default) the extension row loops stop early, 0 they run the reference's rows, 2 both with a fatal error on any difference
static int c2a_early_mode() { const char *e = getenv("MPIBWA_C2A_EARLY"); return e ? atoi(e) : 1; }
// MPIBWA_DEV_DEDUP=1: the redundancy pass of mem_sort_dedup_patch runs on the device (dedup_kernel.hip) and the host gathers its result;
// without it, or with MPIBWA_HOST_DEDUP=1, nothing is launched and the host sorts every read (the default: DESIGN §4.3c has the numbers)
static bool dev_dedup_on()
{
	const char *on = getenv("MPIBWA_DEV_DEDUP"), *off = getenv("MPIBWA_HOST_DEDUP");
	return on && atoi(on) != 0 && !(off && atoi(off) != 0);
}
// Reads with more than a handful of chains (high-copy repeats: hundreds of chains at hundreds of loci) are not walked by one
// wavefront: their chains are split into groups that cannot see each other's regions (c2a_groups.hip), a unit of c2a_kernel each.
// MPIBWA_C2A_HEAVY=<chains> moves the threshold (0: every read is walked by one wavefront, as before round 4).  Read once per process.
static int c2a_heavy_t() { static const int t = getenv("MPIBWA_C2A_HEAVY") ? atoi(getenv("MPIBWA_C2A_HEAVY")) : 8; return t; }
// The sub-batches (and the other calls in flight) take turns on the big kernels: each one fills the chip by itself, and running them one
// after the other staggers the sub-batches so that the host stages of one fall under the kernels of the other.  MPIBWA_TURNS=0: no
// turns.  Read once per process.
static bool take_turns() { static const bool on = !(getenv("MPIBWA_TURNS") && atoi(getenv("MPIBWA_TURNS")) == 0); return on; }
static TurnLock g_smem_turn, g_c2a_turn;
static std::mutex g_pes_lock;

// ---- what runs while a turn is held: functions of plain pointers, sized by the stage that calls them.  A DevBuf that does not fit may
// wait for another call to end (device_memory_pressure), and a call queued behind the holder of a turn cannot end: nothing here allocates.
struct SeedTurn {
	int n_sb, cap, max_len, n_quads; size_t per_quad; bool count_blocks;
	const uint8_t *d_seq; const int64_t *d_off; const int *d_len;
	uint64_t *d_intv; int *d_nintv, *d_nseeds, *d_lrep; unsigned long long *d_cnt; void *d_scr;
	unsigned long long *cnt; int *nseeds, *lrep, *nintv;   // where the counts come back
};
static void seed_turn(hipStream_t lst, const FmDev &fm, const mem_opt_t *opt, const SeedTurn &T, EvTimer &ev_smem)
{
	stage(20);
	std::unique_lock<TurnLock> turn(g_smem_turn, std::defer_lock);
	if (take_turns()) turn.lock();
	stage(21);
	ev_smem.start(lst);
	launch_smem(lst, fm, smem_params(opt), T.n_sb, T.d_seq, T.d_off, T.d_len, T.cap, T.d_intv, T.d_nintv, T.max_len, T.d_cnt, T.d_scr, T.per_quad, T.n_quads, T.count_blocks);
	ev_smem.stop(lst);
	// seed bookkeeping queued right behind it (src/bwamem.c:265-283): one host round trip for both
	launch_seed_prep(lst, T.n_sb, T.cap, T.d_intv, T.d_nintv, opt->max_occ, T.d_nseeds, T.d_lrep);
	HIP_OK(hipMemcpyAsync(T.cnt, T.d_cnt, 64, hipMemcpyDeviceToHost, lst));
	HIP_OK(hipMemcpyAsync(T.nseeds, T.d_nseeds, (size_t)T.n_sb * 4, hipMemcpyDeviceToHost, lst));
	HIP_OK(hipMemcpyAsync(T.lrep, T.d_lrep, (size_t)T.n_sb * 4, hipMemcpyDeviceToHost, lst));
	HIP_OK(hipMemcpyAsync(T.nintv, T.d_nintv, (size_t)T.n_sb * 4, hipMemcpyDeviceToHost, lst));
	stream_wait(lst);
	HIP_OK(hipGetLastError());
}

struct ExtendTurn {
	C2aJob job; int early;            // c2a_early_mode()
	DevReg *d_first; int *d_nfirst;   // first_reg_kernel: the sub-batch's slice of the chunk-wide arrays (null: not wanted)
	// the redundancy pass on the device (ev_dd null: not run) and the host copies of its results
	EvTimer *ev_dd; DedupParams dd;
	uint8_t *d_dd_status; int *d_dd_m, *d_dd_keep, *d_dd_list; uint8_t *h_dd_status; int *h_dd_m, *h_dd_keep;
	// the first download: counters, regions per read, the first `guess` regions (and survivor places)
	int64_t guess; unsigned long long *stat_h; int *nregs; DevReg *hregs;
};
static void extend_turn(hipStream_t lst, const mem_opt_t *opt, int64_t l_pac, const ExtendTurn &T, EvTimer &ev_ext)
{
	const C2aJob &J = T.job;
	const int n_sb = J.n_reads;
	stage(50);
	std::unique_lock<TurnLock> turn(g_c2a_turn, std::defer_lock);
	if (take_turns()) turn.lock();
	stage(51);
	queue_c2a(lst, opt, l_pac, T.early, J, ev_ext.a, ev_ext.b);
	if (T.d_first) launch_first_reg(lst, n_sb, J.d_reg_pos, J.d_nregs, J.d_packed, T.d_first, T.d_nfirst);
	if (T.ev_dd) {   // reads the raw lists, writes none of them: first_reg_kernel and the copies below see what reg_pack left
		T.ev_dd->start(lst);
		launch_dedup(lst, T.dd, n_sb, J.d_packed, J.d_reg_pos, J.d_nregs, T.d_dd_status, T.d_dd_m, T.d_dd_keep, T.d_dd_list);
		T.ev_dd->stop(lst);
	}
	// one copy of what is usually enough (2 regions per read); the rare rest follows once the total is known
	HIP_OK(hipMemcpyAsync(T.stat_h, J.d_stat, C2A_STAT_SLOTS * 64, hipMemcpyDeviceToHost, lst));
	HIP_OK(hipMemcpyAsync(T.nregs, J.d_nregs, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
	HIP_OK(hipMemcpyAsync(T.hregs, J.d_packed, (size_t)T.guess * sizeof(DevReg), hipMemcpyDeviceToHost, lst));
	if (T.ev_dd) {
		HIP_OK(hipMemcpyAsync(T.h_dd_status, T.d_dd_status, (size_t)n_sb, hipMemcpyDeviceToHost, lst));
		HIP_OK(hipMemcpyAsync(T.h_dd_m, T.d_dd_m, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
		HIP_OK(hipMemcpyAsync(T.h_dd_keep, T.d_dd_keep, (size_t)T.guess * 4, hipMemcpyDeviceToHost, lst));
	}
	stream_wait(lst);
	HIP_OK(hipGetLastError());
}

// ---- the stages of a sub-batch ----
// reads lo .. hi of the chunk, on the lane's stream with the lane's buffers and up to lane_thr host threads; the regions go to
// regs[lo .. hi) (slices of reg_arena), the first regions of every read to d_pr_first / d_pr_nfirst, the insert-size votes to pes_hist
void Call::phase1(int lo, int hi, LaneBufs &L, HostBuf &reg_arena, hipStream_t lst, int lane_thr, P1 &ps)
{
	SubBatch B{lo, hi, hi - lo, L, reg_arena, lst, lane_thr, ps};
	HIP_OK(hipSetDevice(ix.device));
	stage(2);
	encode(B);
	const double t1 = now_ms();
	seed(B);            // (stages 20: waiting for the turn, 21: holding it)
	const double t2 = now_ms();
	stage(3);
	sa_and_chain(B);
	const double t3 = now_ms();
	stage(4);
	host_chain(B);
	const double t4 = now_ms();
	stage(5);
	extend(B);          // (stages 50, 51)
	const double t5 = now_ms();
	stage(6);
	regions(B);
	votes(B);
	const double t6 = now_ms();
	ps.smem = t2 - t1; ps.sa = t3 - t2; ps.chain = t4 - t3; ps.ext = t5 - t4; ps.regs = t6 - t5;
}

void Call::encode(SubBatch &B)
{
	const int lo = B.lo, hi = B.hi;
	bseq1_t *seqs_r = seqs + lo;
	// nt4-encode this sub-batch in place (the caller sees the codes, src/bwamem.c:1057-1058) and into the staging buffer
	parallel_for(B.lane_thr, B.n_sb, 4096, [&](int i) {
		char *s = seqs_r[i].seq;
		uint8_t *d = flat + off[lo + i];
		for (int k = 0; k < seqs_r[i].l_seq; ++k) {
			s[k] = s[k] < 4 ? s[k] : (char)nt4_table[(uint8_t)s[k]];
			d[k] = (uint8_t)s[k];
		}
	});
	HIP_OK(hipMemcpyAsync((uint8_t *)W.seq.p + off[lo], flat + off[lo], (size_t)(off[hi] - off[lo]) + (hi == n ? 16 : 0), hipMemcpyHostToDevice, B.lst));
	B.d_cnt = (unsigned long long *)B.L.cnt.ensure(256);
	B.cnt = (unsigned long long *)B.L.h_cnt.ensure(256);
	// length tables for the device (the floating-point decisions of the reference, resolved per length on the host)
	B.TS = max_len + 2;
	c2a_length_tables(opt, max_len, B.tab);
	B.d_tab = (int *)B.L.tab.ensure(B.tab.size() * 4);
	HIP_OK(hipMemcpyAsync(B.d_tab, B.tab.data(), B.tab.size() * 4, hipMemcpyHostToDevice, B.lst));
}

// SMEM seeding (retry with a larger per-read capacity in the rare overflow case)
void Call::seed(SubBatch &B)
{
	LaneBufs &L = B.L;
	const int n_sb = B.n_sb;
	EvTimer ev_smem;
	uint64_t range_bases = 0;
	for (int i = 0; i < n_sb; ++i) range_bases += lens[B.lo + i];
	SeedTurn T{};
	T.n_sb = n_sb; T.max_len = max_len; T.d_seq = D.d_seq; T.d_off = D.d_off + B.lo; T.d_len = D.d_len + B.lo;
	T.n_quads = smem_grid_quads(max_len, &T.per_quad);
	T.d_scr = L.scratch.ensure(T.per_quad * T.n_quads);
	T.d_nseeds = B.d_nseeds = (int *)L.nseeds.ensure((size_t)n_sb * 4); T.d_lrep = B.d_lrep = (int *)L.lrep.ensure((size_t)n_sb * 4);
	T.nseeds = B.nseeds = (int *)L.h_nseeds.ensure((size_t)n_sb * 4 + 8); T.lrep = B.lrep = (int *)L.h_lrep.ensure((size_t)n_sb * 4 + 8);
	T.nintv = B.nintv = (int *)L.h_nintv.ensure((size_t)n_sb * 4 + 8);
	T.d_cnt = B.d_cnt; T.cnt = B.cnt;
	// MPIBWA_SMEM_COUNT=1: the seeding kernel also counts the occ blocks the reference would touch (the algorithmic bytes of
	// SURVEY §8d; a property of the reads, so the bench counts every chunk once, outside its timed region)
	const char *ce = getenv("MPIBWA_SMEM_COUNT");
	T.count_blocks = B.count_blocks = ce && atoi(ce) != 0;
	for (T.cap = std::max(64, std::min(max_len, 96));; T.cap *= 4) {
		T.d_intv = (uint64_t *)L.intv.ensure((size_t)n_sb * T.cap * 32);
		T.d_nintv = (int *)L.nintv.ensure((size_t)n_sb * 4);
		HIP_OK(hipMemsetAsync(B.d_cnt, 0, 256, B.lst));
		seed_turn(B.lst, ix.fm, opt, T, ev_smem);
		B.ps.k_smem += ev_smem.ms();
		if (B.cnt[2] == 0) break;
	}
	B.cap = T.cap; B.d_intv = T.d_intv; B.d_nintv = T.d_nintv;
	B.ps.smem_bytes = B.count_blocks ? B.cnt[1] * 64 + range_bases : 0;
	B.ps.smem_tab_bytes = B.cnt[4] * 64;
}

// seed enumeration + SA lookup (+ chaining on the device)
void Call::sa_and_chain(SubBatch &B)
{
	LaneBufs &L = B.L;
	P1 &ps = B.ps;
	const hipStream_t lst = B.lst;
	const int n_sb = B.n_sb;
	const int *nseeds = B.nseeds;
	int64_t *seed_off = B.seed_off = (int64_t *)L.h_seed_off.ensure((size_t)(n_sb + 1) * 8 + 64);
	seed_off[0] = 0;
	uint64_t n_intv = 0;
	for (int i = 0; i < n_sb; ++i) { seed_off[i + 1] = seed_off[i] + nseeds[i]; n_intv += B.nintv[i]; }
	const int64_t S = B.S = seed_off[n_sb];
	if (B.count_blocks) ps.smem_bytes += n_intv * 32;
	ps.n_intv = n_intv; ps.n_seeds = S;
	uint64_t *sa = B.sa = (uint64_t *)L.h_sa.ensure((size_t)S * 8 + 8);
	int32_t *qbl = B.qbl = (int32_t *)L.h_qbl.ensure((size_t)S * 8 + 8);
	// Chaining on the device for the reads whose ordered map stays a single B-tree node (chain_kernel.hip); the
	// others (n_chains = -1: ~2 % on 2x150 bp) and, with MPIBWA_HOST_CHAIN=1, all reads are chained by the host (host_chain).
	B.dev_chain = getenv("MPIBWA_HOST_CHAIN") == nullptr && S > 0;
	if (S == 0) return;
	EvTimer ev_sa;
	int64_t *d_seed_off = (int64_t *)L.seed_off.ensure((size_t)(n_sb + 1) * 8);
	uint64_t *d_rows = (uint64_t *)L.rows.ensure((size_t)S * 8), *d_sa = (uint64_t *)L.sa.ensure((size_t)S * 8);
	int32_t *d_qbl = (int32_t *)L.qbl.ensure((size_t)S * 8);
	HIP_OK(hipMemcpyAsync(d_seed_off, seed_off, (size_t)(n_sb + 1) * 8, hipMemcpyHostToDevice, lst));
	launch_seed_enum(lst, n_sb, B.cap, B.d_intv, B.d_nintv, opt->max_occ, d_seed_off, d_rows, d_qbl);
	if (S > 0x7fffffff) die("too many seeds in one batch");
	HIP_OK(hipMemsetAsync(B.d_cnt, 0, 256, lst));
	ev_sa.start(lst);
	if (ix.fm.sa_full) launch_sa_dense(lst, ix.fm, (int)S, d_rows, d_sa);   // one 8-byte load per row
	else launch_sa(lst, ix.fm, (int)S, d_rows, d_sa, B.d_cnt);              // LF walk on the sampled SA
	ev_sa.stop(lst);
	if (B.dev_chain) {   // queued right behind the SA lookup: one host round trip for both
		// (room for the tail the host appends: its reads cannot keep more seeds than the S they had)
		DevChain *d_chains = (DevChain *)L.chains.ensure((size_t)2 * S * sizeof(DevChain));
		DevSeed *d_seeds = (DevSeed *)L.seeds.ensure((size_t)2 * S * sizeof(DevSeed));
		unsigned int *d_srt = (unsigned int *)L.srt.ensure((size_t)2 * S * 4);
		int *d_nch = (int *)L.nch.ensure((size_t)n_sb * 4);
		launch_chain(lst, chain_params(opt, bns->l_pac), n_sb, D.d_len + B.lo, B.d_nseeds, B.d_lrep, d_seed_off, d_sa, d_qbl, D.d_ann_off, D.d_ann_alt, bns->n_seqs, B.d_tab, B.TS,
		             d_chains, d_seeds, d_srt, d_nch, L.chain_scratch.ensure(chain_scratch_bytes(n_sb)));
		B.nch = (int *)L.h_nch.ensure((size_t)n_sb * 4 + 8);
		HIP_OK(hipMemcpyAsync(B.nch, d_nch, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
	}
	HIP_OK(hipMemcpyAsync(B.cnt, B.d_cnt, 64, hipMemcpyDeviceToHost, lst));
	// The seeds themselves (16 bytes each, 124 MB per chunk of 2x150 bp) only come back for the reads the host chains: all of
	// them in host mode; in device mode the few reads chain_kernel declined, as a handful of spans once their list is known
	// (one short round trip more) — or everything again when those reads are many (repeat-rich references).
	if (!B.dev_chain) {
		HIP_OK(hipMemcpyAsync(sa, d_sa, (size_t)S * 8, hipMemcpyDeviceToHost, lst));
		HIP_OK(hipMemcpyAsync(qbl, d_qbl, (size_t)S * 8, hipMemcpyDeviceToHost, lst));
	}
	stream_wait(lst);
	HIP_OK(hipGetLastError());
	if (B.dev_chain) {
		const int64_t GAP = 1 << 15;          // spans closer than this many seeds travel as one
		std::vector<std::pair<int64_t, int64_t>> span;
		int64_t covered = 0;
		for (int i = 0; i < n_sb; ++i) {
			if (B.nch[i] >= 0 || nseeds[i] == 0) continue;
			if (!span.empty() && seed_off[i] - span.back().second <= GAP) span.back().second = seed_off[i + 1];
			else span.emplace_back(seed_off[i], seed_off[i + 1]);
		}
		for (auto &sp : span) covered += sp.second - sp.first;
		if (span.size() > 256 || covered > S / 2) { span.clear(); span.emplace_back(0, S); }
		for (auto &sp : span) {
			HIP_OK(hipMemcpyAsync(sa + sp.first, d_sa + sp.first, (size_t)(sp.second - sp.first) * 8, hipMemcpyDeviceToHost, lst));
			HIP_OK(hipMemcpyAsync(qbl + 2 * sp.first, d_qbl + 2 * sp.first, (size_t)(sp.second - sp.first) * 8, hipMemcpyDeviceToHost, lst));
		}
		if (!span.empty()) stream_wait(lst);
	}
	ps.k_sa = ev_sa.ms();
	ps.sa_bytes = ix.fm.sa_full ? (uint64_t)S * 16 : B.cnt[1] * 64 + (uint64_t)S * 8;
}

// chaining and chain filters (host).  Each block of reads is chained by one thread with recycled scratch and packed
// straight into the device layout (block-local offsets); the blocks are then concatenated after a prefix sum.
void Call::host_chain(SubBatch &B)
{
	LaneBufs &L = B.L;
	const int n_sb = B.n_sb;
	const int *nseeds = B.nseeds;
	const bseq1_t *seqs_r = seqs + B.lo;
	std::vector<int> todo;            // reads chained by the host
	if (B.dev_chain) {
		for (int i = 0; i < n_sb; ++i)
			if (B.nch[i] < 0) todo.push_back(i);
	} else {
		todo.resize(n_sb);
		for (int i = 0; i < n_sb; ++i) todo[i] = i;
	}
	const int n_todo = (int)todo.size();
	const int CB = 256, n_cb = (n_todo + CB - 1) / CB;
	struct BlockOut { std::vector<DevChain> ch; std::vector<DevSeed> sd; std::vector<unsigned int> srt; };
	std::vector<BlockOut> bo(n_cb);
	std::vector<int> chain_off(n_todo + 1), reg_off(n_todo + 1);   // per entry of `todo`
	{
		const int nt = std::max(1, B.lane_thr);
		std::vector<std::unique_ptr<HostChainer>> hcv(nt);
		parallel_blocks(nt, n_todo, CB, [&](int tid, int b, int t_lo, int t_hi) {
			if (!hcv[tid]) { hcv[tid].reset(new HostChainer()); hcv[tid]->prof = cpusec_on(); }
			BlockOut &o = bo[b];
			int64_t est = 0;
			for (int t = t_lo; t < t_hi; ++t) est += nseeds[todo[t]];
			o.sd.reserve(est); o.srt.reserve(est); o.ch.reserve((t_hi - t_lo) * 2);
			for (int t = t_lo; t < t_hi; ++t) {
				const int i = todo[t];
				const int64_t so = B.seed_off[i];
				const size_t c0 = o.ch.size(), s0 = o.sd.size();
				chain_off[t + 1] = host_chain_read(opt, bns, pac, seqs_r[i].l_seq, (const uint8_t *)seqs_r[i].seq, B.sa + so, B.qbl + 2 * so, nseeds[i], B.lrep[i],
				                                   B.tab.data(), *hcv[tid], o.ch, o.sd);   // (seed_beg: block-local for now)
				reg_off[t + 1] = (int)(o.sd.size() - s0);
				o.srt.resize(o.sd.size());
				for (size_t c = c0; c < o.ch.size(); ++c)   // the order array only carries "skipped" marks
					for (int k = 0; k < o.ch[c].n_seeds; ++k) o.srt[o.ch[c].seed_beg + k] = (unsigned int)k;
			}
		});
		if (cpusec_on()) {
			unsigned long long t[8] = {0};
			for (int a = 0; a < nt; ++a) for (int b = 0; hcv[a] && b < 8; ++b) t[b] += hcv[a]->tsc[b];
			fprintf(stderr, "[chain Mcycles] seeds->HSeed %.0f  chaining %.0f  filter %.0f  flt_seeds %.0f  pack %.0f   (%llu seeds, %llu reads with >64 seeds, %d reads)\n",
			        t[0] * 1e-6, t[1] * 1e-6, t[2] * 1e-6, t[3] * 1e-6, t[4] * 1e-6, t[5], t[6], n_sb);
		}
	}
	if (getenv("MPIBWA_CHAIN_HIST")) {   // which reads the host chained: seeds in, chains out (log2 buckets)
		unsigned long long hs[20] = {0}, hc[20] = {0}, ss[20] = {0};
		for (int t = 0; t < n_todo; ++t) {
			int b = 0, c = 0;
			while ((1 << (b + 1)) <= nseeds[todo[t]] && b < 19) ++b;
			while ((1 << (c + 1)) <= chain_off[t + 1] && c < 19) ++c;
			++hs[b]; ss[b] += nseeds[todo[t]]; ++hc[c];
		}
		fprintf(stderr, "[chain hist] %d host-chained reads; by seeds (2^b..): ", n_todo);
		for (int b = 0; b < 20; ++b) if (hs[b]) fprintf(stderr, " %d:%llu(%llu)", b, hs[b], ss[b]);
		fprintf(stderr, "; by kept chains: ");
		for (int b = 0; b < 20; ++b) if (hc[b]) fprintf(stderr, " %d:%llu", b, hc[b]);
		fprintf(stderr, "\n");
	}
	chain_off[0] = reg_off[0] = 0;
	for (int t = 0; t < n_todo; ++t) { chain_off[t + 1] += chain_off[t]; reg_off[t + 1] += reg_off[t]; }
	const int NC = B.NC = chain_off[n_todo], NS = B.NS = reg_off[n_todo];   // chains / kept seeds of the host-chained reads
	// Device layout.  Host mode: dense arrays.  Device mode: read r owns slots seed_off[r].. of all three arrays, and what
	// the host chained is appended behind the S seed slots.
	const int64_t base = B.base = B.dev_chain ? B.S : 0;
	DevChain *hchains = B.hchains = (DevChain *)L.h_chains.ensure((size_t)NC * sizeof(DevChain) + 8);
	DevSeed *hseeds = B.hseeds = (DevSeed *)L.h_seeds.ensure((size_t)NS * sizeof(DevSeed) + 8);
	unsigned int *hsrt = B.hsrt = (unsigned int *)L.h_srt.ensure((size_t)NS * 4 + 8);
	parallel_blocks(B.lane_thr, n_todo, CB, [&](int, int b, int t_lo, int) {
		BlockOut &o = bo[b];
		const int c0 = chain_off[t_lo], s0 = reg_off[t_lo];
		for (size_t c = 0; c < o.ch.size(); ++c) { hchains[c0 + c] = o.ch[c]; hchains[c0 + c].seed_beg += (int)(base + s0); }
		if (!o.sd.empty()) {
			memcpy((void *)(hseeds + s0), (const void *)o.sd.data(), o.sd.size() * sizeof(DevSeed));
			memcpy(hsrt + s0, o.srt.data(), o.srt.size() * 4);
		}
		BlockOut().ch.swap(o.ch); std::vector<DevSeed>().swap(o.sd); std::vector<unsigned int>().swap(o.srt);
	});
	if (base + NS > 0x7fffffff || base + NC > 0x7fffffff) die("too many seeds in one batch");
	int *chain_beg = B.chain_beg = (int *)L.h_cbeg.ensure((size_t)n_sb * 4 + 8), *chain_cnt = B.chain_cnt = (int *)L.h_ccnt.ensure((size_t)n_sb * 4 + 8);
	int *reg_beg = B.reg_beg = (int *)L.h_rbeg.ensure((size_t)n_sb * 4 + 8);
	uint64_t n_chains_total = NC;
	if (B.dev_chain) {
		for (int i = 0; i < n_sb; ++i) { chain_beg[i] = reg_beg[i] = (int)B.seed_off[i]; chain_cnt[i] = B.nch[i] > 0 ? B.nch[i] : 0; n_chains_total += chain_cnt[i]; }
	} else memset(chain_cnt, 0, (size_t)n_sb * 4);
	for (int t = 0; t < n_todo; ++t) {
		const int i = todo[t];
		chain_beg[i] = (int)(base + chain_off[t]); chain_cnt[i] = chain_off[t + 1] - chain_off[t]; reg_beg[i] = (int)(base + reg_off[t]);
	}
	B.ps.n_chains = n_chains_total;
	B.n_slots = base + NS;    // size of the seed / order / region arrays on the device
}

// chain -> regions on the GPU: everything is uploaded and sized here, the kernels and the first download run in extend_turn
void Call::extend(SubBatch &B)
{
	LaneBufs &L = B.L;
	P1 &ps = B.ps;
	const hipStream_t lst = B.lst;
	const int n_sb = B.n_sb, lo = B.lo, NC = B.NC, NS = B.NS;
	const int64_t base = B.base, n_slots = B.n_slots;
	B.nregs = (int *)L.h_nregs.ensure((size_t)n_sb * 4 + 8);
	B.reg_pos.assign(n_sb + 1, 0);   // where the regions of read i start in hregs
	if (n_slots == 0) {
		memset(B.nregs, 0, (size_t)n_sb * 4);
		// no read of the sub-batch has a seed: first_reg_kernel does not run, so the pairing kernel's slice of region counts must
		// be cleared here (it would otherwise read the previous chunk's, or whatever hipMalloc left there)
		if (d_pr_nfirst) { HIP_OK(hipMemsetAsync(d_pr_nfirst + lo, 0, (size_t)n_sb * 4, lst)); stream_wait(lst); }
		return;
	}
	ExtendTurn T{};
	C2aJob &J = T.job;
	int *d_chain_beg = (int *)L.chain_off.ensure((size_t)n_sb * 4), *d_chain_cnt = (int *)L.chain_cnt.ensure((size_t)n_sb * 4);
	int *d_reg_beg = (int *)L.reg_off.ensure((size_t)n_sb * 4);
	// (device mode: already sized 2 S in sa_and_chain, so these calls never move what chain_kernel wrote)
	DevChain *d_chains = (DevChain *)L.chains.ensure((size_t)std::max<int64_t>(base + NC, 1) * sizeof(DevChain));
	DevSeed *d_seeds = (DevSeed *)L.seeds.ensure((size_t)n_slots * sizeof(DevSeed));
	unsigned int *d_srt = (unsigned int *)L.srt.ensure((size_t)n_slots * 4);
	J.d_regs = (DevReg *)L.regs.ensure((size_t)n_slots * sizeof(DevReg));
	J.d_nregs = (int *)L.nregs.ensure((size_t)(n_sb + 1) * 4);
	HIP_OK(hipMemcpyAsync(d_chain_beg, B.chain_beg, (size_t)n_sb * 4, hipMemcpyHostToDevice, lst));
	HIP_OK(hipMemcpyAsync(d_chain_cnt, B.chain_cnt, (size_t)n_sb * 4, hipMemcpyHostToDevice, lst));
	HIP_OK(hipMemcpyAsync(d_reg_beg, B.reg_beg, (size_t)n_sb * 4, hipMemcpyHostToDevice, lst));
	if (NC) HIP_OK(hipMemcpyAsync(d_chains + base, B.hchains, (size_t)NC * sizeof(DevChain), hipMemcpyHostToDevice, lst));
	if (NS) HIP_OK(hipMemcpyAsync(d_seeds + base, B.hseeds, (size_t)NS * sizeof(DevSeed), hipMemcpyHostToDevice, lst));
	if (NS) HIP_OK(hipMemcpyAsync(d_srt + base, B.hsrt, (size_t)NS * 4, hipMemcpyHostToDevice, lst));
	J.d_stat = (unsigned long long *)L.c2a_stat.ensure(C2A_STAT_SLOTS * 64);
	HIP_OK(hipMemsetAsync(J.d_stat, 0, C2A_STAT_SLOTS * 64, lst));
	// launch order: reads by decreasing number of seeds (counting sort), the long-running ones first
	int *order = (int *)L.h_order.ensure((size_t)n_sb * 4 + 8);
	c2a_launch_order(n_sb, B.nseeds, order);
	int *d_order = (int *)L.order.ensure((size_t)n_sb * 4);
	HIP_OK(hipMemcpyAsync(d_order, order, (size_t)n_sb * 4, hipMemcpyHostToDevice, lst));
	J.units = c2a_prepare_units(lst, L.grp, c2a_heavy_t(), n_sb, B.chain_cnt, (size_t)std::max<int64_t>(base + NC, 1), d_chain_beg, d_reg_beg, d_chains, J.d_nregs,
	                            [](void *s) { stream_wait((hipStream_t)s); });
	J.n_reads = n_sb; J.max_len = max_len; J.d_seq = D.d_seq; J.d_off = D.d_off + lo; J.d_len = D.d_len + lo;
	J.d_chain_beg = d_chain_beg; J.d_chain_cnt = d_chain_cnt; J.d_reg_beg = d_reg_beg; J.d_order = d_order;
	J.d_chains = d_chains; J.d_seeds = d_seeds; J.d_srt = d_srt; J.d_tab = B.d_tab; J.tab_stride = B.TS; J.d_pac = (const uint8_t *)ix.d_pac;
	// Everything the turn needs is sized before it is taken: the packed regions (usually 2 per read come back at once: `guess`), ...
	const int64_t guess = T.guess = std::min<int64_t>(n_slots, (int64_t)2 * n_sb + 1024);
	J.d_reg_pos = (int *)L.reg_pos.ensure((size_t)(n_sb + 1) * 4);
	J.d_packed = (DevReg *)L.regs_packed.ensure((size_t)n_slots * sizeof(DevReg));
	J.tmp_bytes = reg_pack_tmp_bytes(n_sb);
	J.d_tmp = L.pack_tmp.ensure(J.tmp_bytes);
	T.hregs = (DevReg *)L.h_regs.ensure((size_t)guess * sizeof(DevReg) + 8);
	T.stat_h = (unsigned long long *)L.h_c2a_stat.ensure(C2A_STAT_SLOTS * 64);
	T.nregs = B.nregs; T.early = c2a_early_mode();
	T.d_first = d_pr_first ? d_pr_first + (size_t)lo * PR_MAXREG : nullptr;
	T.d_nfirst = d_pr_first ? d_pr_nfirst + lo : nullptr;
	// ... and the redundancy pass on the device
	const bool dev_dedup = dev_dedup_on();
	EvTimer ev_ext;
	std::unique_ptr<EvTimer> ev_dd;
	if (dev_dedup) {
		ev_dd.reset(new EvTimer());
		T.ev_dd = ev_dd.get();
		T.dd = dedup_params(opt, bns->l_pac);
		T.d_dd_status = (uint8_t *)L.dd_status.ensure((size_t)n_sb);
		T.d_dd_m = (int *)L.dd_m.ensure((size_t)n_sb * 4);
		T.d_dd_keep = (int *)L.dd_keep.ensure((size_t)n_slots * 4);
		T.d_dd_list = (int *)L.dd_list.ensure(dedup_list_ints(n_sb) * 4);
		T.h_dd_status = (uint8_t *)L.h_dd_status.ensure((size_t)n_sb + 8);
		T.h_dd_m = (int *)L.h_dd_m.ensure((size_t)n_sb * 4 + 8);
		T.h_dd_keep = (int *)L.h_dd_keep.ensure((size_t)guess * 4 + 8);
	}
	extend_turn(lst, opt, bns->l_pac, T, ev_ext);
	ps.k_ext = ev_ext.ms();
	unsigned long long cnt[4] = {0, 0, 0, 0};
	for (int k = 0; k < 4; ++k)
		for (int sl = 0; sl < C2A_STAT_SLOTS; ++sl) cnt[k] += T.stat_h[sl * 8 + k];
	ps.cells = cnt[0]; ps.n_ext = cnt[1];
	if (T.early == 2 && cnt[3]) die("c2a_kernel: %llu of %llu extensions change when their row loops stop early", cnt[3], cnt[1]);
	if (cpusec_on()) fprintf(stderr, "[c2a] %llu extensions, %llu without DP, %llu cells, kernel %.2f ms\n", cnt[1], cnt[2], cnt[0], ps.k_ext);
	for (int i = 0; i < n_sb; ++i) B.reg_pos[i + 1] = B.reg_pos[i] + B.nregs[i];
	const int64_t NR = B.reg_pos[n_sb];
	B.hregs = T.hregs;
	if (NR > guess) {   // the rest follows now that the total is known
		B.hregs = (DevReg *)L.h_regs2.ensure((size_t)NR * sizeof(DevReg) + 8);
		HIP_OK(hipMemcpyAsync(B.hregs, J.d_packed, (size_t)NR * sizeof(DevReg), hipMemcpyDeviceToHost, lst));
		if (dev_dedup) {
			T.h_dd_keep = (int *)L.h_dd_keep2.ensure((size_t)NR * 4 + 8);
			HIP_OK(hipMemcpyAsync(T.h_dd_keep, T.d_dd_keep, (size_t)NR * 4, hipMemcpyDeviceToHost, lst));
		}
		stream_wait(lst);
	}
	if (dev_dedup) {
		B.dd_status = T.h_dd_status; B.dd_m = T.h_dd_m; B.dd_keep = T.h_dd_keep;
		ps.k_dedup = ev_dd->ms();
		if (cpusec_on()) {
			unsigned long long c[5] = {0, 0, 0, 0, 0};
			for (int i = 0; i < n_sb; ++i) ++c[B.dd_status[i] < 5 ? B.dd_status[i] : 0];
			fprintf(stderr, "[dedup] kernels %.2f ms; reads taken %llu, more than %d regions %llu, to patch %llu\n", ps.k_dedup, c[DD_TAKEN], DD_MAXREG,
			        c[DD_HOST_MAXREG], c[DD_HOST_PATCH]);
		}
	}
}

// region post-processing (host); every read gets a slice of the batch-wide arena: its regions + room for rescued mates
void Call::regions(SubBatch &B)
{
	const int n_sb = B.n_sb, lo = B.lo;
	const int *nregs = B.nregs;
	const uint8_t *dd_status = B.dd_status;
	bseq1_t *seqs_r = seqs + lo;
	const int SLACK = 4;
	std::vector<int64_t> slice(n_sb + 1);
	slice[0] = 0;
	for (int i = 0; i < n_sb; ++i) slice[i + 1] = slice[i] + nregs[i] + SLACK;
	HReg *arena = (HReg *)B.reg_arena.ensure((size_t)slice[n_sb] * sizeof(HReg));
	parallel_for(B.lane_thr, n_sb, 256, [&](int i) {
		HRegV &v = regs[lo + i];
		const int n_raw = nregs[i], at = B.reg_pos[i];
		// a read the device took: its survivors gathered in the reference's final order, nothing to sort; every other read from its raw list
		const bool taken = dd_status && dd_status[i] == DD_TAKEN;
		const int m = taken ? B.dd_m[i] : n_raw;
		v.attach(arena + slice[i], (uint32_t)(n_raw + SLACK));
		v.resize(m);
		for (int k = 0; k < m; ++k) {
			const DevReg &d = B.hregs[at + (taken ? B.dd_keep[at + k] : k)];
			HReg &r = v[k];
			r.rb = d.rb; r.re = d.re; r.qb = d.qb; r.qe = d.qe; r.rid = d.rid; r.score = d.score; r.truesc = d.truesc;
			r.w = d.w; r.seedcov = d.seedcov; r.seedlen0 = d.seedlen0; r.frac_rep = d.frac_rep;
			if (taken && n_raw > 1) r.n_comp = 1;
		}
		if (taken) v.settled = true;
		else sort_dedup_patch(opt, bns, pac, (uint8_t *)seqs_r[i].seq, v);
		for (HReg &r : v)
			if (r.rid >= 0 && bns->anns[r.rid].is_alt) r.is_alt = 1;
	});
	for (int i = 0; i < n_sb; ++i)
		if (nregs[i] > 1) ++(dd_status && dd_status[i] == DD_TAKEN ? B.ps.n_dedup_dev : B.ps.n_dedup_host);
}

// insert-size votes of this sub-batch (src/bwamem_pair.c:52-63), so that the barrier only has to add histograms up
void Call::votes(SubBatch &B)
{
	if (!pes_hist) return;
	const int plo = B.lo >> 1, np_ = B.n_sb >> 1, nt = std::max(1, std::min(B.lane_thr, np_ / 4096));
	const size_t hsz = 4 * ((size_t)opt->max_ins + 1);
	std::vector<std::vector<uint64_t>> part(nt);
	parallel_blocks(nt, nt, 1, [&](int, int b, int, int) {
		part[b].assign(hsz, 0);
		pestat_gather(opt, bns->l_pac, plo + (int)((int64_t)np_ * b / nt), plo + (int)((int64_t)np_ * (b + 1) / nt), regs.data(), part[b].data());
	});
	std::lock_guard<std::mutex> g(g_pes_lock);
	for (int b = 0; b < nt; ++b)
		for (size_t v = 0; v < hsz; ++v) pes_hist[v] += part[b][v];
}

void Call::phase1_all()
{
	stage(24);
	if (pe && !pes0 && pestat_can_count(opt)) pes_hist_v.assign(4 * ((size_t)opt->max_ins + 1), 0);
	pes_hist = pes_hist_v.empty() ? nullptr : pes_hist_v.data();
	// Pairs with one plain hit per end are decided on the device after the insert-size statistics (pair_kernel.hip): every
	// sub-batch leaves the first region and the region count of its reads in chunk-wide arrays.
	dev_pair = pe && getenv("MPIBWA_HOST_PAIR") == nullptr && !(opt->flag & (MEM_F_NOPAIRING | MEM_F_ALL | MEM_F_REF_HDR | MEM_F_PRIMARY5)) &&
	           opt->mapQ_coef_len > 0;
	// (a single-end call that may take the device path fills the same arrays for se_simple_kernel)
	d_pr_first = dev_pair || se_want ? (DevReg *)W.pr_first.ensure((size_t)n * PR_MAXREG * sizeof(DevReg)) : nullptr;
	d_pr_nfirst = dev_pair || se_want ? (int *)W.pr_nfirst.ensure((size_t)n * 4) : nullptr;
	// K sub-batches are worked off by up to MAX_LANES host threads ("lanes"), each with its own HIP stream and workspace
	// Sub-batches overlap the GPU and host stages of ONE call.  When enough other calls are in flight they provide that
	// overlap, and one launch per kernel over the whole chunk is cheaper than three (one tail instead of three: the SMEM
	// kernel needs 23 ms for the chunk in one launch, 3 x 10 ms in three).
	// (two sub-batches since round 3: with the pairing decisions on the device the host stages of a sub-batch are short, and a
	// third sub-batch only adds a third tail to every big kernel: 93.5 vs 103-105 ms per chunk with one call in flight)
	n_sub = crowded ? 1 : 2; n_lanes = 2;
	if (const char *e = getenv("MPIBWA_SUBBATCH")) n_sub = atoi(e);
	if (const char *e = getenv("MPIBWA_LANES")) n_lanes = atoi(e);
	n_sub = std::max(1, std::min(n_sub, 16));
	n_lanes = std::max(1, std::min(n_lanes, std::min(n_sub, MAX_LANES)));
	int min_sub = 40000;   // below this a chunk is not worth splitting
	if (const char *e = getenv("MPIBWA_SUBBATCH_MIN")) min_sub = atoi(e);
	if (n < min_sub) n_sub = n_lanes = 1;
	std::vector<P1> ps(n_sub);
	if (n_sub == 1) phase1(0, n, C.ws[0], C.reg_arena[0], st, n_thr, ps[0]);
	else {
		hipStream_t *s_streams = C.p_streams;
		std::vector<int> cut(n_sub + 1);
		for (int k = 0; k <= n_sub; ++k) cut[k] = (int)((int64_t)n * k / n_sub) & ~1;   // keep mates together
		cut[n_sub] = n;
		// every lane may use all host threads: while one lane waits for a kernel the other one gets the whole CPU share
		int thr_each = n_thr;
		if (const char *e = getenv("MPIBWA_P1_THREADS")) thr_each = std::max(1, atoi(e));
		std::atomic<int> next(0);
		auto lane = [&](int l) {
			for (;;) {
				int k = next.fetch_add(1);
				if (k >= n_sub) break;
				phase1(cut[k], cut[k + 1], C.ws[l], C.reg_arena[k], s_streams[l], thr_each, ps[k]);
			}
		};
		std::vector<std::thread> th;
		for (int l = 1; l < n_lanes; ++l) th.emplace_back(lane, l);
		lane(0);
		for (auto &t : th) t.join();
	}
	for (int k = 0; k < n_sub; ++k) {
		STAT.k_smem_ms += ps[k].k_smem; STAT.k_sa_ms += ps[k].k_sa; STAT.k_ext_ms += ps[k].k_ext;
		STAT.smem_bytes += ps[k].smem_bytes; STAT.smem_tab_bytes += ps[k].smem_tab_bytes; STAT.sa_bytes += ps[k].sa_bytes; STAT.ext_cells += ps[k].cells; STAT.n_ext += ps[k].n_ext;
		STAT.n_dedup_dev += ps[k].n_dedup_dev; STAT.n_dedup_host += ps[k].n_dedup_host;
		STAT.n_intv += ps[k].n_intv; STAT.n_seeds += ps[k].n_seeds; STAT.n_chains += ps[k].n_chains;
		// per-stage wall times: the sub-batches of a lane run back to back and the lanes side by side, so sum / lanes
		STAT.smem_ms += ps[k].smem / n_lanes; STAT.sa_ms += ps[k].sa / n_lanes;
		STAT.chain_ms += ps[k].chain / n_lanes; STAT.ext_ms += ps[k].ext / n_lanes;
		STAT.regs_ms += ps[k].regs / n_lanes;
	}
	t_phase1 = now_ms();
	STAT.phase1_ms = t_phase1 - t_packed;
	STAT.n_sub = n_sub;
	c_phase1 = cpu_sec();
}

} // namespace mbw
