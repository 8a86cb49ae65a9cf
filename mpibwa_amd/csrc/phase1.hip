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
// The turns on the big kernels are taken in the order of arrival.  With a plain mutex a caller whose thread had to be scheduled
// first (more runnable threads than cores) kept losing the turn to callers that were already running: now and then a chunk that
// takes 0.6 s took 3 s with eight callers, the others none the faster for it.
class TurnLock {
public:
	void lock()
	{
		std::unique_lock<std::mutex> lk(m_);
		const unsigned long long mine = next_++;
		cv_.wait(lk, [&]() { return serving_ == mine; });
	}
	void unlock()
	{
		{ std::lock_guard<std::mutex> lk(m_); ++serving_; }
		cv_.notify_all();
	}
private:
	std::mutex m_;
	std::condition_variable cv_;
	unsigned long long next_ = 0, serving_ = 0;
};
static TurnLock g_smem_turn, g_c2a_turn;
static std::mutex g_pes_lock;

// reads lo .. hi of the chunk, on the lane's stream with the lane's buffers and up to lane_thr host threads; the regions go to
// regs[lo .. hi) (slices of reg_arena), the first regions of every read to d_pr_first / d_pr_nfirst, the insert-size votes to pes_hist
void Call::phase1(int lo, int hi, LaneBufs &L, HostBuf &reg_arena, hipStream_t lst, int lane_thr, P1 &ps)
{
	static const bool take_turns = !(getenv("MPIBWA_TURNS") && atoi(getenv("MPIBWA_TURNS")) == 0);
	const int n_sb = hi - lo;
	bseq1_t *seqs_r = seqs + lo;
	const int64_t *d_off_r = D.d_off + lo;
	const int *d_len_r = D.d_len + lo;
	const uint8_t *d_seq = D.d_seq;
	HIP_OK(hipSetDevice(ix.device));
	stage(2);
	// nt4-encode this sub-batch in place (the caller sees the codes, src/bwamem.c:1057-1058) and into the staging buffer
	parallel_for(lane_thr, n_sb, 4096, [&](int i) {
		char *s = seqs_r[i].seq;
		uint8_t *d = flat + off[lo + i];
		for (int k = 0; k < seqs_r[i].l_seq; ++k) {
			s[k] = s[k] < 4 ? s[k] : (char)nt4_table[(uint8_t)s[k]];
			d[k] = (uint8_t)s[k];
		}
	});
	HIP_OK(hipMemcpyAsync((uint8_t *)W.seq.p + off[lo], flat + off[lo], (size_t)(off[hi] - off[lo]) + (hi == n ? 16 : 0), hipMemcpyHostToDevice, lst));
	EvTimer ev_smem, ev_sa, ev_ext;
	unsigned long long *d_cnt = (unsigned long long *)L.cnt.ensure(256);
	unsigned long long *cnt = (unsigned long long *)L.h_cnt.ensure(256);
	// length tables for the device (the floating-point decisions of the reference, resolved per length on the host)
	const int TS = max_len + 2;
	std::vector<int> tab;
	c2a_length_tables(opt, max_len, tab);
	const int *gap_h = tab.data();   // (row 0: cal_max_gap)
	int *d_tab = (int *)L.tab.ensure(tab.size() * 4);
	HIP_OK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, lst));

	double t1 = now_ms();
	uint64_t range_bases = 0;
	for (int i = 0; i < n_sb; ++i) range_bases += lens[lo + i];
	// SMEM seeding (retry with a larger per-read capacity in the rare overflow case)
	int cap = std::max(64, std::min(max_len, 96));
	uint64_t *d_intv; int *d_nintv;
	size_t per_quad = 0;
	int n_quads = smem_grid_quads(max_len, &per_quad);
	void *d_scr = L.scratch.ensure(per_quad * n_quads);
	int *d_nseeds = (int *)L.nseeds.ensure((size_t)n_sb * 4), *d_lrep = (int *)L.lrep.ensure((size_t)n_sb * 4);
	int *nseeds = (int *)L.h_nseeds.ensure((size_t)n_sb * 4 + 8), *lrep = (int *)L.h_lrep.ensure((size_t)n_sb * 4 + 8);
	int *nintv = (int *)L.h_nintv.ensure((size_t)n_sb * 4 + 8);
	// MPIBWA_SMEM_COUNT=1: the seeding kernel also counts the occ blocks the reference would touch (the algorithmic bytes of
	// SURVEY §8d; a property of the reads, so the bench counts every chunk once, outside its timed region)
	const char *ce = getenv("MPIBWA_SMEM_COUNT");
	const bool count_blocks = ce && atoi(ce) != 0;
	for (;;) {
		d_intv = (uint64_t *)L.intv.ensure((size_t)n_sb * cap * 32);
		d_nintv = (int *)L.nintv.ensure((size_t)n_sb * 4);
		HIP_OK(hipMemsetAsync(d_cnt, 0, 256, lst));
		// the sub-batches (and the other calls in flight) take turns on the big kernels: each one fills the chip by itself, and running them one
		// after the other staggers the sub-batches so that the host stages of one fall under the kernels of the other
		stage(20);
		std::unique_lock<TurnLock> turn(g_smem_turn, std::defer_lock);
		if (take_turns) turn.lock();
		stage(21);
		ev_smem.start(lst);
		launch_smem(lst, ix.fm, smem_params(opt), n_sb, d_seq, d_off_r, d_len_r, cap, d_intv, d_nintv, max_len, d_cnt, d_scr, per_quad, n_quads, count_blocks);
		ev_smem.stop(lst);
		// seed bookkeeping queued right behind it (src/bwamem.c:265-283): one host round trip for both
		launch_seed_prep(lst, n_sb, cap, d_intv, d_nintv, opt->max_occ, d_nseeds, d_lrep);
		HIP_OK(hipMemcpyAsync(cnt, d_cnt, 64, hipMemcpyDeviceToHost, lst));
		HIP_OK(hipMemcpyAsync(nseeds, d_nseeds, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
		HIP_OK(hipMemcpyAsync(lrep, d_lrep, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
		HIP_OK(hipMemcpyAsync(nintv, d_nintv, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
		stream_wait(lst);
		HIP_OK(hipGetLastError());
		if (take_turns) turn.unlock();
		ps.k_smem += ev_smem.ms();
		if (cnt[2] == 0) break;
		cap *= 4;
	}
	ps.smem_bytes = count_blocks ? cnt[1] * 64 + range_bases : 0;
	ps.smem_tab_bytes = cnt[4] * 64;
	double t2 = now_ms();
	stage(3);

	// seed enumeration + SA lookup (+ chaining on the device)
	int64_t *seed_off = (int64_t *)L.h_seed_off.ensure((size_t)(n_sb + 1) * 8 + 64);
	seed_off[0] = 0;
	uint64_t n_intv = 0;
	for (int i = 0; i < n_sb; ++i) { seed_off[i + 1] = seed_off[i] + nseeds[i]; n_intv += nintv[i]; }
	const int64_t S = seed_off[n_sb];
	if (count_blocks) ps.smem_bytes += n_intv * 32;
	ps.n_intv = n_intv; ps.n_seeds = S;
	uint64_t *sa = (uint64_t *)L.h_sa.ensure((size_t)S * 8 + 8);
	int32_t *qbl = (int32_t *)L.h_qbl.ensure((size_t)S * 8 + 8);
	// Chaining on the device for the reads whose ordered map stays a single B-tree node (chain_kernel.hip); the
	// others (n_chains = -1: ~2 % on 2x150 bp) and, with MPIBWA_HOST_CHAIN=1, all reads are chained by the host below.
	const bool host_chain_all = getenv("MPIBWA_HOST_CHAIN") != nullptr;
	const bool dev_chain = !host_chain_all && S > 0;
	int *nch = nullptr;               // device mode: chains kept per read (-1 = host)
	DevChain *d_chains = nullptr; DevSeed *d_seeds = nullptr; unsigned int *d_srt = nullptr;
	if (S > 0) {
		int64_t *d_seed_off = (int64_t *)L.seed_off.ensure((size_t)(n_sb + 1) * 8);
		uint64_t *d_rows = (uint64_t *)L.rows.ensure((size_t)S * 8), *d_sa = (uint64_t *)L.sa.ensure((size_t)S * 8);
		int32_t *d_qbl = (int32_t *)L.qbl.ensure((size_t)S * 8);
		HIP_OK(hipMemcpyAsync(d_seed_off, seed_off, (size_t)(n_sb + 1) * 8, hipMemcpyHostToDevice, lst));
		launch_seed_enum(lst, n_sb, cap, d_intv, d_nintv, opt->max_occ, d_seed_off, d_rows, d_qbl);
		if (S > 0x7fffffff) die("too many seeds in one batch");
		HIP_OK(hipMemsetAsync(d_cnt, 0, 256, lst));
		ev_sa.start(lst);
		if (ix.fm.sa_full) launch_sa_dense(lst, ix.fm, (int)S, d_rows, d_sa);   // one 8-byte load per row
		else launch_sa(lst, ix.fm, (int)S, d_rows, d_sa, d_cnt);                // LF walk on the sampled SA
		ev_sa.stop(lst);
		if (dev_chain) {   // queued right behind the SA lookup: one host round trip for both
			// (room for the tail the host appends: its reads cannot keep more seeds than the S they had)
			d_chains = (DevChain *)L.chains.ensure((size_t)2 * S * sizeof(DevChain));
			d_seeds = (DevSeed *)L.seeds.ensure((size_t)2 * S * sizeof(DevSeed));
			d_srt = (unsigned int *)L.srt.ensure((size_t)2 * S * 4);
			int *d_nch = (int *)L.nch.ensure((size_t)n_sb * 4);
			launch_chain(lst, chain_params(opt, bns->l_pac), n_sb, d_len_r, d_nseeds, d_lrep, d_seed_off, d_sa, d_qbl, D.d_ann_off, D.d_ann_alt, bns->n_seqs, d_tab, TS, d_chains,
			             d_seeds, d_srt, d_nch, L.chain_scratch.ensure(chain_scratch_bytes(n_sb)));
			nch = (int *)L.h_nch.ensure((size_t)n_sb * 4 + 8);
			HIP_OK(hipMemcpyAsync(nch, d_nch, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
		}
		HIP_OK(hipMemcpyAsync(cnt, d_cnt, 64, hipMemcpyDeviceToHost, lst));
		// The seeds themselves (16 bytes each, 124 MB per chunk of 2x150 bp) only come back for the reads the host chains: all of
		// them in host mode; in device mode the few reads chain_kernel declined, as a handful of spans once their list is known
		// (one short round trip more) — or everything again when those reads are many (repeat-rich references).
		bool seeds_fetched = false;
		if (!dev_chain) {
			HIP_OK(hipMemcpyAsync(sa, d_sa, (size_t)S * 8, hipMemcpyDeviceToHost, lst));
			HIP_OK(hipMemcpyAsync(qbl, d_qbl, (size_t)S * 8, hipMemcpyDeviceToHost, lst));
			seeds_fetched = true;
		}
		stream_wait(lst);
		HIP_OK(hipGetLastError());
		if (!seeds_fetched) {
			const int64_t GAP = 1 << 15;          // spans closer than this many seeds travel as one
			std::vector<std::pair<int64_t, int64_t>> span;
			int64_t covered = 0;
			for (int i = 0; i < n_sb; ++i) {
				if (nch[i] >= 0 || nseeds[i] == 0) continue;
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
		ps.sa_bytes = ix.fm.sa_full ? (uint64_t)S * 16 : cnt[1] * 64 + (uint64_t)S * 8;
	}
	double t3 = now_ms();
	stage(4);

	// chaining and chain filters (host).  Each block of reads is chained by one thread with recycled scratch and packed
	// straight into the device layout (block-local offsets); the blocks are then concatenated after a prefix sum.
	std::vector<int> todo;            // reads chained by the host
	if (dev_chain) {
		for (int i = 0; i < n_sb; ++i)
			if (nch[i] < 0) todo.push_back(i);
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
		const int nt = std::max(1, lane_thr);
		std::vector<std::unique_ptr<ChainScratch>> scr(nt);
		std::vector<std::vector<HSeed>> hsv(nt);
		std::vector<std::vector<HChain *>> chv(nt);
		std::vector<std::vector<uint64_t>> keyv(nt);
		static const bool prof_chain = getenv("MPIBWA_CPUSEC") != nullptr;
		std::vector<unsigned long long> tsc((size_t)nt * 8, 0);
		parallel_blocks(nt, n_todo, CB, [&](int tid, int b, int t_lo, int t_hi) {
			if (!scr[tid]) scr[tid].reset(new ChainScratch());
			std::vector<HSeed> &hs = hsv[tid];
			std::vector<HChain *> &chains = chv[tid];
			std::vector<uint64_t> &key = keyv[tid];
			BlockOut &o = bo[b];
			int64_t est = 0;
			for (int t = t_lo; t < t_hi; ++t) est += nseeds[todo[t]];
			o.sd.reserve(est); o.srt.reserve(est); o.ch.reserve((t_hi - t_lo) * 2);
			for (int t = t_lo; t < t_hi; ++t) {
				const int i = todo[t];
				int ns = nseeds[i];
				chain_off[t + 1] = reg_off[t + 1] = 0;
				if (ns == 0) continue;
				const unsigned long long c0 = prof_chain ? __builtin_ia32_rdtsc() : 0;
				hs.resize(ns);
				for (int k = 0; k < ns; ++k) {
					int64_t so = seed_off[i] + k;
					hs[k].rbeg = (int64_t)sa[so]; hs[k].qbeg = qbl[2 * so]; hs[k].len = hs[k].score = qbl[2 * so + 1];
				}
				const unsigned long long c1 = prof_chain ? __builtin_ia32_rdtsc() : 0;
				chains_from_seeds(opt, bns, seqs_r[i].l_seq, hs.data(), ns, lrep[i], *scr[tid], chains);
				const unsigned long long c2 = prof_chain ? __builtin_ia32_rdtsc() : 0;
				chain_filter(opt, *scr[tid], chains);
				const unsigned long long c3 = prof_chain ? __builtin_ia32_rdtsc() : 0;
				filter_chained_seeds(opt, bns, pac, seqs_r[i].l_seq, (const uint8_t *)seqs_r[i].seq, chains);
				const unsigned long long c4 = prof_chain ? __builtin_ia32_rdtsc() : 0;
				if (prof_chain) { tsc[tid * 8 + 0] += c1 - c0; tsc[tid * 8 + 1] += c2 - c1; tsc[tid * 8 + 2] += c3 - c2; tsc[tid * 8 + 3] += c4 - c3; tsc[tid * 8 + 5] += ns; tsc[tid * 8 + 6] += ns > 64; }
				int tot = 0;
				for (const HChain *cp_ : chains) {
					const HChain &ch = *cp_;
					const int cs = (int)ch.seeds.size();
					DevChain d;
					const size_t at = o.sd.size();
					o.sd.resize(at + cs); o.srt.resize(at + cs);
					pack_chain_for_device(bns, ch, seqs_r[i].l_seq, gap_h, key, d, o.sd.data() + at);
					d.seed_beg = (int)at;   // block-local for now
					for (int k = 0; k < cs; ++k) o.srt[at + k] = (unsigned int)k;   // the order array only carries "skipped" marks
					o.ch.push_back(d);
					tot += cs;
				}
				chain_off[t + 1] = (int)chains.size();
				reg_off[t + 1] = tot;
				if (prof_chain) tsc[tid * 8 + 4] += __builtin_ia32_rdtsc() - c4;
			}
		});
		if (prof_chain) {
			unsigned long long t[8] = {0};
			for (int a = 0; a < nt; ++a) for (int b = 0; b < 8; ++b) t[b] += tsc[(size_t)a * 8 + b];
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
	const int NC = chain_off[n_todo], NS = reg_off[n_todo];   // chains / kept seeds of the host-chained reads
	// Device layout.  Host mode: dense arrays.  Device mode: read r owns slots seed_off[r].. of all three arrays, and what
	// the host chained is appended behind the S seed slots.
	const int64_t base = dev_chain ? S : 0;
	DevChain *hchains = (DevChain *)L.h_chains.ensure((size_t)NC * sizeof(DevChain) + 8);
	DevSeed *hseeds = (DevSeed *)L.h_seeds.ensure((size_t)NS * sizeof(DevSeed) + 8);
	unsigned int *hsrt = (unsigned int *)L.h_srt.ensure((size_t)NS * 4 + 8);
	parallel_blocks(lane_thr, n_todo, CB, [&](int, int b, int t_lo, int) {
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
	int *chain_beg = (int *)L.h_cbeg.ensure((size_t)n_sb * 4 + 8), *chain_cnt = (int *)L.h_ccnt.ensure((size_t)n_sb * 4 + 8);
	int *reg_beg = (int *)L.h_rbeg.ensure((size_t)n_sb * 4 + 8);
	uint64_t n_chains_total = NC;
	if (dev_chain) {
		for (int i = 0; i < n_sb; ++i) { chain_beg[i] = reg_beg[i] = (int)seed_off[i]; chain_cnt[i] = nch[i] > 0 ? nch[i] : 0; n_chains_total += chain_cnt[i]; }
	} else memset(chain_cnt, 0, (size_t)n_sb * 4);
	for (int t = 0; t < n_todo; ++t) {
		const int i = todo[t];
		chain_beg[i] = (int)(base + chain_off[t]); chain_cnt[i] = chain_off[t + 1] - chain_off[t]; reg_beg[i] = (int)(base + reg_off[t]);
	}
	ps.n_chains = n_chains_total;
	const int64_t n_slots = base + NS;    // size of the seed / order / region arrays on the device
	double t4 = now_ms();
	stage(5);

	// chain -> regions on the GPU
	int *nregs = (int *)L.h_nregs.ensure((size_t)n_sb * 4 + 8);
	std::vector<int> reg_pos(n_sb + 1, 0);   // where the regions of read i start in hregs
	DevReg *hregs = nullptr;
	// the redundancy pass on the device: status / survivors / their places in the raw list, per read of the sub-batch (null: not run)
	const bool dev_dedup = dev_dedup_on();
	const uint8_t *dd_status = nullptr;
	const int *dd_m = nullptr, *dd_keep = nullptr;
	if (n_slots == 0) {
		memset(nregs, 0, (size_t)n_sb * 4);
		// no read of the sub-batch has a seed: first_reg_kernel does not run, so the pairing kernel's slice of region counts must
		// be cleared here (it would otherwise read the previous chunk's, or whatever hipMalloc left there)
		if (d_pr_nfirst) { HIP_OK(hipMemsetAsync(d_pr_nfirst + lo, 0, (size_t)n_sb * 4, lst)); stream_wait(lst); }
	} else {
		int *d_chain_beg = (int *)L.chain_off.ensure((size_t)n_sb * 4), *d_chain_cnt = (int *)L.chain_cnt.ensure((size_t)n_sb * 4);
		int *d_reg_beg = (int *)L.reg_off.ensure((size_t)n_sb * 4);
		// (device mode: already sized 2 S above, so these calls never move what chain_kernel wrote)
		d_chains = (DevChain *)L.chains.ensure((size_t)std::max<int64_t>(base + NC, 1) * sizeof(DevChain));
		d_seeds = (DevSeed *)L.seeds.ensure((size_t)n_slots * sizeof(DevSeed));
		d_srt = (unsigned int *)L.srt.ensure((size_t)n_slots * 4);
		DevReg *d_regs = (DevReg *)L.regs.ensure((size_t)n_slots * sizeof(DevReg));
		int *d_nregs = (int *)L.nregs.ensure((size_t)(n_sb + 1) * 4);
		HIP_OK(hipMemcpyAsync(d_chain_beg, chain_beg, (size_t)n_sb * 4, hipMemcpyHostToDevice, lst));
		HIP_OK(hipMemcpyAsync(d_chain_cnt, chain_cnt, (size_t)n_sb * 4, hipMemcpyHostToDevice, lst));
		HIP_OK(hipMemcpyAsync(d_reg_beg, reg_beg, (size_t)n_sb * 4, hipMemcpyHostToDevice, lst));
		if (NC) HIP_OK(hipMemcpyAsync(d_chains + base, hchains, (size_t)NC * sizeof(DevChain), hipMemcpyHostToDevice, lst));
		if (NS) HIP_OK(hipMemcpyAsync(d_seeds + base, hseeds, (size_t)NS * sizeof(DevSeed), hipMemcpyHostToDevice, lst));
		if (NS) HIP_OK(hipMemcpyAsync(d_srt + base, hsrt, (size_t)NS * 4, hipMemcpyHostToDevice, lst));
		unsigned long long *d_c2a_stat = (unsigned long long *)L.c2a_stat.ensure(C2A_STAT_SLOTS * 64);
		HIP_OK(hipMemsetAsync(d_c2a_stat, 0, C2A_STAT_SLOTS * 64, lst));
		// launch order: reads by decreasing number of seeds (counting sort), the long-running ones first
		int *order = (int *)L.h_order.ensure((size_t)n_sb * 4 + 8);
		c2a_launch_order(n_sb, nseeds, order);
		int *d_order = (int *)L.order.ensure((size_t)n_sb * 4);
		HIP_OK(hipMemcpyAsync(d_order, order, (size_t)n_sb * 4, hipMemcpyHostToDevice, lst));
		// Reads with more than a handful of chains (high-copy repeats: hundreds of chains at hundreds of loci) are not walked by one
		// wavefront: their chains are split into groups that cannot see each other's regions (c2a_groups.hip), a unit of c2a_kernel each.
		// MPIBWA_C2A_HEAVY=<chains> moves the threshold (0: every read is walked by one wavefront, as before round 4).
		static const int heavy_t = getenv("MPIBWA_C2A_HEAVY") ? atoi(getenv("MPIBWA_C2A_HEAVY")) : 8;
		const C2aUnits units = c2a_prepare_units(lst, L.grp, heavy_t, n_sb, chain_cnt, (size_t)std::max<int64_t>(base + NC, 1), d_chain_beg, d_reg_beg,
		                                         d_chains, d_nregs, [](void *s) { stream_wait((hipStream_t)s); });
		C2aParams cp;
		ExtParams ep;
		c2a_params(opt, bns->l_pac, c2a_early_mode(), cp, ep);
		// (everything the turn needs is sized before it is taken: an allocation under the lock stalls every caller behind it)
		const int64_t guess = std::min<int64_t>(n_slots, (int64_t)2 * n_sb + 1024);
		uint8_t *d_dd_status = nullptr, *h_dd_status = nullptr;
		int *d_dd_m = nullptr, *d_dd_keep = nullptr, *d_dd_list = nullptr, *h_dd_m = nullptr, *h_dd_keep = nullptr;
		std::unique_ptr<EvTimer> ev_dd;
		if (dev_dedup) {
			ev_dd.reset(new EvTimer());
			d_dd_status = (uint8_t *)L.dd_status.ensure((size_t)n_sb);
			d_dd_m = (int *)L.dd_m.ensure((size_t)n_sb * 4);
			d_dd_keep = (int *)L.dd_keep.ensure((size_t)n_slots * 4);
			d_dd_list = (int *)L.dd_list.ensure(dedup_list_ints(n_sb) * 4);
			h_dd_status = (uint8_t *)L.h_dd_status.ensure((size_t)n_sb + 8);
			h_dd_m = (int *)L.h_dd_m.ensure((size_t)n_sb * 4 + 8);
			h_dd_keep = (int *)L.h_dd_keep.ensure((size_t)guess * 4 + 8);
		}
		stage(50);
		std::unique_lock<TurnLock> turn(g_c2a_turn, std::defer_lock);
		if (take_turns) turn.lock();
		stage(51);
		ev_ext.start(lst);
		// one wavefront per read (any read length)
		launch_c2a(lst, cp, ep, n_sb, d_seq, d_off_r, d_len_r, d_chain_beg, d_chain_cnt, d_chains, d_seeds, d_srt, d_reg_beg, d_regs, d_nregs,
		           d_tab, TS, (const uint8_t *)ix.d_pac, d_c2a_stat, max_len, d_order, units.max_units > 0 ? &units : nullptr);
		ev_ext.stop(lst);
		// the regions sit in sparse per-read slots: prefix-sum + pack on the device, queued behind the kernel, then one
		// copy of what is usually enough (2 regions per read); the rare rest follows once the total is known
		int *d_reg_pos = (int *)L.reg_pos.ensure((size_t)(n_sb + 1) * 4);
		DevReg *d_packed = (DevReg *)L.regs_packed.ensure((size_t)n_slots * sizeof(DevReg));
		const size_t tmp_bytes = reg_pack_tmp_bytes(n_sb);
		void *d_tmp = L.pack_tmp.ensure(tmp_bytes);
		launch_reg_pack(lst, n_sb, d_reg_beg, d_nregs, d_reg_pos, d_regs, d_packed, d_tmp, tmp_bytes, units.max_units > 0 ? &units : nullptr, d_chain_beg, d_chain_cnt);
		if (d_pr_first) launch_first_reg(lst, n_sb, d_reg_pos, d_nregs, d_packed, d_pr_first + (size_t)lo * PR_MAXREG, d_pr_nfirst + lo);
		if (dev_dedup) {   // reads the raw lists, writes none of them: first_reg_kernel and the copies below see what reg_pack left
			ev_dd->start(lst);
			launch_dedup(lst, dedup_params(opt, bns->l_pac), n_sb, d_packed, d_reg_pos, d_nregs, d_dd_status, d_dd_m, d_dd_keep, d_dd_list);
			ev_dd->stop(lst);
		}
		hregs = (DevReg *)L.h_regs.ensure((size_t)guess * sizeof(DevReg) + 8);
		unsigned long long *stat_h = (unsigned long long *)L.h_c2a_stat.ensure(C2A_STAT_SLOTS * 64);
		HIP_OK(hipMemcpyAsync(stat_h, d_c2a_stat, C2A_STAT_SLOTS * 64, hipMemcpyDeviceToHost, lst));
		HIP_OK(hipMemcpyAsync(nregs, d_nregs, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
		HIP_OK(hipMemcpyAsync(hregs, d_packed, (size_t)guess * sizeof(DevReg), hipMemcpyDeviceToHost, lst));
		if (dev_dedup) {
			HIP_OK(hipMemcpyAsync(h_dd_status, d_dd_status, (size_t)n_sb, hipMemcpyDeviceToHost, lst));
			HIP_OK(hipMemcpyAsync(h_dd_m, d_dd_m, (size_t)n_sb * 4, hipMemcpyDeviceToHost, lst));
			HIP_OK(hipMemcpyAsync(h_dd_keep, d_dd_keep, (size_t)guess * 4, hipMemcpyDeviceToHost, lst));
		}
		stream_wait(lst);
		HIP_OK(hipGetLastError());
		if (take_turns) turn.unlock();
		ps.k_ext = ev_ext.ms();
		for (int k = 0; k < 4; ++k) { cnt[k] = 0; for (int sl = 0; sl < C2A_STAT_SLOTS; ++sl) cnt[k] += stat_h[sl * 8 + k]; }
		ps.cells = cnt[0]; ps.n_ext = cnt[1];
		if (cp.early == 2 && cnt[3]) die("c2a_kernel: %llu of %llu extensions change when their row loops stop early", cnt[3], cnt[1]);
		if (getenv("MPIBWA_CPUSEC")) fprintf(stderr, "[c2a] %llu extensions, %llu without DP, %llu cells, kernel %.2f ms\n", cnt[1], cnt[2], cnt[0], ev_ext.ms());
		for (int i = 0; i < n_sb; ++i) reg_pos[i + 1] = reg_pos[i] + nregs[i];
		const int64_t NR = reg_pos[n_sb];
		if (NR > guess) {
			DevReg *all = (DevReg *)L.h_regs2.ensure((size_t)NR * sizeof(DevReg) + 8);
			HIP_OK(hipMemcpyAsync(all, d_packed, (size_t)NR * sizeof(DevReg), hipMemcpyDeviceToHost, lst));
			if (dev_dedup) {
				int *all_keep = (int *)L.h_dd_keep2.ensure((size_t)NR * 4 + 8);
				HIP_OK(hipMemcpyAsync(all_keep, d_dd_keep, (size_t)NR * 4, hipMemcpyDeviceToHost, lst));
				h_dd_keep = all_keep;
			}
			stream_wait(lst);
			hregs = all;
		}
		if (dev_dedup) {
			dd_status = h_dd_status; dd_m = h_dd_m; dd_keep = h_dd_keep;
			ps.k_dedup = ev_dd->ms();
			if (getenv("MPIBWA_CPUSEC")) {
				unsigned long long c[5] = {0, 0, 0, 0, 0};
				for (int i = 0; i < n_sb; ++i) ++c[dd_status[i] < 5 ? dd_status[i] : 0];
				fprintf(stderr, "[dedup] kernels %.2f ms; reads taken %llu, more than %d regions %llu, to patch %llu\n", ps.k_dedup, c[DD_TAKEN], DD_MAXREG,
				        c[DD_HOST_MAXREG], c[DD_HOST_PATCH]);
			}
		}
	}
	double t5 = now_ms();
	stage(6);

	// region post-processing (host); every read gets a slice of the batch-wide arena: its regions + room for rescued mates
	const int SLACK = 4;
	std::vector<int64_t> slice(n_sb + 1);
	slice[0] = 0;
	for (int i = 0; i < n_sb; ++i) slice[i + 1] = slice[i] + nregs[i] + SLACK;
	HReg *arena = (HReg *)reg_arena.ensure((size_t)slice[n_sb] * sizeof(HReg));
	parallel_for(lane_thr, n_sb, 256, [&](int i) {
		HRegV &v = regs[lo + i];
		const int n_raw = nregs[i];
		// a read the device took: its survivors gathered in the reference's final order, nothing to sort; every other read from its raw list
		const bool taken = dd_status && dd_status[i] == DD_TAKEN;
		const int m = taken ? dd_m[i] : n_raw;
		v.attach(arena + slice[i], (uint32_t)(n_raw + SLACK));
		v.resize(m);
		for (int k = 0; k < m; ++k) {
			const DevReg &d = hregs[reg_pos[i] + (taken ? dd_keep[reg_pos[i] + k] : k)];
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
	// insert-size votes of this sub-batch (src/bwamem_pair.c:52-63), so that the barrier only has to add histograms up
	if (pes_hist) {
		const int plo = lo >> 1, np_ = n_sb >> 1, nt = std::max(1, std::min(lane_thr, np_ / 4096));
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
	for (int i = 0; i < n_sb; ++i)
		if (nregs[i] > 1) ++(dd_status && dd_status[i] == DD_TAKEN ? ps.n_dedup_dev : ps.n_dedup_host);
	double t6 = now_ms();
	ps.smem = t2 - t1; ps.sa = t3 - t2; ps.chain = t4 - t3; ps.ext = t5 - t4; ps.regs = t6 - t5;
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
