// pipeline.h — what pipeline.hip (contexts, admission, statistics, mem_process_seqs), phase1.hip (one sub-batch from seeding to
// regions) and sam_stage.hip (decisions, CIGAR-and-SAM jobs, records) share: the helper threads, the call context and its work
// buffers, and the state of one call with its stages.  Internal to the three files.
#ifndef MBW_PIPELINE_H
#define MBW_PIPELINE_H
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <initializer_list>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include <sys/resource.h>
#include <sys/time.h>
#include <unistd.h>

#include "hip_util.h"
#include "device.h"
#include "host.h"
#include "hprof.h"


namespace mbw {

int usable_cpus();
int host_threads(const mem_opt_t *opt);

// ---- the library's helper threads ----
// One persistent pool for all calls in flight (created on first use, as many threads as the rank's share of the node's CPUs).  A parallel region
// queues one ticket per helper it would like; a pool thread that takes a ticket runs the region's work loop until the region's
// items are gone; the caller runs the same loop, then withdraws the tickets nobody has taken and waits for the helpers that
// did start.  (Regions used to create and join their own threads: ~450 thread creations per call, six calls in flight — stack
// mappings, page faults and exits that all serialise on the process's address-space lock — and up to 96 runnable threads on 16 cores.)
// MPIBWA_THREAD_POOL=0: threads per region as before.
class HelperPool {
public:
	struct Job {
		void (*run)(void *, int);   // (region, helper number 1..)
		void *region;
		std::atomic<int> started{0}, finished{0};
	};
	static HelperPool &get() { static HelperPool *p = new HelperPool;   // never destroyed: its threads wait on it until the process ends
		return *p; }
	bool enabled() const { return !th_.empty(); }
	void run(int helpers, Job &job, void (*self)(void *), void *region)
	{
		if (helpers > 0) {
			{
				std::lock_guard<std::mutex> lk(m_);
				for (int t = 0; t < helpers; ++t) q_.push_back(&job);
			}
			for (int t = 0; t < helpers; ++t) cv_.notify_one();   // (not notify_all: the pool may hold many more threads than this region asks for)
		}
		self(region);
		if (helpers > 0) {
			int mine = 0;
			{
				std::lock_guard<std::mutex> lk(m_);
				for (auto it = q_.begin(); it != q_.end();)
					if (*it == &job) { it = q_.erase(it); ++mine; } else ++it;
			}
			const int took = helpers - mine;   // tickets a pool thread has taken (it bumps `finished` when it is done with the region)
			for (int spin = 0; job.finished.load(std::memory_order_acquire) < took; ++spin)
				if (spin < 200) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(20));
		}
	}
private:
	HelperPool()
	{
		const char *e = getenv("MPIBWA_THREAD_POOL");
		if (e && atoi(e) == 0) return;
		const int n = host_threads(nullptr);   // this rank's share of the node's CPUs (MPIBWA_HOST_THREADS overrides)
		for (int t = 0; t < n; ++t) th_.emplace_back([this]() { loop(); });
		for (auto &t : th_) t.detach();   // they live as long as the process
	}
	void loop()
	{
		for (;;) {
			Job *j;
			{
				std::unique_lock<std::mutex> lk(m_);
				cv_.wait(lk, [this]() { return !q_.empty(); });
				j = q_.front();
				q_.pop_front();
			}
			const int tid = j->started.fetch_add(1) + 1;
			j->run(j->region, tid);
			if (g_hprof_on) t_hprof.flush();   // (hprof.h: a helper's record is folded in when it leaves a region)
			j->finished.fetch_add(1, std::memory_order_release);
		}
	}
	std::mutex m_;
	std::condition_variable cv_;
	std::deque<Job *> q_;
	std::vector<std::thread> th_;
};

template <class F>
static void parallel_for(int n_threads, int n, int chunk, F f)
{
	if (n <= 0) return;
	if (n_threads <= 1 || n <= chunk) { for (int i = 0; i < n; ++i) f(i); return; }
	struct Region {
		std::atomic<int> next{0};
		int n, chunk;
		F *f;
		void work()
		{
			for (;;) {
				int b = next.fetch_add(chunk);
				if (b >= n) break;
				int e = std::min(n, b + chunk);
				for (int i = b; i < e; ++i) (*f)(i);
			}
		}
	} R;
	R.n = n; R.chunk = chunk; R.f = &f;
	const int helpers = std::min(n_threads - 1, (n + chunk - 1) / chunk - 1);
	HelperPool &P = HelperPool::get();
	if (P.enabled()) {
		HelperPool::Job job;
		job.run = [](void *r, int) { ((Region *)r)->work(); };
		job.region = &R;
		P.run(helpers, job, [](void *r) { ((Region *)r)->work(); }, &R);
		return;
	}
	std::vector<std::thread> th;
	for (int t = 0; t < helpers; ++t) th.emplace_back([&R]() { R.work(); });
	R.work();
	for (auto &t : th) t.join();
}

// same, handing whole blocks to f(thread, block, lo, hi) so that a stage can keep per-thread scratch and per-block output
// (thread numbers are 0 .. n_threads - 1 and unique among the threads working on the region at the same time)
template <class F>
static void parallel_blocks(int n_threads, int n, int chunk, F f)
{
	if (n <= 0) return;
	const int nb = (n + chunk - 1) / chunk;
	if (n_threads > nb) n_threads = nb;
	struct Region {
		std::atomic<int> next{0};
		int n, nb, chunk;
		F *f;
		void work(int tid)
		{
			for (;;) {
				int b = next.fetch_add(1);
				if (b >= nb) break;
				(*f)(tid, b, b * chunk, std::min(n, (b + 1) * chunk));
			}
		}
	} R;
	R.n = n; R.nb = nb; R.chunk = chunk; R.f = &f;
	HelperPool &P = HelperPool::get();
	if (P.enabled() && n_threads > 1) {
		HelperPool::Job job;
		job.run = [](void *r, int tid) { ((Region *)r)->work(tid); };
		job.region = &R;
		P.run(n_threads - 1, job, [](void *r) { ((Region *)r)->work(0); }, &R);
		return;
	}
	std::vector<std::thread> th;
	for (int t = 1; t < n_threads; ++t) th.emplace_back([&R, t]() { R.work(t); });
	R.work(0);
	for (auto &t : th) t.join();
}

double now_ms();
double sys_sec();
long page_faults();
double cpu_sec();
// where the calling thread's call is (MPIBWA_SAMPLE, pipeline.hip); stream_wait marks the stage as waiting for the GPU
void stage(int id);
// Wait for a stream without burning a core (pipeline.hip)
void stream_wait(hipStream_t st);
// MPIBWA_CPUSEC: the stages print where their host cycles and their work items went (read once per process)
inline bool cpusec_on() { static const bool on = getenv("MPIBWA_CPUSEC") != nullptr; return on; }

// The turns on the big kernels of phase 1 are taken in the order of arrival.  With a plain mutex a caller whose thread had to be
// scheduled first (more runnable threads than cores) kept losing the turn to callers that were already running: now and then a chunk
// that takes 0.6 s took 3 s with eight callers, the others none the faster for it.
// Whoever holds a turn must not allocate: the code between lock() and unlock() is a function of plain pointers.
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

struct EvTimer {
	hipEvent_t a, b;
	EvTimer() { HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); }
	~EvTimer() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
	void start(hipStream_t s) { HIP_OK(hipEventRecord(a, s)); }
	void stop(hipStream_t s) { HIP_OK(hipEventRecord(b, s)); }
	double ms() { HIP_OK(hipEventSynchronize(b)); float m = 0; HIP_OK(hipEventElapsedTime(&m, a, b)); return m; }
};

// grow-only host buffer kept across calls (no page faults / frees per chunk)
struct HostBuf {
	void *p = nullptr; size_t cap = 0;
	void *ensure(size_t bytes) { if (bytes > cap) { free(p); cap = bytes + bytes / 4 + 4096; p = malloc(cap); if (!p) die("out of memory"); } return p; }
};

// ---- device work buffers, grown on demand and kept across calls ----
// (every copy to or from the device uses page-locked host memory: a pageable target makes hipMemcpyAsync wait — spinning —
// for the kernels queued before it, and a pageable source is pinned page by page at every call)
// What one lane of phase 1 uses for the sub-batch it is working on (phase1.hip)
struct LaneBufs {
	PinBuf h_nch, h_cbeg, h_ccnt, h_rbeg, h_nseeds, h_lrep, h_nintv, h_cnt, h_seed_off, h_c2a_stat, h_order;
	PinBuf h_sa, h_qbl, h_chains, h_seeds, h_srt, h_regs, h_regs2, h_nregs;
	DevBuf nch, chain_cnt, reg_pos, regs_packed, pack_tmp, order, chain_scratch, c2a_stat;
	// reads with many chains, extended as independent groups of chains (c2a_groups.hip)
	C2aGroupBufs grp;
	DevBuf intv, nintv, cnt, scratch, nseeds, lrep, seed_off, rows, qbl, sa;
	DevBuf chain_off, chains, seeds, srt, reg_off, regs, nregs, tab;
	// the redundancy pass on the device (dedup_kernel.hip): status and survivor count per read, the survivors' places per region slot, the
	// wave kernel's list; the host copies (the places come back in two steps, like the regions)
	DevBuf dd_status, dd_m, dd_keep, dd_list;
	PinBuf h_dd_status, h_dd_m, h_dd_keep, h_dd_keep2;
};
// One CIGAR-and-SAM job of the SAM stage (sam_stage.hip): requests (the host's: the units decided on the device bring their own array),
// result headers and pool, counters, the kernel's lists; request base per unit, record arena, its cursor, record offsets and lengths
struct JobBufs {
	DevBuf req, hdr, pool, cnt, lists, base, arena, used, ooff, olen;
	PinBuf h_hdr, h_pool, h_base, h_arena, h_ooff, h_olen;
};
// One work list of a wave kernel: the units handed over (chunk numbering), their packed region lists and the lists' offsets, per pair
// the first rescue request, the tags and their offsets, status bytes, the kernel's requests and descriptors, the XA entries' requests and
// counts, and where each item's requests go in the job of the units it decided (dst).  pair_wave_kernel: one list per part of the
// SAM stage, behind the part's mate-rescue kernel; se_wave_kernel: one over the chunk, in slot 0 (a call is either paired or
// single-end), with dst still the part's slot: both parts' jobs are in flight at once.
struct WaveBufs {
	PinBuf h_work, h_lists, h_loff, h_mfirst, h_tags, h_toff, h_status, h_xcnt, h_dst;
	DevBuf work, lists, loff, mfirst, tags, toff, status, req, desc, xreq, xcnt, dst;
	// se_wave_kernel's reads of several lines (device.h: SeLines): line counts per item, and per (item, line) descriptors, requests, XA
	// counts and XA requests; ldst: where such an item's requests go in the part's job (the part's slot, like dst)
	PinBuf h_nlines, h_lxcnt, h_ldst;
	DevBuf nlines, ldesc, lreq, lxcnt, lxreq, ldst;
};
// What belongs to the chunk as a whole: packed reads, the inputs of the SAM stage, the decisions made on the device, and per part of
// the SAM stage the mate-rescue alignments and the two jobs
struct ChunkBufs {
	PinBuf h_off, h_len, h_flat;
	DevBuf seq, off, len, ann_off, ann_alt, agap;
	// SAM text on the device (sam_kernel.hip): line descriptors, names / qualities of the chunk, contig names
	DevBuf sdesc, squal, snames, snoff, sann_names, sann_noff;
	PinBuf h_sdesc, h_names, h_noff, h_qual;
	// units decided on the device (pair_kernel.hip, se_kernel.hip): first regions / region count per read, flags, tables, requests, descriptors
	DevBuf pr_first, pr_nfirst, pr_ok, pr_status, pr_ptab, pr_req, pr_desc;
	PinBuf h_pr_ok, h_pr_status, h_pr_tab;
	PinBuf h_mreq[2], h_mres[2], h_mlist[2];
	DevBuf mreq[2], mres[2], mrows[2], mlist[2], mtail[2];
	// the work lists of the wave kernels, the job of pair_wave_kernel's pairs when the device units' job of the part has already gone out,
	// and the job of the units with requests of their own count (XA entries; se_wave_kernel's reads): its requests, and its descriptors
	// (chunk-wide, by read)
	WaveBufs wave[2];
	JobBufs wave_job[2];
	DevBuf xa_req[2], xa_desc;
	JobBufs xa_job[2];
	PinBuf h_areq[2];     // the host's CIGAR requests of a part, as listed
	JobBufs host_job[2];  // the host's units ...
	JobBufs dev_job[2];   // ... and the units decided on the device, launched right behind the deciding kernel
	PinBuf h_small[2];    // counters coming back from the jobs (a pageable target would make the copy spin behind queued kernels)
};
static const int MAX_LANES = 4;
static const int MAX_CALLS = 12;
// Everything one mem_process_seqs() call owns between its first and last line.  MAX_CALLS of them: that many caller threads may be
// inside the function at once (chunk i+1 seeding and extending on the GPU while the host pairs and prints chunk i — the stage that
// keeps the GPU busy and the stage that keeps the host busy belong to different halves of a call).  One caller more waits.
struct CallCtx {
	// (first and last members: every DevBuf constructed in between enters `bufs`)
	std::vector<DevBuf *> bufs;
	struct Open { Open(std::vector<DevBuf *> *l) { g_devbuf_owner = l; } } open_{&bufs};
	// ws[lane] / reg_arena[k]: a call with neighbours in flight runs its chunk in one piece through ws[0], a lone call its two
	// sub-batches through ws[0] and ws[1].  The buffers only grow, so a context that has served a lone call regrows ws[0] ONCE,
	// at its first whole chunk (65 buffers: hipFree + hipMalloc stall every stream) — a caller that wants that out of its
	// measurements starts its first rounds of calls together, as bench.py's warm-up does.  (Separate buffer sets per mode
	// were tried: no regrowth at all, but twice the footprint in the first two contexts, and the repeat-rich workload of §6.1
	// no longer fitted with four calls in flight.)
	LaneBufs ws[MAX_LANES];
	HostBuf reg_arena[17];     // the regions live until the SAM stage
	ChunkBufs gws;
	hipStream_t p_streams[MAX_LANES] = {nullptr}, a_streams[2] = {nullptr, nullptr}, d_streams[2] = {nullptr, nullptr};
	bool busy = false;
	const bseq1_t *seq_lo = nullptr, *seq_hi = nullptr;   // the caller's array while the call runs
	int calls_done = 0;   // since its buffers were last given back (under g_ctx_mu)
	struct Close { Close() { g_devbuf_owner = nullptr; } } close_;
	size_t device_bytes() const { size_t b = 0; for (const DevBuf *d : bufs) b += d->cap; return b; }
	void release_device() { for (DevBuf *d : bufs) d->release(); calls_done = 0; }
};

// ---- one call ----
// what a sub-batch of phase 1 reports: kernel times, wall times per stage, counters
struct P1 { double k_smem = 0, k_sa = 0, k_ext = 0, k_dedup = 0, smem = 0, sa = 0, chain = 0, ext = 0, regs = 0; uint64_t smem_bytes = 0, smem_tab_bytes = 0, sa_bytes = 0, cells = 0, n_ext = 0, n_intv = 0, n_seeds = 0, n_chains = 0, n_dedup_dev = 0, n_dedup_host = 0; };

// What a sub-batch of phase 1 carries from stage to stage (phase1.hip): reads lo .. hi of the chunk on the lane's stream, with the lane's
// buffers and up to lane_thr host threads; every pointer below is into those buffers (d_*: device; the others: page-locked host copies)
struct SubBatch {
	const int lo, hi, n_sb;
	LaneBufs &L; HostBuf &reg_arena; const hipStream_t lst; const int lane_thr; P1 &ps;
	// encode: a block of counters, the length tables of c2a_length_tables (row 0: cal_max_gap) and their stride
	unsigned long long *d_cnt = nullptr, *cnt = nullptr;
	std::vector<int> tab;
	int *d_tab = nullptr, TS = 0;
	// seed: the capacity per read that held every interval list, the lists and their lengths; seeds / l_rep / intervals per read
	int cap = 0;
	bool count_blocks = false;        // MPIBWA_SMEM_COUNT
	uint64_t *d_intv = nullptr;
	int *d_nintv = nullptr, *d_nseeds = nullptr, *d_lrep = nullptr, *nseeds = nullptr, *lrep = nullptr, *nintv = nullptr;
	// sa_and_chain: read i's seeds are seed_off[i] .. seed_off[i + 1] of S; their SA values and (qbeg, len) pairs where the host chains
	int64_t *seed_off = nullptr, S = 0;
	uint64_t *sa = nullptr; int32_t *qbl = nullptr;
	bool dev_chain = false;           // chain_kernel ran: nch[i] = chains it kept for read i, -1 = the host's read
	int *nch = nullptr;
	// host_chain: NC chains and NS kept seeds of the host-chained reads, behind `base` slots on the device; n_slots = size of the seed /
	// order / region arrays there; per read its first chain, its chains, its first region slot
	int64_t base = 0, n_slots = 0;
	int NC = 0, NS = 0;
	DevChain *hchains = nullptr; DevSeed *hseeds = nullptr; unsigned int *hsrt = nullptr;
	int *chain_beg = nullptr, *chain_cnt = nullptr, *reg_beg = nullptr;
	// extend: regions per read, where they start in hregs; the redundancy pass on the device: status / survivors / their places in the
	// raw list, per read (null: not run)
	int *nregs = nullptr;
	std::vector<int> reg_pos;
	DevReg *hregs = nullptr;
	const uint8_t *dd_status = nullptr;
	const int *dd_m = nullptr, *dd_keep = nullptr;
};

// One CIGAR-and-SAM job in flight: what was launched, and the host copies of what came back
struct Job {
	JobBufs *B = nullptr;
	bool launched = false, sam_launched = false;
	hipStream_t st = 0;
	size_t n_req = 0, pool_bytes = 0, arena_bytes = 0;
	int n_reads = 0;
	AlnHdr *d_hdr = nullptr; uint8_t *d_pool = nullptr; unsigned long long *d_cnt = nullptr;
	unsigned long long *small_cnt = nullptr, *small_used = nullptr;   // its slots of h_small
	EvTimer ev;
	const AlnHdrH *hdr = nullptr; const uint8_t *pool = nullptr;   // CIGAR results
	// records written by sam_emit_kernel: arena / offsets / lengths, for the reads of the part
	const uint8_t *sarena = nullptr; const unsigned long long *sooff = nullptr; const int *solen = nullptr;
};
// A part of the chunk in the SAM stage: units lo .. hi (pairs, or single-end reads)
struct Part {
	int lo = 0, hi = 0, slot = 0;
	AlnReqH *req = nullptr;           // the host's CIGAR requests of the part, in a page-locked buffer of the call context
	size_t n_req = 0;
	std::vector<uint32_t> base;       // first request of every unit of the part
	Job host;                         // the host's units
	Job dev;                          // the units decided on the device: their requests (the deciding kernel's array, in place) and records
	// mate-rescue alignments of the part: requests of unit k are mreq[mbase[k] .. mbase[k+1])
	MswReqH *mreq = nullptr; MswResH *mres = nullptr;
	std::vector<uint32_t> mbase;
	size_t n_mreq = 0;
	hipStream_t mst = 0;
	EvTimer mev;
	bool m_launched = false, msw_launched = false;
	// the pairs handed to pair_wave_kernel (chunk numbering), their status bytes once mfinish has waited, how many it decided
	std::vector<int> work;
	std::vector<unsigned> w_mfirst;
	std::vector<int> w_toff;
	std::vector<int16_t> w_tags;
	const uint8_t *wstatus = nullptr;
	int n_wave_dec = 0;
	Job wave;                         // the job of the pairs it decided, when they do not ride in `dev`
	const uint8_t *wxcnt = nullptr;   // XA entries per (work item, end), with the status bytes
	const uint8_t *wnlines = nullptr, *wlxcnt = nullptr;   // (dev_pair_lines) lines per (work item, end); XA entries per (work item, end, line)
	int n_lines_dec = 0;              // the pairs it decided end by end (PW_DECIDED_LINES): they ride in the job of the XA pairs
	int n_xa_dec = 0;                 // the pairs it decided with an XA tag, their request bases (per unit of the part) and their job
	std::vector<uint32_t> xa_base;
	Job xa;
	// CIGAR requests while they are being listed: per block of 256 units, and where each unit's run starts
	std::vector<std::vector<AlnReqH>> blk_req;
	std::vector<uint32_t> u_first, u_cnt;
};

// What one mem_process_seqs() invocation owns, and its stages in the order mem_process_seqs runs them
struct Call {
	// ---- arguments, context ----
	const mem_opt_t *const opt; const bntseq_t *const bns; const uint8_t *const pac;
	const int64_t n_processed; const int n; bseq1_t *const seqs; const mem_pestat_t *const pes0;
	DevIndex &ix; CallCtx &C; ChunkBufs &W; mi355x_stats_t &STAT;
	const bool crowded;               // other calls in flight (CtxLease)
	const int n_thr; const bool pe;
	const hipStream_t st;             // never the null stream: another call may be in flight
	Call(const mem_opt_t *opt_, const bntseq_t *bns_, const uint8_t *pac_, int64_t n_processed_, int n_, bseq1_t *seqs_, const mem_pestat_t *pes0_,
	     DevIndex &ix_, CallCtx &C_, mi355x_stats_t &STAT_, bool crowded_)
		: opt(opt_), bns(bns_), pac(pac_), n_processed(n_processed_), n(n_), seqs(seqs_), pes0(pes0_), ix(ix_), C(C_), W(C_.gws), STAT(STAT_),
		  crowded(crowded_), n_thr(host_threads(opt_)), pe((opt_->flag & MEM_F_PE) != 0), st(C_.p_streams[0]), regs(n_) {}

	// ---- the packed chunk (pack) ----
	int64_t *off = nullptr;           // 16-byte aligned slot of every read in the packed buffer
	int *lens = nullptr;
	int max_len = 0;
	size_t flat_bytes = 0;
	uint8_t *flat = nullptr;
	ChunkDev D;                       // what is resident of it (the SAM inputs: once sam_inputs is joined)
	void pack();                      // offsets, lengths, contig table: host and device

	// ---- feature flags, inputs of the SAM stage (sam_stage.hip) ----
	bool gpu_aln = false, gpu_sam = false, se_want = false, dev_se = false, dev_pair = false;
	SamDescH *sdesc = nullptr;
	SamParams sam_par;
	struct Joiner {   // (a call that dies on the way out must not leave the thread running on its buffers)
		std::thread t;
		void join() { if (t.joinable()) t.join(); }
		~Joiner() { join(); }
	} sam_inputs;
	void start_sam_inputs();          // names, qualities, contig names, gap table: packed and uploaded by a thread of their own
	void sam_inputs_body();

	// ---- phase 1 (phase1.hip) ----
	std::vector<HRegV> regs;
	std::vector<uint64_t> pes_hist_v; // insert-size votes, gathered sub-batch by sub-batch (when they will be needed and can be counted)
	uint64_t *pes_hist = nullptr;
	DevReg *d_pr_first = nullptr;     // first regions / region count of every read, left by every sub-batch for the deciding kernels
	int *d_pr_nfirst = nullptr;
	int n_sub = 1, n_lanes = 1;
	void phase1_all();                // the sub-batches over the lanes
	void phase1(int lo, int hi, LaneBufs &L, HostBuf &reg_arena, hipStream_t lst, int lane_thr, P1 &ps);   // the schedule of one sub-batch over:
	void encode(SubBatch &B);         // nt4 codes in place and on the device, the length tables
	void seed(SubBatch &B);           // SMEM seeding and the seed counts, under the seeding turn
	void sa_and_chain(SubBatch &B);   // seed enumeration, SA lookup, chaining on the device, the seeds of the reads it declined
	void host_chain(SubBatch &B);     // those reads chained by the host; the device layout of all chains
	void extend(SubBatch &B);         // chain -> regions under the extension turn, the regions' way back
	void regions(SubBatch &B);        // mem_sort_dedup_patch per read (or the device's survivors), into slices of the arena
	void votes(SubBatch &B);          // the insert-size votes of the sub-batch

	// ---- insert-size statistics ----
	mem_pestat_t pes[4];

	// ---- units decided on the device (sam_stage.hip) ----
	uint8_t *ustat = nullptr;            // the deciding kernel's status byte per unit (PR_* / SE_*), the wave kernels' decisions merged in
	bool dev_units = false;              // at least one unit is the device's (ustat[k] = *_DECIDED: its requests and descriptors exist there)
	bool dev_wave = false;               // pair_wave_kernel takes the pairs pair_simple_kernel leaves for rescue / long lists
	bool dev_xa = false;                 // ... and the ones it leaves for an XA tag; it lists the tag's entries (MPIBWA_HOST_XA=1: off)
	bool dev_pair_lines = false;         // ... and the ones mem_sam_pe reports end by end (MPIBWA_HOST_PAIR_LINES=1: off)
	uint64_t n_pair_lines = 0;           // decided that way
	std::atomic<unsigned long long> n_pair_lines_sam{0};   // ... whose text was taken from the device
	uint64_t n_xa_pairs = 0;             // decided with an XA tag, or handed over for the XA test alone and decided without one
	uint64_t n_xa_plain = 0;             // (the latter: status PR_DECIDED, riding with the wave's other pairs)
	std::vector<uint8_t> wave_cand, wave_dec;   // per pair: handed to pair_wave_kernel; decided by it
	PairParams wave_pp;
	const double *d_wave_tab = nullptr;  // the tables of decide_on_device, still on the device
	size_t wave_n_tab = 0;
	uint64_t n_wave = 0;
	// single-end reads se_simple_kernel left for more than eight regions or for its XA test: se_wave_kernel, once over
	// the chunk on the call's stream.  Its decided reads' job of every part is Part::xa with the request bases Part::xa_base, wave_dec
	// marks the reads it decided
	WaveBufs &se_bufs() { return W.wave[0]; }   // its work list (WaveBufs)
	bool dev_se_wave = false;            // MPIBWA_HOST_SE_WAVE=1: off
	bool dev_se_xa = false;              // ... with its XA listing (MPIBWA_HOST_XA=1 or max_XA_hits > PW_XA_CAP: off)
	std::vector<int> se_work;            // the reads handed to it (chunk numbering, ascending)
	const uint8_t *se_wxcnt = nullptr;   // per work item: its XA entries
	uint64_t n_se_wave = 0, n_se_xa = 0; // decided by it with a plain record / with an XA tag
	std::atomic<unsigned long long> n_se_xa_sam{0};   // records with an XA tag taken from the device
	// ... and the reads se_simple_kernel left for a second primary hit: 2 .. SE_LINES_CAP lines, written by sam_lines_kernel
	bool dev_se_supp = false;            // MPIBWA_HOST_SUPP=1: off
	const uint8_t *se_wnlines = nullptr, *se_wlxcnt = nullptr;   // per work item: its lines; per (item, line): the line's XA entries
	uint64_t n_se_supp = 0;              // decided by it with several lines
	std::atomic<unsigned long long> n_se_supp_sam{0};   // ... whose text was taken from the device
	void se_wave_decide();               // candidates, the kernel over their work list, the merge of its decisions (synchronous)
	// a wave kernel's work list, packed and queued: what the launch needs on the device, and where status bytes and XA counts come back
	struct WaveList {
		int *work; DevReg *lists; int *loff; uint8_t *status; AlnReq *req; SamDesc *desc; AlnReq *xreq; uint8_t *xcnt;
		uint8_t *h_status, *h_xcnt;
		SeLines lines;                   // (lines = true) the side arrays for reads of several lines
		uint8_t *h_nlines, *h_lxcnt;
	};
	struct Upload { void *dst; const void *src; size_t bytes; };
	WaveList wave_list(WaveBufs &B, hipStream_t wst, int ends, const std::vector<int> &items, bool xa, std::initializer_list<Upload> more = {},
	                   bool lines = false);
	// the units of the part a wave kernel decided with a request count of their own: a job of their own (asynchronous)
	void own_job_records(Part &P, int ends, const WaveBufs &B, const std::vector<int> &items, const uint8_t *xcnt);
	const AlnReq *d_pr_req = nullptr;
	const SamDesc *d_pr_desc = nullptr;
	double pair_dev_ms = 0;
	void decide_on_device(int ends);

	// ---- SAM stage (sam_stage.hip) ----
	int n_units = 0, n_parts = 1;
	std::vector<PairPlan> plans;
	Part parts[2];
	bool gpu_msw = false;
	double plan_ms = 0, aln_wait_ms = 0, msw_ms = 0, emit_ms = 0;
	std::atomic<unsigned long long> tsc_plan{0}, tsc_emitc{0}, n_sam_dev{0}, tsc_devcopy{0};
	double cpu_msw = 0, cpu_collect = 0, cpu_emit = 0, sys_emit = 0;
	long pf_emit = 0;
	void sam_stage();                 // the part schedule over the steps below
	void mcollect(Part &P);           // mate rescue: list the local alignments the pairs of the part will ask for
	void mlaunch(Part &P);            // ... run them in one launch (asynchronous)
	void mfinish(Part &P);
	void wave_launch(Part &P);        // pair_wave_kernel behind the mate-rescue kernel of the part (asynchronous)
	void wave_records(Part &P, bool own_job);   // its pairs into the device units' arrays; own_job: and a job of their own
	void collect(Part &P, int round); // A: decisions + the list of CIGARs to compute
	void launch_dev(Part &P);         // the job of the units decided on the device (asynchronous)
	void finish_dev(Part &P);
	void launch(Part &P);             // B: the job of the host's units (asynchronous)
	void finish(Part &P);
	void replay(Part &P, int which);  // C: the records
	enum Fetch { FETCH_ALWAYS, FETCH_IF_HANDED_BACK, FETCH_RECORDS };
	void job_launch(Job &J, JobBufs &B, hipStream_t jst, const Part &P, const AlnReq *d_req, size_t n_req, const uint32_t *base, bool with_sam,
	                const SamDescH *h_desc, SamDesc *d_desc, const WaveBufs *multi = nullptr, int n_multi = 0);
	void job_fetch(Job &J, const Part &P, Fetch policy, bool wave_units = false);
	void take_record(int read, const Job &J, int at);
	void report_decisions();

	// ---- timers ----
	double t_packed = 0, c_packed = 0, t_phase1 = 0, c_phase1 = 0;
};

} // namespace mbw
#endif
