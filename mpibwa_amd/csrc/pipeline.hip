// pipeline.hip — mem_process_seqs(): the drop-in batch driver (replaces src/bwamem.c:1161-1234): call contexts, admission, statistics
// and the entry point.  Phase 1 of a sub-batch is phase1.hip, the SAM stage sam_stage.hip; pipeline.h is what the three share.
//
// The reference runs worker1 (seed -> chain -> extend, per read) and worker2
// (pairing -> SAM, per pair) over pthreads with a batch-wide mem_pestat
// barrier in between.  Here the batch is processed stage by stage:
//
//   host   nt4-encode, pack reads                              (bwamem.c:1057-1058)
//   GPU    SMEM seeding                 smem_kernel            (bwamem.c:114-162)
//   GPU    interval sort / seed enumeration                    (bwamem.c:161, 265-283)
//   GPU    suffix-array lookup          sa_dense_kernel        (bwt.c:86-96)
//   GPU    chaining + chain filters     chain_kernel           (bwamem.c:251-385, 598-617); host for reads beyond one B-tree node
//   GPU    chain -> regions, banded DP  c2a_kernel             (bwamem.c:632-786, ksw.c:380-479)
//   host   dedup / patch, insert-size votes                    (bwamem.c:439-497, bwamem_pair.c:59-109)
//   ---- mem_pestat over the whole chunk ----
//   GPU    mate-rescue local alignment  msw_kernel             (bwamem_pair.c:111-180, ksw.c:111-356)
//   host   pairing decisions                                   (bwamem_pair.c:182-388)
//   GPU    CIGAR / MD / NM              aln_kernel             (bwamem.c:1106-1122, bwa.c:121-207)
//   host   SAM text                                            (bwamem.c:824-1010)
//
// Up to MAX_CALLS calls run side by side (CallCtx, pipeline.h): the GPU-bound first half of one chunk overlaps the host-bound
// second half of another.
//
// There is no CPU fallback for the GPU stages: without a gfx950 device the call aborts.
#include "pipeline.h"

namespace mbw {

static mi355x_stats_t g_stats;

// CPUs this process may actually use: the cgroup CPU quota when there is one, else the online CPU count
static int usable_cpus_now()
{
	int hw = (int)std::thread::hardware_concurrency();
	if (hw <= 0) hw = 1;
	if (FILE *fp = fopen("/sys/fs/cgroup/cpu.max", "r")) {
		char q[64];
		long long period = 0;
		if (fscanf(fp, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
			long long quota = atoll(q);
			int c = (int)((quota + period - 1) / period);
			if (c >= 1 && c < hw) hw = c;
		}
		fclose(fp);
	}
	return hw;
}
// (asked once: every call used to open the cgroup file again, and under eight calls in flight that open alone held a call up
// for milliseconds)
int usable_cpus() { static const int c = usable_cpus_now(); return c; }

// Which GPU a lazily uploading rank takes, and how many ranks share the node: the launcher's environment
// (torchrun, Open MPI, MVAPICH2, Slurm/PMI, Intel MPI / MPICH hydra).  -1 / 0 when the launcher says nothing.
static int env_int(const char *const *names, int dflt)
{
	for (; *names; ++names)
		if (const char *e = getenv(*names)) return atoi(e);
	return dflt;
}
static int env_local_rank()
{
	static const char *const n[] = {"LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", "MV2_COMM_WORLD_LOCAL_RANK", "SLURM_LOCALID", "PMI_LOCAL_RANK",
	                                "MPI_LOCALRANKID", nullptr};
	return env_int(n, -1);
}
static int env_local_size()
{
	static const char *const n[] = {"LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE", "MV2_COMM_WORLD_LOCAL_SIZE", "SLURM_NTASKS_PER_NODE", "PMI_LOCAL_SIZE",
	                                "MPI_LOCALNRANKS", nullptr};
	return env_int(n, 0);
}

int host_threads(const mem_opt_t *opt)
{
	if (const char *e = getenv("MPIBWA_HOST_THREADS")) { int v = atoi(e); if (v > 0) return v; }
	// the result does not depend on the thread count (as in the reference), so use what the box gives us, divided among
	// the ranks that share this node (one rank per GPU) — but never more than the caller's -t when it asked for several
	int ranks = env_local_size();
	if (ranks < 1) ranks = 1;
	int thr = std::max(1, std::min(usable_cpus() / ranks, 128));
	if (opt && opt->n_threads > 1) thr = std::min(thr, opt->n_threads);
	return thr;
}

double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
double sys_sec()
{
	struct rusage r;
	getrusage(RUSAGE_SELF, &r);
	return r.ru_stime.tv_sec + 1e-6 * r.ru_stime.tv_usec;
}
long page_faults()
{
	struct rusage r;
	getrusage(RUSAGE_SELF, &r);
	return r.ru_minflt;
}
double cpu_sec()
{
	struct rusage r;
	getrusage(RUSAGE_SELF, &r);
	return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec);
}

// Wait for a stream without burning a core: hipStreamSynchronize spins, and a spinning thread counts against the
// container's CPU quota like a working one (the host stages are the other half of the bottleneck).  Polling with a short
// sleep costs at most ~0.1 ms per wait.
// MPIBWA_SAMPLE=1: where the calls in flight are, sampled every 250 us (which stage, waiting for a kernel or working on the
// host), printed when the process exits: which stages the calls sit in while nobody keeps the GPU busy, and the other way round
static const int SAMPLE_SLOTS = 64, SAMPLE_STAGES = 64, STG_WAIT = 0x100;
static std::atomic<int> g_stage[SAMPLE_SLOTS];
static thread_local std::atomic<int> *t_stage = nullptr;
void stage(int id) { if (t_stage) t_stage->store(id, std::memory_order_relaxed); }
struct StageSampler {
	std::thread th;
	std::atomic<bool> stop{false};
	uint64_t n_samples = 0, in_stage[SAMPLE_STAGES][2] = {{0}}, by_wait[SAMPLE_SLOTS + 1] = {0}, by_host[SAMPLE_SLOTS + 1] = {0};
	uint64_t host_when_idle[SAMPLE_STAGES] = {0}, n_gpu_idle = 0, n_host_idle = 0;
	int min_calls = 1;   // MPIBWA_SAMPLE=n: only samples with at least n calls in flight count
	void run()
	{
		while (!stop.load()) {
			int nw = 0, nh = 0, st[SAMPLE_SLOTS], ns = 0;
			for (int i = 0; i < SAMPLE_SLOTS; ++i) {
				const int v = g_stage[i].load(std::memory_order_relaxed);
				if (!v) continue;
				st[ns++] = v;
				const int id = v & 63, w = (v & STG_WAIT) != 0;
				if (w) ++nw; else if (id != 20 && id != 50) ++nh;
			}
			if (ns >= min_calls) {
				++n_samples; ++by_wait[nw]; ++by_host[nh];
				for (int k = 0; k < ns; ++k) ++in_stage[st[k] & 63][(st[k] & STG_WAIT) != 0];
				if (!nw) { ++n_gpu_idle; for (int k = 0; k < ns; ++k) ++host_when_idle[st[k] & 63]; }
				if (!nh) ++n_host_idle;
			}
			usleep(250);
		}
	}
	void report()
	{
		if (!n_samples) return;
		fprintf(stderr, "[sample] %llu samples with a call in flight; no call waiting for the GPU in %.1f %%, no call on the host in %.1f %%\n",
		        (unsigned long long)n_samples, 100.0 * n_gpu_idle / n_samples, 100.0 * n_host_idle / n_samples);
		fprintf(stderr, "[sample] calls waiting for the GPU:");
		for (int k = 0; k <= 12; ++k) fprintf(stderr, " %d:%.1f%%", k, 100.0 * by_wait[k] / n_samples);
		fprintf(stderr, "\n[sample] calls working on the host:");
		for (int k = 0; k <= 12; ++k) fprintf(stderr, " %d:%.1f%%", k, 100.0 * by_host[k] / n_samples);
		fprintf(stderr, "\n[sample] stage: mean calls in it on the host / waiting for the GPU / on the host while no call waits for the GPU\n");
		for (int id = 0; id < SAMPLE_STAGES; ++id)
			if (in_stage[id][0] + in_stage[id][1])
				fprintf(stderr, "[sample]   %2d: %.3f %.3f %.3f\n", id, (double)in_stage[id][0] / n_samples, (double)in_stage[id][1] / n_samples,
				        n_gpu_idle ? (double)host_when_idle[id] / n_gpu_idle : 0.0);
	}
};
static StageSampler *g_sampler = nullptr;
void sampler_report()
{
	if (!g_sampler) return;
	g_sampler->stop.store(true);
	g_sampler->th.join();
	g_sampler->report();
	delete g_sampler;
	g_sampler = nullptr;
}

void stream_wait(hipStream_t st)
{
	static const bool spin = getenv("MPIBWA_SPIN_WAIT") != nullptr;
	struct Mark {
		Mark() { if (t_stage) t_stage->fetch_or(STG_WAIT, std::memory_order_relaxed); }
		~Mark() { if (t_stage) t_stage->fetch_and(~STG_WAIT, std::memory_order_relaxed); }
	} mark;
	if (!spin) {
		for (;;) {
			hipError_t e = hipStreamQuery(st);
			if (e == hipSuccess) break;
			if (e != hipErrorNotReady) HIP_OK(e);
			(void)hipGetLastError();   // "not ready" is this thread's last error otherwise: the next library that checks it (RCCL) takes it for a failure
			usleep(60);
		}
	}
	HIP_OK(hipStreamSynchronize(st));
}


// ---- 1. encode + pack: the slot of every read in the packed buffer, lengths, the contig table; on the host and on the device ----
void Call::pack()
{
	stage(29);
	off = (int64_t *)W.h_off.ensure((size_t)(n + 1) * 8 + 64);   // 16-byte aligned slot of every read in the packed buffer
	lens = (int *)W.h_len.ensure((size_t)n * 4 + 64);
	{   // lengths and a prefix sum over 667 000 records the caller has just written: by blocks, on all threads
		const int BLK = 8192, nb = (n + BLK - 1) / BLK;
		std::vector<int64_t> bsum(nb + 1, 0);
		std::vector<int> bmax(nb, 0);
		parallel_for(n_thr, nb, 1, [&](int b) {
			const int lo = b * BLK, hi = std::min(n, lo + BLK);
			int64_t sl = 0;
			int m = 0;
			for (int i = lo; i < hi; ++i) {
				const int l = seqs[i].l_seq;
				lens[i] = l; sl += (l + 15) & ~15; m = std::max(m, l);
			}
			bsum[b + 1] = sl; bmax[b] = m;
		});
		for (int b = 0; b < nb; ++b) { bsum[b + 1] += bsum[b]; max_len = std::max(max_len, bmax[b]); }
		parallel_for(n_thr, nb, 1, [&](int b) {
			const int lo = b * BLK, hi = std::min(n, lo + BLK);
			int64_t o = bsum[b];
			for (int i = lo; i < hi; ++i) { off[i] = o; o += (lens[i] + 15) & ~15; }
		});
		off[n] = bsum[nb];
	}
	stage(30);
	flat_bytes = (size_t)off[n] + 16;
	flat = (uint8_t *)W.h_flat.ensure(flat_bytes);
	if ((size_t)max_len + 2 > 9000) die("read of %d bp exceeds the on-chip band buffers of this build (max 8998 bp)", max_len);
	t_packed = now_ms();
	c_packed = cpu_sec();
	stage(22);
	uint8_t *d_seq = (uint8_t *)W.seq.ensure(flat_bytes);
	int64_t *d_off = (int64_t *)W.off.ensure((size_t)(n + 1) * 8);
	int *d_len = (int *)W.len.ensure((size_t)n * 4);
	// the bases themselves are encoded and uploaded per sub-batch, on the sub-batch's own stream (phase1.hip)
	HIP_OK(hipMemcpyAsync(d_off, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_OK(hipMemcpyAsync(d_len, lens, (size_t)n * 4, hipMemcpyHostToDevice, st));
	HIP_OK(hipStreamSynchronize(st));
	stage(23);
	// contig table for the chaining kernel: start of every contig (+ l_pac) and its ALT flag
	std::vector<int64_t> ann_off;
	std::vector<uint8_t> ann_alt;
	contig_table(bns, ann_off, ann_alt);
	int64_t *d_ann_off = (int64_t *)W.ann_off.ensure(ann_off.size() * 8);
	uint8_t *d_ann_alt = (uint8_t *)W.ann_alt.ensure(ann_alt.size());
	HIP_OK(hipMemcpyAsync(d_ann_off, ann_off.data(), ann_off.size() * 8, hipMemcpyHostToDevice, st));
	HIP_OK(hipMemcpyAsync(d_ann_alt, ann_alt.data(), ann_alt.size(), hipMemcpyHostToDevice, st));
	HIP_OK(hipStreamSynchronize(st));
	D.d_seq = d_seq; D.d_off = d_off; D.d_len = d_len; D.max_len = max_len; D.d_pac = (const uint8_t *)ix.d_pac;
	D.d_ann_off = d_ann_off; D.d_ann_alt = d_ann_alt;
}

static CallCtx g_ctx[MAX_CALLS];
static std::mutex g_ctx_mu;
static std::recursive_mutex g_init_mu;
std::recursive_mutex &index_mutex() { return g_init_mu; }
static std::condition_variable g_ctx_cv;
// Calls admitted at once: MAX_CALLS until a work buffer has failed to fit, then what was in flight at that moment minus one (never
// fewer than one): the callers beyond that wait at the door instead of in the middle of a call.
static int g_admit = MAX_CALLS;             // (under g_ctx_mu)
// What a call context holds in HBM once it has seen a chunk (the largest seen so far) — what a call that starts on a fresh context
// will come to hold.  A call is only let in next to others when the HBM that is free, less what the calls in flight may still grow
// by, covers that (+ the runtime's reserve); until a first call has ended nobody knows and a generous guess stands in.  On references
// whose chunks need tens of GB per context (half the genome in repeats) this is what keeps eight callers from filling the HBM
// together and then all waiting for each other.
static size_t g_footprint = 0;              // (under g_ctx_mu)
static bool room_for_another_call(const CallCtx *cand, int n_busy, int n_reads)
{
	if (n_busy == 0) return true;
	// (before any call has ended: 64 KB per read of the chunk — what a chunk needs when half the reference is high-copy repeats, ten
	// times what an ordinary one does: the first calls of a run start side by side as far as that fits, five on a 288-GB device)
	const size_t foot = g_footprint ? g_footprint : (size_t)std::max(n_reads, 1) * 65536;
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return true; }
	// (a context that has been through a call holds what a chunk needs, give or take; only the fresh ones still have their growth
	// to come.  Counting the difference to the LARGEST context against every one of them kept callers at the door for seconds on a
	// device whose contexts were all in place: eight of them, each a little smaller than the largest, "owed" more than was free)
	size_t promised = 0;
	for (int i = 0; i < MAX_CALLS; ++i)
		if (g_ctx[i].busy && g_ctx[i].calls_done == 0 && g_ctx[i].device_bytes() < foot) promised += foot - g_ctx[i].device_bytes();
	const size_t have = cand->device_bytes(), need = (cand->calls_done == 0 && have < foot ? foot - have + ((size_t)8 << 30) : (size_t)1 << 30);
	return fr >= promised + need;
}
// what the caller has said about itself (mi355x_prewarm's n_calls): with three or more calls kept in flight, the first calls of its
// loop run in the busy mode too — they used to start as lone callers (two sub-batches, each waiting for its turns among the
// others' kernels) and took 2-3 s instead of 0.6
static std::atomic<int> g_expected_calls(0);
void expect_calls_in_flight(int n) { g_expected_calls.store(n, std::memory_order_relaxed); }
static int g_waiting_for_memory = 0;        // calls stuck in device_memory_pressure (under g_ctx_mu)
static std::condition_variable g_mem_cv;    // a call has ended
struct CtxLease {
	CallCtx *c = nullptr;
	int others = 0;   // calls that were in flight when this one started
	// ... or in the last two seconds: a caller that keeps several calls in flight is treated as such from its third call on, also
	// when several of its calls happen to end together
	bool crowded = false;
	CtxLease(const bseq1_t *seqs, int n)
	{
		const double t_door = now_ms();
		std::unique_lock<std::mutex> lk(g_ctx_mu);
		for (;;) {
			int n_busy = 0;
			for (int i = 0; i < MAX_CALLS; ++i) n_busy += g_ctx[i].busy ? 1 : 0;
			if (n_busy < g_admit) {
				// a context that already holds buffers first (an idle one with buffers next to a busy fresh one would be HBM nobody uses)
				CallCtx *cand = nullptr;
				for (int pass = 0; pass < 2 && !cand; ++pass)
					for (int i = 0; i < MAX_CALLS && !cand; ++i)
						if (!g_ctx[i].busy && (pass == 1 || g_ctx[i].device_bytes() > 0)) cand = &g_ctx[i];
				if (cand && room_for_another_call(cand, n_busy, n)) { c = cand; c->busy = true; }
			}
			if (c) break;
			g_ctx_cv.wait_for(lk, std::chrono::milliseconds(20));   // (a call that ends wakes the waiters; so does memory given back without one ending)
		}
		for (int i = 0; i < MAX_CALLS; ++i) {
			if (!g_ctx[i].busy || &g_ctx[i] == c) continue;
			++others;
			// calls in flight must not share reads: each writes the seq[] and sam of its own
			if (seqs < g_ctx[i].seq_hi && g_ctx[i].seq_lo < seqs + n)
				die("mem_process_seqs: called on seqs[] that another call in flight is still working on");
		}
		c->seq_lo = seqs; c->seq_hi = seqs + n;
		const double now = now_ms();
		static const bool door_log = getenv("MPIBWA_DOOR_LOG") != nullptr;   // calls that waited to be let in (admission by HBM head room)
		if (door_log && now - t_door > 50.) fprintf(stderr, "[door] a call of %d reads waited %.0f ms to be admitted next to %d others\n", n, now - t_door, others);
		if (others >= 2) last_crowded_ms() = now;
		crowded = now - last_crowded_ms() < 2000.0 || g_expected_calls.load(std::memory_order_relaxed) >= 3;
	}
	static double &last_crowded_ms() { static double t = -1e30; return t; }   // (under g_ctx_mu)
	~CtxLease()
	{
		{
			std::lock_guard<std::mutex> lk(g_ctx_mu);
			// (also when a call ENDS among two others: a caller whose calls take longer than the two seconds — first use of its contexts,
			// a hard reference — would otherwise start its next round as a lone caller)
			int n_busy = 0;
			for (int i = 0; i < MAX_CALLS; ++i) n_busy += g_ctx[i].busy ? 1 : 0;
			if (n_busy >= 3) last_crowded_ms() = now_ms();
			if (c->device_bytes() > g_footprint) g_footprint = c->device_bytes();
			++c->calls_done;
			c->busy = false; c->seq_lo = c->seq_hi = nullptr;
		}
		g_ctx_cv.notify_all();
		g_mem_cv.notify_all();
	}
};
// give back the device buffers of every context that is not inside a call; returns the bytes freed
static size_t release_idle_locked(std::unique_lock<std::mutex> &lk)
{
	size_t freed = 0;
	for (int i = 0; i < MAX_CALLS; ++i) {
		CallCtx &x = g_ctx[i];
		if (x.busy || x.device_bytes() == 0) continue;
		x.busy = true;              // nobody leases it while its buffers go
		lk.unlock();
		freed += x.device_bytes();
		x.release_device();
		lk.lock();
		x.busy = false;
	}
	return freed;
}
void release_idle_work_buffers()
{
	std::unique_lock<std::mutex> lk(g_ctx_mu);
	release_idle_locked(lk);
}
bool device_memory_pressure(size_t wanted)
{
	std::unique_lock<std::mutex> lk(g_ctx_mu);
	if (const size_t freed = release_idle_locked(lk)) {
		fprintf(stderr, "[mpibwa_amd] a device work buffer of %.2f GB did not fit: %.2f GB of idle call contexts' buffers given back\n", wanted / 1e9, freed / 1e9);
		return true;
	}
	int n_busy = 0;
	for (int i = 0; i < MAX_CALLS; ++i) n_busy += g_ctx[i].busy ? 1 : 0;
	if (n_busy <= 1) return false;   // a lone call: nothing to wait for
	if (g_admit > n_busy - 1) {
		g_admit = std::max(1, n_busy - 1);
		fprintf(stderr, "[mpibwa_amd] a device work buffer of %.2f GB does not fit with %d calls in flight: %d calls are admitted at once from now on\n",
		        wanted / 1e9, n_busy, g_admit);
	}
	// wait for another call to end (its context then is idle: its buffers are given back above on the next attempt) — unless every
	// call in flight is waiting here, in which case nobody will ever end
	++g_waiting_for_memory;
	bool ok = true;
	for (;;) {
		if (g_waiting_for_memory >= n_busy) { ok = false; break; }
		g_mem_cv.wait_for(lk, std::chrono::milliseconds(50));
		int now_busy = 0;
		for (int i = 0; i < MAX_CALLS; ++i) now_busy += g_ctx[i].busy ? 1 : 0;
		if (now_busy < n_busy) break;
		n_busy = now_busy;
	}
	--g_waiting_for_memory;
	if (!ok) return false;   // every call in flight waits here: nobody will end (the caller of ensure() reports and ends the process)
	release_idle_locked(lk);
	return true;
}
static thread_local mi355x_stats_t t_stats;   // of the last call made by this thread
static thread_local bool t_stats_set = false;
static std::atomic<int> g_in_flight(0);
int calls_in_flight() { return g_in_flight.load(); }

} // namespace mbw

using namespace mbw;

extern "C" void mi355x_last_stats(mi355x_stats_t *st)
{
	if (t_stats_set) { *st = t_stats; return; }
	std::lock_guard<std::mutex> lk(g_ctx_mu);
	*st = g_stats;
}
extern "C" int mi355x_host_cpus(void) { return usable_cpus(); }
// calls the library runs side by side at most (further callers wait at the door; fewer are admitted when their work buffers do not fit)
extern "C" int mi355x_max_calls(void) { return MAX_CALLS; }
// host threads the library will use for this rank's calls: its share of the node's usable CPUs (the launcher's local size), and
// how many ranks it believes share the node
extern "C" int mi355x_rank_host_threads(int *ranks_on_node)
{
	int ranks = env_local_size();
	if (ranks < 1) ranks = 1;
	if (ranks_on_node) *ranks_on_node = ranks;
	return host_threads(nullptr);
}

// Caller-side helpers mirroring mpiBWA's copy_buffer_thr (src/mainParallel.c:103-127): concatenate all seqs[i].sam into one buffer
// and free the per-read strings.  off[i]: where record i goes (n + 1 entries); returns the total length
static size_t sam_offsets(const bseq1_t *seqs, int n, int n_thr, std::vector<size_t> &off)
{
	off.resize(n + 1);
	parallel_for(n_thr, n, 8192, [&](int i) { off[i + 1] = seqs[i].sam ? strlen(seqs[i].sam) : 0; });
	off[0] = 0;
	for (int i = 0; i < n; ++i) off[i + 1] += off[i];
	return off[n];
}
static void sam_gather(bseq1_t *seqs, int n, int n_thr, const std::vector<size_t> &off, char *b)
{
	parallel_for(n_thr, n, 8192, [&](int i) {
		if (!seqs[i].sam) return;
		memcpy(b + off[i], seqs[i].sam, off[i + 1] - off[i]);
		free(seqs[i].sam);
		seqs[i].sam = 0;
	});
	b[off[n]] = 0;
}
// into a buffer the caller keeps from chunk to chunk (*buf, *cap: grown with realloc when a chunk needs more)
extern "C" size_t mi355x_collect_sam_into(bseq1_t *seqs, int n, char **buf, size_t *cap)
{
	std::vector<size_t> off;
	const int n_thr = std::min(usable_cpus(), 32);
	const size_t tot = sam_offsets(seqs, n, n_thr, off);
	if (tot + 1 > *cap) {
		free(*buf);
		*cap = tot + tot / 8 + 4096;
		*buf = (char *)malloc(*cap);
		if (!*buf) die("out of memory collecting SAM");
	}
	sam_gather(seqs, n, n_thr, off, *buf);
	return tot;
}
// into one malloc'ed buffer
extern "C" char *mi355x_collect_sam(bseq1_t *seqs, int n, size_t *total_len)
{
	std::vector<size_t> off;
	const int n_thr = std::min(usable_cpus(), 32);
	const size_t tot = sam_offsets(seqs, n, n_thr, off);
	char *buf = (char *)malloc(tot + 1);
	if (!buf) die("out of memory collecting SAM");
	sam_gather(seqs, n, n_thr, off, buf);
	if (total_len) *total_len = tot;
	return buf;
}

// The index must be resident, and the one the caller passes (under g_init_mu)
static void require_resident_index(DevIndex &ix, const bwt_t *bwt, const bntseq_t *bns, const uint8_t *pac)
{
	if (!ix.ready) {
		// first call and nobody called mi355x_init / mi355x_index_upload: make the index resident (one rank per GPU, the GPU
		// named by the launcher's local rank).  Several ranks on the node and no local rank known = every rank would pile
		// its 60 GB onto GPU 0: refuse.
		int lr = env_local_rank();
		if (lr < 0) {
			if (env_local_size() > 1) die("mem_process_seqs: %d ranks share this node but the launcher exports no local rank: call mi355x_init(local_rank, ...) first", env_local_size());
			lr = 0;
		}
		mi355x_index_upload(lr, bwt, bns, pac);
	}
	// the resident index must be the one the caller passes: contig table, pac fetches and coordinates of the host stages
	// come from the caller's copy, seeds and extensions from the device's
	const char *what = nullptr;
	if (!index_matches(bwt, bns, &what))
		die("mem_process_seqs: the index passed in is not the one resident on the GPU (%s differs): mi355x_finalize() and upload it first", what);
}

// MPIBWA_SAMPLE: the sampler thread, started by the first call
static void start_sampler_once()
{
	static std::once_flag sampler_once;
	std::call_once(sampler_once, [] {
		if (!getenv("MPIBWA_SAMPLE")) return;
		g_sampler = new StageSampler;
		g_sampler->min_calls = std::max(1, atoi(getenv("MPIBWA_SAMPLE")));
		g_sampler->th = std::thread([] { g_sampler->run(); });
		atexit(sampler_report);
	});
}

// the streams of a call context, created at its first call: p_streams for the lanes of phase 1, a_streams / d_streams for the jobs
// of the SAM stage (the host's units and the units decided on the device), per part
static void create_streams(CallCtx &C)
{
	// the SAM stage's kernels (mate rescue, CIGAR) are short and the host waits for them with all its threads: they go
	// ahead of the seeding / extension kernels of the other calls in flight (MPIBWA_PRIO=n: no priorities, p: reversed)
	int lo_p = 0, hi_p = 0;   // numerically lowest = highest priority
	HIP_OK(hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));
	const char *prio = getenv("MPIBWA_PRIO");
	const int pp = prio && *prio == 'p' ? hi_p : 0, pa = !prio || *prio == 'a' ? hi_p : 0;
	// The runtime spreads the streams of one priority over its few hardware queues in the order they are created: without the
	// rotation from call to call the first stream of every call shares ONE hardware queue, and that queue — 50 ms of phase-1
	// kernels and copies per chunk, strictly one after the other — is the bottleneck of eight calls in flight.  Rotated, the
	// kernels of different calls overlap: 13.0-13.7 vs 12.3-12.7 Mreads/s in alternating runs (the seeding launches stretch
	// from 15-18 to 17-21 ms in that company).  MPIBWA_STREAM_ROT=0: no rotation.
	hipStream_t ps[MAX_LANES], hs[4];
	for (int l = 0; l < MAX_LANES; ++l) HIP_OK(hipStreamCreateWithPriority(&ps[l], hipStreamNonBlocking, pp));
	for (int l = 0; l < 4; ++l) HIP_OK(hipStreamCreateWithPriority(&hs[l], hipStreamNonBlocking, pa));
	const char *re = getenv("MPIBWA_STREAM_ROT");
	const int rot = re && atoi(re) == 0 ? 0 : (int)(&C - g_ctx);
	for (int l = 0; l < MAX_LANES; ++l) C.p_streams[l] = ps[(l + rot) % MAX_LANES];
	for (int l = 0; l < 2; ++l) { C.a_streams[l] = hs[(l + rot) % 4]; C.d_streams[l] = hs[(2 + l + rot) % 4]; }
}

extern "C" void mem_process_seqs(const mem_opt_t *opt, const bwt_t *bwt, const bntseq_t *bns, const uint8_t *pac,
                                 int64_t n_processed, int n, bseq1_t *seqs, const mem_pestat_t *pes0)
{
	const double t_begin = now_ms(), c_begin = cpu_sec(), s_begin = sys_sec();
	DevIndex &ix = dev_index();
	std::unique_lock<std::recursive_mutex> init_lk(g_init_mu);
	require_resident_index(ix, bwt, bns, pac);
	struct InFlight { InFlight() { ++g_in_flight; } ~InFlight() { --g_in_flight; } } in_flight;
	init_lk.unlock();
	HIP_OK(hipSetDevice(ix.device));
	mi355x_stats_t STAT;
	memset(&STAT, 0, sizeof STAT);
	struct Publish {   // the statistics of this call become visible when it returns, whichever way
		mi355x_stats_t &s;
		~Publish() { t_stats = s; t_stats_set = true; std::lock_guard<std::mutex> lk(g_ctx_mu); g_stats = s; }
	} publish{STAT};
	if (n <= 0) return;
	CtxLease lease(seqs, n);
	CallCtx &C = *lease.c;
	start_sampler_once();
	struct StageOwner {
		StageOwner(int slot) { t_stage = &g_stage[slot]; stage(1); }
		~StageOwner() { t_stage->store(0); t_stage = nullptr; }
	} stage_owner((int)(&C - g_ctx));
	if (!C.a_streams[0]) create_streams(C);
	Call call(opt, bns, pac, n_processed, n, seqs, pes0, ix, C, STAT, lease.crowded);

	// ---- 1. encode + pack ----
	call.pack();
	call.start_sam_inputs();

	// ---- 2-6. seeding -> SA -> chaining -> extension -> region clean-up, in sub-batches ----
	call.phase1_all();

	// ---- 7. insert-size statistics over the whole batch ----
	stage(7);
	if (call.pe) {
		if (pes0) memcpy(call.pes, pes0, 4 * sizeof(mem_pestat_t));
		else if (call.pes_hist) pestat_from_hist(opt, call.pes_hist, call.pes);
		else pestat(opt, bns->l_pac, n, call.regs.data(), call.pes, call.n_thr);
	}
	const double t7 = now_ms();

	// ---- 8. pairing decisions, then CIGAR/MD/NM on the GPU, then SAM text ----
	stage(8);
	stage(25);
	call.sam_inputs.join();
	if (call.dev_pair && call.gpu_sam && call.gpu_aln) call.decide_on_device(2);
	if (call.dev_se) call.decide_on_device(1);
	call.sam_stage();
	const double t8 = now_ms();
	stage(19);
	hprof_report("sam stage");

	// ---- statistics ----
	static const bool s_cpusec = getenv("MPIBWA_CPUSEC") != nullptr;
	if (s_cpusec) fprintf(stderr, "[plan Mcycles] sam_pe_plan %.0f  emit(collect) %.0f  device-record copy %.0f (%llu records)\n", call.tsc_plan.load() * 1e-6, call.tsc_emitc.load() * 1e-6, call.tsc_devcopy.load() * 1e-6, call.n_sam_dev.load());
	if (g_hprof_on || s_cpusec)
		fprintf(stderr, "[cpu-sec] encode+h2d %.3f  phase1 %.3f  pestat+sam %.3f (msw-collect %.3f, plan+collect %.3f, emit %.3f [sys %.3f, %ld page faults])  total %.3f  sys %.3f  wall %.3f\n",
		        call.c_packed - c_begin, call.c_phase1 - call.c_packed, cpu_sec() - call.c_phase1, call.cpu_msw, call.cpu_collect, call.cpu_emit, call.sys_emit, call.pf_emit,
		        cpu_sec() - c_begin, sys_sec() - s_begin, (t8 - t_begin) * 1e-3);
	// release the per-read containers in parallel (millions of small blocks: serial destruction costs ~0.2 s per chunk)
	parallel_for(call.n_thr, n, 8192, [&](int i) { HRegV().swap(call.regs[i]); });   // only reads that outgrew their arena slice own memory
	STAT.n_reads = n;
	STAT.h2d_ms = call.t_packed - t_begin;
	STAT.pestat_ms = t7 - call.t_phase1; STAT.sam_ms = t8 - t7; STAT.total_ms = now_ms() - t_begin;
	if (bwa_verbose >= 3)
		fprintf(stderr, "[M::%s] Processed %d reads in %.3f CPU sec, %.3f real sec\n", "mem_process_seqs", n, cpu_sec() - c_begin,
		        (t8 - t_begin) * 1e-3);
}
