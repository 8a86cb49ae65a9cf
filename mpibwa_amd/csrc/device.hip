// device.hip — the grow-only work buffers, index residency in HBM, and the parameter and table builders the pipeline and the stage
// entries (stage_entries.hip) share.
#include <atomic>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hip_util.h"
#include "device.h"
#include "host.h"
#include <cmath>

namespace mbw {

static DevIndex g_idx;
DevIndex &dev_index() { return g_idx; }
static std::atomic<unsigned long long> g_buf_growths(0);
void note_buffer_growth(size_t from, size_t to, const char *kind)
{
	++g_buf_growths;
	static const bool log = getenv("MPIBWA_GROWTH_LOG") != nullptr;
	if (log) fprintf(stderr, "[growth] %s buffer %zu -> %zu bytes (reallocation %llu)\n", kind, from, to, g_buf_growths.load());
}
// (re)allocations of device and page-locked work buffers so far: hipFree / hipMalloc / hipHostMalloc stall every stream of the
// device, so a caller that sees this number move in steady state knows where a slow chunk came from
extern "C" unsigned long long mi355x_buffer_growths(void) { return g_buf_growths.load(); }
std::vector<DevBuf *> *g_devbuf_owner = nullptr;
void *DevBuf::ensure(size_t bytes)
{
	if (bytes > cap) {
		size_t want = bytes + bytes / 4 + 256;
		note_buffer_growth(cap, want, "device");
		if (p) HIP_OK(hipFree(p));
		p = nullptr; cap = 0;
		// (what the runtime itself needs later — kernel scratch, queues, events — comes out of the same HBM, and it aborts the process
		// when it finds none: an allocation that leaves less than a reserve free counts as one that did not fit)
		static const size_t reserve = (size_t)(getenv("MPIBWA_HBM_RESERVE_GB") ? atof(getenv("MPIBWA_HBM_RESERVE_GB")) : 6.0) << 30;
		for (int attempt = 0;; ++attempt) {
			if (hipMalloc(&p, want) == hipSuccess) {
				size_t fr = 0, tot = 0;
				if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr >= reserve) break;
				(void)hipFree(p);
			}
			(void)hipGetLastError();
			p = nullptr;
			if (attempt == 0 && want > bytes + 256) { want = bytes + 256; continue; }   // without the head room first
			if (device_memory_pressure(want)) continue;
			size_t fr = 0, tot = 0;
			(void)hipMemGetInfo(&fr, &tot);
			die("device work buffer of %.2f GB does not fit: %.1f of %.1f GB free (index, dense SA and the work buffers of this call share the HBM; no other "
			    "call is in flight and no idle buffer is left to give back)", want / 1e9, fr / 1e9, tot / 1e9);
		}
		cap = want;
	}
	return p;
}
void DevBuf::release()
{
	if (p) (void)hipFree(p);
	p = nullptr; cap = 0;
}
void *PinBuf::ensure(size_t bytes)
{
	if (bytes > cap) {
		note_buffer_growth(cap, bytes + bytes / 4 + 4096, "page-locked");
		if (p) HIP_OK(hipHostFree(p));
		cap = bytes + bytes / 4 + 4096;
		HIP_OK(hipHostMalloc(&p, cap, hipHostMallocDefault));
	}
	return p;
}
void PinBuf::release()
{
	if (p) HIP_OK(hipHostFree(p));
	p = nullptr; cap = 0;
}

// the device of a rank, after the checks: a usable gfx950 (this thread is then on it)
static int checked_device(int local_rank)
{
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n == 0)
		die("no HIP device visible: the alignment hot path runs on MI355X only, there is no CPU fallback");
	HIP_OK(hipSetDevice(local_rank % n));
	hipDeviceProp_t prop;
	HIP_OK(hipGetDeviceProperties(&prop, local_rank % n));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		die("device %d is %s; this library carries gfx950 (MI355X) code objects only", local_rank % n, prop.gcnArchName);
	return local_rank % n;
}
static void require_device(int local_rank) { g_idx.device = checked_device(local_rank); }

void use_device()
{
	static std::atomic<int> checked(-1);   // device 0 after the checks, for calls before any index (or after mi355x_finalize)
	int d = g_idx.device;
	if (d < 0 && (d = checked.load()) < 0) {
		static std::mutex mu;
		std::lock_guard<std::mutex> lk(mu);
		if (checked.load() < 0) checked = checked_device(0);
		d = checked.load();
	}
	HIP_OK(hipSetDevice(d));
}

static uint64_t index_hash(const bwt_t *bwt, const bntseq_t *bns)
{
	uint64_t h = 1469598103934665603ull;   // FNV-1a
	auto mix = [&](const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
	for (int i = 0; i < bns->n_seqs; ++i) {
		mix(&bns->anns[i].offset, sizeof bns->anns[i].offset);
		mix(&bns->anns[i].len, sizeof bns->anns[i].len);
		if (bns->anns[i].name) mix(bns->anns[i].name, strlen(bns->anns[i].name));
	}
	if (bwt->bwt && bwt->bwt_size >= 16) mix(bwt->bwt, 64);
	return h;
}

// (called under index_mutex() on every mem_process_seqs call: the contig table — 10^5..10^6 names on some references — is only
// hashed again when the caller passes other pointers than the ones that matched last time)
static const void *g_last_ok[4] = {nullptr, nullptr, nullptr, nullptr};
static int g_last_ok_nseqs = -1;
bool index_matches(const bwt_t *bwt, const bntseq_t *bns, const char **what)
{
	const char *w = nullptr;
	const bool same_ptrs = g_last_ok[0] == bwt && g_last_ok[1] == bns && g_last_ok[2] == bns->anns && g_last_ok[3] == bwt->bwt && g_last_ok_nseqs == bns->n_seqs;
	if (bwt->seq_len != g_idx.id_seq_len) w = "seq_len";
	else if (bwt->primary != g_idx.id_primary) w = "primary";
	else if (memcmp(bwt->L2, g_idx.id_L2, sizeof g_idx.id_L2) != 0) w = "L2";
	else if (bns->l_pac != g_idx.l_pac) w = "l_pac";
	else if (bns->n_seqs != g_idx.id_n_seqs) w = "n_seqs";
	else if (!same_ptrs && index_hash(bwt, bns) != g_idx.id_hash) w = "contig table or BWT";
	if (!w) { g_last_ok[0] = bwt; g_last_ok[1] = bns; g_last_ok[2] = bns->anns; g_last_ok[3] = bwt->bwt; g_last_ok_nseqs = bns->n_seqs; }
	else g_last_ok[0] = nullptr;
	if (what) *what = w;
	return w == nullptr;
}

static void no_calls_in_flight(const char *who)
{
	if (calls_in_flight() > 0) die("%s while mem_process_seqs calls are in flight on the resident index", who);
}

// the tables derived from the index on the device (occ32, k-mer tables, jump table, dense SA): freed, and FmDev forgets them
static void free_derived_tables()
{
	for (void **t : {&g_idx.d_occ32, &g_idx.d_kmt, &g_idx.d_p3tab, &g_idx.d_sa_full}) {
		if (*t) (void)hipFree(*t);
		*t = nullptr;
	}
	g_idx.kmt_bytes = 0; g_idx.sa_full_bytes = 0;
	FmDev &fm = g_idx.fm;
	fm.occ32 = nullptr; fm.occ_sb = nullptr; fm.kmt = nullptr; fm.kmt_k = 0; fm.p3tab = nullptr; fm.p3_k = 0; fm.sa_full = nullptr;
}

static void alloc_index(const bwt_t *bwt, const bntseq_t *bns)
{
	std::lock_guard<std::recursive_mutex> lk(index_mutex());   // no call can pass its residency check while the buffers are replaced
	no_calls_in_flight("index upload");
	g_idx.ready = false;
	if (g_idx.d_blk) { (void)hipFree(g_idx.d_blk); (void)hipFree(g_idx.d_sa); (void)hipFree(g_idx.d_pac); }
	g_idx.blk_bytes = ((size_t)bwt->bwt_size * 4 + 63) / 64 * 64 + 64;   // whole 64-B blocks + one pad block
	g_idx.sa_bytes = (size_t)bwt->n_sa * 8;
	g_idx.pac_bytes = (size_t)bns->l_pac / 4 + 1 + 16;
	HIP_OK(hipMalloc(&g_idx.d_blk, g_idx.blk_bytes));
	HIP_OK(hipMalloc(&g_idx.d_sa, g_idx.sa_bytes));
	HIP_OK(hipMalloc(&g_idx.d_pac, g_idx.pac_bytes));
	HIP_OK(hipMemset(g_idx.d_blk, 0, g_idx.blk_bytes));
	HIP_OK(hipMemset(g_idx.d_pac, 0, g_idx.pac_bytes));
	FmDev &fm = g_idx.fm;
	fm.blk = g_idx.d_blk; fm.sa = (const uint64_t *)g_idx.d_sa;
	free_derived_tables();
	fm.primary = bwt->primary; fm.seq_len = bwt->seq_len;
	for (int i = 0; i < 5; ++i) fm.L2[i] = bwt->L2[i];
	int sh = 0;
	while ((1 << sh) < bwt->sa_intv) ++sh;
	if ((1 << sh) != bwt->sa_intv) die("SA sampling interval %d is not a power of two", bwt->sa_intv);
	fm.sa_shift = sh;
	g_idx.l_pac = bns->l_pac;
	g_idx.id_primary = bwt->primary; g_idx.id_seq_len = bwt->seq_len; g_idx.id_n_seqs = bns->n_seqs;
	g_idx.id_hash = index_hash(bwt, bns);
	g_last_ok[0] = nullptr;   // a new resident index: the next call hashes its contig table again
	memcpy(g_idx.id_L2, bwt->L2, sizeof g_idx.id_L2);
	if (bwt->seq_len >= (1ull << 34))
		die("reference of %llu symbols: this build packs SA-interval bounds into 34 bits (references up to 8.5 Gbp)", (unsigned long long)bwt->seq_len);
	// the buffers are handed to collectives on other streams next (RCCL, torch): the memsets above must have landed
	HIP_OK(hipDeviceSynchronize());
}

// Jump table of the third seeding pass (fm_kernels.hip): 4^13 entries x 32 B = 2.1 GB, built in a few tens of ms.
// MPIBWA_P3TAB=0 disables it, MPIBWA_P3TAB=<k> chooses the number of extensions folded into it (default 12).
static void maybe_build_p3()
{
	int k = 12;
	if (const char *e = getenv("MPIBWA_P3TAB")) k = atoi(e);
	if (k < 4 || k > 14) return;
	const size_t bytes = ((size_t)1 << (2 * (k + 1))) * 32;
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + ((size_t)16 << 30)) return;
	HIP_OK(hipMalloc(&g_idx.d_p3tab, bytes));
	launch_p3_build(0, g_idx.fm, k, g_idx.d_p3tab);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	g_idx.fm.p3tab = g_idx.d_p3tab;
	g_idx.fm.p3_k = k;
}

// The seeding kernel's k-mer tables (fm_kernels.hip: kmt_build_kernel): the bi-interval of every string of up to K bases, K chosen
// so that the longest table has about as many entries as the index has rows (beyond that a table entry is as cold as an occ block)
// and at most 14 (5.7 GB).  MPIBWA_KMT=<K> chooses K (0 = no tables: every extension through the occ table).
static void maybe_build_kmt()
{
	int k = 1;
	while (k < 14 && ((uint64_t)1 << (2 * k)) < g_idx.fm.seq_len) ++k;
	if (const char *e = getenv("MPIBWA_KMT")) k = atoi(e);
	if (k < 1) return;
	if (k > 15) k = 15;
	const size_t bytes = kmt_bytes(k);
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + ((size_t)16 << 30)) return;
	HIP_OK(hipMalloc(&g_idx.d_kmt, bytes));
	launch_kmt_build(0, g_idx.fm, k, g_idx.d_kmt);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
	g_idx.kmt_bytes = bytes;
	g_idx.fm.kmt = g_idx.d_kmt;
	g_idx.fm.kmt_k = k;
}

// The seeding kernel's own occ table (fm_kernels.hip: occ32_build_kernel), derived on the device from the bwa-format blocks.
static void build_occ32()
{
	g_idx.occ32_bytes = occ32_bytes(g_idx.fm.seq_len);
	HIP_OK(hipMalloc(&g_idx.d_occ32, g_idx.occ32_bytes));
	launch_occ32_build(0, g_idx.fm, g_idx.d_occ32);
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipGetLastError());
}

// Expand the sampled SA into a dense one when HBM allows it (MPIBWA_SA_DENSE=0 disables it).
static void maybe_expand_sa()
{
	const char *e = getenv("MPIBWA_SA_DENSE");
	if (e && atoi(e) == 0) return;
	size_t need = (size_t)(g_idx.fm.seq_len + 1) * 8, free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + (need >> 1) + ((size_t)8 << 30)) return;   // keep room for the batches
	HIP_OK(hipMalloc(&g_idx.d_sa_full, need));
	unsigned long long *d_cnt;
	HIP_OK(hipMalloc(&d_cnt, 64));
	HIP_OK(hipMemset(d_cnt, 0, 64));
	hipEvent_t a, b;
	HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b));
	HIP_OK(hipEventRecord(a, 0));
	launch_sa_expand(0, g_idx.fm, (uint64_t *)g_idx.d_sa_full, d_cnt);
	HIP_OK(hipEventRecord(b, 0));
	HIP_OK(hipEventSynchronize(b));
	HIP_OK(hipGetLastError());
	float ms = 0;
	HIP_OK(hipEventElapsedTime(&ms, a, b));
	g_idx.sa_expand_ms = ms;
	g_idx.sa_full_bytes = need;
	g_idx.fm.sa_full = (const uint64_t *)g_idx.d_sa_full;
	(void)hipFree(d_cnt); (void)hipEventDestroy(a); (void)hipEventDestroy(b);
}

SmemParams smem_params(const mem_opt_t *opt)
{
	SmemParams sp;
	sp.min_seed_len = opt->min_seed_len;
	sp.split_len = (int)(opt->min_seed_len * opt->split_factor + .499);   // src/bwamem.c:118
	sp.split_width = opt->split_width;
	if (opt->split_width < 0 || opt->split_width >= 65535) die("split_width %d: the seeding kernel packs re-seed requests into 16 bits", opt->split_width);
	sp.max_mem_intv = (int)opt->max_mem_intv;
	return sp;
}

void c2a_length_tables(const mem_opt_t *opt, int max_len, std::vector<int> &tab)
{
	const int TS = max_len + 2;
	tab.assign(6 * (size_t)TS, 0);
	for (int l = 0; l < TS; ++l) {
		tab[l] = cal_max_gap(opt, l);
		tab[TS + l] = clamp_band(opt, l, 1 << 28, opt->pen_clip5);
		tab[2 * TS + l] = clamp_band(opt, l, 1 << 28, opt->pen_clip3);
		tab[3 * TS + l] = (int)ceil(l * .95);
		tab[4 * TS + l] = (int)floor(.1 * l);
		// mem_flt_chained_seeds returns at once for this length (src/bwamem.c:600-602)
		const double min_l = opt->min_chain_weight ? 1.1f * opt->min_chain_weight : 5.5f * log(l > 0 ? l : 1);
		tab[5 * TS + l] = (l > 0 && min_l > 0.05f * l) ? 1 : 0;
	}
}

void c2a_launch_order(int n, const int *nseeds, int *order)
{
	const int NB = 1024;
	std::vector<int> start(NB + 1, 0);
	for (int i = 0; i < n; ++i) ++start[NB - 1 - std::min(nseeds[i], NB - 1) + 1];
	for (int b = 0; b < NB; ++b) start[b + 1] += start[b];
	for (int i = 0; i < n; ++i) order[start[NB - 1 - std::min(nseeds[i], NB - 1)]++] = i;
}

ExtParams ext_params(const mem_opt_t *opt)
{
	ExtParams ep;
	memcpy(ep.mat, opt->mat, 25);
	ep.o_del = opt->o_del; ep.e_del = opt->e_del; ep.o_ins = opt->o_ins; ep.e_ins = opt->e_ins; ep.zdrop = opt->zdrop;
	return ep;
}

void c2a_params(const mem_opt_t *opt, int64_t l_pac, int early, C2aParams &cp, ExtParams &ep)
{
	cp.l_pac = l_pac; cp.a = opt->a; cp.w = opt->w; cp.pen_clip5 = opt->pen_clip5; cp.pen_clip3 = opt->pen_clip3;
	cp.early = early;
	ep = ext_params(opt);
}

ChainParams chain_params(const mem_opt_t *opt, int64_t l_pac)
{
	ChainParams kp;
	kp.l_pac = l_pac; kp.w = opt->w; kp.max_chain_gap = opt->max_chain_gap; kp.min_chain_weight = opt->min_chain_weight;
	kp.min_seed_len = opt->min_seed_len; kp.max_chain_extend = opt->max_chain_extend; kp.mask_level = opt->mask_level; kp.drop_ratio = opt->drop_ratio;
	return kp;
}

void contig_table(const bntseq_t *bns, std::vector<int64_t> &ann_off, std::vector<uint8_t> &ann_alt)
{
	ann_off.assign(bns->n_seqs + 1, bns->l_pac);
	ann_alt.assign(bns->n_seqs + 1, 0);
	for (int k = 0; k < bns->n_seqs; ++k) { ann_off[k] = bns->anns[k].offset; ann_alt[k] = bns->anns[k].is_alt ? 1 : 0; }
}

void aln_params(const mem_opt_t *opt, int64_t l_pac, AlnParams &ap, ExtParams &ep)
{
	ap.l_pac = l_pac; ap.a = opt->a; ap.w = opt->w;
	ep = ext_params(opt);
}

void cigar_gap_table(const mem_opt_t *opt, int max_len, std::vector<int> &tab)
{
	tab.resize(max_len + 2);
	for (int l = 0; l <= max_len + 1; ++l) {
		int max_ins = (int)((double)(((l + 1) >> 1) * opt->mat[0] - opt->o_ins) / opt->e_ins + 1.);
		int max_del = (int)((double)(((l + 1) >> 1) * opt->mat[0] - opt->o_del) / opt->e_del + 1.);
		int g = max_ins > max_del ? max_ins : max_del;
		tab[l] = g > 1 ? g : 1;
	}
}

SamParams sam_params(int64_t l_pac, bool has_qual)
{
	SamParams sp;
	sp.l_pac = l_pac; sp.has_qual = has_qual ? 1 : 0;
	sp.rg_len = (int)strnlen(bwa_rg_id, sizeof bwa_rg_id);
	memset(sp.rg, 0, sizeof sp.rg);
	memcpy(sp.rg, bwa_rg_id, (size_t)sp.rg_len);
	return sp;
}

void contig_names(const bntseq_t *bns, std::vector<char> &names, std::vector<int> &name_off)
{
	name_off.assign(bns->n_seqs + 1, 0);
	for (int k = 0; k < bns->n_seqs; ++k) name_off[k + 1] = name_off[k] + (int)strlen(bns->anns[k].name);
	names.resize((size_t)name_off[bns->n_seqs] + 1);
	for (int k = 0; k < bns->n_seqs; ++k) memcpy(names.data() + name_off[k], bns->anns[k].name, (size_t)(name_off[k + 1] - name_off[k]));
}

void queue_aln_sam(void *stream, const mem_opt_t *opt, int64_t l_pac, const ChunkDev &D, const SamParams &sp, const AlnSamJob &J, void *ev_a, void *ev_b)
{
	hipStream_t st = (hipStream_t)stream;
	HIP_OK(hipMemsetAsync(J.d_cnt, 0, 256, st));
	AlnParams ap;
	ExtParams ep;
	aln_params(opt, l_pac, ap, ep);
	if (ev_a) HIP_OK(hipEventRecord((hipEvent_t)ev_a, st));
	if (J.n_req) launch_aln(st, ap, ep, J.n_req, J.d_req, D.d_seq, D.d_off, D.d_pac, D.d_gap, J.d_hdr, J.d_pool, J.d_cnt, J.pool_bytes, D.max_len, D.max_len + 256, J.d_lists);
	if (ev_b) HIP_OK(hipEventRecord((hipEvent_t)ev_b, st));
	if (!J.n_reads) return;
	const int r0 = J.r0, nr = J.n_reads, nu = nr / J.ends;
	if (J.h_desc) HIP_OK(hipMemcpyAsync(J.d_desc + r0, J.h_desc + r0, (size_t)nr * sizeof(SamDesc), hipMemcpyHostToDevice, st));
	HIP_OK(hipMemcpyAsync(J.d_base, J.h_base, (size_t)(nu + 1) * 4, hipMemcpyHostToDevice, st));
	HIP_OK(hipMemsetAsync(J.d_used, 0, 64, st));
	(J.ends == 2 ? launch_sam_emit : launch_sam_emit_se)(st, sp, nr, J.d_desc + r0, J.d_base, J.d_req, J.d_hdr, J.d_pool, D.d_seq, D.d_off + r0, D.d_len + r0, D.d_qual, D.d_names,
	                                                   D.d_noff + r0, D.d_ann_off, D.d_ann_names, D.d_ann_noff, J.d_arena, J.arena_bytes, J.d_used, J.d_ooff, J.d_olen,
	                                                   J.grid_blocks);
	if (J.n_multi > 0)
		launch_sam_lines(st, sp, (opt->flag & MEM_F_SOFTCLIP) != 0, J.n_multi, J.d_mlist, r0, J.d_mlines, J.d_mdesc, J.d_mbase, J.d_req, J.d_hdr, J.d_pool, D.d_seq, D.d_off + r0,
		                 D.d_len + r0, D.d_qual, D.d_names, D.d_noff + r0, D.d_ann_off, D.d_ann_names, D.d_ann_noff, J.d_arena, J.arena_bytes, J.d_used, J.d_ooff,
		                 J.d_olen, J.grid_blocks, J.ends == 2);
}

void queue_c2a(void *stream, const mem_opt_t *opt, int64_t l_pac, int early, const C2aJob &J, void *ev_a, void *ev_b)
{
	hipStream_t st = (hipStream_t)stream;
	C2aParams cp;
	ExtParams ep;
	c2a_params(opt, l_pac, early, cp, ep);
	const C2aUnits *units = J.units.max_units > 0 ? &J.units : nullptr;
	if (ev_a) HIP_OK(hipEventRecord((hipEvent_t)ev_a, st));
	// one wavefront per read (any read length)
	launch_c2a(st, cp, ep, J.n_reads, J.d_seq, J.d_off, J.d_len, J.d_chain_beg, J.d_chain_cnt, J.d_chains, J.d_seeds, J.d_srt, J.d_reg_beg, J.d_regs, J.d_nregs,
	           J.d_tab, J.tab_stride, J.d_pac, J.d_stat, J.max_len, J.d_order, units);
	if (ev_b) HIP_OK(hipEventRecord((hipEvent_t)ev_b, st));
	// the regions sit in sparse per-read slots: prefix sum + pack on the device, queued behind the kernel
	launch_reg_pack(st, J.n_reads, J.d_reg_beg, J.d_nregs, J.d_reg_pos, J.d_regs, J.d_packed, J.d_tmp, J.tmp_bytes, units, J.d_chain_beg, J.d_chain_cnt);
}

// band clamp of src/ksw.c:395-407 (host side, double arithmetic as in the reference)
int clamp_band(const mem_opt_t *opt, int qlen, int w, int end_bonus)
{
	int mx = 0;
	for (int i = 0; i < 25; ++i) mx = std::max(mx, (int)opt->mat[i]);
	int max_ins = (int)((double)(qlen * mx + end_bonus - opt->o_ins) / opt->e_ins + 1.);
	int max_del = (int)((double)(qlen * mx + end_bonus - opt->o_del) / opt->e_del + 1.);
	w = std::min(w, std::max(max_ins, 1));
	w = std::min(w, std::max(max_del, 1));
	return w;
}


bool pair_params(const mem_opt_t *opt, int64_t l_pac, const mem_pestat_t pes[4], int64_t n_processed, int max_len, PairParams &pp, size_t *n_tab_)
{
	memset(&pp, 0, sizeof pp);
	pp.l_pac = l_pac; pp.a = opt->a; pp.b = opt->b; pp.pen_unpaired = opt->pen_unpaired; pp.min_seed_len = opt->min_seed_len; pp.w = opt->w;
	pp.o_del = opt->o_del; pp.e_del = opt->e_del; pp.o_ins = opt->o_ins; pp.e_ins = opt->e_ins;
	pp.max_chain_gap = opt->max_chain_gap; pp.mask_level_redun = opt->mask_level_redun; pp.mask_level = opt->mask_level;
	pp.XA_drop_ratio = opt->XA_drop_ratio; pp.T = opt->T; pp.max_matesw = opt->max_matesw; pp.id0 = (uint64_t)(n_processed >> 1);
	for (int v = 0; v < 64; ++v) pp.lnq[v] = (int)(4.343 * log(v + 1) + .499);
	pp.no_rescue = ((opt->flag & MEM_F_NO_RESCUE) || opt->max_matesw <= 0) ? 1 : 0;
	bool usable = true;
	size_t n_tab = 0;
	for (int d = 0; d < 4; ++d) {
		pp.low[d] = pes[d].low; pp.high[d] = pes[d].high; pp.failed[d] = pes[d].failed ? 1 : 0;
		pp.tab_off[d] = (int)n_tab;
		if (!pes[d].failed) {
			// (a degenerate distribution — std 0, as a user's -I can give — makes the pair score NaN / infinite for some distances,
			// and the conversion of those to int is the one place where the host's and the device's arithmetic differ: host path)
			if (!(pes[d].std > 0) || !std::isfinite(pes[d].avg) || !std::isfinite(pes[d].std)) usable = false;
			if (pes[d].high < pes[d].low || (int64_t)pes[d].high - pes[d].low > (1 << 20)) usable = false;
			else n_tab += (size_t)(pes[d].high - pes[d].low + 1);
		}
	}
	pp.ltab_n = 4 * max_len + 256;
	pp.max_XA_hits = std::min(opt->max_XA_hits, opt->max_XA_hits_alt);
	*n_tab_ = n_tab;
	return usable;
}
void pair_tables(const mem_opt_t *opt, const mem_pestat_t pes[4], const PairParams &pp, size_t n_tab, double *tab)
{
	for (int d = 0; d < 4; ++d)
		if (!pes[d].failed)
			for (int64_t dist = pes[d].low; dist <= pes[d].high; ++dist)   // src/bwamem_pair.c:218-219, the double part of q
				tab[pp.tab_off[d] + (dist - pes[d].low)] = pair_score_term(pes[d], dist, opt->a);
	double *ltab = tab + n_tab;
	ltab[0] = 1.;
	for (int l = 1; l < pp.ltab_n; ++l) ltab[l] = l < opt->mapQ_coef_len ? 1. : opt->mapQ_coef_fac / log(l);   // src/bwamem.c:964
}
void se_params(const mem_opt_t *opt, int64_t l_pac, int64_t n_processed, int max_len, PairParams &pp, mem_pestat_t pes[4])
{
	memset(pes, 0, 4 * sizeof(mem_pestat_t));
	for (int d = 0; d < 4; ++d) pes[d].failed = 1;
	size_t n_tab = 0;
	pair_params(opt, l_pac, pes, n_processed, max_len, pp, &n_tab);   // (no orientation to tabulate: always usable, n_tab = 0)
	pp.id0 = (uint64_t)n_processed;   // NOT pair_params' n_processed >> 1: the hash id of a single-end read is n_processed + i, of a pair (n_processed >> 1) + i
	pp.no_rescue = 1;
}
MswParams msw_params(const mem_opt_t *opt, int64_t l_pac)
{
	MswParams P;
	P.l_pac = l_pac;
	int8_t mn = 127, mx = 0;   // initial values of the reference's scan (src/ksw.c:83-87)
	for (int i = 0; i < 25; ++i) {
		if (opt->mat[i] < mn) mn = opt->mat[i];
		if (opt->mat[i] > mx) mx = opt->mat[i];
	}
	for (int t = 0; t < 4; ++t) {
		P.slo[t] = 0;
		for (int q = 0; q < 4; ++q) P.slo[t] |= (uint32_t)(uint8_t)opt->mat[t * 5 + q] << (8 * q);
		P.s4[t] = opt->mat[t * 5 + 4];
	}
	P.o_del = opt->o_del; P.e_del = opt->e_del; P.o_ins = opt->o_ins; P.e_ins = opt->e_ins;
	P.a = opt->a; P.min_seed_len = opt->min_seed_len;
	P.max_sc = mx > 0 ? mx : 1;
	P.shift = (uint8_t)(256 - (uint8_t)mn);
	return P;
}

bool msw_on_device(const mem_opt_t *opt) { return opt->o_ins > 0; }

// What upload and broadcast-and-commit end with: the three index buffers are filled — derive the tables (any earlier ones are dropped
// first) and mark the index usable.  MPIBWA_DEBUG: a progress line per step.
static void build_derived_tables(const char *who)
{
	const bool dbg = getenv("MPIBWA_DEBUG") != nullptr;
	free_derived_tables();
	build_occ32();
	if (dbg) fprintf(stderr, "[%s] occ32 built\n", who);
	maybe_expand_sa();
	if (dbg) fprintf(stderr, "[%s] SA expanded\n", who);
	maybe_build_p3();
	maybe_build_kmt();
	if (dbg) fprintf(stderr, "[%s] jump table and k-mer tables built\n", who);
	g_idx.ready = true;
}

} // namespace mbw

using namespace mbw;

// GPUs this process can see (0 when there is none: callers decide how many ranks share a device)
extern "C" int mi355x_device_count(void)
{
	int n = 0;
	return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// compute units of the current device (hipDeviceProp_t::multiProcessorCount: what the launchers size their grids by); 0 on failure
extern "C" int mi355x_device_cus(void)
{
	int dev = 0;
	hipDeviceProp_t prop;
	if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
	return prop.multiProcessorCount;
}

// free / total bytes of the device the index lives on (0 on success), through this library's own HIP runtime
extern "C" int mi355x_device_memory(size_t *free_bytes, size_t *total_bytes)
{
	size_t fr = 0, tot = 0;
	if (g_idx.device >= 0 && hipSetDevice(g_idx.device) != hipSuccess) return -1;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) return -1;
	if (free_bytes) *free_bytes = fr;
	if (total_bytes) *total_bytes = tot;
	return 0;
}

extern "C" int mi355x_index_alloc(int local_rank, const bwt_t *bwt, const bntseq_t *bns)
{
	require_device(local_rank);
	alloc_index(bwt, bns);   // buffers only: fill them with mi355x_index_d2d / ncclBroadcast, then mi355x_index_commit()
	return 0;
}

extern "C" int mi355x_index_upload(int local_rank, const bwt_t *bwt, const bntseq_t *bns, const uint8_t *pac)
{
	require_device(local_rank);
	alloc_index(bwt, bns);
	HIP_OK(hipMemcpy(g_idx.d_blk, bwt->bwt, (size_t)bwt->bwt_size * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(g_idx.d_sa, bwt->sa, g_idx.sa_bytes, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(g_idx.d_pac, pac, (size_t)bns->l_pac / 4 + 1, hipMemcpyHostToDevice));
	if (getenv("MPIBWA_DEBUG")) fprintf(stderr, "[upload] copied\n");
	build_derived_tables("upload");
	return 0;
}

extern "C" int mi355x_index_buffers(void **d_bwt, size_t *bwt_bytes, void **d_sa, size_t *sa_bytes, void **d_pac,
                                    size_t *pac_bytes)
{
	if (!g_idx.d_blk) return -1;
	*d_bwt = g_idx.d_blk; *bwt_bytes = g_idx.blk_bytes;
	*d_sa = g_idx.d_sa; *sa_bytes = g_idx.sa_bytes;
	*d_pac = g_idx.d_pac; *pac_bytes = g_idx.pac_bytes;
	return 0;
}

// Copy `bytes` from a device pointer owned by the caller (e.g. a torch tensor that has just received an RCCL broadcast)
// into index buffer `which` (0 = occ blocks, 1 = sampled SA, 2 = pac), or out of it when to_index == 0.
extern "C" int mi355x_index_d2d(int which, void *ext, size_t bytes, int to_index)
{
	if (!g_idx.d_blk) return -1;
	void *buf = which == 0 ? g_idx.d_blk : which == 1 ? g_idx.d_sa : g_idx.d_pac;
	size_t cap = which == 0 ? g_idx.blk_bytes : which == 1 ? g_idx.sa_bytes : g_idx.pac_bytes;
	if (bytes > cap) return -2;
	HIP_OK(hipMemcpy(to_index ? buf : ext, to_index ? ext : buf, bytes, hipMemcpyDeviceToDevice));
	return 0;
}
// after the three buffers have been filled by broadcast: expand the dense SA and mark the index usable
extern "C" int mi355x_index_commit(void)
{
	if (!g_idx.d_blk) return -1;
	build_derived_tables("commit");
	return 0;
}

extern "C" void mi355x_finalize(void)
{
	std::lock_guard<std::recursive_mutex> lk(index_mutex());
	no_calls_in_flight("mi355x_finalize");
	if (g_idx.d_blk) { (void)hipFree(g_idx.d_blk); (void)hipFree(g_idx.d_sa); (void)hipFree(g_idx.d_pac); }
	free_derived_tables();
	g_idx = DevIndex();
	release_idle_work_buffers();   // a process that is done with this index gives the HBM of its call contexts back too
	release_bgzf_contexts();
	release_bgzf_in_contexts();
	release_bam_contexts();
	release_bam_sort_contexts();
}
