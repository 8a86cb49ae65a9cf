// sam_stage.hip — the second half of mem_process_seqs(): the inputs of the SAM kernels, the units decided on the
// device, mate rescue, the host's decisions and request lists, the CIGAR-and-SAM jobs, the records, and the schedule of the parts.
#include "pipeline.h"

namespace mbw {

static_assert(sizeof(SamDesc) == sizeof(SamDescH), "host/device record layouts differ");
static_assert(sizeof(MswReq) == sizeof(MswReqH) && sizeof(MswRes) == sizeof(MswResH), "host/device record layouts differ");
static_assert(sizeof(AlnReq) == sizeof(AlnReqH) && sizeof(AlnHdr) == sizeof(AlnHdrH), "host/device record layouts differ");
static const int MSW_MAX_T = 4096;

// ---- inputs of the SAM stage (names, qualities, contig names, the gap table of the CIGAR kernel): packed and uploaded by a
// thread of their own on a side stream while phase 1 runs — 100 MB of qualities per chunk that nothing before the SAM stage reads
void Call::start_sam_inputs()
{
	// (reads so long that one request's arrays do not fit the LDS of a CU — beyond ~1 700 bp — get their CIGARs from the library's host code)
	gpu_aln = getenv("MPIBWA_HOST_CIGAR") == nullptr && aln_lds_per_block(max_len, max_len + 256) <= (size_t)160 * 1024;
	// Single-end input: the reads that end in one record are decided by se_simple_kernel and written by the single-end instantiation of
	// sam_emit_kernel (se_kernel.hip); the rest of the chunk takes the host path.  MPIBWA_HOST_SE=1 keeps every read there.
	// (-5: mem_reorder_primary5 stays host code, so the whole call does.)
	se_want = !pe && gpu_aln && getenv("MPIBWA_HOST_SAM") == nullptr && getenv("MPIBWA_HOST_SE") == nullptr && opt->mapQ_coef_len > 0 &&
	          !(opt->flag & (MEM_F_ALL | MEM_F_REF_HDR | MEM_F_PRIMARY5));
	sam_inputs.t = std::thread([this] { sam_inputs_body(); });
}

// (sets gpu_sam, dev_se — se_want and the reads uniformly with or without qualities —, sam_par, sdesc and the SAM inputs of D: read
// by the caller once the thread is joined)
void Call::sam_inputs_body()
{
	HIP_OK(hipSetDevice(ix.device));
	hipStream_t sst = C.d_streams[1];
	std::vector<int> gaptab;
	cigar_gap_table(opt, max_len, gaptab);
	int *d_gap = (int *)W.agap.ensure(gaptab.size() * 4);
	D.d_gap = d_gap;
	HIP_OK(hipMemcpyAsync(d_gap, gaptab.data(), gaptab.size() * 4, hipMemcpyHostToDevice, sst));
	// ---- SAM text of confidently paired reads on the device (sam_kernel.hip) ----
	// The COLLECT pass describes the two lines of every pair that qualifies (AlnCtx::desc); the kernel runs right behind the
	// CIGAR kernel of the part; the REPLAY pass only copies those records out of the arena and formats the rest itself.
	gpu_sam = pe && gpu_aln && getenv("MPIBWA_HOST_SAM") == nullptr && !(opt->flag & (MEM_F_ALL | MEM_F_REF_HDR));
	dev_se = se_want;
	if (gpu_sam || dev_se) {
		bool any_q = false, all_q = true;
		for (int i = 0; i < n; ++i) { if (seqs[i].qual) any_q = true; else all_q = false; }
		if (any_q && !all_q) gpu_sam = dev_se = false;   // a mix of reads with and without qualities: the host formats the chunk
		if (dev_se) {   // a chunk whose reads all carry a comment (-C) is the host's: no set-up for a kernel that would take none
			bool any_plain = false;
			for (int i = 0; i < n && !any_plain; ++i) any_plain = !seqs[i].comment;
			dev_se = any_plain;
		}
		sam_par = sam_params(bns->l_pac, any_q);
	}
	if (gpu_sam || dev_se) {
		if (gpu_sam) sdesc = (SamDescH *)W.h_sdesc.ensure((size_t)n * sizeof(SamDescH) + 64);
		int *noff = (int *)W.h_noff.ensure((size_t)(n + 1) * 4 + 64);
		std::vector<int> nlen(n);
		parallel_for(n_thr, n, 8192, [&](int i) { if (sdesc) sdesc[i].req = -1; nlen[i] = (int)strlen(seqs[i].name); });
		noff[0] = 0;
		for (int i = 0; i < n; ++i) noff[i + 1] = noff[i] + nlen[i];
		uint8_t *names = (uint8_t *)W.h_names.ensure((size_t)noff[n] + 64);
		uint8_t *hq = sam_par.has_qual ? (uint8_t *)W.h_qual.ensure(flat_bytes) : nullptr;
		parallel_for(n_thr, n, 4096, [&](int i) {
			memcpy(names + noff[i], seqs[i].name, (size_t)nlen[i]);
			if (hq) memcpy(hq + off[i], seqs[i].qual, (size_t)seqs[i].l_seq);
		});
		uint8_t *dn = (uint8_t *)W.snames.ensure((size_t)noff[n] + 64);
		int *dno = (int *)W.snoff.ensure((size_t)(n + 1) * 4);
		HIP_OK(hipMemcpyAsync(dn, names, (size_t)noff[n], hipMemcpyHostToDevice, sst));
		HIP_OK(hipMemcpyAsync(dno, noff, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, sst));
		if (hq) {
			uint8_t *dq = (uint8_t *)W.squal.ensure(flat_bytes);
			HIP_OK(hipMemcpyAsync(dq, hq, flat_bytes, hipMemcpyHostToDevice, sst));
			D.d_qual = dq;
		}
		std::vector<int> cno;
		std::vector<char> cn;
		contig_names(bns, cn, cno);
		char *dcn = (char *)W.sann_names.ensure(cn.size() + 64);
		int *dcno = (int *)W.sann_noff.ensure(cno.size() * 4);
		HIP_OK(hipMemcpyAsync(dcn, cn.data(), cn.size(), hipMemcpyHostToDevice, sst));
		HIP_OK(hipMemcpyAsync(dcno, cno.data(), cno.size() * 4, hipMemcpyHostToDevice, sst));
		stream_wait(sst);
		D.d_names = dn; D.d_noff = dno; D.d_ann_names = dcn; D.d_ann_noff = dcno;
	}
	stream_wait(sst);
}

// ---- units with one plain hit per read: decided on the device (pair_kernel.hip: pairs, ends = 2; se_kernel.hip: single-end reads
// that end in one record, ends = 1) ----
// status[k] = PR_DECIDED / SE_DECIDED: the unit's CIGAR requests and line descriptors exist on the device; the host neither lists rescue alignments nor
// marks primary hits nor plans nor formats it (it only copies the finished records out, or takes the unit back if the device hands
// a record back).
void Call::decide_on_device(int ends)
{
	const double tp0 = now_ms();
	stage(9);
	const int nu = n / ends;
	PairParams pp;
	size_t n_tab = 0;
	mem_pestat_t none[4];
	const bool usable = ends == 2 ? pair_params(opt, bns->l_pac, pes, n_processed, max_len, pp, &n_tab) : true;
	if (ends == 1) se_params(opt, bns->l_pac, n_processed, max_len, pp, none);
	if (usable) {
		const size_t tab_n = n_tab + (size_t)pp.ltab_n;   // pair scores (none for single-end reads), then the per-length table
		double *tab = (double *)W.h_pr_tab.ensure(tab_n * 8 + 64);
		pair_tables(opt, ends == 2 ? pes : none, pp, n_tab, tab);
		stage(28);
		uint8_t *ok = (uint8_t *)W.h_pr_ok.ensure((size_t)nu + 64);
		parallel_for(n_thr, nu, 8192, [&](int k) {
			const bseq1_t *s = &seqs[ends * k];
			ok[k] = ends == 2 ? !s[0].comment && !s[1].comment && strcmp(s[0].name, s[1].name) == 0 : !s[0].comment;
		});
		double *d_tab = (double *)W.pr_ptab.ensure(tab_n * 8 + 64);
		uint8_t *d_ok = (uint8_t *)W.pr_ok.ensure((size_t)nu + 64);
		uint8_t *d_status = (uint8_t *)W.pr_status.ensure((size_t)nu + 64);
		AlnReq *d_rq = (AlnReq *)W.pr_req.ensure((size_t)n * sizeof(AlnReq));
		SamDesc *d_ds = (SamDesc *)W.pr_desc.ensure((size_t)n * sizeof(SamDesc));
		uint8_t *hs = (uint8_t *)W.h_pr_status.ensure((size_t)nu + 64);
		HIP_OK(hipMemcpyAsync(d_tab, tab, tab_n * 8, hipMemcpyHostToDevice, st));
		HIP_OK(hipMemcpyAsync(d_ok, ok, (size_t)nu, hipMemcpyHostToDevice, st));
		if (ends == 2) launch_pair_simple(st, pp, nu, d_pr_first, d_pr_nfirst, d_ok, D.d_ann_off, D.d_ann_alt, d_tab, d_tab + n_tab, d_status, d_rq, d_ds);
		else launch_se_simple(st, pp, nu, d_pr_first, d_pr_nfirst, d_ok, D.d_ann_alt, d_tab, d_status, d_rq, d_ds);
		HIP_OK(hipMemcpyAsync(hs, d_status, (size_t)nu, hipMemcpyDeviceToHost, st));
		stream_wait(st);
		HIP_OK(hipGetLastError());
		bool any_dev = ends == 2;   // (single-end, none taken: no device job over n empty requests)
		for (int i = 0; i < nu && !any_dev; ++i) any_dev = hs[i] == SE_DECIDED;
		ustat = hs; dev_units = any_dev;
		wave_pp = pp; d_wave_tab = d_tab; wave_n_tab = n_tab;   // (the wave kernels: the same parameters and table)
		if (any_dev) { d_pr_req = d_rq; d_pr_desc = d_ds; }
	}
	pair_dev_ms = now_ms() - tp0;
}

// ---- mate rescue on the device: list the local alignments the pairs of a part will ask for, run them in one launch ----
void Call::mcollect(Part &P)
{
	stage(10);
	if (!gpu_msw) return;
	double ta = now_ms();
	const double ca = cpu_sec();
	const int nu = P.hi - P.lo, n_blk = (nu + 255) / 256;
	std::vector<std::vector<MswReqH>> blk_req(n_blk);
	std::vector<uint32_t> u_first(nu), u_cnt(nu);
	// (dev_wave: the pairs pair_simple_kernel left for rescue, long lists or an end without a hit also get their tags, and are pair_wave_kernel's;
	// dev_xa: the ones it left for an XA tag too; dev_pair_lines: and the ones it left for no_pairing:, codes 8 / 9 / 10)
	std::vector<std::vector<int16_t>> blk_tag(dev_wave ? n_blk : 0);
	std::vector<std::vector<int>> blk_work(dev_wave ? n_blk : 0);   // (pair, first tag in blk_tag) ...
	parallel_for(n_thr, n_blk, 1, [&](int blk) {
		std::vector<MswReqH> &rq = blk_req[blk];
		rq.reserve(256);
		const int lo = P.lo + blk * 256, hi = std::min(P.hi, lo + 256);
		for (int i = lo; i < hi; ++i) {
			const size_t before = rq.size();
			if (!(dev_units && ustat[i] == PR_DECIDED)) {
				const bseq1_t *s = &seqs[i << 1];
				const bool cand = dev_wave && (ustat[i] == PR_HOST_MAXREG || ustat[i] == PR_HOST_RESCUE || ustat[i] == PR_HOST_NO_HIT || (dev_xa && ustat[i] == PR_HOST_XA) ||
				                               (dev_pair_lines && (ustat[i] == PR_HOST_NO_PAIR || ustat[i] == PR_HOST_SCORE || ustat[i] == PR_HOST_SUPP))) &&
				                  !s[0].comment && !s[1].comment && strcmp(s[0].name, s[1].name) == 0 && pair_wave_eligible(&regs[i << 1], PW_MAXREG, dev_pair_lines);
				if (cand) {
					blk_work[blk].push_back(i); blk_work[blk].push_back((int)blk_tag[blk].size());
					sam_pe_msw_collect_tagged(opt, bns, pes, s, &regs[i << 1], i << 1, MSW_MAX_T, rq, blk_tag[blk]);
					wave_cand[i] = 1;
				} else sam_pe_msw_collect(opt, bns, pes, s, &regs[i << 1], i << 1, MSW_MAX_T, rq);
			}
			u_first[i - P.lo] = (uint32_t)before; u_cnt[i - P.lo] = (uint32_t)(rq.size() - before);
		}
	});
	P.mbase.assign(nu + 1, 0);
	for (int i = 0; i < nu; ++i) P.mbase[i + 1] = P.mbase[i] + u_cnt[i];
	P.work.clear(); P.w_mfirst.clear(); P.w_toff.clear(); P.w_tags.clear();
	for (int blk = 0; blk < (int)blk_work.size(); ++blk) {
		const size_t tag0 = P.w_tags.size();
		for (size_t x = 0; x < blk_work[blk].size(); x += 2) {
			const int i = blk_work[blk][x];
			P.work.push_back(i);
			P.w_mfirst.push_back(P.mbase[i - P.lo]);
			P.w_toff.push_back((int)(tag0 + (size_t)blk_work[blk][x + 1]));
		}
		P.w_tags.insert(P.w_tags.end(), blk_tag[blk].begin(), blk_tag[blk].end());
	}
	P.w_toff.push_back((int)P.w_tags.size());
	P.n_mreq = P.mbase[nu];
	P.mreq = (MswReqH *)W.h_mreq[P.slot].ensure(P.n_mreq * sizeof(MswReqH) + 64);
	P.mres = (MswResH *)W.h_mres[P.slot].ensure(P.n_mreq * sizeof(MswResH) + 64);
	parallel_for(n_thr, nu, 4096, [&](int i) {
		if (u_cnt[i]) memcpy(&P.mreq[P.mbase[i]], &blk_req[i >> 8][u_first[i]], (size_t)u_cnt[i] * sizeof(MswReqH));
	});
	msw_ms += now_ms() - ta;
	cpu_msw += cpu_sec() - ca;
}

void Call::mlaunch(Part &P)
{
	stage(11);
	if (!gpu_msw || (P.n_mreq == 0 && P.work.empty())) return;
	P.mst = C.a_streams[P.slot];
	P.m_launched = true;
	if (P.n_mreq == 0) { wave_launch(P); return; }
	P.msw_launched = true;
	int max_t = 1;
	for (size_t k = 0; k < P.n_mreq; ++k) max_t = std::max(max_t, (int)(P.mreq[k].re - P.mreq[k].rb));
	MswReq *d_req = (MswReq *)W.mreq[P.slot].ensure(P.n_mreq * sizeof(MswReq));
	MswRes *d_res = (MswRes *)W.mres[P.slot].ensure(P.n_mreq * sizeof(MswRes));
	// row-maximum scratch: at most 2 GiB at a time
	size_t per = std::max<size_t>(64, (((size_t)1 << 31) / ((size_t)max_t * 2)) & ~(size_t)63);
	per = std::min(per, (P.n_mreq + 63) & ~(size_t)63);
	uint16_t *d_rows = (uint16_t *)W.mrows[P.slot].ensure(per * (size_t)max_t * 2);
	HIP_OK(hipMemcpyAsync(d_req, P.mreq, P.n_mreq * sizeof(MswReq), hipMemcpyHostToDevice, P.mst));
	const MswParams mp = msw_params(opt, bns->l_pac);
	P.mev.start(P.mst);
	int *h_ml = (int *)W.h_mlist[P.slot].ensure(2 * P.n_mreq * sizeof(int) + 64), *d_ml = (int *)W.mlist[P.slot].ensure(2 * P.n_mreq * sizeof(int) + 64);
	int *d_mt = (int *)W.mtail[P.slot].ensure(msw_tail_ints(per) * sizeof(int));   // (one batch after the other on the stream)
	for (size_t b = 0; b < P.n_mreq; b += per) {
		const int cnt = (int)std::min(per, P.n_mreq - b);
		launch_msw(P.mst, mp, cnt, d_req + b, D.d_seq, D.d_off, D.d_len, D.d_pac, d_res + b, d_rows, max_len, (const MswReq *)(P.mreq + b), lens,
		           h_ml + 2 * b, d_ml + 2 * b, d_mt);
	}
	P.mev.stop(P.mst);
	wave_launch(P);
	HIP_OK(hipMemcpyAsync(P.mres, d_res, P.n_mreq * sizeof(MswRes), hipMemcpyDeviceToHost, P.mst));   // pinned: truly asynchronous
}

// (the work list's size moves from chunk to chunk: twice the first size seen, so that the buffers settle during the first calls.  Not
// rounded to a power of two: the headline's 26 000 pairs a chunk sit at such a boundary, and one chunk in a few crossed it)
static size_t roomy(size_t bytes)
{
	return std::max<size_t>(2 * bytes, (size_t)1 << 16);
}

// a read's region list as the wave kernels take it: the fields of mem_alnreg_t the deciding stages read
static void pack_list(const HRegV &v, DevReg *o)
{
	for (size_t j = 0; j < v.size(); ++j) {
		const HReg &h = v[j];
		DevReg d;
		d.rb = h.rb; d.re = h.re; d.qb = h.qb; d.qe = h.qe; d.rid = h.rid; d.score = h.score; d.truesc = h.truesc; d.w = h.w;
		d.seedcov = h.seedcov; d.seedlen0 = h.seedlen0; d.frac_rep = h.frac_rep; d.pad = 0;
		o[j] = d;
	}
}

// A wave kernel's work list on stream wst: `ends` region lists per item — the host's own (after mem_sort_dedup_patch), packed with
// offsets —, status bytes and (xa) XA counts cleared, room for the kernel's requests, descriptors and XA requests (PW_XA_CAP per
// (item, end)).  more: what else the kernel reads per item, uploaded behind the lists and before the clears.
// lines: the side arrays by line (se_wave_kernel's reads of several lines, pair_wave_kernel's pairs reported end by end), SE_LINES_CAP
// slots per list, line counts cleared.
Call::WaveList Call::wave_list(WaveBufs &B, hipStream_t wst, int ends, const std::vector<int> &items, bool xa, std::initializer_list<Upload> more, bool lines)
{
	const int nw = (int)items.size(), nl = ends * nw;   // items, lists
	size_t n_regs = 0;
	int *loff = (int *)B.h_loff.ensure(roomy(((size_t)nl + 1) * 4 + 64));
	loff[0] = 0;
	for (int t = 0; t < nw; ++t)
		for (int e = 0; e < ends; ++e) { n_regs += regs[ends * items[t] + e].size(); loff[ends * t + e + 1] = (int)n_regs; }
	DevReg *hl = (DevReg *)B.h_lists.ensure(roomy(n_regs * sizeof(DevReg) + 64));
	parallel_for(n_thr, nw, 512, [&](int t) {
		for (int e = 0; e < ends; ++e) pack_list(regs[ends * items[t] + e], hl + loff[ends * t + e]);
	});
	int *hw = (int *)B.h_work.ensure(roomy((size_t)nw * 4 + 64));
	memcpy(hw, items.data(), (size_t)nw * 4);
	WaveList L;
	L.h_status = (uint8_t *)B.h_status.ensure(roomy((size_t)nw + 64));
	L.work = (int *)B.work.ensure(roomy((size_t)nw * 4));
	L.lists = (DevReg *)B.lists.ensure(roomy(n_regs * sizeof(DevReg) + 64));
	L.loff = (int *)B.loff.ensure(roomy(((size_t)nl + 1) * 4));
	L.status = (uint8_t *)B.status.ensure(roomy((size_t)nw + 64));
	L.req = (AlnReq *)B.req.ensure(roomy((size_t)nl * sizeof(AlnReq)));
	L.desc = (SamDesc *)B.desc.ensure(roomy((size_t)nl * sizeof(SamDesc)));
	HIP_OK(hipMemcpyAsync(L.work, hw, (size_t)nw * 4, hipMemcpyHostToDevice, wst));
	if (n_regs) HIP_OK(hipMemcpyAsync(L.lists, hl, n_regs * sizeof(DevReg), hipMemcpyHostToDevice, wst));
	HIP_OK(hipMemcpyAsync(L.loff, loff, ((size_t)nl + 1) * 4, hipMemcpyHostToDevice, wst));
	for (const Upload &u : more)
		if (u.bytes) HIP_OK(hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, wst));
	HIP_OK(hipMemsetAsync(L.status, 0, (size_t)nw, wst));
	L.xreq = nullptr; L.xcnt = L.h_xcnt = nullptr;
	if (xa) {
		L.xreq = (AlnReq *)B.xreq.ensure(roomy((size_t)nl * PW_XA_CAP * sizeof(AlnReq)));
		L.xcnt = (uint8_t *)B.xcnt.ensure(roomy((size_t)nl + 64));
		L.h_xcnt = (uint8_t *)B.h_xcnt.ensure(roomy((size_t)nl + 64));
		HIP_OK(hipMemsetAsync(L.xcnt, 0, (size_t)nl, wst));
	}
	L.h_nlines = L.h_lxcnt = nullptr;
	if (lines) {
		const size_t ns = (size_t)nl * SE_LINES_CAP;   // line slots
		L.lines.n_lines = (uint8_t *)B.nlines.ensure(roomy((size_t)nl + 64));
		L.lines.desc = (SamDesc *)B.ldesc.ensure(roomy(ns * sizeof(SamDesc)));
		L.lines.reqs = (AlnReq *)B.lreq.ensure(roomy(ns * sizeof(AlnReq)));
		L.lines.xa_cnt = (uint8_t *)B.lxcnt.ensure(roomy(ns + 64));
		L.lines.xa_reqs = xa ? (AlnReq *)B.lxreq.ensure(roomy(ns * PW_XA_CAP * sizeof(AlnReq))) : nullptr;
		L.h_nlines = (uint8_t *)B.h_nlines.ensure(roomy((size_t)nl + 64));
		L.h_lxcnt = (uint8_t *)B.h_lxcnt.ensure(roomy(ns + 64));
		se_lines_options(opt, L.lines);
		HIP_OK(hipMemsetAsync(L.lines.n_lines, 0, (size_t)nl, wst));
		HIP_OK(hipMemsetAsync(L.lines.xa_cnt, 0, ns, wst));
	}
	return L;
}

// pair_wave_kernel over the part's work list, behind the mate-rescue kernel on its stream; the status bytes come back on the same
// stream, so that mfinish's wait delivers them.
void Call::wave_launch(Part &P)
{
	const int nw = (int)P.work.size();
	if (nw == 0) return;
	const int s = P.slot;
	WaveBufs &B = W.wave[s];
	unsigned *hm = (unsigned *)B.h_mfirst.ensure(roomy((size_t)nw * 4 + 64));
	int *ht = (int *)B.h_toff.ensure(roomy((size_t)(nw + 1) * 4 + 64));
	int16_t *hg = (int16_t *)B.h_tags.ensure(roomy(P.w_tags.size() * 2 + 64));
	memcpy(hm, P.w_mfirst.data(), (size_t)nw * 4); memcpy(ht, P.w_toff.data(), (size_t)(nw + 1) * 4);
	memcpy(hg, P.w_tags.data(), P.w_tags.size() * 2);
	unsigned *d_mf = (unsigned *)B.mfirst.ensure(roomy((size_t)nw * 4));
	int *d_toff = (int *)B.toff.ensure(roomy((size_t)(nw + 1) * 4));
	short *d_tags = (short *)B.tags.ensure(roomy(P.w_tags.size() * 2 + 64));
	// (a part without a rescue request has no request or result array: the kernel reads neither, every tag says so)
	const MswReq *d_req = (const MswReq *)W.mreq[s].ensure(std::max<size_t>(P.n_mreq, 1) * sizeof(MswReq));
	const MswRes *d_res = (const MswRes *)W.mres[s].ensure(std::max<size_t>(P.n_mreq, 1) * sizeof(MswRes));
	const WaveList L = wave_list(B, P.mst, 2, P.work, dev_xa,
	                             {{d_mf, hm, (size_t)nw * 4}, {d_toff, ht, (size_t)(nw + 1) * 4}, {d_tags, hg, P.w_tags.size() * 2}}, dev_pair_lines);
	launch_pair_wave(P.mst, wave_pp, nw, L.work, L.lists, L.loff, D.d_len, d_req, d_res, d_mf, d_tags, d_toff, D.d_ann_off, d_wave_tab, d_wave_tab + wave_n_tab,
	                 L.status, L.req, L.desc, L.xreq, L.xcnt, dev_pair_lines ? &L.lines : nullptr);
	HIP_OK(hipMemcpyAsync(L.h_status, L.status, (size_t)nw, hipMemcpyDeviceToHost, P.mst));
	if (dev_xa) HIP_OK(hipMemcpyAsync(L.h_xcnt, L.xcnt, (size_t)2 * nw, hipMemcpyDeviceToHost, P.mst));
	if (dev_pair_lines) {
		HIP_OK(hipMemcpyAsync(L.h_nlines, L.lines.n_lines, (size_t)2 * nw, hipMemcpyDeviceToHost, P.mst));
		HIP_OK(hipMemcpyAsync(L.h_lxcnt, L.lines.xa_cnt, (size_t)2 * nw * SE_LINES_CAP, hipMemcpyDeviceToHost, P.mst));
	}
	P.wstatus = L.h_status; P.wxcnt = L.h_xcnt; P.wnlines = L.h_nlines; P.wlxcnt = L.h_lxcnt;
}

// The units a wave kernel decided with a request count of their own — pair_wave_kernel's pairs with an XA tag (3 to 2 + 2 PW_XA_CAP
// requests each), se_wave_kernel's reads (1 to 1 + PW_XA_CAP) — never ride in the part's device job (`ends` requests per unit, in place):
// the host lays out their request bases (no request for any other unit of the part), a kernel moves requests and descriptors there, and
// one more CIGAR-and-SAM job runs over the part for these units alone.  B, items: the work list; xcnt: its XA counts, or null.
void Call::own_job_records(Part &P, int ends, const WaveBufs &B, const std::vector<int> &items, const uint8_t *xcnt)
{
	const int s = P.slot, nw = (int)items.size(), nu = P.hi - P.lo;
	auto in_job = [&](int t) {
		const int i = items[t];
		return ends == 2 ? (P.wstatus[t] == PW_DECIDED_XA && dev_xa) || (P.wstatus[t] == PW_DECIDED_LINES && dev_pair_lines) : i >= P.lo && i < P.hi && wave_dec[i];
	};
	// (se_wave_kernel's reads of several lines: a request per line and per XA entry of a line, from the counts that came back with the
	// status bytes; they ride in the same job, and sam_lines_kernel writes them behind sam_emit_kernel)
	// (pair_wave_kernel's pairs reported end by end: the same per end, 0 .. SE_LINES_CAP lines each; a pair of two unaligned records has
	// no request and is a unit of sam_lines_kernel all the same)
	const bool by_line = ends == 1 ? dev_se_supp && se_wnlines : dev_pair_lines && P.wnlines;
	const uint8_t *nlines = ends == 1 ? se_wnlines : P.wnlines, *lxcnt = ends == 1 ? se_wlxcnt : P.wlxcnt;
	auto lines_unit = [&](int t) { return by_line && (ends == 1 ? nlines[t] > 0 : P.wstatus[t] == PW_DECIDED_LINES); };
	auto n_lines_of = [&](int x) { return (int)std::min<int>(nlines[x], SE_LINES_CAP); };   // x: the list, ends * t + e
	P.xa_base.assign(nu + 1, 0);
	int n_dec = 0, n_multi = 0;
	for (int t = 0; t < nw; ++t) {
		if (!in_job(t)) continue;
		const bool lu = lines_unit(t);
		for (int e = 0; e < ends; ++e) {
			const int x = ends * t + e;
			if (!lu) { P.xa_base[items[t] - P.lo + 1] += 1 + (xcnt ? std::min<int>(xcnt[x], PW_XA_CAP) : 0); continue; }
			for (int j = 0; j < n_lines_of(x); ++j) P.xa_base[items[t] - P.lo + 1] += 1 + std::min<int>(lxcnt[(size_t)x * SE_LINES_CAP + j], PW_XA_CAP);
		}
		++n_dec;
		n_multi += lu;
	}
	if (n_dec == 0) return;
	hipStream_t jst = C.d_streams[s];
	for (int k = 0; k < nu; ++k) P.xa_base[k + 1] += P.xa_base[k];
	int *dst = (int *)W.wave[s].h_dst.ensure(roomy((size_t)nw * 4 + 64));   // (the part's: se_wave_kernel's one list serves both parts)
	for (int t = 0; t < nw; ++t) dst[t] = in_job(t) && !lines_unit(t) ? (int)P.xa_base[items[t] - P.lo] : -1;
	const size_t n_req = P.xa_base[nu];
	int *d_dst = (int *)W.wave[s].dst.ensure(roomy((size_t)nw * 4));
	int *d_ldst = nullptr;
	if (n_multi) {
		int *ldst = (int *)W.wave[s].h_ldst.ensure(roomy((size_t)nw * 4 + 64));
		for (int t = 0; t < nw; ++t) ldst[t] = in_job(t) && lines_unit(t) ? (int)P.xa_base[items[t] - P.lo] : -1;
		d_ldst = (int *)W.wave[s].ldst.ensure(roomy((size_t)nw * 4));
		HIP_OK(hipMemcpyAsync(d_ldst, ldst, (size_t)nw * 4, hipMemcpyHostToDevice, C.d_streams[s]));
	}
	AlnReq *d_rq = (AlnReq *)W.xa_req[s].ensure(roomy(n_req * sizeof(AlnReq)));
	SamDesc *d_ds = (SamDesc *)W.xa_desc.ensure((size_t)n * sizeof(SamDesc));
	HIP_OK(hipMemcpyAsync(d_dst, dst, (size_t)nw * 4, hipMemcpyHostToDevice, jst));
	launch_wave_job_scatter(jst, ends, nw, (const int *)B.work.p, d_dst, (const AlnReq *)B.req.p, (const SamDesc *)B.desc.p, xcnt ? (const AlnReq *)B.xreq.p : nullptr,
	                        xcnt ? (const uint8_t *)B.xcnt.p : nullptr, d_rq, d_ds, ends * P.lo, ends * nu);
	if (n_multi)
		launch_lines_job_scatter(jst, ends, nw, d_ldst, (const uint8_t *)B.nlines.p, (const AlnReq *)B.lreq.p, (const uint8_t *)B.lxcnt.p, (const AlnReq *)B.lxreq.p, d_rq);
	HIP_OK(hipGetLastError());
	unsigned long long *small = (unsigned long long *)W.h_small[s].ensure(512);
	P.xa.small_used = small + 48; P.xa.small_cnt = small + 56;
	job_launch(P.xa, W.xa_job[s], jst, P, d_rq, n_req, P.xa_base.data(), true, nullptr, d_ds, n_multi ? &B : nullptr, n_multi ? nw : 0);
}

// ---- single-end reads with long lists or an XA tag: se_wave_kernel (se_wave_kernel.hip) ----
// The reads se_simple_kernel left with "more than eight regions" or "a secondary region with an XA entry", once over the chunk: their
// work list and the kernel on the call's stream, status bytes and XA counts back, merged into the chunk's decisions.
// MPIBWA_HOST_SE_WAVE=1 turns the path off; MPIBWA_HOST_XA=1 or max_XA_hits beyond the kernel's side array only its XA listing (such a
// read comes back with SE_HOST_XA).
void Call::se_wave_decide()
{
	dev_se_wave = !pe && dev_se && ustat && getenv("MPIBWA_HOST_SE_WAVE") == nullptr;
	if (!dev_se_wave) return;
	const double tp0 = now_ms();
	dev_se_xa = wave_pp.max_XA_hits <= PW_XA_CAP && getenv("MPIBWA_HOST_XA") == nullptr;
	// reads of several lines: on unless MPIBWA_HOST_SUPP is set to something other than 0
	const char *hs = getenv("MPIBWA_HOST_SUPP");
	dev_se_supp = !(hs && atoi(hs) != 0);
	wave_dec.assign(n, 0);
	se_work.clear();
	for (int i = 0; i < n; ++i)
		if ((ustat[i] == SE_HOST_MAXREG || ustat[i] == SE_HOST_XA || (dev_se_supp && ustat[i] == SE_HOST_SUPP)) && !seqs[i].comment &&
		    se_wave_eligible(regs[i], PW_MAXREG))
			se_work.push_back(i);
	const int nw = (int)se_work.size();
	if (nw == 0) return;
	const WaveList L = wave_list(se_bufs(), st, 1, se_work, dev_se_xa, {}, dev_se_supp);
	launch_se_wave(st, wave_pp, nw, L.work, L.lists, L.loff, D.d_ann_alt, d_wave_tab + wave_n_tab, L.status, L.req, L.desc, L.xreq, L.xcnt,
	               dev_se_supp ? &L.lines : nullptr);
	HIP_OK(hipMemcpyAsync(L.h_status, L.status, (size_t)nw, hipMemcpyDeviceToHost, st));
	if (dev_se_xa) HIP_OK(hipMemcpyAsync(L.h_xcnt, L.xcnt, (size_t)nw, hipMemcpyDeviceToHost, st));
	if (dev_se_supp) {
		HIP_OK(hipMemcpyAsync(L.h_nlines, L.lines.n_lines, (size_t)nw, hipMemcpyDeviceToHost, st));
		HIP_OK(hipMemcpyAsync(L.h_lxcnt, L.lines.xa_cnt, (size_t)nw * SE_LINES_CAP, hipMemcpyDeviceToHost, st));
	}
	stream_wait(st);
	HIP_OK(hipGetLastError());
	se_wxcnt = L.h_xcnt; se_wnlines = L.h_nlines; se_wlxcnt = L.h_lxcnt;
	for (int t = 0; t < nw; ++t) {   // its decisions: these reads are the device's from here on
		const int i = se_work[t];
		const uint8_t ws = L.h_status[t];
		if (ws == SE_DECIDED) { ustat[i] = SE_DECIDED; wave_dec[i] = 1; ++n_se_wave; }
		else if (ws == SE_DECIDED_XA && dev_se_xa) { ustat[i] = SE_DECIDED_XA; wave_dec[i] = 1; ++n_se_xa; }
		else if (ws == SE_DECIDED_LINES && dev_se_supp) { ustat[i] = SE_DECIDED_LINES; wave_dec[i] = 1; ++n_se_supp; }
		else if (ws) ustat[i] = ws;   // (why not: for the statistics line)
	}
	if (n_se_wave + n_se_xa + n_se_supp) dev_units = true;   // (se_simple_kernel may have taken none)
	pair_dev_ms += now_ms() - tp0;
}

// The pairs pair_wave_kernel decided become units of the device: their requests and descriptors go into the chunk-wide arrays of the
// deciding kernels, on the stream of the part's device job.  own_job (that job has already gone out and is back): the arrays are
// cleared for the part first, and one more job of the same type runs over it — the wave's pairs alone.
void Call::wave_records(Part &P, bool own_job)
{
	if (P.n_wave_dec == 0) return;
	const int s = P.slot, nw = (int)P.work.size();
	hipStream_t jst = C.d_streams[s];
	launch_pair_wave_scatter(jst, nw, (const int *)W.wave[s].work.p, (const uint8_t *)W.wave[s].status.p, (const AlnReq *)W.wave[s].req.p, (const SamDesc *)W.wave[s].desc.p,
	                         const_cast<AlnReq *>(d_pr_req), const_cast<SamDesc *>(d_pr_desc), 2 * P.lo, own_job ? 2 * (P.hi - P.lo) : 0);
	HIP_OK(hipGetLastError());
	if (!own_job) return;
	unsigned long long *small = (unsigned long long *)W.h_small[s].ensure(512);
	P.wave.small_used = small + 32; P.wave.small_cnt = small + 40;
	job_launch(P.wave, W.wave_job[s], jst, P, d_pr_req + (size_t)P.lo * 2, (size_t)(P.hi - P.lo) * 2, nullptr, true, nullptr, const_cast<SamDesc *>(d_pr_desc));
}

void Call::mfinish(Part &P)
{
	stage(12);
	if (!P.m_launched) return;
	double ta = now_ms();
	stream_wait(P.mst);
	HIP_OK(hipGetLastError());
	if (P.msw_launched) STAT.k_msw_ms += P.mev.ms();
	STAT.n_msw += P.n_mreq;
	uint64_t n_plain_from_xa = 0;
	for (size_t t = 0; t < P.work.size(); ++t) {   // pair_wave_kernel's decisions: its pairs are the device's from here on
		const int i = P.work[t];
		// (pair_simple_kernel's XA test is coarse — any close secondary hit under any primary one —, so some of the pairs it left for XA
		// come back plain: more than max_XA_hits entries, or entries under a hit that is not the chosen one)
		if (P.wstatus[t] == PR_DECIDED) { if (ustat[i] == PR_HOST_XA) ++n_plain_from_xa; ustat[i] = PR_DECIDED; wave_dec[i] = 1; ++P.n_wave_dec; }
		else if (P.wstatus[t] == PW_DECIDED_XA && dev_xa) { ustat[i] = PW_DECIDED_XA; ++P.n_xa_dec; }
		else if (P.wstatus[t] == PW_DECIDED_LINES && dev_pair_lines) { ustat[i] = PW_DECIDED_LINES; ++P.n_lines_dec; }
		else if (P.wstatus[t]) ustat[i] = P.wstatus[t];   // (why not: for the statistics line)
	}
	n_pair_lines += (uint64_t)P.n_lines_dec;
	n_wave += (uint64_t)P.n_wave_dec - n_plain_from_xa;
	n_xa_plain += n_plain_from_xa;
	n_xa_pairs += (uint64_t)P.n_xa_dec + n_plain_from_xa;
	msw_ms += now_ms() - ta;
}

// A: decisions + the list of CIGARs to compute.  Two rounds, so that the units that asked for no mate-rescue alignment
// (most of them) are done while msw_kernel is still running: round 0 = those units, round 1 = the rest + the flat list.
void Call::collect(Part &P, int round)
{
	stage(13);
	double ta = now_ms();
	const double ca = cpu_sec();
	const int nu = P.hi - P.lo, n_blk = (nu + 255) / 256;
	if (round == 0) { P.blk_req.assign(n_blk, std::vector<AlnReqH>()); P.u_first.assign(nu, 0); P.u_cnt.assign(nu, 0); }
	parallel_for(n_thr, n_blk, 1, [&](int blk) {
		std::vector<AlnReqH> &rq = P.blk_req[blk];
		if (round == 0) rq.reserve(256 * 3);
		AlnCtx ctx;
		ctx.mode = AlnCtx::COLLECT; ctx.reqs = &rq;
		const int lo = P.lo + blk * 256, hi = std::min(P.hi, lo + 256);
		unsigned long long tsc_plan_blk = 0, tsc_emitc_blk = 0;
		for (int i = lo; i < hi; ++i) {
			const int k = i - P.lo;
			if (dev_units && (ustat[i] == PR_DECIDED || ustat[i] == PW_DECIDED_XA || ustat[i] == SE_DECIDED_LINES)) continue;   // decided on the device (17 is PW_DECIDED_LINES too)
			const bool has_msw = P.m_launched && P.mbase[k + 1] != P.mbase[k];   // needs results of the mate-rescue kernel
			const bool waits = has_msw || (dev_wave && wave_cand[i]);            // ... or pair_wave_kernel's word on whose pair it is
			if (waits != (round == 1)) continue;
			const size_t before = rq.size();
			if (pe) {
				MswCtx mc;
				if (has_msw) { mc.req = P.mreq + P.mbase[k]; mc.res = P.mres + P.mbase[k]; mc.n = (int)(P.mbase[k + 1] - P.mbase[k]); }
				const unsigned long long c0 = cpusec_on() ? __builtin_ia32_rdtsc() : 0;
				sam_pe_plan(opt, bns, pac, pes, (uint64_t)((n_processed >> 1) + i), &seqs[i << 1], &regs[i << 1], plans[i], has_msw ? &mc : nullptr,
				            i << 1);
				const unsigned long long c1 = cpusec_on() ? __builtin_ia32_rdtsc() : 0;
				ctx.desc = gpu_sam ? &sdesc[i << 1] : nullptr;
				if (gpu_aln) sam_pe_emit(opt, bns, pac, pes, &seqs[i << 1], &regs[i << 1], plans[i], &ctx, i << 1);
				if (cpusec_on()) { tsc_plan_blk += c1 - c0; tsc_emitc_blk += __builtin_ia32_rdtsc() - c1; }
			} else {
				mark_primary_se(opt, regs[i], n_processed + i);
				if (opt->flag & MEM_F_PRIMARY5) reorder_primary5(opt->T, regs[i]);
				if (gpu_aln) reg2sam(opt, bns, pac, &seqs[i], regs[i], 0, 0, &ctx, i);
			}
			P.u_first[k] = (uint32_t)before; P.u_cnt[k] = (uint32_t)(rq.size() - before);
		}
		if (cpusec_on()) { tsc_plan += tsc_plan_blk; tsc_emitc += tsc_emitc_blk; }
	});
	if (round == 1) {
		P.base.assign(nu + 1, 0);
		for (int i = 0; i < nu; ++i) P.base[i + 1] = P.base[i] + P.u_cnt[i];
		P.n_req = P.base[nu];
		P.req = (AlnReqH *)W.h_areq[P.slot].ensure(P.n_req * sizeof(AlnReqH) + 64);
		parallel_for(n_thr, nu, 4096, [&](int i) {
			if (P.u_cnt[i]) memcpy(&P.req[P.base[i]], &P.blk_req[i >> 8][P.u_first[i]], (size_t)P.u_cnt[i] * sizeof(AlnReqH));
		});
	}
	plan_ms += now_ms() - ta;
	cpu_collect += cpu_sec() - ca;
}

// ---- the CIGAR-and-SAM job ----
// Queue a job over the reads of part P on jst.  d_req: the requests where they are on the device, or null: P.req is uploaded.  base:
// the first request of every unit, or null: `ends` requests per unit.  with_sam: the records behind the CIGARs, from the descriptors
// d_desc (of the chunk; h_desc given: the part's are uploaded first).
void Call::job_launch(Job &J, JobBufs &B, hipStream_t jst, const Part &P, const AlnReq *d_req, size_t n_req, const uint32_t *base, bool with_sam,
                      const SamDescH *h_desc, SamDesc *d_desc, const WaveBufs *multi, int n_multi)
{
	const int ends = pe ? 2 : 1;   // reads per unit
	const int nu = P.hi - P.lo, nr = nu * ends;
	J.B = &B; J.st = jst; J.n_req = n_req; J.n_reads = nr;
	J.pool_bytes = aln_pool_bytes(n_req);
	AlnSamJob Q;
	AlnReq *d_up = d_req ? nullptr : (AlnReq *)B.req.ensure(n_req * sizeof(AlnReq));
	J.d_hdr = (AlnHdr *)B.hdr.ensure(n_req * sizeof(AlnHdr));
	J.d_pool = (uint8_t *)B.pool.ensure(J.pool_bytes);
	J.d_cnt = (unsigned long long *)B.cnt.ensure(256);
	if (d_up) HIP_OK(hipMemcpyAsync(d_up, P.req, n_req * sizeof(AlnReq), hipMemcpyHostToDevice, jst));
	Q.n_req = (int)n_req; Q.d_req = d_req ? d_req : d_up; Q.d_hdr = J.d_hdr; Q.d_pool = J.d_pool; Q.pool_bytes = J.pool_bytes; Q.d_cnt = J.d_cnt;
	Q.d_lists = (int *)B.lists.ensure(n_req * 3 * sizeof(int));
	if (with_sam) {
		int *hb = (int *)B.h_base.ensure((size_t)(nu + 1) * 4 + 64);
		for (int k = 0; k <= nu; ++k) hb[k] = base ? (int)base[k] : ends * k;
		J.arena_bytes = sam_arena_bytes(nr, max_len);
		Q.ends = ends; Q.r0 = P.lo * ends; Q.n_reads = nr;
		Q.h_desc = (const SamDesc *)h_desc; Q.d_desc = d_desc;
		Q.h_base = hb; Q.d_base = (int *)B.base.ensure((size_t)(nu + 1) * 4);
		Q.d_arena = (uint8_t *)B.arena.ensure(J.arena_bytes); Q.arena_bytes = J.arena_bytes;
		Q.d_used = (unsigned long long *)B.used.ensure(64);
		Q.d_ooff = (unsigned long long *)B.ooff.ensure((size_t)nr * 8);
		Q.d_olen = (int *)B.olen.ensure((size_t)nr * 4);
		if (multi && n_multi > 0) {   // a wave kernel's units of several lines: a unit per item of its work list, those of this job by ldst >= 0
			const int s = P.slot;
			Q.n_multi = n_multi; Q.d_mlist = (const int *)multi->work.p; Q.d_mlines = (const uint8_t *)multi->nlines.p;
			Q.d_mdesc = (const SamDesc *)multi->ldesc.p; Q.d_mbase = (const int *)W.wave[s].ldst.p;
		}
	}
	// (the results are fetched in job_fetch: a D2H copy into pageable memory would block the host here)
	queue_aln_sam(jst, opt, bns->l_pac, D, sam_par, Q, J.ev.a, J.ev.b);
	J.launched = true; J.sam_launched = with_sam;
}

// the CIGAR results of a job: counters, then headers and what is used of the pool
static void fetch_results(Job &J)
{
	JobBufs &B = *J.B;
	HIP_OK(hipMemcpyAsync(J.small_cnt, J.d_cnt, 64, hipMemcpyDeviceToHost, J.st));
	stream_wait(J.st);
	const size_t used = std::min<size_t>(J.small_cnt[0], J.pool_bytes);
	AlnHdrH *hh = (AlnHdrH *)B.h_hdr.ensure(J.n_req * sizeof(AlnHdr) + 64);
	uint8_t *hp = (uint8_t *)B.h_pool.ensure(used + 64);
	HIP_OK(hipMemcpyAsync(hh, J.d_hdr, J.n_req * sizeof(AlnHdr), hipMemcpyDeviceToHost, J.st));
	if (used) HIP_OK(hipMemcpyAsync(hp, J.d_pool, used, hipMemcpyDeviceToHost, J.st));
	stream_wait(J.st);
	J.hdr = hh; J.pool = hp;
}

// its records: the arena cursor, then what is used of the arena, offsets and lengths
static void fetch_records(Job &J)
{
	JobBufs &B = *J.B;
	const int nr = J.n_reads;
	HIP_OK(hipMemcpyAsync(J.small_used, B.used.p, 8, hipMemcpyDeviceToHost, J.st));
	stream_wait(J.st);
	const unsigned long long used = std::min<unsigned long long>(J.small_used[0], J.arena_bytes);
	uint8_t *ha = (uint8_t *)B.h_arena.ensure((size_t)used + 64);
	unsigned long long *ho = (unsigned long long *)B.h_ooff.ensure((size_t)nr * 8 + 64);
	int *hl = (int *)B.h_olen.ensure((size_t)nr * 4 + 64);
	if (used) HIP_OK(hipMemcpyAsync(ha, B.arena.p, (size_t)used, hipMemcpyDeviceToHost, J.st));
	HIP_OK(hipMemcpyAsync(ho, B.ooff.p, (size_t)nr * 8, hipMemcpyDeviceToHost, J.st));
	HIP_OK(hipMemcpyAsync(hl, B.olen.p, (size_t)nr * 4, hipMemcpyDeviceToHost, J.st));
	stream_wait(J.st);
	J.sarena = ha; J.sooff = ho; J.solen = hl;
}

// Wait for a job and fetch what the host needs of it.  FETCH_ALWAYS: the CIGAR results, then the records (the host's units: REPLAY reads
// the results).  FETCH_IF_HANDED_BACK: the records, and the CIGAR results only if a unit decided on the device comes back without a
// record (CIGAR declined, row overflow): the host redoes that unit and needs them.
void Call::job_fetch(Job &J, const Part &P, Fetch policy, bool wave_units)
{
	if (!J.launched) return;
	const double ta = now_ms();
	stream_wait(J.st);
	HIP_OK(hipGetLastError());
	STAT.k_aln_ms += J.ev.ms();
	STAT.n_aln += J.n_req;
	if (policy == FETCH_ALWAYS) fetch_results(J);   // (FETCH_RECORDS: the records alone; the host redoes a unit handed back from scratch)
	if (J.sam_launched) fetch_records(J);
	if (policy == FETCH_IF_HANDED_BACK) {
		const int ends = pe ? 2 : 1;
		bool any_back = false;
		for (int k = 0; k < P.hi - P.lo && !any_back; ++k)
			for (int e = 0; e < ends; ++e)
				any_back = any_back || (ustat[P.lo + k] == PR_DECIDED && (!wave_units || wave_dec[P.lo + k]) && !(dev_se_wave && wave_dec[P.lo + k]) &&
				                        J.solen[ends * k + e] < 0);   // (se_wave_kernel's reads have a job of their own)
		if (any_back) fetch_results(J);
	}
	aln_wait_ms += now_ms() - ta;
}

// The units decided on the device need nothing from the host any more: their CIGARs and records are queued right behind the
// deciding kernel, on a stream of their own, and run under the host's rescue listing, planning and the mate-rescue kernel.
void Call::launch_dev(Part &P)
{
	stage(14);
	if (!dev_units || !d_pr_req || P.hi == P.lo) return;   // (!d_pr_req: a single-end chunk of which only se_wave_kernel took reads)
	const int ends = pe ? 2 : 1;   // reads (and requests) per unit
	unsigned long long *small = (unsigned long long *)W.h_small[P.slot].ensure(512);
	P.dev.small_used = small; P.dev.small_cnt = small + 8;
	job_launch(P.dev, W.dev_job[P.slot], C.d_streams[P.slot], P, d_pr_req + (size_t)P.lo * ends, (size_t)(P.hi - P.lo) * ends, nullptr, true, nullptr,
	           const_cast<SamDesc *>(d_pr_desc));
}
void Call::finish_dev(Part &P)
{
	stage(15);
	job_fetch(P.dev, P, FETCH_IF_HANDED_BACK);
}
void Call::launch(Part &P)   // B (asynchronous)
{
	stage(16);
	if (!gpu_aln || P.n_req == 0) return;
	unsigned long long *small = (unsigned long long *)W.h_small[P.slot].ensure(512);
	P.host.small_cnt = small + 16; P.host.small_used = small + 24;
	// (gpu_sam: the records of the part's qualifying pairs, queued right behind their CIGARs)
	SamDesc *d_desc = gpu_sam ? (SamDesc *)W.sdesc.ensure((size_t)n * sizeof(SamDesc)) : nullptr;
	job_launch(P.host, W.host_job[P.slot], C.a_streams[P.slot], P, nullptr, P.n_req, P.base.data(), gpu_sam, sdesc, d_desc);
}
void Call::finish(Part &P)   // wait for B, fetch the pool
{
	stage(17);
	job_fetch(P.host, P, FETCH_ALWAYS);
	if (cpusec_on() && P.host.launched) {
		unsigned long long c[16];
		HIP_OK(hipMemcpy(c, P.host.d_cnt, sizeof c, hipMemcpyDeviceToHost));
		fprintf(stderr, "[aln lists] %zu requests: same-length %llu, narrow DP %llu, full DP %llu\n", P.host.n_req, c[8], c[9], c[10]);
	}
}

// ---- C: the records ----
// a finished record out of a job's arena: ownership passes to the caller, who free()s it
void Call::take_record(int read, const Job &J, int at)
{
	const int len = J.solen[at];
	char *sam = (char *)malloc((size_t)len + 1);
	if (!sam) die("out of memory");
	memcpy(sam, J.sarena + J.sooff[at], (size_t)len);
	sam[len] = 0;
	seqs[read].sam = sam;
}

// which: 0 = the records of the units decided on the device (as soon as their job is back: the copies run under the kernels
// of the other units), 1 = everything else, 2 = both
void Call::replay(Part &P, int which)
{
	stage(18);
	const double ta = now_ms(), ca = cpu_sec(), sa_ = sys_sec();
	const long pf = page_faults();
	const int ends = pe ? 2 : 1;
	// (a single-end chunk without reads of the device's has no pass 0)
	// per-block counters: a shared atomic bumped once per unit costs more than copying the unit's records
	if (pe || which != 0 || dev_units) parallel_blocks(n_thr, P.hi - P.lo, pe ? 128 : 256, [&](int, int, int k_lo, int k_hi) {
		unsigned long long n_dev = 0, n_se_xa_w = 0, n_se_supp_w = 0, n_pair_lines_w = 0, tsc = 0;
		for (int k = k_lo; k < k_hi; ++k) {
			const int i = P.lo + k, r = ends * i;   // the unit, its first read
			// pair_wave_kernel's pair with an XA tag, or se_wave_kernel's read (with or without one): the job of those
			const bool lines_k = pe && dev_units && ustat[i] == PW_DECIDED_LINES;   // pair_wave_kernel's pair reported end by end: the same job
			const bool xa_k = (dev_units && ustat[i] == PW_DECIDED_XA) || lines_k || (dev_se_wave && wave_dec[i]);
			const bool dev_k = xa_k || (dev_units && ustat[i] == PR_DECIDED);
			const bool own_k = xa_k || (dev_k && P.wave.launched && wave_dec[i]);   // pair_wave_kernel's pair with the job of its own
			const Job &J = xa_k ? P.xa : own_k ? P.wave : dev_k ? P.dev : P.host;
			bool written = J.solen != nullptr;   // every record of the unit was written by sam_emit_kernel
			for (int e = 0; e < ends && written; ++e) written = J.solen[ends * k + e] >= 0;
			const bool early = dev_k && written && !own_k;   // pass 0's units
			if (which != 2 && early != (which == 0)) continue;
			if (written) {
				const unsigned long long tq0 = cpusec_on() ? __builtin_ia32_rdtsc() : 0;
				for (int e = 0; e < ends; ++e) take_record(r + e, J, ends * k + e);
				if (!pe && ustat[i] == SE_DECIDED_XA) ++n_se_xa_w;   // (counted apart: n_sam_dev stays the plain records of n_se_dev)
				else if (!pe && ustat[i] == SE_DECIDED_LINES) ++n_se_supp_w;   // (its one string holds all the read's lines)
				else if (lines_k) ++n_pair_lines_w;   // (counted apart too: n_sam_dev stays what it is without the path)
				else n_dev += ends;
				if (cpusec_on()) tsc += __builtin_ia32_rdtsc() - tq0;
				continue;
			}
			AlnCtx ctx;
			if (gpu_aln) { ctx.mode = AlnCtx::REPLAY; ctx.hdr = P.host.hdr; ctx.pool = P.host.pool; ctx.cursor = P.base[k]; }
			// the device decided the unit but handed a record back: the host decides it again (the same `ends` requests, same order)
			if (dev_k) { ctx.hdr = J.hdr; ctx.pool = J.pool; ctx.cursor = (size_t)ends * k; }
			if (pe) {
				MswCtx mc;   // (pair_wave_kernel's pair: the rescue alignments are there)
				const bool has_msw = dev_k && dev_wave && (wave_dec[i] || xa_k) && P.msw_launched && P.mbase[k + 1] != P.mbase[k];
				if (has_msw) { mc.req = P.mreq + P.mbase[k]; mc.res = P.mres + P.mbase[k]; mc.n = (int)(P.mbase[k + 1] - P.mbase[k]); }
				if (dev_k) sam_pe_plan(opt, bns, pac, pes, (uint64_t)((n_processed >> 1) + i), &seqs[r], &regs[r], plans[i], has_msw ? &mc : nullptr, r);
				// (an XA pair handed back: the host lists the XA entries of every primary hit, in another order than the device's
				// requests, so it aligns the few such pairs itself)
				sam_pe_emit(opt, bns, pac, pes, &seqs[r], &regs[r], plans[i], gpu_aln && !xa_k ? &ctx : nullptr, r);
			} else {
				if (dev_k) mark_primary_se(opt, regs[i], n_processed + i);
				// (se_wave_kernel's read handed back: up to 1 + PW_XA_CAP requests in the device's order, so the host aligns it itself)
				reg2sam(opt, bns, pac, &seqs[i], regs[i], 0, 0, gpu_aln && !xa_k ? &ctx : nullptr, i);
			}
		}
		n_sam_dev += n_dev; n_se_xa_sam += n_se_xa_w; n_se_supp_sam += n_se_supp_w; n_pair_lines_sam += n_pair_lines_w; tsc_devcopy += tsc;
	});
	emit_ms += now_ms() - ta;
	cpu_emit += cpu_sec() - ca;
	sys_emit += sys_sec() - sa_; pf_emit += page_faults() - pf;
}

// ---- pairing decisions, then CIGAR/MD/NM on the GPU, then SAM text ----
// Per part of the chunk:  A  decisions + a COLLECT pass that records which regions need a global re-alignment
// (mem_reg2aln's DP);  B  aln_kernel does them all at once;  C  the same emission again (REPLAY) with the results
// plugged in.  Two parts are software-pipelined so that B of one part runs while the host does A / C of the other.
void Call::sam_stage()
{
	n_units = pe ? n >> 1 : n;
	plans.resize(pe ? n_units : 0);
	n_parts = (gpu_aln && n_units >= 20000 && n_sub > 1) ? 2 : 1;
	if (const char *e = getenv("MPIBWA_SAM_PARTS")) n_parts = std::max(1, std::min(2, atoi(e)));
	gpu_msw = pe && !(opt->flag & MEM_F_NO_RESCUE) && getenv("MPIBWA_HOST_MATESW") == nullptr && (int64_t)max_len * opt->a < 8192 &&
	          msw_lds_bytes(max_len) <= 160 * 1024 && msw_on_device(opt);
	// When does the device units' job go out?  Alone, right behind the pairing kernel (its kernels and the copies of its records run
	// under the host's work on the other pairs: 94.8-96.8 vs 98.7-102.8 ms per chunk); with other calls in flight, next to the host
	// pairs' job (their kernels fill the gaps anyway and an early launch only delays their seeding: 12.0-12.7 vs 10.9-11.3 Mreads/s).
	// MPIBWA_DEV_JOB_LATE=0/1 forces either.
	const char *dle = getenv("MPIBWA_DEV_JOB_LATE");
	const bool dev_late = dle ? atoi(dle) != 0 : crowded;
	// Single-end calls have no rescue listing to run the device job under: its records are fetched once the host's reads are planned
	// and their CIGAR job is out (dev_mid), so that the job runs under the planning and the copies of its records under that kernel.
	// Where the device job of a part is fetched (finish_dev + replay 0), relative to the host reads' CIGAR job (launch .. finish):
	//   dev_early  pairs, one call in flight     launch_dev, rescue listing, FETCH, collect, launch, finish          (as before)
	//   dev_last   pairs, other calls in flight  rescue listing, collect, launch_dev, launch, finish, FETCH          (as before)
	//   dev_mid    single-end, either            launch_dev (before or after collect, by dev_late), launch, FETCH, finish
	// Exactly one of the three holds; replay 1 (the host's records) closes every part.
	const bool dev_early = pe && !dev_late, dev_mid = !pe, dev_last = pe && dev_late;
	// pair_wave_kernel: wherever pair_simple_kernel ran and mate rescue runs on the device.  MPIBWA_HOST_RESCUE=1 turns it off.
	dev_wave = pe && dev_units && gpu_msw && getenv("MPIBWA_HOST_RESCUE") == nullptr;
	if (dev_wave) { wave_cand.assign(n_units, 0); wave_dec.assign(n_units, 0); }
	// its XA listing: wherever it runs and the tags fit the kernel's side array.  MPIBWA_HOST_XA=1 turns it off.
	dev_xa = dev_wave && gpu_sam && wave_pp.max_XA_hits <= PW_XA_CAP && getenv("MPIBWA_HOST_XA") == nullptr;
	// the pairs reported end by end: wherever it runs and the device writes records; on unless MPIBWA_HOST_PAIR_LINES is set
	// to something other than 0.  The XA listing of their lines goes with dev_xa.
	const char *hpl = getenv("MPIBWA_HOST_PAIR_LINES");
	dev_pair_lines = dev_wave && gpu_sam && !(hpl && atoi(hpl) != 0);
	for (int p = 0; p < n_parts; ++p) {   // (slot 0: the whole chunk or its first half)
		parts[p].slot = p;
		parts[p].lo = p ? n_units / 2 : 0;
		parts[p].hi = p == n_parts - 1 ? n_units : n_units / 2;
	}
	// single-end: se_wave_kernel on the reads se_simple_kernel left for long lists or an XA tag, before any job goes out (the host waits
	// for its status bytes: behind the CIGAR kernel of 300 000 reads that wait was 5 ms per chunk, on an idle device it is not seen) ...
	if (!pe) se_wave_decide();
	if (!dev_late)
		for (int p = 0; p < n_parts; ++p) launch_dev(parts[p]);
	// ... and the job of the reads it decided, behind the device job of the part on the same stream: both run under the host's planning
	// of the remaining reads
	if (dev_se_wave)
		for (int p = 0; p < n_parts; ++p) own_job_records(parts[p], 1, se_bufs(), se_work, se_wxcnt);
	for (int p = 0; p < n_parts; ++p) { mcollect(parts[p]); mlaunch(parts[p]); }
	for (int p = 0; p < n_parts; ++p) {   // (the mate-rescue kernels of all parts are running)
		Part &P = parts[p];
		if (dev_early) { finish_dev(P); replay(P, 0); }
		collect(P, 0); mfinish(P); collect(P, 1);
		// (the wave's pairs ride in the part's device job when it has not gone out yet, and get a job of their own behind it otherwise)
		if (dev_wave) wave_records(P, !dev_late);
		if (dev_xa || dev_pair_lines) own_job_records(P, 2, W.wave[P.slot], P.work, dev_xa ? P.wxcnt : nullptr);
		if (dev_late) launch_dev(P);
		launch(P);
	}
	for (int p = 0; p < n_parts; ++p) {
		Part &P = parts[p];
		if (dev_mid) { finish_dev(P); replay(P, 0); }
		finish(P);
		if (dev_last) { finish_dev(P); replay(P, 0); }
		job_fetch(P.wave, P, FETCH_IF_HANDED_BACK, true);
		job_fetch(P.xa, P, FETCH_RECORDS);
		if (n_parts == 1) hprof_report("decisions + request lists");
		replay(P, 1);
	}
	STAT.plan_ms = plan_ms; STAT.aln_ms = aln_wait_ms; STAT.msw_ms = msw_ms; STAT.emit_ms = emit_ms;
	STAT.n_sam_dev = n_sam_dev.load();
	report_decisions();
	STAT.plan_ms += pair_dev_ms;
}

// how many units the device decided, and (MPIBWA_CPUSEC) why the others went to the host
void Call::report_decisions()
{
	if (!ustat) return;
	uint64_t c[32] = {0};
	for (int k = 0; k < n_units; ++k) ++c[ustat[k] & 31];
	if (pe) {
		STAT.n_pair_dev = c[PR_DECIDED] - n_wave - n_xa_plain; STAT.n_pair_wave_dev = n_wave; STAT.n_pair_xa_dev = n_xa_pairs;
		STAT.n_pair_lines_dev = n_pair_lines; STAT.n_pair_lines_sam_dev = n_pair_lines_sam.load();
	}
	else {
		STAT.n_se_dev = c[SE_DECIDED]; STAT.n_se_wave_dev = n_se_wave; STAT.n_se_xa_dev = c[SE_DECIDED_XA]; STAT.n_se_xa_sam_dev = n_se_xa_sam.load();
		STAT.n_se_supp_dev = n_se_supp; STAT.n_se_supp_sam_dev = n_se_supp_sam.load();
		if (cpusec_on()) fprintf(stderr, "[se_kernel] %d reads: decided %llu; host: comment %llu, > %d hits %llu, patch %llu, length %llu, ALT %llu, second primary hit %llu, XA %llu; se_wave_kernel: handed %zu, decided plain %llu, decided with an XA tag %llu, XA records written %llu, list past %d %llu, tie %llu, decided with several lines %llu, their text written %llu\n",
		                      n_units, (unsigned long long)c[SE_DECIDED], (unsigned long long)c[SE_HOST_COMMENT], PR_MAXREG, (unsigned long long)c[SE_HOST_MAXREG],
		                      (unsigned long long)c[SE_HOST_PATCH], (unsigned long long)c[SE_HOST_LENGTH], (unsigned long long)c[SE_HOST_ALT],
		                      (unsigned long long)c[SE_HOST_SUPP], (unsigned long long)c[SE_HOST_XA], se_work.size(), (unsigned long long)n_se_wave,
		                      (unsigned long long)c[SE_DECIDED_XA], n_se_xa_sam.load(), PW_MAXREG, (unsigned long long)c[SE_HOST_FULL], (unsigned long long)c[SE_HOST_TIE],
		                      (unsigned long long)n_se_supp, n_se_supp_sam.load());
	}
	if (pe && cpusec_on()) fprintf(stderr, "[pair_kernel] %d pairs: decided %llu; host: no/unnamed hit %llu, > %d hits %llu, patch %llu, ALT/length %llu, rescue %llu, no proper pair %llu, score %llu, second primary hit %llu, XA %llu; pair_wave_kernel decided %llu of them and %llu with an XA tag, left: rescue result not on the device %llu, list past %d %llu, tie %llu; reported end by end: decided %llu, their text written %llu\n",
	                      n_units, (unsigned long long)c[PR_DECIDED], (unsigned long long)c[PR_HOST_NO_HIT], PR_MAXREG, (unsigned long long)c[PR_HOST_MAXREG],
	                      (unsigned long long)c[PR_HOST_PATCH], (unsigned long long)c[PR_HOST_LENGTH], (unsigned long long)c[PR_HOST_RESCUE], (unsigned long long)c[PR_HOST_NO_PAIR],
	                      (unsigned long long)c[PR_HOST_SCORE], (unsigned long long)c[PR_HOST_SUPP], (unsigned long long)c[PR_HOST_XA],
	                      (unsigned long long)n_wave, (unsigned long long)n_xa_pairs, (unsigned long long)c[PW_HOST_NO_RESULT], PW_MAXREG, (unsigned long long)c[PW_HOST_FULL], (unsigned long long)c[PW_HOST_TIE],
	                      (unsigned long long)n_pair_lines, n_pair_lines_sam.load());
}

} // namespace mbw
