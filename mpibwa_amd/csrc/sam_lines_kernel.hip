// sam_lines_kernel.hip — SAM text on the device for single-end reads whose record has several lines: a primary line and up to
// SE_LINES_CAP - 1 supplementary lines, as se_wave_kernel decides them (se_wave_kernel.hip: SE_DECIDED_LINES), and (the paired
// instantiation) for the pairs mem_sam_pe reports end by end through no_pairing: (src/bwamem_pair.c:371-392), as pair_wave_kernel decides
// them (pair_wave_kernel.hip: PW_DECIDED_LINES): 0 .. SE_LINES_CAP lines per end.
//
// Device counterpart of mem_aln2sam (src/bwamem.c:825-946, add_cigar :812-823) called for every entry of mem_reg2sam's list
// (src/bwamem.c:1039-1040) without a mate:
//   * lines behind the first print the clips of their CIGAR as H and cut SEQ and QUAL to the aligned part (:818-819, :875-878, :889-892),
//     unless MEM_F_SOFTCLIP;
//   * every line carries SA:Z: (:912-931) with the other lines as "rname,pos,strand,CIGAR,mapq,NM;" — the CIGAR as mem_reg2aln left it
//     (clips as S), the MAPQ after the cap of :1029;
//   * under MEM_F_NO_MULTI the lines behind the first print 0x100 for the reference's 0x10000 and are supplementary lines in every other
//     respect (the tests of :871 and :912 look at 0x100 before the translation of :846);
//   * tags in the order NM MD AS XS RG SA XA.
// The record of one line stays sam_emit_kernel's (sam_kernel.hip), which writes 98 % of a chunk; these reads are a per cent of it.
// The paired instantiation adds mem_aln2sam's mate (:830-840, :856-867, :908).  The mate of every line of end e is line 0 of the other
// end, or the unaligned record:
//   * an end without a line takes its mate's contig, position and strand (:835-836): flag 0x4 (and 0x10 | 0x20 with a reversed mate,
//     SEQ / QUAL reversed then), CIGAR *, RNEXT =, TLEN 0, no NM / MD, MC:Z: with the mate's CIGAR, AS:i:0 XS:i:0;
//   * a line whose mate is unaligned lends it its own contig, position and strand (:837-838; every supplementary line its own): flag
//     0x8 (and 0x20 on a reversed line), RNEXT =, PNEXT = POS, TLEN 0, no MC;
//   * two ends without a line: "* 0 0 * * 0 0", flags 0x4 | 0x8;
//   * MC:Z: prints the mate's CIGAR through add_cigar(opt, m, str, which): on a line behind the first, and not under MEM_F_SOFTCLIP,
//     the MATE's clips are printed as H (:818-819, :908);
//   * an end of one line carries no SA tag; tags in the order NM MD MC AS XS RG SA XA.
//
// A wavefront per read (per pair: lanes 0-3 take the lines of end 0, lanes 4-7 those of end 1; an end without a line has its record
// written by the first lane of its four).  A lane per line works out the line's alignment fields (sam_aln), prints its short fields into a row of
// LINES_ROW bytes in LDS and the numbers of the entry the OTHER lines' SA tags quote (",pos,strand,CIGAR,mapq,NM;") into a slot of
// SA_STAGE bytes, and adds up the line's length; the wave sums the lines, takes the read's place in the arena with one atomic and
// copies line after line across its lanes, 64 consecutive bytes per store.  XA entries go through the staging slots of sam_emit_kernel's
// scheme.  A read is handed back whole (out_len = -1) when aln_kernel declined one of its requests, a row, an SA slot or an XA slot
// is too small, or the arena is full.
//
// 3 456 B of LDS per wave (the paired instantiation: 5 888 B), no scratch; the register counts are in DESIGN §4.5e / §4.4e.
#include <hip/hip_runtime.h>
#include "sam_common.cuh"

namespace mbw {

#define LINES_ROW 512    // bytes of LDS per line for its short fields: FLAG POS MAPQ CIGAR * 0 0 [*] NM MD: AS XS RG:
#define SA_STAGE 96      // bytes of LDS per line for what the other lines' SA tags say of it behind its contig name

// the mate columns of a line without a mate (src/bwamem.c:867)
__device__ __forceinline__ void mate_columns_none(Sink &S) { S.lit("*\t0\t0\t"); }

// the line's own CIGAR (add_cigar): clips as `clip` (S, or H on a line behind the first)
__device__ __forceinline__ void line_cigar(Sink &S, const SamAln &a, char clip)
{
	if (a.clip5) { S.num32(a.clip5); S.ch(clip); }
	for (int k = a.skip_front; k < a.n_cigar - a.skip_back; ++k) {
		const uint32_t c = a.cig[k];
		S.num32(c >> 4);
		S.ch("MIDSH"[c & 0xf]);
	}
	if (a.clip3) { S.num32(a.clip3); S.ch(clip); }
}

// Unit u of the launch.
// !PE: read rd = list ? list[u] - r0 : u of the job's arrays (off, lens, name_off, out_off, out_len), n_lines[u] lines with their
// descriptors at ldesc[u * SE_LINES_CAP ..], its requests from req_base[u] (SamDesc::req relative to it; a line's XA requests follow
// its own).  n_lines[u] = 0 or req_base[u] < 0: not a unit of this job, nothing is read or written for it.
// PE: pair pr = list ? list[u] : u of the chunk, whose reads are rd = 2 pr - r0 + e of the job's arrays; n_lines[2u + e] lines of end e
// (0: the unaligned record) with their descriptors at ldesc[(2u + e) * SE_LINES_CAP ..], the pair's requests from req_base[u].  A unit
// is marked by req_base[u] >= 0 alone: a pair of two unaligned records has no request and is a unit all the same.  out_off / out_len
// are written per read, a read's string holds all its lines, and the pair is handed back whole (both out_len = -1).
template <bool PE>
__global__ void __launch_bounds__(64)
sam_lines_kernel(SamParams P, int soft, int n_units, const int *__restrict__ list, int r0, const uint8_t *__restrict__ n_lines, const SamDesc *__restrict__ ldesc,
                 const int *__restrict__ req_base, const AlnReq *__restrict__ reqs, const AlnHdr *__restrict__ hdr, const uint8_t *__restrict__ pool,
                 const uint8_t *__restrict__ seq, const int64_t *__restrict__ off, const int *__restrict__ lens, const uint8_t *__restrict__ qual,
                 const uint8_t *__restrict__ names, const int *__restrict__ name_off, const long long *__restrict__ ann_off,
                 const char *__restrict__ ann_names, const int *__restrict__ ann_name_off, uint8_t *__restrict__ arena, unsigned long long arena_bytes,
                 unsigned long long *arena_used, unsigned long long *out_off, int *out_len)
{
	constexpr int LANES = (PE ? 2 : 1) * SE_LINES_CAP;   // the lanes with a line: slot u * LANES + lane of ldesc
	__shared__ uint8_t rows[LANES * LINES_ROW];
	__shared__ uint8_t sa_rows[LANES * SA_STAGE];
	__shared__ uint8_t xa_rows[(SAM_XA_MASK + 1) * XA_STAGE];
	const int lane = threadIdx.x;
	const int e = PE ? lane / SE_LINES_CAP & 1 : 0;   // the lane's end
	// what is the same for all lines of a read is uniform without a mate and the lane's own with one
	auto of_line = [&](auto v, int i) { if constexpr (PE) return bcast(v, i); else return v; };
	for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
		int nl = n_lines[PE ? 2 * u + e : u], nl_mate = 0;   // the lines of the lane's end, of the other end
		if (nl > SE_LINES_CAP) nl = SE_LINES_CAP;
		const int base = req_base[u];
		if ((!PE && nl <= 0) || base < 0) continue;
		int rd;
		if constexpr (PE) {
			rd = 2 * (list ? list[u] : u) - r0 + e;
			nl_mate = n_lines[2 * u + (e ^ 1)];
			if (nl_mate > SE_LINES_CAP) nl_mate = SE_LINES_CAP;
		} else rd = list ? list[u] - r0 : u;
		const int lq = lens[rd];
		const int name_at = name_off[rd], name_len = name_off[rd + 1] - name_at;
		const long long sq_at = off[rd];
		// the lane has a line to write: one of the end's lines, or (PE) the unaligned record of an end without a line
		const bool active = PE ? lane < LANES && lane % SE_LINES_CAP < (nl ? nl : 1) : lane < nl;
		const bool has_sa = !PE || nl > 1;   // (:912-915: an SA tag when the list holds other lines)
		// ---- phase 1: a lane per line ----
		bool fits = true;
		int total = 0;                   // bytes of the line
		int e_a = 0, e_m = 0, e_b = 0, e_c = 0;   // ends of the pieces in the row; the row ends at row_len
		int row_len = 0, rn_at = 0, rn_len = 0, mn_at = 0, mn_len = 0, sa_len = 0, is_rev = 0, md_len = 0, cut5 = 0, n_seq = 0, n_xa = 0, xa_len = 0;
		const uint8_t *md = nullptr;
		SamDesc D;
		if (active) {
			SamAln m;   // (PE) the mate: line 0 of the other end, when that end has a line
			int n_m = 0;
			bool m_ok = true;
			if constexpr (PE)
				if (nl_mate) {
					m = sam_aln(ldesc[(size_t)u * LANES + (e ^ 1) * SE_LINES_CAP], hdr, pool, base, P.l_pac, ann_off, lens[rd + 1 - 2 * e]);
					n_m = m.n_cigar - m.skip_front - m.skip_back + (m.clip5 ? 1 : 0) + (m.clip3 ? 1 : 0);
					m_ok = m.ok;
				}
			Sink S;
			S.row = rows + lane * LINES_ROW; S.len = 0; S.cap = LINES_ROW;
			if (PE && nl == 0) {   // the unaligned record (src/bwamem.c:1033-1037) with its mate's coordinate (:835-836), or without any
				fits = m_ok;
				if (m_ok) {
					S.ch('\t'); S.num32((uint32_t)(0x40 << e | 0x5 | (nl_mate ? (m.is_rev ? 0x30 : 0) : 0x8))); S.ch('\t');
					e_a = S.len;
					if (nl_mate) {
						rn_at = ann_name_off[m.rid]; rn_len = ann_name_off[m.rid + 1] - rn_at;
						S.ch('\t'); S.num(m.pos + 1); S.lit("\t0\t*\t=\t"); S.num(m.pos + 1); S.lit("\t0\t");
						is_rev = m.is_rev;
					} else S.lit("*\t0\t0\t*\t*\t0\t0\t");
					e_m = e_b = S.len;
					if (!P.has_qual) S.ch('*');
					e_c = S.len;
					if (n_m) { S.lit("\tMC:Z:"); line_cigar(S, m, 'S'); }
					S.lit("\tAS:i:0\tXS:i:0");
					if (P.rg_len) S.lit("\tRG:Z:");
					row_len = S.len;
					n_seq = lq;
					fits = row_len <= LINES_ROW;
				}
			} else {
				D = ldesc[(size_t)u * LANES + lane];
				const SamAln p = sam_aln(D, hdr, pool, base, P.l_pac, ann_off, lq);
				fits = p.ok && m_ok;
				if (fits) {
					const bool supp = lane % SE_LINES_CAP > 0;
					const bool hard = supp && !soft;
					const int n_p = p.n_cigar - p.skip_front - p.skip_back + (p.clip5 ? 1 : 0) + (p.clip3 ? 1 : 0);
					int flag = (D.flag & 0xffff) | (p.is_rev ? 0x10 : 0);
					if constexpr (PE) flag |= 0x1 | (nl_mate ? (m.is_rev ? 0x20 : 0) : 0x8 | (p.is_rev ? 0x20 : 0));   // (:837-838: an unaligned mate copies the line)
					rn_at = ann_name_off[p.rid]; rn_len = ann_name_off[p.rid + 1] - rn_at;
					S.ch('\t'); S.num32((uint32_t)flag); S.ch('\t');
					e_a = S.len;
					S.ch('\t'); S.num(p.pos + 1); S.ch('\t'); S.num32((uint32_t)D.mapq); S.ch('\t');
					if (n_p) line_cigar(S, p, hard ? 'H' : 'S'); else S.ch('*');
					S.ch('\t');
					if constexpr (PE) {   // RNEXT PNEXT TLEN (:856-867)
						const bool same = !nl_mate || p.rid == m.rid;
						if (same) S.ch('=');
						else { mn_at = ann_name_off[m.rid]; mn_len = ann_name_off[m.rid + 1] - mn_at; }
						e_m = S.len;
						S.ch('\t'); S.num((nl_mate ? m.pos : p.pos) + 1); S.ch('\t');
						if (nl_mate && same) sam_tlen(S, p, n_p, m, n_m);
						else S.ch('0');
						S.ch('\t');
					} else mate_columns_none(S);
					e_b = S.len;
					if (!P.has_qual) S.ch('*');
					if (n_p) {
						S.lit("\tNM:i:"); S.num32((uint32_t)p.NM);
						S.lit("\tMD:Z:");
						md = p.md; md_len = p.md_len;
					}
					e_c = S.len;
					if (PE && n_m) { S.lit("\tMC:Z:"); line_cigar(S, m, hard ? 'H' : 'S'); }   // (:908: add_cigar with the LINE's `which`)
					if (D.score >= 0) { S.lit("\tAS:i:"); S.num32((uint32_t)D.score); }
					if (D.sub >= 0) { S.lit("\tXS:i:"); S.num32((uint32_t)D.sub); }
					if (P.rg_len) S.lit("\tRG:Z:");
					row_len = S.len;
					if (has_sa) {   // what the other lines say of this one
						Sink A;
						A.row = sa_rows + lane * SA_STAGE; A.len = 0; A.cap = SA_STAGE;
						A.ch(','); A.num(p.pos + 1); A.ch(','); A.ch(p.is_rev ? '-' : '+'); A.ch(',');
						A.cigar(p);
						A.ch(','); A.num32((uint32_t)D.mapq); A.ch(','); A.num32((uint32_t)p.NM); A.ch(';');
						sa_len = A.len;
					}
					is_rev = p.is_rev;
					cut5 = hard && n_p ? p.clip5 : 0;
					n_seq = lq - cut5 - (hard && n_p ? p.clip3 : 0);
					// the XA tag, counted here as sam_emit_kernel counts it
					bool xa_ok = true;
					n_xa = D.flag >> SAM_XA_SHIFT & SAM_XA_MASK;
					if (n_xa) xa_len = 6;
					for (int j = 0; j < n_xa && xa_ok; ++j) {
						const SamAln x = xa_aln(D, j, reqs, hdr, pool, base, P.l_pac, ann_off, lq);
						Sink C;
						C.row = nullptr; C.len = 0; C.cap = 0;
						xa_numbers(C, x);
						xa_ok = x.ok && C.len <= XA_STAGE;
						xa_len += ann_name_off[x.rid + 1] - ann_name_off[x.rid] + C.len;
					}
					fits = row_len <= LINES_ROW && sa_len <= SA_STAGE && xa_ok;
				}
			}
		}
		const bool whole = __ballot(!fits) == 0;
		// every line's SA tag lists all the lines of its read but itself (the four lanes of an end are neighbours)
		const int sa_mine = has_sa && active ? rn_len + sa_len : 0;
		int sa_all = sa_mine;
		for (int d = 1; d < SE_LINES_CAP; d <<= 1) sa_all += __shfl_xor(sa_all, d);
		if (active)   // QNAME a RNAME [m mate's RNAME] b SEQ \t [QUAL] c MD rest RG [\tSA:Z: entries] [XA] \n
			total = name_len + row_len + rn_len + mn_len + n_seq + 1 + (P.has_qual ? n_seq : 0) + md_len + P.rg_len + (has_sa ? 6 + sa_all - sa_mine : 0) + xa_len + 1;
		int incl = total;
		for (int d = 1; d < LANES; d <<= 1) {
			const int up = __shfl_up(incl, d);
			if (lane >= d) incl += up;
		}
		const int read_total = whole ? __shfl(incl, LANES - 1) : 0;   // (PE: of the pair)
		unsigned long long at0 = 0;
		if (lane == 0 && read_total) at0 = atomicAdd(arena_used, (unsigned long long)read_total);
		at0 = bcast(at0, 0);
		const bool room = read_total > 0 && at0 + (unsigned long long)read_total <= arena_bytes;
		if constexpr (PE) {
			const int first = __shfl(incl, SE_LINES_CAP - 1);   // the bytes of end 0
			if (lane < 2) {
				const int r = rd - e + lane;
				out_len[r] = room ? (lane ? read_total - first : first) : -1;
				if (room) out_off[r] = at0 + (lane ? first : 0);
			}
		} else if (lane == 0) {
			out_len[rd] = room ? read_total : -1;
			if (room) out_off[rd] = at0;
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the rows are read across the lanes from here on
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		if (room) {
			// ---- phase 2: the wave copies the lines out, one after the other ----
			uint8_t *o = arena + at0;
			auto spread = [&](int n, auto f) {
				for (int k = lane; k < n; k += 64) o[k] = (uint8_t)f(k);
				o += n;
			};
			for (unsigned long long todo = __ballot(active); todo; todo &= todo - 1) {
				const int i = __builtin_ctzll(todo);
				const uint8_t *row = rows + i * LINES_ROW;
				const int ea = bcast(e_a, i), eb = bcast(e_b, i), ec = bcast(e_c, i), rl = bcast(row_len, i);
				const int rev = bcast(is_rev, i), c5 = bcast(cut5, i), ns = bcast(n_seq, i);
				const int lqi = of_line(lq, i);
				const long long so = of_line(sq_at, i);
				{ const uint8_t *nm = names + of_line(name_at, i); spread(of_line(name_len, i), [&](int k) { return nm[k]; }); }
				spread(ea, [&](int k) { return row[k]; });
				{ const char *cn = ann_names + bcast(rn_at, i); spread(bcast(rn_len, i), [&](int k) { return cn[k]; }); }
				if constexpr (PE) {
					const int em = bcast(e_m, i);
					spread(em - ea, [&](int k) { return row[ea + k]; });
					{ const char *cn = ann_names + bcast(mn_at, i); spread(bcast(mn_len, i), [&](int k) { return cn[k]; }); }
					spread(eb - em, [&](int k) { return row[em + k]; });
				} else spread(eb - ea, [&](int k) { return row[ea + k]; });
				{
					const uint8_t *sq = seq + so;
					if (!rev) spread(ns, [&](int k) { const int c = sq[c5 + k]; return "ACGTN"[c > 4 ? 4 : c]; });
					else spread(ns, [&](int k) { const int c = sq[lqi - 1 - c5 - k]; return "TGCAN"[c > 4 ? 4 : c]; });
				}
				spread(1, [&](int) { return '\t'; });
				if (P.has_qual) {
					const uint8_t *ql = qual + so;
					if (!rev) spread(ns, [&](int k) { return ql[c5 + k]; });
					else spread(ns, [&](int k) { return ql[lqi - 1 - c5 - k]; });
				}
				spread(ec - eb, [&](int k) { return row[eb + k]; });
				{ const uint8_t *mdp = bcast(md, i); spread(bcast(md_len, i), [&](int k) { return mdp[k]; }); }
				spread(rl - ec, [&](int k) { return row[ec + k]; });
				const int nli = of_line(nl, i);
				if (!PE || nli > 1) {
					spread(P.rg_len + 6, [&](int k) { return k < P.rg_len ? P.rg[k] : "\tSA:Z:"[k - P.rg_len]; });
					const int j0 = PE ? i / SE_LINES_CAP * SE_LINES_CAP : 0;   // the first line of the read
					for (int j = j0; j < j0 + nli; ++j) {
						const int at = bcast(rn_at, j), nlen = bcast(rn_len, j), slen = bcast(sa_len, j);
						if (j == i) continue;
						const char *cn = ann_names + at;
						spread(nlen, [&](int k) { return cn[k]; });
						const uint8_t *sr = sa_rows + j * SA_STAGE;
						spread(slen, [&](int k) { return sr[k]; });
					}
				} else spread(P.rg_len, [&](int k) { return P.rg[k]; });
				const int nx = bcast(n_xa, i);
				if (nx) {   // a lane per entry prints its numbers, the wave copies (as in sam_emit_kernel)
					spread(6, [&](int k) { return "\tXA:Z:"[k]; });
					const SamDesc Di = ldesc[(size_t)u * LANES + i];
					int x_len = 0, x_at = 0, x_nlen = 0;
					if (lane < nx) {
						const SamAln x = xa_aln(Di, lane, reqs, hdr, pool, base, P.l_pac, ann_off, lqi);
						Sink T;
						T.row = xa_rows + lane * XA_STAGE; T.len = 0; T.cap = XA_STAGE;
						xa_numbers(T, x);
						x_len = T.len; x_at = ann_name_off[x.rid]; x_nlen = ann_name_off[x.rid + 1] - x_at;
					}
					__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
					__builtin_amdgcn_wave_barrier();
					__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
					for (int j = 0; j < nx; ++j) {
						const char *cn = ann_names + bcast(x_at, j);
						spread(bcast(x_nlen, j), [&](int k) { return cn[k]; });
						const uint8_t *xr = xa_rows + j * XA_STAGE;
						spread(bcast(x_len, j), [&](int k) { return xr[k]; });
					}
					__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the staging slots are rewritten for the next line with a tag
					__builtin_amdgcn_wave_barrier();
					__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
				}
				spread(1, [&](int) { return '\n'; });
			}
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the rows are rewritten by the wave's next read
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
}

int sam_lines_row(void) { return LINES_ROW; }
int sam_lines_sa_stage(void) { return SA_STAGE; }

void launch_sam_lines(void *stream, const SamParams &P, bool softclip, int n_units, const int *d_list, int r0, const uint8_t *d_n_lines, const SamDesc *d_ldesc,
                      const int *d_req_base, const AlnReq *d_req, const AlnHdr *d_hdr, const uint8_t *d_pool, const uint8_t *d_seq, const int64_t *d_off,
                      const int *d_len, const uint8_t *d_qual, const uint8_t *d_names, const int *d_name_off, const int64_t *d_ann_off,
                      const char *d_ann_names, const int *d_ann_name_off, uint8_t *d_arena, size_t arena_bytes, unsigned long long *d_arena_used,
                      unsigned long long *d_out_off, int *d_out_len, int grid_blocks, bool pe)
{
	if (n_units <= 0) return;
	int blocks = n_units < 256 * 16 ? n_units : 256 * 16;
	if (grid_blocks > 0 && grid_blocks < blocks) blocks = grid_blocks;
	hipLaunchKernelGGL(pe ? sam_lines_kernel<true> : sam_lines_kernel<false>, dim3(blocks), dim3(64), 0, (hipStream_t)stream, P, softclip ? 1 : 0, n_units, d_list, r0,
	                   d_n_lines, d_ldesc, d_req_base, d_req, d_hdr, d_pool, d_seq, d_off, d_len, d_qual, d_names, d_name_off, (const long long *)d_ann_off, d_ann_names,
	                   d_ann_name_off, d_arena, (unsigned long long)arena_bytes, d_arena_used, d_out_off, d_out_len);
}

} // namespace mbw
