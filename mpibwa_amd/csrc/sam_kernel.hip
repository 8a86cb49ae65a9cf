// sam_kernel.hip — SAM text on the device for the records of confidently paired reads and of single-end reads with one record.
//
// Device counterpart of the tail of mem_reg2aln (src/bwamem.c:1123-1157: position, strand, squeeze of a leading /
// trailing deletion, soft clips) and of mem_aln2sam (src/bwamem.c:825-946) for the case that makes up the bulk of a
// chunk: a pair that mem_sam_pe reports through its "paired" branch (src/bwamem_pair.c:315-345) with ONE line per read —
// no supplementary / ALT line, no pa tag, no comment, no XR; an XA tag when the descriptor lists its entries (mem_gen_alt,
// src/bwamem_extra.c:115-131, for pair_wave_kernel's pairs) — and (round 3) the two records of a pair without any hit.  Everything else (unpaired ends, supplementary
// lines, other XA, -a, -C, -V) stays with the host's formatter (host_regs.cpp: aln2sam) — but for the single-end reads with
// supplementary lines, which sam_lines_kernel.hip writes with what the two kernels share in sam_common.cuh —, and the host takes
// a pair back whenever the device flags one of its reads (CIGAR computed by the host, record longer than the staging
// buffer).  The host decides WHICH records are written here and all their numbers that involve floating point
// (MAPQ); the kernel turns numbers into bytes.  The single-end instantiation (sam_emit_kernel<false>) writes the one record of a
// read that mem_reg2sam (src/bwamem.c:1003-1049) reports with one line, from the descriptors of se_simple_kernel (se_kernel.hip).
//
// One wavefront per 64 reads, in two phases.
//   1. a lane per read: the lane works out its record's alignment fields (sam_aln) and prints the short fields — FLAG, POS,
//      MAPQ, CIGAR, PNEXT, TLEN and the tags' numbers — into its own scratch row in LDS, as four "pieces" of text, and adds
//      up the record's length.  A wave prefix sum of the lengths and ONE atomic on the arena cursor place the 64 records
//      back to back (an atomic per record, 1.3 M on one address, cost more than the rest of the kernel).
//   2. the wave walks its records and copies each out across the lanes: QNAME, piece, RNAME, piece, SEQ, QUAL, piece, MD,
//      piece, RG — 64 consecutive bytes per store.
// The XA tag does not pass through the row (five entries are 140 bytes: with the short fields they would outgrow it).  Phase 1 adds up
// its length, entry by entry, without storing a byte; phase 2 writes it behind the read group: a lane per entry prints ",±pos,CIGAR,NM;"
// into a staging slot of XA_STAGE bytes in LDS, then the wave copies contig name and slot, entry after entry, into the arena.
#include <hip/hip_runtime.h>
#include "sam_common.cuh"

namespace mbw {

// PE: the records of pairs (a unit of req_base is a pair, reads 2k and 2k + 1 describe each other's RNEXT / PNEXT / TLEN / MC and go
// back to the host together); !PE: single-end records (a unit is a read, "*\t0\t0" for the mate columns, a read goes back alone)
template <bool PE>
__global__ void __launch_bounds__(64)
sam_emit_kernel(SamParams P, int n_reads, const SamDesc *__restrict__ desc, const int *__restrict__ req_base, const AlnReq *__restrict__ reqs,
                const AlnHdr *__restrict__ hdr,
                const uint8_t *__restrict__ pool, const uint8_t *__restrict__ seq, const int64_t *__restrict__ off, const int *__restrict__ lens,
                const uint8_t *__restrict__ qual, const uint8_t *__restrict__ names, const int *__restrict__ name_off,
                const long long *__restrict__ ann_off, const char *__restrict__ ann_names, const int *__restrict__ ann_name_off,
                uint8_t *__restrict__ arena, unsigned long long arena_bytes, unsigned long long *arena_used, unsigned long long *out_off, int *out_len)
{
	__shared__ uint8_t rows[64 * SAM_ROW];
	__shared__ uint8_t xa_rows[(SAM_XA_MASK + 1) * XA_STAGE];
	const int lane = threadIdx.x;
	const int n_batch = (n_reads + 63) >> 6;
	for (int bt = blockIdx.x; bt < n_batch; bt += gridDim.x) {
		const int r = (bt << 6) + lane;
		// ---- phase 1: a lane per read ----
		int status = -2;                 // out_len of a read without a device record
		int total = 0;                   // bytes of the record
		int e_a = 0, e_b = 0, e_c = 0, e_d = 0;   // ends of the four pieces in the row
		int name_at = 0, name_len = 0, rn_at = 0, rn_len = 0, mn_at = 0, mn_len = 0, lq = 0, is_rev = 0, md_len = 0;
		int n_xa = 0, xa_len = 0;        // entries and bytes of the XA tag
		long long sq_at = 0;
		const uint8_t *md = nullptr;
		if (r < n_reads) {
			const SamDesc D = desc[r];
			if (D.req == -3) {   // a read without any hit (of a pair, or a single-end read): "QNAME FLAG * 0 0 * * 0 0 SEQ QUAL AS:i:0 XS:i:0 [RG]" (src/bwamem.c:853-858, 928-929)
				lq = lens[r];
				Sink S;
				S.row = rows + lane * SAM_ROW; S.len = 0;
				name_at = name_off[r]; name_len = name_off[r + 1] - name_at;
				S.ch('\t'); S.num32((uint32_t)(D.flag & 0xffff)); S.ch('\t');
				e_a = S.len;
				S.lit("*\t0\t0\t*\t");
				e_b = S.len;
				S.lit("*\t0\t0\t");
				e_c = S.len;
				if (!P.has_qual) S.ch('*');
				e_d = S.len;
				S.lit("\tAS:i:0\tXS:i:0");
				if (P.rg_len) S.lit("\tRG:Z:");
				is_rev = 0; sq_at = off[r];
				total = name_len + S.len + lq + 1 + (P.has_qual ? lq : 0) + P.rg_len + 1;
				status = total;
			} else if (D.req >= 0) {   // mem_aln2sam; !PE: without a mate (src/bwamem.c:867: "*\t0\t0"; no MC)
				const int unit = PE ? r >> 1 : r;
				lq = lens[r];
				const SamAln p = sam_aln(D, hdr, pool, req_base[unit], P.l_pac, ann_off, lq);
				SamAln m = p;            // (PE: the mate's line; !PE: never read)
				if constexpr (PE) m = sam_aln(desc[r ^ 1], hdr, pool, req_base[unit], P.l_pac, ann_off, lens[r ^ 1]);
				status = -1;             // a CIGAR the device declined, or a row that overflows: the host formats the pair (the read)
				if (p.ok && m.ok) {
					Sink S;
					S.row = rows + lane * SAM_ROW; S.len = 0;
					const int flag = (D.flag & 0xffff) | (PE ? 0x1 : 0) | (p.is_rev ? 0x10 : 0) | (PE && m.is_rev ? 0x20 : 0);
					const int n_p = p.n_cigar - p.skip_front - p.skip_back + (p.clip5 ? 1 : 0) + (p.clip3 ? 1 : 0);
					const int n_m = m.n_cigar - m.skip_front - m.skip_back + (m.clip5 ? 1 : 0) + (m.clip3 ? 1 : 0);
					name_at = name_off[r]; name_len = name_off[r + 1] - name_at;
					rn_at = ann_name_off[p.rid]; rn_len = ann_name_off[p.rid + 1] - rn_at;
					S.ch('\t'); S.num32(flag); S.ch('\t');
					e_a = S.len;
					S.ch('\t'); S.num(p.pos + 1); S.ch('\t'); S.num32(D.mapq); S.ch('\t');
					if (n_p) S.cigar(p); else S.ch('*');
					S.ch('\t');
					if constexpr (PE) {
						if (p.rid == m.rid) S.ch('=');
						else { mn_at = ann_name_off[m.rid]; mn_len = ann_name_off[m.rid + 1] - mn_at; }
						e_b = S.len;
						S.ch('\t'); S.num(m.pos + 1); S.ch('\t');
						if (p.rid == m.rid) sam_tlen(S, p, n_p, m, n_m);
						else S.ch('0');
						S.ch('\t');
					} else {
						S.ch('*');
						e_b = S.len;
						S.lit("\t0\t0\t");
					}
					e_c = S.len;
					if (!P.has_qual) S.ch('*');   // (which = 0: SEQ and QUAL are never trimmed)
					if (n_p) {
						S.lit("\tNM:i:"); S.num32(p.NM);
						S.lit("\tMD:Z:");
						md = p.md; md_len = p.md_len;
					}
					e_d = S.len;
					if (PE && n_m) { S.lit("\tMC:Z:"); S.cigar(m); }
					if (D.score >= 0) { S.lit("\tAS:i:"); S.num32(D.score); }
					if (D.sub >= 0) { S.lit("\tXS:i:"); S.num32(D.sub); }
					if (P.rg_len) S.lit("\tRG:Z:");
					is_rev = p.is_rev; sq_at = off[r];
					// the XA tag: "\tXA:Z:" and per entry "name,±pos,CIGAR,NM;", counted here; a declined CIGAR among them and the pair is the host's
					bool xa_ok = true;
					n_xa = reqs ? D.flag >> SAM_XA_SHIFT & SAM_XA_MASK : 0;
					if (n_xa) xa_len = 6;
					for (int j = 0; j < n_xa && xa_ok; ++j) {
						const SamAln x = xa_aln(D, j, reqs, hdr, pool, req_base[unit], P.l_pac, ann_off, lq);
						Sink C;
						C.row = nullptr; C.len = 0; C.cap = 0;
						xa_numbers(C, x);
						xa_ok = x.ok && C.len <= XA_STAGE;
						xa_len += ann_name_off[x.rid + 1] - ann_name_off[x.rid] + C.len;
					}
					if (S.len <= SAM_ROW && xa_ok) {
						// QNAME a RNAME b [mate RNAME] c SEQ \t [QUAL] d MD rest RG [XA] \n
						total = name_len + S.len + rn_len + mn_len + lq + 1 + (P.has_qual ? lq : 0) + md_len + P.rg_len + xa_len + 1;
						status = total;
					}
				}
			}
		}
		// PE: a pair goes back as a whole: the two rows of a pair need not overflow together (other POS, TLEN sign, NM), and the host
		// formats both records as soon as one is missing (reads 2k and 2k + 1 are neighbouring lanes).  !PE: a read goes back alone.
		if (PE && __shfl_xor(status, 1) == -1 && status >= 0) { status = -1; total = 0; }
		// place the wave's records back to back: exclusive prefix sum of the lengths, one atomic
		int incl = total;
		for (int d = 1; d < 64; d <<= 1) {
			const int up = __shfl_up(incl, d);
			if (lane >= d) incl += up;
		}
		const int wave_total = __shfl(incl, 63);
		unsigned long long base = 0;
		if (lane == 0 && wave_total) base = atomicAdd(arena_used, (unsigned long long)wave_total);
		base = bcast(base, 0);
		if (base + (unsigned long long)wave_total > arena_bytes) { if (total) { status = -1; total = 0; } }   // (the host sizes the arena for every record)
		const unsigned long long at_mine = base + (unsigned long long)(incl - total);
		if (r < n_reads) { out_len[r] = status; if (total) out_off[r] = at_mine; }
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the rows are read across the lanes from here on
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		// ---- phase 2: the wave copies the records out, one after the other ----
		unsigned long long todo = __ballot(total > 0);
		while (todo) {
			const int i = __builtin_ctzll(todo);
			todo &= todo - 1;
			uint8_t *o = arena + bcast(at_mine, i);
			const uint8_t *row = rows + i * SAM_ROW;
			const int ea = bcast(e_a, i), eb = bcast(e_b, i), ec = bcast(e_c, i), ed = bcast(e_d, i);
			const int l = bcast(lq, i), rev = bcast(is_rev, i);
			auto spread = [&](int n, auto f) {
				for (int k = lane; k < n; k += 64) o[k] = (uint8_t)f(k);
				o += n;
			};
			{ const uint8_t *nm = names + bcast(name_at, i); spread(bcast(name_len, i), [&](int k) { return nm[k]; }); }
			spread(ea, [&](int k) { return row[k]; });
			{ const char *cn = ann_names + bcast(rn_at, i); spread(bcast(rn_len, i), [&](int k) { return cn[k]; }); }
			spread(eb - ea, [&](int k) { return row[ea + k]; });
			{ const char *cn = ann_names + bcast(mn_at, i); spread(bcast(mn_len, i), [&](int k) { return cn[k]; }); }
			spread(ec - eb, [&](int k) { return row[eb + k]; });
			const long long so = bcast(sq_at, i);
			{
				const uint8_t *sq = seq + so;
				if (!rev) spread(l, [&](int k) { return "ACGTN"[sq[k] > 4 ? 4 : sq[k]]; });
				else spread(l, [&](int k) { const int c = sq[l - 1 - k]; return "TGCAN"[c > 4 ? 4 : c]; });
			}
			spread(1, [&](int) { return '\t'; });
			if (P.has_qual) {
				const uint8_t *ql = qual + so;
				if (!rev) spread(l, [&](int k) { return ql[k]; });
				else spread(l, [&](int k) { return ql[l - 1 - k]; });
			}
			spread(ed - ec, [&](int k) { return row[ec + k]; });
			{ const uint8_t *mdp = bcast(md, i); spread(bcast(md_len, i), [&](int k) { return mdp[k]; }); }
			const int nx = bcast(n_xa, i);
			const int rest = bcast(status, i) - (int)(o - (arena + bcast(at_mine, i))) - P.rg_len - bcast(xa_len, i) - 1;   // what is left of the row
			spread(rest, [&](int k) { return row[ed + k]; });
			if (nx == 0) { spread(P.rg_len + 1, [&](int k) { return k < P.rg_len ? P.rg[k] : '\n'; }); continue; }
			// ---- the XA tag (src/bwamem.c:940 puts it behind RG / SA / pa): a lane per entry prints its numbers, the wave copies ----
			spread(P.rg_len + 6, [&](int k) { return k < P.rg_len ? P.rg[k] : "\tXA:Z:"[k - P.rg_len]; });
			const int ri = (bt << 6) + i;   // (wave-uniform: every lane reads the record's descriptor)
			int x_len = 0, x_at = 0, x_nlen = 0;
			if (lane < nx) {
				const SamAln x = xa_aln(desc[ri], lane, reqs, hdr, pool, req_base[PE ? ri >> 1 : ri], P.l_pac, ann_off, l);
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
			spread(1, [&](int) { return '\n'; });
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the staging slots are rewritten for the wave's next record with a tag
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the rows are rewritten by the wave's next batch
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
}

// Room for the records of n_reads reads: SEQ + QUAL + 320 bytes for everything else, and a megabyte.  Names, contig names, MD
// and a read group can add up to more; a wave whose records do not fit any more hands them back to the host (status -1).
size_t sam_arena_bytes(int n_reads, int max_len)
{
	return (size_t)n_reads * (size_t)(2 * max_len + 320) + (1 << 20);
}

template <bool PE>
static void launch_sam_emit_t(void *stream, const SamParams &P, int n_reads, const SamDesc *d_desc, const int *d_req_base, const AlnReq *d_req, const AlnHdr *d_hdr,
                     const uint8_t *d_pool, const uint8_t *d_seq, const int64_t *d_off, const int *d_len, const uint8_t *d_qual,
                     const uint8_t *d_names, const int *d_name_off, const int64_t *d_ann_off, const char *d_ann_names, const int *d_ann_name_off,
                     uint8_t *d_arena, size_t arena_bytes, unsigned long long *d_arena_used, unsigned long long *d_out_off, int *d_out_len,
                     int grid_blocks)
{
	if (n_reads <= 0) return;
	const int n_batch = (n_reads + 63) >> 6;
	int blocks = n_batch < 256 * 8 ? n_batch : 256 * 8;   // 17.7 KB of LDS per wave: nine waves per CU
	if (grid_blocks > 0 && grid_blocks < blocks) blocks = grid_blocks;
	hipLaunchKernelGGL(sam_emit_kernel<PE>, dim3(blocks), dim3(64), 0, (hipStream_t)stream, P, n_reads, d_desc, d_req_base, d_req, d_hdr, d_pool, d_seq, d_off,
	                   d_len, d_qual, d_names, d_name_off, (const long long *)d_ann_off, d_ann_names, d_ann_name_off, d_arena,
	                   (unsigned long long)arena_bytes, d_arena_used, d_out_off, d_out_len);
}

#define SAM_EMIT_ARGS stream, P, n_reads, d_desc, d_req_base, d_req, d_hdr, d_pool, d_seq, d_off, d_len, d_qual, d_names, d_name_off, d_ann_off, d_ann_names, \
	d_ann_name_off, d_arena, arena_bytes, d_arena_used, d_out_off, d_out_len, grid_blocks
void launch_sam_emit(void *stream, const SamParams &P, int n_reads, const SamDesc *d_desc, const int *d_req_base, const AlnReq *d_req, const AlnHdr *d_hdr,
                     const uint8_t *d_pool, const uint8_t *d_seq, const int64_t *d_off, const int *d_len, const uint8_t *d_qual,
                     const uint8_t *d_names, const int *d_name_off, const int64_t *d_ann_off, const char *d_ann_names, const int *d_ann_name_off,
                     uint8_t *d_arena, size_t arena_bytes, unsigned long long *d_arena_used, unsigned long long *d_out_off, int *d_out_len,
                     int grid_blocks)
{
	launch_sam_emit_t<true>(SAM_EMIT_ARGS);
}
void launch_sam_emit_se(void *stream, const SamParams &P, int n_reads, const SamDesc *d_desc, const int *d_req_base, const AlnReq *d_req, const AlnHdr *d_hdr,
                        const uint8_t *d_pool, const uint8_t *d_seq, const int64_t *d_off, const int *d_len, const uint8_t *d_qual,
                        const uint8_t *d_names, const int *d_name_off, const int64_t *d_ann_off, const char *d_ann_names, const int *d_ann_name_off,
                        uint8_t *d_arena, size_t arena_bytes, unsigned long long *d_arena_used, unsigned long long *d_out_off, int *d_out_len,
                        int grid_blocks)
{
	launch_sam_emit_t<false>(SAM_EMIT_ARGS);
}
#undef SAM_EMIT_ARGS

} // namespace mbw
