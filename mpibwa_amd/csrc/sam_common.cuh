// sam_common.cuh — what the two SAM text kernels share (sam_kernel.hip: sam_emit_kernel, records of one line, a lane per record;
// sam_lines_kernel.hip: records of several lines, a wavefront per read): the alignment fields of a line as mem_reg2aln leaves them
// (src/bwamem.c:1123-1157), the lane's byte sink, TLEN (src/bwamem.c:861-865), the numbers of an XA entry (src/bwamem_extra.c:122-129)
// and the lane broadcast.
#ifndef MBW_SAM_COMMON_CUH
#define MBW_SAM_COMMON_CUH
#include <hip/hip_runtime.h>
#include "device.h"

namespace mbw {

#define XA_STAGE 64      // bytes of LDS per XA entry being written (",±pos,CIGAR,NM;": a CIGAR of a dozen operations fits), 16 entries
#define SAM_ROW 260      // bytes of LDS scratch per lane (65 dwords: rows start in different banks); a record whose short
                         // fields outgrow it (a CIGAR of dozens of operations) goes back to the host

struct SamAln {   // mem_aln_t as mem_reg2aln leaves it, for the fields mem_aln2sam reads
	long long pos;       // 0-based on its contig
	int rid, is_rev, n_cigar, rlen, NM, md_len;
	int clip5, clip3;    // soft clips added in front / behind the device's CIGAR
	int skip_front, skip_back;   // 1 when the first / last operation of the device's CIGAR (a deletion) is dropped
	const uint32_t *cig;
	const uint8_t *md;
	bool ok;
};

__device__ __forceinline__ SamAln sam_aln(const SamDesc &D, const AlnHdr *__restrict__ hdr, const uint8_t *__restrict__ pool, int req_base,
                                          long long l_pac, const long long *__restrict__ ann_off, int l_query)
{
	SamAln a;
	const AlnHdr h = hdr[req_base + D.req];
	a.ok = h.flags == 0;
	a.cig = (const uint32_t *)(pool + (size_t)h.pool_off * 4);
	a.md = (const uint8_t *)(a.cig + h.n_cigar);
	a.n_cigar = h.n_cigar; a.NM = h.NM & 0x3fffff; a.md_len = h.md_len;
	a.is_rev = D.rb >= l_pac;
	const long long p = D.rb < l_pac ? D.rb : D.re - 1;                 // bns_depos
	long long pos = a.is_rev ? (l_pac << 1) - 1 - p : p;
	a.skip_front = a.skip_back = 0;
	if (a.ok && a.n_cigar > 0) {   // squeeze out a leading or trailing deletion
		const uint32_t c0 = a.cig[0], c1 = a.cig[a.n_cigar - 1];
		if ((c0 & 0xf) == 2) { pos += c0 >> 4; a.skip_front = 1; }
		else if ((c1 & 0xf) == 2) a.skip_back = 1;
	}
	a.clip5 = a.clip3 = 0;
	if (D.qb != 0 || D.qe != l_query) {
		a.clip5 = a.is_rev ? l_query - D.qe : D.qb;
		a.clip3 = a.is_rev ? D.qb : l_query - D.qe;
	}
	a.rid = D.rid;
	a.pos = pos - ann_off[D.rid];
	int rl = 0;
	if (a.ok)
		for (int k = a.skip_front; k < a.n_cigar - a.skip_back; ++k) {
			const uint32_t c = a.cig[k];
			if ((c & 0xf) == 0 || (c & 0xf) == 2) rl += (int)(c >> 4);
		}
	a.rlen = rl;
	return a;
}

// ---- the lane's byte sink: its scratch row ----
struct Sink {
	uint8_t *row;
	int len;
	int cap = SAM_ROW;   // (0: the bytes are counted only)
	__device__ __forceinline__ void ch(char c) { if (len < cap) row[len] = (uint8_t)c; ++len; }
	__device__ __forceinline__ void lit(const char *s) { for (; *s; ++s) ch(*s); }
	__device__ __forceinline__ void num32(uint32_t u)
	{
		char tmp[12];
		int n = 0;
		do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
		while (n) ch(tmp[--n]);
	}
	__device__ __forceinline__ void num(long long v)
	{
		unsigned long long u = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
		if (v < 0) ch('-');
		if (u >> 32) {   // never on a real genome (contigs are shorter than 2^31), kept for the general case
			char tmp[24];
			int n = 0;
			do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
			while (n) ch(tmp[--n]);
		} else num32((uint32_t)u);
	}
	// clip5 S + the device's operations (without a dropped deletion) + clip3 S, as text
	__device__ __forceinline__ void cigar(const SamAln &a)
	{
		if (a.clip5) { num32(a.clip5); ch('S'); }
		for (int k = a.skip_front; k < a.n_cigar - a.skip_back; ++k) {
			const uint32_t c = a.cig[k];
			num32(c >> 4);
			ch("MIDSH"[c & 0xf]);
		}
		if (a.clip3) { num32(a.clip3); ch('S'); }
	}
};

// TLEN of a line p whose mate m lies on the same contig (src/bwamem.c:861-865); n_p, n_m: the operations of the two CIGARs as printed
__device__ __forceinline__ void sam_tlen(Sink &S, const SamAln &p, int n_p, const SamAln &m, int n_m)
{
	const long long p0 = p.pos + (p.is_rev ? p.rlen - 1 : 0), p1 = m.pos + (m.is_rev ? m.rlen - 1 : 0);
	if (n_m == 0 || n_p == 0) S.ch('0');
	else S.num(-(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0)));
}

// XA entry j of the line D (its request follows the line's own): the alignment as mem_reg2aln leaves it, clips as S
__device__ __forceinline__ SamAln xa_aln(const SamDesc &D, int j, const AlnReq *__restrict__ reqs, const AlnHdr *__restrict__ hdr, const uint8_t *__restrict__ pool,
                                         int req_base, long long l_pac, const long long *__restrict__ ann_off, int l_query)
{
	const AlnReq q = reqs[req_base + D.req + 1 + j];
	SamDesc X;
	X.rb = q.rb; X.re = q.re; X.qb = q.qb; X.qe = q.qe; X.req = D.req + 1 + j; X.rid = q.pad;
	X.flag = X.mapq = X.score = X.sub = 0;
	return sam_aln(X, hdr, pool, req_base, l_pac, ann_off, l_query);
}
// the entry behind its contig name (src/bwamem_extra.c:122-129)
__device__ __forceinline__ void xa_numbers(Sink &S, const SamAln &x)
{
	S.ch(','); S.ch(x.is_rev ? '-' : '+'); S.num(x.pos + 1);
	S.ch(','); S.cigar(x);
	S.ch(','); S.num32((uint32_t)x.NM); S.ch(';');
}

template <class T>
__device__ __forceinline__ T bcast(T v, int src)   // the value lane `src` (wave-uniform) holds
{
	static_assert(sizeof(T) == 4 || sizeof(T) == 8, "");
	if (sizeof(T) == 4) {
		int x = __builtin_amdgcn_readlane(*(int *)&v, src);
		return *(T *)&x;
	}
	int lo = __builtin_amdgcn_readlane(((int *)&v)[0], src), hi = __builtin_amdgcn_readlane(((int *)&v)[1], src);
	unsigned long long x = (unsigned)lo | ((unsigned long long)(unsigned)hi << 32);
	return *(T *)&x;
}

} // namespace mbw
#endif
