// pairmath_main.cpp — stand-alone driver of mpibwa_amd/csrc/pairmath.h for tests/test_pairmath.py (built with ASan + UBSan).
// stdin: one case per line, a letter and its integers; stdout: one line of results per case.
//   H key                                                  hash_64
//   D l_pac b1 b2                                          infer_dir: orientation, distance
//   W l1 l2 score a q r                                    infer_bw
//   B l1 l2 truesc a o_del e_del o_ins e_ins w_opt w_reg   reg2aln_band
//   T a b o_del e_del o_ins e_ins                          sub_n_margin
//   K l_pac rb rid contig_offset score i r                 pair_key: x, y
//   M id y                                                 pair_id_mix(id), and the low word of hash_64(y ^ mix) as mem_pair puts it into p.x
//   F ...                                                  every floating-point function once (see below): the sanitizers look at them
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <vector>
#include "pairmath.h"

using namespace mbw;

int main()
{
	char c;
	while (std::scanf(" %c", &c) == 1) {
		long long v[16];
		const int want = c == 'H' ? 1 : c == 'D' ? 3 : c == 'W' ? 6 : c == 'B' ? 10 : c == 'T' ? 6 : c == 'K' ? 7 : c == 'M' ? 2 : c == 'F' ? 12 : -1;
		if (want < 0) return 2;
		for (int i = 0; i < want; ++i)
			if (std::scanf("%lli", &v[i]) != 1) return 2;
		if (c == 'H') std::printf("%" PRIu64 "\n", hash_64((uint64_t)v[0]));
		else if (c == 'D') {
			int64_t dist;
			const int dir = infer_dir(v[0], v[1], v[2], &dist);
			std::printf("%d %" PRId64 "\n", dir, dist);
		} else if (c == 'W') std::printf("%d\n", infer_bw((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5]));
		else if (c == 'B')
			std::printf("%d\n", reg2aln_band((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9]));
		else if (c == 'T') std::printf("%d\n", sub_n_margin((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5]));
		else if (c == 'K') {
			const Pair64 k = pair_key(v[0], v[1], (int)v[2], v[3], (int)v[4], (int)v[5], (int)v[6]);
			std::printf("%" PRIu64 " %" PRIu64 "\n", k.x, k.y);
		} else if (c == 'M') {
			const int mix = pair_id_mix((uint64_t)v[0]);
			std::printf("%d %" PRIu64 "\n", mix, hash_64((uint64_t)v[1] ^ (uint64_t)(int64_t)mix) & 0xffffffffU);
		} else {
			// F id l_pac rb0 rb1 score0 score1 low high avg_x100 std_x100 a b: two hits, one per end, on the forward strand of contig 0 —
			// their keys, mem_pair's candidates with libm's score term, then the MAPQ functions and the overlap tests on the same numbers
			const uint64_t id = (uint64_t)v[0];
			const int64_t l_pac = v[1];
			const int a = (int)v[10], b = (int)v[11];
			std::vector<Pair64> key = {pair_key(l_pac, v[2], 0, 0, (int)v[4], 0, 0), pair_key(l_pac, v[3], 0, 0, (int)v[5], 0, 1)};
			if (pair_lt(key[1], key[0])) std::swap(key[0], key[1]);
			const int low[4] = {(int)v[6], (int)v[6], (int)v[6], (int)v[6]}, high[4] = {(int)v[7], (int)v[7], (int)v[7], (int)v[7]}, failed[4] = {0, 0, 1, 1};
			const double avg = v[8] / 100., sd = v[9] / 100.;
			std::vector<Pair64> u;
			int y[4] = {-1, -1, -1, -1};
			for (int i = 0; i < (int)key.size(); ++i) {
				pair_candidates_of(key.data(), i, low, high, failed, pair_id_mix(id), [&](int which) { return y[which]; },
				                   [&](int, int64_t dist) { return .721 * std::log(2. * std::erfc(std::fabs((dist - avg) / sd) * M_SQRT1_2)) * a; },
				                   [&](const Pair64 &p) { u.push_back(p); });
				y[key[i].y & 3] = i;
			}
			std::printf("%zu", u.size());
			for (const Pair64 &p : u) std::printf(" %" PRIu64 " %" PRIu64, p.x, p.y);
			const int o = u.empty() ? 0 : (int)(u[0].x >> 32), s0 = (int)v[4], s1 = (int)v[5];
			const int l = 150;
			const int q_pe = mapq_pe(o, 0, s0 + s1 - 17, (int)(4.343 * std::log(2 + 1) + .499), a, 0.f, .25f);
			const int q_se = mapq_se_q(s0, 0, 2, 30, l, .125f, a, b, 19, l < 50 ? 1. : std::log(50.) / std::log(l), (int)(4.343 * std::log(2 + 1) + .499));
			std::printf(" %d %d %d %d", raw_mapq(o - s0, a), q_pe, q_se, mapq_se_in_pair(q_se, q_pe, s0, 30, a));
			// two regions of 150 and 100 bases on the query and the reference, 60 apart, and the same pair seen as hits of one read
			std::printf(" %d %d %d\n", (int)redundant_overlap(.95f, v[2], v[2] + 150, 0, 150, v[2] + 60, v[2] + 160, 60, 160),
			            patch_reg_w(l_pac, 100, v[2], v[2] + 100, 0, 100, v[2] + 58, v[2] + 162, 60, 160), (int)query_overlap(.5f, 0, 150, 60, 160));
		}
	}
	return 0;
}
