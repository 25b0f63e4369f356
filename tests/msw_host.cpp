// The host walk of the mate rescue's local alignment (csrc/local_sw.cpp) as a program of its own, for a run under the address and
// undefined-behaviour sanitizers (tests/test_msw_cases.py): reads the jobs of tests/msw_cases.py from a file, prints the seven result
// words of each.  File: one job per three lines --
//   a b o_del e_del o_ins e_ins xtra qlen tlen
//   the query's codes, one digit each
//   the target's codes, one digit each
// The arrays handed to bmh_local_sw are exactly as long as the job says (heap blocks of their own: a read beside them is seen).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "local_sw.h"

static bool read_line(FILE *f, std::string &s)
{
	s.clear();
	int c;
	while ((c = fgetc(f)) != EOF && c != '\n') s.push_back((char)c);
	return c != EOF || !s.empty();
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s jobs.txt\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "r");
	if (!f) { perror(argv[1]); return 2; }
	std::string head, qs, ts;
	size_t n = 0;
	while (read_line(f, head) && !head.empty()) {
		bmh_ext_params_t p;
		memset(&p, 0, sizeof(p));
		int xtra = 0, qlen = 0, tlen = 0;
		if (sscanf(head.c_str(), "%d %d %d %d %d %d %d %d %d", &p.a, &p.b, &p.o_del, &p.e_del, &p.o_ins, &p.e_ins, &xtra, &qlen, &tlen) != 9 ||
		    !read_line(f, qs) || !read_line(f, ts) || (int)qs.size() != qlen || (int)ts.size() != tlen) {
			fprintf(stderr, "job %zu: malformed\n", n);
			return 2;
		}
		uint8_t *q = (uint8_t *)malloc(qlen ? qlen : 1), *t = (uint8_t *)malloc(tlen ? tlen : 1);
		for (int i = 0; i < qlen; ++i) q[i] = (uint8_t)(qs[i] - '0');
		for (int i = 0; i < tlen; ++i) t[i] = (uint8_t)(ts[i] - '0');
		const bmh_sw_result_t r = bmh_local_sw(qlen, q, tlen, t, p, xtra);
		for (int i = 0; i < qlen; ++i) if (q[i] != (uint8_t)(qs[i] - '0')) { fprintf(stderr, "job %zu: the query came back changed\n", n); return 3; }
		for (int i = 0; i < tlen; ++i) if (t[i] != (uint8_t)(ts[i] - '0')) { fprintf(stderr, "job %zu: the target came back changed\n", n); return 3; }
		printf("%d %d %d %d %d %d %d\n", r.score, r.te, r.qe, r.score2, r.te2, r.tb, r.qb);
		free(q); free(t);
		++n;
	}
	fclose(f);
	fprintf(stderr, "%zu jobs\n", n);
	return 0;
}
