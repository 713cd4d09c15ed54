// eval_ensemble_main.cpp -- the per-sample arithmetic of the ensemble analysis (csrc/eval_elements.hpp: irrl_eval_ensemble_features,
// irrl_eval_ensemble_key, irrl_eval_ensemble_bin, irrl_eval_ensemble_spec_error) run on the HOST, with a plain serial count of the distinct keys
// in place of the kernel's sort: tests/test_eval_ensemble_host.py compiles this file with g++ and the address / undefined-behaviour sanitizers,
// hands it a case file and compares what it writes with the numpy twin (evaluate.ensemble_numpy).  No HIP, no Python loading.  The twin of
// eval_gait_main.cpp.
//
//   eval_ensemble_main <case file> <result file>
// case file:   int32 rows, N, C | f64 lb[6] ub[6] prec[6] hist_lo[6] hist_hi[6] | int32 hist_bins | u8 mask[N] | f32 body[rows][N][13]
// result file: f64 x[rows][N][6] | u64 key[rows][N] | u8 kept[rows][N] (finite AND mask) | int32 bin[rows][N][6] (-1: none) |
//              f64 entropy[C][rows] | u32 counts[C][rows][3] (kept M | distinct keys | largest cell)
// A spec that irrl_eval_ensemble_spec_error refuses: the text on stderr, exit status 3, no result file.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eval_elements.hpp"

template <class T>
static void rd(FILE *f, T *p, size_t n) {
  if (n == 0) return;
  if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "case file too short\n"); exit(2); }
}
template <class T>
static void wr(FILE *f, const T *p, size_t n) {
  if (n == 0) return;
  if (fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); }
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[3];
  rd(f, hdr, 3);
  irrl_eval_ensemble_spec spec;
  rd(f, spec.lb, 6); rd(f, spec.ub, 6); rd(f, spec.prec, 6); rd(f, spec.hist_lo, 6); rd(f, spec.hist_hi, 6);
  rd(f, &spec.hist_bins, 1);
  const int rows = hdr[0], N = hdr[1], C = hdr[2];
  if (rows < 0 || N < 1 || C < 1 || N % C) { fprintf(stderr, "bad header\n"); return 2; }
  if (const char *bad = irrl_eval_ensemble_spec_error(spec)) { fprintf(stderr, "spec: %s\n", bad); return 3; }
  const int E = N / C;
  const size_t RN = (size_t)rows * (size_t)N;
  std::vector<uint8_t> mask((size_t)N);
  std::vector<float> body(RN * 13);
  rd(f, mask.data(), mask.size());
  rd(f, body.data(), body.size());
  fclose(f);

  std::vector<double> x(RN * 6), entropy((size_t)C * (size_t)rows, 0.0);
  std::vector<uint64_t> key(RN, 0);
  std::vector<uint8_t> kept(RN, 0);
  std::vector<int> bin(RN * 6, -1);
  std::vector<uint32_t> counts((size_t)C * (size_t)rows * 3, 0);
  for (int r = 0; r < rows; r++) {
    for (int c = 0; c < C; c++) {
      std::vector<uint64_t> cell;
      for (int e = 0; e < E; e++) {
        const size_t s = (size_t)r * (size_t)N + (size_t)c * (size_t)E + (size_t)e;
        irrl_eval_ensemble_features(&body[s * 13], &x[s * 6]);
        uint64_t k = 0;
        const bool ok = irrl_eval_ensemble_key(&x[s * 6], spec, &k);
        if (ok) key[s] = k;
        kept[s] = ok && mask[(size_t)c * (size_t)E + (size_t)e] != 0 ? 1 : 0;
        if (!kept[s]) continue;
        cell.push_back(k);
        if (spec.hist_bins > 0)
          for (int i = 0; i < 6; i++) bin[s * 6 + (size_t)i] = irrl_eval_ensemble_bin(x[s * 6 + (size_t)i], spec.hist_lo[i], spec.hist_hi[i], spec.hist_bins);
      }
      // the plain serial count: sort, then walk
      std::sort(cell.begin(), cell.end());
      const size_t M = cell.size(), o = (size_t)c * (size_t)rows + (size_t)r;
      uint32_t distinct = 0, largest = 0;
      double h = 0.0;
      for (size_t i = 0; i < M;) {
        size_t j = i;
        while (j < M && cell[j] == cell[i]) j++;
        const uint32_t n = (uint32_t)(j - i);
        const double p = (double)n / (double)M;
        const double term = p * log(p);
        h -= term;
        distinct++;
        if (n > largest) largest = n;
        i = j;
      }
      entropy[o] = h;
      counts[o * 3] = (uint32_t)M; counts[o * 3 + 1] = distinct; counts[o * 3 + 2] = largest;
    }
  }

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  wr(f, x.data(), x.size()); wr(f, key.data(), key.size()); wr(f, kept.data(), kept.size()); wr(f, bin.data(), bin.size());
  wr(f, entropy.data(), entropy.size()); wr(f, counts.data(), counts.size());
  fclose(f);
  return 0;
}
