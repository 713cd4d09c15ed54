// eval_footfall_main.cpp -- the per-sample rules of the gait recorder's analyses (csrc/eval_elements.hpp: irrl_eval_footfall_flag, _filter,
// _fill_end, _phase_bin, _spec_error; irrl_eval_motor_sample, _up, _low, _classes, _spec_error; irrl_eval_ensemble_bin) run on the HOST from
// plain serial loops in place of the kernels' word arithmetic: tests/test_eval_footfall_host.py compiles this file with g++ and the address /
// undefined-behaviour sanitizers, hands it a case file and compares what it writes with the numpy twins (evaluate.footfall_numpy,
// evaluate.motor_plane_numpy).  No HIP, no Python loading.
//
//   eval_footfall_main <case file> <result file>
// case file:   int32 mode (0 footfall, 1 motor plane), rows, N, frame_first, frame_every, T, has_done, conditions |
//              mode 0: int32 reach, hold, phase_bins;  mode 1: f64 [9] tau_max .. w_hi, int32 t_bins, w_bins, period |
//              f32 rec_gait[rows][N][32] | u8 rec_done[rows][N] if has_done
// result file: mode 0: u8 f[N][4][T] (the sequential rule; 0 behind T_e) | u8 the same by the closed form | u32 counts[N][4][14] |
//                      u32 support[N][16] | u32 phase[N][3][phase_bins] | u8 pattern[T][N]
//              mode 1: u32 counts[C][12][6] | u32 hist[C][12][t_bins][w_bins] | f64 fold[C][12][period][3]
// A spec that the _spec_error functions refuse: the text on stderr, exit status 3, no result file.
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

static void footfall(const std::vector<float> &rec, const std::vector<int> &te, int N, int frame_first, int frame_every, int T,
                     const irrl_eval_footfall_spec &spec, FILE *out) {
  const int bins = spec.phase_bins;
  std::vector<uint8_t> fs((size_t)N * 4 * (size_t)T, 0), fc((size_t)N * 4 * (size_t)T, 0), pattern((size_t)T * (size_t)N, 0);
  std::vector<uint32_t> counts((size_t)N * 4 * IRRL_EVAL_FOOTFALL_COUNTS, 0), support((size_t)N * 16, 0), phase((size_t)N * 3 * (size_t)bins, 0);
  for (int e = 0; e < N; e++) {
    const int n = te[(size_t)e];
    std::vector<int> td0;                                  // the touchdowns of leg 0
    for (int l = 0; l < 4; l++) {
      std::vector<uint8_t> c((size_t)n), d((size_t)n);
      for (int k = 0; k < n; k++) {
        const size_t row = (size_t)irrl_eval_recurrence_row(frame_first, frame_every, k);
        c[(size_t)k] = irrl_eval_footfall_flag(rec[(row * (size_t)N + (size_t)e) * 32 + 24 + (size_t)l]) ? 1 : 0;
      }
      uint8_t *f = &fs[((size_t)e * 4 + (size_t)l) * (size_t)T], *g = &fc[((size_t)e * 4 + (size_t)l) * (size_t)T];
      irrl_eval_footfall_filter(c.data(), n, spec.reach, spec.hold, f);
      // the closed form: the dilation by a zero-hold run of the same function, then gap by gap
      irrl_eval_footfall_filter(c.data(), n, spec.reach, 0, d.data());
      int a = -1;
      for (int k = 0; k < n; k++) g[k] = d[(size_t)k];
      for (int k = 0; k < n; k++) {
        if (!d[(size_t)k]) continue;
        if (a >= 0 && k > a + 1) {
          const int end = irrl_eval_footfall_fill_end(n, spec.hold, a, k);
          for (int i = a + 1; i < end; i++) g[i] = 1;
        }
        a = k;
      }
      uint32_t *o = &counts[((size_t)e * 4 + (size_t)l) * IRRL_EVAL_FOOTFALL_COUNTS];
      o[IRRL_EVAL_FOOTFALL_FRAMES] = (uint32_t)n;
      o[IRRL_EVAL_FOOTFALL_FIRST_TD] = o[IRRL_EVAL_FOOTFALL_LAST_TD] = IRRL_EVAL_FOOTFALL_NONE;
      int last_td = -1, last_lo = -1;
      for (int k = 0; k < n; k++) {
        if (c[(size_t)k]) o[IRRL_EVAL_FOOTFALL_RAW_STANCE]++;
        if (k >= 1 && !c[(size_t)k - 1] && c[(size_t)k]) o[IRRL_EVAL_FOOTFALL_RAW_TOUCHDOWNS]++;
        if (f[k]) { o[IRRL_EVAL_FOOTFALL_STANCE]++; pattern[(size_t)k * (size_t)N + (size_t)e] |= (uint8_t)(1u << l); }
        if (k >= 1 && !f[k - 1] && f[k]) {
          o[IRRL_EVAL_FOOTFALL_TOUCHDOWNS]++;
          if (o[IRRL_EVAL_FOOTFALL_FIRST_TD] == IRRL_EVAL_FOOTFALL_NONE) o[IRRL_EVAL_FOOTFALL_FIRST_TD] = (uint32_t)k;
          o[IRRL_EVAL_FOOTFALL_LAST_TD] = (uint32_t)k;
          if (last_lo >= 0) {
            const uint32_t len = (uint32_t)(k - last_lo);
            o[IRRL_EVAL_FOOTFALL_SWING_PHASES]++; o[IRRL_EVAL_FOOTFALL_SWING_SUM] += len;
            if (len > o[IRRL_EVAL_FOOTFALL_SWING_MAX]) o[IRRL_EVAL_FOOTFALL_SWING_MAX] = len;
          }
          last_td = k;
          if (l == 0) td0.push_back(k);
        }
        if (k >= 1 && f[k - 1] && !f[k]) {
          o[IRRL_EVAL_FOOTFALL_LIFTOFFS]++;
          if (last_td >= 0) {
            const uint32_t len = (uint32_t)(k - last_td);
            o[IRRL_EVAL_FOOTFALL_STANCE_PHASES]++; o[IRRL_EVAL_FOOTFALL_STANCE_SUM] += len;
            if (len > o[IRRL_EVAL_FOOTFALL_STANCE_MAX]) o[IRRL_EVAL_FOOTFALL_STANCE_MAX] = len;
          }
          last_lo = k;
        }
        if (l > 0 && bins > 0 && k >= 1 && !f[k - 1] && f[k]) {
          for (size_t s = 0; s + 1 < td0.size(); s++)
            if (td0[s] <= k && k < td0[s + 1])
              phase[((size_t)e * 3 + (size_t)l - 1) * (size_t)bins + (size_t)irrl_eval_footfall_phase_bin(k, td0[s], td0[s + 1], bins)]++;
        }
      }
    }
    for (int k = 0; k < n; k++) support[(size_t)e * 16 + pattern[(size_t)k * (size_t)N + (size_t)e]]++;
  }
  wr(out, fs.data(), fs.size()); wr(out, fc.data(), fc.size()); wr(out, counts.data(), counts.size()); wr(out, support.data(), support.size());
  wr(out, phase.data(), phase.size()); wr(out, pattern.data(), pattern.size());
}

static void motor(const std::vector<float> &rec, const std::vector<int> &te, int N, int C, int frame_first, int frame_every,
                  const irrl_eval_motor_spec &s, FILE *out) {
  const int R = N / C, tb = s.t_bins, wb = s.w_bins, period = s.period;
  const size_t cells = (size_t)tb * (size_t)wb;
  std::vector<uint32_t> counts((size_t)C * 12 * IRRL_EVAL_MOTOR_COUNTS, 0), hist((size_t)C * 12 * cells, 0);
  std::vector<double> fold((size_t)C * 12 * (size_t)period * 3, 0.0);
  for (int c = 0; c < C; c++)
    for (int j = 0; j < 12; j++) {
      const size_t cj = (size_t)c * 12 + (size_t)j;
      for (int r = 0; r < R; r++) {
        const size_t e = (size_t)c * (size_t)R + (size_t)r;
        for (int i = 0; i < te[e]; i++) {
          const size_t row = (size_t)irrl_eval_recurrence_row(frame_first, frame_every, i);
          const float *g = &rec[(row * (size_t)N + e) * 32];
          double m, w;
          if (!irrl_eval_motor_sample(g[j], g[12 + j], j, s.knee_ratio, &m, &w)) continue;
          const unsigned bits = irrl_eval_motor_classes(m, w, s);
          counts[cj * IRRL_EVAL_MOTOR_COUNTS]++;
          for (int k = 1; k < IRRL_EVAL_MOTOR_COUNTS; k++) counts[cj * IRRL_EVAL_MOTOR_COUNTS + (size_t)k] += (bits >> (k - 1)) & 1u;
          if (cells > 0) {
            const int bt = irrl_eval_ensemble_bin(m, s.t_lo, s.t_hi, tb), bw = irrl_eval_ensemble_bin(w, s.w_lo, s.w_hi, wb);
            if (bt >= 0 && bw >= 0) hist[cj * cells + (size_t)bt * (size_t)wb + (size_t)bw]++;
          }
          if (period > 0) {
            double *f = &fold[(cj * (size_t)period + (size_t)(i % period)) * 3];
            f[0] = f[0] + 1.0;
            f[1] = f[1] + m;
            f[2] = f[2] + w;
          }
        }
      }
    }
  wr(out, counts.data(), counts.size()); wr(out, hist.data(), hist.size()); wr(out, fold.data(), fold.size());
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[8];
  rd(f, hdr, 8);
  const int mode = hdr[0], rows = hdr[1], N = hdr[2], frame_first = hdr[3], frame_every = hdr[4], T = hdr[5], has_done = hdr[6], C = hdr[7];
  if ((mode != 0 && mode != 1) || rows < 0 || N < 1 || T < 0 || T > IRRL_EVAL_FOOTFALL_MAX_FRAMES || frame_first < 0 || frame_every < 1 ||
      (T > 0 && irrl_eval_recurrence_row(frame_first, frame_every, T - 1) >= rows) || C < 1 || N % C != 0) { fprintf(stderr, "bad header\n"); return 2; }
  irrl_eval_footfall_spec fspec = {0, 0, 0};
  irrl_eval_motor_spec mspec = {};
  if (mode == 0) {
    int v[3];
    rd(f, v, 3);
    fspec.reach = v[0]; fspec.hold = v[1]; fspec.phase_bins = v[2];
    if (const char *bad = irrl_eval_footfall_spec_error(fspec)) { fprintf(stderr, "spec: %s\n", bad); return 3; }
  } else {
    double d[9];
    int v[3];
    rd(f, d, 9); rd(f, v, 3);
    mspec.tau_max = d[0]; mspec.w_crit = d[1]; mspec.w_max = d[2]; mspec.knee_ratio = d[3]; mspec.sat = d[4];
    mspec.t_lo = d[5]; mspec.t_hi = d[6]; mspec.w_lo = d[7]; mspec.w_hi = d[8];
    mspec.t_bins = v[0]; mspec.w_bins = v[1]; mspec.period = v[2];
    if (const char *bad = irrl_eval_motor_spec_error(mspec)) { fprintf(stderr, "spec: %s\n", bad); return 3; }
  }
  std::vector<float> rec((size_t)rows * (size_t)N * 32);
  rd(f, rec.data(), rec.size());
  std::vector<uint8_t> done;
  if (has_done) { done.resize((size_t)rows * (size_t)N); rd(f, done.data(), done.size()); }
  fclose(f);
  std::vector<int> te((size_t)N, T);
  if (has_done)
    for (int e = 0; e < N; e++)
      for (int i = 0; i < T; i++)
        if (done[(size_t)irrl_eval_recurrence_row(frame_first, frame_every, i) * (size_t)N + (size_t)e] != 0) { te[(size_t)e] = i; break; }
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  if (mode == 0) footfall(rec, te, N, frame_first, frame_every, T, fspec, f);
  else motor(rec, te, N, C, frame_first, frame_every, mspec, f);
  fclose(f);
  return 0;
}
