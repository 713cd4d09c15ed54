// eval_correlation_main.cpp -- the correlation moments (csrc/eval_elements.hpp: irrl_eval_corr_add, _min, _max, _sums, _work_per_env,
// _spec_error; irrl_eval_recurrence_row) run on the HOST from plain serial loops in the stated order -- per robot the frames ascending from +0.0,
// per condition the robots ascending from +0.0: tests/test_eval_correlation_host.py compiles this file with g++ and the address / undefined-
// behaviour sanitizers, hands it a case file and compares what it writes with the numpy twin (evaluate.correlation_numpy) byte for byte.
// No HIP, no Python loading.
//
//   eval_correlation_main <case file> <result file>
// case file:   int32 rows, N, frame_first, frame_every, T, has_done, conditions, same (1: y is x's buffer) | int32 x_dim, x_first, x_count, y_dim,
//              y_first, y_count | f32 x[rows][N][x_dim] | f32 y[rows][N][y_dim] unless same | u8 rec_done[rows][N] if has_done
// result file: i64 count[C] | f64 sx[C][cx][2] | f64 sy[C][cy][2] | f64 sxy[C][cx][cy] | f32 range_x[C][cx][2] | f32 range_y[C][cy][2] |
//              u64 irrl_eval_corr_work_per_env
// A spec that irrl_eval_corr_spec_error refuses: the text on stderr, exit status 3, no result file.
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
  int hdr[8], sp[6];
  rd(f, hdr, 8);
  rd(f, sp, 6);
  const int rows = hdr[0], N = hdr[1], frame_first = hdr[2], frame_every = hdr[3], T = hdr[4], has_done = hdr[5], C = hdr[6], same = hdr[7];
  irrl_eval_corr_spec s;
  s.x_dim = sp[0]; s.x_first = sp[1]; s.x_count = sp[2]; s.y_dim = sp[3]; s.y_first = sp[4]; s.y_count = sp[5];
  if (const char *bad = irrl_eval_corr_spec_error(s)) { fprintf(stderr, "spec: %s\n", bad); return 3; }
  if (rows < 1 || N < 1 || T < 1 || T > IRRL_EVAL_CORR_MAX_FRAMES || frame_first < 0 || frame_every < 1 ||
      irrl_eval_recurrence_row(frame_first, frame_every, T - 1) >= rows || C < 1 || N % C != 0 || (same && s.x_dim != s.y_dim)) {
    fprintf(stderr, "bad header\n"); return 2;
  }
  std::vector<float> xbuf((size_t)rows * (size_t)N * (size_t)s.x_dim), ybuf;
  rd(f, xbuf.data(), xbuf.size());
  if (!same) { ybuf.resize((size_t)rows * (size_t)N * (size_t)s.y_dim); rd(f, ybuf.data(), ybuf.size()); }
  const std::vector<float> &x = xbuf, &y = same ? xbuf : ybuf;
  std::vector<uint8_t> done;
  if (has_done) { done.resize((size_t)rows * (size_t)N); rd(f, done.data(), done.size()); }
  fclose(f);

  const size_t cx = (size_t)s.x_count, cy = (size_t)s.y_count, G = (size_t)C, R = (size_t)(N / C);
  std::vector<int64_t> count(G, 0);
  std::vector<double> sx(G * cx * 2, 0.0), sy(G * cy * 2, 0.0), sxy(G * cx * cy, 0.0);
  std::vector<float> rx(G * cx * 2), ry(G * cy * 2);
  for (size_t i = 0; i < G * cx; i++) { rx[2 * i] = INFINITY; rx[2 * i + 1] = -INFINITY; }
  for (size_t i = 0; i < G * cy; i++) { ry[2 * i] = INFINITY; ry[2 * i + 1] = -INFINITY; }
  std::vector<double> px(cx * 2), py(cy * 2), pxy(cx * cy);
  std::vector<float> prx(cx * 2), pry(cy * 2);
  for (size_t g = 0; g < G; g++)
    for (size_t r = 0; r < R; r++) {
      const size_t e = g * R + r;
      int te = T;
      if (has_done)
        for (int i = 0; i < T; i++)
          if (done[(size_t)irrl_eval_recurrence_row(frame_first, frame_every, i) * (size_t)N + e] != 0) { te = i; break; }
      for (auto &v : px) v = 0.0;
      for (auto &v : py) v = 0.0;
      for (auto &v : pxy) v = 0.0;
      for (size_t c = 0; c < cx; c++) { prx[2 * c] = INFINITY; prx[2 * c + 1] = -INFINITY; }
      for (size_t c = 0; c < cy; c++) { pry[2 * c] = INFINITY; pry[2 * c + 1] = -INFINITY; }
      for (int i = 0; i < te; i++) {                              // the robot's frames in ascending order
        const size_t row = (size_t)irrl_eval_recurrence_row(frame_first, frame_every, i);
        const float *xr = &x[(row * (size_t)N + e) * (size_t)s.x_dim + (size_t)s.x_first];
        const float *yr = &y[(row * (size_t)N + e) * (size_t)s.y_dim + (size_t)s.y_first];
        for (size_t c = 0; c < cx; c++) {
          px[2 * c] = irrl_eval_corr_add(px[2 * c], xr[c], 1.0f);
          px[2 * c + 1] = irrl_eval_corr_add(px[2 * c + 1], xr[c], xr[c]);
          prx[2 * c] = irrl_eval_corr_min(prx[2 * c], xr[c]);
          prx[2 * c + 1] = irrl_eval_corr_max(prx[2 * c + 1], xr[c]);
          for (size_t j = 0; j < cy; j++) pxy[c * cy + j] = irrl_eval_corr_add(pxy[c * cy + j], xr[c], yr[j]);
        }
        for (size_t j = 0; j < cy; j++) {
          py[2 * j] = irrl_eval_corr_add(py[2 * j], yr[j], 1.0f);
          py[2 * j + 1] = irrl_eval_corr_add(py[2 * j + 1], yr[j], yr[j]);
          pry[2 * j] = irrl_eval_corr_min(pry[2 * j], yr[j]);
          pry[2 * j + 1] = irrl_eval_corr_max(pry[2 * j + 1], yr[j]);
        }
      }
      count[g] += te;                                             // the condition's robots in ascending order
      for (size_t k = 0; k < cx * 2; k++) sx[g * cx * 2 + k] = sx[g * cx * 2 + k] + px[k];
      for (size_t k = 0; k < cy * 2; k++) sy[g * cy * 2 + k] = sy[g * cy * 2 + k] + py[k];
      for (size_t k = 0; k < cx * cy; k++) sxy[g * cx * cy + k] = sxy[g * cx * cy + k] + pxy[k];
      for (size_t c = 0; c < cx; c++) {
        rx[(g * cx + c) * 2] = irrl_eval_corr_min(rx[(g * cx + c) * 2], prx[2 * c]);
        rx[(g * cx + c) * 2 + 1] = irrl_eval_corr_max(rx[(g * cx + c) * 2 + 1], prx[2 * c + 1]);
      }
      for (size_t c = 0; c < cy; c++) {
        ry[(g * cy + c) * 2] = irrl_eval_corr_min(ry[(g * cy + c) * 2], pry[2 * c]);
        ry[(g * cy + c) * 2 + 1] = irrl_eval_corr_max(ry[(g * cy + c) * 2 + 1], pry[2 * c + 1]);
      }
    }

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  wr(f, count.data(), count.size());
  wr(f, sx.data(), sx.size());
  wr(f, sy.data(), sy.size());
  wr(f, sxy.data(), sxy.size());
  wr(f, rx.data(), rx.size());
  wr(f, ry.data(), ry.size());
  const uint64_t per = (uint64_t)irrl_eval_corr_work_per_env(s);
  wr(f, &per, 1);
  fclose(f);
  return 0;
}
