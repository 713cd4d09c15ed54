// eval_footfall.hip -- the two analyses of a gait recorder (irrl_eval_footfall, irrl_eval_motor_plane, include/irrl_env.h): debounced footfalls
// per robot and leg, and the motor's torque-speed plane per (condition, joint).  A translation unit of its own, compiled by the plain driver; no
// global atomics and no floating-point atomics: every output word has exactly one writer.  The per-sample rules: csrc/eval_elements.hpp.
//
// irrl_eval_footfall_kernel, one workgroup per robot.  A robot's work is 4 x T flags, so the flags live in LDS as 64-frame BIT WORDS (a wave's
// ballot of one load per lane) and every later step is word arithmetic: one task = (leg, word), leg = tid & 3, word = tid >> 2, ... -- a lane keeps
// its leg.  T = 1000 is 16 words x 4 legs = 64 tasks: ONE wave per robot with every lane busy, which is why the workgroup is 64 threads up to
// T = 4096 (at most 4 tasks a lane) and 256 threads (4 waves) above.  Order of the work:
//   1. load: wave v takes words v, v + waves, ...; lane = frame; the four flags and the `done` byte; five ballots; T_e by an LDS atomicMin.
//   2. dilate: d = OR of the flags shifted by -reach .. reach across the word borders, masked to k < T_e.
//   3. hold (the closed form): for every run of zeros of d inside the word, a = the last set bit in front (in an earlier word: a max-scan
//      walked backwards over the words until one is non-zero), b = the first set bit behind (a min-scan walked forwards), and
//      irrl_eval_footfall_fill_end says how far the run is filled.  A run over several words gets the same (a, b) from each of its words.
//   4. edges: touchdown and liftoff words of f, popcounts, first / last touchdown; for every liftoff the start of its stance (the last zero
//      of f in front, walked backwards), for every touchdown the start of its swing (the last one in front); the support patterns 4 leg .. 4 leg + 3
//      of the word by popcounts of the four legs' words.
//   5. phase: every touchdown of legs 1 .. 3 between the neighbouring touchdowns of leg 0 (the same two walks over leg 0's touchdown words),
//      counted in LDS with integer LDS atomics; the gait diagram, a byte per frame.
//   6. the counters: xor-butterfly over the lanes of one leg (offsets 4 .. 32), the waves through LDS, one thread per output word.
// The walks are linear in the words (at most 256): a gait's gaps are shorter than a word, so they end at once; nothing was tuned.
//
// irrl_eval_motor_plane_kernel, one workgroup of 256 threads per (condition, joint), the condition's robots in chunks of 64: T_e per robot by
// LDS atomicMin over the flattened (frame, robot) pairs, then the same pairs again for the six counters (registers) and the 2-D histogram (LDS,
// integer atomics), then thread p walks the chunk's robots in index order and each robot's frames p, p + period, ... in order, adding to its own
// three f64 words in LDS: the sums have ONE order, whatever the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eval_footfall.hpp"

typedef unsigned long long ff_word;
#define FF_MAX_WAVES 4
#define FF_C IRRL_EVAL_FOOTFALL_COUNTS

// bits k < n of word w of a window of n frames
static __device__ __forceinline__ ff_word ff_valid(int w, int n) {
  const int left = n - w * 64;
  return left <= 0 ? 0ull : left >= 64 ? ~0ull : ((1ull << left) - 1ull);
}
static __device__ __forceinline__ ff_word ff_low_bits(int n) { return n <= 0 ? 0ull : n >= 64 ? ~0ull : ((1ull << n) - 1ull); }
// the last index < k whose bit is set (inverted: clear), -1 if none; every index < k is a frame of the window
static __device__ __forceinline__ int ff_last_before(const ff_word *words, int k, bool inverted) {
  if (k <= 0) return -1;
  int v = (k - 1) >> 6;
  ff_word x = (inverted ? ~words[v] : words[v]) & ff_low_bits(((k - 1) & 63) + 1);
  for (;;) {
    if (x != 0ull) return v * 64 + 63 - __clzll((long long)x);
    if (--v < 0) return -1;
    x = inverted ? ~words[v] : words[v];
  }
}
// the first index > k whose bit is set, -1 if none (bits beyond the window are clear)
static __device__ __forceinline__ int ff_first_after(const ff_word *words, int k, int W) {
  int v = (k + 1) >> 6;
  if (v >= W) return -1;
  ff_word x = words[v] & ~ff_low_bits((k + 1) & 63);
  for (;;) {
    if (x != 0ull) return v * 64 + __ffsll((long long)x) - 1;
    if (++v >= W) return -1;
    x = words[v];
  }
}

__global__ __launch_bounds__(256) void irrl_eval_footfall_kernel(const FootfallArgs a) {
  extern __shared__ __attribute__((aligned(16))) ff_word ff_lds[];      // raw [4][W] | f [4][W] | d, later touchdowns [4][W]
  __shared__ int te_s;
  __shared__ unsigned part_s[FF_MAX_WAVES][4][FF_C];
  __shared__ unsigned sup_s[FF_MAX_WAVES][16];
  __shared__ unsigned phase_s[3 * IRRL_EVAL_FOOTFALL_MAX_BINS];
  const int T = a.T, W = irrl_eval_footfall_words(T), N = a.N;
  ff_word *Cw = ff_lds, *Fw = ff_lds + 4 * W, *Xw = ff_lds + 8 * W;
  const int e = (int)blockIdx.x, tid = (int)threadIdx.x, threads = (int)blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, waves = threads >> 6;
  const int leg = tid & 3;
  const int reach = a.spec.reach, hold = a.spec.hold;
  const int bins = a.phase ? a.spec.phase_bins : 0;

  if (tid == 0) te_s = T;
  for (int i = tid; i < 3 * IRRL_EVAL_FOOTFALL_MAX_BINS; i += threads) phase_s[i] = 0u;
  __syncthreads();

  // 1. load
  for (int w = wave; w < W; w += waves) {
    const int i = w * 64 + lane;
    bool c0 = false, c1 = false, c2 = false, c3 = false, dn = false;
    if (i < T) {
      const size_t row = (size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i);
      const float *g = a.rec_gait + (row * (size_t)N + (size_t)e) * IRRL_EVAL_GAIT_REC_DIM + 24;
      c0 = irrl_eval_footfall_flag(g[0]); c1 = irrl_eval_footfall_flag(g[1]);
      c2 = irrl_eval_footfall_flag(g[2]); c3 = irrl_eval_footfall_flag(g[3]);
      if (a.rec_done) dn = a.rec_done[row * (size_t)N + (size_t)e] != 0;
    }
    const ff_word b0 = __ballot(c0), b1 = __ballot(c1), b2 = __ballot(c2), b3 = __ballot(c3), bd = __ballot(dn);
    if (lane == 0) {
      Cw[w] = b0; Cw[W + w] = b1; Cw[2 * W + w] = b2; Cw[3 * W + w] = b3;
      if (bd != 0ull) atomicMin(&te_s, w * 64 + __ffsll((long long)bd) - 1);
    }
  }
  __syncthreads();
  const int Te = te_s;
  const ff_word *Cl = Cw + leg * W;
  ff_word *Fl = Fw + leg * W, *Xl = Xw + leg * W;

  // 2. dilate
  for (int w = tid >> 2; w < W; w += threads >> 2) {
    const ff_word cur = Cl[w] & ff_valid(w, Te);
    const ff_word prev = w > 0 ? Cl[w - 1] & ff_valid(w - 1, Te) : 0ull;
    const ff_word next = w + 1 < W ? Cl[w + 1] & ff_valid(w + 1, Te) : 0ull;
    ff_word d = cur;
    for (int s = 1; s <= reach; s++) d |= (cur << s) | (prev >> (64 - s)) | (cur >> s) | (next << (64 - s));
    Xl[w] = d & ff_valid(w, Te);
  }
  __syncthreads();

  // 3. hold
  for (int w = tid >> 2; w < W; w += threads >> 2) {
    const ff_word vm = ff_valid(w, Te), d = Xl[w];
    ff_word f = d, z = ~d & vm;
    if (z != 0ull) {
      const int A = ff_last_before(Xl, w * 64, false);
      int B = ff_first_after(Xl, w * 64 + 63, W);
      if (B < 0) B = Te;
      while (z != 0ull) {
        const int s = __ffsll((long long)z) - 1;
        const ff_word t = ~(z >> s);
        const int len = t != 0ull ? __ffsll((long long)t) - 1 : 64;
        const int end_bit = s + len;                          // <= 64
        const int ga = s > 0 ? w * 64 + s - 1 : A;            // (the bit in front of a run inside the word is set)
        const int gb = end_bit >= 64 ? B : ((vm >> end_bit) & 1ull) ? w * 64 + end_bit : Te;
        int n = irrl_eval_footfall_fill_end(Te, hold, ga, gb) - (w * 64 + s);
        n = n < 0 ? 0 : n > len ? len : n;
        f |= ff_low_bits(n) << s;
        z &= ~(ff_low_bits(len) << s);
      }
    }
    Fl[w] = f;
  }
  __syncthreads();

  // 4. edges, counters, support
  unsigned raw_stance = 0u, raw_td = 0u, stance = 0u, tds = 0u, los = 0u, first_td = IRRL_EVAL_FOOTFALL_NONE;
  int last_td = -1;
  unsigned st_n = 0u, st_sum = 0u, st_max = 0u, sw_n = 0u, sw_sum = 0u, sw_max = 0u;
  unsigned sup[4] = {0u, 0u, 0u, 0u};
  for (int w = tid >> 2; w < W; w += threads >> 2) {
    const ff_word vm = ff_valid(w, Te);
    const ff_word c = Cl[w] & vm, cp = w > 0 ? (Cl[w - 1] & ff_valid(w - 1, Te)) >> 63 : 1ull;
    raw_stance += (unsigned)__popcll(c);
    raw_td += (unsigned)__popcll(c & ~((c << 1) | cp));
    const ff_word f = Fl[w], fp = w > 0 ? Fl[w - 1] >> 63 : 0ull;
    const ff_word td = f & ~((f << 1) | (w > 0 ? fp : 1ull));   // frame 0 is no touchdown
    const ff_word lo = ((f << 1) | fp) & ~f & vm;
    Xl[w] = td;                                                  // (d is no longer read: the barrier behind step 3)
    stance += (unsigned)__popcll(f);
    tds += (unsigned)__popcll(td);
    los += (unsigned)__popcll(lo);
    if (td != 0ull) {
      const unsigned lowest = (unsigned)(w * 64 + __ffsll((long long)td) - 1);
      const int highest = w * 64 + 63 - __clzll((long long)td);
      first_td = lowest < first_td ? lowest : first_td;
      last_td = highest > last_td ? highest : last_td;
    }
    for (ff_word m = lo; m != 0ull; m &= m - 1ull) {            // a liftoff at u: its stance began behind the last frame without f
      const int u = w * 64 + __ffsll((long long)m) - 1;
      const int zero = ff_last_before(Fl, u, true);
      if (zero >= 0) {
        const unsigned n = (unsigned)(u - zero - 1);
        st_n += 1u; st_sum += n; st_max = n > st_max ? n : st_max;
      }
    }
    for (ff_word m = td; m != 0ull; m &= m - 1ull) {            // a touchdown at t: its swing began behind the last frame with f
      const int t = w * 64 + __ffsll((long long)m) - 1;
      const int one = ff_last_before(Fl, t, false);
      if (one >= 0) {
        const unsigned n = (unsigned)(t - one - 1);
        sw_n += 1u; sw_sum += n; sw_max = n > sw_max ? n : sw_max;
      }
    }
    if (a.support) {
      const ff_word f0 = Fw[w], f1 = Fw[W + w], f2 = Fw[2 * W + w], f3 = Fw[3 * W + w];
      for (int q = 0; q < 4; q++) {
        const int p = 4 * leg + q;
        const ff_word m = ((p & 1) ? f0 : ~f0) & ((p & 2) ? f1 : ~f1) & ((p & 4) ? f2 : ~f2) & ((p & 8) ? f3 : ~f3) & vm;
        sup[q] += (unsigned)__popcll(m);
      }
    }
  }
  __syncthreads();

  // 5. phase of legs 1 .. 3 against leg 0, the gait diagram
  if (bins > 0 && leg != 0) {
    for (int w = tid >> 2; w < W; w += threads >> 2)
      for (ff_word m = Xl[w]; m != 0ull; m &= m - 1ull) {
        const int t = w * 64 + __ffsll((long long)m) - 1;
        const int ta = ff_last_before(Xw, t + 1, false), tb = ff_first_after(Xw, t, W);
        if (ta >= 0 && tb >= 0) atomicAdd(&phase_s[(leg - 1) * IRRL_EVAL_FOOTFALL_MAX_BINS + irrl_eval_footfall_phase_bin(t, ta, tb, bins)], 1u);
      }
  }
  if (a.pattern)
    for (int i = tid; i < T; i += threads) {
      unsigned p = 0u;
      if (i < Te)
        for (int l = 0; l < 4; l++) p |= (unsigned)((Fw[l * W + (i >> 6)] >> (i & 63)) & 1ull) << l;
      a.pattern[(size_t)i * (size_t)N + (size_t)e] = (uint8_t)p;
    }

  // 6. the counters: the lanes of a leg, then the waves
  unsigned v[FF_C] = {0u, raw_stance, raw_td, stance, tds, los, first_td, (unsigned)(last_td + 1), st_n, st_sum, st_max, sw_n, sw_sum, sw_max};
  for (int c = 0; c < FF_C; c++) {                             // (LAST_TD travels as index + 1, 0 = none: an unsigned maximum)
    const bool is_min = c == IRRL_EVAL_FOOTFALL_FIRST_TD;
    const bool is_max = c == IRRL_EVAL_FOOTFALL_LAST_TD || c == IRRL_EVAL_FOOTFALL_STANCE_MAX || c == IRRL_EVAL_FOOTFALL_SWING_MAX;
    for (int d = 32; d >= 4; d >>= 1) {
      const unsigned o = __shfl_xor(v[c], d, 64);
      v[c] = is_min ? (o < v[c] ? o : v[c]) : is_max ? (o > v[c] ? o : v[c]) : v[c] + o;
    }
    if (lane < 4) part_s[wave][leg][c] = v[c];
  }
  for (int q = 0; q < 4; q++) {
    for (int d = 32; d >= 4; d >>= 1) sup[q] += __shfl_xor(sup[q], d, 64);
    if (lane < 4) sup_s[wave][4 * leg + q] = sup[q];
  }
  __syncthreads();
  for (int o = tid; o < 4 * FF_C; o += threads) {
    const int l = o / FF_C, c = o % FF_C;
    const bool is_min = c == IRRL_EVAL_FOOTFALL_FIRST_TD;
    const bool is_max = c == IRRL_EVAL_FOOTFALL_LAST_TD || c == IRRL_EVAL_FOOTFALL_STANCE_MAX || c == IRRL_EVAL_FOOTFALL_SWING_MAX;
    unsigned t = is_min ? IRRL_EVAL_FOOTFALL_NONE : 0u;
    for (int w = 0; w < waves; w++) {
      const unsigned x = part_s[w][l][c];
      t = is_min ? (x < t ? x : t) : is_max ? (x > t ? x : t) : t + x;
    }
    if (c == IRRL_EVAL_FOOTFALL_FRAMES) t = (unsigned)Te;
    if (c == IRRL_EVAL_FOOTFALL_LAST_TD) t = t - 1u;           // 0 - 1 = 0xFFFFFFFF: none
    a.counts[((size_t)e * 4 + (size_t)l) * FF_C + (size_t)c] = t;
  }
  if (a.support)
    for (int p = tid; p < 16; p += threads) {
      unsigned t = 0u;
      for (int w = 0; w < waves; w++) t += sup_s[w][p];
      a.support[(size_t)e * 16 + (size_t)p] = t;
    }
  if (bins > 0)
    for (int o = tid; o < 3 * bins; o += threads)
      a.phase[(size_t)e * 3 * (size_t)bins + (size_t)o] = phase_s[(o / bins) * IRRL_EVAL_FOOTFALL_MAX_BINS + o % bins];
}

hipError_t irrl_eval_footfall_launch(const FootfallArgs &a, hipStream_t stream) {
  const int W = irrl_eval_footfall_words(a.T);
  const int threads = 4 * W <= 256 ? 64 : 256;
  const size_t lds = (size_t)12 * (size_t)W * sizeof(ff_word);    // 24 KB at T = 16384
  hipLaunchKernelGGL(irrl_eval_footfall_kernel, dim3((unsigned)a.N), dim3((unsigned)threads), lds, stream, a);
  return hipGetLastError();
}

#define MP_THREADS 256
#define MP_WAVES (MP_THREADS / 64)
#define MP_CHUNK 64
#define MP_C IRRL_EVAL_MOTOR_COUNTS

__global__ __launch_bounds__(MP_THREADS) void irrl_eval_motor_plane_kernel(const MotorPlaneArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mp_lds[];   // fold f64 [period][3] | hist u32 [t_bins][w_bins]
  __shared__ int te_s[MP_CHUNK];
  __shared__ unsigned part_s[MP_WAVES][MP_C];
  const int T = a.T, N = a.N, R = a.R;
  const int c = (int)blockIdx.x / 12, j = (int)blockIdx.x % 12;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int period = a.fold ? a.spec.period : 0;
  const int tb = a.hist ? a.spec.t_bins : 0, wb = a.hist ? a.spec.w_bins : 0;
  const int cells = tb * wb;
  double *fold_s = reinterpret_cast<double *>(mp_lds);
  unsigned *hist_s = reinterpret_cast<unsigned *>(mp_lds + (size_t)period * 3 * sizeof(double));
  for (int i = tid; i < period * 3; i += MP_THREADS) fold_s[i] = 0.0;
  for (int i = tid; i < cells; i += MP_THREADS) hist_s[i] = 0u;

  unsigned cnt[MP_C] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (int r0 = 0; r0 < R; r0 += MP_CHUNK) {
    const int nr = R - r0 < MP_CHUNK ? R - r0 : MP_CHUNK;
    const size_t env0 = (size_t)c * (size_t)R + (size_t)r0;
    const int pairs = nr * T;                                   // <= 64 x 16384
    __syncthreads();                                            // (the last chunk's walk has read te_s; the zeroed LDS is visible)
    if (tid < nr) te_s[tid] = T;
    __syncthreads();
    if (a.rec_done)
      for (int idx = tid; idx < pairs; idx += MP_THREADS) {
        const int i = idx / nr, rr = idx - i * nr;
        const size_t row = (size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i);
        if (a.rec_done[row * (size_t)N + env0 + (size_t)rr] != 0) atomicMin(&te_s[rr], i);
      }
    __syncthreads();
    for (int idx = tid; idx < pairs; idx += MP_THREADS) {
      const int i = idx / nr, rr = idx - i * nr;
      if (i >= te_s[rr]) continue;
      const size_t row = (size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i);
      const float *g = a.rec_gait + (row * (size_t)N + env0 + (size_t)rr) * IRRL_EVAL_GAIT_REC_DIM;
      double m, w;
      if (!irrl_eval_motor_sample(g[j], g[12 + j], j, a.spec.knee_ratio, &m, &w)) continue;
      const unsigned bits = irrl_eval_motor_classes(m, w, a.spec);
      cnt[0] += 1u;
      for (int k = 1; k < MP_C; k++) cnt[k] += (bits >> (k - 1)) & 1u;
      if (cells > 0) {
        const int bt = irrl_eval_ensemble_bin(m, a.spec.t_lo, a.spec.t_hi, tb), bw = irrl_eval_ensemble_bin(w, a.spec.w_lo, a.spec.w_hi, wb);
        if (bt >= 0 && bw >= 0) atomicAdd(&hist_s[bt * wb + bw], 1u);
      }
    }
    for (int p = tid; p < period; p += MP_THREADS) {           // thread p alone touches fold_s[p]: robots in order, frames in order
      double n = fold_s[p * 3], sm = fold_s[p * 3 + 1], sw = fold_s[p * 3 + 2];
      for (int rr = 0; rr < nr; rr++) {
        const int te = te_s[rr];
        for (int i = p; i < te; i += period) {
          const size_t row = (size_t)irrl_eval_recurrence_row(a.frame_first, a.frame_every, i);
          const float *g = a.rec_gait + (row * (size_t)N + env0 + (size_t)rr) * IRRL_EVAL_GAIT_REC_DIM;
          double m, w;
          if (!irrl_eval_motor_sample(g[j], g[12 + j], j, a.spec.knee_ratio, &m, &w)) continue;
          n = n + 1.0;
          sm = sm + m;
          sw = sw + w;
        }
      }
      fold_s[p * 3] = n; fold_s[p * 3 + 1] = sm; fold_s[p * 3 + 2] = sw;
    }
  }

  for (int k = 0; k < MP_C; k++) {
    for (int d = 32; d > 0; d >>= 1) cnt[k] += __shfl_xor(cnt[k], d, 64);
    if (lane == 0) part_s[wave][k] = cnt[k];
  }
  __syncthreads();
  const size_t cj = (size_t)c * 12 + (size_t)j;
  if (tid < MP_C) {
    unsigned t = 0u;
    for (int w = 0; w < MP_WAVES; w++) t += part_s[w][tid];
    a.counts[cj * MP_C + (size_t)tid] = t;
  }
  for (int i = tid; i < cells; i += MP_THREADS) a.hist[cj * (size_t)cells + (size_t)i] = hist_s[i];
  for (int i = tid; i < period * 3; i += MP_THREADS) a.fold[cj * (size_t)period * 3 + (size_t)i] = fold_s[i];
}

hipError_t irrl_eval_motor_plane_launch(const MotorPlaneArgs &a, hipStream_t stream) {
  const int period = a.fold ? a.spec.period : 0;
  const int cells = a.hist ? a.spec.t_bins * a.spec.w_bins : 0;
  const size_t lds = (size_t)period * 3 * sizeof(double) + (size_t)cells * sizeof(unsigned);   // at most 24 KB + 16 KB
  hipLaunchKernelGGL(irrl_eval_motor_plane_kernel, dim3((unsigned)a.C * 12u), dim3(MP_THREADS), lds, stream, a);
  return hipGetLastError();
}
