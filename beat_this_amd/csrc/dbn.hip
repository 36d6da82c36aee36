// DBN beat / downbeat decoding (Postprocessor(type="dbn"), reference postprocessor.py:28-37,138-173): a re-statement of
// madmom's DBNDownBeatTrackingProcessor -- bar state spaces for 3 and 4 beats per bar, tempo transitions between beats,
// the RNN downbeat observation model, float64 Viterbi with madmom's evaluation order and tie rules, HMM choice and the
// `correct` peak step.  DESIGN.md section 9 has the algorithm and the kernel shape.
//
// Three launches per ragged batch: (1) one workgroup per track: sigmoid / combined activation / threshold trim / log
// densities in fp64; (2) one workgroup per (track, HMM): the whole Viterbi recursion with both value vectors in LDS, one
// barrier per frame; (3) one wave per track: HMM choice, backtracking by beats (not frames) and the peak per beat range.
// The value path is plain IEEE fp64 add / compare: this file is compiled with -ffp-contract=off (and says so below).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/beat_this_amd.h"

#pragma clang fp contract(off)

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

constexpr int MAX_K = 255;          // intervals (backpointers are uint8 interval indices)
constexpr int MAX_HMM = 4;
constexpr int MAX_BEATS = 16;
constexpr int MAX_STATES = 8192;    // per HMM: two fp64 vectors = 128 KiB of LDS
constexpr int MAX_NNZ = 1536;       // nonzero tempo transitions per beat boundary
constexpr int NT = 1024;            // Viterbi threads per workgroup
constexpr int PER = MAX_STATES / NT;
constexpr uint32_t MAGIC = 0x314e4244u;   // "DBN1"

// The table blob of bt_dbn_tables (layout documented in include/beat_this_amd.h).
struct Tables {
  int32_t magic, K, n_hmm, spb, nnz, reserved;
  int32_t beats[MAX_HMM], num_states[MAX_HMM];
  double init[MAX_HMM];       // log(1 / num_states)
  double obs_norm;            // observation_lambda - 1
  double threshold;
  int32_t intervals[256];
  int32_t first[256];         // first state of interval j inside one beat
  int32_t band_ptr[258];      // transitions INTO the first state of interval j: entries band_ptr[j] .. band_ptr[j+1]-1
  int32_t band_from[MAX_NNZ]; // from-interval of each entry, ascending inside a band
  double logp[MAX_NNZ];       // log transition probability of each entry
  uint8_t cnt[MAX_BEATS][256];// leading states of interval j in beat b whose observation pointer is >= 1
};
static_assert(offsetof(Tables, logp) == 9328 && sizeof(Tables) == 25712, "bt_dbn_tables layout (beat_this_amd.h)");

__host__ __device__ inline bool nan_(double x) { return x != x; }

// numpy argmax order: the first NaN wins, then the largest value, then the lowest index
__host__ __device__ inline bool argmax_better(double a, int ia, double b, int ib) {
  if (nan_(a) || nan_(b)) return nan_(a) && (!nan_(b) || ia < ib);
  return a > b || (a == b && ia < ib);
}

// madmom's inner loop for a state with one predecessor of log probability 0: max(-inf, prev + 0) with a strict '>',
// then + the observation
__host__ __device__ inline double shift_step(double prev, double d) {
  double cur = -INFINITY;
  const double tp = prev + 0.0;
  if (tp > cur) cur = tp;
  return cur + d;
}

// combined_act of one frame (postp_dbn / _postp_dbn_item): sigmoid in fp64, squeezed into [eps/2, 1 - eps/2]
__host__ __device__ inline void combined_act(double lb, double ld, double& a0, double& a1) {
  const double eps = 1e-5;
  double bp = 1.0 / (1.0 + exp(-lb));
  double dp = 1.0 / (1.0 + exp(-ld));
  bp = bp * (1.0 - eps) + eps / 2;
  dp = dp * (1.0 - eps) + eps / 2;
  const double x = bp - dp;
  a0 = x < eps / 2 ? eps / 2 : x;   // np.maximum (a NaN stays NaN)
  a1 = dp;
}

__host__ __device__ inline void log_densities(const Tables& tb, double a0, double a1, double* d) {
  d[0] = log((1.0 - (a0 + a1)) / tb.obs_norm);
  d[1] = log(a0);
  d[2] = log(a1);
}

__host__ __device__ inline int interval_of(const Tables& tb, int r) {
  int j = 0;
  while (j + 1 < tb.K && tb.first[j + 1] <= r) ++j;
  return j;
}

// Walk the Viterbi path back from (frame T-1, state end_state) one beat at a time.  Every state that is not the first of
// its interval has the single predecessor state - 1, so the path inside one interval is a straight chain; only the first
// states have stored backpointers (bp[t][beat][interval] = from-interval).  seg(f0, f1, b, j, start) reports frames
// f0..f1 spent in interval j of beat b, the chain's first state sitting at frame `start` (< 0 if the path began inside it).
template <class F>
__host__ __device__ void backtrack(const Tables& tb, int nb, const uint8_t* bp, int T, int end_state, F&& seg) {
  const int K = tb.K;
  int t = T - 1;
  int b = end_state / tb.spb;
  int j = interval_of(tb, end_state - b * tb.spb);
  int k = end_state - b * tb.spb - tb.first[j];
  for (;;) {
    const int start = t - k;
    seg(start > 0 ? start : 0, t, b, j, start);
    if (start <= 0) break;
    j = bp[((size_t)start * nb + b) * K + j];
    b = (b == 0 ? nb : b) - 1;
    k = tb.intervals[j] - 1;
    t = start - 1;
  }
}

// one beat range (frames lo .. hi-1 of the trimmed activation) -> the frame of the largest activation value
__host__ __device__ inline int range_peak(const double* act, int lo, int hi) {
  int best = 2 * lo;
  for (int i = 2 * lo + 1; i < 2 * hi; ++i)
    if (argmax_better(act[i], i, act[best], best)) best = i;
  return best / 2;   // (np.argmax(act[lo:hi]) // 2 + lo: best is already absolute)
}

// the `correct` step over a decoded path: beat ranges (pointer >= 1), one peak each -> rows (frame + offset, beat number),
// written backwards from rows_end (the path is walked from its end); returns the row count
__host__ __device__ inline int correct_rows(const Tables& tb, int nb, const uint8_t* bp, int T, int end_state,
                                            const double* act, int offset, int32_t* rows_end) {
  int n = 0;
  backtrack(tb, nb, bp, T, end_state, [&](int f0, int f1, int b, int j, int start) {
    const int hi = std::min(f1 + 1, start + (int)tb.cnt[b][j]);
    if (hi > f0) {
      ++n;
      rows_end[-2 * n] = range_peak(act, f0, hi) + offset;
      rows_end[-2 * n + 1] = b + 1;
    }
  });
  return n;
}

// index of the HMM with the largest log probability (np.argmax over the HMMs: the first wins ties)
__host__ __device__ inline int best_hmm(const double* logp, int n_hmm) {
  int h = 0;
  for (int i = 1; i < n_hmm; ++i)
    if (argmax_better(logp[i], i, logp[h], h)) h = i;
  return h;
}

// ----------------------------------------------------------------------------------------------------------------------
// tables (host)

// np.sum of one row of a C-contiguous array (numpy's pairwise summation, 8 accumulators)
double np_sum(const double* a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  if (n <= 128) {
    double r[8];
    for (int i = 0; i < 8; ++i) r[i] = a[i];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int q = 0; q < 8; ++q) r[q] += a[i + q];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_sum(a, n2) + np_sum(a + n2, n - n2);
}

// BeatStateSpace intervals: arange(round(min), round(max) + 1), or the log-spaced set when that has more than num_tempi
std::vector<int> beat_intervals(double min_i, double max_i, int num_tempi) {
  std::vector<int> iv;
  for (double x = std::nearbyint(min_i); x <= std::nearbyint(max_i); x += 1.0) iv.push_back((int)x);
  if (num_tempi > 0 && num_tempi < (int)iv.size()) {
    const double a = std::log2(min_i), b = std::log2(max_i);
    for (int n = num_tempi;; ++n) {
      std::vector<int> u;
      const double step = (b - a) / (n - 1);
      for (int i = 0; i < n; ++i) {
        const double y = (n > 1 && i == n - 1) ? b : (n > 1 ? i * step + a : a);
        u.push_back((int)std::nearbyint(std::pow(2.0, y)));
      }
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
      iv = u;
      if ((int)iv.size() >= num_tempi) break;
    }
  }
  return iv;
}

int build_tables(double fps, double min_bpm, double max_bpm, int num_tempi, double transition_lambda,
                 double observation_lambda, double threshold, const int32_t* beats, int n_hmm, Tables& tb) {
  auto err = [](const std::string& m) { return bt_set_error_external(BT_ERR_ARG, m.c_str()); };
  if (!(fps > 0) || !(min_bpm > 0) || !(max_bpm > min_bpm) || !(transition_lambda > 0) || !(observation_lambda > 1) ||
      !(threshold >= 0) || !beats || n_hmm < 1 || n_hmm > MAX_HMM)
    return err("bt_dbn_tables: bad parameters");
  std::memset(&tb, 0, sizeof tb);
  const double min_i = 60. * fps / max_bpm, max_i = 60. * fps / min_bpm;
  const std::vector<int> iv = beat_intervals(min_i, max_i, num_tempi);
  const int K = (int)iv.size();
  if (K < 1 || iv[0] < 1) return err("bt_dbn_tables: no beat intervals for these parameters");
  if (K > MAX_K) return err("bt_dbn_tables: " + std::to_string(K) + " beat intervals, the DBN kernel supports at most " +
                            std::to_string(MAX_K));
  tb.magic = (int32_t)MAGIC;
  tb.K = K;
  tb.n_hmm = n_hmm;
  int spb = 0;
  for (int j = 0; j < K; ++j) {
    tb.intervals[j] = iv[j];
    tb.first[j] = spb;
    spb += iv[j];
  }
  tb.spb = spb;
  for (int h = 0; h < n_hmm; ++h) {
    if (beats[h] < 1 || beats[h] > MAX_BEATS) return err("bt_dbn_tables: beats per bar must be 1.." + std::to_string(MAX_BEATS));
    tb.beats[h] = beats[h];
    tb.num_states[h] = beats[h] * spb;
    if (tb.num_states[h] > MAX_STATES)
      return err("bt_dbn_tables: " + std::to_string(tb.num_states[h]) + " states for " + std::to_string(beats[h]) +
                 " beats per bar; the DBN kernel keeps at most " + std::to_string(MAX_STATES) + " in LDS");
    tb.init[h] = std::log(1.0 / tb.num_states[h]);
  }
  tb.obs_norm = observation_lambda - 1.0;
  tb.threshold = threshold;
  // exponential_transition(from, to, lambda): rows = from, p = exp(-lambda |to/from - 1|), p <= eps(1) -> 0, rows sum to 1
  std::vector<double> p((size_t)K * K);
  for (int f = 0; f < K; ++f) {
    for (int t = 0; t < K; ++t) {
      const double ratio = (double)iv[t] / (double)iv[f];
      double v = std::exp(-transition_lambda * std::fabs(ratio - 1.0));
      p[(size_t)f * K + t] = v <= 2.220446049250313e-16 ? 0.0 : v;
    }
    const double s = np_sum(&p[(size_t)f * K], K);
    for (int t = 0; t < K; ++t) p[(size_t)f * K + t] /= s;
  }
  int nnz = 0;
  for (int t = 0; t < K; ++t) {
    tb.band_ptr[t] = nnz;
    int prev = -2;
    for (int f = 0; f < K; ++f) {
      const double v = p[(size_t)f * K + t];
      if (v == 0.0) continue;
      if (nnz >= MAX_NNZ) return err("bt_dbn_tables: more than " + std::to_string(MAX_NNZ) + " tempo transitions");
      if (prev >= 0 && f != prev + 1) return err("bt_dbn_tables: tempo transitions into one interval are not contiguous");
      if (std::isnan(v)) return err("bt_dbn_tables: NaN transition probability");
      tb.band_from[nnz] = f;
      tb.logp[nnz] = std::log(v);
      prev = f;
      ++nnz;
    }
    if (tb.band_ptr[t] == nnz) return err("bt_dbn_tables: an interval cannot be reached");
  }
  tb.band_ptr[K] = nnz;
  tb.nnz = nnz;
  // observation pointers: 2 where position < 1/lambda, else 1 where position % 1 < 1/lambda, else 0 -- they must be a
  // leading run of each interval, shorter than it (the beat ranges of the `correct` step then never span two beats)
  const double thr = 1. / observation_lambda;
  int max_beats = 0;
  for (int h = 0; h < n_hmm; ++h) max_beats = std::max(max_beats, beats[h]);
  for (int b = 0; b < max_beats; ++b)
    for (int j = 0; j < K; ++j) {
      const double step = 1.0 / iv[j];
      int c = 0;
      bool run = true;
      for (int k = 0; k < iv[j]; ++k) {
        const double pos = k * step + b;
        const bool on = b == 0 ? pos < thr : std::fmod(pos, 1.0) < thr;
        if (on && !run) return err("bt_dbn_tables: observation pointers are not a leading run of an interval");
        if (on) ++c; else run = false;
      }
      if (c >= iv[j]) return err("bt_dbn_tables: observation_lambda too small for the shortest interval");
      tb.cnt[b][j] = (uint8_t)c;
    }
  return BT_OK;
}

// ----------------------------------------------------------------------------------------------------------------------
// workspace layout of bt_dbn_decode / bt_dbn_viterbi

struct Ws {
  size_t info, logp, state, act, dens, bp, total;
};

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

__host__ __device__ inline int beat_sum(const Tables& tb) {
  int s = 0;
  for (int h = 0; h < tb.n_hmm; ++h) s += tb.beats[h];
  return s;
}

Ws ws_layout(const Tables& tb, int n, int64_t frames) {
  Ws w;
  size_t off = 0;
  w.info = off; off = al(off + (size_t)n * 4 * sizeof(int32_t));
  w.logp = off; off = al(off + (size_t)n * MAX_HMM * sizeof(double));
  w.state = off; off = al(off + (size_t)n * MAX_HMM * sizeof(int32_t));
  w.act = off; off = al(off + (size_t)frames * 2 * sizeof(double));
  w.dens = off; off = al(off + (size_t)frames * 3 * sizeof(double));
  w.bp = off; off = al(off + (size_t)frames * beat_sum(tb) * tb.K);
  w.total = off;
  return w;
}

// ----------------------------------------------------------------------------------------------------------------------
// kernels

// (1) per track: combined activation, threshold trim, log densities.  info[k] = {first, trimmed length, frame_off, span}
__global__ __launch_bounds__(1024) void dbn_front_kernel(const Tables* __restrict__ tbp, const void* __restrict__ logits,
                                                         int f64, const int32_t* __restrict__ spans,
                                                         int32_t* __restrict__ info, double* __restrict__ act,
                                                         double* __restrict__ dens) {
  const Tables& tb = *tbp;
  const int k = blockIdx.x;
  const int bo = spans[4 * k], dof = spans[4 * k + 1], len = spans[4 * k + 2], foff = spans[4 * k + 3];
  __shared__ int s_min, s_max;
  if (threadIdx.x == 0) { s_min = 0x7fffffff; s_max = -1; }
  __syncthreads();
  auto load = [&](int i) { return f64 ? ((const double*)logits)[i] : (double)((const float*)logits)[i]; };
  int lmin = 0x7fffffff, lmax = -1;
  for (int f = threadIdx.x; f < len; f += blockDim.x) {
    double a0, a1;
    combined_act(load(bo + f), load(dof + f), a0, a1);
    if (a0 >= tb.threshold || a1 >= tb.threshold) { lmin = min(lmin, f); lmax = max(lmax, f); }
  }
  if (lmax >= 0) { atomicMin(&s_min, lmin); atomicMax(&s_max, lmax); }
  __syncthreads();
  // madmom: `if idx.any()` -- a lone frame 0 above the threshold counts as none
  const int first = s_max > 0 ? s_min : 0;
  const int n = s_max > 0 ? s_max + 1 - first : 0;
  if (threadIdx.x == 0) {
    info[4 * k] = first;
    info[4 * k + 1] = n;
    info[4 * k + 2] = foff;
    info[4 * k + 3] = len;
  }
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    double a0, a1, d[3];
    combined_act(load(bo + first + t), load(dof + first + t), a0, a1);
    log_densities(tb, a0, a1, d);
    const size_t r = (size_t)foff + t;
    act[2 * r] = a0;
    act[2 * r + 1] = a1;
    dens[3 * r] = d[0];
    dens[3 * r + 1] = d[1];
    dens[3 * r + 2] = d[2];
  }
}

// (2) one workgroup per (track, HMM): the Viterbi recursion over all frames.  info == nullptr: one sequence of n_direct
// frames at dens, HMM hmm_direct (bt_dbn_viterbi).
__global__ __launch_bounds__(NT) void dbn_viterbi_kernel(const Tables* __restrict__ tbp, const double* __restrict__ dens,
                                                         const int32_t* __restrict__ info, int n_direct, int hmm_direct,
                                                         uint8_t* __restrict__ bp_base, double* __restrict__ res_logp,
                                                         int32_t* __restrict__ res_state) {
  __shared__ double v[2][MAX_STATES];
  __shared__ double s_lp[MAX_NNZ];
  __shared__ int16_t s_last[MAX_NNZ];   // last state (inside one beat) of each entry's from-interval
  __shared__ uint8_t s_from[MAX_NNZ];
  __shared__ int s_ridx[NT];
  __shared__ int s_band[257];
  const Tables& tb = *tbp;
  const int k = blockIdx.x;
  const int h = info ? (int)blockIdx.y : hmm_direct;
  if (h >= tb.n_hmm) return;
  const int K = tb.K, spb = tb.spb, nb = tb.beats[h], S = tb.num_states[h];
  int T = n_direct;
  size_t foff = 0, bpoff = 0;
  if (info) {
    T = info[4 * k + 1];
    foff = (size_t)info[4 * k + 2];
    int pre = 0;
    for (int q = 0; q < h; ++q) pre += tb.beats[q];
    bpoff = foff * beat_sum(tb) * K + (size_t)pre * info[4 * k + 3] * K;
  }
  const double* d_t = dens + 3 * foff;
  uint8_t* bp = bp_base + bpoff;
  for (int j = threadIdx.x; j <= K; j += NT) s_band[j] = tb.band_ptr[j];
  for (int e = threadIdx.x; e < tb.nnz; e += NT) {
    const int f = tb.band_from[e];
    s_lp[e] = tb.logp[e];
    s_last[e] = (int16_t)(tb.first[f] + tb.intervals[f] - 1);
    s_from[e] = (uint8_t)f;
  }
  // the states of this thread: s = tid + m NT.  desc: bits 0-1 observation pointer, bit 2 first state of an interval,
  // bits 3-10 interval; base: s - 1 for a shift state, the previous beat's offset for a first state
  int desc[PER], base[PER];
#pragma unroll
  for (int m = 0; m < PER; ++m) {
    const int s = threadIdx.x + m * NT;
    desc[m] = 0;
    base[m] = 0;
    if (s < S) {
      const int b = s / spb, r = s - b * spb;
      const int j = interval_of(tb, r), kk = r - tb.first[j];
      const int ptr = kk < tb.cnt[b][j] ? (b == 0 ? 2 : 1) : 0;
      desc[m] = ptr | (kk == 0 ? 4 : 0) | (j << 3) | (b << 11);
      base[m] = kk == 0 ? ((b == 0 ? nb : b) - 1) * spb : s - 1;
      v[0][s] = tb.init[h];
    }
  }
  __syncthreads();
  int cur = 0;
  double d0 = 0, d1 = 0, d2 = 0;
  if (T > 0) { d0 = d_t[0]; d1 = d_t[1]; d2 = d_t[2]; }
  for (int t = 0; t < T; ++t) {
    double n0 = 0, n1 = 0, n2 = 0;
    if (t + 1 < T) { n0 = d_t[3 * (t + 1)]; n1 = d_t[3 * (t + 1) + 1]; n2 = d_t[3 * (t + 1) + 2]; }
    const double* pv = v[cur];
    double* nv = v[cur ^ 1];
#pragma unroll
    for (int m = 0; m < PER; ++m) {
      const int s = threadIdx.x + m * NT;
      if (s < S) {
        const int ds = desc[m];
        const double d = (ds & 3) == 0 ? d0 : ((ds & 3) == 1 ? d1 : d2);
        if (ds & 4) {
          const int j = (ds >> 3) & 255, e0 = s_band[j], e1 = s_band[j + 1];
          double best = -INFINITY;
          int win = s_from[e0];
          for (int e = e0; e < e1; ++e) {
            const double tp = pv[base[m] + s_last[e]] + s_lp[e];
            if (tp > best) { best = tp; win = s_from[e]; }
          }
          nv[s] = best + d;
          bp[((size_t)t * nb + (ds >> 11)) * K + j] = (uint8_t)win;
        } else {
          nv[s] = shift_step(pv[base[m]], d);
        }
      }
    }
    __syncthreads();
    cur ^= 1;
    d0 = n0; d1 = n1; d2 = n2;
  }
  // argmax of the final vector (numpy order), reduced through the free buffer
  double bv = -INFINITY;
  int bi = -1;
  for (int m = 0; m < PER; ++m) {
    const int s = threadIdx.x + m * NT;
    if (s < S && (bi < 0 || argmax_better(v[cur][s], s, bv, bi))) { bv = v[cur][s]; bi = s; }
  }
  double* rv = v[cur ^ 1];
  rv[threadIdx.x] = bv;
  s_ridx[threadIdx.x] = bi;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const int o = threadIdx.x + w;
      if (s_ridx[o] >= 0 && (s_ridx[threadIdx.x] < 0 || argmax_better(rv[o], s_ridx[o], rv[threadIdx.x], s_ridx[threadIdx.x]))) {
        rv[threadIdx.x] = rv[o];
        s_ridx[threadIdx.x] = s_ridx[o];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    res_logp[k * MAX_HMM + h] = T > 0 ? rv[0] : -INFINITY;
    res_state[k * MAX_HMM + h] = s_ridx[0];
  }
}

// (3) per track: HMM choice, backtracking, the `correct` step.  out = [count per track | rows]: track k's rows
// (frame, beat number) at out + n_tracks + 2 frame_off[k], at most span[k] of them.
__global__ __launch_bounds__(64) void dbn_finish_kernel(const Tables* __restrict__ tbp, const int32_t* __restrict__ info,
                                                        const double* __restrict__ act, const uint8_t* __restrict__ bp_base,
                                                        const double* __restrict__ res_logp, const int32_t* __restrict__ res_state,
                                                        int n_tracks, int32_t* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const Tables& tb = *tbp;
  const int k = blockIdx.x;
  const int first = info[4 * k], T = info[4 * k + 1], foff = info[4 * k + 2], span = info[4 * k + 3];
  int n = 0;
  if (T > 0) {
    const int h = best_hmm(res_logp + k * MAX_HMM, tb.n_hmm);
    if (!isinf(res_logp[k * MAX_HMM + h])) {
      int pre = 0;
      for (int q = 0; q < h; ++q) pre += tb.beats[q];
      const uint8_t* bp = bp_base + (size_t)foff * beat_sum(tb) * tb.K + (size_t)pre * span * tb.K;
      int32_t* rows = out + n_tracks + 2 * (size_t)foff;
      n = correct_rows(tb, tb.beats[h], bp, T, res_state[k * MAX_HMM + h], act + 2 * (size_t)foff, first, rows + 2 * span);
      for (int i = 0; i < 2 * n; ++i) rows[i] = rows[2 * span - 2 * n + i];
    }
  }
  out[k] = n;
}

// bt_dbn_viterbi: the full state path of one sequence
__global__ __launch_bounds__(64) void dbn_path_kernel(const Tables* __restrict__ tbp, int h, int T, const uint8_t* __restrict__ bp,
                                                      const double* __restrict__ res_logp, const int32_t* __restrict__ res_state,
                                                      int32_t* __restrict__ path, double* __restrict__ log_prob) {
  if (threadIdx.x != 0) return;
  const Tables& tb = *tbp;
  const double lp = res_logp[h];
  *log_prob = lp;
  if (T <= 0 || isinf(lp)) return;
  backtrack(tb, tb.beats[h], bp, T, res_state[h], [&](int f0, int f1, int b, int j, int start) {
    for (int f = f0; f <= f1; ++f) path[f] = b * tb.spb + tb.first[j] + (f - start);
  });
}

// ----------------------------------------------------------------------------------------------------------------------
// host decoder (the same recursion, same order)

void viterbi_host(const Tables& tb, int h, const double* dens, int T, std::vector<uint8_t>& bp, double& logp, int& state) {
  const int K = tb.K, spb = tb.spb, nb = tb.beats[h], S = tb.num_states[h];
  std::vector<double> a(S, tb.init[h]), c(S);
  bp.assign((size_t)std::max(T, 0) * nb * K, 0);
  std::vector<int16_t> last(tb.nnz);
  for (int e = 0; e < tb.nnz; ++e) last[e] = (int16_t)(tb.first[tb.band_from[e]] + tb.intervals[tb.band_from[e]] - 1);
  std::vector<uint8_t> ptr(S);
  for (int s = 0; s < S; ++s) {
    const int b = s / spb, j = interval_of(tb, s - b * spb), kk = s - b * spb - tb.first[j];
    ptr[s] = kk < tb.cnt[b][j] ? (b == 0 ? 2 : 1) : 0;
  }
  for (int t = 0; t < T; ++t) {
    const double* d = dens + 3 * (size_t)t;
    for (int b = 0; b < nb; ++b) {
      const int pb = ((b == 0 ? nb : b) - 1) * spb;
      for (int j = 0; j < K; ++j) {
        const int s0 = b * spb + tb.first[j];
        double best = -INFINITY;
        int win = tb.band_from[tb.band_ptr[j]];
        for (int e = tb.band_ptr[j]; e < tb.band_ptr[j + 1]; ++e) {
          const double tp = a[pb + last[e]] + tb.logp[e];
          if (tp > best) { best = tp; win = tb.band_from[e]; }
        }
        c[s0] = best + d[ptr[s0]];
        bp[((size_t)t * nb + b) * K + j] = (uint8_t)win;
        for (int s = s0 + 1; s < s0 + tb.intervals[j]; ++s) c[s] = shift_step(a[s - 1], d[ptr[s]]);
      }
    }
    a.swap(c);
  }
  state = 0;
  for (int s = 1; s < S; ++s)
    if (argmax_better(a[s], s, a[state], state)) state = s;
  logp = T > 0 ? a[state] : -INFINITY;
}

// madmom's process() on a (T, 2) activation -> rows (frame, beat number)
int decode_host(const Tables& tb, const double* act, int64_t n, int32_t* rows) {
  int lo = -1, hi = -1;
  for (int64_t f = 0; f < n; ++f)
    if (act[2 * f] >= tb.threshold || act[2 * f + 1] >= tb.threshold) { if (lo < 0) lo = (int)f; hi = (int)f; }
  const int first = hi > 0 ? lo : 0, T = hi > 0 ? hi + 1 - first : 0;
  if (T == 0) return 0;
  const double* a = act + 2 * (size_t)first;
  std::vector<double> dens((size_t)T * 3);
  for (int t = 0; t < T; ++t) log_densities(tb, a[2 * t], a[2 * t + 1], &dens[3 * (size_t)t]);
  std::vector<uint8_t> bp[MAX_HMM];
  double logp[MAX_HMM];
  int state[MAX_HMM];
  for (int h = 0; h < tb.n_hmm; ++h) viterbi_host(tb, h, dens.data(), T, bp[h], logp[h], state[h]);
  const int h = best_hmm(logp, tb.n_hmm);
  if (std::isinf(logp[h])) return 0;
  std::vector<int32_t> tmp(2 * (size_t)T);
  const int m = correct_rows(tb, tb.beats[h], bp[h].data(), T, state[h], a, first, tmp.data() + 2 * (size_t)T);
  std::memcpy(rows, tmp.data() + 2 * ((size_t)T - m), 2 * (size_t)m * sizeof(int32_t));
  return m;
}

const Tables* checked(const void* p) {
  const Tables* tb = (const Tables*)p;
  return tb && (uint32_t)tb->magic == MAGIC ? tb : nullptr;
}

}  // namespace

extern "C" {

int bt_dbn_tables(double fps, double min_bpm, double max_bpm, int num_tempi, double transition_lambda,
                  double observation_lambda, double threshold, const int32_t* beats_per_bar, int n_hmm, void* tables,
                  size_t* bytes) {
  if (!bytes) return bt_set_error_external(BT_ERR_ARG, "bt_dbn_tables: null size");
  if (!tables) {
    *bytes = sizeof(Tables);
    return BT_OK;
  }
  if (*bytes < sizeof(Tables)) return bt_set_error_external(BT_ERR_ARG, "bt_dbn_tables: buffer too small");
  *bytes = sizeof(Tables);
  return build_tables(fps, min_bpm, max_bpm, num_tempi, transition_lambda, observation_lambda, threshold, beats_per_bar,
                      n_hmm, *(Tables*)tables);
}

size_t bt_dbn_workspace_bytes(const void* tables, int n_tracks, int64_t total_frames) {
  const Tables* tb = checked(tables);
  if (!tb || n_tracks < 0 || total_frames < 0) return 0;
  return ws_layout(*tb, n_tracks, total_frames).total;
}

int bt_dbn_decode(void* stream, const void* tables, const void* d_tables, const void* d_logits, int f64,
                  const int32_t* d_spans, int n_tracks, int64_t total_frames, int32_t* d_out, void* d_ws, size_t ws_bytes) {
  const Tables* tb = checked(tables);
  if (!tb || !d_tables || !d_logits || !d_spans || !d_out || !d_ws || n_tracks <= 0 || total_frames < 0 ||
      total_frames > 0x7fffffffL || (f64 != 0 && f64 != 1))
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_dbn_decode");
  const Ws w = ws_layout(*tb, n_tracks, total_frames);
  if (ws_bytes < w.total) return bt_set_error_external(BT_ERR_WORKSPACE, "bt_dbn_decode: workspace too small");
  char* ws = (char*)d_ws;
  hipStream_t s = (hipStream_t)stream;
  const Tables* dt = (const Tables*)d_tables;
  hipLaunchKernelGGL(dbn_front_kernel, dim3(n_tracks), dim3(1024), 0, s, dt, d_logits, f64, d_spans, (int32_t*)(ws + w.info),
                     (double*)(ws + w.act), (double*)(ws + w.dens));
  hipLaunchKernelGGL(dbn_viterbi_kernel, dim3(n_tracks, tb->n_hmm), dim3(NT), 0, s, dt, (const double*)(ws + w.dens),
                     (const int32_t*)(ws + w.info), 0, 0, (uint8_t*)(ws + w.bp), (double*)(ws + w.logp), (int32_t*)(ws + w.state));
  hipLaunchKernelGGL(dbn_finish_kernel, dim3(n_tracks), dim3(64), 0, s, dt, (const int32_t*)(ws + w.info),
                     (const double*)(ws + w.act), (const uint8_t*)(ws + w.bp), (const double*)(ws + w.logp),
                     (const int32_t*)(ws + w.state), n_tracks, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string("bt_dbn_decode: ") + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_dbn_viterbi(void* stream, const void* tables, const void* d_tables, int hmm, const double* d_dens, int64_t n,
                   int32_t* d_path, double* d_log_prob, void* d_ws, size_t ws_bytes) {
  const Tables* tb = checked(tables);
  if (!tb || !d_tables || hmm < 0 || hmm >= tb->n_hmm || n < 0 || n > 0x7fffffffL || (n > 0 && (!d_dens || !d_path)) ||
      !d_log_prob || !d_ws)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_dbn_viterbi");
  // (the bookkeeping of a one-track decode: backpointers of every HMM's size fit)
  const Ws w = ws_layout(*tb, 1, n);
  if (ws_bytes < w.total) return bt_set_error_external(BT_ERR_WORKSPACE, "bt_dbn_viterbi: workspace too small");
  char* ws = (char*)d_ws;
  hipStream_t s = (hipStream_t)stream;
  const Tables* dt = (const Tables*)d_tables;
  hipLaunchKernelGGL(dbn_viterbi_kernel, dim3(1, 1), dim3(NT), 0, s, dt, d_dens, (const int32_t*)nullptr, (int)n, hmm,
                     (uint8_t*)(ws + w.bp), (double*)(ws + w.logp), (int32_t*)(ws + w.state));
  hipLaunchKernelGGL(dbn_path_kernel, dim3(1), dim3(64), 0, s, dt, hmm, (int)n, (const uint8_t*)(ws + w.bp),
                     (const double*)(ws + w.logp), (const int32_t*)(ws + w.state), d_path, d_log_prob);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string("bt_dbn_viterbi: ") + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_dbn_viterbi_host(const void* tables, int hmm, const double* dens, int64_t n, int32_t* path, double* log_prob) {
  const Tables* tb = checked(tables);
  if (!tb || hmm < 0 || hmm >= tb->n_hmm || n < 0 || n > 0x7fffffffL || (n > 0 && (!dens || !path)) || !log_prob)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_dbn_viterbi_host");
  std::vector<uint8_t> bp;
  double lp;
  int state;
  viterbi_host(*tb, hmm, dens, (int)n, bp, lp, state);
  *log_prob = lp;
  if (n > 0 && !std::isinf(lp))
    backtrack(*tb, tb->beats[hmm], bp.data(), (int)n, state, [&](int f0, int f1, int b, int j, int start) {
      for (int f = f0; f <= f1; ++f) path[f] = b * tb->spb + tb->first[j] + (f - start);
    });
  return BT_OK;
}

int bt_dbn_host_act(const void* tables, const double* act, int64_t n, int32_t* rows, int32_t* n_rows) {
  const Tables* tb = checked(tables);
  if (!tb || n < 0 || n > 0x7fffffffL || (n > 0 && (!act || !rows)) || !n_rows)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_dbn_host_act");
  *n_rows = decode_host(*tb, act, n, rows);
  return BT_OK;
}

int bt_dbn_host(const void* tables, const double* beat, const double* downbeat, int64_t n, int32_t* rows, int32_t* n_rows) {
  const Tables* tb = checked(tables);
  if (!tb || n < 0 || n > 0x7fffffffL || (n > 0 && (!beat || !downbeat || !rows)) || !n_rows)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_dbn_host");
  std::vector<double> act(2 * (size_t)n);
  for (int64_t f = 0; f < n; ++f) combined_act(beat[f], downbeat[f], act[2 * f], act[2 * f + 1]);
  *n_rows = decode_host(*tb, act.data(), n, rows);
  return BT_OK;
}

}  // extern "C"
