// Beat-tracking evaluation metrics (the reference's Metrics, pl_module.py:320-339, used by
// launch_scripts/compute_paper_metrics.py): a restatement of mir_eval.beat's trim_beats, f_measure, cemgil and continuity
// (mir_eval 0.7 / 0.8 published algorithm; mir_eval itself is never imported).  DESIGN.md section 10 has the algorithm, the
// kernel shape and what is and is not pinned.
//
// Device: two launches per ragged batch.  (1) One single-wave workgroup per (track, job): jobs 0..4 are the reference
// variations of _get_reference_beat_variations (original, off-beat, double, half odd, half even) and compute Cemgil's sum
// (binary search per reference beat + a wave reduction) and the continuity counts (nearest annotation per estimate by binary
// search, the "used annotation" rule as a segmented scan over runs of equal nearest, the longest run of successes as a
// segmented max-run scan, both on 64-bit ballots); job 5 validates both arrays and computes the F-measure matching (greedy over
// independent window segments, one lane per segment).  Each job leaves WS_SLOT doubles in the workspace.  (2) One thread per
// track combines them into the 12-double output row.
// Host: bt_beat_metrics_host runs mir_eval's sequential loops (the literal used-annotation array) on the same helpers.
// Every fp64 operation is the one numpy performs, in its order: this file is compiled with -ffp-contract=off.
//
// The rest of mir_eval.beat (goto, p_score, information_gain) has kernels of its own further down,
// bt_beat_metrics_ext: the same two-launch shape with four jobs per track, and bt_beat_metrics_ext_host beside it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/beat_this_amd.h"

#pragma clang fp contract(off)

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

constexpr int NJOB = 6;          // per track: 5 reference variations + the validation / F-measure job
constexpr int WS_SLOT = 8;       // doubles per (track, job) in the workspace
constexpr double MAX_TIME = 30000.0;   // mir_eval.util.validate_events' max_time
constexpr int COLS = BT_METRICS_COLS;

struct Params {
  double min_time, f_window, sigma, phase_thr, period_thr;
};

// ---- the reference variations (mir_eval.beat._get_reference_beat_variations) -----------------------------------------------
// double tempo = np.interp(arange(0, n - .5, .5), arange(n), r): r[k] at the integers, slope * 0.5 + r[k] in between, where
// slope = (r[k+1] - r[k]) / 1.0 (numpy's interp; not (r[k] + r[k+1]) / 2)
__host__ __device__ inline double midpoint(const double* r, int k) { return (r[k + 1] - r[k]) * 0.5 + r[k]; }

__host__ __device__ inline int var_len(int n, int v) {
  switch (v) {
    case 0: return n;                   // original
    case 1: return n > 0 ? n - 1 : 0;   // off-beat: double[1::2]
    case 2: return n > 0 ? 2 * n - 1 : 0;   // double tempo
    case 3: return (n + 1) / 2;         // half tempo odd: r[::2]
    default: return n / 2;              // half tempo even: r[1::2]
  }
}

struct Var {   // element i of variation v of the (trimmed) reference r
  const double* r;
  int v;
  __host__ __device__ double operator[](int i) const {
    switch (v) {
      case 0: return r[i];
      case 1: return midpoint(r, i);
      case 2: return (i & 1) ? midpoint(r, i >> 1) : r[i >> 1];
      case 3: return r[2 * i];
      default: return r[2 * i + 1];
    }
  }
};

// np.searchsorted(a, x, side="left") / side="right" on a non-decreasing a[0..n)
template <class A>
__host__ __device__ inline int lower_bound(const A& a, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <class A>
__host__ __device__ inline int upper_bound(const A& a, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// np.argmin(np.abs(x - a)) on a non-decreasing a[0..n), n >= 1: the FIRST index of the smallest rounded distance.  Left of the
// insertion point p the distances fl(x - a[k]) are non-increasing in k, right of it fl(a[k] - x) non-decreasing (rounding is
// monotone), so the minimum is a[p-1] or a[p]; rounding can tie several left entries, hence the search for the first of them.
template <class A>
__host__ __device__ inline int nearest(const A& a, int n, double x) {
  const int p = lower_bound(a, n, x);
  if (p == 0) return 0;
  const double dl = x - a[p - 1];
  if (p < n && a[p] - x < dl) return p;
  int lo = 0, hi = p - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x - a[mid] <= dl) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// np.min(np.abs(x - e)) on a non-decreasing e[0..m), m >= 1
__host__ __device__ inline double min_dist(const double* e, int m, double x) {
  const int p = lower_bound(e, m, x);
  double d = INFINITY;
  if (p > 0) d = x - e[p - 1];
  if (p < m) d = fmin(d, e[p] - x);
  return d;
}

// Cemgil's Gaussian: np.exp(-(d**2) / (2.0 * sigma**2))
__host__ __device__ inline double cemgil_term(double d, double sigma) { return exp(-(d * d) / (2.0 * (sigma * sigma))); }

// continuity: whether estimate m (nearest annotation k of variation v[0..nv)) meets the phase and period conditions, with
// mir_eval's branches: the look-forward branch for m == 0 or k == 0 (x[-1] wraps like Python's, a zero reference interval
// fails both conditions), else the look-back branch (numpy fp64 division: x / 0 is inf or NaN, and comparisons with NaN fail)
template <class V>
__host__ __device__ inline bool cont_cond(const V& v, int nv, const double* e, int M, int m, int k, const Params& P) {
  const double d = fabs(e[m] - v[k]);
  double ri, ei;
  if (m == 0 || k == 0) {
    ri = k + 1 < nv ? v[k + 1] - v[k] : v[k] - v[k == 0 ? nv - 1 : k - 1];
    ei = m + 1 < M ? e[m + 1] - e[m] : e[m] - e[m == 0 ? M - 1 : m - 1];
    if (ri == 0) return false;
  } else {
    ri = v[k] - v[k - 1];
    ei = e[m] - e[m - 1];
  }
  return fabs(d / ri) < P.phase_thr && fabs(1.0 - ei / ri) < P.period_thr;
}

// util.f_measure(precision, recall) with beta = 1: (1 + beta**2) * p * r / (beta**2 * p + r), 0 when both are 0
__host__ __device__ inline double f_of(double p, double r) { return p == 0 && r == 0 ? 0.0 : 2.0 * p * r / (1.0 * p + r); }

// mir_eval's validate on the kept part (x >= min_time, trim_beats) of one array: events finite, <= 30000 s, non-decreasing.
// The kept part must be a suffix (true for every sorted array); status bits of the reference array, << 3 for the estimates.
__host__ __device__ inline int check_event(const double* a, int64_t n, int64_t i, double t) {
  const double x = a[i];
  int bits = 0;
  if (!(x - x == 0.0)) bits |= BT_METRICS_NONFINITE;   // (inf - inf and NaN - NaN are NaN)
  if (x >= t) {
    if (x > MAX_TIME) bits |= BT_METRICS_LATE;
    if (i + 1 < n && !(a[i + 1] >= x)) bits |= BT_METRICS_UNSORTED;
  }
  return bits;
}

__host__ __device__ inline void write_row(double* row, double F, double Pr, double Rc, const double* cem, const double* cont,
                                          const double* tot, int n, int M, int status) {
  double cmax = cem[0], amlc = cont[0], amlt = tot[0];
  for (int v = 1; v < 5; ++v) {
    cmax = fmax(cmax, cem[v]);
    amlc = fmax(amlc, cont[v]);
    amlt = fmax(amlt, tot[v]);
  }
  const double vals[9] = {F, Pr, Rc, cem[0], cmax, cont[0], tot[0], amlc, amlt};
  for (int c = 0; c < 9; ++c) row[c] = status ? NAN : vals[c];
  row[9] = n;
  row[10] = M;
  row[11] = status;
}

// ---- device -----------------------------------------------------------------------------------------------------------------
__device__ inline double wave_sum(double x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__device__ inline int wave_sum_i(int x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__device__ inline int wave_max_i(int x) {
  for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
  return x;
}

__device__ inline int wave_or(int x) {
  for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o, 64);
  return x;
}

__device__ inline uint64_t upto(int lane) { return lane == 63 ? ~0ull : (2ull << lane) - 1; }   // bits 0 .. lane

struct Track {
  const double* r;   // trimmed reference, n events
  const double* e;   // trimmed estimates, M events
  int n, M;
  int bad;           // offsets unusable
};

__device__ inline Track track_of(const double* ref, const int64_t* ref_off, const double* est, const int64_t* est_off, int t,
                                 double min_time, int64_t& nr_raw, int64_t& ne_raw) {
  Track k{};
  const int64_t r0 = ref_off[t], r1 = ref_off[t + 1], e0 = est_off[t], e1 = est_off[t + 1];
  nr_raw = r1 - r0;
  ne_raw = e1 - e0;
  if (r0 < 0 || e0 < 0 || nr_raw < 0 || ne_raw < 0 || nr_raw > 0x3fffffff || ne_raw > 0x3fffffff) {
    k.bad = 1;
    nr_raw = ne_raw = 0;
    return k;
  }
  const int sr = lower_bound(ref + r0, (int)nr_raw, min_time), se = lower_bound(est + e0, (int)ne_raw, min_time);
  k.r = ref + r0 + sr;
  k.e = est + e0 + se;
  k.n = (int)nr_raw - sr;
  k.M = (int)ne_raw - se;
  return k;
}

// job v < 5 of a track: Cemgil's sum and the continuity counts of reference variation v -> ws [cemgil, continuous, total,
// nearest-not-monotone flag]
__device__ void variation_job(const Track& k, int v, const Params& P, double* out) {
  const int lane = threadIdx.x;
  const Var var{k.r, v};
  const int nv = var_len(k.n, v), M = k.M;
  double cem = 0.0, cont = 0.0, tot = 0.0;
  int flag = 0;
  if (M > 0 && k.n > 0) {
    double acc = 0.0;
    for (int i = lane; i < nv; i += 64) acc += cemgil_term(min_dist(k.e, M, var[i]), P.sigma);
    cem = wave_sum(acc) / (0.5 * (M + nv));
  }
  if (M > 1 && k.n > 1) {
    // beat m succeeds iff it meets the conditions and no earlier estimate with the same nearest annotation did.  nearest is
    // non-decreasing in m, so those estimates form one run: success = cond && no cond earlier in the run of equal nearest.
    int carry_k = -1, carry_used = 0, carry_run = 0, best = 0, count = 0;
    for (int base = 0; base < M; base += 64) {
      const int m = base + lane;
      const bool valid = m < M;
      const int kk = valid ? nearest(var, nv, k.e[m]) : 0x7fffffff;
      const bool c = valid && cont_cond(var, nv, k.e, M, m, kk, P);
      int prev = __shfl_up(kk, 1, 64);
      if (lane == 0) prev = carry_k;
      if (__any(valid && kk < prev)) flag = 1;
      const uint64_t heads = __ballot(kk != prev), passes = __ballot(c);
      const uint64_t hb = heads & upto(lane);
      const int s = hb ? 63 - __clzll(hb) : -1;   // first lane of this lane's run in the chunk; -1: the run began earlier
      const uint64_t before = ((1ull << lane) - 1) & ~((1ull << (s < 0 ? 0 : s)) - 1);
      const bool used = (passes & before) != 0 || (s < 0 && carry_used);
      const bool succ = c && !used;
      const uint64_t fails = ~__ballot(succ) & upto(lane);
      const int run = fails ? lane - (63 - __clzll(fails)) : carry_run + lane + 1;   // successes ending at this lane
      best = max(best, wave_max_i(run));
      count += __popcll(__ballot(succ));
      carry_run = __shfl(run, 63, 64);
      carry_used = __shfl((int)(used || c), 63, 64);
      carry_k = __shfl(kk, 63, 64);
    }
    const int L = max(nv, M);   // len(beat_successes)
    cont = best / (1.0 * L);
    tot = count / (1.0 * L);
  }
  if (lane == 0) {
    out[0] = cem;
    out[1] = cont;
    out[2] = tot;
    out[3] = flag;
  }
}

// job 5: validation, trimmed counts and the F-measure -> ws [F, P, R, status, n, M]
__device__ void fmeasure_job(const Track& k, const double* ref_raw, int64_t nr_raw, const double* est_raw, int64_t ne_raw,
                             const Params& P, double* out) {
  const int lane = threadIdx.x;
  int bits = 0;
  for (int64_t i = lane; i < nr_raw; i += 64) bits |= check_event(ref_raw, nr_raw, i, P.min_time);
  for (int64_t i = lane; i < ne_raw; i += 64) bits |= check_event(est_raw, ne_raw, i, P.min_time) << 3;
  int status = wave_or(bits) | (k.bad ? BT_METRICS_OFFSETS : 0);
  // util.match_events: estimate i may take the references in [searchsorted(r, e_i - w, left), searchsorted(r, e_i + w, right)).
  // Both ends are non-decreasing in i, so greedy in ascending order is a maximum matching, and estimates whose windows share
  // no reference with the previous one's start an independent segment: one lane runs the greedy over each segment.
  const double* r = k.r;
  const double* e = k.e;
  const int n = k.n, M = k.M;
  int cnt = 0;
  if (n > 0) {
    for (int base = 0; base < M; base += 64) {
      const int i = base + lane;
      if (i >= M) break;
      int lo = lower_bound(r, n, e[i] - P.f_window), hi = upper_bound(r, n, e[i] + P.f_window);
      if (i > 0 && lo < upper_bound(r, n, e[i - 1] + P.f_window)) continue;   // inside another lane's segment
      int q = lo;
      for (int j = i;;) {
        q = max(q, lo);
        if (q < hi) { ++cnt; ++q; }
        if (++j >= M) break;
        const int nlo = lower_bound(r, n, e[j] - P.f_window);
        if (nlo >= hi) break;
        lo = nlo;
        hi = upper_bound(r, n, e[j] + P.f_window);
      }
    }
  }
  cnt = wave_sum_i(cnt);
  double F = 0, Pr = 0, Rc = 0;
  if (n > 0 && M > 0) {
    Pr = (double)cnt / M;
    Rc = (double)cnt / n;
    F = f_of(Pr, Rc);
  }
  if (lane == 0) {
    out[0] = F;
    out[1] = Pr;
    out[2] = Rc;
    out[3] = status;
    out[4] = n;
    out[5] = M;
  }
}

__global__ __launch_bounds__(64) void metrics_kernel(const double* ref, const int64_t* ref_off, const double* est,
                                                     const int64_t* est_off, int n_tracks, Params P, double* ws) {
  const int t = blockIdx.x / NJOB, job = blockIdx.x % NJOB;
  int64_t nr_raw, ne_raw;
  const Track k = track_of(ref, ref_off, est, est_off, t, P.min_time, nr_raw, ne_raw);
  double* out = ws + ((size_t)t * NJOB + job) * WS_SLOT;
  if (job < 5)
    variation_job(k, job, P, out);
  else
    fmeasure_job(k, ref + (k.bad ? 0 : ref_off[t]), nr_raw, est + (k.bad ? 0 : est_off[t]), ne_raw, P, out);
}

__global__ __launch_bounds__(256) void metrics_finish_kernel(const double* ws, int n_tracks, double* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tracks) return;
  const double* w = ws + (size_t)t * NJOB * WS_SLOT;
  double cem[5], cont[5], tot[5];
  int status = (int)w[5 * WS_SLOT + 3];
  for (int v = 0; v < 5; ++v) {
    cem[v] = w[v * WS_SLOT];
    cont[v] = w[v * WS_SLOT + 1];
    tot[v] = w[v * WS_SLOT + 2];
    if (w[v * WS_SLOT + 3] != 0) status |= BT_METRICS_NEAREST;
  }
  const double* f = w + 5 * WS_SLOT;
  write_row(out + (size_t)t * COLS, f[0], f[1], f[2], cem, cont, tot, (int)f[4], (int)f[5], status);
}

// ---- host: mir_eval's loops ---------------------------------------------------------------------------------------------------
void track_host(const double* ref, int64_t nr_raw, const double* est, int64_t ne_raw, const Params& P, double* row) {
  int status = 0;
  for (int64_t i = 0; i < nr_raw; ++i) status |= check_event(ref, nr_raw, i, P.min_time);
  for (int64_t i = 0; i < ne_raw; ++i) status |= check_event(est, ne_raw, i, P.min_time) << 3;
  const int sr = lower_bound(ref, (int)nr_raw, P.min_time), se = lower_bound(est, (int)ne_raw, P.min_time);
  const double* r = ref + sr;
  const double* e = est + se;
  const int n = (int)nr_raw - sr, M = (int)ne_raw - se;
  double F = 0, Pr = 0, Rc = 0, cem[5] = {}, cont[5] = {}, tot[5] = {};
  if (status == 0 && n > 0 && M > 0) {
    // f_measure: two-pointer greedy matching (a maximum matching: all windows have one width)
    int q = 0, cnt = 0;
    for (int i = 0; i < M; ++i) {
      const double lo = e[i] - P.f_window, hi = e[i] + P.f_window;
      while (q < n && r[q] < lo) ++q;
      if (q < n && r[q] <= hi) { ++cnt; ++q; }
    }
    Pr = (double)cnt / M;
    Rc = (double)cnt / n;
    F = f_of(Pr, Rc);
    for (int v = 0; v < 5; ++v) {   // cemgil
      const Var var{r, v};
      const int nv = var_len(n, v);
      double acc = 0.0;
      for (int i = 0; i < nv; ++i) acc += cemgil_term(min_dist(e, M, var[i]), P.sigma);
      cem[v] = acc / (0.5 * (M + nv));
    }
  }
  if (status == 0 && n > 1 && M > 1) {
    std::vector<uint8_t> used, succ;
    for (int v = 0; v < 5; ++v) {   // continuity
      const Var var{r, v};
      const int nv = var_len(n, v), L = std::max(nv, M);
      used.assign(L, 0);
      succ.assign(L, 0);
      for (int m = 0; m < M; ++m) {
        const int k = nearest(var, nv, e[m]);
        if (!used[k] && cont_cond(var, nv, e, M, m, k, P)) used[k] = succ[m] = 1;
      }
      int best = 0, run = 0, count = 0;
      for (int i = 0; i < L; ++i) {
        run = succ[i] ? run + 1 : 0;
        best = std::max(best, run);
        count += succ[i];
      }
      cont[v] = best / (1.0 * L);
      tot[v] = count / (1.0 * L);
    }
  }
  write_row(row, F, Pr, Rc, cem, cont, tot, n, M, status);
}

// ---- the extended metrics: mir_eval.beat's goto, p_score and information_gain (DESIGN.md section on them) -------------------
constexpr int XJOB = 4;          // per track: Goto (+ validation), P-score, entropy forward, entropy backward
constexpr int XCOLS = BT_METRICS_EXT_COLS;
constexpr int MAX_BINS = 1024;

struct XParams {
  double min_time, g_thr, g_mu, g_sigma, p_thr;
  int bins;
};

// goto's beat_error[k] of reference beat k: 1 at both ends and unless exactly one estimate lies in [window_min, window_max)
__host__ __device__ inline double goto_error(const double* r, int n, const double* e, int M, int k) {
  if (k <= 0 || k >= n - 1) return 1.0;
  const double prev = 0.5 * (r[k] - r[k - 1]), wmin = r[k] - prev;
  const double nxt = 0.5 * (r[k + 1] - r[k]), wmax = r[k] + nxt;
  const int lo = lower_bound(e, M, wmin), hi = lower_bound(e, M, wmax);
  if (hi - lo != 1) return 1.0;
  const double off = e[lo] - r[k];
  return off < 0 ? off / prev : off / nxt;
}

// goto's slice ``track`` from the incorrect beats (their count, first and last, and the first longest gap tl between
// consecutive ones, which starts at tstart): beat_error[first + 1 : last - 1] for fewer than three (the literal slice: it
// stops before the last correct beat), else beat_error[tstart : tstart + tl + 1] (both incorrect ends) if the gap is long
// enough.  No incorrect beat at all (goto_threshold >= 1, where mir_eval raises IndexError): no track.
struct GotoPick {
  int crit, start, len;
};

__host__ __device__ inline GotoPick goto_pick(int n, int cnt, int first, int last, int tl, int tstart) {
  GotoPick g{0, 0, 0};
  if (cnt == 0) return g;
  if (cnt < 3) {
    int b = last - 1;
    if (b < 0) b += n;   // (a negative stop counts from the end)
    b = b < 0 ? 0 : (b > n ? n : b);
    g.crit = 1;
    g.start = first + 1;
    g.len = b > g.start ? b - g.start : 0;
  } else if ((double)(tl - 1) > .25 * (double)(n - 2)) {
    g.crit = 1;
    g.start = tstart;
    g.len = tl + 1;
  }
  return g;
}

// p_score's impulse-train index of time t: np.ceil((t - offset) * 100).astype(int); at most 3e6 for valid events, clamped so
// that invalid ones (whose row is NaN anyway) stay integers
__host__ __device__ inline int pidx(double t, double off) {
  const double x = ceil((t - off) * 100.0);
  if (!(x > -1e9)) return x != x ? 0 : -1000000000;
  return x > 1e9 ? 1000000000 : (int)x;
}

struct Pidx {
  const double* a;
  double off;
  __host__ __device__ int operator[](int i) const { return pidx(a[i], off); }
};

// _get_entropy's beat error of estimate x against the beats r[0..R), R >= 2, after np.mod(. + .5, -1) + .5
__host__ __device__ inline double entropy_error(const double* r, int R, double x) {
  const int c = nearest(r, R, x);
  const double ae = x - r[c];
  double iv;
  if (c == R - 1)
    iv = .5 * (r[R - 1] - r[R - 2]);
  else if (ae < 0)
    iv = .5 * (r[c] - r[c == 0 ? R - 1 : c - 1]);   // c == 0: reference_beats[-1], the last beat
  else
    iv = .5 * (r[c + 1] - r[c]);
  const double be = .5 * ae / iv;
  double m = fmod(be + .5, -1.0);   // numpy's mod: the sign of the divisor
  if (m != 0) {
    if (!(m < 0)) m += -1.0;
  } else {
    m = -0.0;
  }
  return m + .5;
}

struct Edges {   // np.linspace(-.5, .5, bins + 1)[i] for i < bins; the last edge is exactly .5
  double step;
  __host__ __device__ double operator[](int i) const { return i * step + (-.5); }
};

// np.histogram's bin of x: [lo, hi), the last bin closed; -1: in no bin (NaN)
__host__ __device__ inline int entropy_bin(double x, int bins, double step) {
  if (!(x <= .5)) return -1;
  if (x == .5) return bins - 1;
  return upper_bound(Edges{step}, bins, x) - 1;
}

__host__ __device__ inline void write_row_ext(double* row, int n, int M, int bins, double g, double crit, double len,
                                              double mean, double sd, double p, double win, double hits, double fwd, double bwd,
                                              int status) {
  double ig = 0.0;
  if (n > 1 && M > 1) {
    const double norm = log2((double)bins);
    ig = fwd > bwd ? (norm - fwd) / norm : (norm - bwd) / norm;
  }
  const double vals[11] = {g, p, ig, crit, len, mean, sd, win, hits, fwd, bwd};
  const bool bad = (status & ~BT_METRICS_PSCORE) != 0;
  for (int c = 0; c < 11; ++c) row[c] = bad ? NAN : vals[c];
  if (status & BT_METRICS_PSCORE) row[1] = row[7] = row[8] = NAN;
  row[11] = status;
}

// ---- device -----------------------------------------------------------------------------------------------------------------
__device__ inline int wave_min_i(int x) {
  for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
  return x;
}

__device__ inline long long wave_sum_ll(long long x) {
  int lo = (int)(x & 0xffffffffll), hi = (int)(x >> 32);
  for (int o = 32; o > 0; o >>= 1) {
    const long long y = ((long long)__shfl_xor(hi, o, 64) << 32) | (unsigned)__shfl_xor(lo, o, 64);
    x += y;
    lo = (int)(x & 0xffffffffll);
    hi = (int)(x >> 32);
  }
  return x;
}

// job 0: validation (as fmeasure_job) and Goto -> ws [goto, criteria, track length, mean, std, status, n, M]
__device__ void goto_job(const Track& k, const double* ref_raw, int64_t nr_raw, const double* est_raw, int64_t ne_raw,
                         const XParams& P, double* out) {
  const int lane = threadIdx.x;
  int bits = 0;
  for (int64_t i = lane; i < nr_raw; i += 64) bits |= check_event(ref_raw, nr_raw, i, P.min_time);
  for (int64_t i = lane; i < ne_raw; i += 64) bits |= check_event(est_raw, ne_raw, i, P.min_time) << 3;
  const int status = wave_or(bits) | (k.bad ? BT_METRICS_OFFSETS : 0);
  const double* r = k.r;
  const double* e = k.e;
  const int n = k.n, M = k.M;
  double crit = 0, len = 0, mean = 0, sd = 0;
  if (n > 0 && M > 0) {
    // incorrect beats: their count, first, last and the first longest gap between consecutive ones, carried across chunks
    int cnt = 0, first = -1, last = -1, tl = 0, tstart = 0;
    for (int base = 0; base < n; base += 64) {
      const int kk = base + lane;
      const bool inc = kk < n && fabs(goto_error(r, n, e, M, kk)) > P.g_thr;
      const uint64_t mask = __ballot(inc);
      if (mask == 0) continue;
      const uint64_t below = mask & ((1ull << lane) - 1);
      const int prev = below ? base + 63 - __clzll(below) : last;
      const int gap = inc && prev >= 0 ? kk - prev : 0;
      const int gmax = wave_max_i(gap);
      if (gmax > tl) {   // (a later equal gap does not replace an earlier one: np.flatnonzero(diff == max)[0])
        const int kmin = wave_min_i(inc && gap == gmax ? kk : 0x7fffffff);
        tl = gmax;
        tstart = kmin - gmax;
      }
      if (first < 0) first = base + __ffsll((unsigned long long)mask) - 1;
      last = base + 63 - __clzll(mask);
      cnt += __popcll(mask);
    }
    const GotoPick g = goto_pick(n, cnt, first, last, tl, tstart);
    crit = g.crit;
    len = g.len;
    mean = sd = NAN;
    if (g.crit) {
      double sa = 0.0, s = 0.0;
      for (int i = lane; i < g.len; i += 64) {
        const double b = goto_error(r, n, e, M, g.start + i);
        sa += fabs(b);
        s += b;
      }
      sa = wave_sum(sa);
      s = wave_sum(s);
      if (g.len > 0) mean = sa / g.len;
      if (g.len > 1) {
        const double m = s / g.len;
        double q = 0.0;
        for (int i = lane; i < g.len; i += 64) {
          const double d = goto_error(r, n, e, M, g.start + i) - m;
          q += d * d;
        }
        sd = sqrt(wave_sum(q) / (g.len - 1));
      }
      if (mean < P.g_mu && sd < P.g_sigma) crit = 3;
    }
  }
  if (lane == 0) {
    out[0] = crit == 3 ? 1.0 : 0.0;
    out[1] = crit;
    out[2] = len;
    out[3] = mean;
    out[4] = sd;
    out[5] = status;
    out[6] = n;
    out[7] = M;
  }
}

// job 1: P-score -> ws [p_score, win_size, hits, status bit].  The impulse trains are never built: the hits are the pairs of
// distinct 10 ms indices no more than win apart.  Distinct indices are the first occurrences in the (non-decreasing) index
// sequence; their number before a position comes from ballots over blocks of 4096 estimates, 64 masks held one per lane.
__device__ void pscore_job(const Track& k, const XParams& P, double* out) {
  const int lane = threadIdx.x;
  const int n = k.n, M = k.M;
  double p = 0, wout = 0, hout = 0;
  int pstatus = 0;
  if (n > 1 && M > 1) {
    const double off = fmin(k.e[0], k.r[0]);
    const Pidx R{k.r, off}, E{k.e, off};
    // the intervals between distinct reference indices: R[i] - R[i - 1] where it is not 0
    int K = 0;
    for (int i = 1 + lane; i < n; i += 64) K += R[i] - R[i - 1] > 0;
    K = wave_sum_i(K);
    if (K == 0) {
      pstatus = BT_METRICS_PSCORE;
    } else {
      const int span = max(R[n - 1] - R[0], 1);
      // the kk-th smallest interval (0-based) by bisection on its value: the smallest v with kk + 1 intervals in [1, v]
      auto kth = [&](int kk, int from) {
        int lo = from, hi = span;
        while (lo < hi) {
          const int mid = lo + ((hi - lo) >> 1);
          int c = 0;
          for (int i = 1 + lane; i < n; i += 64) {
            const int d = R[i] - R[i - 1];
            c += d > 0 && d <= mid;
          }
          if (wave_sum_i(c) > kk) hi = mid; else lo = mid + 1;
        }
        return lo;
      };
      double median;
      if (K & 1) {
        median = kth(K / 2, 1);
      } else {
        const int a = kth(K / 2 - 1, 1), b = kth(K / 2, a);
        median = ((double)a + (double)b) / 2.0;
      }
      const double w = rint(P.p_thr * median);   // np.round: half to even
      long long hits = 0;
      if (w >= 0) {
        const int win = w > 1e9 ? 1000000000 : (int)w;
        int dbase = 0;   // distinct estimate indices before the block
        for (int B0 = 0; B0 < M; B0 += 4096) {
          const int B1 = min(B0 + 4096, M);
          uint64_t mymask = 0;   // lane c: first-occurrence flags of estimates B0 + 64 c ..
          for (int c = 0; c < 64 && B0 + c * 64 < B1; ++c) {
            const int j = B0 + c * 64 + lane;
            const uint64_t m = __ballot(j < B1 && (j == 0 || E[j] != E[j - 1]));
            if (lane == c) mymask = m;
          }
          const int pc = __popcll(mymask);
          int incl = pc;
          for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
          }
          const int excl = dbase + incl - pc;
          const int mlo = (int)(mymask & 0xffffffffull), mhi = (int)(mymask >> 32);
          // the reference beats whose window [index - win, index + win] reaches into estimates (B0, B1]
          const int i0 = lower_bound(R, n, (double)E[B0] - (double)win);
          const int i1 = B1 < M ? upper_bound(R, n, (double)E[B1] + (double)win) : n;
          for (int base = i0; base < i1; base += 64) {
            const int i = base + lane;
            const bool f = i < i1 && (i == 0 || R[i] != R[i - 1]);
            int lo = 0, hi = 0;
            if (f) {
              const double v = R[i];
              lo = lower_bound(E, M, v - (double)win);
              hi = upper_bound(E, M, v + (double)win);
            }
            for (int s = 0; s < 2; ++s) {   // + distinct estimates before hi, - those before lo
              const int pos = s ? lo : hi;
              const bool in = f && pos > B0 && pos <= B1;
              const int q = in ? pos - B0 - 1 : 0;
              const uint64_t m = ((uint64_t)(unsigned)__shfl(mhi, q >> 6, 64) << 32) | (unsigned)__shfl(mlo, q >> 6, 64);
              const int ex = __shfl(excl, q >> 6, 64);
              if (in) {
                const int D = ex + __popcll(m & upto(q & 63));
                hits += s ? -D : D;
              }
            }
          }
          dbase += __shfl(incl, 63, 64);
        }
        hits = wave_sum_ll(hits);
      }
      wout = w;
      hout = (double)hits;
      p = (double)hits / (double)max(n, M);
    }
  }
  if (lane == 0) {
    out[0] = p;
    out[1] = wout;
    out[2] = hout;
    out[3] = pstatus;
  }
}

// jobs 2, 3: _get_entropy(r, e) -> ws [entropy]; integer bin counters in LDS
__device__ void entropy_job(const double* r, int R, const double* e, int M, int bins, int* cnt, double* out) {
  const int lane = threadIdx.x;
  double H = 0;
  if (R > 1 && M > 1) {
    const double step = 1.0 / bins;
    for (int b = lane; b < bins; b += 64) cnt[b] = 0;
    __syncthreads();
    for (int i = lane; i < M; i += 64) {
      const int b = entropy_bin(entropy_error(r, R, e[i]), bins, step);
      if (b >= 0) atomicAdd(&cnt[b], 1);
    }
    __syncthreads();
    int tot = 0;
    for (int b = lane; b < bins; b += 64) tot += cnt[b];
    tot = wave_sum_i(tot);
    double acc = 0.0;
    for (int b = lane; b < bins; b += 64) {
      double raw = cnt[b] / (1.0 * tot);   // (0 / 0: every error dropped, the entropy is NaN)
      if (raw == 0) raw = 1;
      acc += raw * log2(raw);
    }
    H = -wave_sum(acc);
  }
  if (lane == 0) out[0] = H;
}

__global__ __launch_bounds__(64) void metrics_ext_kernel(const double* ref, const int64_t* ref_off, const double* est,
                                                         const int64_t* est_off, int n_tracks, XParams P, double* ws) {
  __shared__ int cnt[MAX_BINS];
  const int t = blockIdx.x / XJOB, job = blockIdx.x % XJOB;
  int64_t nr_raw, ne_raw;
  const Track k = track_of(ref, ref_off, est, est_off, t, P.min_time, nr_raw, ne_raw);
  double* out = ws + ((size_t)t * XJOB + job) * WS_SLOT;
  if (job == 0)
    goto_job(k, ref + (k.bad ? 0 : ref_off[t]), nr_raw, est + (k.bad ? 0 : est_off[t]), ne_raw, P, out);
  else if (job == 1)
    pscore_job(k, P, out);
  else if (job == 2)
    entropy_job(k.r, k.n, k.e, k.M, P.bins, cnt, out);
  else
    entropy_job(k.e, k.M, k.r, k.n, P.bins, cnt, out);
}

__global__ __launch_bounds__(256) void metrics_ext_finish_kernel(const double* ws, int n_tracks, int bins, double* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tracks) return;
  const double* g = ws + (size_t)t * XJOB * WS_SLOT;
  const double* p = g + WS_SLOT;
  write_row_ext(out + (size_t)t * XCOLS, (int)g[6], (int)g[7], bins, g[0], g[1], g[2], g[3], g[4], p[0], p[1], p[2],
                g[2 * WS_SLOT], g[3 * WS_SLOT], (int)g[5] | (int)p[3]);
}

// ---- host: the sequential loops ---------------------------------------------------------------------------------------------
double entropy_host(const double* r, int R, const double* e, int M, int bins) {
  std::vector<int64_t> cnt(bins, 0);
  const double step = 1.0 / bins;
  int64_t tot = 0;
  for (int i = 0; i < M; ++i) {
    const int b = entropy_bin(entropy_error(r, R, e[i]), bins, step);
    if (b >= 0) {
      ++cnt[b];
      ++tot;
    }
  }
  double acc = 0.0;
  for (int b = 0; b < bins; ++b) {
    double raw = cnt[b] / (1.0 * tot);
    if (raw == 0) raw = 1;
    acc += raw * log2(raw);
  }
  return -acc;
}

void track_ext_host(const double* ref, int64_t nr_raw, const double* est, int64_t ne_raw, const XParams& P, double* row) {
  int status = 0;
  for (int64_t i = 0; i < nr_raw; ++i) status |= check_event(ref, nr_raw, i, P.min_time);
  for (int64_t i = 0; i < ne_raw; ++i) status |= check_event(est, ne_raw, i, P.min_time) << 3;
  const int sr = lower_bound(ref, (int)nr_raw, P.min_time), se = lower_bound(est, (int)ne_raw, P.min_time);
  const double* r = ref + sr;
  const double* e = est + se;
  const int n = (int)nr_raw - sr, M = (int)ne_raw - se;
  double crit = 0, len = 0, mean = 0, sd = 0, p = 0, win = 0, hits = 0, fwd = 0, bwd = 0;
  if (status == 0 && n > 0 && M > 0) {   // goto
    std::vector<double> be(n);
    for (int k = 0; k < n; ++k) be[k] = goto_error(r, n, e, M, k);
    int cnt = 0, first = -1, last = -1, tl = 0, tstart = 0;
    for (int k = 0; k < n; ++k) {
      if (!(fabs(be[k]) > P.g_thr)) continue;
      if (last >= 0 && k - last > tl) {
        tl = k - last;
        tstart = last;
      }
      if (first < 0) first = k;
      last = k;
      ++cnt;
    }
    const GotoPick g = goto_pick(n, cnt, first, last, tl, tstart);
    crit = g.crit;
    len = g.len;
    mean = sd = NAN;
    if (g.crit) {
      double sa = 0.0, s = 0.0;
      for (int i = 0; i < g.len; ++i) {
        sa += fabs(be[g.start + i]);
        s += be[g.start + i];
      }
      if (g.len > 0) mean = sa / g.len;
      if (g.len > 1) {
        const double m = s / g.len;
        double q = 0.0;
        for (int i = 0; i < g.len; ++i) {
          const double d = be[g.start + i] - m;
          q += d * d;
        }
        sd = sqrt(q / (g.len - 1));
      }
      if (mean < P.g_mu && sd < P.g_sigma) crit = 3;
    }
  }
  if (status == 0 && n > 1 && M > 1) {
    // p_score, the counting form: distinct indices, the median of their intervals, pairs no more than win apart
    const double off = fmin(e[0], r[0]);
    const Pidx R{r, off}, E{e, off};
    std::vector<int> ri, ei, d;
    for (int i = 0; i < n; ++i)
      if (ri.empty() || R[i] != ri.back()) ri.push_back(R[i]);
    for (int i = 0; i < M; ++i)
      if (ei.empty() || E[i] != ei.back()) ei.push_back(E[i]);
    for (size_t i = 1; i < ri.size(); ++i) d.push_back(ri[i] - ri[i - 1]);
    if (d.empty()) {
      status |= BT_METRICS_PSCORE;
    } else {
      std::sort(d.begin(), d.end());
      const size_t K = d.size();
      const double median = (K & 1) ? (double)d[K / 2] : ((double)d[K / 2 - 1] + (double)d[K / 2]) / 2.0;
      win = rint(P.p_thr * median);
      int64_t h = 0;
      if (win >= 0) {
        const int w = win > 1e9 ? 1000000000 : (int)win;
        for (const int v : ri)
          h += std::upper_bound(ei.begin(), ei.end(), v + w) - std::lower_bound(ei.begin(), ei.end(), v - w);
      }
      hits = (double)h;
      p = (double)h / (double)std::max(n, M);
    }
    fwd = entropy_host(r, n, e, M, P.bins);
    bwd = entropy_host(e, M, r, n, P.bins);
  }
  write_row_ext(row, n, M, P.bins, crit == 3 ? 1.0 : 0.0, crit, len, mean, sd, p, win, hits, fwd, bwd, status);
}

bool args_ok(const int64_t* ref_off, const int64_t* est_off, int n_tracks, double* out) {
  return ref_off && est_off && out && n_tracks > 0 && n_tracks <= 0x7fffffff / NJOB;
}

}  // namespace

extern "C" {

size_t bt_beat_metrics_workspace_bytes(int n_tracks, int64_t total_ref, int64_t total_est) {
  if (n_tracks <= 0 || n_tracks > 0x7fffffff / NJOB || total_ref < 0 || total_est < 0) return 0;
  return (size_t)n_tracks * NJOB * WS_SLOT * sizeof(double);
}

int bt_beat_metrics(void* stream, const double* d_ref, const int64_t* d_ref_off, const double* d_est, const int64_t* d_est_off,
                    int n_tracks, double min_beat_time, double f_window, double cemgil_sigma, double phase_thr,
                    double period_thr, void* d_ws, size_t ws_bytes, double* d_out) {
  if (!args_ok(d_ref_off, d_est_off, n_tracks, d_out) || !d_ref || !d_est || !d_ws)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_beat_metrics");
  if (ws_bytes < bt_beat_metrics_workspace_bytes(n_tracks, 0, 0))
    return bt_set_error_external(BT_ERR_WORKSPACE, "bt_beat_metrics: workspace too small");
  const Params P{min_beat_time, f_window, cemgil_sigma, phase_thr, period_thr};
  hipStream_t s = (hipStream_t)stream;
  double* ws = (double*)d_ws;
  hipLaunchKernelGGL(metrics_kernel, dim3(n_tracks * NJOB), dim3(64), 0, s, d_ref, d_ref_off, d_est, d_est_off, n_tracks, P, ws);
  hipLaunchKernelGGL(metrics_finish_kernel, dim3((n_tracks + 255) / 256), dim3(256), 0, s, (const double*)ws, n_tracks, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string("bt_beat_metrics: ") + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_beat_metrics_host(const double* ref, const int64_t* ref_off, const double* est, const int64_t* est_off, int n_tracks,
                         double min_beat_time, double f_window, double cemgil_sigma, double phase_thr, double period_thr,
                         double* out) {
  if (!args_ok(ref_off, est_off, n_tracks, out)) return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_beat_metrics_host");
  const Params P{min_beat_time, f_window, cemgil_sigma, phase_thr, period_thr};
  for (int t = 0; t < n_tracks; ++t) {
    const int64_t r0 = ref_off[t], e0 = est_off[t], nr = ref_off[t + 1] - r0, ne = est_off[t + 1] - e0;
    double* row = out + (size_t)t * COLS;
    if (r0 < 0 || e0 < 0 || nr < 0 || ne < 0 || nr > 0x3fffffff || ne > 0x3fffffff || (nr && !ref) || (ne && !est)) {
      const double z[5] = {};
      write_row(row, 0, 0, 0, z, z, z, 0, 0, BT_METRICS_OFFSETS);
      continue;
    }
    track_host(ref + r0, nr, est + e0, ne, P, row);
  }
  return BT_OK;
}

size_t bt_beat_metrics_ext_workspace_bytes(int n_tracks, int64_t total_ref, int64_t total_est) {
  if (n_tracks <= 0 || n_tracks > 0x7fffffff / NJOB || total_ref < 0 || total_est < 0) return 0;
  return (size_t)n_tracks * XJOB * WS_SLOT * sizeof(double);
}

int bt_beat_metrics_ext(void* stream, const double* d_ref, const int64_t* d_ref_off, const double* d_est,
                        const int64_t* d_est_off, int n_tracks, double min_beat_time, double goto_threshold, double goto_mu,
                        double goto_sigma, double p_score_threshold, int bins, void* d_ws, size_t ws_bytes, double* d_out) {
  if (!args_ok(d_ref_off, d_est_off, n_tracks, d_out) || !d_ref || !d_est || !d_ws || bins < 1 || bins > MAX_BINS)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_beat_metrics_ext");
  if (ws_bytes < bt_beat_metrics_ext_workspace_bytes(n_tracks, 0, 0))
    return bt_set_error_external(BT_ERR_WORKSPACE, "bt_beat_metrics_ext: workspace too small");
  const XParams P{min_beat_time, goto_threshold, goto_mu, goto_sigma, p_score_threshold, bins};
  hipStream_t s = (hipStream_t)stream;
  double* ws = (double*)d_ws;
  hipLaunchKernelGGL(metrics_ext_kernel, dim3(n_tracks * XJOB), dim3(64), 0, s, d_ref, d_ref_off, d_est, d_est_off, n_tracks, P,
                     ws);
  hipLaunchKernelGGL(metrics_ext_finish_kernel, dim3((n_tracks + 255) / 256), dim3(256), 0, s, (const double*)ws, n_tracks, bins,
                     d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return bt_set_error_external(BT_ERR_HIP, (std::string("bt_beat_metrics_ext: ") + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_beat_metrics_ext_host(const double* ref, const int64_t* ref_off, const double* est, const int64_t* est_off, int n_tracks,
                             double min_beat_time, double goto_threshold, double goto_mu, double goto_sigma,
                             double p_score_threshold, int bins, double* out) {
  if (!args_ok(ref_off, est_off, n_tracks, out) || bins < 1 || bins > MAX_BINS)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_beat_metrics_ext_host");
  const XParams P{min_beat_time, goto_threshold, goto_mu, goto_sigma, p_score_threshold, bins};
  for (int t = 0; t < n_tracks; ++t) {
    const int64_t r0 = ref_off[t], e0 = est_off[t], nr = ref_off[t + 1] - r0, ne = est_off[t + 1] - e0;
    double* row = out + (size_t)t * XCOLS;
    if (r0 < 0 || e0 < 0 || nr < 0 || ne < 0 || nr > 0x3fffffff || ne > 0x3fffffff || (nr && !ref) || (ne && !est)) {
      write_row_ext(row, 0, 0, bins, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, BT_METRICS_OFFSETS);
      continue;
    }
    track_ext_host(ref + r0, nr, est + e0, ne, P, row);
  }
  return BT_OK;
}

}  // extern "C"
