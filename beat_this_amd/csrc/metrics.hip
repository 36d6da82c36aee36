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

}  // extern "C"
