// Time stretch, pitch shift and arbitrary-ratio resampling for building training bundles from audio (the step the
// reference leaves to pedalboard / Rubber Band in launch_scripts/preprocess_audio.py).  The algorithm is this package's own
// and is defined by include/beat_this_amd.h (bt_stretch, bt_resample_ratio); tests/stretch_reference.py is its numpy twin,
// DESIGN.md section 20 the description.
//
// bt_stretch: phase vocoder, n_fft 2048, synthesis hop 512, identity phase locking, phases as 32-bit fixed-point turns.
//   (1) analysis_kernel   one workgroup per output frame: the two analysis frames (a synthesis hop apart) through a 1024-point
//                         complex FFT + real split -> |X1| (fp64), q(X1), d = q(X1) - q(X0)
//   (2) scan_sums_kernel / scan_apply_kernel   S = prefix sum of d along the frames, per bin, in uint32: blocks of
//                         BT_STRETCH_SCAN_BLOCK frames, block totals first, then every block from its offset (exact, any order)
//   (3) synth_kernel      one workgroup per frame: peaks -> 1025-bit map by wave ballots, owner of every bin by bit scans,
//                         phi = S[owner] + q1 - q1[owner], Y = |X1| e^{i phi}, inverse real FFT, synthesis window -> frame buffer
//   (4) ola_kernel        one thread per output sample gathers its four frames in ascending order and divides by the sum of
//                         squared windows: no atomics, the same bits on every run
// The analysis runs in fp64: which bin is a peak is a comparison of neighbouring magnitudes, and in fp32 the FFT's rounding
// (relative to the frame's strongest partial) decides near-ties among weak bins differently from the fp64 definition about
// once in ten frames.  In fp64 the decisions are the definition's, and the phases are exact to the last unit of 2^-32 turns.
// The synthesis (no decisions) is fp32.  The FFT is a radix-4 Stockham autosort in LDS, 256 threads, one butterfly per
// thread and stage, five stages; twiddles come from a table computed in fp64 on the host (tables.stretch_tables).
//
// bt_resample_ratio: one thread per output sample; the position m * step and the filter argument are fp64, the taps run in
// ascending input index, the filter value is a linear interpolation in a one-sided fp32 table.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/beat_this_amd.h"

#pragma clang fp contract(off)

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

#define DEVI __device__ __forceinline__

constexpr int NFFT = 2048, HS = 512, BINS = 1025, PITCH = 1028, NC = 1024;   // PITCH: row pitch of the per-frame bin arrays
constexpr int SCAN_BLOCK = BT_STRETCH_SCAN_BLOCK;
constexpr int TAB_WIN = 0, TAB_TW = 2048, TAB_SPLIT = 2048 + 2 * 1024;       // offsets into the table (doubles)
static_assert(BT_STRETCH_TABLE_DOUBLES == TAB_SPLIT + 2 * BINS, "table layout");

template <typename T> struct C2 { T re, im; };
template <typename T> DEVI C2<T> cadd(C2<T> a, C2<T> b) { return {a.re + b.re, a.im + b.im}; }
template <typename T> DEVI C2<T> csub(C2<T> a, C2<T> b) { return {a.re - b.re, a.im - b.im}; }
template <typename T> DEVI C2<T> cmul(C2<T> a, C2<T> b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// 1024-point complex DFT of a[] (sign -1, or +1 and unnormalised with INV) by 256 threads, t = threadIdx.x: radix-4 Stockham,
// stage s combines sub-transforms of length Ns = 4^s.  The caller has synchronised after filling a[]; every stage ends with a
// barrier; the result is in the returned buffer (b, after five stages).
template <typename T, bool INV> DEVI C2<T>* fft1024(C2<T>* a, C2<T>* b, const double* __restrict__ tw, int t) {
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int Ns = 1 << (2 * s);
    const int k = t & (Ns - 1);
    C2<T> v0 = a[t], v1 = a[t + 256], v2 = a[t + 512], v3 = a[t + 768];
    if (s > 0) {
      const int e = k * (256 >> (2 * s));   // exp(-+2 pi i r k / (4 Ns)) = tw[r e], r e < 768
      const C2<T> w1 = {(T)tw[2 * e], (T)(INV ? -tw[2 * e + 1] : tw[2 * e + 1])};
      const C2<T> w2 = {(T)tw[4 * e], (T)(INV ? -tw[4 * e + 1] : tw[4 * e + 1])};
      const C2<T> w3 = {(T)tw[6 * e], (T)(INV ? -tw[6 * e + 1] : tw[6 * e + 1])};
      v1 = cmul(v1, w1);
      v2 = cmul(v2, w2);
      v3 = cmul(v3, w3);
    }
    const C2<T> s02 = cadd(v0, v2), d02 = csub(v0, v2), s13 = cadd(v1, v3), d13 = csub(v1, v3);
    const C2<T> rot = INV ? C2<T>{-d13.im, d13.re} : C2<T>{d13.im, -d13.re};   // +i d13 / -i d13
    const int j0 = ((t - k) << 2) + k;
    b[j0] = cadd(s02, s13);
    b[j0 + Ns] = cadd(d02, rot);
    b[j0 + 2 * Ns] = csub(s02, s13);
    b[j0 + 3 * Ns] = csub(d02, rot);
    __syncthreads();
    C2<T>* tmp = a;
    a = b;
    b = tmp;
  }
  return a;
}

// q(z): the phase as 32-bit fixed-point turns, round(atan2(im, re) / 2 pi * 2^32) mod 2^32, q(0) = 0
DEVI uint32_t qphase(double re, double im) {
  if (re == 0.0 && im == 0.0) return 0u;
  const double turns = atan2(im, re) * (1.0 / (2.0 * 3.14159265358979323846));
  return (uint32_t)(long long)rint(turns * 4294967296.0);
}

__global__ __launch_bounds__(256) void analysis_kernel(const float* __restrict__ x, long N, double L, const double* __restrict__ tab,
                                                       double* __restrict__ mag, uint32_t* __restrict__ q1, uint32_t* __restrict__ d) {
  __shared__ C2<double> A[NC];
  __shared__ C2<double> B[NC];
  const int t = threadIdx.x, n = blockIdx.x;
  const long a_n = (long)floor((double)((long)n * HS) / L + 0.5);
  const double* win = tab + TAB_WIN;
  uint32_t q0[5] = {0u, 0u, 0u, 0u, 0u};
  for (int pass = (n == 0 ? 1 : 0); pass < 2; ++pass) {   // pass 0: X0 (centre a_n - Hs), pass 1: X1 (centre a_n)
    const long first = a_n - (pass ? 0 : HS) - NFFT / 2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                          // z[i] = xw[2 i] + i xw[2 i + 1]
      const int i = t + 256 * r;
      const long j = first + 2 * i;
      const float x0 = (j >= 0 && j < N) ? x[j] : 0.f;
      const float x1 = (j + 1 >= 0 && j + 1 < N) ? x[j + 1] : 0.f;
      A[i] = {(double)x0 * win[2 * i], (double)x1 * win[2 * i + 1]};
    }
    __syncthreads();
    const C2<double>* Z = fft1024<double, false>(A, B, tab + TAB_TW, t);
#pragma unroll
    for (int r = 0; r < 5; ++r) {                          // split step: X[k], k = 0 .. 1024
      const int k = t + 256 * r;
      if (k < BINS) {
        const int k0 = k & (NC - 1), m = (NC - k) & (NC - 1);
        const double a = Z[k0].re, b = Z[k0].im, c = Z[m].re, e = Z[m].im;
        const double er = 0.5 * (a + c), ei = 0.5 * (b - e), orr = 0.5 * (a - c), oi = 0.5 * (b + e);
        const double tx = tab[TAB_SPLIT + 2 * k], ty = tab[TAB_SPLIT + 2 * k + 1];   // (cos, -sin) 2 pi k / 2048
        const double xr = er + (tx * oi + ty * orr);
        const double xi = ei - (tx * orr - ty * oi);
        const uint32_t q = qphase(xr, xi);
        if (pass == 0) {
          q0[r] = q;
        } else {
          const size_t o = (size_t)n * PITCH + k;
          mag[o] = sqrt(xr * xr + xi * xi);
          q1[o] = q;
          d[o] = n == 0 ? q : q - q0[r];
        }
      }
    }
    __syncthreads();
  }
}

// grid (blocks of SCAN_BLOCK frames, 5): sums[blk][k] = sum of d[n][k] over the block's frames (mod 2^32)
__global__ __launch_bounds__(256) void scan_sums_kernel(const uint32_t* __restrict__ d, int F, uint32_t* __restrict__ sums) {
  const int k = blockIdx.y * 256 + threadIdx.x;
  if (k >= BINS) return;
  const int n0 = blockIdx.x * SCAN_BLOCK, n1 = min(F, n0 + SCAN_BLOCK);
  uint32_t acc = 0u;
  for (int n = n0; n < n1; ++n) acc += d[(size_t)n * PITCH + k];
  sums[(size_t)blockIdx.x * PITCH + k] = acc;
}

// same grid: d[n][k] <- S[n][k] = sum of d[0 .. n][k]
__global__ __launch_bounds__(256) void scan_apply_kernel(uint32_t* __restrict__ d, int F, const uint32_t* __restrict__ sums) {
  const int k = blockIdx.y * 256 + threadIdx.x;
  if (k >= BINS) return;
  uint32_t acc = 0u;
  for (int b = 0; b < (int)blockIdx.x; ++b) acc += sums[(size_t)b * PITCH + k];
  const int n0 = blockIdx.x * SCAN_BLOCK, n1 = min(F, n0 + SCAN_BLOCK);
  for (int n = n0; n < n1; ++n) {
    acc += d[(size_t)n * PITCH + k];
    d[(size_t)n * PITCH + k] = acc;
  }
}

// the 1025-bit peak map: bin k is bit (k & 63) of word (k >> 6); word 16 holds bin 1024 alone
DEVI int prev_peak(const unsigned long long* bits, int k) {   // largest peak < k, or -1
  int w = k >> 6;
  unsigned long long m = bits[w] & ((1ull << (k & 63)) - 1ull);
  for (;;) {
    if (m) return w * 64 + 63 - __clzll((long long)m);
    if (--w < 0) return -1;
    m = bits[w];
  }
}
DEVI int next_peak(const unsigned long long* bits, int k) {   // smallest peak > k, or -1
  int w = k >> 6;
  const int b = k & 63;
  unsigned long long m = b == 63 ? 0ull : bits[w] & (~0ull << (b + 1));
  for (;;) {
    if (m) return w * 64 + __ffsll((long long)m) - 1;
    if (++w > 16) return -1;
    m = bits[w];
  }
}

__global__ __launch_bounds__(256) void synth_kernel(const double* __restrict__ mag, const uint32_t* __restrict__ q1,
                                                    const uint32_t* __restrict__ S, const double* __restrict__ tab,
                                                    float* __restrict__ frames) {
  __shared__ C2<float> A[NC];
  __shared__ C2<float> B[NC];
  __shared__ C2<float> Y[BINS];
  __shared__ double smag[BINS];
  __shared__ unsigned long long bits[17];
  const int t = threadIdx.x, n = blockIdx.x;
  const size_t row = (size_t)n * PITCH;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const int k = t + 256 * r;
    if (k < BINS) smag[k] = mag[row + k];
  }
  __syncthreads();
  // peak: mag > 0, greater than the two bins below, not smaller than the two bins above (where they exist)
  auto is_peak = [&](int k) -> bool {
    const double m = smag[k];
    bool p = m > 0.0;
    if (k >= 1) p = p && m > smag[k - 1];
    if (k >= 2) p = p && m > smag[k - 2];
    if (k + 1 < BINS) p = p && m >= smag[k + 1];
    if (k + 2 < BINS) p = p && m >= smag[k + 2];
    return p;
  };
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned long long word = __ballot(is_peak(t + 256 * r));
    if ((t & 63) == 0) bits[r * 4 + (t >> 6)] = word;
  }
  if (t == 0) bits[16] = is_peak(NC) ? 1ull : 0ull;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const int k = t + 256 * r;
    if (k < BINS) {
      int own = k;
      if (!((bits[k >> 6] >> (k & 63)) & 1ull)) {
        const int lo = prev_peak(bits, k), hi = next_peak(bits, k);
        if (lo >= 0 && hi >= 0) own = k <= ((lo + hi) >> 1) ? lo : hi;
        else if (lo >= 0) own = lo;
        else if (hi >= 0) own = hi;
      }
      const uint32_t phi = S[row + own] + q1[row + k] - q1[row + own];
      const float half_turns = (float)(int32_t)phi * 4.656612873077392578125e-10f;   // 2^-31: the angle in units of pi
      float sn, cs;
      sincospif(half_turns, &sn, &cs);
      const float m = (float)smag[k];
      Y[k] = {m * cs, (k == 0 || k == NC) ? 0.f : m * sn};   // (the inverse real FFT has no use for Im Y[0], Im Y[1024])
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {   // Z[k] = E[k] + i O[k]: spectra of the even and the odd output samples
    const int k = t + 256 * r;
    const C2<float> yk = Y[k], ym = {Y[NC - k].re, -Y[NC - k].im};
    const C2<float> E = {0.5f * (yk.re + ym.re), 0.5f * (yk.im + ym.im)};
    const C2<float> D = {0.5f * (yk.re - ym.re), 0.5f * (yk.im - ym.im)};
    const C2<float> w = {(float)tab[TAB_SPLIT + 2 * k], (float)-tab[TAB_SPLIT + 2 * k + 1]};   // e^{+2 pi i k / 2048}
    const C2<float> O = cmul(D, w);
    A[k] = {E.re - O.im, E.im + O.re};
  }
  __syncthreads();
  const C2<float>* z = fft1024<float, true>(A, B, tab + TAB_TW, t);
  float* out = frames + (size_t)n * NFFT;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = t + 256 * r;
    const float2 v = {z[i].re * (1.0f / 1024.0f) * (float)tab[TAB_WIN + 2 * i], z[i].im * (1.0f / 1024.0f) * (float)tab[TAB_WIN + 2 * i + 1]};
    *reinterpret_cast<float2*>(out + 2 * i) = v;
  }
}

__global__ __launch_bounds__(256) void ola_kernel(const float* __restrict__ frames, const double* __restrict__ tab, int F, long M,
                                                  float* __restrict__ out) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const long top = (m + NFFT / 2) / HS;
  float acc = 0.f, norm = 0.f;
#pragma unroll
  for (int j = 3; j >= 0; --j) {   // ascending frame index
    const long n = top - j;
    if (n >= 0 && n < F) {
      const int i = (int)(m + NFFT / 2 - n * HS);
      const float w = (float)tab[TAB_WIN + i];
      acc = acc + frames[(size_t)n * NFFT + i];
      norm = norm + w * w;
    }
  }
  out[m] = acc / norm;
}

__global__ __launch_bounds__(256) void resample_ratio_kernel(const float* __restrict__ x, long n_in, double step, double c,
                                                             const float* __restrict__ table, float* __restrict__ y, long n_out) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= n_out) return;
  constexpr double P = BT_RESAMPLE_RATIO_TAPS;
  constexpr double PZ = (double)BT_RESAMPLE_RATIO_TAPS * BT_RESAMPLE_RATIO_CROSSINGS;
  const double pos = (double)m * step;
  const double reach = (double)BT_RESAMPLE_RATIO_CROSSINGS / c;
  const long j_lo = (long)ceil(pos - reach);
  const int n_taps = (int)floor(2.0 * reach) + 1;
  float acc = 0.f;
  for (int o = 0; o < n_taps; ++o) {
    const long j = j_lo + o;
    const double u = fabs(c * (pos - (double)j)) * P;
    if (u < PZ && j >= 0 && j < n_in) {
      const int i = (int)u;
      const float f = (float)(u - (double)i);
      const float t0 = table[i], t1 = table[i + 1];
      const float h = t0 + f * (t1 - t0);
      acc = acc + x[j] * h;
    }
  }
  y[m] = acc * (float)c;
}

struct Layout {
  long M;
  int F, n_blocks;
  size_t off_mag, off_q1, off_s, off_sums, off_frames, total;
};

// false: unsupported (L outside [0.5, 2] or not a number, a length outside 1 .. BT_STRETCH_MAX_SAMPLES)
bool layout(int64_t n_in, double L, Layout& y) {
  if (!(L >= 0.5 && L <= 2.0) || n_in < 1 || n_in > BT_STRETCH_MAX_SAMPLES) return false;
  y.M = (long)std::floor((double)n_in * L + 0.5);
  if (y.M < 1 || y.M > BT_STRETCH_MAX_SAMPLES) return false;
  y.F = (int)((y.M + HS - 1) / HS) + 1;
  y.n_blocks = (y.F + SCAN_BLOCK - 1) / SCAN_BLOCK;
  size_t o = 0;
  y.off_mag = o;    o += (size_t)y.F * PITCH * sizeof(double);
  y.off_q1 = o;     o += (size_t)y.F * PITCH * sizeof(uint32_t);
  y.off_s = o;      o += (size_t)y.F * PITCH * sizeof(uint32_t);
  y.off_sums = o;   o += (size_t)y.n_blocks * PITCH * sizeof(uint32_t);
  y.off_frames = o; o += (size_t)y.F * NFFT * sizeof(float);
  y.total = o;
  return true;
}

int fail(const char* fn, const char* msg, int code = BT_ERR_ARG) {
  return bt_set_error_external(code, (std::string(fn) + ": " + msg).c_str());
}

int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? BT_OK : fail(fn, hipGetErrorString(e), BT_ERR_HIP);
}

}  // namespace

extern "C" {

int64_t bt_stretch_out_len(int64_t n_in, double L) {
  Layout y;
  return layout(n_in, L, y) ? (int64_t)y.M : 0;
}

size_t bt_stretch_workspace_bytes(int64_t n_in, double L) {
  Layout y;
  return layout(n_in, L, y) ? y.total : 0;
}

int bt_stretch(void* stream, const double* d_tables, const float* d_in, int64_t n_in, double L, float* d_out, int64_t n_out,
               void* d_ws, size_t ws_bytes) {
  const char* fn = "bt_stretch";
  if (!d_tables || !d_in || !d_out || !d_ws) return fail(fn, "null argument");
  Layout y;
  if (!layout(n_in, L, y)) return fail(fn, "need 0.5 <= L <= 2 and 1 <= n_in, n_out <= BT_STRETCH_MAX_SAMPLES");
  if (n_out != y.M) return fail(fn, "n_out must be floor(n_in L + 0.5)");
  if (((uintptr_t)d_ws & 15) || ((uintptr_t)d_tables & 7)) return fail(fn, "the workspace must be 16-byte aligned, the table 8-byte");
  if (ws_bytes < y.total) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
  char* ws = static_cast<char*>(d_ws);
  double* mag = reinterpret_cast<double*>(ws + y.off_mag);
  uint32_t* q1 = reinterpret_cast<uint32_t*>(ws + y.off_q1);
  uint32_t* s = reinterpret_cast<uint32_t*>(ws + y.off_s);
  uint32_t* sums = reinterpret_cast<uint32_t*>(ws + y.off_sums);
  float* frames = reinterpret_cast<float*>(ws + y.off_frames);
  hipStream_t st = (hipStream_t)stream;
  const dim3 scan_grid((unsigned)y.n_blocks, (BINS + 255) / 256);
  hipLaunchKernelGGL(analysis_kernel, dim3((unsigned)y.F), dim3(256), 0, st, d_in, (long)n_in, L, d_tables, mag, q1, s);
  hipLaunchKernelGGL(scan_sums_kernel, scan_grid, dim3(256), 0, st, s, y.F, sums);
  hipLaunchKernelGGL(scan_apply_kernel, scan_grid, dim3(256), 0, st, s, y.F, sums);
  hipLaunchKernelGGL(synth_kernel, dim3((unsigned)y.F), dim3(256), 0, st, mag, q1, s, d_tables, frames);
  hipLaunchKernelGGL(ola_kernel, dim3((unsigned)((y.M + 255) / 256)), dim3(256), 0, st, frames, d_tables, y.F, y.M, d_out);
  return launched(fn);
}

int bt_resample_ratio(void* stream, const float* d_in, int64_t n_in, double step, const float* d_table, float* d_out,
                      int64_t n_out) {
  const char* fn = "bt_resample_ratio";
  if (!d_in || !d_table || !d_out) return fail(fn, "null argument");
  if (!(step >= 0.25 && step <= 4.0)) return fail(fn, "need 0.25 <= step <= 4");
  if (n_in < 1 || n_out < 1 || n_in > 4 * (int64_t)BT_STRETCH_MAX_SAMPLES || n_out > 4 * (int64_t)BT_STRETCH_MAX_SAMPLES)
    return fail(fn, "need 1 <= n_in, n_out <= 4 BT_STRETCH_MAX_SAMPLES");
  const double c = step > 1.0 ? 1.0 / step : 1.0;
  hipLaunchKernelGGL(resample_ratio_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_in,
                     (long)n_in, step, c, d_table, d_out, (long)n_out);
  return launched(fn);
}

}  // extern "C"
