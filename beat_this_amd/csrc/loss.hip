// The reference's training losses (beat_this/model/loss.py: MaskedBCELoss, ShiftTolerantBCELoss, SplittedShiftTolerantBCELoss)
// with their gradients with respect to the logits.  DESIGN.md section 11 has the formulation and what is pinned.
//
// Rows come in CSR form (row r is elements off[r] .. off[r + 1] of logits, targets and mask).  For a row of T frames and
// h = 2 * tolerance (0 for the masked loss) the output frames are t in [h, T - h); frame t contributes
//   masked:          bce(x_t, y_t) * m_t                                      x_t = logit t
//   shift-tolerant:  bce(X_t, y_t) * ((y_t + (1 - S_t)) * m_t)                X_t = max of logits [t - tol, t + tol]
//   splitted:        bce(X_t, y_t) * (y_t * m_t) + bce(X_t, S_t) * ((1 - S_t) * m_t)
// with S_t the max of targets [t - 2 tol, t + 2 tol] and torch's
//   bce(x, y) = (1 - y) * x + (1 + (pw - 1) * y) * (log1p(exp(-|x|)) + max(-x, 0)).
// A window's maximum is the first index holding it, except that a NaN always takes the window (torch's CPU max_pool1d:
// `v > max || isnan(v)`); the gradient of a window's term goes to that index only.
//
// Device: one 256-thread workgroup per (row, segment of SEG frames).  It stages the segment's logits with a 2 tol halo and its
// targets with a 3 tol halo in LDS, evaluates the terms of the output frames [j0 - tol, j0 + SEG + tol) together with their
// window argmax and d(term)/dX, and then GATHERS the gradient: frame j sums, over t = j - tol .. j + tol in ascending order, the
// d(term)/dX of the windows whose argmax is j.  No floating-point atomics anywhere.  The segment's terms are summed in fp64 by
// a fixed 256-leaf tree; a second launch (one workgroup) adds each row's segments in index order and the rows into the total
// by a fixed shape (thread i takes rows i, i + 256, ..., then a 256-leaf tree).  None of it depends on the launch geometry or
// on the other rows: a row alone and inside a ragged batch has the same bits.
// Host: bt_bce_loss_host repeats the same fp32 operations and the same fp64 trees.  exp and log1p are written out here in
// plain fp32 arithmetic (no libm, no device intrinsics) and the file is compiled with -ffp-contract=off, so the device's
// per-frame terms and gradients are bit-identical to the host's.
#include <hip/hip_fp16.h>
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

constexpr int SEG = BT_LOSS_SEGMENT;       // frames per workgroup; also the threads of a workgroup
constexpr int MAXTOL = BT_LOSS_MAX_TOLERANCE;
constexpr int FIN = 256;                   // threads of the finishing workgroup (fixes the shape of the total's tree)

// ---- element loads (exact conversions) ------------------------------------------------------------------------------------
__host__ __device__ inline float bits_f32(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

__host__ __device__ inline uint32_t f32_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

__host__ __device__ inline float h2f(uint16_t h) {
  const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ff;
  if (e == 0) {   // zero / subnormal: m * 2^-24 is exact in fp32
    const float v = (float)m * 5.9604644775390625e-8f;
    return s ? -v : v;
  }
  if (e == 31) return bits_f32(s | 0x7f800000u | (m << 13));
  return bits_f32(s | ((e + 112) << 23) | (m << 13));
}

__host__ __device__ inline float load(const void* p, int dt, int64_t i) {
  switch (dt) {
    case BT_LOSS_F16: return h2f(((const uint16_t*)p)[i]);
    case BT_LOSS_BF16: return bits_f32((uint32_t)((const uint16_t*)p)[i] << 16);
    case BT_LOSS_U8: return (float)((const uint8_t*)p)[i];
    default: return ((const float*)p)[i];
  }
}

// ---- fp32 math, the same operations on host and device -----------------------------------------------------------------------
// exp(a) for a <= 0 (a NaN stays NaN).  Below -80 the result is flushed to 0 (< 1.9e-35: it keeps every intermediate normal).
__host__ __device__ inline float exp_neg(float a) {
  if (a != a) return a;
  if (a < -80.0f) return 0.0f;
  const float k = rintf(a * 1.44269504f);
  float r = a - k * 0.693145752f;   // ln 2 = 0.693145752 (8 significant bits: k * it is exact) + 1.42860677e-6
  r = r - k * 1.42860677e-6f;
  // exp(r), |r| <= 0.347: Taylor to r^7 (next term < 6e-9 relative)
  float p = 1.98412698e-4f;
  p = p * r + 1.38888889e-3f;
  p = p * r + 8.33333333e-3f;
  p = p * r + 4.16666667e-2f;
  p = p * r + 1.66666667e-1f;
  p = p * r + 0.5f;
  p = p * r + 1.0f;
  p = p * r + 1.0f;
  return p * bits_f32((uint32_t)((int)k + 127) << 23);   // k in [-115, 0]: the scale is a normal power of two
}

// log1p(e) for e in [0, 1] (NaN stays NaN): log(u) of u = 1 + e by u = 2^k m, m in (0.707, 1.415], and
// log m = 2 atanh(s), s = (m - 1) / (m + 1); then scaled by e / (u - 1), which undoes the rounding of u
__host__ __device__ inline float log1p_01(float e) {
  const float u = 1.0f + e;
  if (u == 1.0f) return e;
  float m = u, kl = 0.0f;
  if (u > 1.41421356f) {
    m = u * 0.5f;
    kl = 0.693147181f;
  }
  const float s = (m - 1.0f) / (m + 1.0f), s2 = s * s;
  float p = 1.0f / 11.0f;
  p = p * s2 + 1.0f / 9.0f;
  p = p * s2 + 1.0f / 7.0f;
  p = p * s2 + 0.2f;
  p = p * s2 + 1.0f / 3.0f;
  p = p * s2 + 1.0f;
  const float l = kl + 2.0f * s * p;
  return l * (e / (u - 1.0f));
}

// torch's binary_cross_entropy_with_logits term with pos_weight (loss.cpp) and its derivative in the logit, in torch's backward
// form ((pw y + 1 - y) sigmoid(x) - pw y)
__host__ __device__ inline void bce(float x, float y, float pw, float& loss, float& dx) {
  const float e = exp_neg(-fabsf(x));
  float c = -x;
  c = c < 0.0f ? 0.0f : c;   // clamp_min(-x, 0); NaN stays NaN
  const float lw = (pw - 1.0f) * y + 1.0f;
  loss = (1.0f - y) * x + lw * (log1p_01(e) + c);
  const float r = 1.0f / (1.0f + e);
  const float sig = x >= 0.0f ? r : e * r;   // sigmoid(x) from exp(-|x|)
  const float t = pw * y;
  dx = ((t + 1.0f) - y) * sig - t;
}

// window maximum of a[lo .. hi] (inclusive): the first index of the maximum, or of the last NaN (torch's CPU max_pool1d)
__host__ __device__ inline float window_max(const float* a, int lo, int hi, int& arg) {
  float mv = a[lo];
  arg = lo;
  for (int i = lo + 1; i <= hi; ++i) {
    const float v = a[i];
    if (v > mv || v != v) {
      mv = v;
      arg = i;
    }
  }
  return mv;
}

struct Cfg {
  int kind, tol;
  float pw;
};

// the term of output frame t and d(term)/dX.  xs / ys: logits / targets of the row from frame xb / yb on (staged copies, valid
// over the windows of t); m: the mask value of frame t; *arg: frame of the window's maximum logit.
__host__ __device__ inline void frame_term(const Cfg& c, const float* xs, int xb, const float* ys, int yb, int t, float m,
                                           float& term, float& g, int& arg) {
  const float y = ys[t - yb];
  if (c.kind == BT_LOSS_MASKED) {
    arg = t;
    float l, d;
    bce(xs[t - xb], y, c.pw, l, d);
    term = l * m;
    g = d * m;
    return;
  }
  const float X = window_max(xs, t - c.tol - xb, t + c.tol - xb, arg);
  arg += xb;
  int unused;
  const float S = window_max(ys, t - 2 * c.tol - yb, t + 2 * c.tol - yb, unused);
  float l, d;
  bce(X, y, c.pw, l, d);
  if (c.kind == BT_LOSS_SHIFT_TOLERANT) {
    const float w = (y + (1.0f - S)) * m;   // look_at = cropped targets + (1 - spread targets), times the cropped mask
    term = l * w;
    g = d * w;
  } else {   // splitted: the positive part on the targets, the negative part on the spread targets
    const float wp = y * m, wn = (1.0f - S) * m;
    float l2, d2;
    bce(X, S, c.pw, l2, d2);
    term = l * wp + l2 * wn;
    g = d * wp + d2 * wn;
  }
}

__host__ __device__ inline int halo_of(const Cfg& c) { return c.kind == BT_LOSS_MASKED ? 0 : 2 * c.tol; }

// ---- device ---------------------------------------------------------------------------------------------------------------
struct DevArgs {
  const void* logits;
  const void* targets;
  const void* mask;
  const int64_t* off;
  const float* d_pw;
  int logit_dt, target_dt, mask_dt, n_rows, nseg;
  int64_t min_len, max_len;
  Cfg c;
  double* ws;
  float* grad;
  float* terms;
};

__global__ __launch_bounds__(SEG) void loss_segment_kernel(DevArgs a) {
  __shared__ float xs_s[SEG + 4 * MAXTOL];
  __shared__ float ys_s[SEG + 6 * MAXTOL];
  __shared__ float g_s[SEG + 2 * MAXTOL];
  __shared__ float t_s[SEG + 2 * MAXTOL];
  __shared__ int arg_s[SEG + 2 * MAXTOL];
  __shared__ double red[SEG];
  const int r = blockIdx.x / a.nseg, seg = blockIdx.x % a.nseg, p = threadIdx.x;
  const int64_t base = a.off[r], T64 = a.off[r + 1] - base;
  if (T64 < a.min_len || T64 > a.max_len || base < 0) return;   // (the finishing launch marks the row)
  const int T = (int)T64, j0 = seg * SEG;
  if (j0 >= T) return;
  Cfg c = a.c;
  if (a.d_pw) c.pw = *a.d_pw;
  const int tol = c.kind == BT_LOSS_MASKED ? 0 : c.tol, h = halo_of(c), lo = h, hi = T - h;
  // staged frames: logits [j0 - 2 tol, j0 + SEG + 2 tol), targets [j0 - 3 tol, j0 + SEG + 3 tol), clipped to the row
  const int xb = j0 - 2 * tol, yb = j0 - 3 * tol;
  const int nx = SEG + 4 * tol, ny = SEG + 6 * tol;
  for (int i = p; i < nx; i += SEG) {
    const int f = xb + i;
    xs_s[i] = (f >= 0 && f < T) ? load(a.logits, a.logit_dt, base + f) : 0.0f;
  }
  for (int i = p; i < ny; i += SEG) {
    const int f = yb + i;
    ys_s[i] = (f >= 0 && f < T) ? load(a.targets, a.target_dt, base + f) : 0.0f;
  }
  __syncthreads();
  // terms of the output frames t = j0 - tol + i, i < SEG + 2 tol
  for (int i = p; i < SEG + 2 * tol; i += SEG) {
    const int t = j0 - tol + i;
    float term = 0.0f, g = 0.0f;
    int arg = -1;
    if (t >= lo && t < hi) {
      const float m = a.mask ? load(a.mask, a.mask_dt, base + t) : 1.0f;
      frame_term(c, xs_s, xb, ys_s, yb, t, m, term, g, arg);
    }
    t_s[i] = term;
    g_s[i] = g;
    arg_s[i] = arg;
  }
  __syncthreads();
  const int j = j0 + p;
  const bool in_row = j < T, out_frame = j >= lo && j < hi;
  if (in_row && a.grad) {   // gather: the windows t = j - tol .. j + tol whose maximum is frame j, in ascending t
    float acc = 0.0f;
    for (int i = p; i <= p + 2 * tol; ++i)
      if (arg_s[i] == j) acc += g_s[i];
    a.grad[base + j] = acc;
  }
  if (in_row && a.terms) a.terms[base + j] = out_frame ? t_s[p + tol] : 0.0f;
  red[p] = (in_row && out_frame) ? (double)t_s[p + tol] : 0.0;
  __syncthreads();
  for (int s = SEG / 2; s > 0; s >>= 1) {
    if (p < s) red[p] += red[p + s];
    __syncthreads();
  }
  if (p == 0) a.ws[(size_t)r * a.nseg + seg] = red[0];
}

__device__ inline void store_scalar(void* out, int dt, double v) {
  const float f = (float)v;
  if (dt == BT_LOSS_F16) {
    ((__half*)out)[0] = __float2half(f);
  } else if (dt == BT_LOSS_BF16) {
    uint32_t u = f32_bits(f);
    u = (f != f) ? (u | 0x400000u) : u + 0x7fffu + ((u >> 16) & 1u);   // round to nearest even; NaN stays quiet NaN
    ((uint16_t*)out)[0] = (uint16_t)(u >> 16);
  } else {
    ((float*)out)[0] = f;
  }
}

__global__ __launch_bounds__(FIN) void loss_finish_kernel(const double* ws, const int64_t* off, int n_rows, int nseg,
                                                          int64_t min_len, int64_t max_len, int halo, double* row_sum,
                                                          int64_t* row_count, void* loss, int loss_dt) {
  __shared__ double red[FIN];
  __shared__ int64_t cnt[FIN];
  const int p = threadIdx.x;
  double part = 0.0;
  int64_t n = 0;
  for (int r = p; r < n_rows; r += FIN) {
    const int64_t T = off[r + 1] - off[r];
    double acc = 0.0;
    int64_t k = T - 2 * halo;
    if (T < min_len || T > max_len || off[r] < 0) {   // outside the bounds the caller declared: NaN, count -1
      acc = NAN;
      k = -1;
    } else {
      for (int s = 0; s * (int64_t)SEG < T; ++s) acc += ws[(size_t)r * nseg + s];
    }
    if (row_sum) row_sum[r] = acc;
    if (row_count) row_count[r] = k;
    part += acc;
    n += k;
  }
  red[p] = part;
  cnt[p] = n;
  __syncthreads();
  for (int s = FIN / 2; s > 0; s >>= 1) {
    if (p < s) {
      red[p] += red[p + s];
      cnt[p] += cnt[p + s];
    }
    __syncthreads();
  }
  if (p == 0 && loss) store_scalar(loss, loss_dt, red[0] / (double)cnt[0]);
}

__device__ inline float load_dev(const void* p, int dt) { return load(p, dt, 0); }

__global__ __launch_bounds__(256) void loss_backward_kernel(const float* g, int64_t n, const void* go, int go_dt, double count,
                                                            void* out, int out_dt) {
  const float scale = (float)((double)load_dev(go, go_dt) / count);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = g[i] * scale;
    if (out_dt == BT_LOSS_F16) {
      ((__half*)out)[i] = __float2half(v);
    } else if (out_dt == BT_LOSS_BF16) {
      uint32_t u = f32_bits(v);
      u = (v != v) ? (u | 0x400000u) : u + 0x7fffu + ((u >> 16) & 1u);
      ((uint16_t*)out)[i] = (uint16_t)(u >> 16);
    } else {
      ((float*)out)[i] = v;
    }
  }
}

// ---- host twin ---------------------------------------------------------------------------------------------------------------
// one row: the same staged windows, terms, gathers and segment trees as loss_segment_kernel
double row_host(const Cfg& c, const void* logits, int ldt, const void* targets, int tdt, const void* mask, int mdt, int64_t base,
                int T, float* grad, float* terms) {
  const int tol = c.kind == BT_LOSS_MASKED ? 0 : c.tol, h = halo_of(c), lo = h, hi = T - h;
  std::vector<float> xs(T), ys(T), g(T, 0.0f), tm(T, 0.0f);
  std::vector<int> arg(T, -1);
  for (int f = 0; f < T; ++f) {
    xs[f] = load(logits, ldt, base + f);
    ys[f] = load(targets, tdt, base + f);
  }
  for (int t = lo; t < hi; ++t) {
    const float m = mask ? load(mask, mdt, base + t) : 1.0f;
    frame_term(c, xs.data(), 0, ys.data(), 0, t, m, tm[t], g[t], arg[t]);
  }
  double acc = 0.0, red[SEG];
  for (int j0 = 0; j0 < T; j0 += SEG) {
    for (int p = 0; p < SEG; ++p) {
      const int j = j0 + p;
      red[p] = (j < T && j >= lo && j < hi) ? (double)tm[j] : 0.0;
      if (j >= T) continue;
      if (grad) {
        float s = 0.0f;
        for (int t = j - tol; t <= j + tol; ++t)
          if (t >= lo && t < hi && arg[t] == j) s += g[t];
        grad[base + j] = s;
      }
      if (terms) terms[base + j] = (j >= lo && j < hi) ? tm[j] : 0.0f;
    }
    for (int s = SEG / 2; s > 0; s >>= 1)
      for (int p = 0; p < s; ++p) red[p] += red[p + s];
    acc += red[0];
  }
  return acc;
}

bool dtypes_ok(int ldt, int tdt, const void* mask, int mdt) {
  return ldt >= BT_LOSS_F32 && ldt <= BT_LOSS_BF16 && (tdt == BT_LOSS_F32 || tdt == BT_LOSS_F16) &&
         (!mask || mdt == BT_LOSS_F32 || mdt == BT_LOSS_U8);
}

const char* cfg_error(int kind, int tol) {
  if (kind < BT_LOSS_MASKED || kind > BT_LOSS_SPLITTED) return "bad loss kind";
  if (tol < 0 || tol > MAXTOL) return "tolerance outside [0, BT_LOSS_MAX_TOLERANCE]";
  return nullptr;
}

int64_t min_frames(int kind, int tol) { return kind == BT_LOSS_MASKED ? 0 : 1 + 4 * (int64_t)tol; }

}  // namespace

extern "C" {

size_t bt_bce_loss_workspace_bytes(int n_rows, int64_t max_len) {
  if (n_rows <= 0 || max_len < 0) return 0;
  const int64_t nseg = max_len > 0 ? (max_len + SEG - 1) / SEG : 1;
  if (nseg * n_rows > 0x7fffffff) return 0;
  return (size_t)(nseg * n_rows) * sizeof(double);
}

int bt_bce_loss(void* stream, int kind, int tolerance, float pos_weight, const float* d_pos_weight, const void* d_logits,
                int logit_dtype, const void* d_targets, int target_dtype, const void* d_mask, int mask_dtype,
                const int64_t* d_offsets, int n_rows, int64_t min_len, int64_t max_len, void* d_ws, size_t ws_bytes,
                double* d_row_sum, int64_t* d_row_count, void* d_loss, int loss_dtype, float* d_grad, float* d_terms) {
  if (const char* e = cfg_error(kind, tolerance)) return bt_set_error_external(BT_ERR_ARG, (std::string("bt_bce_loss: ") + e).c_str());
  if (!d_logits || !d_targets || !d_offsets || !d_ws || n_rows <= 0 || !dtypes_ok(logit_dtype, target_dtype, d_mask, mask_dtype) ||
      (d_loss && (loss_dtype < BT_LOSS_F32 || loss_dtype > BT_LOSS_BF16)) || min_len < 0 || max_len < min_len ||
      max_len > 0x7fffffff - SEG)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_bce_loss");
  if (min_len < min_frames(kind, tolerance))
    return bt_set_error_external(BT_ERR_ARG, ("bt_bce_loss: rows of " + std::to_string(min_len) + " frames, the loss needs at least " +
                                              std::to_string(min_frames(kind, tolerance)) + " (1 + 4 * tolerance)").c_str());
  const size_t need = bt_bce_loss_workspace_bytes(n_rows, max_len);
  if (need == 0) return bt_set_error_external(BT_ERR_ARG, "bt_bce_loss: too many segments");
  if (ws_bytes < need) return bt_set_error_external(BT_ERR_WORKSPACE, "bt_bce_loss: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  DevArgs a{};
  a.logits = d_logits;
  a.targets = d_targets;
  a.mask = d_mask;
  a.off = d_offsets;
  a.d_pw = d_pos_weight;
  a.logit_dt = logit_dtype;
  a.target_dt = target_dtype;
  a.mask_dt = mask_dtype;
  a.n_rows = n_rows;
  a.nseg = (int)(need / sizeof(double) / n_rows);
  a.min_len = min_len;
  a.max_len = max_len;
  a.c = Cfg{kind, tolerance, pos_weight};
  a.ws = (double*)d_ws;
  a.grad = d_grad;
  a.terms = d_terms;
  hipLaunchKernelGGL(loss_segment_kernel, dim3(n_rows * a.nseg), dim3(SEG), 0, s, a);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(FIN), 0, s, (const double*)a.ws, d_offsets, n_rows, a.nseg, min_len,
                     max_len, halo_of(a.c), d_row_sum, d_row_count, d_loss, loss_dtype);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string("bt_bce_loss: ") + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_bce_loss_backward(void* stream, const float* d_grad, int64_t n, const void* d_grad_output, int grad_output_dtype,
                         int64_t count, void* d_grad_in, int grad_in_dtype) {
  if (!d_grad || !d_grad_output || !d_grad_in || n < 0 || grad_output_dtype < BT_LOSS_F32 || grad_output_dtype > BT_LOSS_BF16 ||
      grad_in_dtype < BT_LOSS_F32 || grad_in_dtype > BT_LOSS_BF16)
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_bce_loss_backward");
  if (n == 0) return BT_OK;
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(loss_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_grad, n, d_grad_output,
                     grad_output_dtype, (double)count, d_grad_in, grad_in_dtype);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return bt_set_error_external(BT_ERR_HIP, (std::string("bt_bce_loss_backward: ") + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_bce_loss_host(int kind, int tolerance, float pos_weight, const void* logits, int logit_dtype, const void* targets,
                     int target_dtype, const void* mask, int mask_dtype, const int64_t* offsets, int n_rows, double* row_sum,
                     int64_t* row_count, double* total, float* grad, float* terms) {
  if (const char* e = cfg_error(kind, tolerance))
    return bt_set_error_external(BT_ERR_ARG, (std::string("bt_bce_loss_host: ") + e).c_str());
  if (!logits || !targets || !offsets || n_rows <= 0 || !dtypes_ok(logit_dtype, target_dtype, mask, mask_dtype))
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_bce_loss_host");
  const int64_t need = min_frames(kind, tolerance);
  for (int r = 0; r < n_rows; ++r) {
    const int64_t T = offsets[r + 1] - offsets[r];
    if (offsets[r] < 0 || T < need || T > 0x7fffffff - SEG)
      return bt_set_error_external(BT_ERR_ARG, ("bt_bce_loss_host: row " + std::to_string(r) + " has " + std::to_string(T) +
                                                " frames, the loss needs at least " + std::to_string(need) + " (1 + 4 * tolerance)").c_str());
  }
  const Cfg c{kind, tolerance, pos_weight};
  const int h = halo_of(c);
  double red[FIN] = {};
  int64_t cnt[FIN] = {};
  for (int r = 0; r < n_rows; ++r) {
    const int64_t T = offsets[r + 1] - offsets[r];
    const double acc = row_host(c, logits, logit_dtype, targets, target_dtype, mask, mask_dtype, offsets[r], (int)T, grad, terms);
    if (row_sum) row_sum[r] = acc;
    if (row_count) row_count[r] = T - 2 * h;
    red[r % FIN] += acc;
    cnt[r % FIN] += T - 2 * h;
  }
  for (int s = FIN / 2; s > 0; s >>= 1)
    for (int p = 0; p < s; ++p) {
      red[p] += red[p + s];
      cnt[p] += cnt[p + s];
    }
  if (total) *total = red[0] / (double)cnt[0];
  return BT_OK;
}

}  // extern "C"
