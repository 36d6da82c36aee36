// Training forward and backward of the frontend's own units: everything of BeatThis.frontend that is
// no attention / feed-forward leaf (those run on the unit code of train.hip):
//   stem         y = gelu(bn2d(conv(4, 3)/(4, 1) of bn1d(x)))                    (beat_tracker.py:108-126)
//   conv unit    y = gelu(norm(conv(2, 3)/(2, 1) of x)), three instances          (beat_tracker.py:155-166)
//   swap         (b, t, f, c) <-> (b, f, t, c), the layout change between the two directions of a partial transformer
//   projection   y = frontend.linear of "b c f t -> b t (c f)"                    (beat_tracker.py:71-76)
// Activations are the library's (b, t, f, c), channels last, fp32; the parameters are read in the reference's layout straight
// from the nn.Parameter storage and the gradients are written in that layout.  BatchNorm runs on its running statistics
// (eval-mode arithmetic): s = weight / sqrt(var + 1e-5), sh = bias - mean s, evaluated in fp64 and rounded once, by a small
// launch at the head of every call (into the call's workspace).  The bt_front_bn_* entry points run the
// stem and the conv unit on the statistics of the call's own batch instead -- torch's training-mode BatchNorm: the same
// kernels, the fold table written by the launch that finishes the statistics and moves the running buffers, one elementwise
// launch for the GELU, and one that centres the gradient at each BatchNorm's input.
//
// The conv unit's three matrix products are implicit GEMMs on v_mfma_f32_32x32x2_f32: the operand tiles are staged into LDS
// straight from the activation (a row of the implicit A matrix is three runs of 2 Cin floats at t - 1, t, t + 1, zeros
// outside the sequence), no im2col buffer exists.  With rows m = (b, t, f') over the F' = F / 2 output bins:
//   forward          pre [M, Cout]     = A [M, 6 Cin] W^T                  k = dt 2 Cin + df Cin + ci
//   backward-data    gx  [M, 2 Cin]    = G [M, 3 Cout] W                   k = dt Cout + co; the 2 Cin columns of a row are the
//                                                                           bins 2 f', 2 f' + 1 of gx (b, t, f, ci): the products
//                                                                           of the M = B T F, N = Cin form, two rows at a time
//   backward-weight  gW  [Cout, 6 Cin] = sum over rows of G^T A            partials per DW_ROWS rows, added in chunk order
// The forward saves `pre` (the backward needs it for gelu' and for the gain's gradient and would otherwise repeat the GEMM);
// the stem (K = 12, vector unit) recomputes it.
// With `mixed = 1` in the argument struct the same three products run on v_mfma_f32_32x32x16_f16 with both
// operands rounded to fp16 as they are staged (train_front_mixed.inc) and the projection's GEMMs take bt_train_matmul's mixed
// route; everything around the products is the code below either way.
//
// Reproducibility, as in train.hip: no atomics; every output element is written by one thread of one launch; a GEMM element
// sums k ascending; weight gradients over chunks of DW_ROWS rows and column sums over chunks of CS_ROWS rows, partials added in
// chunk order by a second launch; a row's results depend on its own sequence only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/beat_this_amd.h"
#include "train_common.h"   // f32x16, gelu_f, gelu_grad_f

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

constexpr int DW_ROWS = BT_TRAIN_DW_ROWS;
constexpr int CS_ROWS = BT_TRAIN_CS_ROWS;
constexpr int GT = 64;   // GEMM tile: GT x GT outputs, GK deep; four waves, one 32 x 32 MFMA tile each
constexpr int GK = 16;
constexpr int MEL = 128, STEM_C = 32, STEM_F = 32, STEM_TAPS = 12;

unsigned blocks_of(long n, int per) { return (unsigned)((n + per - 1) / per); }
int dw_chunks(long M) { return (int)((M + DW_ROWS - 1) / DW_ROWS); }
int cs_chunks(long M) { return (int)((M + CS_ROWS - 1) / CS_ROWS); }

// fold [4][C]: s, sh, 1 / sqrt(var + eps), mean
__global__ __launch_bounds__(256) void bn_fold_kernel(const float* w, const float* b, const float* mean, const float* var, int C,
                                                      float* fold) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double rstd = 1.0 / sqrt((double)var[c] + 1e-5);
  const double s = (double)w[c] * rstd;
  fold[c] = (float)s;
  fold[C + c] = (float)((double)b[c] - (double)mean[c] * s);
  fold[2 * C + c] = (float)rstd;
  fold[3 * C + c] = mean[c];
}

// part[chunk][j] = sum over the chunk's CS_ROWS rows of a[m][j], rows ascending
__global__ __launch_bounds__(256) void front_colsum_kernel(const float* a, long M, int N, float* part) {
  const int j = blockIdx.y * 256 + threadIdx.x;
  if (j >= N) return;
  const long mb = (long)blockIdx.x * CS_ROWS, me = std::min<long>(M, mb + CS_ROWS);
  float acc = 0.0f;
  for (long m = mb; m < me; ++m) acc += a[m * N + j];
  part[(long)blockIdx.x * N + j] = acc;
}

__global__ __launch_bounds__(256) void front_reduce_kernel(const float* part, long n, int chunks, float* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = part[i];
  for (int c = 1; c < chunks; ++c) acc += part[(long)c * n + i];
  out[i] = acc;
}

void colsum(hipStream_t s, const float* a, long M, int N, float* part, float* out) {
  const int chunks = cs_chunks(M);
  hipLaunchKernelGGL(front_colsum_kernel, dim3((unsigned)chunks, blocks_of(N, 256)), dim3(256), 0, s, a, M, N, part);
  hipLaunchKernelGGL(front_reduce_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, s, (const float*)part, (long)N, chunks, out);
}

// ---- batch-statistics BatchNorm ----------------------------------------------------------------------------
// part[chunk][0][j] = the mean of column j over the chunk's CS_ROWS rows, part[chunk][1][j] = the sum of squared deviations from
// that mean: rows ascending, fp64 (centred per chunk, so nothing cancels whatever the column's offset is)
__global__ __launch_bounds__(256) void bn_moments_kernel(const float* a, long M, int N, double* part) {
  const int j = blockIdx.y * 256 + threadIdx.x;
  if (j >= N) return;
  const long mb = (long)blockIdx.x * CS_ROWS, me = std::min<long>(M, mb + CS_ROWS);
  const float* col = a + mb * N + j;
  double sum = 0.0, mean, m2 = 0.0;
  if (me - mb == CS_ROWS) {   // a whole chunk: its column in registers, all loads in flight at once, the tensor read once
    float v[CS_ROWS];
#pragma unroll
    for (int r = 0; r < CS_ROWS; ++r) v[r] = col[(long)r * N];
#pragma unroll
    for (int r = 0; r < CS_ROWS; ++r) sum += (double)v[r];
    mean = sum / (double)CS_ROWS;
#pragma unroll
    for (int r = 0; r < CS_ROWS; ++r) {
      const double d = (double)v[r] - mean;
      m2 += d * d;
    }
  } else {                    // the ragged last chunk: the same sums in the same order
    const int rows = (int)(me - mb);
    for (int r = 0; r < rows; ++r) sum += (double)col[(long)r * N];
    mean = sum / (double)rows;
    for (int r = 0; r < rows; ++r) {
      const double d = (double)col[(long)r * N] - mean;
      m2 += d * d;
    }
  }
  part[((long)blockIdx.x * 2) * N + j] = mean;
  part[((long)blockIdx.x * 2 + 1) * N + j] = m2;
}

// count, mean and sum of squared deviations of a run of rows; `a` then `b`, the run on the left first (Chan et al.)
struct Moments {
  double n, mean, m2;
};
__device__ inline Moments merge(const Moments& a, const Moments& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double tot = a.n + b.n, d = b.mean - a.mean;
  return Moments{tot, a.mean + d * (b.n / tot), a.m2 + b.m2 + d * d * (a.n * b.n / tot)};
}

// One workgroup per channel merges the chunks' moments in chunk order, fp64: thread t its run of ceil(chunks / 256) consecutive
// chunks one by one, then the 256 runs pairwise, the left neighbour first (a fixed tree over the shapes alone; one thread
// walking 6000 chunks took 1.5 ms).  Thread 0 rounds once: the batch's mean and 1 / sqrt(var_b + eps) go to save_mean /
// save_rstd, the fold table is built from those ROUNDED values (the backward rebuilds the same table from them, bit for bit), and
// the running statistics move: running_mean = 0.9 running_mean + 0.1 mean_b, running_var = 0.9 running_var + 0.1 var_b n /
// (n - 1); channel 0 counts the batch.
__global__ __launch_bounds__(256) void bn_finish_kernel(const double* part, long M, int C, int chunks, const float* w, const float* b,
                                                        float* fold, float* save_mean, float* save_rstd, float* run_mean,
                                                        float* run_var, int64_t* tracked) {
  __shared__ Moments runs[256];
  const int c = blockIdx.x, t = threadIdx.x;
  const int per = (chunks + 255) / 256, k1 = std::min(chunks, (t + 1) * per);
  Moments m{0.0, 0.0, 0.0};
  for (int k = t * per; k < k1; ++k) {
    const double rows = (double)(std::min<long>(M, (long)(k + 1) * CS_ROWS) - (long)k * CS_ROWS);
    m = merge(m, Moments{rows, part[((long)k * 2) * C + c], part[((long)k * 2 + 1) * C + c]});
  }
  runs[t] = m;
  __syncthreads();
  for (int step = 1; step < 256; step <<= 1) {
    if (t % (2 * step) == 0) runs[t] = merge(runs[t], runs[t + step]);
    __syncthreads();
  }
  if (t != 0) return;
  if (c == 0 && tracked) *tracked += 1;
  const double n = runs[0].n, mean = runs[0].mean, var = runs[0].m2 / n;
  const float mean_f = (float)mean, rstd_f = (float)(1.0 / sqrt(var + 1e-5));
  const double s = (double)w[c] * (double)rstd_f;
  fold[c] = (float)s;
  fold[C + c] = (float)((double)b[c] - (double)mean_f * s);
  fold[2 * C + c] = rstd_f;
  fold[3 * C + c] = mean_f;
  save_mean[c] = mean_f;
  save_rstd[c] = rstd_f;
  run_mean[c] = (float)(0.9 * (double)run_mean[c] + 0.1 * mean);
  run_var[c] = (float)(0.9 * (double)run_var[c] + 0.1 * (var * (n / (n - 1.0))));
}

// the backward's fold table, from the forward's saved batch statistics
__global__ __launch_bounds__(256) void bn_fold_saved_kernel(const float* w, const float* b, const float* mean, const float* rstd, int C,
                                                            float* fold) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double s = (double)w[c] * (double)rstd[c];
  fold[c] = (float)s;
  fold[C + c] = (float)((double)b[c] - (double)mean[c] * s);
  fold[2 * C + c] = rstd[c];
  fold[3 * C + c] = mean[c];
}

// y = gelu(s pre + sh), the expression of conv_gemm<0>'s epilogue
__global__ __launch_bounds__(256) void bn_gelu_kernel(const float* pre, const float* fold, long n, int C, float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  y[i] = gelu_f(fold[c] * pre[i] + fold[C + c]);
}

// The statistics are functions of the batch: g [rows, C], the gradient at the BatchNorm's output (times gelu'), becomes
// g - g_bias / n - xhat g_weight / n in place; v is the BatchNorm's input, gb / gw the two column sums.  With gx: gx = s (that)
// and g stays as it is (bn1d, whose output gradient nothing reads afterwards).
__global__ __launch_bounds__(256) void bn_centre_kernel(float* g, const float* v, const float* fold, const float* gb, const float* gw,
                                                        long n, int C, float rows, float* gx) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  const float xhat = (v[i] - fold[3 * C + c]) * fold[2 * C + c];
  const float r = g[i] - gb[c] / rows - xhat * (gw[c] / rows);
  if (gx) gx[i] = r * fold[c];
  else g[i] = r;
}

void batch_stats(hipStream_t s, const float* a, long M, int C, double* part, const float* w, const float* b, float* fold,
                 float* save_mean, float* save_rstd, float* run_mean, float* run_var, int64_t* tracked) {
  const int chunks = cs_chunks(M);
  hipLaunchKernelGGL(bn_moments_kernel, dim3((unsigned)chunks, blocks_of(C, 256)), dim3(256), 0, s, a, M, C, part);
  hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)C), dim3(256), 0, s, (const double*)part, M, C, chunks, w, b, fold,
                     save_mean, save_rstd, run_mean, run_var, tracked);
}

// ---- conv unit -------------------------------------------------------------------------------------------------------------
struct ConvP {
  const float* x;      // [B, T, F, Cin] = [M, 2 Cin]
  const float* w;      // [Cout][Cin][2][3]
  const float* g;      // g_pre [M, Cout]
  const float* fold;   // [4][Cout]
  float* out;
  float* out2;
  int T, Fo, Cin, Cout;
  long M;              // B T Fo
  const _Float16* wh;  // 16-mixed: the packed fp16 weight of the launch's MODE (train_front_mixed.inc)
};

// implicit A of the forward: row m = (b, t, fo), column k = dt 2 Cin + (df Cin + ci); zeros at t + dt - 1 outside [0, T)
__device__ inline float conv_a(const ConvP& p, long m, int k) {
  const int C2 = 2 * p.Cin, dt = k / C2, j = k - dt * C2;
  const int t = (int)((m / p.Fo) % p.T) + dt - 1;
  return t >= 0 && t < p.T ? p.x[(m + (long)(dt - 1) * p.Fo) * C2 + j] : 0.0f;
}
// implicit A of the backward-data: g_conv = g_pre s of row (b, t - (dt - 1), fo), column k = dt Cout + co
__device__ inline float conv_g(const ConvP& p, long m, int k) {
  const int dt = k / p.Cout, co = k - dt * p.Cout;
  const int t = (int)((m / p.Fo) % p.T) - (dt - 1);
  return t >= 0 && t < p.T ? p.g[(m - (long)(dt - 1) * p.Fo) * p.Cout + co] * p.fold[co] : 0.0f;
}
// W[co][ci][df][dt] for j = df Cin + ci
__device__ inline float conv_w(const ConvP& p, int co, int j, int dt) {
  const int df = j / p.Cin, ci = j - df * p.Cin;
  return p.w[((long)co * p.Cin + ci) * 6 + df * 3 + dt];
}

// MODE 0: forward, 1: backward-data, 2: backward-weight (blockIdx.z = chunk of DW_ROWS rows)
template <int MODE>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const ConvP p) {
  __shared__ float As[GK][GT + 4];
  __shared__ float Bs[GK][GT + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, lr = lane & 31, wm = wave >> 1, wn = wave & 1;
  const int C2 = 2 * p.Cin;
  const long GM = MODE == 2 ? (long)p.Cout : p.M;
  const int GN = MODE == 0 ? p.Cout : MODE == 1 ? C2 : 3 * C2;
  const long kb = MODE == 2 ? (long)blockIdx.z * DW_ROWS : 0;
  const long ke = MODE == 0 ? 3L * C2 : MODE == 1 ? 3L * p.Cout : std::min<long>(p.M, kb + DW_ROWS);
  const long m0 = (long)blockIdx.y * GT;
  const int n0 = blockIdx.x * GT;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (long k0 = kb; k0 < ke; k0 += GK) {
#pragma unroll
    for (int i = 0; i < GT * GK / 256; ++i) {
      const int e = tid + i * 256;
      // MODE 0 / 1: the k index runs fastest (a row of A is contiguous in k); MODE 2: the tile's row / column does
      const int kk = MODE == 2 ? e / GT : e % GK, mn = MODE == 2 ? e % GT : e / GK;
      const long gk = k0 + kk, gm = m0 + mn;
      const int gn = n0 + mn;
      float a = 0.0f, b = 0.0f;
      if (gk < ke) {
        if (gm < GM) {
          if (MODE == 0) a = conv_a(p, gm, (int)gk);
          if (MODE == 1) a = conv_g(p, gm, (int)gk);
          if (MODE == 2) a = p.g[gk * p.Cout + gm] * p.fold[gm];
        }
        if (gn < GN) {
          if (MODE == 0) b = conv_w(p, gn, (int)gk % C2, (int)gk / C2);
          if (MODE == 1) b = conv_w(p, (int)gk % p.Cout, gn, (int)gk / p.Cout);
          if (MODE == 2) b = conv_a(p, gk, gn);
        }
      }
      As[kk][mn] = a;
      Bs[kk][mn] = b;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + g][wm * 32 + lr], Bs[kk + g][wn * 32 + lr], acc, 0, 0, 0);
    __syncthreads();
  }
  const int col = n0 + wn * 32 + lr;
  if (col >= GN) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {   // (C / D map of the 32x32 MFMAs: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5))
    const long row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
    if (row >= GM) continue;
    if (MODE == 0) {
      p.out[row * p.Cout + col] = acc[r];
      if (p.out2) p.out2[row * p.Cout + col] = gelu_f(p.fold[col] * acc[r] + p.fold[p.Cout + col]);   // (null: batch statistics)
    } else if (MODE == 1) {
      p.out[row * C2 + col] = acc[r];
    } else {
      p.out[((long)blockIdx.z * p.Cout + row) * (3 * C2) + col] = acc[r];
    }
  }
}

#include "train_front_mixed.inc"   // conv_pack_kernel, conv_gemm_mixed_kernel<MODE>: the same three products on fp16 MFMAs

// gw [Cout][Cin][2][3] = the partials [chunk][Cout][dt 2 Cin + df Cin + ci] added in chunk order
__global__ __launch_bounds__(256) void conv_dw_reduce_kernel(const float* part, int Cout, int Cin, int chunks, float* gw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Cout * Cin * 6) return;
  const int dt = i % 3, df = (i / 3) % 2, ci = (i / 6) % Cin, co = i / (6 * Cin);
  const int k = dt * 2 * Cin + df * Cin + ci;
  const long n = (long)Cout * 6 * Cin;
  float acc = part[(long)co * 6 * Cin + k];
  for (int c = 1; c < chunks; ++c) acc += part[c * n + (long)co * 6 * Cin + k];
  gw[i] = acc;
}

// gp = gy gelu'(s pre + sh), gh = gp (pre - mean) / sqrt(var + eps)
__global__ __launch_bounds__(256) void conv_gpre_kernel(const float* pre, const float* gy, const float* fold, long n, int C, float* gp,
                                                        float* gh) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  const float v = pre[i];
  const float gv = gy[i] * gelu_grad_f(fold[c] * v + fold[C + c]);
  gp[i] = gv;
  gh[i] = gv * ((v - fold[3 * C + c]) * fold[2 * C + c]);
}

// ---- stem: bn1d, conv 1 -> 32 channels (4, 3) / (4, 1), bn2d, GELU; K = 12, on the vector unit --------------------------------
__device__ inline float stem_xn(const float* x, const float* f1, long bt, int f) { return x[bt * MEL + f] * f1[f] + f1[MEL + f]; }

// pre of (row bt = b T + t, fo, co): taps dt ascending, df ascending inside
__device__ inline float stem_pre(const float* x, const float* w, const float* f1, int T, long bt, int fo, int co) {
  const int t = (int)(bt % T);
  float acc = 0.0f;
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
    const int tt = t + dt - 1;
    if (tt < 0 || tt >= T) continue;
#pragma unroll
    for (int df = 0; df < 4; ++df) acc = fmaf(w[co * STEM_TAPS + df * 3 + dt], stem_xn(x, f1, bt + dt - 1, 4 * fo + df), acc);
  }
  return acc;
}

__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* x, const float* w, const float* f1, const float* f2, long BT, int T,
                                                       float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BT * STEM_F * STEM_C) return;
  const int co = (int)(i % STEM_C), fo = (int)((i / STEM_C) % STEM_F);
  const float pre = stem_pre(x, w, f1, T, i / (STEM_F * STEM_C), fo, co);
  y[i] = gelu_f(f2[co] * pre + f2[STEM_C + co]);
}

__global__ __launch_bounds__(256) void stem_gpre_kernel(const float* x, const float* w, const float* f1, const float* f2,
                                                        const float* gy, long BT, int T, float* gp, float* gh) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BT * STEM_F * STEM_C) return;
  const int co = (int)(i % STEM_C), fo = (int)((i / STEM_C) % STEM_F);
  const float pre = stem_pre(x, w, f1, T, i / (STEM_F * STEM_C), fo, co);
  const float gv = gy[i] * gelu_grad_f(f2[co] * pre + f2[STEM_C + co]);
  gp[i] = gv;
  gh[i] = gv * ((pre - f2[3 * STEM_C + co]) * f2[2 * STEM_C + co]);
}

// batch statistics: pre alone, staged in the workspace for its statistics and the GELU pass
__global__ __launch_bounds__(256) void stem_pre_kernel(const float* x, const float* w, const float* f1, long BT, int T, float* pre) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BT * STEM_F * STEM_C) return;
  pre[i] = stem_pre(x, w, f1, T, i / (STEM_F * STEM_C), (int)((i / STEM_C) % STEM_F), (int)(i % STEM_C));
}

// bn_centre_kernel for bn2d, whose input is recomputed
__global__ __launch_bounds__(256) void stem_centre_kernel(const float* x, const float* w, const float* f1, const float* f2, float* g,
                                                          const float* gb, const float* gw, long BT, int T, float rows) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BT * STEM_F * STEM_C) return;
  const int co = (int)(i % STEM_C), fo = (int)((i / STEM_C) % STEM_F);
  const float pre = stem_pre(x, w, f1, T, i / (STEM_F * STEM_C), fo, co);
  const float xhat = (pre - f2[3 * STEM_C + co]) * f2[2 * STEM_C + co];
  g[i] = g[i] - gb[co] / rows - xhat * (gw[co] / rows);
}

// part[chunk][co][df][dt] = sum over the chunk's DW_ROWS rows (b, t, fo) of g_conv[row][co] xn(b, t + dt - 1, 4 fo + df)
__global__ __launch_bounds__(STEM_C * STEM_TAPS) void stem_dw_kernel(const float* x, const float* f1, const float* f2, const float* gp,
                                                                     long M, int T, float* part) {
  const int co = threadIdx.x % STEM_C, tap = threadIdx.x / STEM_C, df = tap / 3, dt = tap % 3;
  const long mb = (long)blockIdx.x * DW_ROWS, me = std::min<long>(M, mb + DW_ROWS);
  const float s = f2[co];
  float acc = 0.0f;
  for (long m = mb; m < me; ++m) {
    const long bt = m / STEM_F;
    const int fo = (int)(m % STEM_F), tt = (int)(bt % T) + dt - 1;
    const float xn = tt >= 0 && tt < T ? stem_xn(x, f1, bt + dt - 1, 4 * fo + df) : 0.0f;
    acc = fmaf(gp[m * STEM_C + co] * s, xn, acc);
  }
  part[((long)blockIdx.x * STEM_C + co) * STEM_TAPS + tap] = acc;
}

// gradient of the bn1d output, per (b, t, f): gxn; ghn = gxn (x - mean) / sqrt(var + eps); gx = gxn s (gx may be null)
__global__ __launch_bounds__(256) void stem_dx_kernel(const float* x, const float* w, const float* f1, const float* f2, const float* gp,
                                                      long BT, int T, float* gxn, float* ghn, float* gx) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BT * MEL) return;
  const int f = (int)(i % MEL), fo = f >> 2, df = f & 3;
  const long bt = i / MEL;
  const int t = (int)(bt % T);
  float acc = 0.0f;
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
    const int tt = t - (dt - 1);
    if (tt < 0 || tt >= T) continue;
    const float* gr = gp + ((bt - (dt - 1)) * STEM_F + fo) * STEM_C;
    for (int co = 0; co < STEM_C; ++co) acc = fmaf(w[co * STEM_TAPS + df * 3 + dt] * f2[co], gr[co], acc);
  }
  gxn[i] = acc;
  ghn[i] = acc * ((x[i] - f1[3 * MEL + f]) * f1[2 * MEL + f]);
  if (gx) gx[i] = acc * f1[f];
}

// ---- layout: y[b][q][p][c] = x[b][p][q][c] ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swap_kernel(const float* x, long n, int P, int Q, int C, float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // index into y
  if (i >= n) return;
  const int c = (int)(i % C);
  const long r = i / C;
  const int p = (int)(r % P), q = (int)((r / P) % Q);
  const long b = r / ((long)P * Q);
  y[i] = x[((b * P + p) * Q + q) * C + c];
}

void swap(hipStream_t s, const float* x, long B, int P, int Q, int C, float* y) {
  const long n = B * P * Q * C;
  hipLaunchKernelGGL(swap_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, x, n, P, Q, C, y);
}

// ---- workspace layouts (floats; every region a multiple of 64 floats) ---------------------------------------------------------
size_t up64(size_t n) { return (n + 63) / 64 * 64; }

struct Layout {
  size_t fold, fold1, a, b, c, d, part, wimg, total;
};

// mixed: the conv unit's fp16 weight image (Cout 6 Cin halves; the forward's, or the backward-data's transposed one)
Layout layout(int unit, int backward, long BT, int F, int C, int dim, bool mixed = false) {
  Layout L{};
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += up64(n); return o; };
  switch (unit) {
    case BT_FRONT_STEM: {
      const size_t M = (size_t)BT * STEM_F;
      L.fold1 = take(4 * MEL);
      L.fold = take(4 * STEM_C);
      if (backward) {
        L.a = take(M * STEM_C);          // g_pre
        L.b = take(M * STEM_C);          // g_pre xhat
        L.c = take((size_t)BT * MEL);    // gradient of the bn1d output
        L.d = take((size_t)BT * MEL);    // the same times xhat
        L.part = take(std::max({(size_t)dw_chunks(M) * STEM_C * STEM_TAPS, (size_t)cs_chunks(M) * STEM_C, (size_t)cs_chunks(BT) * MEL}));
      }
      break;
    }
    case BT_FRONT_CONV: {
      const size_t M = (size_t)BT * (F / 2), Cout = 2 * (size_t)C;
      L.fold = take(4 * Cout);
      if (backward) {
        L.a = take(M * Cout);            // g_pre
        L.b = take(M * Cout);            // g_pre xhat
        L.part = take(std::max((size_t)dw_chunks(M) * Cout * 6 * C, (size_t)cs_chunks(M) * Cout));
      }
      if (mixed) L.wimg = take(Cout * 3 * C);
      break;
    }
    case BT_FRONT_LINEAR: {
      const size_t K = (size_t)F * C;
      L.a = take((size_t)BT * K);        // the input in the weight's column order (c f)
      if (backward) {
        L.b = take((size_t)BT * K);      // its gradient
        L.part = take(std::max(bt_train_matmul_workspace_bytes(2, dim, (int)K, (int)BT) / sizeof(float), (size_t)cs_chunks(BT) * dim));
      }
      break;
    }
    default:
      break;
  }
  L.total = std::max<size_t>(at, 64);
  return L;
}

const char* check_shape(int unit, int B, int T, int F, int C, int dim) {
  if (unit < BT_FRONT_STEM || unit > BT_FRONT_SWAP) return "unit must be BT_FRONT_STEM, _CONV, _LINEAR or _SWAP";
  if (B < 1 || T < 1) return "need B >= 1 and T >= 1";
  if (unit == BT_FRONT_SWAP)   // (serves both directions: T and F are the two swapped extents, whichever is the time)
    return F < 1 || F > (1 << 22) || C < 1 || C > 1024 || (long)B * T > (1L << 22) || (long)B * T * F > (1L << 22)
               ? "the swap needs F >= 1, 1 <= C <= 1024 and B T F <= 2^22 rows"
               : nullptr;
  if ((long)B * T > 65535) return "more than 65535 frames (B T): the frequency direction runs one sequence per frame";
  if ((long)B * T * 32 > (1L << 22)) return "more than 2^22 rows (B T 32)";
  switch (unit) {
    case BT_FRONT_STEM:
      if (F != MEL || C != STEM_C) return "the stem takes F = 128 mel bins and writes C = 32 channels";
      break;
    case BT_FRONT_CONV:
      if (F < 2 || F > 32 || F % 2 || C < 32 || C > 512 || C % 32) return "the conv unit needs an even F <= 32 and C a multiple of 32 up to 512";
      break;
    case BT_FRONT_LINEAR:
      if (F < 1 || F > 32 || C < 32 || C > 1024 || C % 32 || dim < 32 || dim > 1024 || dim % 32)
        return "the projection needs 1 <= F <= 32 and C, dim multiples of 32 up to 1024";
      break;
    default:
      break;
  }
  return nullptr;
}

int fail(const char* fn, const char* msg, int code = BT_ERR_ARG) {
  return bt_set_error_external(code, (std::string(fn) + ": " + msg).c_str());
}

int finish(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(fn, hipGetErrorString(e), BT_ERR_HIP);
  return BT_OK;
}

void fold(hipStream_t s, const float* w, const float* b, const float* mean, const float* var, int C, float* out) {
  hipLaunchKernelGGL(bn_fold_kernel, dim3(blocks_of(C, 256)), dim3(256), 0, s, w, b, mean, var, C, out);
}

dim3 conv_grid(long GM, int GN, int chunks) { return dim3(blocks_of(GN, GT), blocks_of(GM, GT), (unsigned)chunks); }

// 16-mixed: the argument check shared by the four entry points, and the weight image of one MODE
const char* check_mixed(int unit, int mixed, bool linear_too) {
  if (mixed != 0 && mixed != 1) return "mixed must be 0 or 1";
  if (mixed && unit != BT_FRONT_CONV && !(linear_too && unit == BT_FRONT_LINEAR))
    return "mixed = 1 belongs to BT_FRONT_CONV and (bt_front_args) BT_FRONT_LINEAR: the other units have no product worth an MFMA";
  return nullptr;
}

void conv_pack(hipStream_t s, const float* w, int Cout, int Cin, int transposed, float* img) {
  hipLaunchKernelGGL(conv_pack_kernel, dim3(blocks_of((long)Cout * 6 * Cin, 256)), dim3(256), 0, s, w, Cout, Cin, transposed,
                     (_Float16*)img);
}

// the forward GEMM (p.out = pre, p.out2 = y or null); wimg: the workspace of the fp16 weight image, null = the fp32 kernel
void conv_forward_gemm(hipStream_t s, ConvP p, float* wimg) {
  if (wimg) {
    conv_pack(s, p.w, p.Cout, p.Cin, 0, wimg);
    p.wh = (const _Float16*)wimg;
    hipLaunchKernelGGL(conv_gemm_mixed_kernel<0>, conv_grid(p.M, p.Cout, 1), dim3(256), 0, s, p);
  } else {
    hipLaunchKernelGGL(conv_gemm_kernel<0>, conv_grid(p.M, p.Cout, 1), dim3(256), 0, s, p);
  }
}

// the conv unit's backward-data and backward-weight GEMMs on p.g = g_pre (they multiply by s = p.fold while staging)
void conv_backward_gemms(hipStream_t s, ConvP p, float* part, float* gx, float* g_w, float* wimg) {
  if (gx) {
    p.out = gx;
    if (wimg) {
      conv_pack(s, p.w, p.Cout, p.Cin, 1, wimg);
      p.wh = (const _Float16*)wimg;
      hipLaunchKernelGGL(conv_gemm_mixed_kernel<1>, conv_grid(p.M, 2 * p.Cin, 1), dim3(256), 0, s, p);
    } else {
      hipLaunchKernelGGL(conv_gemm_kernel<1>, conv_grid(p.M, 2 * p.Cin, 1), dim3(256), 0, s, p);
    }
  }
  if (g_w) {
    const int chunks = dw_chunks(p.M);
    p.out = part;
    if (wimg)
      hipLaunchKernelGGL(conv_gemm_mixed_kernel<2>, conv_grid(p.Cout, 6 * p.Cin, chunks), dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL(conv_gemm_kernel<2>, conv_grid(p.Cout, 6 * p.Cin, chunks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(conv_dw_reduce_kernel, dim3(blocks_of((long)p.Cout * 6 * p.Cin, 256)), dim3(256), 0, s, (const float*)part,
                       p.Cout, p.Cin, chunks, g_w);
  }
}

// the stem's weight gradient from gp = g_pre
void stem_dw(hipStream_t s, const float* x, const float* f1, const float* f2, const float* gp, long M, int T, float* part, float* g_w) {
  const int chunks = dw_chunks(M);
  hipLaunchKernelGGL(stem_dw_kernel, dim3((unsigned)chunks), dim3(STEM_C * STEM_TAPS), 0, s, x, f1, f2, gp, M, T, part);
  hipLaunchKernelGGL(front_reduce_kernel, dim3(blocks_of(STEM_C * STEM_TAPS, 256)), dim3(256), 0, s, (const float*)part,
                     (long)STEM_C * STEM_TAPS, chunks, g_w);
}

// ---- batch statistics: workspace and argument checks ---------------------------------------------------------------------------
struct BnLayout {
  size_t fold, fold1, pre, a, b, c, d, sums, sums1, part, wimg, total;
};

// a chunk's moments are two doubles per column: four floats of the workspace
BnLayout bn_layout(int unit, int backward, long BT, int F, int C, bool mixed = false) {
  BnLayout L{};
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += up64(n); return o; };
  if (unit == BT_FRONT_STEM) {
    const size_t M = (size_t)BT * STEM_F;
    L.fold1 = take(4 * MEL);
    L.fold = take(4 * STEM_C);
    if (backward) {
      L.a = take(M * STEM_C);          // g_pre
      L.b = take(M * STEM_C);          // g_pre xhat
      L.c = take((size_t)BT * MEL);    // gradient of the bn1d output
      L.d = take((size_t)BT * MEL);    // the same times xhat
      L.sums = take(2 * STEM_C);       // g_bias, g_weight of bn2d when the caller wants none
      L.sums1 = take(2 * MEL);         // the same of bn1d
      L.part = take(std::max({(size_t)dw_chunks(M) * STEM_C * STEM_TAPS, (size_t)cs_chunks(M) * STEM_C, (size_t)cs_chunks(BT) * MEL}));
    } else {
      L.pre = take(M * STEM_C);
      L.part = take(4 * std::max((size_t)cs_chunks(M) * STEM_C, (size_t)cs_chunks(BT) * MEL));
    }
  } else {
    const size_t M = (size_t)BT * (F / 2), Cout = 2 * (size_t)C;
    L.fold = take(4 * Cout);
    if (backward) {
      L.a = take(M * Cout);
      L.b = take(M * Cout);
      L.sums = take(2 * Cout);
      L.part = take(std::max((size_t)dw_chunks(M) * Cout * 6 * C, (size_t)cs_chunks(M) * Cout));
    } else {
      L.part = take(4 * (size_t)cs_chunks(M) * Cout);
    }
    if (mixed) L.wimg = take(Cout * 3 * C);   // the fp16 weight image, as layout()
  }
  L.total = at;
  return L;
}

const char* bn_check_shape(int unit, int B, int T, int F, int C) {
  if (unit != BT_FRONT_STEM && unit != BT_FRONT_CONV) return "batch statistics: unit must be BT_FRONT_STEM or BT_FRONT_CONV";
  if (const char* e = check_shape(unit, B, T, F, C, 0)) return e;
  if ((long)B * T * (unit == BT_FRONT_STEM ? 1 : F / 2) < 2) return "Expected more than 1 value per channel when training";
  return nullptr;
}

}  // namespace

extern "C" {

void bt_front_struct_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(bt_front_args);
  out[1] = (int32_t)offsetof(bt_front_args, w);
  out[2] = (int32_t)offsetof(bt_front_args, x);
  out[3] = (int32_t)offsetof(bt_front_args, gy);
  out[4] = (int32_t)offsetof(bt_front_args, gx);
  out[5] = (int32_t)offsetof(bt_front_args, ws);
  out[6] = (int32_t)offsetof(bt_front_args, ws_bytes);
}

size_t bt_front_workspace_bytes(int unit, int backward, int B, int T, int F, int C, int dim) {
  if (check_shape(unit, B, T, F, C, dim)) return 0;
  return layout(unit, backward != 0, (long)B * T, F, C, dim).total * sizeof(float);
}

size_t bt_front_workspace_bytes_mixed(int unit, int backward, int B, int T, int F, int C, int dim) {
  if (check_shape(unit, B, T, F, C, dim) || check_mixed(unit, 1, true)) return 0;
  return layout(unit, backward != 0, (long)B * T, F, C, dim, true).total * sizeof(float);
}

int bt_front_forward(void* stream, int unit, const bt_front_args* ap) {
  const char* fn = "bt_front_forward";
  if (!ap) return fail(fn, "null argument");
  const bt_front_args& a = *ap;
  if (const char* e = check_shape(unit, a.B, a.T, a.F, a.C, a.dim)) return fail(fn, e);
  if (const char* e = check_mixed(unit, a.mixed, true)) return fail(fn, e);
  const long BT = (long)a.B * a.T;
  const Layout L = layout(unit, 0, BT, a.F, a.C, a.dim, a.mixed != 0);
  if (!a.x || !a.y || !a.ws) return fail(fn, "null x, y or workspace");
  if (a.mixed && (uintptr_t)a.ws % 16) return fail(fn, "mixed = 1: the workspace must be 16-byte aligned");
  if (a.ws_bytes < L.total * sizeof(float)) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)a.ws;
  switch (unit) {
    case BT_FRONT_STEM: {
      if (!a.w || !a.bn_w || !a.bn_b || !a.bn_mean || !a.bn_var || !a.bn1_w || !a.bn1_b || !a.bn1_mean || !a.bn1_var)
        return fail(fn, "null parameter");
      fold(s, a.bn1_w, a.bn1_b, a.bn1_mean, a.bn1_var, MEL, ws + L.fold1);
      fold(s, a.bn_w, a.bn_b, a.bn_mean, a.bn_var, STEM_C, ws + L.fold);
      hipLaunchKernelGGL(stem_fwd_kernel, dim3(blocks_of(BT * STEM_F * STEM_C, 256)), dim3(256), 0, s, a.x, a.w,
                         (const float*)(ws + L.fold1), (const float*)(ws + L.fold), BT, a.T, a.y);
      break;
    }
    case BT_FRONT_CONV: {
      if (!a.w || !a.bn_w || !a.bn_b || !a.bn_mean || !a.bn_var || !a.save_pre) return fail(fn, "null parameter or saved-tensor pointer");
      const int Cout = 2 * a.C;
      fold(s, a.bn_w, a.bn_b, a.bn_mean, a.bn_var, Cout, ws + L.fold);
      conv_forward_gemm(s, ConvP{a.x, a.w, nullptr, ws + L.fold, a.save_pre, a.y, a.T, a.F / 2, a.C, Cout, BT * (a.F / 2)},
                        a.mixed ? ws + L.wimg : nullptr);
      break;
    }
    case BT_FRONT_LINEAR: {
      if (!a.w || !a.b) return fail(fn, "null parameter");
      const int K = a.F * a.C;
      swap(s, a.x, BT, a.F, a.C, 1, ws + L.a);   // (f c) -> (c f)
      if (int rc = bt_train_matmul(stream, a.mixed, 0, ws + L.a, a.w, (int)BT, a.dim, K, a.y, a.b, nullptr, 0, nullptr, nullptr, 0, 0,
                                   nullptr, 0))
        return rc;
      break;
    }
    default:
      swap(s, a.x, a.B, a.T, a.F, a.C, a.y);
      break;
  }
  return finish(fn);
}

int bt_front_backward(void* stream, int unit, const bt_front_args* ap) {
  const char* fn = "bt_front_backward";
  if (!ap) return fail(fn, "null argument");
  const bt_front_args& a = *ap;
  if (const char* e = check_shape(unit, a.B, a.T, a.F, a.C, a.dim)) return fail(fn, e);
  if (const char* e = check_mixed(unit, a.mixed, true)) return fail(fn, e);
  const long BT = (long)a.B * a.T;
  const Layout L = layout(unit, 1, BT, a.F, a.C, a.dim, a.mixed != 0);
  if (!a.gy || !a.ws) return fail(fn, "null upstream gradient or workspace");
  if (unit != BT_FRONT_SWAP && !a.x) return fail(fn, "null x");
  if (a.mixed && (uintptr_t)a.ws % 16) return fail(fn, "mixed = 1: the workspace must be 16-byte aligned");
  if (a.ws_bytes < L.total * sizeof(float)) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)a.ws;
  switch (unit) {
    case BT_FRONT_STEM: {
      if (!a.w || !a.bn_w || !a.bn_b || !a.bn_mean || !a.bn_var || !a.bn1_w || !a.bn1_b || !a.bn1_mean || !a.bn1_var)
        return fail(fn, "null parameter");
      const long M = BT * STEM_F;
      const float* f1 = ws + L.fold1;
      const float* f2 = ws + L.fold;
      fold(s, a.bn1_w, a.bn1_b, a.bn1_mean, a.bn1_var, MEL, ws + L.fold1);
      fold(s, a.bn_w, a.bn_b, a.bn_mean, a.bn_var, STEM_C, ws + L.fold);
      hipLaunchKernelGGL(stem_gpre_kernel, dim3(blocks_of(M * STEM_C, 256)), dim3(256), 0, s, a.x, a.w, f1, f2, a.gy, BT, a.T,
                         ws + L.a, ws + L.b);
      if (a.g_bn_b) colsum(s, ws + L.a, M, STEM_C, ws + L.part, a.g_bn_b);
      if (a.g_bn_w) colsum(s, ws + L.b, M, STEM_C, ws + L.part, a.g_bn_w);
      if (a.g_w) stem_dw(s, a.x, f1, f2, ws + L.a, M, a.T, ws + L.part, a.g_w);
      if (a.gx || a.g_bn1_w || a.g_bn1_b) {
        hipLaunchKernelGGL(stem_dx_kernel, dim3(blocks_of(BT * MEL, 256)), dim3(256), 0, s, a.x, a.w, f1, f2, (const float*)(ws + L.a),
                           BT, a.T, ws + L.c, ws + L.d, a.gx);
        if (a.g_bn1_b) colsum(s, ws + L.c, BT, MEL, ws + L.part, a.g_bn1_b);
        if (a.g_bn1_w) colsum(s, ws + L.d, BT, MEL, ws + L.part, a.g_bn1_w);
      }
      break;
    }
    case BT_FRONT_CONV: {
      if (!a.w || !a.bn_w || !a.bn_b || !a.bn_mean || !a.bn_var || !a.save_pre) return fail(fn, "null parameter or saved-tensor pointer");
      const int Cout = 2 * a.C, Fo = a.F / 2;
      const long M = BT * Fo;
      fold(s, a.bn_w, a.bn_b, a.bn_mean, a.bn_var, Cout, ws + L.fold);
      hipLaunchKernelGGL(conv_gpre_kernel, dim3(blocks_of(M * Cout, 256)), dim3(256), 0, s, (const float*)a.save_pre, a.gy,
                         (const float*)(ws + L.fold), M * Cout, Cout, ws + L.a, ws + L.b);
      if (a.g_bn_b) colsum(s, ws + L.a, M, Cout, ws + L.part, a.g_bn_b);
      if (a.g_bn_w) colsum(s, ws + L.b, M, Cout, ws + L.part, a.g_bn_w);
      conv_backward_gemms(s, ConvP{a.x, a.w, ws + L.a, ws + L.fold, nullptr, nullptr, a.T, Fo, a.C, Cout, M}, ws + L.part, a.gx, a.g_w,
                          a.mixed ? ws + L.wimg : nullptr);
      break;
    }
    case BT_FRONT_LINEAR: {
      if (!a.w) return fail(fn, "null parameter");
      const int K = a.F * a.C;
      if (a.g_b) colsum(s, a.gy, BT, a.dim, ws + L.part, a.g_b);
      if (a.g_w) {
        swap(s, a.x, BT, a.F, a.C, 1, ws + L.a);
        if (int rc = bt_train_matmul(stream, a.mixed, 2, a.gy, ws + L.a, a.dim, K, (int)BT, a.g_w, nullptr, nullptr, 0, nullptr, nullptr, 0, 0,
                                     ws + L.part, (L.total - L.part) * sizeof(float)))
          return rc;
      }
      if (a.gx) {
        if (int rc = bt_train_matmul(stream, a.mixed, 1, a.gy, a.w, (int)BT, K, a.dim, ws + L.b, nullptr, nullptr, 0, nullptr, nullptr, 0, 0,
                                     nullptr, 0))
          return rc;
        swap(s, ws + L.b, BT, a.C, a.F, 1, a.gx);   // (c f) -> (f c)
      }
      break;
    }
    default:   // y = swap(x) over (T, F): gx = the swap over (F, T) of gy
      if (!a.gx) return fail(fn, "null gx");
      swap(s, a.gy, a.B, a.F, a.T, a.C, a.gx);
      break;
  }
  return finish(fn);
}

// ---- batch-statistics BatchNorm: the same kernels, the statistics from the call's own batch -------------
void bt_front_bn_struct_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(bt_front_bn_args);
  out[1] = (int32_t)offsetof(bt_front_bn_args, w);
  out[2] = (int32_t)offsetof(bt_front_bn_args, bn_tracked);
  out[3] = (int32_t)offsetof(bt_front_bn_args, save_mean);
  out[4] = (int32_t)offsetof(bt_front_bn_args, x);
  out[5] = (int32_t)offsetof(bt_front_bn_args, gy);
  out[6] = (int32_t)offsetof(bt_front_bn_args, gx);
  out[7] = (int32_t)offsetof(bt_front_bn_args, ws);
  out[8] = (int32_t)offsetof(bt_front_bn_args, ws_bytes);
}

size_t bt_front_bn_workspace_bytes(int unit, int backward, int B, int T, int F, int C) {
  if (bn_check_shape(unit, B, T, F, C)) return 0;
  return bn_layout(unit, backward != 0, (long)B * T, F, C).total * sizeof(float);
}

size_t bt_front_bn_workspace_bytes_mixed(int unit, int backward, int B, int T, int F, int C) {
  if (bn_check_shape(unit, B, T, F, C) || check_mixed(unit, 1, false)) return 0;
  return bn_layout(unit, backward != 0, (long)B * T, F, C, true).total * sizeof(float);
}

int bt_front_bn_forward(void* stream, int unit, const bt_front_bn_args* ap) {
  const char* fn = "bt_front_bn_forward";
  if (!ap) return fail(fn, "null argument");
  const bt_front_bn_args& a = *ap;
  if (const char* e = bn_check_shape(unit, a.B, a.T, a.F, a.C)) return fail(fn, e);
  if (const char* e = check_mixed(unit, a.mixed, false)) return fail(fn, e);
  const long BT = (long)a.B * a.T;
  const BnLayout L = bn_layout(unit, 0, BT, a.F, a.C, a.mixed != 0);
  if (!a.x || !a.y || !a.ws) return fail(fn, "null x, y or workspace");
  if (!a.w || !a.bn_w || !a.bn_b || !a.bn_mean || !a.bn_var || !a.save_mean || !a.save_rstd)
    return fail(fn, "null parameter, running buffer or saved-statistics pointer");
  if ((uintptr_t)a.ws % 8) return fail(fn, "the workspace must be 8-byte aligned");
  if (a.mixed && (uintptr_t)a.ws % 16) return fail(fn, "mixed = 1: the workspace must be 16-byte aligned");
  if (a.ws_bytes < L.total * sizeof(float)) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)a.ws;
  double* part = (double*)(ws + L.part);
  if (unit == BT_FRONT_STEM) {
    if (!a.bn1_w || !a.bn1_b || !a.bn1_mean || !a.bn1_var || !a.save1_mean || !a.save1_rstd)
      return fail(fn, "null bn1d parameter, running buffer or saved-statistics pointer");
    const long M = BT * STEM_F;
    batch_stats(s, a.x, BT, MEL, part, a.bn1_w, a.bn1_b, ws + L.fold1, a.save1_mean, a.save1_rstd, a.bn1_mean, a.bn1_var, a.bn1_tracked);
    hipLaunchKernelGGL(stem_pre_kernel, dim3(blocks_of(M * STEM_C, 256)), dim3(256), 0, s, a.x, a.w, (const float*)(ws + L.fold1), BT,
                       a.T, ws + L.pre);
    batch_stats(s, ws + L.pre, M, STEM_C, part, a.bn_w, a.bn_b, ws + L.fold, a.save_mean, a.save_rstd, a.bn_mean, a.bn_var, a.bn_tracked);
    hipLaunchKernelGGL(bn_gelu_kernel, dim3(blocks_of(M * STEM_C, 256)), dim3(256), 0, s, (const float*)(ws + L.pre),
                       (const float*)(ws + L.fold), M * STEM_C, STEM_C, a.y);
  } else {
    if (!a.save_pre) return fail(fn, "null saved-tensor pointer");
    const int Cout = 2 * a.C;
    const long M = BT * (a.F / 2);
    // (pre alone: no fold, no GELU output)
    conv_forward_gemm(s, ConvP{a.x, a.w, nullptr, nullptr, a.save_pre, nullptr, a.T, a.F / 2, a.C, Cout, M}, a.mixed ? ws + L.wimg : nullptr);
    batch_stats(s, a.save_pre, M, Cout, part, a.bn_w, a.bn_b, ws + L.fold, a.save_mean, a.save_rstd, a.bn_mean, a.bn_var, a.bn_tracked);
    hipLaunchKernelGGL(bn_gelu_kernel, dim3(blocks_of(M * Cout, 256)), dim3(256), 0, s, (const float*)a.save_pre,
                       (const float*)(ws + L.fold), M * Cout, Cout, a.y);
  }
  return finish(fn);
}

int bt_front_bn_backward(void* stream, int unit, const bt_front_bn_args* ap) {
  const char* fn = "bt_front_bn_backward";
  if (!ap) return fail(fn, "null argument");
  const bt_front_bn_args& a = *ap;
  if (const char* e = bn_check_shape(unit, a.B, a.T, a.F, a.C)) return fail(fn, e);
  if (const char* e = check_mixed(unit, a.mixed, false)) return fail(fn, e);
  const long BT = (long)a.B * a.T;
  const BnLayout L = bn_layout(unit, 1, BT, a.F, a.C, a.mixed != 0);
  if (!a.x || !a.gy || !a.ws) return fail(fn, "null x, upstream gradient or workspace");
  if (a.mixed && (uintptr_t)a.ws % 16) return fail(fn, "mixed = 1: the workspace must be 16-byte aligned");
  if (!a.w || !a.bn_w || !a.bn_b || !a.save_mean || !a.save_rstd) return fail(fn, "null parameter or saved-statistics pointer");
  if (a.ws_bytes < L.total * sizeof(float)) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)a.ws;
  const float* f2 = ws + L.fold;
  if (unit == BT_FRONT_STEM) {
    if (!a.bn1_w || !a.bn1_b || !a.save1_mean || !a.save1_rstd) return fail(fn, "null bn1d parameter or saved-statistics pointer");
    const long M = BT * STEM_F;
    const float* f1 = ws + L.fold1;
    float* gb = a.g_bn_b ? a.g_bn_b : ws + L.sums;
    float* gw = a.g_bn_w ? a.g_bn_w : ws + L.sums + STEM_C;
    hipLaunchKernelGGL(bn_fold_saved_kernel, dim3(1), dim3(256), 0, s, a.bn1_w, a.bn1_b, (const float*)a.save1_mean,
                       (const float*)a.save1_rstd, MEL, ws + L.fold1);
    hipLaunchKernelGGL(bn_fold_saved_kernel, dim3(1), dim3(256), 0, s, a.bn_w, a.bn_b, (const float*)a.save_mean,
                       (const float*)a.save_rstd, STEM_C, ws + L.fold);
    hipLaunchKernelGGL(stem_gpre_kernel, dim3(blocks_of(M * STEM_C, 256)), dim3(256), 0, s, a.x, a.w, f1, f2, a.gy, BT, a.T, ws + L.a,
                       ws + L.b);
    colsum(s, ws + L.a, M, STEM_C, ws + L.part, gb);
    colsum(s, ws + L.b, M, STEM_C, ws + L.part, gw);
    hipLaunchKernelGGL(stem_centre_kernel, dim3(blocks_of(M * STEM_C, 256)), dim3(256), 0, s, a.x, a.w, f1, f2, ws + L.a,
                       (const float*)gb, (const float*)gw, BT, a.T, (float)M);
    if (a.g_w) stem_dw(s, a.x, f1, f2, ws + L.a, M, a.T, ws + L.part, a.g_w);
    if (a.gx || a.g_bn1_w || a.g_bn1_b) {
      float* gb1 = a.g_bn1_b ? a.g_bn1_b : ws + L.sums1;
      float* gw1 = a.g_bn1_w ? a.g_bn1_w : ws + L.sums1 + MEL;
      hipLaunchKernelGGL(stem_dx_kernel, dim3(blocks_of(BT * MEL, 256)), dim3(256), 0, s, a.x, a.w, f1, f2, (const float*)(ws + L.a), BT,
                         a.T, ws + L.c, ws + L.d, (float*)nullptr);
      colsum(s, ws + L.c, BT, MEL, ws + L.part, gb1);
      colsum(s, ws + L.d, BT, MEL, ws + L.part, gw1);
      if (a.gx)
        hipLaunchKernelGGL(bn_centre_kernel, dim3(blocks_of(BT * MEL, 256)), dim3(256), 0, s, ws + L.c, a.x, f1, (const float*)gb1,
                           (const float*)gw1, BT * MEL, MEL, (float)BT, a.gx);
    }
  } else {
    if (!a.save_pre) return fail(fn, "null saved-tensor pointer");
    const int Cout = 2 * a.C, Fo = a.F / 2;
    const long M = BT * Fo;
    float* gb = a.g_bn_b ? a.g_bn_b : ws + L.sums;
    float* gw = a.g_bn_w ? a.g_bn_w : ws + L.sums + Cout;
    hipLaunchKernelGGL(bn_fold_saved_kernel, dim3(blocks_of(Cout, 256)), dim3(256), 0, s, a.bn_w, a.bn_b, (const float*)a.save_mean,
                       (const float*)a.save_rstd, Cout, ws + L.fold);
    hipLaunchKernelGGL(conv_gpre_kernel, dim3(blocks_of(M * Cout, 256)), dim3(256), 0, s, (const float*)a.save_pre, a.gy, f2, M * Cout,
                       Cout, ws + L.a, ws + L.b);
    colsum(s, ws + L.a, M, Cout, ws + L.part, gb);
    colsum(s, ws + L.b, M, Cout, ws + L.part, gw);
    hipLaunchKernelGGL(bn_centre_kernel, dim3(blocks_of(M * Cout, 256)), dim3(256), 0, s, ws + L.a, (const float*)a.save_pre, f2,
                       (const float*)gb, (const float*)gw, M * Cout, Cout, (float)M, (float*)nullptr);
    conv_backward_gemms(s, ConvP{a.x, a.w, ws + L.a, f2, nullptr, nullptr, a.T, Fo, a.C, Cout, M}, ws + L.part, a.gx, a.g_w,
                        a.mixed ? ws + L.wimg : nullptr);
  }
  return finish(fn);
}

}  // extern "C"
