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
// Both families of entry points fill one description of the call (Call) and run one preamble and one launch sequence per unit and
// direction, which branches on `batch` at exactly those three points.  Every refusal comes before any launch, checked in this
// order: null struct, shape, mixed, required pointers, workspace alignment, workspace size.
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
// route; `operand = BT_OPERAND_BF16` beside it (section 24) rounds to bfloat16 on v_mfma_f32_32x32x16_bf16 instead, and
// `BT_OPERAND_BF16X3` (section 25) splits every operand into two bfloat16 images for three such MFMAs per product; everything
// around the products is the code below either way.
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

// fold [4][C]: s, sh, 1 / sqrt(var + eps), mean.  The one writer of a channel's four entries: s = w rstd in fp64, rounded once.
__device__ inline void write_fold(float* fold, int C, int c, float w, float b, float mean, double rstd) {
  const double s = (double)w * rstd;
  fold[c] = (float)s;
  fold[C + c] = (float)((double)b - (double)mean * s);
  fold[2 * C + c] = (float)rstd;
  fold[3 * C + c] = mean;
}

// saved == 0: stat = the running variance, rstd stays unrounded fp64 inside s; saved != 0: stat = the forward's saved batch
// rstd, the ROUNDED value bn_finish_kernel built its table from (the backward rebuilds that table bit for bit)
__global__ __launch_bounds__(256) void bn_fold_kernel(const float* w, const float* b, const float* mean, const float* stat, int saved,
                                                      int C, float* fold) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  write_fold(fold, C, c, w[c], b[c], mean[c], saved ? (double)stat[c] : 1.0 / sqrt((double)stat[c] + 1e-5));
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
  write_fold(fold, C, c, w[c], b[c], mean_f, (double)rstd_f);
  save_mean[c] = mean_f;
  save_rstd[c] = rstd_f;
  run_mean[c] = (float)(0.9 * (double)run_mean[c] + 0.1 * mean);
  run_var[c] = (float)(0.9 * (double)run_var[c] + 0.1 * (var * (n / (n - 1.0))));
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
  const void* wh;      // 16-mixed: the packed fp16 / bfloat16 weight of the launch's MODE (train_front_mixed.inc)
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

// The frame of a conv GEMM, the fp32 kernel's below and the fp16 one's in train_front_mixed.inc: what differs between the two is
// how the operand tiles are staged and multiplied, nothing else.
// MODE 0: forward, 1: backward-data, 2: backward-weight (blockIdx.z = chunk of DW_ROWS rows).  The product is GM x GN; a workgroup
// owns the GT x GT tile at (m0, n0) and sums k over [kb, ke).
template <int MODE>
struct ConvTile {
  int C2;
  long GM;
  int GN;
  long kb, ke, m0;
  int n0;
  __device__ explicit ConvTile(const ConvP& p)
      : C2(2 * p.Cin),
        GM(MODE == 2 ? (long)p.Cout : p.M),
        GN(MODE == 0 ? p.Cout : MODE == 1 ? C2 : 3 * C2),
        kb(MODE == 2 ? (long)blockIdx.z * DW_ROWS : 0),
        ke(MODE == 0 ? 3L * C2 : MODE == 1 ? 3L * p.Cout : std::min<long>(p.M, kb + DW_ROWS)),
        m0((long)blockIdx.y * GT),
        n0(blockIdx.x * GT) {}
};

// The epilogue of wave (wm, wn), lane (g, lr): the 32 x 32 accumulator tile to p.out (MODE 0: pre, and y = gelu(s pre + sh) to
// p.out2 unless that is null; MODE 1: g_x; MODE 2: the chunk's partial of g_W).  C / D map of the 32x32 MFMAs, fp32 and fp16
// alike: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
template <int MODE>
__device__ inline void conv_store(const ConvP& p, const ConvTile<MODE> t, const f32x16& acc, int wm, int wn, int lr, int g) {
  const int col = t.n0 + wn * 32 + lr;
  if (col >= t.GN) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long row = t.m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
    if (row >= t.GM) continue;
    if (MODE == 0) {
      p.out[row * p.Cout + col] = acc[r];
      if (p.out2) p.out2[row * p.Cout + col] = gelu_f(p.fold[col] * acc[r] + p.fold[p.Cout + col]);   // (null: batch statistics)
    } else if (MODE == 1) {
      p.out[row * t.C2 + col] = acc[r];
    } else {
      p.out[((long)blockIdx.z * p.Cout + row) * (3 * t.C2) + col] = acc[r];
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const ConvP p) {
  __shared__ float As[GK][GT + 4];
  __shared__ float Bs[GK][GT + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, lr = lane & 31, wm = wave >> 1, wn = wave & 1;
  const ConvTile<MODE> tile(p);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (long k0 = tile.kb; k0 < tile.ke; k0 += GK) {
#pragma unroll
    for (int i = 0; i < GT * GK / 256; ++i) {
      const int e = tid + i * 256;
      // MODE 0 / 1: the k index runs fastest (a row of A is contiguous in k); MODE 2: the tile's row / column does
      const int kk = MODE == 2 ? e / GT : e % GK, mn = MODE == 2 ? e % GT : e / GK;
      const long gk = k0 + kk, gm = tile.m0 + mn;
      const int gn = tile.n0 + mn;
      float a = 0.0f, b = 0.0f;
      if (gk < tile.ke) {
        if (gm < tile.GM) {
          if (MODE == 0) a = conv_a(p, gm, (int)gk);
          if (MODE == 1) a = conv_g(p, gm, (int)gk);
          if (MODE == 2) a = p.g[gk * p.Cout + gm] * p.fold[gm];
        }
        if (gn < tile.GN) {
          if (MODE == 0) b = conv_w(p, gn, (int)gk % tile.C2, (int)gk / tile.C2);
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
  conv_store<MODE>(p, tile, acc, wm, wn, lr, g);
}

#include "train_front_mixed.inc"   // conv_pack_kernel<E>, conv_gemm_mixed_kernel<E, MODE>: the same three products on 16-bit MFMAs

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

// The head of the stem's four elementwise kernels: this thread's flat element i = (bt, fo, co) of the [BT, 32, 32] output, its
// channel and its recomputed pre; `in` is false past the end
struct StemElement {
  long i;
  int co;
  float pre;
  bool in;
};
__device__ inline StemElement stem_element(const float* x, const float* w, const float* f1, long BT, int T) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BT * STEM_F * STEM_C) return StemElement{i, 0, 0.0f, false};
  const int co = (int)(i % STEM_C), fo = (int)((i / STEM_C) % STEM_F);
  return StemElement{i, co, stem_pre(x, w, f1, T, i / (STEM_F * STEM_C), fo, co), true};
}

__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* x, const float* w, const float* f1, const float* f2, long BT, int T,
                                                       float* y) {
  const StemElement e = stem_element(x, w, f1, BT, T);
  if (e.in) y[e.i] = gelu_f(f2[e.co] * e.pre + f2[STEM_C + e.co]);
}

__global__ __launch_bounds__(256) void stem_gpre_kernel(const float* x, const float* w, const float* f1, const float* f2,
                                                        const float* gy, long BT, int T, float* gp, float* gh) {
  const StemElement e = stem_element(x, w, f1, BT, T);
  if (!e.in) return;
  const float gv = gy[e.i] * gelu_grad_f(f2[e.co] * e.pre + f2[STEM_C + e.co]);
  gp[e.i] = gv;
  gh[e.i] = gv * ((e.pre - f2[3 * STEM_C + e.co]) * f2[2 * STEM_C + e.co]);
}

// batch statistics: pre alone, staged in the workspace for its statistics and the GELU pass
__global__ __launch_bounds__(256) void stem_pre_kernel(const float* x, const float* w, const float* f1, long BT, int T, float* pre) {
  const StemElement e = stem_element(x, w, f1, BT, T);
  if (e.in) pre[e.i] = e.pre;
}

// bn_centre_kernel for bn2d, whose input is recomputed
__global__ __launch_bounds__(256) void stem_centre_kernel(const float* x, const float* w, const float* f1, const float* f2, float* g,
                                                          const float* gb, const float* gw, long BT, int T, float rows) {
  const StemElement e = stem_element(x, w, f1, BT, T);
  if (!e.in) return;
  const float xhat = (e.pre - f2[3 * STEM_C + e.co]) * f2[2 * STEM_C + e.co];
  g[e.i] = g[e.i] - gb[e.co] / rows - xhat * (gw[e.co] / rows);
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

// ---- workspace layout (floats; every region a multiple of 64 floats) -----------------------------------------------------------
size_t up64(size_t n) { return (n + 63) / 64 * 64; }

struct Layout {
  size_t fold, fold1, pre, a, b, c, d, sums, sums1, part, wimg, total;
};

// The one layout of every route.  batch (section 18) adds the column sums of the backward (its centring needs them whether the
// caller wants them or not) and, to the forward, the stem's staged pre and the chunks' moments (two doubles per column: four floats
// of the workspace); mixed (section 19) adds the conv unit's fp16 weight image (Cout 6 Cin halves; the forward's, or the
// backward-data's transposed one) `images` times: one for fp16 or bfloat16 operands, the hi and the lo image for the split ones
// of section 25.
int images_of(int mixed, int operand) { return pick_route(route_of(mixed, operand), 0, BT_FOR_OPERANDS(operand_images)); }
Layout layout(int unit, bool backward, bool batch, int images, long BT, int F, int C, int dim) {
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
        if (batch) {
          L.sums = take(2 * STEM_C);     // g_bias, g_weight of bn2d when the caller wants none
          L.sums1 = take(2 * MEL);       // the same of bn1d
        }
        L.part = take(std::max({(size_t)dw_chunks(M) * STEM_C * STEM_TAPS, (size_t)cs_chunks(M) * STEM_C, (size_t)cs_chunks(BT) * MEL}));
      } else if (batch) {
        L.pre = take(M * STEM_C);
        L.part = take(4 * std::max((size_t)cs_chunks(M) * STEM_C, (size_t)cs_chunks(BT) * MEL));
      }
      break;
    }
    case BT_FRONT_CONV: {
      const size_t M = (size_t)BT * (F / 2), Cout = 2 * (size_t)C;
      L.fold = take(4 * Cout);
      if (backward) {
        L.a = take(M * Cout);            // g_pre
        L.b = take(M * Cout);            // g_pre xhat
        if (batch) L.sums = take(2 * Cout);
        L.part = take(std::max((size_t)dw_chunks(M) * Cout * 6 * C, (size_t)cs_chunks(M) * Cout));
      } else if (batch) {
        L.part = take(4 * (size_t)cs_chunks(M) * Cout);
      }
      if (images) L.wimg = take(images * Cout * 3 * C);
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

const char* bn_check_shape(int unit, int B, int T, int F, int C) {
  if (unit != BT_FRONT_STEM && unit != BT_FRONT_CONV) return "batch statistics: unit must be BT_FRONT_STEM or BT_FRONT_CONV";
  if (const char* e = check_shape(unit, B, T, F, C, 0)) return e;
  if ((long)B * T * (unit == BT_FRONT_STEM ? 1 : F / 2) < 2) return "Expected more than 1 value per channel when training";
  return nullptr;
}

// 16-mixed: the units that have a mixed form (the projection's is bt_train_matmul's, which bt_front_bn_args does not reach), and
// the operand format, which only a mixed call reads
const char* check_mixed(int unit, int mixed, int operand, bool linear_too) {
  if (mixed != 0 && mixed != 1) return "mixed must be 0 or 1";
  if (mixed && unit != BT_FRONT_CONV && !(linear_too && unit == BT_FRONT_LINEAR))
    return "mixed = 1 belongs to BT_FRONT_CONV and (bt_front_args) BT_FRONT_LINEAR: the other units have no product worth an MFMA";
  if (mixed && !known_operand(operand)) return "mixed = 1: operand must be BT_OPERAND_F16, BT_OPERAND_BF16 or BT_OPERAND_BF16X3";
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

// ---- one description of a call, whichever argument struct it came in ------------------------------------------------------------
// One BatchNorm: gain and bias; the running buffers (read on running statistics, moved by the batch forward, left alone by the
// batch backward); the batch route's counter and saved statistics; the two gradients.
struct Bn {
  const float *w, *b;
  float *mean, *var;
  int64_t* tracked;
  float *save_mean, *save_rstd;
  float *g_w, *g_b;
};

struct Call {
  int B, T, F, C, dim;
  int mixed, operand;   // as the caller gave them: check_mixed refuses what it does not know
  bool batch, backward;
  Bn bn, bn1;  // bn2d or blocks.i.norm; the stem's bn1d
  const float *w, *b, *x, *gy;
  float *y, *save_pre, *gx, *g_w, *g_b;
  void* ws;
  size_t ws_bytes;
};

Call describe(const bt_front_args& a, bool backward) {
  Call c{a.B, a.T, a.F, a.C, a.dim, a.mixed, a.operand, false, backward};
  // (running statistics: the two buffers are only read)
  c.bn = Bn{a.bn_w, a.bn_b, const_cast<float*>(a.bn_mean), const_cast<float*>(a.bn_var), nullptr, nullptr, nullptr, a.g_bn_w, a.g_bn_b};
  c.bn1 = Bn{a.bn1_w, a.bn1_b, const_cast<float*>(a.bn1_mean), const_cast<float*>(a.bn1_var), nullptr, nullptr, nullptr, a.g_bn1_w, a.g_bn1_b};
  c.w = a.w, c.b = a.b, c.x = a.x, c.gy = a.gy;
  c.y = a.y, c.save_pre = a.save_pre, c.gx = a.gx, c.g_w = a.g_w, c.g_b = a.g_b;
  c.ws = a.ws, c.ws_bytes = a.ws_bytes;
  return c;
}

Call describe(const bt_front_bn_args& a, bool backward) {
  Call c{a.B, a.T, a.F, a.C, 0, a.mixed, a.operand, true, backward};
  c.bn = Bn{a.bn_w, a.bn_b, a.bn_mean, a.bn_var, a.bn_tracked, a.save_mean, a.save_rstd, a.g_bn_w, a.g_bn_b};
  c.bn1 = Bn{a.bn1_w, a.bn1_b, a.bn1_mean, a.bn1_var, a.bn1_tracked, a.save1_mean, a.save1_rstd, a.g_bn1_w, a.g_bn1_b};
  c.w = a.w, c.x = a.x, c.gy = a.gy;
  c.y = a.y, c.save_pre = a.save_pre, c.gx = a.gx, c.g_w = a.g_w;
  c.ws = a.ws, c.ws_bytes = a.ws_bytes;
  return c;
}

// what the call needs of one BatchNorm
bool bn_complete(const Call& c, const Bn& n) {
  return n.w && n.b && ((c.batch && c.backward) || (n.mean && n.var)) && (!c.batch || (n.save_mean && n.save_rstd));
}

// the required pointers; the texts name the groups as each entry point's documentation does
const char* check_pointers(int unit, const Call& c) {
  const bool stem = unit == BT_FRONT_STEM, conv = unit == BT_FRONT_CONV;
  if (c.batch) {
    if (!c.backward && (!c.x || !c.y || !c.ws)) return "null x, y or workspace";
    if (c.backward && (!c.x || !c.gy || !c.ws)) return "null x, upstream gradient or workspace";
    if (!c.w || !bn_complete(c, c.bn))
      return c.backward ? "null parameter or saved-statistics pointer" : "null parameter, running buffer or saved-statistics pointer";
    if (stem && !bn_complete(c, c.bn1))
      return c.backward ? "null bn1d parameter or saved-statistics pointer"
                        : "null bn1d parameter, running buffer or saved-statistics pointer";
    if (conv && !c.save_pre) return "null saved-tensor pointer";
    return nullptr;
  }
  if (!c.backward && (!c.x || !c.y || !c.ws)) return "null x, y or workspace";
  if (c.backward && (!c.gy || !c.ws)) return "null upstream gradient or workspace";
  if (c.backward && unit != BT_FRONT_SWAP && !c.x) return "null x";
  if (stem && (!c.w || !bn_complete(c, c.bn) || !bn_complete(c, c.bn1))) return "null parameter";
  if (conv && (!c.w || !bn_complete(c, c.bn) || !c.save_pre)) return "null parameter or saved-tensor pointer";
  if (unit == BT_FRONT_LINEAR && (!c.w || (!c.backward && !c.b))) return "null parameter";
  if (unit == BT_FRONT_SWAP && c.backward && !c.gx) return "null gx";
  return nullptr;
}

// The preamble of the four entry points, before any launch.  The order: shape, mixed, required pointers, alignment, workspace size.
int prepare(const char* fn, int unit, const Call& c, Layout& L) {
  const char* e = c.batch ? bn_check_shape(unit, c.B, c.T, c.F, c.C) : check_shape(unit, c.B, c.T, c.F, c.C, c.dim);
  if (!e) e = check_mixed(unit, c.mixed, c.operand, !c.batch);
  if (!e) e = check_pointers(unit, c);
  if (!e && c.batch && !c.backward && (uintptr_t)c.ws % 8) e = "the workspace must be 8-byte aligned";   // (the moments are doubles)
  if (!e && c.mixed && (uintptr_t)c.ws % 16) e = "mixed = 1: the workspace must be 16-byte aligned";
  if (e) return fail(fn, e);
  L = layout(unit, c.backward, c.batch, images_of(c.mixed, c.operand), (long)c.B * c.T, c.F, c.C, c.dim);
  if (c.ws_bytes < L.total * sizeof(float)) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
  return BT_OK;
}

// ---- launch sequences: one per unit and direction.  They branch on c.batch where section 18 says the routes differ: where the
// fold table comes from (fold_table), one centring launch per BatchNorm in the backward, the GELU as a launch of its own in the
// forward -----------------------------------------------------------------------------------------------------------------------
// On running statistics the table is folded from the running buffers; the batch forward takes the moments of v [rows, C] (and
// writes the saved statistics and moves the running buffers in the same launch); the batch backward folds the saved statistics.
void fold_table(hipStream_t s, const Call& c, const Bn& n, int C, const float* v, long rows, const Layout& L, float* out) {
  if (c.batch && !c.backward) {
    const int chunks = cs_chunks(rows);
    double* part = (double*)((float*)c.ws + L.part);
    hipLaunchKernelGGL(bn_moments_kernel, dim3((unsigned)chunks, blocks_of(C, 256)), dim3(256), 0, s, v, rows, C, part);
    hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)C), dim3(256), 0, s, (const double*)part, rows, C, chunks, n.w, n.b, out,
                       n.save_mean, n.save_rstd, n.mean, n.var, n.tracked);
  } else {
    hipLaunchKernelGGL(bn_fold_kernel, dim3(blocks_of(C, 256)), dim3(256), 0, s, n.w, n.b, (const float*)(c.batch ? n.save_mean : n.mean),
                       (const float*)(c.batch ? n.save_rstd : n.var), (int)c.batch, C, out);
  }
}

// g_bias = the column sums of g, g_weight = those of gh = g xhat, into the caller's pointers; on batch statistics, whose centring
// reads both, into `spare` [2][C] of the workspace where the caller gave none.  Returns where they are.
struct BnSums {
  const float *b, *w;
};
BnSums bn_sums(hipStream_t s, const Call& c, const Bn& n, const float* g, const float* gh, long M, int C, float* part, float* spare) {
  float* gb = n.g_b ? n.g_b : c.batch ? spare : nullptr;
  float* gw = n.g_w ? n.g_w : c.batch ? spare + C : nullptr;
  if (gb) colsum(s, g, M, C, part, gb);
  if (gw) colsum(s, gh, M, C, part, gw);
  return BnSums{gb, gw};
}

void stem_forward(hipStream_t s, const Call& c, const Layout& L) {
  float* ws = (float*)c.ws;
  const long BT = (long)c.B * c.T, M = BT * STEM_F;
  const float *f1 = ws + L.fold1, *f2 = ws + L.fold, *pre = ws + L.pre;
  const dim3 grid(blocks_of(M * STEM_C, 256));
  fold_table(s, c, c.bn1, MEL, c.x, BT, L, ws + L.fold1);
  if (c.batch)   // bn2d's statistics are those of pre: staged, then its table, then the GELU
    hipLaunchKernelGGL(stem_pre_kernel, grid, dim3(256), 0, s, c.x, c.w, f1, BT, c.T, ws + L.pre);
  fold_table(s, c, c.bn, STEM_C, pre, M, L, ws + L.fold);
  if (c.batch)
    hipLaunchKernelGGL(bn_gelu_kernel, grid, dim3(256), 0, s, pre, f2, M * STEM_C, STEM_C, c.y);
  else
    hipLaunchKernelGGL(stem_fwd_kernel, grid, dim3(256), 0, s, c.x, c.w, f1, f2, BT, c.T, c.y);
}

void stem_backward(hipStream_t s, const Call& c, const Layout& L) {
  float* ws = (float*)c.ws;
  const long BT = (long)c.B * c.T, M = BT * STEM_F;
  const float *f1 = ws + L.fold1, *f2 = ws + L.fold, *gp = ws + L.a;
  float* part = ws + L.part;
  fold_table(s, c, c.bn1, MEL, nullptr, 0, L, ws + L.fold1);
  fold_table(s, c, c.bn, STEM_C, nullptr, 0, L, ws + L.fold);
  hipLaunchKernelGGL(stem_gpre_kernel, dim3(blocks_of(M * STEM_C, 256)), dim3(256), 0, s, c.x, c.w, f1, f2, c.gy, BT, c.T, ws + L.a,
                     ws + L.b);
  const BnSums g = bn_sums(s, c, c.bn, gp, ws + L.b, M, STEM_C, part, ws + L.sums);
  if (c.batch)
    hipLaunchKernelGGL(stem_centre_kernel, dim3(blocks_of(M * STEM_C, 256)), dim3(256), 0, s, c.x, c.w, f1, f2, ws + L.a, g.b, g.w, BT,
                       c.T, (float)M);
  if (c.g_w) {   // the weight gradient from gp = g_pre
    const int chunks = dw_chunks(M);
    hipLaunchKernelGGL(stem_dw_kernel, dim3((unsigned)chunks), dim3(STEM_C * STEM_TAPS), 0, s, c.x, f1, f2, gp, M, c.T, part);
    hipLaunchKernelGGL(front_reduce_kernel, dim3(blocks_of(STEM_C * STEM_TAPS, 256)), dim3(256), 0, s, (const float*)part,
                       (long)STEM_C * STEM_TAPS, chunks, c.g_w);
  }
  if (c.gx || c.bn1.g_w || c.bn1.g_b) {
    // running statistics: stem_dx writes gx = gxn s itself; batch statistics: gx is the centred gxn, times s
    hipLaunchKernelGGL(stem_dx_kernel, dim3(blocks_of(BT * MEL, 256)), dim3(256), 0, s, c.x, c.w, f1, f2, gp, BT, c.T, ws + L.c,
                       ws + L.d, c.batch ? nullptr : c.gx);
    const BnSums g1 = bn_sums(s, c, c.bn1, ws + L.c, ws + L.d, BT, MEL, part, ws + L.sums1);
    if (c.batch && c.gx)
      hipLaunchKernelGGL(bn_centre_kernel, dim3(blocks_of(BT * MEL, 256)), dim3(256), 0, s, ws + L.c, c.x, f1, g1.b, g1.w, BT * MEL, MEL,
                         (float)BT, c.gx);
  }
}

dim3 conv_grid(long GM, int GN, int chunks) { return dim3(blocks_of(GN, GT), blocks_of(GM, GT), (unsigned)chunks); }

// One conv GEMM.  wimg: the workspace of the 16-bit weight image (16-mixed, operand format E: one image, or hi then lo), null =
// the fp32 kernel.  MODE 0 and 1 read the weight from the image, which a launch ahead of the GEMM packs ([co][k] for MODE 0,
// transposed for MODE 1); MODE 2 has no weight operand.
template <typename E, int MODE>
void launch_conv_as(hipStream_t s, ConvP p, float* wimg, dim3 grid) {
  if (wimg && MODE != 2) {
    hipLaunchKernelGGL(conv_pack_kernel<E>, dim3(blocks_of((long)p.Cout * 6 * p.Cin, 256)), dim3(256), 0, s, p.w, p.Cout, p.Cin, MODE,
                       (el16<E>*)wimg);
    p.wh = wimg;
  }
  const auto kernel = wimg ? conv_gemm_mixed_kernel<E, MODE> : conv_gemm_kernel<MODE>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, p);
}
// ... with the operand format of the call (read only where wimg is given).  The chain is written out, not pick_route over
// BT_FOR_OPERANDS: this order of first use is the order of the conv kernels in the code object.
template <int MODE>
void launch_conv(hipStream_t s, const Call& c, const ConvP& p, float* wimg, dim3 grid) {
  if (wimg && c.operand == BT_OPERAND_BF16X3) launch_conv_as<bf16x3, MODE>(s, p, wimg, grid);
  else if (wimg && c.operand == BT_OPERAND_BF16) launch_conv_as<__bf16, MODE>(s, p, wimg, grid);
  else launch_conv_as<_Float16, MODE>(s, p, wimg, grid);
}

void conv_forward(hipStream_t s, const Call& c, const Layout& L) {
  float* ws = (float*)c.ws;
  const int Cout = 2 * c.C, Fo = c.F / 2;
  const long M = (long)c.B * c.T * Fo;
  const float* f2 = ws + L.fold;
  // batch statistics: the GEMM writes pre alone (no GELU output), the table comes from pre's moments, then the GELU
  if (!c.batch) fold_table(s, c, c.bn, Cout, nullptr, 0, L, ws + L.fold);
  launch_conv<0>(s, c, ConvP{c.x, c.w, nullptr, f2, c.save_pre, c.batch ? nullptr : c.y, c.T, Fo, c.C, Cout, M},
                 c.mixed ? ws + L.wimg : nullptr, conv_grid(M, Cout, 1));
  if (c.batch) {
    fold_table(s, c, c.bn, Cout, c.save_pre, M, L, ws + L.fold);
    hipLaunchKernelGGL(bn_gelu_kernel, dim3(blocks_of(M * Cout, 256)), dim3(256), 0, s, (const float*)c.save_pre, f2, M * Cout, Cout, c.y);
  }
}

void conv_backward(hipStream_t s, const Call& c, const Layout& L) {
  float* ws = (float*)c.ws;
  const int Cout = 2 * c.C, Fo = c.F / 2;
  const long M = (long)c.B * c.T * Fo;
  const float *f2 = ws + L.fold, *pre = c.save_pre;
  float *part = ws + L.part, *wimg = c.mixed ? ws + L.wimg : nullptr;
  fold_table(s, c, c.bn, Cout, nullptr, 0, L, ws + L.fold);
  hipLaunchKernelGGL(conv_gpre_kernel, dim3(blocks_of(M * Cout, 256)), dim3(256), 0, s, pre, c.gy, f2, M * Cout, Cout, ws + L.a, ws + L.b);
  const BnSums g = bn_sums(s, c, c.bn, ws + L.a, ws + L.b, M, Cout, part, ws + L.sums);
  if (c.batch)
    hipLaunchKernelGGL(bn_centre_kernel, dim3(blocks_of(M * Cout, 256)), dim3(256), 0, s, ws + L.a, pre, f2, g.b, g.w, M * Cout, Cout,
                       (float)M, (float*)nullptr);
  // backward-data and backward-weight on p.g = g_pre (they multiply by s = p.fold while staging)
  ConvP p{c.x, c.w, ws + L.a, f2, nullptr, nullptr, c.T, Fo, c.C, Cout, M};
  if (c.gx) {
    p.out = c.gx;
    launch_conv<1>(s, c, p, wimg, conv_grid(M, 2 * c.C, 1));
  }
  if (c.g_w) {
    const int chunks = dw_chunks(M);
    p.out = part;
    launch_conv<2>(s, c, p, wimg, conv_grid(Cout, 6 * c.C, chunks));
    hipLaunchKernelGGL(conv_dw_reduce_kernel, dim3(blocks_of((long)Cout * 6 * c.C, 256)), dim3(256), 0, s, (const float*)part, Cout, c.C,
                       chunks, c.g_w);
  }
}

// the projection's `mixed` of bt_train_matmul: 0, or 1 + the operand format
int matmul_route(const Call& c) { return route_of(c.mixed, c.operand); }

int linear_forward(void* stream, const Call& c, const Layout& L) {
  float* ws = (float*)c.ws;
  const long BT = (long)c.B * c.T;
  swap((hipStream_t)stream, c.x, BT, c.F, c.C, 1, ws + L.a);   // (f c) -> (c f)
  return bt_train_matmul(stream, matmul_route(c), 0, ws + L.a, c.w, (int)BT, c.dim, c.F * c.C, c.y, c.b, nullptr, 0, nullptr, nullptr, 0, 0,
                         nullptr, 0);
}

int linear_backward(void* stream, const Call& c, const Layout& L) {
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)c.ws;
  const long BT = (long)c.B * c.T;
  const int K = c.F * c.C;
  if (c.g_b) colsum(s, c.gy, BT, c.dim, ws + L.part, c.g_b);
  if (c.g_w) {
    swap(s, c.x, BT, c.F, c.C, 1, ws + L.a);
    if (int rc = bt_train_matmul(stream, matmul_route(c), 2, c.gy, ws + L.a, c.dim, K, (int)BT, c.g_w, nullptr, nullptr, 0, nullptr, nullptr, 0, 0,
                                 ws + L.part, (L.total - L.part) * sizeof(float)))
      return rc;
  }
  if (c.gx) {
    if (int rc = bt_train_matmul(stream, matmul_route(c), 1, c.gy, c.w, (int)BT, K, c.dim, ws + L.b, nullptr, nullptr, 0, nullptr, nullptr, 0, 0,
                                 nullptr, 0))
      return rc;
    swap(s, ws + L.b, BT, c.C, c.F, 1, c.gx);   // (c f) -> (f c)
  }
  return BT_OK;
}

int run(const char* fn, void* stream, int unit, const Call& c) {
  Layout L;
  if (int rc = prepare(fn, unit, c, L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  switch (unit) {
    case BT_FRONT_STEM:
      c.backward ? stem_backward(s, c, L) : stem_forward(s, c, L);
      break;
    case BT_FRONT_CONV:
      c.backward ? conv_backward(s, c, L) : conv_forward(s, c, L);
      break;
    case BT_FRONT_LINEAR:
      if (int rc = c.backward ? linear_backward(stream, c, L) : linear_forward(stream, c, L)) return rc;
      break;
    default:   // y = swap(x) over (T, F): gx = the swap over (F, T) of gy
      c.backward ? swap(s, c.gy, c.B, c.F, c.T, c.C, c.gx) : swap(s, c.x, c.B, c.T, c.F, c.C, c.y);
      break;
  }
  return finish(fn);
}

size_t workspace_bytes(int unit, int backward, bool batch, int images, int B, int T, int F, int C, int dim) {
  if (batch ? bn_check_shape(unit, B, T, F, C) : check_shape(unit, B, T, F, C, dim)) return 0;
  if (images && check_mixed(unit, 1, BT_OPERAND_F16, !batch)) return 0;
  return layout(unit, backward != 0, batch, images, (long)B * T, F, C, dim).total * sizeof(float);
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

size_t bt_front_workspace_bytes(int unit, int backward, int B, int T, int F, int C, int dim) {
  return workspace_bytes(unit, backward, false, 0, B, T, F, C, dim);
}
size_t bt_front_workspace_bytes_mixed(int unit, int backward, int B, int T, int F, int C, int dim) {
  return workspace_bytes(unit, backward, false, 1, B, T, F, C, dim);
}
size_t bt_front_workspace_bytes_x3(int unit, int backward, int B, int T, int F, int C, int dim) {
  return workspace_bytes(unit, backward, false, 2, B, T, F, C, dim);
}
size_t bt_front_bn_workspace_bytes(int unit, int backward, int B, int T, int F, int C) {
  return workspace_bytes(unit, backward, true, 0, B, T, F, C, 0);
}
size_t bt_front_bn_workspace_bytes_mixed(int unit, int backward, int B, int T, int F, int C) {
  return workspace_bytes(unit, backward, true, 1, B, T, F, C, 0);
}
size_t bt_front_bn_workspace_bytes_x3(int unit, int backward, int B, int T, int F, int C) {
  return workspace_bytes(unit, backward, true, 2, B, T, F, C, 0);
}

// running statistics and batch statistics (section 18): adapter, shared preamble, dispatch
int bt_front_forward(void* stream, int unit, const bt_front_args* a) {
  const char* fn = "bt_front_forward";
  return a ? run(fn, stream, unit, describe(*a, false)) : fail(fn, "null argument");
}
int bt_front_backward(void* stream, int unit, const bt_front_args* a) {
  const char* fn = "bt_front_backward";
  return a ? run(fn, stream, unit, describe(*a, true)) : fail(fn, "null argument");
}
int bt_front_bn_forward(void* stream, int unit, const bt_front_bn_args* a) {
  const char* fn = "bt_front_bn_forward";
  return a ? run(fn, stream, unit, describe(*a, false)) : fail(fn, "null argument");
}
int bt_front_bn_backward(void* stream, int unit, const bt_front_bn_args* a) {
  const char* fn = "bt_front_bn_backward";
  return a ? run(fn, stream, unit, describe(*a, true)) : fail(fn, "null argument");
}

}  // extern "C"
