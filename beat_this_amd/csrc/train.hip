// Training forward and backward of the transformer trunk's units and of the task heads:
//   attention unit   y = [x +] to_out(sigmoid(to_gates(n)) * softmax(rope(q) rope(k)^T / sqrt(32)) v),  n = RMSNorm(x)
//   feed-forward     y = [x +] W2 gelu(W1 RMSNorm(x) + b1) + b2                     (roformer.py:38-61, 99-132)
//   final norm       y = RMSNorm(x)
//   head             beat, downbeat of SumHead / Head                                  (beat_tracker.py:304-346)
// Everything is fp32 with fp32 accumulation and reads the parameters in the reference's layout, straight from the
// nn.Parameter storage (no packed copies).  The matrix products of the linear layers run on v_mfma_f32_32x32x2_f32 (exact
// fp32); the attention products (head dim 32) run on the fp32 vector unit, one query (forward, dQ) or one key (dK / dV) per
// thread, with the other side staged in LDS 64 rows at a time.
//
// Reproducibility: no atomics, no spinning.  Every output element is written by one thread of one launch, and the order of
// its sum depends on (B, T, D) only:
//   * a GEMM element sums its k range in ascending order (MFMA steps of 2);
//   * a weight gradient dW = dY^T A is split over the B T rows into chunks of DW_ROWS rows, each chunk writes a partial
//     [N, K] matrix into the workspace, and a second launch adds the partials in chunk order;
//   * column sums (bias and gamma gradients) do the same with chunks of CS_ROWS rows;
//   * dQ of a query adds its keys in ascending order, dK / dV of a key add the queries in ascending order (two sweeps:
//     seven products per tile pair instead of five, the price of needing no atomics).
// A row's results do not depend on the other rows of the batch, so grad_x of a sequence is the same alone and in a batch.
//
// Saved by the training forward: the attention's pre-gate output O [B T, D] and the per-(row, head) base-2 log-sum-exp;
// everything else (RMSNorm, projections, RoPE, gates, GELU) is recomputed in the backward from the unit's input x.
//
// Dropout: the kernels that meet one of the four sites have a second instantiation (template
// parameter DROP) that evaluates the masks of dropout.h for the elements it touches; the masks are stored nowhere, and the
// instantiations without dropout are the code and the launches they were before.  The order of every sum is the same.
//
// 16-mixed: the *_mixed entry points run the same unit code with `mixed` set, which sends the GEMMs and
// the three attention sweeps to the fp16 MFMA kernels of train_mixed.inc (bt_train_args.operand = BT_OPERAND_BF16, section 24: their bfloat16 instantiations;
// BT_OPERAND_BF16X3, section 25: the ones on split bfloat16 operands, three MFMAs per product); every other launch, and every
// launch of the entry points that existed before, is unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/beat_this_amd.h"
#include "train_common.h"    // GemmP, gemm_epilogue, the vector types and constants shared with the 16-mixed kernels
#include "train_mixed.inc"   // the 16-mixed route's kernels: fp16 MFMA GEMM and attention sweeps

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

constexpr int DW_ROWS = BT_TRAIN_DW_ROWS;   // rows per partial of a weight gradient
constexpr int CS_ROWS = BT_TRAIN_CS_ROWS;   // rows per partial of a column sum
constexpr int AB = BT_TRAIN_ATTN_BLOCK;     // queries per workgroup = keys per LDS tile (and the reverse in the dK / dV sweep)
constexpr int GT = 64;                      // GEMM tile: GT x GT outputs, GK deep
constexpr int GK = 16;
static_assert(AB == 64, "the attention kernels stage with one 64-lane wave");
constexpr float RMS_EPS = 1e-12f;

// ---- GEMM (GemmP and the epilogue: train_common.h), one 32 x 32 MFMA tile per wave -----------------------------------------
template <bool AT, bool BT, bool DROP>
__device__ inline void gemm_body(const GemmP& p, const DropSite& ds, int drop_act) {
  __shared__ float As[GK][GT + 4];
  __shared__ float Bs[GK][GT + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, lr = lane & 31, wm = wave >> 1, wn = wave & 1;
  const long m0 = (long)blockIdx.y * GT, n0 = (long)blockIdx.x * GT;
  const long kb = (long)blockIdx.z * p.kchunk, ke = std::min<long>(p.K, kb + p.kchunk);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (long k0 = kb; k0 < ke; k0 += GK) {
#pragma unroll
    for (int i = 0; i < GT * GK / 256; ++i) {
      const int e = tid + i * 256;
      {
        const int kk = AT ? e / GT : e % GK, mm = AT ? e % GT : e / GK;
        const long gm = m0 + mm, gk = k0 + kk;
        float v = 0.0f;
        if (gm < p.M && gk < ke) v = AT ? p.A[gk * p.lda + gm] : p.A[gm * p.lda + gk];
        As[kk][mm] = v;
      }
      {
        const int kk = BT ? e / GT : e % GK, nn = BT ? e % GT : e / GK;
        const long gn = n0 + nn, gk = k0 + kk;
        float v = 0.0f;
        if (gn < p.N && gk < ke) v = BT ? p.B[gk * p.ldb + gn] : p.B[gn * p.ldb + gk];
        Bs[kk][nn] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + g][wm * 32 + lr], Bs[kk + g][wn * 32 + lr], acc, 0, 0, 0);
    __syncthreads();
  }
  float* C = p.C ? p.C + (long)blockIdx.z * p.cz : nullptr;
  gemm_epilogue<DROP>(p, ds, drop_act, C, acc, m0 + wm * 32, n0 + wn * 32 + lr, lane);
}

template <bool AT, bool BT>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmP p) {
  gemm_body<AT, BT, false>(p, DropSite{}, 0);
}

__global__ __launch_bounds__(256) void gemm_drop_kernel(const GemmP p, const DropSite ds, const int drop_act) {
  gemm_body<false, false, true>(p, ds, drop_act);
}

unsigned blocks_of(long n, int per) { return (unsigned)((n + per - 1) / per); }

// What every launch helper below needs to know of the call it serves: the stream, the route (mixed: train_common.h's route_of:
// 0 = the fp32 kernels of this file, else the MFMA kernels of train_mixed.inc on the operand format mixed - 1), and the dropout
// of the call (null: none, otherwise p > 0).
constexpr int MIXED_F16 = route_of(1, BT_OPERAND_F16);
const char* const BAD_ROUTE = "mixed must be 0 (fp32), 1 (fp16 operands), 2 (bfloat16 operands) or 4 (split bfloat16 operands)";
struct Launch {
  hipStream_t s;
  int mixed;
  const bt_train_dropout* dp;
  bool drop() const { return dp != nullptr; }
  DropSite site(int id) const { return drop_site(dp->p, dp->seed, dp->stream, id); }
  // the kernel of the call's route among the four forms of one launch
  template <typename K> K pick(K f32, K f16, K bf16, K x3) const { return pick_route(mixed, f32, f16, bf16, x3); }
};
constexpr int NO_SITE = -1;   // linear_fwd: a result that no dropout site covers

dim3 gemm_grid(const Launch& lc, const GemmP& p, int chunks) {
  const int t = lc.mixed ? MT : GT;
  return dim3(blocks_of(p.N, t), blocks_of(p.M, t), (unsigned)chunks);
}

template <bool AT, bool BT> void launch_gemm(const Launch& lc, const GemmP& p, int chunks) {
  const auto kernel = lc.pick(gemm_kernel<AT, BT>, BT_FOR_OPERANDS(mx_gemm_kernel, AT, BT));
  hipLaunchKernelGGL(kernel, gemm_grid(lc, p, chunks), dim3(256), 0, lc.s, p);
}

// Y[M, N] (+)= A[M, K] W[N, K]^T (+ bias, + resid; act = gelu(Y)); site: with dropout, the BT_DROP_* row site over Y
// (drop_act == 0) or over act, or NO_SITE
void linear_fwd(const Launch& lc, const float* A, const float* W, const float* bias, long M, int N, int K, float* Y, const float* resid,
                float* act, int site = NO_SITE, int drop_act = 0, bool accum = false) {
  GemmP p{};
  p.A = A; p.lda = K; p.B = W; p.ldb = K; p.M = (int)M; p.N = N; p.K = K; p.kchunk = K;
  p.C = Y; p.ldc = N; p.bias = bias; p.resid = resid; p.ldr = N; p.accum = accum; p.act = act; p.ldact = N;
  if (!lc.drop() || site == NO_SITE) return launch_gemm<false, false>(lc, p, 1);
  const auto kernel = lc.pick(gemm_drop_kernel, BT_FOR_OPERANDS(mx_gemm_drop_kernel));
  hipLaunchKernelGGL(kernel, gemm_grid(lc, p, 1), dim3(256), 0, lc.s, p, lc.site(site), drop_act);
}

// dA[M, K] (+)= dY[M, N] W[N, K]
void linear_bwd_input(const Launch& lc, const float* dY, const float* W, long M, int N, int K, float* dA, bool accum = false) {
  GemmP p{};
  p.A = dY; p.lda = N; p.B = W; p.ldb = K; p.M = (int)M; p.N = K; p.K = N; p.kchunk = N;
  p.C = dA; p.ldc = K; p.accum = accum;
  launch_gemm<false, true>(lc, p, 1);
}

__global__ __launch_bounds__(256) void reduce_parts_kernel(const float* part, long n, int chunks, float* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = part[i];
  for (int c = 1; c < chunks; ++c) acc += part[(long)c * n + i];
  out[i] = acc;
}

int dw_chunks(long M) { return (int)((M + DW_ROWS - 1) / DW_ROWS); }
int cs_chunks(long M) { return (int)((M + CS_ROWS - 1) / CS_ROWS); }

// dW[N, K] = dY[M, N]^T A[M, K]: partials over DW_ROWS-row chunks in `part`, then added in chunk order
void linear_bwd_weight(const Launch& lc, const float* dY, const float* A, long M, int N, int K, float* part, float* dW) {
  const int chunks = dw_chunks(M);
  GemmP p{};
  p.A = dY; p.lda = N; p.B = A; p.ldb = K; p.M = N; p.N = K; p.K = (int)M; p.kchunk = DW_ROWS;
  p.C = part; p.ldc = K; p.cz = (long)N * K;
  launch_gemm<true, true>(lc, p, chunks);
  const long n = (long)N * K;
  hipLaunchKernelGGL(reduce_parts_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, lc.s, (const float*)part, n, chunks, dW);
}

// out[j] = sum_m a[m][j] (* b[m][j]) (* r[m rs]), j < N: partials over CS_ROWS-row chunks, then added in chunk order
__global__ __launch_bounds__(256) void colsum_kernel(const float* a, long lda, const float* b, long ldb, const float* r, long rs,
                                                     long M, int N, float* part) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  const long mb = (long)blockIdx.y * CS_ROWS, me = std::min<long>(M, mb + CS_ROWS);
  float acc = 0.0f;
  for (long m = mb; m < me; ++m) {
    float v = a[m * lda + j];
    if (b) v *= b[m * ldb + j];
    if (r) v *= r[m * rs];
    acc += v;
  }
  part[(long)blockIdx.y * N + j] = acc;
}

void colsum(const Launch& lc, const float* a, long lda, const float* b, long ldb, const float* r, long rs, long M, int N, float* part,
            float* out) {
  const int chunks = cs_chunks(M);
  hipLaunchKernelGGL(colsum_kernel, dim3(blocks_of(N, 256), (unsigned)chunks), dim3(256), 0, lc.s, a, lda, b, ldb, r, rs, M, N, part);
  hipLaunchKernelGGL(reduce_parts_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, lc.s, (const float*)part, (long)N, chunks, out);
}

// ---- RMSNorm (roformer.py:22-32): y = x / max(|x|, 1e-12) sqrt(D) gamma; one wave per row ---------------------------------
__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void rms_fwd_kernel(const float* x, const float* gamma, long M, int D, float* y, float* rinv) {
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const float* xr = x + m * D;
  float ss = 0.0f;
  for (int j = lane; j < D; j += 64) ss = fmaf(xr[j], xr[j], ss);
  ss = wave_sum(ss);
  const float r = sqrtf((float)D) / fmaxf(sqrtf(ss), RMS_EPS);
  for (int j = lane; j < D; j += 64) y[m * D + j] = xr[j] * r * gamma[j];
  if (rinv && lane == 0) rinv[m] = r;
}

// gx = [resid +] d RMSNorm / dx applied to dy; rinv[m] = the row's factor (what the gamma gradient's column sum reads)
__global__ __launch_bounds__(256) void rms_bwd_kernel(const float* x, const float* gamma, const float* dy, const float* resid, long M,
                                                      int D, float* gx, float* rinv) {
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const float* xr = x + m * D;
  const float* dr = dy + m * D;
  float ss = 0.0f, dot = 0.0f;
  for (int j = lane; j < D; j += 64) {
    ss = fmaf(xr[j], xr[j], ss);
    dot = fmaf(dr[j] * gamma[j], xr[j], dot);
  }
  ss = wave_sum(ss);
  dot = wave_sum(dot);
  const float nrm = sqrtf(ss);
  const bool clamped = !(nrm > RMS_EPS);
  const float r = sqrtf((float)D) / (clamped ? RMS_EPS : nrm);
  const float coef = clamped ? 0.0f : dot * r / ss;   // (the norm's own derivative; none where the clamp holds)
  if (gx)
    for (int j = lane; j < D; j += 64) {
      float v = dr[j] * gamma[j] * r - xr[j] * coef;
      if (resid) v += resid[m * D + j];
      gx[m * D + j] = v;
    }
  if (lane == 0) rinv[m] = r;
}

// ---- RoPE on the q and k sections of qkv [M, 3 D] (interleaved pairs, table [rope_len][16][2] = cos, sin) -------------------
__global__ __launch_bounds__(256) void rope_kernel(float* qkv, const float* rope, long M, int T, int D, int inverse) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // (row, section, pair)
  const long per_row = D;                                 // 2 sections of D / 2 pairs
  if (i >= M * per_row) return;
  const long m = i / per_row;
  const int c = (int)(i % per_row), sec = c / (D / 2), pr = c % (D / 2);
  const int pos = (int)(m % T);
  const float cs = rope[(pos * 16 + (pr & 15)) * 2], sn = rope[(pos * 16 + (pr & 15)) * 2 + 1];
  float* p = qkv + m * 3 * D + (long)sec * D + 2 * pr;
  const float e = p[0], o = p[1];
  if (!inverse) {
    p[0] = e * cs - o * sn;
    p[1] = o * cs + e * sn;
  } else {   // the transpose of the rotation
    p[0] = e * cs + o * sn;
    p[1] = o * cs - e * sn;
  }
}

// ---- attention, head dim 32 ------------------------------------------------------------------------------------------------
// rows of one (batch, head): element d of token t of section s at base[(b T + t) ld + s D + h 32 + d]
__device__ inline void load_row32(const float* p, bool ok, float* v) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4 t = ok ? reinterpret_cast<const f32x4*>(p)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    v[4 * i] = t[0]; v[4 * i + 1] = t[1]; v[4 * i + 2] = t[2]; v[4 * i + 3] = t[3];
  }
}
__device__ inline void store_row32(float* p, const float* v, float scale) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    reinterpret_cast<f32x4*>(p)[i] = f32x4{v[4 * i] * scale, v[4 * i + 1] * scale, v[4 * i + 2] * scale, v[4 * i + 3] * scale};
}
// stage rows [t0, t0 + AB) of a [T, 32] slice (row stride ld) into tile[AB][32]; rows >= T read as zeros
__device__ inline void stage_tile(const float* base, long ld, int t0, int T, float (*tile)[32], int lane) {
#pragma unroll
  for (int i = 0; i < AB * 8 / 64; ++i) {
    const int idx = i * 64 + lane, row = idx >> 3, part = idx & 7;
    const int t = t0 + row;
    const f32x4 v = t < T ? reinterpret_cast<const f32x4*>(base + (long)t * ld)[part] : f32x4{0.f, 0.f, 0.f, 0.f};
    reinterpret_cast<f32x4*>(&tile[row][0])[part] = v;
  }
}
__device__ inline float dot32(const float* a, const float* b) {
  float s = 0.0f;
#pragma unroll
  for (int d = 0; d < 32; ++d) s = fmaf(a[d], b[d], s);
  return s;
}

// O = softmax(q k^T / sqrt(32)) v (before the gate) and lse = base-2 log-sum-exp of the scaled scores.
// DROP: the normaliser and the maximum see every key, the accumulator only the kept (query, key) pairs; O is the dropped
// output, scaled by 1 / (1 - p).  A thread walks its query's keys four at a time: one call per group.
template <bool DROP>
__device__ inline void attn_fwd_body(const float* qkv, int T, int D, float* O, float* lse, const DropSite& ds) {
  __shared__ __attribute__((aligned(16))) float Ks[AB][32];
  __shared__ __attribute__((aligned(16))) float Vs[AB][32];
  const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z, H = D / 32;
  const int t = blockIdx.x * AB + lane;
  const bool ok = t < T;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + h * 32;
  float q[32], acc[32];
  load_row32(base + (long)t * ld, ok, q);
#pragma unroll
  for (int d = 0; d < 32; ++d) acc[d] = 0.0f;
  float mx = -INFINITY, l = 0.0f;
  for (int k0 = 0; k0 < T; k0 += AB) {
    __syncthreads();
    stage_tile(base + D, ld, k0, T, Ks, lane);
    stage_tile(base + 2 * D, ld, k0, T, Vs, lane);
    __syncthreads();
    const int nk = min(AB, T - k0);
    auto step = [&](int j, bool kept) {   // key j of the tile
      const float s = dot32(q, Ks[j]) * QK_SCALE_LOG2E;
      if (s > mx) {
        const float corr = exp2f(mx - s);
        l *= corr;
#pragma unroll
        for (int d = 0; d < 32; ++d) acc[d] *= corr;
        mx = s;
      }
      const float p = exp2f(s - mx);
      l += p;
      const float pk = kept ? p : 0.0f;
#pragma unroll
      for (int d = 0; d < 32; ++d) acc[d] = fmaf(pk, Vs[j][d], acc[d]);
    };
    if constexpr (!DROP) {
      for (int j = 0; j < nk; ++j) step(j, true);
    } else {
      for (int j0 = 0; j0 < nk; j0 += 4) {
        const PhiloxWords w = drop_words(ds, drop_attn_group((uint64_t)b * H + h, (uint32_t)T, (uint32_t)t, (uint32_t)(k0 + j0)));
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          if (j0 + jj < nk) step(j0 + jj, w.w[jj] >= ds.thr);
      }
    }
  }
  if (!ok) return;
  const long m = (long)b * T + t;
  store_row32(O + m * D + h * 32, acc, DROP ? ds.scale / l : 1.0f / l);
  lse[m * H + h] = mx + log2f(l);
}

__global__ __launch_bounds__(AB) void attn_fwd_kernel(const float* qkv, int T, int D, float* O, float* lse) {
  attn_fwd_body<false>(qkv, T, D, O, lse, DropSite{});
}
__global__ __launch_bounds__(AB) void attn_fwd_drop_kernel(const float* qkv, int T, int D, float* O, float* lse, const DropSite ds) {
  attn_fwd_body<true>(qkv, T, D, O, lse, ds);
}

// dq of a query: keys in ascending order.  DROP: dP = m c (dO . v), dS = P (dP - delta)
template <bool DROP>
__device__ inline void attn_dq_body(const float* qkv, const float* dO, const float* lse, const float* delta, int T, int D, float* dqkv,
                                    const DropSite& ds) {
  __shared__ __attribute__((aligned(16))) float Ks[AB][32];
  __shared__ __attribute__((aligned(16))) float Vs[AB][32];
  const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z, H = D / 32;
  const int t = blockIdx.x * AB + lane;
  const bool ok = t < T;
  const long ld = 3L * D, m = (long)b * T + (ok ? t : 0);
  const float* base = qkv + (long)b * T * ld + h * 32;
  float q[32], go[32], acc[32];
  load_row32(base + (long)t * ld, ok, q);
  load_row32(dO + m * D + h * 32, ok, go);
#pragma unroll
  for (int d = 0; d < 32; ++d) acc[d] = 0.0f;
  const float ls = ok ? lse[m * H + h] : 0.0f, dl = ok ? delta[m * H + h] : 0.0f;
  for (int k0 = 0; k0 < T; k0 += AB) {
    __syncthreads();
    stage_tile(base + D, ld, k0, T, Ks, lane);
    stage_tile(base + 2 * D, ld, k0, T, Vs, lane);
    __syncthreads();
    const int nk = min(AB, T - k0);
    auto step = [&](int j, bool kept) {   // key j of the tile
      const float p = exp2f(dot32(q, Ks[j]) * QK_SCALE_LOG2E - ls);
      float dp = dot32(go, Vs[j]);
      if constexpr (DROP) dp = kept ? dp * ds.scale : 0.0f;
      const float ds_ = p * (dp - dl);
#pragma unroll
      for (int d = 0; d < 32; ++d) acc[d] = fmaf(ds_, Ks[j][d], acc[d]);
    };
    if constexpr (!DROP) {
      for (int j = 0; j < nk; ++j) step(j, true);
    } else {
      for (int j0 = 0; j0 < nk; j0 += 4) {
        const PhiloxWords w = drop_words(ds, drop_attn_group((uint64_t)b * H + h, (uint32_t)T, (uint32_t)t, (uint32_t)(k0 + j0)));
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          if (j0 + jj < nk) step(j0 + jj, w.w[jj] >= ds.thr);
      }
    }
  }
  if (ok) store_row32(dqkv + ((long)b * T + t) * ld + h * 32, acc, QK_SCALE);
}

__global__ __launch_bounds__(AB) void attn_dq_kernel(const float* qkv, const float* dO, const float* lse, const float* delta, int T,
                                                     int D, float* dqkv) {
  attn_dq_body<false>(qkv, dO, lse, delta, T, D, dqkv, DropSite{});
}
__global__ __launch_bounds__(AB) void attn_dq_drop_kernel(const float* qkv, const float* dO, const float* lse, const float* delta,
                                                          int T, int D, float* dqkv, const DropSite ds) {
  attn_dq_body<true>(qkv, dO, lse, delta, T, D, dqkv, ds);
}

// dk and dv of a key: queries in ascending order.  DROP: dV += (m c P)^T dO, and dS as in the dq sweep.  The four keys of a
// quad of lanes are one group of every query: the lanes evaluate four queries' groups, one each, and exchange the words.
template <bool DROP>
__device__ inline void attn_dkv_body(const float* qkv, const float* dO, const float* lse, const float* delta, int T, int D,
                                     float* dqkv, const DropSite& ds) {
  __shared__ __attribute__((aligned(16))) float Qs[AB][32];
  __shared__ __attribute__((aligned(16))) float Gs[AB][32];
  __shared__ float Ls[AB], Ds[AB];
  const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z, H = D / 32;
  const int t = blockIdx.x * AB + lane;
  const bool ok = t < T;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + h * 32;
  const float* gbase = dO + (long)b * T * D + h * 32;
  float k[32], v[32], dk[32], dv[32];
  load_row32(base + D + (long)t * ld, ok, k);
  load_row32(base + 2 * D + (long)t * ld, ok, v);
#pragma unroll
  for (int d = 0; d < 32; ++d) dk[d] = dv[d] = 0.0f;
  for (int q0 = 0; q0 < T; q0 += AB) {
    __syncthreads();
    stage_tile(base, ld, q0, T, Qs, lane);
    stage_tile(gbase, D, q0, T, Gs, lane);
    {
      const int tq = q0 + lane;
      const long mq = (long)b * T + tq;
      Ls[lane] = tq < T ? lse[mq * H + h] : 0.0f;
      Ds[lane] = tq < T ? delta[mq * H + h] : 0.0f;
    }
    __syncthreads();
    const int nq = min(AB, T - q0);
    auto step = [&](int i, bool kept) {   // query i of the tile
      const float p = exp2f(dot32(Qs[i], k) * QK_SCALE_LOG2E - Ls[i]);
      float pm = p, dp = dot32(Gs[i], v);
      if constexpr (DROP) {
        pm = kept ? p * ds.scale : 0.0f;
        dp = kept ? dp * ds.scale : 0.0f;
      }
      const float ds_ = p * (dp - Ds[i]);
#pragma unroll
      for (int d = 0; d < 32; ++d) {
        dv[d] = fmaf(pm, Gs[i][d], dv[d]);
        dk[d] = fmaf(ds_, Qs[i][d], dk[d]);
      }
    };
    if constexpr (!DROP) {
      for (int i = 0; i < nq; ++i) step(i, true);
    } else {
      for (int i0 = 0; i0 < nq; i0 += 4) {   // (every lane of the wave takes part, also the ones behind key T - 1)
        const PhiloxWords w =
            drop_words(ds, drop_attn_group((uint64_t)b * H + h, (uint32_t)T, (uint32_t)(q0 + i0 + (lane & 3)), (uint32_t)t));
        uint32_t mine[4] = {w.w[0], w.w[1], w.w[2], w.w[3]};
        quad_transpose(mine, lane);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          if (i0 + jj < nq) step(i0 + jj, mine[jj] >= ds.thr);
      }
    }
  }
  if (!ok) return;
  float* out = dqkv + ((long)b * T + t) * ld + h * 32;
  store_row32(out + D, dk, QK_SCALE);
  store_row32(out + 2 * D, dv, 1.0f);
}

__global__ __launch_bounds__(AB) void attn_dkv_kernel(const float* qkv, const float* dO, const float* lse, const float* delta, int T,
                                                      int D, float* dqkv) {
  attn_dkv_body<false>(qkv, dO, lse, delta, T, D, dqkv, DropSite{});
}
__global__ __launch_bounds__(AB) void attn_dkv_drop_kernel(const float* qkv, const float* dO, const float* lse, const float* delta,
                                                           int T, int D, float* dqkv, const DropSite ds) {
  attn_dkv_body<true>(qkv, dO, lse, delta, T, D, dqkv, ds);
}

__device__ inline float sigmoid_f(float v) { return 1.0f / (1.0f + expf(-v)); }

// og[m][h 32 + d] = O * sigmoid(gate logit[m][h])
__global__ __launch_bounds__(256) void gate_fwd_kernel(const float* O, const float* gl, long M, int D, float* og) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * D) return;
  const long m = i / D;
  const int h = (int)(i % D) >> 5;
  og[i] = O[i] * sigmoid_f(gl[m * (D / 32) + h]);
}

// per (row, head), 32 lanes: dog -> dO = dog sigmoid (in place), delta = sum_d dO O, dgl = sum_d dog O sigmoid'
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* O, const float* gl, float* dog, long M, int D, float* delta,
                                                       float* dgl) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // (a 32-lane group never straddles the end: M D is a multiple of 32)
  if (i >= M * D) return;
  const long m = i / D;
  const int H = D / 32, h = (int)(i % D) >> 5;
  const float sg = sigmoid_f(gl[m * H + h]);
  const float go = dog[i];
  float dotp = go * O[i];
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) dotp += __shfl_xor(dotp, o, 64);
  dog[i] = go * sg;
  if ((threadIdx.x & 31) == 0) {
    delta[m * H + h] = dotp * sg;
    dgl[m * H + h] = dotp * sg * (1.0f - sg);
  }
}

// dh = da * gelu'(h), in place over h
__global__ __launch_bounds__(256) void gelu_bwd_kernel(float* h, const float* da, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) h[i] = da[i] * gelu_grad_f(h[i]);
}

// the same behind a dropped GELU: dh = da m c gelu'(h); a thread takes one group of four (n4 = n / 4 groups of a row site)
__global__ __launch_bounds__(256) void gelu_bwd_drop_kernel(float* h, const float* da, long n4, const DropSite ds) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const PhiloxWords w = drop_words(ds, (uint64_t)i);
  const f32x4 a = reinterpret_cast<const f32x4*>(da)[i], x = reinterpret_cast<const f32x4*>(h)[i];
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = a[j] * (w.w[j] >= ds.thr ? ds.scale : 0.0f) * gelu_grad_f(x[j]);
  reinterpret_cast<f32x4*>(h)[i] = r;
}

// out = in m c over a row site (n4 = elements / 4): the masked upstream gradient behind to_out / the second FF linear
__global__ __launch_bounds__(256) void mask_kernel(const float* in, long n4, const DropSite ds, float* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const PhiloxWords w = drop_words(ds, (uint64_t)i);
  const f32x4 a = reinterpret_cast<const f32x4*>(in)[i];
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = a[j] * (w.w[j] >= ds.thr ? ds.scale : 0.0f);
  reinterpret_cast<f32x4*>(out)[i] = r;
}

// ---- head ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* x, const float* w, const float* bias, long M, int D, int sum_head,
                                                       float* beat, float* down) {
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  float a0 = 0.0f, a1 = 0.0f;
  for (int j = lane; j < D; j += 64) {
    const float v = x[m * D + j];
    a0 = fmaf(v, w[j], a0);
    a1 = fmaf(v, w[D + j], a1);
  }
  a0 = wave_sum(a0) + bias[0];
  a1 = wave_sum(a1) + bias[1];
  if (lane == 0) {
    beat[m] = sum_head ? a0 + a1 : a0;
    down[m] = a1;
  }
}

// gradients of the two linear outputs (gbd [M][2]) and of x
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* g_beat, const float* g_down, const float* w, long M, int D,
                                                       int sum_head, float* gbd, float* gx) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * D) return;
  const long m = i / D;
  const int j = (int)(i % D);
  const float gb = g_beat ? g_beat[m] : 0.0f, gd = g_down ? g_down[m] : 0.0f;
  const float g0 = gb, g1 = sum_head ? gb + gd : gd;
  if (j == 0) {
    gbd[2 * m] = g0;
    gbd[2 * m + 1] = g1;
  }
  if (gx) gx[i] = g0 * w[j] + g1 * w[D + j];
}

// ---- workspace layouts (floats; every region a multiple of 64 floats = 256 bytes) ---------------------------------------------
size_t up64(size_t n) { return (n + 63) / 64 * 64; }

struct Layout {
  size_t xn, rinv, a, b, c, d, e, small0, small1, small2, part, gm, total;   // offsets in floats
};

// drop: the backward of the attention and the feed-forward with dropout keeps the masked upstream gradient in one more
// region, behind the others (whose offsets are the same with and without)
Layout layout(int unit, int backward, long M, int D, int HID, bool drop = false) {
  Layout L{};
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += up64(n); return o; };
  const size_t MD = (size_t)M * D, MH = (size_t)M * HID, H = D / 32;
  const size_t dwc = dw_chunks(M), csc = cs_chunks(M);
  switch (unit) {
    case BT_UNIT_FF:
      L.xn = take(MD);
      L.rinv = take(M);
      L.a = take(MH);                    // forward: gelu(h); backward: h, then dh
      if (backward) {
        L.b = take(MH);                  // gelu(h), then da
        L.part = take(std::max(dwc * (size_t)HID * D, csc * (size_t)std::max(HID, D)));
      }
      break;
    case BT_UNIT_ATTN:
      L.xn = take(MD);
      L.rinv = take(M);
      L.a = take(3 * MD);                // qkv
      L.small0 = take(M * H);            // gate logits
      L.b = take(MD);                    // gated attention output; backward: then d xn
      if (backward) {
        L.c = take(MD);                  // d og, then dO
        L.d = take(3 * MD);              // d qkv
        L.small1 = take(M * H);          // delta
        L.small2 = take(M * H);          // d gate logits
        L.part = take(std::max(dwc * 3 * (size_t)D * D, csc * (size_t)D));
      }
      break;
    case BT_UNIT_NORM:
      if (backward) {
        L.rinv = take(M);
        L.part = take(csc * (size_t)D);
      }
      break;
    default:   // head
      if (backward) {
        L.small0 = take(2 * (size_t)M);
        L.part = take(csc * (size_t)D);
      }
      break;
  }
  if (drop && backward && (unit == BT_UNIT_FF || unit == BT_UNIT_ATTN)) L.gm = take(MD);
  L.total = std::max<size_t>(at, 64);
  return L;
}

const char* check_width(int D) {
  return D < 32 || D > 1024 || D % 32 ? "unsupported width (a multiple of 32 from 32 to 1024)" : nullptr;
}

const char* check_shape(int unit, int B, int T, int D, int HID, int rope_len) {
  if (unit != BT_UNIT_ATTN && unit != BT_UNIT_FF && unit != BT_UNIT_NORM && unit != BT_TRAIN_UNIT_HEAD)
    return "unit must be BT_UNIT_ATTN, BT_UNIT_FF, BT_UNIT_NORM or BT_TRAIN_UNIT_HEAD";
  if (const char* e = check_width(D)) return e;
  if (unit == BT_UNIT_FF && (HID < D || HID > 16 * D || HID % D)) return "unsupported hidden width (ff_mult 1 .. 16 times the width)";
  const int max_T = rope_len > 0 ? rope_len : 1536;
  if (B < 1 || T < 1 || T > max_T) return "need B >= 1 and 1 <= T <= rope_len (rows of the rotary table)";
  if ((long)B * T > (1L << 22)) return "more than 2^22 rows";
  return nullptr;
}

const char* check_mnk(int M, int N, int K) {
  return M < 1 || N < 1 || K < 1 || M > (1 << 22) || N > (1 << 22) || K > (1 << 22) ? "need 1 <= M, N, K <= 2^22" : nullptr;
}

// 0 <= p < 1 (NaN fails); *active: dropout is on (dp may be null: off)
const char* check_p(const bt_train_dropout* dp, bool* active) {
  *active = false;
  if (dp && !(dp->p >= 0.0f && dp->p < 1.0f)) return "dropout p must satisfy 0 <= p < 1";
  *active = dp && dp->p > 0.0f;
  return nullptr;
}

// the same for a unit call: p > 0 on the attention or the feed-forward only
const char* check_dropout(int unit, const bt_train_dropout* dp, bool* active) {
  if (const char* e = check_p(dp, active)) return e;
  if (*active && unit != BT_UNIT_ATTN && unit != BT_UNIT_FF) return "dropout applies to BT_UNIT_ATTN and BT_UNIT_FF only";
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

// the attention's forward sweep over qkv [B T, 3 D] (after RoPE) -> O, lse; with dropout, the BT_DROP_ATTN_P site
void attn_fwd_sweep(const Launch& lc, const float* qkv, int B, int T, int D, float* O, float* lse) {
  const dim3 grid(blocks_of(T, lc.mixed ? XB : AB), D / 32, B), block(lc.mixed ? 64 : AB);
  if (!lc.drop()) {
    const auto kernel = lc.pick(attn_fwd_kernel, BT_FOR_OPERANDS(mx_attn_fwd_kernel));
    hipLaunchKernelGGL(kernel, grid, block, 0, lc.s, qkv, T, D, O, lse);
  } else {
    const auto kernel = lc.pick(attn_fwd_drop_kernel, BT_FOR_OPERANDS(mx_attn_fwd_drop_kernel));
    hipLaunchKernelGGL(kernel, grid, block, 0, lc.s, qkv, T, D, O, lse, lc.site(BT_DROP_ATTN_P));
  }
}

// the attention's two backward sweeps (dK / dV, then dQ) -> dqkv [B T, 3 D], before the backward RoPE
// (delta = sum_d dO O holds with the dropped O: sum_k P dP = sum_k (m c P)(dO . v) = dO . O)
void attn_bwd_sweeps(const Launch& lc, const float* qkv, const float* dO, const float* lse, const float* delta, int B, int T, int D,
                     float* dqkv) {
  const dim3 grid(blocks_of(T, lc.mixed ? XB : AB), D / 32, B), block(lc.mixed ? 64 : AB);
  if (!lc.drop()) {
    const auto dkv = lc.pick(attn_dkv_kernel, BT_FOR_OPERANDS(mx_attn_dkv_kernel));
    const auto dq = lc.pick(attn_dq_kernel, BT_FOR_OPERANDS(mx_attn_dq_kernel));
    hipLaunchKernelGGL(dkv, grid, block, 0, lc.s, qkv, dO, lse, delta, T, D, dqkv);
    hipLaunchKernelGGL(dq, grid, block, 0, lc.s, qkv, dO, lse, delta, T, D, dqkv);
  } else {
    const DropSite pd = lc.site(BT_DROP_ATTN_P);
    const auto dkv = lc.pick(attn_dkv_drop_kernel, BT_FOR_OPERANDS(mx_attn_dkv_drop_kernel));
    const auto dq = lc.pick(attn_dq_drop_kernel, BT_FOR_OPERANDS(mx_attn_dq_drop_kernel));
    hipLaunchKernelGGL(dkv, grid, block, 0, lc.s, qkv, dO, lse, delta, T, D, dqkv, pd);
    hipLaunchKernelGGL(dq, grid, block, 0, lc.s, qkv, dO, lse, delta, T, D, dqkv, pd);
  }
}

// the recomputed part shared by the attention's forward and backward: xn, rinv, rotated qkv, gate logits
void attn_prologue(const Launch& lc, const bt_train_args& a, const Layout& L, float* ws, long M) {
  const int D = a.dim, H = D / 32;
  hipLaunchKernelGGL(rms_fwd_kernel, dim3(blocks_of(M, 4)), dim3(256), 0, lc.s, a.x, a.gamma, M, D, ws + L.xn, ws + L.rinv);
  linear_fwd(lc, ws + L.xn, a.w1, nullptr, M, 3 * D, D, ws + L.a, nullptr, nullptr);
  hipLaunchKernelGGL(rope_kernel, dim3(blocks_of(M * D, 256)), dim3(256), 0, lc.s, ws + L.a, a.rope, M, a.T, D, 0);
  linear_fwd(lc, ws + L.xn, a.w2, a.b2, M, H, D, ws + L.small0, nullptr, nullptr);
}

}  // namespace

extern "C" {

void bt_train_struct_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(bt_train_args);
  out[1] = (int32_t)offsetof(bt_train_args, rope);
  out[2] = (int32_t)offsetof(bt_train_args, x);
  out[3] = (int32_t)offsetof(bt_train_args, gy);
  out[4] = (int32_t)offsetof(bt_train_args, gx);
  out[5] = (int32_t)offsetof(bt_train_args, ws);
  out[6] = (int32_t)offsetof(bt_train_args, ws_bytes);
}

size_t bt_train_workspace_bytes(int unit, int backward, int B, int T, int dim, int hidden) {
  if (check_shape(unit, B, T, dim, hidden, 1 << 30)) return 0;
  return layout(unit, backward != 0, (long)B * T, dim, hidden).total * sizeof(float);
}

void bt_train_dropout_struct_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(bt_train_dropout);
  out[1] = (int32_t)offsetof(bt_train_dropout, p);
  out[2] = (int32_t)offsetof(bt_train_dropout, seed);
  out[3] = (int32_t)offsetof(bt_train_dropout, stream);
}

size_t bt_train_workspace_bytes_dropout(int unit, int backward, int B, int T, int dim, int hidden) {
  if (check_shape(unit, B, T, dim, hidden, 1 << 30)) return 0;
  return layout(unit, backward != 0, (long)B * T, dim, hidden, true).total * sizeof(float);
}

void bt_philox4x32_10_host(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  const PhiloxWords w = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = w.w[i];
}

int bt_dropout_mask_host(const bt_train_dropout* dp, int site, int B, int T, int dim, int hidden, uint8_t* out) {
  const char* fn = "bt_dropout_mask_host";
  if (!dp || !out) return fail(fn, "null argument");
  bool drop = false;   // (p == 0 is served like any other p: every element kept)
  if (const char* e = check_p(dp, &drop)) return fail(fn, e);
  if (site < BT_DROP_ATTN_P || site > BT_DROP_FF_OUT) return fail(fn, "site must be one of BT_DROP_*");
  if (B < 1 || T < 1 || dim < 32 || dim % 32 || (site == BT_DROP_FF_HIDDEN && (hidden < 4 || hidden % 4)))
    return fail(fn, "need B, T >= 1, dim a multiple of 32 and hidden a multiple of 4");
  const DropSite ds = drop_site(dp->p, dp->seed, dp->stream, site);
  if (site == BT_DROP_ATTN_P) {
    const int H = dim / 32;
    for (long bh = 0; bh < (long)B * H; ++bh)
      for (int q = 0; q < T; ++q)
        for (int k0 = 0; k0 < T; k0 += 4) {
          const PhiloxWords w = drop_words(ds, drop_attn_group((uint64_t)bh, (uint32_t)T, (uint32_t)q, (uint32_t)k0));
          for (int k = k0; k < std::min(T, k0 + 4); ++k) out[(bh * T + q) * T + k] = w.w[k - k0] >= ds.thr;
        }
    return BT_OK;
  }
  const int N = site == BT_DROP_FF_HIDDEN ? hidden : dim;
  for (long row = 0; row < (long)B * T; ++row)
    for (int c0 = 0; c0 < N; c0 += 4) {
      const PhiloxWords w = drop_words(ds, drop_row_group((uint64_t)row, (uint32_t)N, (uint32_t)c0));
      for (int j = 0; j < 4; ++j) out[row * N + c0 + j] = w.w[j] >= ds.thr;
    }
  return BT_OK;
}

int bt_train_forward(void* stream, int unit, const bt_train_args* ap) { return bt_train_forward_dropout(stream, unit, ap, nullptr); }

int bt_train_backward(void* stream, int unit, const bt_train_args* ap) { return bt_train_backward_dropout(stream, unit, ap, nullptr); }

// mixed (Launch): the 16-mixed route (train_mixed.inc) -- the GEMMs and the attention sweeps on fp16 or bfloat16 MFMAs, everything
// else as it is
static int train_forward(const char* fn, void* stream, int unit, const bt_train_args* ap, const bt_train_dropout* dp, int mixed) {
  if (!ap) return fail(fn, "null argument");
  const bt_train_args& a = *ap;
  if (const char* e = check_shape(unit, a.B, a.T, a.dim, a.hidden, a.rope_len)) return fail(fn, e);
  bool drop = false;
  if (const char* e = check_dropout(unit, dp, &drop)) return fail(fn, e);
  const long M = (long)a.B * a.T;
  const int D = a.dim, HID = a.hidden;
  const Layout L = layout(unit, 0, M, D, HID, drop);
  if (!a.x || !a.y || !a.ws) return fail(fn, "null x, y or workspace");
  if (a.ws_bytes < L.total * sizeof(float)) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
  const Launch lc{(hipStream_t)stream, mixed, drop ? dp : nullptr};
  hipStream_t s = lc.s;
  float* ws = (float*)a.ws;
  const float* resid = a.residual ? a.x : nullptr;
  switch (unit) {
    case BT_UNIT_NORM:
      if (!a.gamma) return fail(fn, "null parameter");
      hipLaunchKernelGGL(rms_fwd_kernel, dim3(blocks_of(M, 4)), dim3(256), 0, s, a.x, a.gamma, M, D, a.y, (float*)nullptr);
      break;
    case BT_TRAIN_UNIT_HEAD:
      if (!a.w1 || !a.b1 || !a.y2) return fail(fn, "null parameter or output");
      hipLaunchKernelGGL(head_fwd_kernel, dim3(blocks_of(M, 4)), dim3(256), 0, s, a.x, a.w1, a.b1, M, D, a.sum_head, a.y, a.y2);
      break;
    case BT_UNIT_FF:
      if (!a.gamma || !a.w1 || !a.b1 || !a.w2 || !a.b2) return fail(fn, "null parameter");
      hipLaunchKernelGGL(rms_fwd_kernel, dim3(blocks_of(M, 4)), dim3(256), 0, s, a.x, a.gamma, M, D, ws + L.xn, ws + L.rinv);
      linear_fwd(lc, ws + L.xn, a.w1, a.b1, M, HID, D, nullptr, nullptr, ws + L.a, BT_DROP_FF_HIDDEN, 1);
      linear_fwd(lc, ws + L.a, a.w2, a.b2, M, D, HID, a.y, resid, nullptr, BT_DROP_FF_OUT);
      break;
    default:   // attention
      if (!a.gamma || !a.w1 || !a.w2 || !a.b2 || !a.w3 || !a.rope || !a.save_o || !a.save_lse)
        return fail(fn, "null parameter, rotary table or saved-tensor pointer");
      attn_prologue(lc, a, L, ws, M);
      attn_fwd_sweep(lc, ws + L.a, a.B, a.T, D, a.save_o, a.save_lse);
      hipLaunchKernelGGL(gate_fwd_kernel, dim3(blocks_of(M * D, 256)), dim3(256), 0, s, (const float*)a.save_o,
                         (const float*)(ws + L.small0), M, D, ws + L.b);
      linear_fwd(lc, ws + L.b, a.w3, nullptr, M, D, D, a.y, resid, nullptr, BT_DROP_ATTN_OUT);
      break;
  }
  return finish(fn);
}

int bt_train_forward_dropout(void* stream, int unit, const bt_train_args* ap, const bt_train_dropout* dp) {
  return train_forward(dp ? "bt_train_forward_dropout" : "bt_train_forward", stream, unit, ap, dp, 0);
}

static int train_backward(const char* fn, void* stream, int unit, const bt_train_args* ap, const bt_train_dropout* dp, int mixed) {
  if (!ap) return fail(fn, "null argument");
  const bt_train_args& a = *ap;
  if (const char* e = check_shape(unit, a.B, a.T, a.dim, a.hidden, a.rope_len)) return fail(fn, e);
  bool drop = false;
  if (const char* e = check_dropout(unit, dp, &drop)) return fail(fn, e);
  const long M = (long)a.B * a.T;
  const int D = a.dim, HID = a.hidden, H = D / 32;
  const Layout L = layout(unit, 1, M, D, HID, drop);
  if (!a.x || !a.ws) return fail(fn, "null x or workspace");
  if (unit != BT_TRAIN_UNIT_HEAD && !a.gy) return fail(fn, "null upstream gradient");
  if (drop && (uintptr_t)a.gy % 16) return fail(fn, "with dropout the upstream gradient must be 16-byte aligned");
  if (a.ws_bytes < L.total * sizeof(float)) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
  const Launch lc{(hipStream_t)stream, mixed, drop ? dp : nullptr};
  hipStream_t s = lc.s;
  float* ws = (float*)a.ws;
  float* part = ws + L.part;
  const float* resid = a.residual ? a.gy : nullptr;
  // gy as the last linear layer of the unit sees it: behind the output site's mask with dropout (the residual takes a.gy)
  const float* gy = drop ? ws + L.gm : a.gy;
  auto mask_gy = [&](int site) {
    if (drop)
      hipLaunchKernelGGL(mask_kernel, dim3(blocks_of(M * D / 4, 256)), dim3(256), 0, s, a.gy, M * D / 4, lc.site(site), ws + L.gm);
  };
  switch (unit) {
    case BT_UNIT_NORM:
      if (!a.gamma) return fail(fn, "null parameter");
      hipLaunchKernelGGL(rms_bwd_kernel, dim3(blocks_of(M, 4)), dim3(256), 0, s, a.x, a.gamma, a.gy, (const float*)nullptr, M, D, a.gx,
                         ws + L.rinv);
      if (a.g_gamma) colsum(lc, a.gy, D, a.x, D, ws + L.rinv, 1, M, D, part, a.g_gamma);
      break;
    case BT_TRAIN_UNIT_HEAD: {
      if (!a.w1) return fail(fn, "null parameter");
      float* gbd = ws + L.small0;
      hipLaunchKernelGGL(head_bwd_kernel, dim3(blocks_of(M * D, 256)), dim3(256), 0, s, a.gy, a.gy2, a.w1, M, D, a.sum_head, gbd, a.gx);
      if (a.g_w1)
        for (int c = 0; c < 2; ++c) colsum(lc, a.x, D, nullptr, 0, gbd + c, 2, M, D, part, a.g_w1 + (long)c * D);
      if (a.g_b1) colsum(lc, gbd, 2, nullptr, 0, nullptr, 0, M, 2, part, a.g_b1);
      break;
    }
    case BT_UNIT_FF: {
      if (!a.gamma || !a.w1 || !a.b1 || !a.w2 || !a.b2) return fail(fn, "null parameter");
      float* xn = ws + L.xn;
      float* h = ws + L.a;
      float* act = ws + L.b;
      mask_gy(BT_DROP_FF_OUT);
      hipLaunchKernelGGL(rms_fwd_kernel, dim3(blocks_of(M, 4)), dim3(256), 0, s, a.x, a.gamma, M, D, xn, ws + L.rinv);
      linear_fwd(lc, xn, a.w1, a.b1, M, HID, D, h, nullptr, act, BT_DROP_FF_HIDDEN, 1);
      if (a.g_w2) linear_bwd_weight(lc, gy, act, M, D, HID, part, a.g_w2);
      if (a.g_b2) colsum(lc, gy, D, nullptr, 0, nullptr, 0, M, D, part, a.g_b2);
      linear_bwd_input(lc, gy, a.w2, M, D, HID, act);                                    // da over gelu(h)
      if (!drop)
        hipLaunchKernelGGL(gelu_bwd_kernel, dim3(blocks_of(M * HID, 256)), dim3(256), 0, s, h, (const float*)act, M * HID);   // dh over h
      else
        hipLaunchKernelGGL(gelu_bwd_drop_kernel, dim3(blocks_of(M * HID / 4, 256)), dim3(256), 0, s, h, (const float*)act, M * HID / 4,
                           lc.site(BT_DROP_FF_HIDDEN));
      if (a.g_w1) linear_bwd_weight(lc, h, xn, M, HID, D, part, a.g_w1);
      if (a.g_b1) colsum(lc, h, HID, nullptr, 0, nullptr, 0, M, HID, part, a.g_b1);
      if (a.gx || a.g_gamma) {
        linear_bwd_input(lc, h, a.w1, M, HID, D, xn);                                    // d xn over xn
        hipLaunchKernelGGL(rms_bwd_kernel, dim3(blocks_of(M, 4)), dim3(256), 0, s, a.x, a.gamma, (const float*)xn, resid, M, D, a.gx,
                           ws + L.rinv);
        if (a.g_gamma) colsum(lc, xn, D, a.x, D, ws + L.rinv, 1, M, D, part, a.g_gamma);
      }
      break;
    }
    default: {   // attention
      if (!a.gamma || !a.w1 || !a.w2 || !a.b2 || !a.w3 || !a.rope || !a.save_o || !a.save_lse)
        return fail(fn, "null parameter, rotary table or saved tensor");
      float* xn = ws + L.xn;
      float* qkv = ws + L.a;
      float* gl = ws + L.small0;
      float* og = ws + L.b;
      float* dO = ws + L.c;
      float* dqkv = ws + L.d;
      float* delta = ws + L.small1;
      float* dgl = ws + L.small2;
      mask_gy(BT_DROP_ATTN_OUT);
      attn_prologue(lc, a, L, ws, M);
      if (a.g_w3) {
        hipLaunchKernelGGL(gate_fwd_kernel, dim3(blocks_of(M * D, 256)), dim3(256), 0, s, (const float*)a.save_o, (const float*)gl, M, D,
                           og);
        linear_bwd_weight(lc, gy, og, M, D, D, part, a.g_w3);
      }
      linear_bwd_input(lc, gy, a.w3, M, D, D, dO);                                       // d og
      hipLaunchKernelGGL(gate_bwd_kernel, dim3(blocks_of(M * D, 256)), dim3(256), 0, s, (const float*)a.save_o, (const float*)gl, dO, M,
                         D, delta, dgl);                                             // -> dO, delta, d gate logits
      attn_bwd_sweeps(lc, qkv, dO, a.save_lse, delta, a.B, a.T, D, dqkv);
      hipLaunchKernelGGL(rope_kernel, dim3(blocks_of(M * D, 256)), dim3(256), 0, s, dqkv, a.rope, M, a.T, D, 1);
      if (a.g_w1) linear_bwd_weight(lc, dqkv, xn, M, 3 * D, D, part, a.g_w1);
      if (a.g_w2) linear_bwd_weight(lc, dgl, xn, M, H, D, part, a.g_w2);
      if (a.g_b2) colsum(lc, dgl, H, nullptr, 0, nullptr, 0, M, H, part, a.g_b2);
      if (a.gx || a.g_gamma) {
        float* dxn = og;   // (the gated output is no longer needed)
        linear_bwd_input(lc, dqkv, a.w1, M, 3 * D, D, dxn);
        linear_bwd_input(lc, dgl, a.w2, M, H, D, dxn, true);
        hipLaunchKernelGGL(rms_bwd_kernel, dim3(blocks_of(M, 4)), dim3(256), 0, s, a.x, a.gamma, (const float*)dxn, resid, M, D, a.gx,
                           ws + L.rinv);
        if (a.g_gamma) colsum(lc, dxn, D, a.x, D, ws + L.rinv, 1, M, D, part, a.g_gamma);
      }
      break;
    }
  }
  return finish(fn);
}

int bt_train_backward_dropout(void* stream, int unit, const bt_train_args* ap, const bt_train_dropout* dp) {
  return train_backward(dp ? "bt_train_backward_dropout" : "bt_train_backward", stream, unit, ap, dp, 0);
}

// ---- the 16-mixed route: the attention and the feed-forward only ---------------------------------------
size_t bt_train_workspace_bytes_mixed(int unit, int backward, int B, int T, int dim, int hidden, int with_dropout) {
  if (unit != BT_UNIT_ATTN && unit != BT_UNIT_FF) return 0;
  if (check_shape(unit, B, T, dim, hidden, 1 << 30)) return 0;
  return layout(unit, backward != 0, (long)B * T, dim, hidden, with_dropout != 0).total * sizeof(float);
}

// what the two entry points below refuse ahead of everything the fp32 ones check; *mixed: the route of bt_train_args.operand
static const char* check_mixed_call(int unit, const bt_train_args* ap, int* mixed) {
  if (unit != BT_UNIT_ATTN && unit != BT_UNIT_FF) return "unit must be BT_UNIT_ATTN or BT_UNIT_FF";
  if (ap && !known_operand(ap->operand)) return "operand must be BT_OPERAND_F16, BT_OPERAND_BF16 or BT_OPERAND_BF16X3";
  *mixed = ap ? route_of(1, ap->operand) : MIXED_F16;
  return nullptr;
}

int bt_train_forward_mixed(void* stream, int unit, const bt_train_args* ap, const bt_train_dropout* dp) {
  int mixed = 0;
  if (const char* e = check_mixed_call(unit, ap, &mixed)) return fail("bt_train_forward_mixed", e);
  return train_forward("bt_train_forward_mixed", stream, unit, ap, dp, mixed);
}

int bt_train_backward_mixed(void* stream, int unit, const bt_train_args* ap, const bt_train_dropout* dp) {
  int mixed = 0;
  if (const char* e = check_mixed_call(unit, ap, &mixed)) return fail("bt_train_backward_mixed", e);
  return train_backward("bt_train_backward_mixed", stream, unit, ap, dp, mixed);
}

int bt_train_matmul_mixed(void* stream, int form, const float* A, const float* B, int M, int N, int K, float* C) {
  const char* fn = "bt_train_matmul_mixed";
  if (!A || !B || !C) return fail(fn, "null argument");
  if (form < 0 || form > 2) return fail(fn, "form must be 0 (A W^T), 1 (dY W) or 2 (dY^T A)");
  if (const char* e = check_mnk(M, N, K)) return fail(fn, e);
  const Launch lc{(hipStream_t)stream, MIXED_F16, nullptr};
  if (form == 0) {          // A [M, K], B [N, K]
    linear_fwd(lc, A, B, nullptr, M, N, K, C, nullptr, nullptr);
  } else if (form == 1) {   // A [M, K], B [K, N]
    linear_bwd_input(lc, A, B, M, K, N, C);
  } else {                  // A [K, M], B [K, N]: the chunks of BT_TRAIN_DW_ROWS summed rows, added in place in chunk order
    GemmP p{};
    p.M = M; p.N = N; p.C = C; p.ldc = N;
    for (long k0 = 0; k0 < K; k0 += DW_ROWS) {
      p.A = A + k0 * M; p.lda = M; p.B = B + k0 * N; p.ldb = N;
      p.K = (int)std::min<long>(DW_ROWS, K - k0); p.kchunk = p.K; p.accum = k0 > 0;
      launch_gemm<true, true>(lc, p, 1);
    }
  }
  return finish(fn);
}

size_t bt_train_matmul_workspace_bytes(int form, int M, int N, int K) {
  if (form != 2 || check_mnk(M, N, K)) return 0;
  return (size_t)dw_chunks(K) * (size_t)M * (size_t)N * sizeof(float);
}

int bt_train_matmul(void* stream, int mixed, int form, const float* A, const float* B, int M, int N, int K, float* C,
                    const float* bias, const float* resid, int accum, float* act, const bt_train_dropout* dp, int site,
                    int drop_act, void* ws, size_t ws_bytes) {
  const char* fn = "bt_train_matmul";
  if (!known_route(mixed)) return fail(fn, BAD_ROUTE);
  if (!A || !B || !C) return fail(fn, "null argument");
  if (form < 0 || form > 2) return fail(fn, "form must be 0 (A W^T), 1 (dY W) or 2 (dY^T A)");
  if (const char* e = check_mnk(M, N, K)) return fail(fn, e);
  if (form != 0 && (bias || resid || act || dp)) return fail(fn, "bias, resid, act and dropout belong to form 0");
  if (form == 2 && accum) return fail(fn, "form 2 overwrites C");
  bool drop = false;
  if (const char* e = check_p(dp, &drop)) return fail(fn, e);
  if (drop && (site < BT_DROP_ATTN_OUT || site > BT_DROP_FF_OUT)) return fail(fn, "site must be one of the row sites of BT_DROP_*");
  if (drop && N % 4) return fail(fn, "with dropout N must be a multiple of 4");
  if (drop && drop_act && !act) return fail(fn, "drop_act masks act, which is null");
  const Launch lc{(hipStream_t)stream, mixed, drop ? dp : nullptr};
  if (form == 0) {          // A [M, K], B [N, K]
    linear_fwd(lc, A, B, bias, M, N, K, C, resid, act, site, drop_act, accum != 0);
  } else if (form == 1) {   // A [M, K], B [K, N]
    linear_bwd_input(lc, A, B, M, K, N, C, accum != 0);
  } else {                  // A [K, M], B [K, N]: partials of BT_TRAIN_DW_ROWS summed rows in ws, then added in chunk order
    if (!ws) return fail(fn, "form 2 needs a workspace");
    if (ws_bytes < bt_train_matmul_workspace_bytes(2, M, N, K)) return fail(fn, "workspace too small", BT_ERR_WORKSPACE);
    linear_bwd_weight(lc, A, B, K, M, N, (float*)ws, C);
  }
  return finish(fn);
}

int bt_train_attention(void* stream, int mixed, int backward, int B, int T, int dim, const float* qkv,
                       const bt_train_dropout* dp, float* O, float* lse, const float* dO, const float* delta, float* dqkv) {
  const char* fn = "bt_train_attention";
  if (!known_route(mixed)) return fail(fn, BAD_ROUTE);
  if (const char* e = check_width(dim)) return fail(fn, e);
  if (B < 1 || B > 65535 || T < 1 || (long)B * T > (1L << 22)) return fail(fn, "need 1 <= B <= 65535, T >= 1 and B T <= 2^22");
  if (!qkv || !lse || (backward ? !dO || !delta || !dqkv : !O)) return fail(fn, "null argument");
  if ((uintptr_t)qkv % 16 || (backward ? (uintptr_t)dO % 16 || (uintptr_t)dqkv % 16 : (uintptr_t)O % 16))
    return fail(fn, "qkv, O, dO and dqkv must be 16-byte aligned");
  bool drop = false;
  if (const char* e = check_p(dp, &drop)) return fail(fn, e);
  const Launch lc{(hipStream_t)stream, mixed, drop ? dp : nullptr};
  if (!backward)
    attn_fwd_sweep(lc, qkv, B, T, dim, O, lse);
  else
    attn_bwd_sweeps(lc, qkv, dO, lse, delta, B, T, dim, dqkv);
  return finish(fn);
}

}  // extern "C"
