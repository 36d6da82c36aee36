// The 16-mixed kernels of the training route (DESIGN.md section 16), included by train.hip; what they share with its fp32
// kernels (GemmP, the GEMM epilogue, the vector types, the scale constants) is train_common.h.
// THE CONTRACT: both operands of every matrix product are rounded to IEEE fp16 (round to nearest even) as they are staged, and
// the product accumulates in fp32 on v_mfma_f32_32x32x16_f16.  Everything else of the route is the fp32 code of train.hip.  A
// value beyond fp16's range becomes inf and propagates: nothing clamps, the loss scaler sees it in the gradient norm.
// Every kernel below is a template over the operand element type E (Operand<E>, train_common.h): E = _Float16 is that contract,
// E = __bf16 (DESIGN.md section 24) is the same with one word changed -- both operands rounded to bfloat16, to nearest even, NaN
// stays NaN, nothing overflows by rounding -- on v_mfma_f32_32x32x16_bf16.  Staging, lane maps, orders of summation and the mask
// mapping do not depend on E.
// E = bf16x3 (DESIGN.md section 25, "32-high") keeps every staged operand as two bfloat16 images, hi = bf16(a) and lo = bf16(a - hi)
// (to_img, train_common.h), and every product becomes A_lo B_hi + A_hi B_lo + A_hi B_hi, three MFMAs in that order into the one
// accumulator.  The operands rounded in registers (P, dS, the own side's fragments) are split in registers the same way.
//
// Lane maps of the 32x32x16 fp16 MFMA (lane l, r = l & 31, h = l >> 5, element j = 0 .. 7 of a fragment):
//   A[row r][k = 8 h + j],  B[k = 8 h + j][col r],  C / D register i: row = (i & 3) + 8 (i >> 2) + 4 h, col = r.
// A 32 x 32 result X, rounded to fp16 eight registers at a time, is the B operand of a product A X that sums over X's rows:
// element j of lane half h of k-step s is row 16 s + 8 (j >> 2) + 4 h + (j & 3) of X, so the A operand's element j has to come
// from that k (the `t` images below: [d][row] with the two groups of four read as 8-byte words).
//
// Reproducibility is that of train.hip: no atomics, one thread of one launch per output byte, every order of summation a
// function of the shapes alone (a GEMM element: k ascending in MFMA steps of 16; dQ: key tiles of 32 ascending; dK / dV: query
// tiles of 32 ascending), and a row's results do not depend on the other sequences of the batch.

#include "train_common.h"

namespace {

constexpr int MT = 128;        // GEMM tile: MT x MT outputs per workgroup of four waves (2 x 2 waves of 2 x 2 MFMA tiles)
constexpr int MK = 32;         // k per staging step
constexpr int MLD = MK + 8;    // halves per LDS row: 80 bytes, so the 16-byte fragment reads of 32 rows spread over the banks
constexpr int XB = 32;         // attention: queries (keys) per wave and keys (queries) per tile

// Stage rows [r0, r0 + MT) x k [k0, k0 + MK) of an operand as fp16 into S[row][k].  TR: the operand is stored [k][row].  What
// lies behind row R or behind k = ke is zero and is never read; `vec`: 16-byte loads are possible (alignment of the base, the
// leading dimension and the chunk's first k).
template <typename E, bool TR>
__device__ inline void mx_stage(const float* P, long ld, long r0, long R, long k0, long ke, bool vec, el16<E> (*S)[MT][MLD], int tid) {
#pragma unroll
  for (int i = 0; i < MT * MK / 4 / 256; ++i) {
    const int gi = tid + i * 256;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!TR) {
      const int row = gi >> 3, kk = (gi & 7) * 4;
      const long gr = r0 + row, gk = k0 + kk;
      if (gr < R && gk < ke) {
        const float* p = P + gr * ld + gk;
        if (vec && gk + 3 < ke) {
          v = *reinterpret_cast<const f32x4*>(p);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (gk + c < ke) v[c] = p[c];
        }
      }
      const Img4<E> q = to_h4<E>(v);
#pragma unroll
      for (int n = 0; n < Operand<E>::NI; ++n) *reinterpret_cast<h16x4<E>*>(&S[n][row][kk]) = q.v[n];
    } else {
      const int kk = gi >> 5, row = (gi & 31) * 4;
      const long gr = r0 + row, gk = k0 + kk;
      if (gr < R && gk < ke) {
        const float* p = P + gk * ld + gr;
        if (vec && gr + 3 < R) {
          v = *reinterpret_cast<const f32x4*>(p);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (gr + c < R) v[c] = p[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        el16<E> e[Operand<E>::NI];
        to_img<E>(v[c], e);
#pragma unroll
        for (int n = 0; n < Operand<E>::NI; ++n) S[n][row + c][kk] = e[n];
      }
    }
  }
}

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// gemm_body with fp16 operands: the same GemmP, the same epilogue (bias, residual, +=, GELU into a second output, dropout)
template <typename E, bool AT, bool BT, bool DROP>
__device__ inline void mx_gemm_body(const GemmP& p, const DropSite& ds, int drop_act) {
  __shared__ __attribute__((aligned(16))) el16<E> As[Operand<E>::NI][MT][MLD];
  __shared__ __attribute__((aligned(16))) el16<E> Bs[Operand<E>::NI][MT][MLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, lr = lane & 31, wm = wave >> 1, wn = wave & 1;
  const long m0 = (long)blockIdx.y * MT, n0 = (long)blockIdx.x * MT;
  const long kb = (long)blockIdx.z * p.kchunk, ke = std::min<long>(p.K, kb + p.kchunk);
  const bool va = aligned16(p.A) && p.lda % 4 == 0 && (AT || kb % 4 == 0);
  const bool vb = aligned16(p.B) && p.ldb % 4 == 0 && (BT || kb % 4 == 0);
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  for (long k0 = kb; k0 < ke; k0 += MK) {
    mx_stage<E, AT>(p.A, p.lda, m0, p.M, k0, ke, va, As, tid);
    mx_stage<E, BT>(p.B, p.ldb, n0, p.N, k0, ke, vb, Bs, tid);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < MK / 16; ++s) {
      Img8<E> a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < Operand<E>::NI; ++n) {
          a[i].v[n] = *reinterpret_cast<const h16x8<E>*>(&As[n][wm * 64 + i * 32 + lr][16 * s + 8 * g]);
          b[i].v[n] = *reinterpret_cast<const h16x8<E>*>(&Bs[n][wn * 64 + i * 32 + lr][16 * s + 8 * g]);
        }
      // term-major over the four accumulators: consecutive MFMAs never depend on each other, each accumulator sees its terms in order
#pragma unroll
      for (int t = 0; t < Operand<E>::NT; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = Operand<E>::mfma(a[i].v[Operand<E>::ta(t)], b[j].v[Operand<E>::tb(t)], acc[i][j]);
    }
    __syncthreads();
  }
  float* C = p.C ? p.C + (long)blockIdx.z * p.cz : nullptr;
  gemm_epilogue<DROP>(p, ds, drop_act, C, acc[0][0], m0 + wm * 64, n0 + wn * 64 + lr, lane);
  gemm_epilogue<DROP>(p, ds, drop_act, C, acc[0][1], m0 + wm * 64, n0 + wn * 64 + 32 + lr, lane);
  gemm_epilogue<DROP>(p, ds, drop_act, C, acc[1][0], m0 + wm * 64 + 32, n0 + wn * 64 + lr, lane);
  gemm_epilogue<DROP>(p, ds, drop_act, C, acc[1][1], m0 + wm * 64 + 32, n0 + wn * 64 + 32 + lr, lane);
}

template <typename E, bool AT, bool BT>
__global__ __launch_bounds__(256) void mx_gemm_kernel(const GemmP p) {
  mx_gemm_body<E, AT, BT, false>(p, DropSite{}, 0);
}

template <typename E>
__global__ __launch_bounds__(256) void mx_gemm_drop_kernel(const GemmP p, const DropSite ds, const int drop_act) {
  mx_gemm_body<E, false, false, true>(p, ds, drop_act);
}

// ---- attention, head dim 32, one wave per workgroup: XB own rows against tiles of XB rows of the other side -------------------
// Stage rows [t0, t0 + XB) of a [T, 32] slice (row stride ld) as fp16: R[row][d] and / or Tt[d][row]; rows >= T are zeros.
template <typename E>
__device__ inline void mx_stage32(const float* base, long ld, int t0, int T, el16<E> (*R)[XB][MLD], el16<E> (*Tt)[XB][MLD], int lane) {
#pragma unroll
  for (int i = 0; i < XB * 8 / 64; ++i) {
    const int idx = i * 64 + lane, row = idx >> 3, part = idx & 7;
    const int t = t0 + row;
    const f32x4 v = t < T ? reinterpret_cast<const f32x4*>(base + (long)t * ld)[part] : f32x4{0.f, 0.f, 0.f, 0.f};
    const Img4<E> q = to_h4<E>(v);
#pragma unroll
    for (int n = 0; n < Operand<E>::NI; ++n) {
      if (R) *reinterpret_cast<h16x4<E>*>(&R[n][row][4 * part]) = q.v[n];
      if (Tt) {
#pragma unroll
        for (int c = 0; c < 4; ++c) Tt[n][4 * part + c][row] = q.v[n][c];
      }
    }
  }
}

// the own side's row r as the B operand [k = d][col r] of both k-steps
template <typename E>
__device__ inline void mx_own_frag(const float* row, bool ok, int h, Img8<E> (&f)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const f32x4 lo = ok ? reinterpret_cast<const f32x4*>(row + 16 * s + 8 * h)[0] : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 hi = ok ? reinterpret_cast<const f32x4*>(row + 16 * s + 8 * h)[1] : f32x4{0.f, 0.f, 0.f, 0.f};
    const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    f[s] = to_h8<E>(x);
  }
}

// X[tile row][own col] = sum_d R[tile row][d] own[col][d]
template <typename E>
__device__ inline f32x16 mx_first(const el16<E> (*R)[XB][MLD], const Img8<E> (&own)[2], int r, int h) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    Img8<E> a;
#pragma unroll
    for (int n = 0; n < Operand<E>::NI; ++n) a.v[n] = *reinterpret_cast<const h16x8<E>*>(&R[n][r][16 * s + 8 * h]);
    acc = mfma_terms<E>(a, own[s], acc);
  }
  return acc;
}

// acc[d][own col] += sum_rows Tt[d][tile row] X[tile row][own col], X = the sixteen fp32 values of a lane, rounded here
template <typename E>
__device__ inline void mx_second(const el16<E> (*Tt)[XB][MLD], const float (&x)[16], int r, int h, f32x16& acc) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    Img8<E> a;
#pragma unroll
    for (int n = 0; n < Operand<E>::NI; ++n) {
      const h16x4<E> a0 = *reinterpret_cast<const h16x4<E>*>(&Tt[n][r][16 * s + 4 * h]);
      const h16x4<E> a1 = *reinterpret_cast<const h16x4<E>*>(&Tt[n][r][16 * s + 8 + 4 * h]);
      a.v[n] = h16x8<E>{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    }
    const float xs[8] = {x[8 * s], x[8 * s + 1], x[8 * s + 2], x[8 * s + 3], x[8 * s + 4], x[8 * s + 5], x[8 * s + 6], x[8 * s + 7]};
    acc = mfma_terms<E>(a, to_h8<E>(xs), acc);
  }
}

// out[d] = acc[d][own col] * scale for the sixteen d of this lane (four groups of four consecutive ones)
__device__ inline void mx_store_t(float* out, const f32x16& acc, int h, float scale) {
#pragma unroll
  for (int gq = 0; gq < 4; ++gq)
    *reinterpret_cast<f32x4*>(out + 8 * gq + 4 * h) =
        f32x4{acc[4 * gq] * scale, acc[4 * gq + 1] * scale, acc[4 * gq + 2] * scale, acc[4 * gq + 3] * scale};
}

// O = softmax(q k^T / sqrt(32)) v before the gate and lse, as attn_fwd_body: the scores of a key tile are S^T[key][query] (the
// query on the lane), the running maximum and sum are per lane, and P^T -- relative to the running maximum, times the mask and
// 1 / (1 - p) with DROP, rounded to fp16 -- is the B operand of O^T += V^T P^T.
template <typename E, bool DROP>
__device__ inline void mx_attn_fwd_body(const float* qkv, int T, int D, float* O, float* lse, const DropSite& ds) {
  __shared__ __attribute__((aligned(16))) el16<E> Kr[Operand<E>::NI][XB][MLD];
  __shared__ __attribute__((aligned(16))) el16<E> Vt[Operand<E>::NI][XB][MLD];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5, hd = blockIdx.y, b = blockIdx.z, H = D / 32;
  const int t = blockIdx.x * XB + r;
  const bool ok = t < T;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + hd * 32;
  Img8<E> qf[2];
  mx_own_frag<E>(base + (long)(ok ? t : 0) * ld, ok, h, qf);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  float mx = -INFINITY, l = 0.0f;   // (l: this lane's half of the keys; the halves meet at the end)
  for (int k0 = 0; k0 < T; k0 += XB) {
    __syncthreads();
    mx_stage32<E>(base + D, ld, k0, T, Kr, nullptr, lane);
    mx_stage32<E>(base + 2 * D, ld, k0, T, nullptr, Vt, lane);
    __syncthreads();
    const f32x16 st = mx_first<E>(Kr, qf, r, h);
    float sc[16], tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * h;
      sc[i] = key < T ? st[i] * QK_SCALE_LOG2E : -INFINITY;
      tm = fmaxf(tm, sc[i]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));   // (a tile has at least one key: finite)
    const float mnew = fmaxf(mx, tm), corr = exp2f(mx - mnew);
    mx = mnew;
    l *= corr;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] *= corr;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      PhiloxWords w{};
      if constexpr (DROP)
        w = drop_words(ds, drop_attn_group((uint64_t)b * H + hd, (uint32_t)T, (uint32_t)t, (uint32_t)(k0 + 8 * gq + 4 * h)));
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float p = exp2f(sc[4 * gq + jj] - mx);
        l += p;
        sc[4 * gq + jj] = DROP ? (w.w[jj] >= ds.thr ? p * ds.scale : 0.0f) : p;
      }
    }
    mx_second<E>(Vt, sc, r, h, acc);
  }
  l += __shfl_xor(l, 32, 64);
  if (!ok) return;
  const long m = (long)b * T + t;
  mx_store_t(O + m * D + hd * 32, acc, h, 1.0f / l);
  if (h == 0) lse[m * H + hd] = mx + log2f(l);
}

template <typename E>
__global__ __launch_bounds__(64) void mx_attn_fwd_kernel(const float* qkv, int T, int D, float* O, float* lse) {
  mx_attn_fwd_body<E, false>(qkv, T, D, O, lse, DropSite{});
}
template <typename E>
__global__ __launch_bounds__(64) void mx_attn_fwd_drop_kernel(const float* qkv, int T, int D, float* O, float* lse, const DropSite ds) {
  mx_attn_fwd_body<E, true>(qkv, T, D, O, lse, ds);
}

// dq of XB queries: key tiles in ascending order.  S^T and dP^T = V dO^T have the query on the lane; dS^T = P^T (dP^T - delta)
// in fp32, rounded, is the B operand of dQ^T += K^T dS^T.
template <typename E, bool DROP>
__device__ inline void mx_attn_dq_body(const float* qkv, const float* dO, const float* lse, const float* delta, int T, int D,
                                       float* dqkv, const DropSite& ds) {
  __shared__ __attribute__((aligned(16))) el16<E> Kr[Operand<E>::NI][XB][MLD];
  __shared__ __attribute__((aligned(16))) el16<E> Kt[Operand<E>::NI][XB][MLD];
  __shared__ __attribute__((aligned(16))) el16<E> Vr[Operand<E>::NI][XB][MLD];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5, hd = blockIdx.y, b = blockIdx.z, H = D / 32;
  const int t = blockIdx.x * XB + r;
  const bool ok = t < T;
  const long ld = 3L * D, m = (long)b * T + (ok ? t : 0);
  const float* base = qkv + (long)b * T * ld + hd * 32;
  Img8<E> qf[2], gf[2];
  mx_own_frag<E>(base + (long)(ok ? t : 0) * ld, ok, h, qf);
  mx_own_frag<E>(dO + m * D + hd * 32, ok, h, gf);
  const float ls = ok ? lse[m * H + hd] : 0.0f, dl = ok ? delta[m * H + hd] : 0.0f;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  for (int k0 = 0; k0 < T; k0 += XB) {
    __syncthreads();
    mx_stage32<E>(base + D, ld, k0, T, Kr, Kt, lane);
    mx_stage32<E>(base + 2 * D, ld, k0, T, Vr, nullptr, lane);
    __syncthreads();
    const f32x16 st = mx_first<E>(Kr, qf, r, h);
    const f32x16 dp = mx_first<E>(Vr, gf, r, h);
    float dst[16];
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      PhiloxWords w{};
      if constexpr (DROP)
        w = drop_words(ds, drop_attn_group((uint64_t)b * H + hd, (uint32_t)T, (uint32_t)t, (uint32_t)(k0 + 8 * gq + 4 * h)));
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int i = 4 * gq + jj, key = k0 + 8 * gq + 4 * h + jj;
        const float p = key < T ? exp2f(st[i] * QK_SCALE_LOG2E - ls) : 0.0f;
        const float d = DROP ? (w.w[jj] >= ds.thr ? dp[i] * ds.scale : 0.0f) : dp[i];
        dst[i] = p * (d - dl);
      }
    }
    mx_second<E>(Kt, dst, r, h, acc);
  }
  if (ok) mx_store_t(dqkv + ((long)b * T + t) * ld + hd * 32, acc, h, QK_SCALE);
}

template <typename E>
__global__ __launch_bounds__(64) void mx_attn_dq_kernel(const float* qkv, const float* dO, const float* lse, const float* delta, int T,
                                                        int D, float* dqkv) {
  mx_attn_dq_body<E, false>(qkv, dO, lse, delta, T, D, dqkv, DropSite{});
}
template <typename E>
__global__ __launch_bounds__(64) void mx_attn_dq_drop_kernel(const float* qkv, const float* dO, const float* lse, const float* delta,
                                                             int T, int D, float* dqkv, const DropSite ds) {
  mx_attn_dq_body<E, true>(qkv, dO, lse, delta, T, D, dqkv, ds);
}

// dk and dv of XB keys: query tiles in ascending order.  S and dP = dO V^T have the key on the lane and the queries in the
// registers; P (masked and scaled with DROP) and dS, rounded, are the B operands of dV^T += dO^T P and dK^T += Q^T dS.  The four
// keys of a quad of lanes are one mask group of every query: the lanes evaluate four queries' groups and exchange the words.
template <typename E, bool DROP>
__device__ inline void mx_attn_dkv_body(const float* qkv, const float* dO, const float* lse, const float* delta, int T, int D,
                                        float* dqkv, const DropSite& ds) {
  __shared__ __attribute__((aligned(16))) el16<E> Qr[Operand<E>::NI][XB][MLD];
  __shared__ __attribute__((aligned(16))) el16<E> Qt[Operand<E>::NI][XB][MLD];
  __shared__ __attribute__((aligned(16))) el16<E> Gr[Operand<E>::NI][XB][MLD];
  __shared__ __attribute__((aligned(16))) el16<E> Gt[Operand<E>::NI][XB][MLD];
  __shared__ float Ls[XB], Ds[XB];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5, hd = blockIdx.y, b = blockIdx.z, H = D / 32;
  const int t = blockIdx.x * XB + r;
  const bool ok = t < T;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + hd * 32;
  const float* gbase = dO + (long)b * T * D + hd * 32;
  Img8<E> kf[2], vf[2];
  mx_own_frag<E>(base + D + (long)(ok ? t : 0) * ld, ok, h, kf);
  mx_own_frag<E>(base + 2 * D + (long)(ok ? t : 0) * ld, ok, h, vf);
  f32x16 dk, dv;
#pragma unroll
  for (int i = 0; i < 16; ++i) dk[i] = dv[i] = 0.0f;
  for (int q0 = 0; q0 < T; q0 += XB) {
    __syncthreads();
    mx_stage32<E>(base, ld, q0, T, Qr, Qt, lane);
    mx_stage32<E>(gbase, D, q0, T, Gr, Gt, lane);
    if (lane < XB) {
      const int tq = q0 + lane;
      const long mq = (long)b * T + tq;
      Ls[lane] = tq < T ? lse[mq * H + hd] : 0.0f;
      Ds[lane] = tq < T ? delta[mq * H + hd] : 0.0f;
    }
    __syncthreads();
    const f32x16 st = mx_first<E>(Qr, kf, r, h);
    const f32x16 dp = mx_first<E>(Gr, vf, r, h);
    float pm[16], dst[16];
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      uint32_t mine[4] = {0u, 0u, 0u, 0u};
      if constexpr (DROP) {   // (every lane of the wave takes part, also the ones behind key T - 1)
        const PhiloxWords w = drop_words(
            ds, drop_attn_group((uint64_t)b * H + hd, (uint32_t)T, (uint32_t)(q0 + 8 * gq + 4 * h + (lane & 3)), (uint32_t)t));
        mine[0] = w.w[0]; mine[1] = w.w[1]; mine[2] = w.w[2]; mine[3] = w.w[3];
        quad_transpose(mine, lane);
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int i = 4 * gq + jj, row = 8 * gq + 4 * h + jj;
        const float p = q0 + row < T ? exp2f(st[i] * QK_SCALE_LOG2E - Ls[row]) : 0.0f;
        const bool kept = !DROP || mine[jj] >= ds.thr;
        const float c = DROP ? ds.scale : 1.0f;
        pm[i] = kept ? p * c : 0.0f;
        dst[i] = p * ((kept ? dp[i] * c : 0.0f) - Ds[row]);
      }
    }
    mx_second<E>(Gt, pm, r, h, dv);
    mx_second<E>(Qt, dst, r, h, dk);
  }
  if (!ok) return;
  float* out = dqkv + ((long)b * T + t) * ld + hd * 32;
  mx_store_t(out + D, dk, h, QK_SCALE);
  mx_store_t(out + 2 * D, dv, h, 1.0f);
}

template <typename E>
__global__ __launch_bounds__(64) void mx_attn_dkv_kernel(const float* qkv, const float* dO, const float* lse, const float* delta, int T,
                                                         int D, float* dqkv) {
  mx_attn_dkv_body<E, false>(qkv, dO, lse, delta, T, D, dqkv, DropSite{});
}
template <typename E>
__global__ __launch_bounds__(64) void mx_attn_dkv_drop_kernel(const float* qkv, const float* dO, const float* lse, const float* delta,
                                                              int T, int D, float* dqkv, const DropSite ds) {
  mx_attn_dkv_body<E, true>(qkv, dO, lse, delta, T, D, dqkv, ds);
}

}  // namespace
