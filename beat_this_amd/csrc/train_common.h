// What the fp32 kernels of train.hip and the 16-mixed kernels of train_mixed.inc share: the GEMM's parameter block and its
// epilogue, the vector types, the attention's scale constants, GELU and the quad exchange of mask words.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/beat_this_amd.h"   // BT_OPERAND_*
#include "dropout.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// The operand format of the 16-mixed kernels (DESIGN.md sections 16, 19, 24 and 25): _Float16, __bf16, or bf16x3 -- the 32-high
// format, every fp32 operand as two bfloat16 images.  `el` is the element type of an image, NI the number of images, x4 / x8 the
// fragments of four and eight and `mfma` the 32x32x16 MFMA.  Lane maps and rates are the same for all; float -> el is the
// compiler's conversion (round to nearest even; fp16 overflows to inf, bf16 has fp32's exponent range).
// A product is NT MFMAs into the one accumulator: term t multiplies image ta(t) of A with image tb(t) of B.  bf16x3 (image 0 = hi,
// 1 = lo) issues lo hi, hi lo, hi hi -- the small terms first -- and drops lo lo.
struct bf16x3 {};
template <typename E> struct Operand;
template <> struct Operand<_Float16> {
  typedef _Float16 el;
  typedef _Float16 x4 __attribute__((ext_vector_type(4)));
  typedef _Float16 x8 __attribute__((ext_vector_type(8)));
  static constexpr int NI = 1, NT = 1;
  static constexpr int ta(int) { return 0; }
  static constexpr int tb(int) { return 0; }
  static __device__ inline f32x16 mfma(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct Operand<__bf16> {
  typedef __bf16 el;
  typedef __bf16 x4 __attribute__((ext_vector_type(4)));
  typedef __bf16 x8 __attribute__((ext_vector_type(8)));
  static constexpr int NI = 1, NT = 1;
  static constexpr int ta(int) { return 0; }
  static constexpr int tb(int) { return 0; }
  static __device__ inline f32x16 mfma(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Operand<bf16x3> : Operand<__bf16> {
  static constexpr int NI = 2, NT = 3;
  static constexpr int ta(int t) { return t == 0; }
  static constexpr int tb(int t) { return t == 1; }
};
template <typename E> using el16 = typename Operand<E>::el;
template <typename E> using h16x4 = typename Operand<E>::x4;
template <typename E> using h16x8 = typename Operand<E>::x8;
template <typename E> constexpr int operand_images = Operand<E>::NI;

// The list of the formats for the host code of train.hip and train_front.hip (a new one: a specialisation above, an entry in
// known_operand, BT_FOR_OPERANDS and pick_route, and a branch of train_front.hip's launch_conv).  A call's route is 0 for the
// fp32 kernels, else 1 + BT_OPERAND_*: the `mixed` of bt_train_matmul / bt_train_attention.
constexpr bool known_operand(int operand) { return operand == BT_OPERAND_F16 || operand == BT_OPERAND_BF16 || operand == BT_OPERAND_BF16X3; }
constexpr int route_of(int mixed, int operand) { return mixed ? 1 + operand : 0; }
constexpr bool known_route(int route) { return route == 0 || known_operand(route - 1); }
// the instantiations of a template K<E, ...> over the formats, in the order pick_route takes them
#define BT_FOR_OPERANDS(K, ...) K<_Float16, ##__VA_ARGS__>, K<__bf16, ##__VA_ARGS__>, K<bf16x3, ##__VA_ARGS__>
// what belongs to a known route among the fp32 form and the three of BT_FOR_OPERANDS
template <typename K> K pick_route(int route, K f32, K f16, K bf16, K x3) {
  return route == route_of(1, BT_OPERAND_BF16X3) ? x3 : route == route_of(1, BT_OPERAND_BF16) ? bf16 : route ? f16 : f32;
}

// the NI images of four / eight consecutive elements
template <typename E> struct Img4 { h16x4<E> v[Operand<E>::NI]; };
template <typename E> struct Img8 { h16x8<E> v[Operand<E>::NI]; };

// The images of one fp32 value.  NI = 1: the rounded value.  bf16x3: hi = bf16(a), lo = bf16(a - hi), the subtraction exact in
// fp32; where hi is not finite (a is inf or NaN, or rounds to inf) lo = 0, so that no inf meets a -inf in the partial products.
template <typename E>
__device__ inline void to_img(float a, el16<E> (&o)[Operand<E>::NI]) {
  o[0] = (el16<E>)a;
  if constexpr (Operand<E>::NI == 2) {
    const float hi = (float)o[0];
    const bool finite = (__float_as_uint(hi) & 0x7f800000u) != 0x7f800000u;
    o[1] = (el16<E>)(finite ? a - hi : 0.0f);
  }
}
template <typename E>
__device__ inline Img4<E> to_h4(f32x4 v) {
  Img4<E> o;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    el16<E> e[Operand<E>::NI];
    to_img<E>(v[c], e);
#pragma unroll
    for (int n = 0; n < Operand<E>::NI; ++n) o.v[n][c] = e[n];
  }
  return o;
}
template <typename E>
__device__ inline Img8<E> to_h8(const float (&x)[8]) {
  Img8<E> o;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    el16<E> e[Operand<E>::NI];
    to_img<E>(x[c], e);
#pragma unroll
    for (int n = 0; n < Operand<E>::NI; ++n) o.v[n][c] = e[n];
  }
  return o;
}
// acc += a b, term by term in the format's order
template <typename E>
__device__ inline f32x16 mfma_terms(const Img8<E>& a, const Img8<E>& b, f32x16 acc) {
#pragma unroll
  for (int t = 0; t < Operand<E>::NT; ++t) acc = Operand<E>::mfma(a.v[Operand<E>::ta(t)], b.v[Operand<E>::tb(t)], acc);
  return acc;
}

constexpr float QK_SCALE = 0.17677669529663687f;            // 32^-0.5
constexpr float QK_SCALE_LOG2E = 0.2550348616841918f;       // 32^-0.5 * log2(e)

// ---- GEMM: C[m][n] (+)= sum_k A(m, k) B(n, k) over k in [z kchunk, (z + 1) kchunk) --------------------------------------
// A(m, k) = AT ? A[k lda + m] : A[m lda + k];  B(n, k) = BT ? B[k ldb + n] : B[n ldb + k]
struct GemmP {
  const float* A; long lda;
  const float* B; long ldb;
  int M, N, K, kchunk;
  float* C; long ldc; long cz;      // C of chunk z starts at C + z cz (C may be null when only act is wanted)
  const float* bias;                // + bias[n]
  const float* resid; long ldr;     // + resid[m][n]
  int accum;                        // + the old C[m][n]
  float* act; long ldact;           // act[m][n] = gelu(value)
};

__device__ inline float gelu_f(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
__device__ inline float gelu_grad_f(float v) {
  return 0.5f * (1.0f + erff(v * 0.70710678118654752f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
}

// a[jj] of lane l of a quad of lanes (4 q .. 4 q + 3) becomes a[l mod 4] of lane 4 q + jj: a 4 x 4 transpose over three
// exchanges.  Every lane of the quad has to be active.
__device__ inline void quad_transpose(uint32_t (&a)[4], int lane) {
  const int ql = lane & 3, qb = lane & ~3;
  uint32_t b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int give = (ql - s) & 3, from = (ql + s) & 3;
    uint32_t v = give == 0 ? a[0] : give == 1 ? a[1] : give == 2 ? a[2] : a[3];
    if (s) v = (uint32_t)__shfl((int)v, qb + from, 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = from == k ? v : b[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = b[k];
}

// The GEMMs' epilogue for one 32 x 32 MFMA tile (C / D map of the 32x32 MFMAs: register r of lane l is row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5)): rows rb .., this lane's column col, C the chunk's output or null.
// DROP: the site `ds` over the [M][N] result (N a multiple of 4): drop_act == 0 masks the value before the residual is added
// (C = resid + m c (acc + bias)), drop_act != 0 masks the second output (act = m c gelu(value)) and leaves C alone.  A lane
// evaluates the groups of four of its sixteen rows and the quad exchanges the words, so every word of a call is used.
template <bool DROP>
__device__ inline void gemm_epilogue(const GemmP& p, const DropSite& ds, int drop_act, float* C, const f32x16& acc, long rb, long col,
                                     int lane) {
  if (col >= p.N) return;   // (DROP: N is a multiple of 4, the four lanes of a quad are all here or all gone)
  const int g = lane >> 5;
  const float b = p.bias ? p.bias[col] : 0.0f;
  uint32_t words[16];
  if constexpr (DROP) {
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) {
      const long row = rb + (lane & 3) + 8 * ri + 4 * g;
      const PhiloxWords w = drop_words(ds, drop_row_group((uint64_t)row, (uint32_t)p.N, (uint32_t)col));
      uint32_t q[4] = {w.w[0], w.w[1], w.w[2], w.w[3]};
      quad_transpose(q, lane);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) words[4 * ri + jj] = q[jj];
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long row = rb + (r & 3) + 8 * (r >> 2) + 4 * g;
    if (row < p.M) {
      float v = acc[r] + b;
      float keep = 1.0f;
      if constexpr (DROP) {
        keep = words[r] >= ds.thr ? ds.scale : 0.0f;
        if (!drop_act) v *= keep;
      }
      if (p.resid) v += p.resid[row * p.ldr + col];
      if (p.accum) v += C[row * p.ldc + col];
      if (C) C[row * p.ldc + col] = v;
      if (p.act) p.act[row * p.ldact + col] = DROP && drop_act ? gelu_f(v) * keep : gelu_f(v);
    }
  }
}

}  // namespace
