// The gradient sum of data-parallel fine-tuning: `world` fp32 arrays ("parts", rank r's at d_parts + r * stride) are added
// element by element IN RANK ORDER, one rounded fp32 add at a time:
//     out[i] = ((parts[0][i] + parts[1][i]) + parts[2][i]) + ...
// which is what autograd's in-place accumulation over the same gradients in the same order computes.  DESIGN.md section 26.
//
// A streaming kernel in the style of the AdamW step (optim.hip): one 256-thread workgroup takes one chunk of BT_REDUCE_CHUNK
// elements, four rounds of one float4 per lane.  A lane issues the `world` loads of its quad before the first add, so their
// latencies overlap; world 2, 4 and 8 are unrolled instantiations, every other world runs a loop over the ranks.  16 bytes per
// (non-temporal) load when d_parts, d_out and stride allow it; otherwise, and for the tail n % 4, one element per lane.  No LDS, no atomics:
// every output element is written by exactly one lane, which has read the `world` inputs of that element and nothing else,
// so d_out may be rank 0's part itself.
// Host: bt_grad_rank_sum_host does the same adds in the same order.  The file is compiled with -ffp-contract=off (there is
// nothing to contract in a chain of adds, the flag keeps it so) and without flushing denormals: device == host bit for bit.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/beat_this_amd.h"

#pragma clang fp contract(off)

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

constexpr int CHUNK = BT_REDUCE_CHUNK;
constexpr int THREADS = 256;
constexpr int ROUNDS = CHUNK / (4 * THREADS);
static_assert(CHUNK % (4 * THREADS) == 0, "whole float4 rounds per workgroup");

__device__ inline float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// The parts are read once and never again: the 16-byte loads are non-temporal, so the stream does not displace what the
// optimiser's kernels read next (tools/ddp_speed.py: 0.0203 against 0.0231 ms at world 2, 0.0179 / 0.0202 at 4, 0.0186 / 0.0201
// at 8 with plain loads, final0's size, spreads of 2 %).
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ inline float4 ld4(const float* p, int i) {
  const f4 v = __builtin_nontemporal_load((const f4*)p + i);
  return make_float4(v.x, v.y, v.z, v.w);
}

// W > 0: the unrolled form for exactly W ranks; W == 0: any world, a loop.  (parts and out may be the same pointer: no
// __restrict__ on either.)
template <int W>
__global__ __launch_bounds__(THREADS) void rank_sum_kernel(const float* parts, int64_t stride, int world, int64_t n, float* out,
                                                           int wide) {
  const int64_t base = (int64_t)blockIdx.x * CHUNK;
  if (base >= n) return;
  const int cnt = (int)(n - base < CHUNK ? n - base : CHUNK);
  const float* P = parts + base;
  float* O = out + base;
  const int p = threadIdx.x;
  const int n4 = wide ? cnt >> 2 : 0;
  if (wide) {   // (base and stride are multiples of 4 elements, both pointers 16-byte aligned)
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
      const int i = k * THREADS + p;
      if (i < n4) {
        float4 acc;
        if (W > 0) {
          float4 v[W > 0 ? W : 1];
#pragma unroll
          for (int r = 0; r < W; ++r) v[r] = ld4(P + (int64_t)r * stride, i);
          acc = v[0];
#pragma unroll
          for (int r = 1; r < W; ++r) acc = add4(acc, v[r]);
        } else {
          acc = ld4(P, i);
#pragma unroll 4
          for (int r = 1; r < world; ++r) acc = add4(acc, ld4(P + (int64_t)r * stride, i));
        }
        ((float4*)O)[i] = acc;
      }
    }
  }
  for (int i = 4 * n4 + p; i < cnt; i += THREADS) {   // misaligned pointers or stride: the whole chunk; else the tail n % 4
    float acc = P[i];
    for (int r = 1; r < world; ++r) acc = acc + P[(int64_t)r * stride + i];
    O[i] = acc;
  }
}

int err(const char* fn, const std::string& what) { return bt_set_error_external(BT_ERR_ARG, (std::string(fn) + ": " + what).c_str()); }

// the refusals shared by the device entry point and its twin; nullptr: the call is fine
const char* arg_error(const float* parts, int64_t stride, int world, int64_t n, const float* out) {
  if (world < 1 || world > BT_REDUCE_MAX_WORLD) return "world outside [1, BT_REDUCE_MAX_WORLD]";
  if (n < 0) return "negative element count";
  if (!parts || !out) return "null pointer";
  if (world > 1 && stride < n) return "stride is smaller than n: the parts would overlap";
  if (n > INT64_MAX / 4 / BT_REDUCE_MAX_WORLD || (world > 1 && stride > INT64_MAX / 4 / BT_REDUCE_MAX_WORLD)) return "n or stride is too large";
  if (((uintptr_t)parts | (uintptr_t)out) & 3) return "a pointer is not 4-byte aligned";
  if (out != parts && n > 0) {   // in place over rank 0's part is the one overlap allowed
    const uintptr_t p0 = (uintptr_t)parts, p1 = p0 + 4 * (uintptr_t)((int64_t)(world - 1) * (world > 1 ? stride : 0) + n);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4 * (uintptr_t)n;
    if (o0 < p1 && p0 < o1) return "d_out overlaps the parts (only d_out == d_parts is allowed)";
  }
  return nullptr;
}

}  // namespace

extern "C" {

int bt_grad_rank_sum(void* stream, const float* d_parts, int64_t stride, int world, int64_t n, float* d_out) {
  const char* fn = "bt_grad_rank_sum";
  if (const char* e = arg_error(d_parts, stride, world, n, d_out)) return err(fn, e);
  if (n == 0) return BT_OK;
  const int64_t chunks = (n + CHUNK - 1) / CHUNK;
  if (chunks > 0x7fffffff) return err(fn, "too many chunks for one launch");
  const int wide = (((uintptr_t)d_parts | (uintptr_t)d_out) & 15) == 0 && (world == 1 || (stride & 3) == 0);
  const dim3 grid((unsigned)chunks), block(THREADS);
  hipStream_t s = (hipStream_t)stream;
  switch (world) {
    case 2: hipLaunchKernelGGL(rank_sum_kernel<2>, grid, block, 0, s, d_parts, stride, world, n, d_out, wide); break;
    case 4: hipLaunchKernelGGL(rank_sum_kernel<4>, grid, block, 0, s, d_parts, stride, world, n, d_out, wide); break;
    case 8: hipLaunchKernelGGL(rank_sum_kernel<8>, grid, block, 0, s, d_parts, stride, world, n, d_out, wide); break;
    default: hipLaunchKernelGGL(rank_sum_kernel<0>, grid, block, 0, s, d_parts, stride, world, n, d_out, wide); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_grad_rank_sum_host(const float* parts, int64_t stride, int world, int64_t n, float* out) {
  if (const char* e = arg_error(parts, stride, world, n, out)) return err("bt_grad_rank_sum_host", e);
  for (int64_t i = 0; i < n; ++i) {
    float acc = parts[i];
    for (int r = 1; r < world; ++r) acc = acc + parts[(int64_t)r * stride + i];
    out[i] = acc;
  }
  return BT_OK;
}

}  // extern "C"
