// The optimiser step of the fine-tuning loop: multi-tensor AdamW in one launch and the global gradient norm in two.
// DESIGN.md section 14 has the arithmetic, the layout and what a step moves.
//
// AdamW (torch.optim.AdamW at its defaults), per element and one rounded fp32 operation at a time:
//     g = grad * gs;   p = p * decay;   m = m + (g - m) * (1 - beta1);   v = v * beta2 + (g * g) * (1 - beta2);
//     p = p - step_size * (m / (sqrt(v) / bias2_sqrt + eps))
// The per-group scalars come by value, computed by the caller in fp64 and rounded once.  Gradients, m and v live in three flat
// buffers (tensor i at a multiple of 4 elements, zero padding between tensors that no kernel writes); the parameters stay in
// their nn.Parameter storage.  One 256-thread workgroup takes one chunk of BT_OPTIM_CHUNK elements of one tensor from the chunk
// table: 16 bytes per lane and access where the parameter pointer is 16-byte aligned (the flat buffers always are), one
// element per lane for a parameter that is only 4-byte aligned and for the tail numel % 4.
//
// Gradient norm: launch 1 writes one fp64 sum of squares per slice of BT_OPTIM_NORM_SLICE elements of the flat gradient buffer
// (thread p adds the squares of its float4s k * 256 + p, k ascending, x y z w in turn; then a 256-leaf tree); launch 2, one
// workgroup, adds the slices in index order and writes {norm, coef}.  No atomics, no memsets, no allocation; every sum's order
// depends on the layout alone, so a step is bitwise reproducible.
// Weight averaging: bt_adamw_ema_step is the same pass with a fourth flat buffer.  The thread that has
// computed an element's new p also moves that element's average, e = p on a copying step and e = e + (p - e) * w otherwise;
// bt_ema_exchange swaps p and e over the same chunk table.  adamw_kernel<false> is the plain step, its body as before.
// Host: bt_adamw_step_host / bt_adamw_ema_step_host / bt_grad_norm_host repeat the same operations in the same order.  The
// file is compiled with -ffp-contract=off, with hipcc's correctly rounded fp32 divide and square root and without flushing
// denormals, so the device and the host agree bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/beat_this_amd.h"

#pragma clang fp contract(off)

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

constexpr int CHUNK = BT_OPTIM_CHUNK;
constexpr int SLICE = BT_OPTIM_NORM_SLICE;
constexpr int THREADS = 256;
static_assert(CHUNK % (4 * THREADS) == 0 && SLICE % (4 * THREADS) == 0, "whole float4 rounds per workgroup");

// ---- the arithmetic, the same operations on host and device ------------------------------------------------------------------
__host__ __device__ inline void adamw_one(float& p, float& m, float& v, float grad, float gs, const bt_optim_group& h) {
  const float g = grad * gs;
  p = p * h.decay;
  m = m + (g - m) * h.one_minus_beta1;
  v = v * h.beta2 + (g * g) * h.one_minus_beta2;
  const float denom = sqrtf(v) / h.bias2_sqrt + h.eps;   // eps outside the square root
  p = p - h.step_size * (m / denom);
}

// the running average of an element, after adamw_one has made its new p (torch's get_ema_multi_avg_fn: lerp(e, p, 1 - decay))
__host__ __device__ inline void ema_one(float& e, float p, float w) { e = e + (p - e) * w; }

__host__ __device__ inline void square_into(double& acc, float x) {
  const double d = (double)x;
  acc += d * d;
}

// {norm, coef} from the sum of squares (torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1); a NaN stays)
__host__ __device__ inline void norm_record(double sum, float grad_scale, float max_norm, float* record) {
  const float norm = (float)(sqrt(sum) * (double)fabsf(grad_scale));
  const float c = max_norm / (norm + 1e-6f);
  record[0] = norm;
  record[1] = c > 1.0f ? 1.0f : c;
}

__host__ __device__ inline bool tensor_ok(const bt_optim_tensor& t, int n_groups, int64_t total) {
  return t.numel >= 0 && t.offset >= 0 && (t.offset & 3) == 0 && t.offset <= total && t.numel <= total - t.offset &&
         t.group >= 0 && t.group < n_groups && (t.param != nullptr || t.numel == 0) && ((uintptr_t)t.param & 3) == 0;
}

// ---- device ------------------------------------------------------------------------------------------------------------------
// EMA: the pass also keeps the average of every element it updates (ema, ema_weight, ema_copy); without it they are unused
template <bool EMA>
__global__ __launch_bounds__(THREADS) void adamw_kernel(const bt_optim_tensor* __restrict__ tensors, int n_tensors,
                                                        const bt_optim_chunk* __restrict__ chunks, float* __restrict__ grad,
                                                        float* __restrict__ m, float* __restrict__ v, int64_t total,
                                                        bt_optim_hyper h, const float* __restrict__ coef,
                                                        float* __restrict__ ema, float ema_weight, int ema_copy) {
  const bt_optim_chunk c = chunks[blockIdx.x];
  if (c.tensor < 0 || c.tensor >= n_tensors || c.chunk < 0) return;   // (a damaged table updates nothing, never outside)
  const bt_optim_tensor t = tensors[c.tensor];
  const int64_t begin = (int64_t)c.chunk * CHUNK;
  if (!tensor_ok(t, h.n_groups, total) || begin >= t.numel) return;
  const bt_optim_group hg = h.g[t.group];
  const float gs = coef ? h.grad_scale * coef[0] : h.grad_scale;
  const int n = (int)(t.numel - begin < CHUNK ? t.numel - begin : CHUNK);
  float* P = t.param + begin;
  const int64_t f = t.offset + begin;   // a multiple of 4: the flat buffers are read and written 16 bytes at a time
  float* G = grad + f;
  float* M = m + f;
  float* V = v + f;
  float* E = EMA ? ema + f : nullptr;
  const bool copy = ema_copy != 0;   // (the first averaged step: e = p, the old e is not read)
  const bool zero = h.zero_grads != 0;
  const int p = threadIdx.x;
  const bool wide = ((uintptr_t)t.param & 15) == 0;   // (begin is a multiple of 4: the chunk is aligned like the tensor)
  const int n4 = n >> 2;
  if (wide) {
#pragma unroll
    for (int k = 0; k < CHUNK / (4 * THREADS); ++k) {
      const int i = k * THREADS + p;
      if (i < n4) {
        float4 pp = ((const float4*)P)[i];
        const float4 gg = ((const float4*)G)[i];
        float4 mm = ((const float4*)M)[i], vv = ((const float4*)V)[i];
        float4 ee;
        if (EMA && !copy) ee = ((const float4*)E)[i];
        adamw_one(pp.x, mm.x, vv.x, gg.x, gs, hg);
        adamw_one(pp.y, mm.y, vv.y, gg.y, gs, hg);
        adamw_one(pp.z, mm.z, vv.z, gg.z, gs, hg);
        adamw_one(pp.w, mm.w, vv.w, gg.w, gs, hg);
        ((float4*)P)[i] = pp;
        ((float4*)M)[i] = mm;
        ((float4*)V)[i] = vv;
        if (zero) ((float4*)G)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (EMA) {
          if (copy) {
            ee = pp;
          } else {
            ema_one(ee.x, pp.x, ema_weight);
            ema_one(ee.y, pp.y, ema_weight);
            ema_one(ee.z, pp.z, ema_weight);
            ema_one(ee.w, pp.w, ema_weight);
          }
          ((float4*)E)[i] = ee;
        }
      }
    }
  }
  for (int i = (wide ? 4 * n4 : 0) + p; i < n; i += THREADS) {   // a parameter that is a view at 4-byte alignment; the tail
    float pp = P[i], mm = M[i], vv = V[i];
    adamw_one(pp, mm, vv, G[i], gs, hg);
    P[i] = pp;
    M[i] = mm;
    V[i] = vv;
    if (zero) G[i] = 0.0f;
    if (EMA) {
      float ee = pp;
      if (!copy) {
        ee = E[i];
        ema_one(ee, pp, ema_weight);
      }
      E[i] = ee;
    }
  }
}

// p <-> e over the chunk table of the step: a pure move, the same three access paths.  The group of a tensor plays no part
// here, so its index is only held to the ABI's range (BT_OPTIM_MAX_GROUPS), not to a step's n_groups.
__global__ __launch_bounds__(THREADS) void ema_exchange_kernel(const bt_optim_tensor* __restrict__ tensors, int n_tensors,
                                                               const bt_optim_chunk* __restrict__ chunks, float* __restrict__ ema,
                                                               int64_t total) {
  const bt_optim_chunk c = chunks[blockIdx.x];
  if (c.tensor < 0 || c.tensor >= n_tensors || c.chunk < 0) return;
  const bt_optim_tensor t = tensors[c.tensor];
  const int64_t begin = (int64_t)c.chunk * CHUNK;
  if (!tensor_ok(t, BT_OPTIM_MAX_GROUPS, total) || begin >= t.numel) return;
  const int n = (int)(t.numel - begin < CHUNK ? t.numel - begin : CHUNK);
  float* P = t.param + begin;
  float* E = ema + t.offset + begin;
  const int p = threadIdx.x;
  const bool wide = ((uintptr_t)t.param & 15) == 0;
  const int n4 = n >> 2;
  if (wide) {
#pragma unroll
    for (int k = 0; k < CHUNK / (4 * THREADS); ++k) {
      const int i = k * THREADS + p;
      if (i < n4) {
        const float4 pp = ((const float4*)P)[i], ee = ((const float4*)E)[i];
        ((float4*)P)[i] = ee;
        ((float4*)E)[i] = pp;
      }
    }
  }
  for (int i = (wide ? 4 * n4 : 0) + p; i < n; i += THREADS) {
    const float pp = P[i], ee = E[i];
    P[i] = ee;
    E[i] = pp;
  }
}

__global__ __launch_bounds__(THREADS) void norm_slice_kernel(const float* __restrict__ grad, int64_t total, double* __restrict__ ws) {
  __shared__ double red[THREADS];
  const int p = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * SLICE;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < SLICE / (4 * THREADS); ++k) {
    const int64_t e = base + 4 * (int64_t)(k * THREADS + p);
    if (e < total) {   // (total is a multiple of 4: a float4 is inside or outside as a whole)
      const float4 g = *(const float4*)(grad + e);
      square_into(acc, g.x);
      square_into(acc, g.y);
      square_into(acc, g.z);
      square_into(acc, g.w);
    }
  }
  red[p] = acc;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (p < s) red[p] += red[p + s];
    __syncthreads();
  }
  if (p == 0) ws[blockIdx.x] = red[0];
}

// one workgroup: the slices' sums in index order (batches of 256 staged in LDS, the next batch loaded while thread 0 adds)
__global__ __launch_bounds__(THREADS) void norm_finish_kernel(const double* __restrict__ ws, int64_t n_slices, float grad_scale,
                                                              float max_norm, float* __restrict__ record) {
  __shared__ double buf[THREADS];
  const int p = threadIdx.x;
  double acc = 0.0;
  double next = p < n_slices ? ws[p] : 0.0;
  for (int64_t b = 0; b < n_slices; b += THREADS) {
    buf[p] = next;
    __syncthreads();
    const int64_t i = b + THREADS + p;
    next = i < n_slices ? ws[i] : 0.0;
    if (p == 0) {
      const int cnt = (int)(n_slices - b < THREADS ? n_slices - b : THREADS);
      for (int j = 0; j < cnt; ++j) acc += buf[j];
    }
    __syncthreads();
  }
  if (p == 0) norm_record(acc, grad_scale, max_norm, record);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int err(const char* fn, const std::string& what) { return bt_set_error_external(BT_ERR_ARG, (std::string(fn) + ": " + what).c_str()); }

const char* hyper_error(const bt_optim_hyper* h) {
  if (!h) return "null hyper-parameters";
  if (h->n_groups < 1 || h->n_groups > BT_OPTIM_MAX_GROUPS) return "n_groups outside [1, BT_OPTIM_MAX_GROUPS]";
  return nullptr;
}

int64_t slices_of(int64_t total) { return (total + SLICE - 1) / SLICE; }

double slice_sum_host(const float* grad, int64_t base, int64_t total) {
  double red[THREADS];
  for (int p = 0; p < THREADS; ++p) {
    double acc = 0.0;
    for (int k = 0; k < SLICE / (4 * THREADS); ++k) {
      const int64_t e = base + 4 * (int64_t)(k * THREADS + p);
      if (e < total)
        for (int j = 0; j < 4; ++j) square_into(acc, grad[e + j]);
    }
    red[p] = acc;
  }
  for (int s = THREADS / 2; s > 0; s >>= 1)
    for (int p = 0; p < s; ++p) red[p] += red[p + s];
  return red[0];
}

const char* WEIGHT_ERROR = "ema_weight = 1 - decay must be a number in (0, 1]";
bool weight_ok(float w) { return w > 0.0f && w <= 1.0f; }   // (a NaN fails both comparisons)

// bt_adamw_step and bt_adamw_ema_step: the refusals, then one launch
int adamw_launch(const char* fn, bool with_ema, void* stream, const bt_optim_tensor* d_tensors, int n_tensors,
                 const bt_optim_chunk* d_chunks, int64_t n_chunks, float* d_grad, float* d_m, float* d_v, float* d_ema, int64_t total,
                 const bt_optim_hyper* hyper, const float* d_coef, float ema_weight, int ema_copy) {
  if (const char* e = hyper_error(hyper)) return err(fn, e);
  if (with_ema && !weight_ok(ema_weight)) return err(fn, WEIGHT_ERROR);
  if (n_tensors < 0 || n_chunks < 0 || n_chunks > 0x7fffffff || total < 0 || (total & 3))
    return err(fn, "negative count, or a flat length that is no multiple of 4");
  if (n_chunks == 0) return BT_OK;
  if (!d_tensors || !d_chunks || !d_grad || !d_m || !d_v || (with_ema && !d_ema)) return err(fn, "null pointer");
  if (((uintptr_t)d_grad | (uintptr_t)d_m | (uintptr_t)d_v | (uintptr_t)d_ema) & 15) return err(fn, "a flat buffer is not 16-byte aligned");
  if ((uintptr_t)d_coef & 3) return err(fn, "the coefficient pointer is not 4-byte aligned");
  const dim3 grid((unsigned)n_chunks), block(THREADS);
  if (with_ema)
    hipLaunchKernelGGL(adamw_kernel<true>, grid, block, 0, (hipStream_t)stream, d_tensors, n_tensors, d_chunks, d_grad, d_m, d_v, total,
                       *hyper, d_coef, d_ema, ema_weight, ema_copy);
  else
    hipLaunchKernelGGL(adamw_kernel<false>, grid, block, 0, (hipStream_t)stream, d_tensors, n_tensors, d_chunks, d_grad, d_m, d_v, total,
                       *hyper, d_coef, (float*)nullptr, 0.0f, 0);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
  return BT_OK;
}

// the host twins: the tables are validated entry by entry, then the chunks in table order
int adamw_host(const char* fn, bool with_ema, const bt_optim_tensor* tensors, int n_tensors, const bt_optim_chunk* chunks,
               int64_t n_chunks, float* grad, float* m, float* v, float* ema, int64_t total, const bt_optim_hyper* hyper,
               const float* coef, float ema_weight, int ema_copy) {
  if (const char* e = hyper_error(hyper)) return err(fn, e);
  if (with_ema && !weight_ok(ema_weight)) return err(fn, WEIGHT_ERROR);
  if (n_tensors < 0 || n_chunks < 0 || total < 0 || (total & 3)) return err(fn, "negative count, or a flat length that is no multiple of 4");
  if (n_chunks == 0) return BT_OK;
  if (!tensors || !chunks || !grad || !m || !v || (with_ema && !ema)) return err(fn, "null pointer");
  if (((uintptr_t)grad | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) return err(fn, "a flat buffer is not 16-byte aligned");
  for (int i = 0; i < n_tensors; ++i)
    if (!tensor_ok(tensors[i], hyper->n_groups, total))
      return err(fn, "tensor " + std::to_string(i) + ": numel < 0, a null or misaligned pointer, a group index out of range or a "
                     "range outside the flat buffers");
  for (int64_t c = 0; c < n_chunks; ++c)
    if (chunks[c].tensor < 0 || chunks[c].tensor >= n_tensors || chunks[c].chunk < 0 ||
        (int64_t)chunks[c].chunk * CHUNK >= tensors[chunks[c].tensor].numel)
      return err(fn, "chunk " + std::to_string(c) + " points outside its tensor");
  const float gs = coef ? hyper->grad_scale * coef[0] : hyper->grad_scale;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const bt_optim_tensor& t = tensors[chunks[c].tensor];
    const bt_optim_group& hg = hyper->g[t.group];
    const int64_t begin = (int64_t)chunks[c].chunk * CHUNK;
    const int64_t n = t.numel - begin < CHUNK ? t.numel - begin : CHUNK;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t f = t.offset + begin + i;
      adamw_one(t.param[begin + i], m[f], v[f], grad[f], gs, hg);
      if (hyper->zero_grads) grad[f] = 0.0f;
      if (with_ema) {
        if (ema_copy)
          ema[f] = t.param[begin + i];
        else
          ema_one(ema[f], t.param[begin + i], ema_weight);
      }
    }
  }
  return BT_OK;
}

}  // namespace

extern "C" {

void bt_optim_struct_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(bt_optim_tensor);
  out[1] = (int32_t)sizeof(bt_optim_chunk);
  out[2] = (int32_t)sizeof(bt_optim_group);
  out[3] = (int32_t)sizeof(bt_optim_hyper);
  out[4] = (int32_t)offsetof(bt_optim_tensor, offset);
  out[5] = (int32_t)offsetof(bt_optim_tensor, group);
  out[6] = (int32_t)offsetof(bt_optim_hyper, g);
  out[7] = BT_OPTIM_CHUNK;
  out[8] = BT_OPTIM_NORM_SLICE;
  out[9] = BT_OPTIM_MAX_GROUPS;
}

int bt_optim_plan(int n_tensors, const void* const* params, const int64_t* numel, const int32_t* groups, int n_groups,
                  bt_optim_tensor* tensors, int64_t* total, bt_optim_chunk* chunks, int64_t chunk_capacity, int64_t* n_chunks) {
  const char* fn = "bt_optim_plan";
  if (n_tensors < 0 || (n_tensors > 0 && (!params || !numel || !groups || !tensors)) || !total || !n_chunks)
    return err(fn, "null pointer or negative tensor count");
  if (n_groups < 1 || n_groups > BT_OPTIM_MAX_GROUPS) return err(fn, "n_groups outside [1, BT_OPTIM_MAX_GROUPS]");
  if (chunks && chunk_capacity < 0) return err(fn, "negative chunk capacity");
  int64_t off = 0, nc = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (numel[i] < 0) return err(fn, "tensor " + std::to_string(i) + " has numel < 0");
    if (groups[i] < 0 || groups[i] >= n_groups)
      return err(fn, "tensor " + std::to_string(i) + " has group index " + std::to_string(groups[i]) + " of " + std::to_string(n_groups));
    if (!params[i] && numel[i] > 0) return err(fn, "tensor " + std::to_string(i) + " has a null parameter pointer");
    if ((uintptr_t)params[i] & 3) return err(fn, "tensor " + std::to_string(i) + ": parameter pointer is not 4-byte aligned");
    const int64_t c = (numel[i] + CHUNK - 1) / CHUNK;
    if (numel[i] > (int64_t)0x7fffffff * CHUNK || off > INT64_MAX / 2 - numel[i] || nc + c > 0x7fffffff)
      return err(fn, "the tensors are too large for one launch");
    tensors[i].param = (float*)params[i];
    tensors[i].offset = off;
    tensors[i].numel = numel[i];
    tensors[i].group = groups[i];
    tensors[i].reserved = 0;
    if (chunks) {
      if (nc + c > chunk_capacity) return err(fn, "chunk table too small");
      for (int64_t k = 0; k < c; ++k) chunks[nc + k] = bt_optim_chunk{i, (int32_t)k};
    }
    nc += c;
    off += (numel[i] + 3) / 4 * 4;
  }
  *total = off;
  *n_chunks = nc;
  return BT_OK;
}

size_t bt_grad_norm_workspace_bytes(int64_t total) {
  if (total < 0) return 0;
  const int64_t n = slices_of(total);
  return (size_t)(n > 0 ? n : 1) * sizeof(double);
}

int bt_grad_norm(void* stream, const float* d_grad, int64_t total, float grad_scale, float max_norm, void* d_ws, size_t ws_bytes,
                 float* d_record) {
  const char* fn = "bt_grad_norm";
  if (!d_grad || !d_ws || !d_record) return err(fn, "null pointer");
  if (total < 0 || (total & 3)) return err(fn, "the flat buffer's length must be a non-negative multiple of 4");
  if ((uintptr_t)d_grad & 15) return err(fn, "the flat gradient buffer is not 16-byte aligned");
  if ((uintptr_t)d_ws & 7) return err(fn, "the workspace is not 8-byte aligned");
  const int64_t n = slices_of(total);
  if (n > 0x7fffffff) return err(fn, "too many slices");
  if (ws_bytes < bt_grad_norm_workspace_bytes(total)) return err(fn, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) hipLaunchKernelGGL(norm_slice_kernel, dim3((unsigned)n), dim3(THREADS), 0, s, d_grad, total, (double*)d_ws);
  hipLaunchKernelGGL(norm_finish_kernel, dim3(1), dim3(THREADS), 0, s, (const double*)d_ws, n, grad_scale, max_norm, d_record);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_adamw_step(void* stream, const bt_optim_tensor* d_tensors, int n_tensors, const bt_optim_chunk* d_chunks, int64_t n_chunks,
                  float* d_grad, float* d_m, float* d_v, int64_t total, const bt_optim_hyper* hyper, const float* d_coef) {
  return adamw_launch("bt_adamw_step", false, stream, d_tensors, n_tensors, d_chunks, n_chunks, d_grad, d_m, d_v, nullptr, total, hyper,
                      d_coef, 0.0f, 0);
}

int bt_adamw_ema_step(void* stream, const bt_optim_tensor* d_tensors, int n_tensors, const bt_optim_chunk* d_chunks, int64_t n_chunks,
                      float* d_grad, float* d_m, float* d_v, float* d_ema, int64_t total, const bt_optim_hyper* hyper,
                      const float* d_coef, float ema_weight, int ema_copy) {
  return adamw_launch("bt_adamw_ema_step", true, stream, d_tensors, n_tensors, d_chunks, n_chunks, d_grad, d_m, d_v, d_ema, total, hyper,
                      d_coef, ema_weight, ema_copy);
}

int bt_ema_exchange(void* stream, const bt_optim_tensor* d_tensors, int n_tensors, const bt_optim_chunk* d_chunks, int64_t n_chunks,
                    float* d_ema, int64_t total) {
  const char* fn = "bt_ema_exchange";
  if (n_tensors < 0 || n_chunks < 0 || n_chunks > 0x7fffffff || total < 0 || (total & 3))
    return err(fn, "negative count, or a flat length that is no multiple of 4");
  if (n_chunks == 0) return BT_OK;
  if (!d_tensors || !d_chunks || !d_ema) return err(fn, "null pointer");
  if ((uintptr_t)d_ema & 15) return err(fn, "the flat buffer of the averages is not 16-byte aligned");
  hipLaunchKernelGGL(ema_exchange_kernel, dim3((unsigned)n_chunks), dim3(THREADS), 0, (hipStream_t)stream, d_tensors, n_tensors,
                     d_chunks, d_ema, total);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string(fn) + ": " + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_grad_norm_host(const float* grad, int64_t total, float grad_scale, float max_norm, float* record) {
  const char* fn = "bt_grad_norm_host";
  if (!grad || !record) return err(fn, "null pointer");
  if (total < 0 || (total & 3)) return err(fn, "the flat buffer's length must be a non-negative multiple of 4");
  double acc = 0.0;
  for (int64_t s = 0; s < slices_of(total); ++s) acc += slice_sum_host(grad, s * SLICE, total);
  norm_record(acc, grad_scale, max_norm, record);
  return BT_OK;
}

int bt_adamw_step_host(const bt_optim_tensor* tensors, int n_tensors, const bt_optim_chunk* chunks, int64_t n_chunks, float* grad,
                       float* m, float* v, int64_t total, const bt_optim_hyper* hyper, const float* coef) {
  return adamw_host("bt_adamw_step_host", false, tensors, n_tensors, chunks, n_chunks, grad, m, v, nullptr, total, hyper, coef, 0.0f, 0);
}

int bt_adamw_ema_step_host(const bt_optim_tensor* tensors, int n_tensors, const bt_optim_chunk* chunks, int64_t n_chunks, float* grad,
                           float* m, float* v, float* ema, int64_t total, const bt_optim_hyper* hyper, const float* coef,
                           float ema_weight, int ema_copy) {
  return adamw_host("bt_adamw_ema_step_host", true, tensors, n_tensors, chunks, n_chunks, grad, m, v, ema, total, hyper, coef, ema_weight,
                    ema_copy);
}

}  // extern "C"
